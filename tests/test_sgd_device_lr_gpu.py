"""A replayed training step that follows a learning-rate schedule: FlatSGD(device_lr=True) keeps the rate in one fp32 element on the
device, `cot_sgd_step_lr`'s kernel reads it when it runs, so ONE capture serves every rate -- against eager steps through the by-value
`cot_sgd_step` with the same set_lr calls, BIT FOR BIT (torch.equal everywhere: same expression, same fp32 rate).

The harness is tests/test_graph_replay_gpu.py's (twins on static buffers, one non-default stream, all batches different)."""
import pytest
import torch

from cotnet_amd import _lib, cot_layer_fused as clf
from cotnet_amd.cotnet import Bottleneck
from cotnet_amd.lr_schedule import CosineSchedule
from tests import sgd_lr_cases as cases, truth
from tests.test_graph_replay_gpu import (CM, NCHW, _Twin, _batches, _capture, _model, _opening, _replay, _same, _stage, _stream, mse,
                                         xent)

pytestmark = pytest.mark.gpu
DEV = "cuda"
WARM = 2
# 2048 blocks x 256 lanes x V = 4 is one round of the grid-stride loop: block 0 runs a second round and the tail still exists
SECOND_ROUND = 2048 * 256 * 4 + 5


@pytest.mark.parametrize("pdt,gdt", cases.DTYPE_PAIRS, ids=cases.PAIR_IDS)
@pytest.mark.parametrize("nesterov", [0, 1])
def test_rate_from_memory_equals_rate_by_value_on_the_device(pdt, gdt, nesterov):
    cases.compare_entry_points(_lib.lib(), torch.device(DEV), _lib.stream(), pdt, gdt, nesterov, cases.SIZES + [SECOND_ROUND],
                               sync=torch.cuda.synchronize)


def _eager(tw, batches, sched):
    losses = []
    for i, b in enumerate(batches):
        tw.opt.set_lr(sched.value(i))
        tw.load(b)
        losses.append(tw.step().clone())
    return losses


def _replayed(tw, batches, sched, s, follow=True):
    """WARM eager steps, ONE capture, a replay per batch but the last -- each behind a set_lr on the replay stream (follow=False: the
    control that leaves the rate where the capture found it) --, and the eager hand-back at yet another rate"""
    losses = []
    for i, b in enumerate(batches[:WARM]):
        tw.opt.set_lr(sched.value(i))
        tw.load(b)
        losses.append(tw.step().clone())
    g, out = _capture(tw, s)
    assert tw.opt._captured_lr is None  # nothing baked
    for i, b in enumerate(batches[WARM:-1], start=WARM):
        if follow:
            tw.opt.set_lr(sched.value(i))
        losses.append(_replay(tw, g, out, b))
    if follow:
        tw.opt.set_lr(sched.value(len(batches) - 1))
    tw.load(batches[-1])
    losses.append(tw.step().clone())
    return losses, g


def schedule_vs_replay(make_model, batches, loss_fn, sw, nodes, sched, control=False, **opt_kw):
    rates = [sched.value(i) for i in range(len(batches))]
    assert len(set(rates)) == len(rates)  # every step at another rate
    _lib.FALLBACKS.clear()
    s = _stream()
    with truth.switches(**sw), torch.cuda.stream(s):
        model = make_model()
        if isinstance(model, torch.nn.Sequential):
            clf.plan_stage_layouts(model)
        e = _Twin(model, loss_fn, batches[0], rates[0], **opt_kw)
        r = _Twin(model, loss_fn, batches[0], rates[0], device_lr=True, **opt_kw)
        le = _eager(e, batches, sched)
        lr_, graph = _replayed(r, batches, sched, s)
        torch.cuda.synchronize()
        assert torch.equal(torch.stack(le), torch.stack(lr_)), f"loss per step, eager {torch.stack(le).tolist()} vs replay {torch.stack(lr_).tolist()}"
        _same(e.state(), r.state(), "after the hand-back, eager by value vs replay with the rate on the device")
        assert len({float(v) for v in le}) == len(batches) and all(torch.isfinite(v) for v in le)
        assert r.opt.lr == e.opt.lr == rates[-1] and r.opt.lr_dev.item() == torch.tensor(rates[-1], dtype=torch.float32).item()
        assert r.names and all(n.startswith(nodes) for n in e.names + r.names), sorted(set(e.names + r.names))
        assert not _lib.FALLBACKS, dict(_lib.FALLBACKS)
        if control:  # a rate that never reached the kernel must show: the same replays without the set_lr calls differ from eager
            c = _Twin(model, loss_fn, batches[0], rates[0], device_lr=True, **opt_kw)
            lc, gc = _replayed(c, batches, sched, s, follow=False)
            torch.cuda.synchronize()
            assert not torch.equal(torch.stack(le), torch.stack(lc))
            assert any(not torch.equal(v, c.state()[k]) for k, v in e.state().items() if k.startswith("param"))
            del gc
        del graph
    torch.cuda.current_stream().wait_stream(s)
    return e, r


def test_replays_follow_the_schedule_on_an_nchw_stage():
    """the smallest real stage of the replay tests: two warm-up steps, one capture, four replays and the hand-back at seven rates"""
    make = _stage(9, _opening(), lambda: Bottleneck(256, 64))
    sched = CosineSchedule(0.05, 7, warmup_t=2, warmup_lr_init=5e-4, lr_min=1e-5)
    schedule_vs_replay(make, _batches((8, 128, 28, 28), (8, 256, 14, 14), 101, n=WARM + 4 + 1), mse, NCHW, "_BottleneckNode", sched,
                       control=True)


def test_replays_follow_the_schedule_with_weight_averaging_on_a_channel_major_stage():
    """the EMA kernels run behind the SGD kernels in the same graph: their buckets and the averaged buffers are in the compared state"""
    make = _stage(135, *[lambda: Bottleneck(512, 128)] * 2)
    sched = CosineSchedule(0.05, 7, warmup_t=2, warmup_lr_init=5e-4, lr_min=1e-5)
    shape = (8, 512, 7, 7)
    e, r = schedule_vs_replay(make, _batches(shape, shape, 102, n=WARM + 4 + 1), mse, CM, "_BottleneckCMNode", sched, ema_decay=0.9999)
    assert any(k.endswith("[ema]") for k in r.state()) and any(k.startswith("opt._buf_ema") for k in r.state())


def test_whole_model_replays_at_three_rates():
    """cotnet50 at B = 2, 224 x 224, cross-entropy: one capture, three replays at three rates, the hand-back"""
    sched = CosineSchedule(0.03, 6, warmup_t=2, warmup_lr_init=3e-4, lr_min=1e-5)
    schedule_vs_replay(_model("cotnet50"), _batches((2, 3, 224, 224), (2,), 103, classes=1000, n=WARM + 3 + 1), xent, truth.SINGLE_NODE,
                       ("_BottleneckNode", "_BottleneckCMNode"), sched)
