"""Gradient clipping by global norm and the non-finite guard on the device: tests/grad_clip_cases.py's kernel cases through the real
library, and FlatSGD(clip_grad=...) replayed from ONE HIP-graph capture over clipped, unclipped and non-finite batches against the same
sequence issued eagerly, BIT FOR BIT (tests/test_graph_replay_gpu.py's harness: twins on static buffers, one non-default stream).

An `inf` in a batch makes backward produce NaN gradients; that is ordinary arithmetic, and the step that follows writes no weight."""
import pytest
import torch

from cotnet_amd import _lib, cot_layer_fused as clf
from cotnet_amd.cotnet import Bottleneck
from cotnet_amd.lr_schedule import CosineSchedule
from tests import grad_clip_cases as cases
from tests import sgd_lr_cases as sgd
from tests import truth
from tests.test_graph_replay_gpu import NCHW, _Twin, _batches, _capture, _opening, _replay, _same, _stage, _stream, mse

pytestmark = pytest.mark.gpu
DEV = "cuda"
WARM = 2
SECOND_ROUND = 2048 * 256 * 4 + 5  # the SGD kernel's grid-stride loop enters a second round (tests/test_sgd_device_lr_gpu.py)


def _L():
    return _lib.lib()


def _run(check, *a):
    check(_L(), torch.device(DEV), _lib.stream(), *a, sync=torch.cuda.synchronize)


@pytest.mark.parametrize("gdt", cases.GRAD_DTYPES, ids=cases.GRAD_IDS)
def test_norm_coefficient_and_determinism(gdt):
    for n in cases.sizes(_L().cot_grad_norm_parts(), cases.vec(gdt)):
        _run(cases.check_norm, gdt, n)


@pytest.mark.parametrize("gdt", cases.GRAD_DTYPES, ids=cases.GRAD_IDS)
def test_zero_gradient(gdt):
    _run(cases.check_zero_gradient, gdt)


@pytest.mark.parametrize("kind,gdt", [(k, dt) for k in cases.NONFINITE for dt in cases.GRAD_DTYPES
                                      if k != "bf16-overflowing-squares" or dt == torch.bfloat16],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_non_finite_gradients_skip(kind, gdt):
    _run(cases.check_nonfinite, kind, gdt)


def test_several_buckets_share_one_norm():
    _run(cases.check_several_buckets)


def test_counters_over_a_scripted_sequence():
    _run(cases.check_counters)


@pytest.mark.parametrize("pdt,gdt", sgd.DTYPE_PAIRS, ids=sgd.PAIR_IDS)
@pytest.mark.parametrize("nesterov", [0, 1])
def test_sgd_behind_the_block_equals_todays_entry_points(pdt, gdt, nesterov):
    _run(cases.check_sgd_clip, pdt, gdt, nesterov, sgd.SIZES + [SECOND_ROUND])


def test_the_reference_fixture():
    _run(cases.check_fixture)


def test_refusals_leave_everything_alone():
    _run(cases.check_refusals)


# ---- one capture serves clipped, unclipped and skipped steps

BAD = WARM + 2  # the batch with an inf in its input: a replayed one, with replays on both sides


def _block_words(tw):
    return tw.opt.clip_state.clone()


def _weights(tw):
    return {k: v.clone() for k, v in tw.state().items() if k.startswith("param") or k.endswith(("[master]", "[mom]"))}


def _same_bits(a, b, what):
    """_same for states that may hold NaN (the BatchNorm running statistics behind the non-finite batch): compared as integers"""
    assert a.keys() == b.keys()
    bad = [k for k in a if not (sgd.same_bits(a[k], b[k]) if a[k].is_floating_point() else torch.equal(a[k], b[k]))]
    assert not bad, f"{what}: {len(bad)} of {len(a)} tensors differ, first {bad[:4]}"


def _eager(tw, batches, sched):
    losses, stats, blocks = [], [], []
    for i, b in enumerate(batches):
        if sched is not None:
            tw.opt.set_lr(sched.value(i))
        tw.load(b)
        losses.append(tw.step().clone())
        blocks.append(_block_words(tw))
        stats.append(tw.opt.clip_stats())
    return losses, stats, blocks


def _replayed(tw, batches, sched, s):
    """WARM eager steps, ONE capture, a replay per remaining batch"""
    losses, stats, blocks = [], [], []
    for i, b in enumerate(batches[:WARM]):
        if sched is not None:
            tw.opt.set_lr(sched.value(i))
        tw.load(b)
        losses.append(tw.step().clone())
        blocks.append(_block_words(tw))
        stats.append(tw.opt.clip_stats())
    g, out = _capture(tw, s)
    assert tw.opt._captured_lr == (None if sched is not None else tw.opt.lr)
    for i, b in enumerate(batches[WARM:], start=WARM):
        if sched is not None:
            tw.opt.set_lr(sched.value(i))
        before = _weights(tw) if i == BAD else None
        losses.append(_replay(tw, g, out, b))
        blocks.append(_block_words(tw))
        stats.append(tw.opt.clip_stats())
        if i == BAD:  # across the non-finite replay the weights keep their bits
            after_bad = _weights(tw)
            _same(before, after_bad, "parameters, masters and momentum across the non-finite replay")
            assert stats[-1]["skip"] == 1 and stats[-1]["skipped"] == 1 and stats[-1]["scale"] == 0.0, stats[-1]
        if i == BAD + 1:  # the next replay trains again
            assert stats[-1]["skip"] == 0 and stats[-1]["skipped"] == 1, stats[-1]
            assert any(not torch.equal(v, after_bad[k]) for k, v in _weights(tw).items() if k.endswith("[master]"))
    return losses, stats, blocks, g


def clip_vs_replay(sched=None, **opt_kw):
    n = WARM + 5
    batches = _batches((8, 128, 28, 28), (8, 256, 14, 14), 111, n=n)
    x_bad = batches[BAD][0].clone()
    x_bad[3, 17, 5, 9] = float("inf")
    batches[BAD] = (x_bad, batches[BAD][1])
    _lib.FALLBACKS.clear()
    s = _stream()
    with truth.switches(**NCHW), torch.cuda.stream(s):
        model = _stage(9, _opening(), lambda: Bottleneck(256, 64))()
        clf.plan_stage_layouts(model)
        lr0 = sched.value(0) if sched is not None else 0.05
        # place clip_grad among the gradient norms this stage really produces: a probe twin with the guard alone records them
        probe = _Twin(model, mse, batches[0], lr0, skip_nonfinite=True, **opt_kw)
        _, pstats, _ = _eager(probe, batches, sched)
        norms = sorted(st["total_norm"] for st in pstats if st["skip"] == 0)
        assert len(norms) == n - 1 and pstats[BAD]["skip"] == 1, pstats
        clip = float(norms[len(norms) // 2] * 0.999)  # about half of the finite steps clip
        e = _Twin(model, mse, batches[0], lr0, clip_grad=clip, **opt_kw)
        r = _Twin(model, mse, batches[0], lr0, clip_grad=clip, **opt_kw)
        le, se, be = _eager(e, batches, sched)
        lr_, sr, br, graph = _replayed(r, batches, sched, s)
        torch.cuda.synchronize()
        # (the loss of the non-finite batch may itself be finite -- a ReLU formed with fmaxf drops a NaN -- or not: bits either way)
        assert sgd.same_bits(torch.stack(le), torch.stack(lr_)), f"loss per step, eager {torch.stack(le).tolist()} vs replay {torch.stack(lr_).tolist()}"
        assert len({float(v) for i, v in enumerate(le) if i != BAD}) == n - 1  # (the steps do differ)
        assert all(torch.equal(u, v) for u, v in zip(be, br)), "the clip block differs between eager and replay"
        _same_bits(e.state(), r.state(), "after the last step, eager vs replay with clipping")
        last = sr[-1]
        assert last == se[-1] and last["steps"] == n and last["skipped"] == 1, last
        assert 0 < last["clipped"] < n - 1, f"clip_grad = {clip} did not separate the steps: {[st['total_norm'] for st in sr]}"
        clipped_in_replays = sr[-1]["clipped"] - sr[WARM - 1]["clipped"]
        assert 0 < clipped_in_replays < n - WARM - 1, [st["scale"] for st in sr]  # clipped AND unclipped steps among the replays
        assert all(bool(torch.isfinite(v).all()) for v in _weights(r).values())
        assert not _lib.FALLBACKS, dict(_lib.FALLBACKS)
        del graph
    torch.cuda.current_stream().wait_stream(s)


def test_one_capture_serves_clipped_unclipped_and_skipped_steps():
    clip_vs_replay()


def test_the_same_with_the_rate_on_the_device_under_a_schedule():
    clip_vs_replay(sched=CosineSchedule(0.05, WARM + 5, warmup_t=2, warmup_lr_init=5e-4, lr_min=1e-5), device_lr=True)
