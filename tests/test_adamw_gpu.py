"""Fused Adam / AdamW (cot_adam_tick, cot_adamw_step, FlatAdamW, FlatAdam) -- on the device.

The kernel cases are tests/adamw_cases.py's, the list tests/test_adamw_emulated.py runs on the host emulator, plus the size at which a
lane makes a second trip of the grid-stride loop.  Then FlatAdamW: against torch.optim.AdamW and Adam, save and resume, and ONE HIP-graph capture of forward, backward and step replayed against eager steps, BIT FOR BIT -- built like
tests/test_graph_replay_gpu.py: twins on static buffers, one non-default stream, all batches different.

The device's pow may be one double ulp off Python's; where a correction of the tick is compared with the Python value, one fp32 ulp is
allowed (adamw_cases.check_tick says why).  Everything between two runs on the device is compared bit for bit.

Against torch, on tests/test_flat_sgd_gpu.py's small net, the criterion is a bound.  Where two RUNS are compared bit for bit (replay, save
and resume) the model is tests/checkpoint_cases.py's matrix-and-BatchNorm model: the fp32 backward of the net's torch convolutions is
not reproducible on this device (adamw_cases.small says what was measured), which is no property of the optimizer."""
import pytest
import torch

from cotnet_amd import _lib, cot_layer_fused as clf
from tests import adamw_cases as cases
from tests import sgd_lr_cases as sgd
from tests.test_graph_replay_gpu import _stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
FORMS, FORM_IDS = [False, True], ["fp32", "mixed-bf16"]
WARM, K = 2, 5


def _dev():
    return _lib.lib(), torch.device(DEV), _lib.stream(), torch.cuda.synchronize


@pytest.mark.parametrize("pdt,gdt", sgd.DTYPE_PAIRS, ids=sgd.PAIR_IDS)
@pytest.mark.parametrize("decoupled", [0, 1])
@pytest.mark.parametrize("n", cases.SIZES + [cases.SECOND_TRIP])
def test_one_step_against_the_formula(pdt, gdt, decoupled, n):
    L, dev, stream, sync = _dev()
    cases.check_step(L, dev, stream, pdt, gdt, decoupled, n, sync)


@pytest.mark.parametrize("t", [1, 2, 3, 1000])
def test_the_reference_fixture(t):
    L, dev, stream, sync = _dev()
    cases.check_fixture_step(L, dev, stream, t, sync)


def test_l2_form_against_torch_adam():
    L, dev, stream, sync = _dev()
    cases.check_l2_against_torch_adam(L, dev, stream, sync)


def test_tick():
    L, dev, stream, sync = _dev()
    cases.check_tick(L, dev, stream, sync)


def test_tick_behind_a_skip():
    L, dev, stream, sync = _dev()
    cases.check_tick_skip(L, dev, stream, sync)


@pytest.mark.parametrize("pdt,gdt", sgd.DTYPE_PAIRS, ids=sgd.PAIR_IDS)
def test_zero_gradient(pdt, gdt):
    L, dev, stream, sync = _dev()
    cases.check_zero_gradient(L, dev, stream, pdt, gdt, sync)


@pytest.mark.parametrize("pdt,gdt", sgd.DTYPE_PAIRS, ids=sgd.PAIR_IDS)
def test_rate_by_value_and_from_memory_give_equal_bits(pdt, gdt):
    L, dev, stream, sync = _dev()
    cases.check_rate_sources(L, dev, stream, pdt, gdt, sync)


@pytest.mark.parametrize("pdt,gdt", sgd.DTYPE_PAIRS, ids=sgd.PAIR_IDS)
def test_clip_block(pdt, gdt):
    L, dev, stream, sync = _dev()
    cases.check_clip_block(L, dev, stream, pdt, gdt, sync)


@pytest.mark.parametrize("pdt,gdt", sgd.DTYPE_PAIRS, ids=sgd.PAIR_IDS)
def test_two_calls_give_equal_bits(pdt, gdt):
    L, dev, stream, sync = _dev()
    cases.check_repeatable(L, dev, stream, pdt, gdt, sync)


def test_refusals_leave_everything_alone():
    L, dev, stream, sync = _dev()
    cases.check_refusals(L, dev, stream, sync)


# ---- FlatAdamW, eager

@pytest.mark.parametrize("mixed", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("decoupled", [True, False], ids=["adamw", "adam"])
def test_flat_optimizer_follows_torch(mixed, decoupled):
    cases.check_flat_against_torch(torch.device(DEV), mixed, decoupled)


@pytest.mark.parametrize("mixed", FORMS, ids=FORM_IDS)
def test_checkpoint_resumes_bit_equal(mixed):
    cases.check_checkpoint(torch.device(DEV), mixed)


@pytest.mark.parametrize("mixed", FORMS, ids=FORM_IDS)
def test_state_dict_goes_to_torch_adamw_and_back(mixed):
    cases.check_torch_interop(torch.device(DEV), mixed)


def test_checkpoint_saver_round_trip(tmp_path):
    cases.check_saver_round_trip(torch.device(DEV), True, tmp_path)


def test_a_non_finite_step_is_skipped_and_not_counted():
    cases.check_skipped_step(torch.device(DEV), True)


# ---- FlatAdamW, one capture replayed

class _Twin:
    """a model and its FlatAdamW reading input and target from static buffers.  `plant`: between backward and step, the one-element
    `poison` buffer is added to one element of the last gradient bucket -- 0 leaves the gradient as it is, inf makes the step one to
    skip; it is part of the captured step, so a replay plants what the buffer holds then."""

    def __init__(self, mixed, batch0, plant=False, **kw):
        self.m, self.opt = cases.build(torch.device(DEV), mixed, **kw)
        self.x, self.t = (torch.empty_like(v) for v in batch0)
        self.plant, self.poison = plant, torch.zeros(1, device=DEV)

    def load(self, batch, poison=0.0):
        self.x.copy_(batch[0])
        self.t.copy_(batch[1])
        self.poison.fill_(poison)

    def step(self):
        self.opt.zero_grad()
        loss = cases.loss_fn(self.m, (self.x, self.t))
        loss.backward()
        if self.plant:
            b = self.opt.reducer.buckets[-1]
            g = self.opt.reducer.reduced(b)
            g[b.offs[0] + 1:b.offs[0] + 2] += self.poison.to(g.dtype)
        self.opt.step()
        return loss.detach()

    def state(self):
        return cases.whole_state(self.m, self.opt)


def _capture(tw, s):
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out = tw.step()
    return g, out


def _eager_vs_replay(mixed, poison_at=None, rates=None, **kw):
    """two twins from the same seed: WARM eager steps each, then K eager steps against ONE capture replayed K times.  poison_at: the
    index of the step whose gradient gets an inf; rates: a rate per step after the warm-up, set between the replays (device_lr)"""
    batches = cases.batches(torch.device(DEV), mixed, WARM + K)
    s = _stream()
    with torch.cuda.stream(s):
        e, r = (_Twin(mixed, batches[0], plant=poison_at is not None, **kw) for _ in range(2))
        assert cases.states_equal(e.state(), r.state())
        for tw in (e, r):
            for b in batches[:WARM]:
                tw.load(b)
                tw.step()
        le, lr_, skipped_state = [], [], None
        for i, b in enumerate(batches[WARM:]):
            if rates is not None:
                e.opt.set_lr(rates[i])
            e.load(b, float("inf") if i == poison_at else 0.0)
            before = e.state() if i == poison_at else None
            le.append(e.step().clone())
            if i == poison_at:
                after = e.state()
                n = len(cases.opt_state(e.m, e.opt))
                assert cases.states_equal(before[:n - 1], after[:n - 1]), "the eager skipped step wrote weights, masters or moments"
                assert torch.equal(before[n - 1][:3], after[n - 1][:3]) and int(after[n - 1][3]) == int(before[n - 1][3]) + 1
        graph, out = _capture(r, s)
        for i, b in enumerate(batches[WARM:]):
            if rates is not None:
                r.opt.set_lr(rates[i])
            r.load(b, float("inf") if i == poison_at else 0.0)
            before = r.state() if i == poison_at else None
            graph.replay()
            clf.invalidate_packs()
            lr_.append(out.clone())
            if i == poison_at:
                after = r.state()
                n = len(cases.opt_state(r.m, r.opt))
                assert cases.states_equal(before[:n - 1], after[:n - 1]), "the replayed skipped step wrote weights, masters or moments"
                assert torch.equal(before[n - 1][:3], after[n - 1][:3]), "the replayed skipped step advanced the count"
        torch.cuda.synchronize()
        assert torch.equal(torch.stack(le), torch.stack(lr_)), (torch.stack(le).tolist(), torch.stack(lr_).tolist())
        assert len({float(v) for v in le}) == K
        assert not cases.differing(e.state(), r.state()), ("eager and replayed runs differ", cases.differing(e.state(), r.state()))
        stats = r.opt.adam_stats()
        assert stats == e.opt.adam_stats() and stats["step"] == WARM + K - (poison_at is not None)
        assert stats["refused"] == (1 if poison_at is not None else 0)
        del graph
    torch.cuda.current_stream().wait_stream(s)
    return e, r


@pytest.mark.parametrize("mixed", FORMS, ids=FORM_IDS)
def test_replay_equals_eager(mixed):
    _eager_vs_replay(mixed, ema_decay=0.9)


def test_replay_follows_a_changed_rate():
    e, r = _eager_vs_replay(True, rates=[2e-3, 1e-3, 1e-3, 5e-4, 2.5e-4], device_lr=True)
    assert r.opt.lr == 2.5e-4 and float(r.opt.lr_dev) == cases.f32(2.5e-4)


def test_replay_skips_a_non_finite_step():
    _eager_vs_replay(True, poison_at=2, skip_nonfinite=True, ema_decay=0.9)


def test_checkpoint_loads_behind_a_capture():
    """the fresh optimizer's step is captured BEFORE the load (after one eager warm-up step of its own); every load is in place, so the
    replays run the loaded state: two replays give what five uninterrupted steps give"""
    s = _stream()
    held = []

    def captured(model, opt):
        batch0 = cases.batches(torch.device(DEV), True, 1, seed=77)[0]
        tw = _Twin.__new__(_Twin)
        tw.m, tw.opt, tw.plant, tw.poison = model, opt, False, torch.zeros(1, device=DEV)
        tw.x, tw.t = (v.clone() for v in batch0)
        tw.step()
        graph, _ = _capture(tw, s)
        held.append(graph)

        def step(b):
            tw.load(b)
            graph.replay()
            clf.invalidate_packs()
        return step
    with torch.cuda.stream(s):
        cases.check_checkpoint(torch.device(DEV), True, captured=captured, device_lr=True, skip_nonfinite=True)
        torch.cuda.synchronize()
        held.clear()
    torch.cuda.current_stream().wait_stream(s)
