"""Lookahead on the flat optimizers (cot_lookahead_tick, cot_lookahead_step, FlatSGD / FlatAdamW(lookahead_k=...)) -- on the device.

The cases are tests/lookahead_cases.py's, the list tests/test_lookahead_emulated.py runs on the host emulator, plus the size at which a
lane makes a second trip of the grid-stride loop.  Then ONE HIP-graph capture of forward, backward and step replayed against eager
steps, BIT FOR BIT -- built like tests/test_adamw_gpu.py: twins on static buffers, one non-default stream, all batches different --
with k = 2, so that the five replays of the one capture are sync steps, non-sync steps and one skipped step.

Everything that compares two runs uses adamw_cases.small(), whose torch operators are reproducible on the device in both forms."""
import pytest
import torch

from cotnet_amd import _lib, cot_layer_fused as clf
from tests import adamw_cases as adamw
from tests import lookahead_cases as cases
from tests.test_graph_replay_gpu import _stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
MIXED, MIXED_IDS = [False, True], ["fp32", "mixed-bf16"]
WARM, REPLAYS = 2, 5


def _dev():
    return _lib.lib(), torch.device(DEV), _lib.stream(), torch.cuda.synchronize


@pytest.mark.parametrize("pdt", cases.FORMS, ids=cases.FORM_IDS)
@pytest.mark.parametrize("alpha", [0.5, 0.3])
@pytest.mark.parametrize("n", cases.SIZES + [cases.SECOND_TRIP])
def test_interpolation_against_the_formula(pdt, alpha, n):
    L, dev, stream, sync = _dev()
    cases.check_interpolation(L, dev, stream, pdt, n, alpha, sync)


@pytest.mark.parametrize("pdt", cases.FORMS, ids=cases.FORM_IDS)
def test_action_0_writes_nothing_and_action_1_only_adopts(pdt):
    L, dev, stream, sync = _dev()
    cases.check_actions(L, dev, stream, pdt, sync)


def test_tick():
    L, dev, stream, sync = _dev()
    cases.check_tick(L, dev, stream, sync)


def test_tick_behind_a_skip():
    L, dev, stream, sync = _dev()
    cases.check_tick_skip(L, dev, stream, sync)


@pytest.mark.parametrize("alpha", [0.5, 0.8])
@pytest.mark.parametrize("t", [3, 6, 8])
def test_the_reference_fixture(alpha, t):
    L, dev, stream, sync = _dev()
    cases.check_fixture_sync(L, dev, stream, alpha, t, sync)


def test_refusals_leave_everything_alone():
    L, dev, stream, sync = _dev()
    cases.check_refusals(L, dev, stream, sync)


@pytest.mark.parametrize("pdt", cases.FORMS, ids=cases.FORM_IDS)
def test_two_calls_give_equal_bits(pdt):
    L, dev, stream, sync = _dev()
    cases.check_repeatable(L, dev, stream, pdt, sync)


# ---- the optimizers, eager

@pytest.mark.parametrize("mixed", MIXED, ids=MIXED_IDS)
@pytest.mark.parametrize("rule", cases.RULES)
def test_twin_protocol(mixed, rule):
    cases.check_twin_protocol(torch.device(DEV), mixed, rule)


@pytest.mark.parametrize("mixed", MIXED, ids=MIXED_IDS)
@pytest.mark.parametrize("rule", cases.RULES)
def test_the_average_follows_the_weights_after_the_sync(mixed, rule):
    cases.check_ema_follows_the_sync(torch.device(DEV), mixed, rule)


@pytest.mark.parametrize("mixed", MIXED, ids=MIXED_IDS)
@pytest.mark.parametrize("rule", cases.RULES)
def test_a_skipped_step_is_not_counted(mixed, rule):
    cases.check_skipped_step(torch.device(DEV), mixed, rule)


@pytest.mark.parametrize("mixed", MIXED, ids=MIXED_IDS)
@pytest.mark.parametrize("rule", cases.RULES)
def test_sync_lookahead(mixed, rule):
    cases.check_sync_lookahead(torch.device(DEV), mixed, rule)


@pytest.mark.parametrize("mixed", MIXED, ids=MIXED_IDS)
@pytest.mark.parametrize("rule", cases.RULES)
@pytest.mark.parametrize("at", [2, 4], ids=["unborn", "born"])
def test_checkpoint_resumes_bit_equal(mixed, rule, at):
    cases.check_checkpoint(torch.device(DEV), mixed, rule, at)


@pytest.mark.parametrize("rule", cases.RULES)
@pytest.mark.parametrize("at", [2, 4], ids=["unborn", "born"])
def test_checkpoint_saver_round_trip(rule, at, tmp_path):
    cases.check_checkpoint(torch.device(DEV), True, rule, at, tmp_path=tmp_path, skip_nonfinite=True)


@pytest.mark.parametrize("rule", cases.RULES)
def test_load_state_dict_refusals(rule):
    cases.check_load_refusals(torch.device(DEV), True, rule)


def test_sync_lookahead_and_the_reads_are_refused_while_capturing(monkeypatch):
    """(the flag alone is set: a real capture that ends in an exception is left to nobody)"""
    model, opt = cases.build(torch.device(DEV), True, "sgd", lookahead_k=2)
    adamw.train_step(model, opt, adamw.batches(torch.device(DEV), True, 1)[0])
    before = cases.whole_state(model, opt, "sgd")
    monkeypatch.setattr(_lib, "capturing", lambda: True)
    for call in (opt.sync_lookahead, opt.lookahead_stats, opt.state_dict):
        with pytest.raises(RuntimeError, match="inside a HIP-graph capture"):
            call()
    monkeypatch.undo()
    assert adamw.states_equal(before, cases.whole_state(model, opt, "sgd"))


# ---- one capture replayed

class _Twin:
    """a model and its optimizer reading input and target from static buffers.  `plant`: between backward and step the one-element
    `poison` buffer is added to one element of the last gradient bucket -- 0 leaves the gradient as it is, inf makes the step one to skip; it
    is part of the captured step, so a replay plants what the buffer holds then."""

    def __init__(self, model, opt, rule, batch0, plant=False):
        self.m, self.opt, self.rule, self.plant = model, opt, rule, plant
        self.x, self.t = (v.clone() for v in batch0)
        self.poison = torch.zeros(1, device=DEV)

    def load(self, batch, poison=0.0):
        self.x.copy_(batch[0])
        self.t.copy_(batch[1])
        self.poison.fill_(poison)

    def step(self):
        self.opt.zero_grad()
        loss = adamw.loss_fn(self.m, (self.x, self.t))
        loss.backward()
        if self.plant:
            b = self.opt.reducer.buckets[-1]
            g = self.opt.reducer.reduced(b)
            g[b.offs[0] + 1:b.offs[0] + 2] += self.poison.to(g.dtype)
        self.opt.step()
        return loss.detach()

    def state(self):
        return cases.whole_state(self.m, self.opt, self.rule)


def _capture(tw, s):
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out = tw.step()
    return g, out


@pytest.mark.parametrize("mixed", MIXED, ids=MIXED_IDS)
@pytest.mark.parametrize("rule", cases.RULES)
def test_replay_equals_eager_through_syncs_and_a_skip(mixed, rule):
    """k = 2: two eager warm-up steps each (the second adopts), then five eager steps against ONE capture replayed five times.  The
    second of the five carries an inf: it would have been step 4, a sync -- it is refused, and the sync happens at the next accepted
    step."""
    dev, poison_at = torch.device(DEV), 1
    batches = adamw.batches(dev, mixed, WARM + REPLAYS)
    s = _stream()
    with torch.cuda.stream(s):
        e, r = (_Twin(*cases.build(dev, mixed, rule, lookahead_k=2, skip_nonfinite=True, ema_decay=0.9), rule, batches[0], plant=True)
                for _ in range(2))
        assert adamw.states_equal(e.state(), r.state())
        for tw in (e, r):
            for b in batches[:WARM]:
                tw.load(b)
                tw.step()
        assert e.opt.lookahead_stats() == dict(step=2, born=1, syncs=1, refused=0)
        le, lr_ = [], []
        for i, b in enumerate(batches[WARM:]):
            e.load(b, float("inf") if i == poison_at else 0.0)
            le.append(e.step().clone())
        graph, out = _capture(r, s)
        assert r.opt._captured_lookahead == (2, 0.5)
        for i, b in enumerate(batches[WARM:]):
            r.load(b, float("inf") if i == poison_at else 0.0)
            graph.replay()
            clf.invalidate_packs()
            lr_.append(out.clone())
        torch.cuda.synchronize()
        assert torch.equal(torch.stack(le), torch.stack(lr_)), (torch.stack(le).tolist(), torch.stack(lr_).tolist())
        diff = adamw.differing(e.state(), r.state())
        assert not diff, ("eager and replayed runs differ", diff)
        stats = r.opt.lookahead_stats()
        assert stats == e.opt.lookahead_stats() == dict(step=WARM + REPLAYS - 1, born=1, syncs=3, refused=1), stats
        assert adamw.states_equal([st["slow"] for st in r.opt.state], cases.weights(r.opt)), "the last replay (step 6) was a sync"
        sd = r.opt.state_dict()
        with pytest.raises(ValueError, match="captured into a HIP graph with \\(lookahead_k, lookahead_alpha\\)"):
            r.opt.load_state_dict(dict(sd, param_groups=[dict(g, lookahead_alpha=0.75) for g in sd["param_groups"]]))
        del graph
    torch.cuda.current_stream().wait_stream(s)


@pytest.mark.parametrize("rule", cases.RULES)
@pytest.mark.parametrize("at", [2, 4], ids=["unborn", "born"])
def test_checkpoint_loads_behind_a_capture(rule, at):
    """the fresh optimizer's step is captured BEFORE the load (after one eager warm-up step of its own); every load is in place, so the
    replays run the loaded state -- slow weights and block included: the replays to step 7 give what seven uninterrupted steps give.
    A load that would change k or alpha behind the capture raises."""
    s = _stream()
    held = []

    def captured(model, opt):
        tw = _Twin(model, opt, rule, adamw.batches(torch.device(DEV), True, 1, seed=77)[0])
        tw.step()
        graph, _ = _capture(tw, s)
        held.append(graph)

        def step(b):
            tw.load(b)
            graph.replay()
            clf.invalidate_packs()
        return step
    with torch.cuda.stream(s):
        cases.check_checkpoint(torch.device(DEV), True, rule, at, captured=captured, device_lr=True, skip_nonfinite=True)
        torch.cuda.synchronize()
        held.clear()
    torch.cuda.current_stream().wait_stream(s)
