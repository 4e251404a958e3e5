"""Adaptive gradient clipping on the device: tests/agc_cases.py's kernel cases through the real library, and FlatSGD(agc=...,
skip_nonfinite=True) replayed from ONE HIP-graph capture against the same sequence issued eagerly, BIT FOR BIT
(tests/test_graph_replay_gpu.py's harness: twins on static buffers, one non-default stream)."""
import pytest
import torch

from cotnet_amd import _lib, cot_layer_fused as clf
from cotnet_amd.cotnet import Bottleneck
from cotnet_amd.lr_schedule import CosineSchedule
from tests import agc_cases as cases
from tests import truth
from tests.test_graph_replay_gpu import NCHW, _Twin, _batches, _capture, _opening, _replay, _same, _stage, _stream, mse

pytestmark = pytest.mark.gpu
DEV = "cuda"
WARM, REPLAYS = 2, 5


def _L():
    return _lib.lib()


def _run(check, *a):
    check(_L(), torch.device(DEV), _lib.stream(), *a, sync=torch.cuda.synchronize)


@pytest.mark.parametrize("gdt", cases.GRAD_DTYPES, ids=cases.GRAD_IDS)
def test_coefficients_clipped_elements_and_determinism(gdt):
    for name in cases.cases(_L()):
        _run(cases.check_case, name, gdt)


@pytest.mark.parametrize("gdt", cases.GRAD_DTYPES, ids=cases.GRAD_IDS)
def test_eps_floor(gdt):
    _run(cases.check_eps_floor, gdt)


@pytest.mark.parametrize("gdt", cases.GRAD_DTYPES, ids=cases.GRAD_IDS)
def test_zero_gradient(gdt):
    _run(cases.check_zero_gradient, gdt)


@pytest.mark.parametrize("kind,gdt", [(k, dt) for k in cases.NONFINITE for dt in cases.GRAD_DTYPES
                                      if k != "bf16-overflowing-squares" or dt == torch.bfloat16],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_non_finite_units_are_marked_and_left_alone(kind, gdt):
    _run(cases.check_nonfinite, kind, gdt)


def test_the_reference_fixture():
    _run(cases.check_fixture)


def test_refusals_leave_everything_alone():
    _run(cases.check_refusals)


# ---- one capture serves every step

CANDIDATES = [0.01, 0.003, 0.03, 0.001, 0.1]  # factors a probe twin tries in turn, the reference's default first


def _coefs(tw):
    return torch.cat(tw.opt._agc_coef).clone()


def _eager(tw, batches, sched):
    losses, coefs, stats = [], [], []
    for i, b in enumerate(batches):
        if sched is not None:
            tw.opt.set_lr(sched.value(i))
        tw.load(b)
        losses.append(tw.step().clone())
        coefs.append(_coefs(tw))
        stats.append(tw.opt.agc_stats())
    return losses, coefs, stats


def _replayed(tw, batches, sched, s):
    """WARM eager steps, ONE capture, a replay per remaining batch"""
    losses, coefs, stats = _eager(tw, batches[:WARM], sched)
    g, out = _capture(tw, s)
    for i, b in enumerate(batches[WARM:], start=WARM):
        if sched is not None:
            tw.opt.set_lr(sched.value(i))
        losses.append(_replay(tw, g, out, b))
        coefs.append(_coefs(tw))
        stats.append(tw.opt.agc_stats())
    return losses, coefs, stats, g


def _mixed(stats):
    """in every step some units clip and some do not, and none is marked"""
    return all(0 < st["clipped"] < st["units"] and st["nonfinite"] == 0 for st in stats)


def agc_vs_replay(sched=None, **opt_kw):
    n = WARM + REPLAYS
    batches = _batches((8, 128, 28, 28), (8, 256, 14, 14), 131, n=n)
    _lib.FALLBACKS.clear()
    s = _stream()
    with truth.switches(**NCHW), torch.cuda.stream(s):
        model = _stage(9, _opening(), lambda: Bottleneck(256, 64))()
        clf.plan_stage_layouts(model)
        lr0 = sched.value(0) if sched is not None else 0.05
        # place the factor among the ratios this stage really produces: a probe twin's agc_stats() per step (the eager twin below,
        # on the same batches with the same factor, repeats the probe bit for bit)
        agc, seen = None, {}
        for cand in CANDIDATES:
            probe = _Twin(model, mse, batches[0], lr0, agc=cand, skip_nonfinite=True, **opt_kw)
            seen[cand] = [(st["clipped"], st["units"]) for st in _eager(probe, batches, sched)[2]]
            del probe
            if all(0 < c < u for c, u in seen[cand]):
                agc = cand
                break
        assert agc is not None, f"no factor separates this stage's units in every step: {seen}"
        e = _Twin(model, mse, batches[0], lr0, agc=agc, skip_nonfinite=True, **opt_kw)
        r = _Twin(model, mse, batches[0], lr0, agc=agc, skip_nonfinite=True, **opt_kw)
        le, ce, se = _eager(e, batches, sched)
        lr_, cr, sr, graph = _replayed(r, batches, sched, s)
        torch.cuda.synchronize()
        assert torch.equal(torch.stack(le), torch.stack(lr_)), f"loss per step, eager {torch.stack(le).tolist()} vs replay {torch.stack(lr_).tolist()}"
        assert len({float(v) for v in le}) == n and all(bool(torch.isfinite(v)) for v in le)  # (the steps do differ)
        assert all(torch.equal(u, v) for u, v in zip(ce, cr)), "the coefficients differ between eager and replay"
        assert se == sr and _mixed(sr), sr
        assert len({tuple(c.tolist()) for c in cr[WARM:]}) == REPLAYS  # (the replays' coefficients are not one frozen set)
        _same(e.state(), r.state(), "after the last step, eager vs replay with agc")
        cs = r.opt.clip_stats()
        assert (cs["steps"], cs["skipped"], cs["clipped"], cs["scale"]) == (n, 0, 0, 1.0), cs
        assert not _lib.FALLBACKS, dict(_lib.FALLBACKS)
        del graph
    torch.cuda.current_stream().wait_stream(s)


def test_one_capture_serves_every_step_with_agc():
    agc_vs_replay()


def test_the_same_with_the_rate_on_the_device_under_a_schedule():
    agc_vs_replay(sched=CosineSchedule(0.05, WARM + REPLAYS, warmup_t=2, warmup_lr_init=5e-4, lr_min=1e-5), device_lr=True)
