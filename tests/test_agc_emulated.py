"""Adaptive gradient clipping (cot_agc_clip, FlatSGD(agc=...)) -- on the host emulator.

The kernel cases are tests/agc_cases.py's, the same list the device runs (tests/test_agc_gpu.py); none is dropped here.  Then FlatSGD on
tests/test_grad_clip_emulated.py's small model and four loss scales: an fp32 net against torch.optim.SGD behind the formula written out
afresh, the mixed-bf16 masters against fp32 SGD fed `grad.float() * coef`, what is allocated and launched with and without agc, the order
of the launches under the guard, and a NaN gradient."""
import pytest
import torch

from cotnet_amd import _lib
from tests import agc_cases as cases
from tests.emul import build_emul
from tests.test_grad_clip_emulated import _EMUL  # (ONE handle: _emulated and _counted put that module's behind _lib.lib())
from tests.test_grad_clip_emulated import HP, STEPS, _counted, _emulated, _equal, _inputs, _loss, _model, _opt, _state, _step

pytestmark = pytest.mark.skipif(_EMUL is None, reason="host emulation build unavailable")
CPU = torch.device("cpu")
CASES = list(cases.cases(_EMUL)) if _EMUL is not None else []


def test_max_groups_is_the_header_constant():
    import os
    import re
    hdr = open(os.path.join(build_emul.ROOT, "include", "cotnet_amd.h")).read()
    assert _EMUL.cot_agc_max_groups() == int(re.search(r"#define COT_AGC_MAX_GROUPS (\d+)", hdr).group(1))
    assert "cot_agc_max_groups" in _lib.NOT_STATUS and "cot_agc_clip" not in _lib.NOT_STATUS


@pytest.mark.parametrize("gdt", cases.GRAD_DTYPES, ids=cases.GRAD_IDS)
@pytest.mark.parametrize("name", CASES)
def test_coefficients_clipped_elements_and_determinism(name, gdt):
    cases.check_case(_EMUL, CPU, None, name, gdt)


@pytest.mark.parametrize("gdt", cases.GRAD_DTYPES, ids=cases.GRAD_IDS)
def test_eps_floor(gdt):
    cases.check_eps_floor(_EMUL, CPU, None, gdt)


@pytest.mark.parametrize("gdt", cases.GRAD_DTYPES, ids=cases.GRAD_IDS)
def test_zero_gradient(gdt):
    cases.check_zero_gradient(_EMUL, CPU, None, gdt)


@pytest.mark.parametrize("kind,gdt", [(k, dt) for k in cases.NONFINITE for dt in cases.GRAD_DTYPES
                                      if k != "bf16-overflowing-squares" or dt == torch.bfloat16],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_non_finite_units_are_marked_and_left_alone(kind, gdt):
    cases.check_nonfinite(_EMUL, CPU, None, kind, gdt)


def test_the_reference_fixture():
    cases.check_fixture(_EMUL, CPU, None)


def test_refusals_leave_everything_alone():
    cases.check_refusals(_EMUL, CPU, None)


# ---- FlatSGD

# The factor.  A clipped unit is stored back into its bucket in the bucket's dtype, so in a bf16 bucket every clipped element carries one
# more rounding of 2^-9 relative, which fp32 SGD fed the unrounded `grad.float() * coef` does not have.  A clipped row has the norm
# agc * wn, so an element of it is at most agc * wn ~ 3 agc |w| here (rows of 8); four nesterov steps at lr 0.1, momentum 0.9 weigh the
# roundings with 0.1 * (1.9 + 2.71 + 3.44 + 4.1) = 1.2 at the most.  For the masters to stay within rtol 1e-5 of that reference whatever
# the signs, 1.2 * 3 * agc * 2^-9 <= 1e-5, i.e. agc <= 1.4e-3: the factor is 1e-3.  (At the reference's default of 0.01 the roundings
# alone come to 1e-5 |w| per step.)  Under the four loss scales some units of this model clip and some do not in every step, which the
# tests assert.
AGC = 1e-3
NAMES = ("cot_sgd_step", "cot_sgd_step_lr", "cot_sgd_step_clip", "cot_grad_sumsq", "cot_grad_clip_finish", "cot_agc_clip")


def _rows(t):
    """[units, elements per unit]: the reference's unitwise_norm"""
    return t.reshape(1, -1) if t.ndim <= 1 else t.reshape(t.shape[0], -1)


def _formula(w, g, factor, eps=1e-3):
    """adaptive_clip_grad, written out: (coef per unit, clipped gradient), in the dtype of w"""
    max_norm = _rows(w).norm(dim=1).clamp(min=eps) * factor
    gn = _rows(g).norm(dim=1)
    coef = torch.where(gn < max_norm, torch.ones_like(gn), max_norm / gn.clamp(min=1e-6))
    return coef, (_rows(g) * coef[:, None]).reshape(g.shape)


def _bucket_units(opt):
    """{param: (start, len) rows of its units inside its bucket}"""
    out = {}
    for b in opt.reducer.buckets:
        for p, off in zip(b.params, b.offs):
            r = _rows(p).shape
            out[p] = [(off + i * r[1], r[1]) for i in range(r[0])]
    return out


def test_unit_tables_follow_the_buckets_slots(monkeypatch):
    _emulated(monkeypatch)
    model = _model(True)
    opt = _opt(model, agc=AGC)
    assert opt.agc == AGC and opt.agc_eps == 1e-3
    units = _bucket_units(opt)
    for b, table, coef in zip(opt.reducer.buckets, opt._agc_units, opt._agc_coef):
        assert table.dtype == torch.int64 and table.is_contiguous() and table.data_ptr() % 8 == 0
        assert table.tolist() == [list(u) for p in b.params for u in units[p]]
        assert coef.dtype == torch.float32 and coef.shape == (table.shape[0],)
    views = opt.agc_coefficients()
    assert [tuple(views[p].shape) for p in model.parameters()] == [(8,), (1,), (1,), (1,)]
    assert sum(v.numel() for v in views.values()) == 11 == opt.agc_stats()["units"]


def test_fp32_net_follows_torch_sgd_behind_the_formula(monkeypatch):
    """tests/test_flat_sgd_gpu.py's fp32 bounds (rtol 2e-5, atol 2e-6) after four steps in each of which some units clip and some do not"""
    _emulated(monkeypatch)
    ours, twin = _model(False), _model(False)
    opt = _opt(ours, agc=AGC)
    decay = [p for n, p in twin.named_parameters() if p.ndim > 1 and not n.endswith(".bias")]
    rest = [p for n, p in twin.named_parameters() if not (p.ndim > 1 and not n.endswith(".bias"))]
    ref = torch.optim.SGD([dict(params=decay, weight_decay=HP["weight_decay"]), dict(params=rest, weight_decay=0.0)], lr=HP["lr"],
                          momentum=HP["momentum"], nesterov=True)
    for i, x in enumerate(_inputs(False)):
        _step(ours, opt, x)
        ref.zero_grad()
        _loss(twin, x).backward()
        clipped = 0
        for p in twin.parameters():
            coef, p.grad = _formula(p.detach(), p.grad, AGC)
            clipped += int((coef < 1).sum())
        ref.step()
        s = opt.agc_stats()
        assert s["units"] == 11 and s["nonfinite"] == 0 and 0 < s["clipped"] < s["units"], (i, s)
        assert s["clipped"] == clipped, (i, s, clipped)
        for p, q in zip(ours.parameters(), twin.parameters()):
            assert torch.allclose(p, q, rtol=2e-5, atol=2e-6), f"step {i}"


def test_mixed_bf16_masters_follow_fp32_sgd_fed_the_clipped_gradient(monkeypatch):
    """the masters against fp32 SGD on `grad.float() * coef`, coef = the device's own (rtol 1e-5, atol 1e-6, test_flat_sgd_gpu.py's bounds
    for this form), and those coefficients against the formula in fp64 on the bucket's gradients and the masters, within
    agc_cases' bound, on the decided units -- of which the seed leaves none out"""
    _emulated(monkeypatch)
    model = _model(True)
    opt = _opt(model, agc=AGC)
    masters = opt.master_parameters()
    ref = {p: masters[p].clone() for p in model.parameters()}
    mom = {p: torch.zeros_like(ref[p]) for p in ref}
    wd = {p: (HP["weight_decay"] if b.key == "decay" else 0.0) for b in opt.reducer.buckets for p in b.params}
    units = _bucket_units(opt)
    for i, x in enumerate(_inputs(True)):
        opt.zero_grad()
        _loss(model, x).backward()
        grads = {p: opt.reducer.reduced(b)[off:off + p.numel()].clone()  # (the gradients live in the buckets: no .grad)
                 for b in opt.reducer.buckets for p, off in zip(b.params, b.offs)}
        before = {p: opt.master_parameters()[p].clone() for p in ref}
        opt.step()
        coefs = {p: c.clone() for p, c in opt.agc_coefficients().items()}
        s = opt.agc_stats()
        assert s["nonfinite"] == 0 and 0 < s["clipped"] < s["units"] == 11, (i, s)
        undecided = 0
        for p in ref:
            gdt = grads[p].dtype
            want, _ = _formula(before[p].double(), grads[p].view_as(p).double(), float(torch.tensor(AGC, dtype=torch.float32)),
                               float(torch.tensor(1e-3, dtype=torch.float32)))
            max_norm = _rows(before[p].double()).norm(dim=1).clamp(min=float(torch.tensor(1e-3, dtype=torch.float32))) \
                * float(torch.tensor(AGC, dtype=torch.float32))
            ratio = _rows(grads[p].view_as(p).double()).norm(dim=1) / max_norm
            bound = torch.tensor([cases.norm_bound(st, n, 4) + cases.norm_bound(st, n, cases.vec(gdt)) + 3 * cases.U for st, n in units[p]],
                                 dtype=torch.float64)
            ok = (ratio - 1).abs() > 2 * bound
            undecided += int((~ok).sum())
            assert bool(((coefs[p].double() - want).abs() <= bound * want)[ok].all()), (i, coefs[p], want)
            assert bool((coefs[p][ok & (want == 1)] == 1.0).all())
            g = (_rows(grads[p].view_as(p).float()) * coefs[p][:, None]).reshape(p.shape) + wd[p] * ref[p]
            mom[p] = HP["momentum"] * mom[p] + g
            ref[p] = ref[p] - HP["lr"] * (g + HP["momentum"] * mom[p])
            m = opt.master_parameters()[p]
            print(f"step {i}, {tuple(p.shape)} {gdt}: worst |master - ref| / (1e-6 + 1e-5 |ref|) = "
                  f"{float(((m - ref[p]).abs() / (1e-6 + 1e-5 * ref[p].abs())).max()):.3f}")
            assert torch.allclose(m, ref[p], rtol=1e-5, atol=1e-6), f"step {i}"
            assert torch.equal(p.detach(), m.to(p.dtype))
        assert undecided == 0, (i, undecided)


def test_off_allocates_nothing_and_launches_the_old_entry_points(monkeypatch):
    _emulated(monkeypatch)
    for kw, used in ((dict(agc=None), "cot_sgd_step"), (dict(agc=0), "cot_sgd_step"), (dict(agc=-1), "cot_sgd_step"),
                     (dict(agc=0.0, device_lr=True), "cot_sgd_step_lr")):
        with monkeypatch.context() as mp:
            calls = {n: _counted(mp, n) for n in NAMES}
            model = _model(True)
            opt = _opt(model, **kw)
            assert opt.agc is None and opt._agc_units is None and opt._agc_coef is None and opt.clip_state is None
            for x in _inputs(True)[:2]:
                _step(model, opt, x)
            n = 2 * len(opt.reducer.buckets)
            assert {k: len(v) for k, v in calls.items()} == {k: (n if k == used else 0) for k in NAMES}, kw
            for read in (opt.agc_stats, opt.agc_coefficients):
                with pytest.raises(RuntimeError, match="without agc"):
                    read()


@pytest.mark.parametrize("device_lr", [False, True])
def test_launches_and_addresses_with_agc(device_lr, monkeypatch):
    """per step one cot_agc_clip per bucket on the reduced gradients, the fp32 weights, the bucket's table and coefficient tensor -- the
    same addresses in every step and under a (mocked) capture -- and then the plain optimizer's launches"""
    _emulated(monkeypatch)
    model = _model(True)
    opt = _opt(model, agc=AGC, device_lr=device_lr)
    nb = len(opt.reducer.buckets)
    addr = [(t.data_ptr(), c.data_ptr()) for t, c in zip(opt._agc_units, opt._agc_coef)]
    calls = {n: _counted(monkeypatch, n) for n in NAMES}
    xs = _inputs(True)
    _step(model, opt, xs[0])
    monkeypatch.setattr(_lib, "capturing", lambda: True)
    _step(model, opt, xs[1])
    with pytest.raises(RuntimeError, match="capture"):
        opt.agc_stats()
    monkeypatch.setattr(_lib, "capturing", lambda: False)
    sgd_name = "cot_sgd_step_lr" if device_lr else "cot_sgd_step"
    assert {k: len(v) for k, v in calls.items()} == {k: (2 * nb if k in (sgd_name, "cot_agc_clip") else 0) for k in NAMES}
    want = []
    for b, st, (t, c), table in zip(opt.reducer.buckets, opt.state, addr, opt._agc_units):
        g = opt.reducer.reduced(b)
        weight = st["master"] if st["master"] is not None else b.pflat
        assert weight.dtype == torch.float32
        want.append((g.data_ptr(), weight.data_ptr(), t, table.shape[0], g.numel(), AGC, 1e-3, c, _lib.dtype_code(g.dtype), None))
    assert [tuple(a) for a in calls["cot_agc_clip"]] == want * 2
    assert [(t.data_ptr(), c.data_ptr()) for t, c in zip(opt._agc_units, opt._agc_coef)] == addr
    assert opt.agc_stats()["units"] == 11


def test_the_guard_follows_the_agc_launches(monkeypatch):
    """with skip_nonfinite=True: every cot_agc_clip of a step, then cot_grad_sumsq per bucket, the finish with max_norm = inf, and
    cot_sgd_step_clip -- the guard sees the gradients the step consumes"""
    _emulated(monkeypatch)
    model = _model(True)
    opt = _opt(model, agc=AGC, skip_nonfinite=True)
    nb = len(opt.reducer.buckets)
    order = []
    for name in NAMES:
        raw = getattr(_EMUL, name)
        monkeypatch.setattr(_EMUL, name, lambda *a, _raw=raw, _name=name: (order.append((_name, a)), _raw(*a))[1])
    _step(model, opt, _inputs(True)[0])
    assert [n for n, _ in order] == ["cot_agc_clip"] * nb + ["cot_grad_sumsq"] * nb + ["cot_grad_clip_finish"] + ["cot_sgd_step_clip"] * nb
    assert order[2 * nb][1][2] == float("inf")
    assert [a[0] for n, a in order if n == "cot_grad_sumsq"] == [a[0] for n, a in order if n == "cot_agc_clip"]
    s = opt.clip_stats()
    assert (s["skip"], s["scale"], s["steps"]) == (0, 1.0, 1), s


def test_agc_together_with_clip_grad_raises(monkeypatch):
    _emulated(monkeypatch)
    with pytest.raises(ValueError, match="one clipping mode per step"):
        _opt(_model(True), agc=0.01, clip_grad=1.0)
    opt = _opt(_model(True), agc=0.01, clip_grad=0.0)  # (clip_grad off: no conflict)
    assert opt.agc == 0.01 and opt.clip_grad is None
    with pytest.raises(ValueError, match="finite and positive"):
        _opt(_model(True), agc=0.01, agc_eps=0.0)


def test_a_planted_nan_skips_the_step_and_stays_where_it_was(monkeypatch):
    """one NaN in ONE bucket: its unit is marked and left alone, the guard skips the step for every bucket, and the value is still there"""
    _emulated(monkeypatch)
    model = _model(True)
    opt = _opt(model, agc=AGC, skip_nonfinite=True)
    xs = _inputs(True)
    _step(model, opt, xs[0])
    before = _state(model, opt)
    opt.zero_grad()
    _loss(model, xs[1]).backward()
    b = opt.reducer.buckets[-1]
    bucket = opt.reducer.reduced(b)
    at = b.offs[0] + 1
    bucket[at] = float("nan")
    opt.step()
    assert bool(torch.isnan(bucket[at])) and int(torch.isnan(bucket).sum()) == 1, "the planted NaN moved or spread"
    s, a = opt.clip_stats(), opt.agc_stats()
    assert (s["skip"], s["scale"], s["steps"], s["skipped"]) == (1, 0.0, 2, 1), s
    assert a["nonfinite"] == 1 and a["units"] == 11, a
    assert _equal(before, _state(model, opt)), "a skipped step wrote parameters, masters or momentum"
    _step(model, opt, xs[2])  # the next step trains again
    s, a = opt.clip_stats(), opt.agc_stats()
    assert (s["skip"], s["steps"], s["skipped"]) == (0, 3, 1) and a["nonfinite"] == 0 and not _equal(before, _state(model, opt)), (s, a)
    assert STEPS == len(xs)
