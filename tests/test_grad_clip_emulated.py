"""Gradient clipping by global norm and the non-finite guard (cot_grad_sumsq, cot_grad_clip_finish, cot_sgd_step_clip,
FlatSGD(clip_grad=..., skip_nonfinite=...)) -- on the host emulator.

The kernel cases are tests/grad_clip_cases.py's, the same list the device runs (tests/test_grad_clip_gpu.py).  Dropped here because
they take more than a few seconds on the emulator: nothing -- the largest, 2^20 + 5 elements, is under a second.  Then FlatSGD:
against torch.optim.SGD behind torch.nn.utils.clip_grad_norm_ on an fp32 twin, against fp32 SGD fed `grad.float() * scale` in the
mixed-bf16 form, the guard alone against the plain optimizer, a NaN gradient, and the launches of the default arguments."""
import copy
import ctypes

import pytest
import torch
from torch import nn

from cotnet_amd import _lib
from tests import grad_clip_cases as cases
from tests import sgd_lr_cases as sgd
from tests.emul import build_emul

try:
    _EMUL = _lib.bind(ctypes.CDLL(build_emul.build()))
except FileNotFoundError:
    _EMUL = None

pytestmark = pytest.mark.skipif(_EMUL is None, reason="host emulation build unavailable")
CPU = torch.device("cpu")


def _sizes(gdt):
    return cases.sizes(_EMUL.cot_grad_norm_parts(), cases.vec(gdt)) if _EMUL is not None else []


def test_parts_is_the_header_constant():
    import os
    import re
    hdr = open(os.path.join(build_emul.ROOT, "include", "cotnet_amd.h")).read()
    assert _EMUL.cot_grad_norm_parts() == int(re.search(r"#define COT_GRAD_NORM_PARTS (\d+)", hdr).group(1))


@pytest.mark.parametrize("gdt,n", [(dt, n) for dt in cases.GRAD_DTYPES for n in _sizes(dt)],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_norm_coefficient_and_determinism(gdt, n):
    cases.check_norm(_EMUL, CPU, None, gdt, n)


@pytest.mark.parametrize("gdt", cases.GRAD_DTYPES, ids=cases.GRAD_IDS)
def test_zero_gradient(gdt):
    cases.check_zero_gradient(_EMUL, CPU, None, gdt)


@pytest.mark.parametrize("kind,gdt", [(k, dt) for k in cases.NONFINITE for dt in cases.GRAD_DTYPES
                                      if k != "bf16-overflowing-squares" or dt == torch.bfloat16],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_non_finite_gradients_skip(kind, gdt):
    cases.check_nonfinite(_EMUL, CPU, None, kind, gdt)


def test_several_buckets_share_one_norm():
    cases.check_several_buckets(_EMUL, CPU, None)


def test_counters_over_a_scripted_sequence():
    cases.check_counters(_EMUL, CPU, None)


@pytest.mark.parametrize("pdt,gdt", sgd.DTYPE_PAIRS, ids=sgd.PAIR_IDS)
@pytest.mark.parametrize("nesterov", [0, 1])
def test_sgd_behind_the_block_equals_todays_entry_points(pdt, gdt, nesterov):
    cases.check_sgd_clip(_EMUL, CPU, None, pdt, gdt, nesterov, sgd.SIZES)


def test_the_reference_fixture():
    cases.check_fixture(_EMUL, CPU, None)


def test_refusals_leave_everything_alone():
    cases.check_refusals(_EMUL, CPU, None)


# ---- FlatSGD

STEPS = 4
HP = dict(lr=0.1, momentum=0.9, weight_decay=4e-5, nesterov=True)


def _emulated(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: _EMUL)
    monkeypatch.setattr(_lib, "DEVICE_ONLY", False)


def _model(mixed):
    from cotnet_amd.flat_sgd import to_mixed_bf16
    torch.manual_seed(3)
    m = nn.Sequential(nn.Linear(8, 8), nn.BatchNorm1d(8)).train()  # a matrix, a bias and BatchNorm vectors: both decay groups
    return to_mixed_bf16(m) if mixed else m


def _opt(model, **kw):
    from cotnet_amd.flat_sgd import FlatSGD
    opt = FlatSGD(model, **HP, **kw)
    assert {b.key for b in opt.reducer.buckets} == {"decay", "no_decay"}
    return opt


def _inputs(mixed, scales=(1.0, 6.0, 0.5, 9.0)):
    """four (batch, loss scale) pairs: the gradients' size follows the loss scale (BatchNorm takes the input's scale out)"""
    g = torch.Generator().manual_seed(8)
    return [(torch.randn(4, 8, generator=g).to(torch.bfloat16 if mixed else torch.float32), s) for s in scales]


def _loss(model, xs):
    x, s = xs
    return s * model(x).float().square().mean()


def _step(model, opt, x):
    opt.zero_grad()
    _loss(model, x).backward()
    opt.step()


def _state(model, opt):
    out = [p.detach().clone() for p in model.parameters()]
    for st in opt.state:
        out += [st["mom"].clone()] + ([st["master"].clone()] if st["master"] is not None else [])
    return out


def _equal(a, b):
    return len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))


def _counted(monkeypatch, name):
    raw, calls = getattr(_EMUL, name), []

    def fn(*a):
        calls.append(a)
        return raw(*a)
    monkeypatch.setattr(_EMUL, name, fn)
    return calls


def _grad_norms(mixed):
    """the unclipped twin's gradient norm per step, to place clip_grad between them"""
    m = _model(mixed)
    opt = torch.optim.SGD(m.parameters(), lr=0.0)
    out = []
    for x in _inputs(mixed):
        opt.zero_grad()
        _loss(m, x).backward()
        out.append(float(torch.sqrt(sum(p.grad.double().square().sum() for p in m.parameters()))))
    return out


def test_fp32_net_follows_torch_sgd_behind_clip_grad_norm(monkeypatch):
    """tests/test_flat_sgd_gpu.py's fp32 bounds (rtol 2e-5, atol 2e-6) after four steps of which some clip and some do not"""
    _emulated(monkeypatch)
    norms = sorted(_grad_norms(False))
    clip = (norms[1] * norms[2]) ** 0.5  # between the second and the third: two steps clip (if the weights' drift keeps the order)
    ours, twin = _model(False), _model(False)
    opt = _opt(ours, clip_grad=clip)
    decay = [p for n, p in twin.named_parameters() if p.ndim > 1 and not n.endswith(".bias")]
    rest = [p for n, p in twin.named_parameters() if not (p.ndim > 1 and not n.endswith(".bias"))]
    ref = torch.optim.SGD([dict(params=decay, weight_decay=HP["weight_decay"]), dict(params=rest, weight_decay=0.0)], lr=HP["lr"],
                          momentum=HP["momentum"], nesterov=True)
    clipped = 0
    for i, x in enumerate(_inputs(False)):
        _step(ours, opt, x)
        ref.zero_grad()
        _loss(twin, x).backward()
        total = torch.nn.utils.clip_grad_norm_(twin.parameters(), clip)
        clipped += int(float(total) > clip)
        ref.step()
        s = opt.clip_stats()
        assert s["steps"] == i + 1 and s["clipped"] == clipped and s["skipped"] == 0 and s["skip"] == 0, s
        assert abs(s["total_norm"] - float(total)) <= 1e-5 * float(total), (s, float(total))
        for p, q in zip(ours.parameters(), twin.parameters()):
            assert torch.allclose(p, q, rtol=2e-5, atol=2e-6), f"step {i}"
    assert 0 < clipped < STEPS, clipped


def test_mixed_bf16_masters_follow_fp32_sgd_fed_the_scaled_gradient(monkeypatch):
    """the masters against fp32 SGD on `grad.float() * scale`, scale = the block's own (rtol 1e-5, atol 1e-6, test_flat_sgd_gpu.py's
    bounds for this form); torch's clip_grad_norm_ would round the scaled bf16 gradients a second time"""
    _emulated(monkeypatch)
    norms = sorted(_grad_norms(True))
    clip = (norms[1] * norms[2]) ** 0.5
    model = _model(True)
    opt = _opt(model, clip_grad=clip)
    masters = opt.master_parameters()
    ref = {p: masters[p].clone() for p in model.parameters()}
    mom = {p: torch.zeros_like(ref[p]) for p in ref}
    wd = {p: (HP["weight_decay"] if b.key == "decay" else 0.0) for b in opt.reducer.buckets for p in b.params}
    for i, x in enumerate(_inputs(True)):
        opt.zero_grad()
        _loss(model, x).backward()
        grads = {p: opt.reducer.reduced(b)[off:off + p.numel()].clone()  # (the gradients live in the buckets: no .grad)
                 for b in opt.reducer.buckets for p, off in zip(b.params, b.offs)}
        opt.step()
        s = opt.clip_stats()
        want = torch.sqrt(sum(g.double().square().sum() for g in grads.values()))
        assert abs(s["total_norm"] - float(want)) <= 2e-6 * float(want)
        scale = torch.tensor(s["scale"], dtype=torch.float32)
        for p in ref:
            g = grads[p].view_as(p).float() * scale + wd[p] * ref[p]
            mom[p] = HP["momentum"] * mom[p] + g
            ref[p] = ref[p] - HP["lr"] * (g + HP["momentum"] * mom[p])
            assert torch.allclose(opt.master_parameters()[p], ref[p], rtol=1e-5, atol=1e-6), f"step {i}"
            assert torch.equal(p.detach(), opt.master_parameters()[p].to(p.dtype))
    s = opt.clip_stats()
    assert 0 < s["clipped"] < STEPS and s["steps"] == STEPS, s


@pytest.mark.parametrize("mixed", [True, False], ids=["mixed-bf16", "fp32"])
@pytest.mark.parametrize("device_lr", [False, True])
def test_the_guard_alone_is_bit_equal_to_the_plain_optimizer(mixed, device_lr, monkeypatch):
    _emulated(monkeypatch)
    base = _model(mixed)
    plain_m, guard_m = copy.deepcopy(base), copy.deepcopy(base)
    plain, guard = _opt(plain_m, device_lr=device_lr), _opt(guard_m, device_lr=device_lr, skip_nonfinite=True)
    assert guard.clip_grad is None and guard.clip_state is not None
    for i, x in enumerate(_inputs(mixed)):
        for o in (plain, guard):
            o.set_lr(0.1 / (i + 1))
        _step(plain_m, plain, x)
        _step(guard_m, guard, x)
        assert _equal(_state(plain_m, plain), _state(guard_m, guard)), f"step {i}"
    s = guard.clip_stats()
    assert (s["steps"], s["clipped"], s["skipped"], s["scale"]) == (STEPS, 0, 0, 1.0), s


@pytest.mark.parametrize("kw", [dict(skip_nonfinite=True), dict(clip_grad=0.5), dict(clip_grad=0.5, device_lr=True)],
                         ids=["guard", "clip", "clip-device-lr"])
def test_a_nan_gradient_skips_the_step_and_the_ema_still_moves(kw, monkeypatch):
    _emulated(monkeypatch)
    model = _model(True)
    opt = _opt(model, ema_decay=0.9, **kw)
    xs = _inputs(True)
    _step(model, opt, xs[0])
    before = _state(model, opt)
    ema0 = [st["ema"].clone() for st in opt.state]
    opt.zero_grad()
    _loss(model, xs[1]).backward()
    bucket = opt.reducer.reduced(opt.reducer.buckets[-1])
    bucket[bucket.numel() // 2] = float("nan")  # one NaN in ONE bucket: every bucket is skipped
    opt.step()
    s = opt.clip_stats()
    assert (s["skip"], s["scale"], s["steps"], s["skipped"]) == (1, 0.0, 2, 1), s
    assert _equal(before, _state(model, opt)), "a skipped step wrote parameters, masters or momentum"
    assert all(not torch.equal(st["ema"], e) for st, e in zip(opt.state, ema0)), "the EMA did not move on the skipped step"
    assert all(bool(torch.isfinite(t).all()) for t in _state(model, opt))
    _step(model, opt, xs[2])  # the next step trains again
    s = opt.clip_stats()
    assert (s["skip"], s["steps"], s["skipped"]) == (0, 3, 1) and not _equal(before, _state(model, opt)), s


def test_default_arguments_allocate_nothing_and_launch_the_old_entry_points(monkeypatch):
    _emulated(monkeypatch)
    names = ("cot_sgd_step", "cot_sgd_step_lr", "cot_sgd_step_clip", "cot_grad_sumsq", "cot_grad_clip_finish")
    for kw, used in ((dict(), "cot_sgd_step"), (dict(device_lr=True), "cot_sgd_step_lr"), (dict(clip_grad=None), "cot_sgd_step"),
                     (dict(clip_grad=0.0), "cot_sgd_step"), (dict(clip_grad=-1.0), "cot_sgd_step")):
        with monkeypatch.context() as mp:
            calls = {n: _counted(mp, n) for n in names}
            model = _model(True)
            opt = _opt(model, **kw)
            assert opt.clip_state is None and opt._clip_parts is None and opt.clip_grad is None
            for x in _inputs(True)[:2]:
                _step(model, opt, x)
            n = 2 * len(opt.reducer.buckets)
            assert {k: len(v) for k, v in calls.items()} == {k: (n if k == used else 0) for k in names}, kw
            with pytest.raises(RuntimeError, match="neither"):
                opt.clip_stats()


@pytest.mark.parametrize("device_lr", [False, True])
def test_launches_and_addresses_with_clipping(device_lr, monkeypatch):
    """per step: one cot_grad_sumsq per bucket into consecutive slices of one partials tensor, one finish over all of them, one
    cot_sgd_step_clip per bucket reading the one block; a capture with the rate by value still records it"""
    _emulated(monkeypatch)
    model = _model(True)
    opt = _opt(model, clip_grad=1.0, device_lr=device_lr)
    parts = _EMUL.cot_grad_norm_parts()
    nb = len(opt.reducer.buckets)
    assert opt.clip_state.dtype == torch.int32 and opt.clip_state.shape == (8,) and not bool(opt.clip_state.any())
    assert opt._clip_parts.dtype == torch.float32 and opt._clip_parts.numel() == nb * parts
    addr = (opt.clip_state.data_ptr(), opt._clip_parts.data_ptr())
    names = ("cot_sgd_step", "cot_sgd_step_lr", "cot_sgd_step_clip", "cot_grad_sumsq", "cot_grad_clip_finish")
    calls = {n: _counted(monkeypatch, n) for n in names}
    xs = _inputs(True)
    _step(model, opt, xs[0])
    monkeypatch.setattr(_lib, "capturing", lambda: True)
    opt.lr = 0.05
    _step(model, opt, xs[1])
    with pytest.raises(RuntimeError, match="capture"):
        opt.clip_stats()
    monkeypatch.setattr(_lib, "capturing", lambda: False)
    assert opt._captured_lr == (None if device_lr else 0.05)
    assert {k: len(v) for k, v in calls.items()} == dict(cot_sgd_step=0, cot_sgd_step_lr=0, cot_sgd_step_clip=2 * nb,
                                                         cot_grad_sumsq=2 * nb, cot_grad_clip_finish=2)
    assert [a[3] for a in calls["cot_grad_sumsq"]] == [addr[1] + 4 * parts * i for i in range(nb)] * 2
    reduced = [opt.reducer.reduced(b) for b in opt.reducer.buckets]
    assert [(a[0], a[1]) for a in calls["cot_grad_sumsq"]] == [(g.data_ptr(), g.numel()) for g in reduced] * 2
    assert all(a[0] == addr[1] and a[1] == nb * parts and a[2] == 1.0 and a[3] == addr[0] for a in calls["cot_grad_clip_finish"])
    assert all(a[7] == addr[0] and a[6] == (opt.lr_dev.data_ptr() if device_lr else None) for a in calls["cot_sgd_step_clip"])
    assert (opt.clip_state.data_ptr(), opt._clip_parts.data_ptr()) == addr
    assert opt.clip_stats()["steps"] == 2
