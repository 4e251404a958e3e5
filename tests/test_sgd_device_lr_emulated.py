"""The learning rate of the fused SGD step read from device memory (cot_sgd_step_lr, FlatSGD(device_lr=True)) -- on the host emulator.

What a HIP graph needs from it is checked on the device (tests/test_sgd_device_lr_gpu.py); here: the new entry point against the
by-value one bit for bit, against the formula in fp32 torch, its refusals, and FlatSGD's two forms stepped side by side over a
schedule, with `_lib.capturing` forced to emulate a capture."""
import copy
import ctypes

import pytest
import torch
from torch import nn

from cotnet_amd import _lib
from cotnet_amd.lr_schedule import CosineSchedule
from tests import sgd_lr_cases as cases
from tests.emul import build_emul

try:
    _EMUL = _lib.bind(ctypes.CDLL(build_emul.build()))
except FileNotFoundError:
    _EMUL = None

pytestmark = pytest.mark.skipif(_EMUL is None, reason="host emulation build unavailable")
P = cases.P
CPU = torch.device("cpu")


@pytest.mark.parametrize("pdt,gdt", cases.DTYPE_PAIRS, ids=cases.PAIR_IDS)
@pytest.mark.parametrize("nesterov", [0, 1])
def test_rate_from_memory_equals_rate_by_value(pdt, gdt, nesterov):
    cases.compare_entry_points(_EMUL, CPU, None, pdt, gdt, nesterov, cases.SIZES)


@pytest.mark.parametrize("pdt,gdt", cases.DTYPE_PAIRS, ids=cases.PAIR_IDS)
@pytest.mark.parametrize("nesterov", [0, 1])
@pytest.mark.parametrize("lr", [0.1, 0.24987413835233163])
def test_rate_from_memory_matches_torch_formula(pdt, gdt, nesterov, lr):
    """independent of cot_sgd_step: the formula in fp32 torch, with test_fused_sgd_kernel_matches_torch_formula's bounds for this
    arithmetic (rtol 1e-6, atol 1e-7)"""
    n = 4 * 1000 + 3
    ops = cases.operands(pdt, gdt, n, CPU)
    p0 = (ops["master"] if ops["master"] is not None else ops["param"])[1].clone()
    mom0, grad = ops["mom"][1].clone(), ops["grad"][1].clone()
    rate = torch.tensor([lr], dtype=torch.float32)
    gg = grad.float() * cases.GS + cases.WD * p0
    buf = cases.MU * mom0 + gg
    ref_p = p0 - rate * (gg + cases.MU * buf if nesterov else buf)
    assert cases.call(_EMUL, "cot_sgd_step_lr", ops, n, P(rate), nesterov, pdt, gdt, None) == 0, _EMUL.cot_last_error()
    assert torch.allclose(ops["mom"][1], buf, rtol=1e-6, atol=1e-7)
    if ops["master"] is not None:
        assert torch.allclose(ops["master"][1], ref_p, rtol=1e-6, atol=1e-7)
        assert torch.equal(ops["param"][1], ops["master"][1].to(pdt))
    else:
        assert torch.allclose(ops["param"][1], ref_p, rtol=1e-6, atol=1e-7)
    assert all(cases.margins_intact(v[0]) for v in ops.values() if v is not None)


def test_refusals_leave_the_operands_alone():
    pdt = gdt = torch.bfloat16
    n = 37
    ops = cases.operands(pdt, gdt, n, CPU)
    keep = cases.clone_ops(ops)
    rate = torch.tensor([0.1, 0.2], dtype=torch.float32)

    def untouched():
        return all(cases.same_bits(ops[k][0], keep[k][0]) for k in ops) and rate.tolist() == torch.tensor([0.1, 0.2]).tolist()

    assert cases.call(_EMUL, "cot_sgd_step_lr", ops, n, None, 1, pdt, gdt, None) == -1  # COT_ERR_INVALID_ARG
    assert b"lr_dev" in _EMUL.cot_last_error() and untouched()
    odd = ctypes.c_void_p(rate.data_ptr() + 2)
    assert cases.call(_EMUL, "cot_sgd_step_lr", ops, n, odd, 1, pdt, gdt, None) == -1
    assert b"4-byte aligned" in _EMUL.cot_last_error() and untouched()
    # the 16-byte rule does not apply to the rate: the second float of the tensor is a valid place for it
    second = cases.clone_ops(ops)
    assert cases.call(_EMUL, "cot_sgd_step_lr", second, n, ctypes.c_void_p(rate.data_ptr() + 4), 1, pdt, gdt, None) == 0
    assert not torch.equal(second["master"][1], keep["master"][1]) and untouched()
    assert cases.call(_EMUL, "cot_sgd_step_lr", ops, n, P(rate), 1, torch.float16, gdt, None) == _lib.COT_ERR_UNSUPPORTED
    assert untouched()
    no_master = dict(ops, master=None)  # bf16 parameters without their fp32 master: no such kernel
    assert cases.call(_EMUL, "cot_sgd_step_lr", no_master, n, P(rate), 1, pdt, gdt, None) == _lib.COT_ERR_UNSUPPORTED
    assert untouched()
    assert cases.call(_EMUL, "cot_sgd_step_lr", ops, 0, P(rate), 1, pdt, gdt, None) == -1
    assert b"element count" in _EMUL.cot_last_error() and untouched()
    misaligned = dict(ops, mom=(ops["mom"][0], ops["mom"][1][1:]))  # the other pointers keep cot_sgd_step's 16-byte rule
    assert cases.call(_EMUL, "cot_sgd_step_lr", misaligned, n - 1, P(rate), 1, pdt, gdt, None) == -1
    assert b"16-byte" in _EMUL.cot_last_error() and untouched()


# ---- FlatSGD(device_lr=True) over a schedule

SCHED = CosineSchedule(0.1, 6, warmup_t=2, warmup_lr_init=1e-3, lr_min=1e-4)
STEPS = 6


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
    opt = FlatSGD(model, lr=SCHED.value(0), momentum=0.9, weight_decay=4e-5, nesterov=True, **kw)
    assert {b.key for b in opt.reducer.buckets} == {"decay", "no_decay"}
    return opt


def _inputs(mixed):
    g = torch.Generator().manual_seed(8)
    return [torch.randn(4, 8, generator=g).to(torch.bfloat16 if mixed else torch.float32) for _ in range(STEPS)]


def _step(model, opt, x):
    opt.zero_grad()
    model(x).float().square().mean().backward()
    opt.step()


def _state(model, opt):
    out = [p.detach().clone() for p in model.parameters()]
    for st in opt.state:
        out += [st["mom"].clone()] + ([st["master"].clone()] if st["master"] is not None else [])
    return out


def _equal(a, b):
    return len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))


def _counted(monkeypatch, name):
    """rebind an entry point on the emulator handle (the checked view looks it up there per call) and count its calls"""
    raw, calls = getattr(_EMUL, name), []

    def fn(*a):
        calls.append(a)
        return raw(*a)
    monkeypatch.setattr(_EMUL, name, fn)
    return calls


@pytest.mark.parametrize("mixed", [True, False], ids=["mixed-bf16", "fp32"])
def test_flat_sgd_with_a_device_rate_follows_the_schedule_like_the_by_value_form(mixed, monkeypatch):
    """three twins on the same inputs and the same set_lr calls: by value (the eager truth), device_lr, and device_lr with a capture
    emulated around step 2 -- parameters, masters and momentum equal after every step; after the 'capture' the device_lr twin
    still takes new rates, and nothing was baked"""
    _emulated(monkeypatch)
    base = _model(mixed)
    models = [copy.deepcopy(base) for _ in range(3)]
    by_value, by_dev, captured = _opt(models[0]), _opt(models[1], device_lr=True), _opt(models[2], device_lr=True)
    assert by_value.lr_dev is None and by_dev.lr_dev.dtype == torch.float32 and by_dev.lr_dev.shape == (1,)
    assert by_dev.lr_dev.item() == torch.tensor(SCHED.value(0), dtype=torch.float32).item()
    address = captured.lr_dev.data_ptr()
    rates = []
    for i, x in enumerate(_inputs(mixed)):
        for opt in (by_value, by_dev, captured):
            rates.append(SCHED.apply(opt, i))
        _step(models[0], by_value, x)
        _step(models[1], by_dev, x)
        if i == 2:
            monkeypatch.setattr(_lib, "capturing", lambda: True)
        _step(models[2], captured, x)
        monkeypatch.setattr(_lib, "capturing", lambda: False)
        want = _state(models[0], by_value)
        assert _equal(want, _state(models[1], by_dev)), f"device_lr differs from the by-value form after step {i}"
        assert _equal(want, _state(models[2], captured)), f"device_lr with an emulated capture differs after step {i}"
        assert captured._captured_lr is None and by_dev._captured_lr is None
        assert captured.lr == by_dev.lr == by_value.lr == SCHED.value(i)
        assert captured.lr_dev.item() == torch.tensor(SCHED.value(i), dtype=torch.float32).item()
    assert len(set(rates)) == STEPS  # every step at another rate
    assert captured.lr_dev.data_ptr() == address
    assert not _equal(_state(base, _opt(copy.deepcopy(base))), _state(models[0], by_value))  # (the steps did move the weights)


def test_set_lr_while_capturing_raises_and_changes_nothing(monkeypatch):
    _emulated(monkeypatch)
    model = _model(True)
    opt = _opt(model, device_lr=True)
    opt.set_lr(0.05)
    monkeypatch.setattr(_lib, "capturing", lambda: True)
    for _ in range(2):
        with pytest.raises(RuntimeError, match="set the rate outside the capture"):
            opt.set_lr(0.005)
        assert opt.lr == 0.05 and opt.lr_dev.item() == torch.tensor(0.05, dtype=torch.float32).item()
    _step(model, opt, _inputs(True)[0])  # a step may be captured
    monkeypatch.setattr(_lib, "capturing", lambda: False)
    opt.set_lr(0.005)
    assert opt.lr == 0.005 and opt.lr_dev.item() == torch.tensor(0.005, dtype=torch.float32).item() and opt._captured_lr is None


@pytest.mark.parametrize("device_lr", [False, True])
def test_one_sgd_launch_per_bucket_through_the_form_that_was_asked_for(device_lr, monkeypatch):
    _emulated(monkeypatch)
    model = _model(True)
    opt = _opt(model, device_lr=device_lr)
    by_value, by_dev = _counted(monkeypatch, "cot_sgd_step"), _counted(monkeypatch, "cot_sgd_step_lr")
    steps = 3
    for i, x in enumerate(_inputs(True)[:steps]):
        SCHED.apply(opt, i)
        _step(model, opt, x)
    n = len(opt.reducer.buckets) * steps
    assert n >= 2 * steps
    assert (len(by_value), len(by_dev)) == ((0, n) if device_lr else (n, 0))
    if device_lr:
        assert all(a[5] == opt.lr_dev.data_ptr() for a in by_dev)  # one address for the optimizer's lifetime
