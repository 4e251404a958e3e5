"""cot_sgd_step_lr (the rate read from device memory) against cot_sgd_step (the rate by value) on cloned operands: what
tests/test_sgd_device_lr_emulated.py runs on the host emulator and tests/test_sgd_device_lr_gpu.py on the device.

Same expression on the same fp32 rate, so `param`, `master` and `mom` must come out EQUAL (torch.equal, no tolerance).  Every operand
is a view into a buffer with NaN margins on both sides, which must stay NaN; the rate tensor must be left as it was."""
import ctypes

import torch

from cotnet_amd import _lib

DTYPE_PAIRS = [(torch.bfloat16, torch.bfloat16), (torch.bfloat16, torch.float32),
               (torch.float32, torch.float32), (torch.float32, torch.bfloat16)]  # (param, grad): what sgd_flat dispatches
PAIR_IDS = ["bf16-bf16", "bf16-f32", "f32-f32", "f32-bf16"]
SIZES = [1, 3, 4, 5, 4 * 1000 + 3]  # V = 4: tail only (1, 3), body only (4), body + tail (5, 4003)
# the last one is a double that is no fp32 value: both forms must see the SAME rounding of it (ctypes' c_float, torch's fp32 tensor)
RATES = [0.1, 0.0, 1e-5, 0.24987413835233163]
MARGIN = 8  # elements on each side: 16 B of bf16, 32 B of fp32 -- the views keep the 16-byte alignment the entry points ask for
MU, WD, GS = 0.9, 1e-2, 0.5


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def margined(values):
    """(buffer, view): `values` inside NaN margins"""
    n = values.numel()
    buf = torch.full((n + 2 * MARGIN,), float("nan"), dtype=values.dtype, device=values.device)
    view = buf[MARGIN:MARGIN + n]
    view.copy_(values)
    assert view.data_ptr() % 16 == 0
    return buf, view


def margins_intact(buf):
    return bool(torch.isnan(buf[:MARGIN]).all()) and bool(torch.isnan(buf[-MARGIN:]).all())


def operands(pdt, gdt, n, dev, seed=4):
    """{name: (buffer, view)} -- master is None for fp32 parameters"""
    g = torch.Generator().manual_seed(seed + n)
    master = torch.randn(n, generator=g)
    mom = torch.randn(n, generator=g) * 0.1
    grad = torch.randn(n, generator=g).to(gdt)
    ops = {"param": margined(master.to(pdt).to(dev)), "mom": margined(mom.to(dev)), "grad": margined(grad.to(dev)),
           "master": margined(master.to(dev)) if pdt != torch.float32 else None}
    return ops


def clone_ops(ops):
    out = {}
    for k, v in ops.items():
        if v is None:
            out[k] = None
        else:
            buf = v[0].clone()
            out[k] = (buf, buf[MARGIN:MARGIN + v[1].numel()])
    return out


def call(L, entry, ops, n, rate, nesterov, pdt, gdt, stream, momentum=MU, wd=WD, gs=GS):
    """rate: a Python float for cot_sgd_step, a pointer (or None) for cot_sgd_step_lr; returns the status"""
    v = {k: (x[1] if x is not None else None) for k, x in ops.items()}
    return getattr(L, entry)(P(v["param"]), P(v["master"]), P(v["mom"]), P(v["grad"]), n, rate, momentum, wd, gs, nesterov,
                             _lib.dtype_code(pdt), _lib.dtype_code(gdt), stream)


def same_bits(a, b):
    """equality of two buffers that hold NaN margins: compared as integers"""
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return torch.equal(a.view(it), b.view(it))


def compare_entry_points(L, dev, stream, pdt, gdt, nesterov, sizes, sync=lambda: None):
    for n in sizes:
        base = operands(pdt, gdt, n, dev)
        for lr in RATES:
            by_value, by_dev = clone_ops(base), clone_ops(base)
            rate = torch.tensor([lr], dtype=torch.float32).to(dev)  # the double reaches the device through an fp32 tensor
            rate0 = rate.clone()
            assert call(L, "cot_sgd_step", by_value, n, lr, nesterov, pdt, gdt, stream) == 0, L.cot_last_error()
            assert call(L, "cot_sgd_step_lr", by_dev, n, P(rate), nesterov, pdt, gdt, stream) == 0, L.cot_last_error()
            sync()
            what = f"n = {n}, lr = {lr!r}"
            for k in ("param", "master", "mom"):
                if base[k] is None:
                    continue
                assert torch.equal(by_value[k][1], by_dev[k][1]), f"{k} differs between the two entry points ({what})"
                assert margins_intact(by_dev[k][0]) and margins_intact(by_value[k][0]), f"{k}: a NaN margin was written ({what})"
            assert same_bits(by_dev["grad"][0], base["grad"][0]), f"the gradient was written ({what})"
            assert torch.equal(rate, rate0), f"the rate was written ({what})"
            if lr != 0.0:
                k = "master" if base["master"] is not None else "param"  # (1e-5 is below a bf16 working copy's rounding)
                assert not torch.equal(by_dev[k][1], base[k][1]), f"the step moved nothing ({what})"
