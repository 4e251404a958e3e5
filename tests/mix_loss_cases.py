"""cot_mix_normalize and cot_soft_target_ce_* through the C ABI against the reference's own results (tests/golden/recipe_mix.npz, written by
tests/golden/make_golden_recipe.py): what tests/test_mix_loss_emulated.py runs on the host emulator and tests/test_mix_loss_gpu.py on the device.

Mixing: the reference's collate gives the mixed uint8 batch; the kernel's output must equal normalize_uint8's arithmetic applied to it --
fp32 bit for bit, bf16 / fp16 the same rule rounded once.  Every output sits inside NaN margins that must stay NaN.

Loss: compared with the reference evaluated in fp64.  The allowance is MEASURED, not chosen: the error of the reference's own fp32 evaluation
against its fp64 evaluation on the same inputs (both in the fixture), times 4 -- the margin for another summation order over K terms.  It is
taken per quantity: the mean loss against 4 x the error of the reference's fp32 mean, the row losses (an extra check: the reference returns
only the mean) against 4 x the largest error of its fp32 rows, the gradient against 4 x its largest element-wise error.  Where the
reference's fp32 mean happens to be the nearest fp32 to the fp64 value, the first of these is a fraction of an ulp: only the nearest fp32
passes, which is what the kernels return (the mean is formed in fp64 and rounded once).
"""
import ctypes
import json

import numpy as np
import torch

from cotnet_amd import _lib
from cotnet_amd.mixup import pack_params
from tests.conftest import load_golden

GOLD = load_golden("recipe_mix")
META = json.loads(str(GOLD["meta"]))
CASES = sorted(META)
MARGIN = 64  # elements of NaN on each side of an output (keeps 16-byte alignment for every dtype)
MEAN = torch.tensor([123.675, 116.28, 103.53])
STD = torch.tensor([58.395, 57.12, 57.375])
FACTOR = 4.0


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def gold(name, key):
    return torch.from_numpy(GOLD[f"{name}__{key}"])


def mode_of(meta):
    return 0 if meta["lam"] == 1.0 else (2 if meta["use_cutmix"] else 1)


def block_of(meta, dev):
    return pack_params(mode_of(meta), meta["lam"], meta["box"]).to(dev)


def margined(shape, dtype, dev):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * MARGIN,), float("nan"), dtype=dtype, device=dev)
    view = buf[MARGIN:MARGIN + n].view(shape)
    assert view.data_ptr() % 16 == 0
    return buf, view


def margins_intact(buf):
    return bool(torch.isnan(buf[:MARGIN]).all()) and bool(torch.isnan(buf[-MARGIN:]).all())


def normalized(u8, dtype):
    """normalize_uint8's arithmetic on the CPU (tests/test_kernels_emulated.py::test_input_normalize_...): the reference loader's"""
    C = u8.shape[1]
    if dtype == torch.float16:
        return u8.half().sub_(MEAN.half().view(1, C, 1, 1)).div_(STD.half().view(1, C, 1, 1))
    return u8.float().sub_(MEAN.view(1, C, 1, 1)).div_(STD.view(1, C, 1, 1)).to(dtype)


def mix(L, dev, stream, x, blk, dtype, sync=lambda: None):
    """-> (status, output on the CPU, margins intact)"""
    m, sd = (MEAN.half().float(), STD.half().float()) if dtype == torch.float16 else (MEAN, STD)
    m, sd, xd = m.to(dev), sd.to(dev), x.to(dev)
    buf, y = margined(tuple(x.shape), dtype, dev)
    N, C, H, W = x.shape
    rc = L.cot_mix_normalize(P(xd), P(y), P(m), P(sd), P(blk), N, C, H, W, _lib.dtype_code(dtype), stream)
    sync()
    assert torch.equal(xd.cpu(), x), "the input was written"
    return rc, y.cpu(), margins_intact(buf)


def check_mix_case(L, dev, stream, name, sync=lambda: None):
    meta = META[name]
    x, mixed = gold(name, "x"), gold(name, "mixed")
    blk = block_of(meta, dev)
    if mode_of(meta):
        assert not torch.equal(x, mixed)  # (the reference did mix this batch)
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        rc, y, intact = mix(L, dev, stream, x, blk, dtype, sync)
        assert rc == 0, L.cot_last_error()
        assert intact, f"{name} {dtype}: a NaN margin was written"
        assert torch.equal(y, normalized(mixed, dtype)), f"{name} {dtype}: differs from the reference's mixed batch, normalised"
    # the same input under `mode 0`: cot_input_normalize's result
    rc, y, intact = mix(L, dev, stream, x, pack_params(0, 1.).to(dev), torch.float32, sync)
    assert rc == 0 and intact and torch.equal(y, normalized(x, torch.float32))


def check_mix_refusals(L, dev):
    x = torch.zeros(3, 3, 16, 32, dtype=torch.uint8, device=dev)
    buf, y = margined((3, 3, 16, 32), torch.float32, dev)
    blk, m, sd = pack_params(1, 0.5).to(dev), MEAN.to(dev), STD.to(dev)
    f32 = _lib.dtype_code(torch.float32)
    assert L.cot_mix_normalize(P(x), P(y), P(m), P(sd), P(blk), 3, 3, 16, 32, f32, None) == -1  # odd N
    assert b"odd" in L.cot_last_error()
    assert L.cot_mix_normalize(P(x), P(y), P(m), P(sd), None, 2, 3, 16, 32, f32, None) == -1 and b"params" in L.cot_last_error()
    assert L.cot_mix_normalize(None, P(y), P(m), P(sd), P(blk), 2, 3, 16, 32, f32, None) == -1
    assert L.cot_mix_normalize(P(x), P(y), P(m), P(sd), P(blk), 2, 3, 16, 32, 1, None) == _lib.COT_ERR_UNSUPPORTED  # fp64 output
    assert L.cot_mix_normalize(P(x), P(y), P(m), P(sd), P(blk), 2, 0, 16, 32, f32, None) == -1
    u8 = torch.zeros(4096, dtype=torch.uint8, device=dev)  # y inside x's bytes
    assert L.cot_mix_normalize(P(u8), P(u8[16:]), P(m), P(sd), P(blk), 2, 1, 4, 4, _lib.dtype_code(torch.bfloat16), None) == -1
    assert b"overlaps" in L.cot_last_error()
    logits = torch.zeros(2, 10, device=dev)
    lab = torch.zeros(2, dtype=torch.int64, device=dev)
    out = torch.zeros(8, device=dev)
    fwd = lambda *a: L.cot_soft_target_ce_forward(*a)  # noqa: E731
    assert fwd(P(logits), P(lab), P(blk), 0.1, P(out), P(out[2:]), P(out[4:]), 2, 0, f32, None) == -1  # K < 1
    assert fwd(P(logits), P(lab), P(blk), 1.0, P(out), P(out[2:]), P(out[4:]), 2, 10, f32, None) == -1 and b"smoothing" in L.cot_last_error()
    assert fwd(P(logits), P(lab), P(blk), -0.1, P(out), P(out[2:]), P(out[4:]), 2, 10, f32, None) == -1
    assert fwd(P(logits), P(lab), None, 0.1, P(out), P(out[2:]), P(out[4:]), 2, 10, f32, None) == -1
    assert fwd(P(logits), None, P(blk), 0.1, P(out), P(out[2:]), P(out[4:]), 2, 10, f32, None) == -1
    assert fwd(P(logits), P(lab), P(blk), 0.1, P(out), P(out[2:]), P(out[4:]), 2, 10, _lib.dtype_code(torch.float16), None) == _lib.COT_ERR_UNSUPPORTED
    assert L.cot_soft_target_ce_backward(P(logits), P(lab), P(blk), 0.1, P(out), None, P(logits), 2, 10, f32, None) == -1
    assert b"grad_out" in L.cot_last_error()
    assert margins_intact(buf) and not out.any()


def loss(L, dev, stream, logits, labels, blk, smoothing, g=1.0, sync=lambda: None):
    """forward and backward through the C ABI -> dict of CPU tensors (mean, rows, lse, grad); every output inside NaN margins"""
    N, K = logits.shape
    x, lab, blk = logits.to(dev).contiguous(), labels.to(dev), blk.to(dev)
    bufs = {k: margined(s, dt, dev) for k, (s, dt) in dict(rows=((N,), torch.float32), lse=((4 * N,), torch.float32),
                                                          mean=((1,), torch.float32), grad=((N, K), logits.dtype)).items()}
    gd = torch.tensor([g], dtype=torch.float32, device=dev)
    dt = _lib.dtype_code(logits.dtype)
    rc = L.cot_soft_target_ce_forward(P(x), P(lab), P(blk), smoothing, P(bufs["rows"][1]), P(bufs["lse"][1]), P(bufs["mean"][1]), N, K, dt,
                                      stream)
    assert rc == 0, L.cot_last_error()
    rc = L.cot_soft_target_ce_backward(P(x), P(lab), P(blk), smoothing, P(bufs["lse"][1]), P(gd), P(bufs["grad"][1]), N, K, dt, stream)
    assert rc == 0, L.cot_last_error()
    sync()
    assert all(margins_intact(b) for b, _ in bufs.values()), "a NaN margin was written"
    assert torch.equal(x.cpu(), logits) and torch.equal(lab.cpu(), labels), "an input was written"
    return {k: v.cpu().clone() for k, (_, v) in bufs.items()}


def allowances(mean32, rows32, grad32, mean64, rows64, grad64):
    """(mean, rows, gradient): FACTOR x the fp32 evaluation's own error against the fp64 one, per quantity (module docstring)"""
    return (FACTOR * abs(float(mean32) - float(mean64)), FACTOR * float((rows32.double() - rows64).abs().max()),
            FACTOR * float((grad32.double() - grad64).abs().max()))


def compare(got, mean64, rows64, grad64, allow, what):
    a_mean, a_rows, a_grad = allow
    e_mean = abs(float(got["mean"]) - float(mean64))
    e_rows = float((got["rows"].double() - rows64).abs().max())
    e_grad = float((got["grad"].double() - grad64).abs().max())
    print(f"{what}: mean loss error {e_mean:.3e} (allowance {a_mean:.3e}); row loss error {e_rows:.3e} (allowance {a_rows:.3e}); "
          f"gradient error {e_grad:.3e} (allowance {a_grad:.3e})")
    assert e_mean <= a_mean, f"{what}: mean loss error {e_mean:.3e} over the allowance {a_mean:.3e}"
    assert e_rows <= a_rows, f"{what}: row loss error {e_rows:.3e} over the allowance {a_rows:.3e}"
    assert e_grad <= a_grad, f"{what}: gradient error {e_grad:.3e} over the allowance {a_grad:.3e}"


def fixture_refs(name, tag):
    f = lambda k: gold(name, f"{tag}_{k}")  # noqa: E731
    return (f("loss_f32"), f("rows_f32"), f("grad_f32")), (f("loss_f64"), f("rows_f64"), f("grad_f64"))


def check_soft_case(L, dev, stream, name, sync=lambda: None):
    """the mixed, smoothed target of the reference's collate (never materialised here) and SoftTargetCrossEntropy"""
    meta = META[name]
    r32, r64 = fixture_refs(name, "soft")
    got = loss(L, dev, stream, gold(name, "logits"), gold(name, "labels"), block_of(meta, dev), meta["kwargs"]["label_smoothing"], sync=sync)
    compare(got, *r64, allowances(*r32, *r64), f"{name} soft target")
    again = loss(L, dev, stream, gold(name, "logits"), gold(name, "labels"), block_of(meta, dev), meta["kwargs"]["label_smoothing"], sync=sync)
    assert all(torch.equal(got[k], again[k]) for k in got), f"{name}: two runs differ"
    # the upstream gradient is read from the device and scales the result
    half = loss(L, dev, stream, gold(name, "logits"), gold(name, "labels"), block_of(meta, dev), meta["kwargs"]["label_smoothing"], g=0.5,
                sync=sync)
    assert torch.equal(half["grad"], got["grad"] * 0.5)


def check_label_smoothing_case(L, dev, stream, name, sync=lambda: None):
    """`mode 0, lam 1`, smoothing 0.1: the reference's LabelSmoothingCrossEntropy(0.1) on the hard labels"""
    r32, r64 = fixture_refs(name, "ls")
    got = loss(L, dev, stream, gold(name, "logits"), gold(name, "labels"), pack_params(0, 1.), 0.1, sync=sync)
    compare(got, *r64, allowances(*r32, *r64), f"{name} label smoothing")


def torch_ce(logits, labels, dtype):
    x = logits.detach().clone().to(dtype).requires_grad_(True)
    rows = torch.nn.functional.cross_entropy(x, labels, reduction="none")
    mean = torch.nn.functional.cross_entropy(x, labels)
    mean.backward()
    return mean.detach(), rows.detach(), x.grad


def check_plain_ce_case(L, dev, stream, name, sync=lambda: None):
    """`mode 0`, smoothing 0: F.cross_entropy"""
    logits, labels = gold(name, "logits"), gold(name, "labels")
    got = loss(L, dev, stream, logits, labels, pack_params(0, 1.), 0.0, sync=sync)
    r32, r64 = torch_ce(logits, labels, torch.float32), torch_ce(logits, labels, torch.float64)
    compare(got, *r64, allowances(*r32, *r64), f"{name} plain cross entropy")


def bf16_order(t):
    """bf16 values as integers in value order: neighbours differ by one"""
    b = t.view(torch.int16).to(torch.int32)
    return torch.where(b < 0, -(b & 0x7FFF), b)


def check_bf16_grad(got_grad, grad64, what):
    """within 1 bf16 ulp, element-wise, of the fp64 gradient rounded to bf16; the share that differs at all is printed, not capped"""
    want = grad64.to(torch.bfloat16)
    d = (bf16_order(got_grad) - bf16_order(want)).abs()
    print(f"{what}: bf16 gradient, {float((d > 0).float().mean()):.4%} of {d.numel()} elements differ from the rounded fp64 gradient, "
          f"largest distance {int(d.max())} ulp")
    assert int(d.max()) <= 1, f"{what}: {int((d > 1).sum())} elements further than 1 bf16 ulp"
    return float((d > 0).float().mean())


def check_bf16_case(L, dev, stream, name, sync=lambda: None):
    meta = META[name]
    logits = gold(name, "logits").bfloat16()
    got = loss(L, dev, stream, logits, gold(name, "labels"), block_of(meta, dev), meta["kwargs"]["label_smoothing"], sync=sync)
    assert got["grad"].dtype == torch.bfloat16
    return check_bf16_grad(got["grad"], gold(name, "soft_grad_bf16_f64"), name)


def out_of_range_labels(L, dev, stream, sync=lambda: None):
    """a label outside [0, K) matches no column: every target entry of that row is `off`, nothing outside the buffers is touched"""
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(2, 37, generator=g)
    got = loss(L, dev, stream, logits, torch.tensor([2 ** 40, -7]), pack_params(1, 0.3), 0.1, sync=sync)
    off = 0.1 / 37
    want = -(off * (0.3 + 0.7)) * torch.log_softmax(logits.double(), -1).sum(-1)
    # 37 fp32 products and additions, each within 2^-24 relative, all of one sign apart from logp's own rounding: far inside 1e-5
    assert torch.allclose(got["rows"].double(), want, rtol=1e-5, atol=0)
