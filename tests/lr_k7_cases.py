"""Shared cases of the 7x7 local relation (csrc/local_relation7.hip) through the C ABI: a window-parametrised runner and an fp64 checker of
their own (tests/test_fuzz_emulated.py's lr_run / lr_reference64 state nine taps).  Every function takes the library `E` (the host emulator or
libcotnet_hip.so) and the device the operands live on, so tests/test_lrnet_k7_emulated.py and tests/test_lrnet_k7_gpu.py run the same code.

Runner: q / k / v / gout / probs inside NaN margins, NaN-filled outputs inside NaN margins that must stay NaN, the workspace at exactly the
reported size, 0x7f-filled, with a guard behind it.  Checker: fp64 from unfold and einsum, differentiated by autograd; no code shared with
the product.

Tolerances are the 3x3 op's (tests/test_fuzz_emulated.py::lr_tolerances), not widened for 49 taps: tol f (1 + |want|) per element, tol = 2e-5
(fp32) / 4e-2 (bf16), f = 1 for out and gv, 4 for gq and gk; gpos within 4 tol max(1, max|want|).

Input scale: q and k are 0.5 x normal, pos = normal + normal, v and gout normal -- logits of a few units, the softmax neither flat nor
one-hot.  At this scale the reference's composition (local_relation_reference over the unfold oracle) evaluated in fp32 on the CPU stays
inside the fp32 bound against the fp64 checker on every directed input below; tests/test_lrnet_k7_cpu.py::
test_fp32_composition_stays_inside_the_fp32_bound asserts it and prints the worst ratio of each output to its bound (out 0.034, gq 0.067,
gk 0.030, gv 0.031, gpos 0.018), so the scale was left as at 3x3."""
import ctypes

import torch
import torch.nn.functional as F

from cotnet_amd import _lib

DTYPES = [torch.float32, torch.bfloat16]
STAGES = [(64, 56), (128, 56), (128, 28), (256, 28), (256, 14), (512, 14), (512, 7)]  # (C, H) of LR-Net-50's attention layers
FWD, BWD = "lr7_fwd", "lr7_bwd_agg+lr7_bwd_rel+lr7_gpos_reduce"

# (N, C, H, W): N = 2, C = 24 (G = 3 separates c mod G from c / 8) unless the row says otherwise
DIRECTED = [
    # planes smaller than the halo
    (2, 24, 1, 1), (2, 24, 2, 150), (2, 24, 3, 3), (2, 24, 7, 7),
    # every loader width: W odd, W % 4 == 2, W % 4 == 0
    (2, 24, 4, 5), (2, 24, 3, 9), (2, 24, 5, 6), (2, 24, 9, 30), (2, 24, 6, 12), (2, 24, 5, 28), (2, 24, 6, 56),
    # ragged last tile and multi-row tiles
    (2, 24, 5, 100), (2, 24, 3, 85), (2, 24, 40, 6),
    # one row per tile (W > 128: the two-pass form, four channels staged at a time)
    (2, 24, 3, 129), (2, 24, 2, 200),
    # one head, and eight
    (2, 8, 5, 12), (2, 8, 3, 9), (1, 64, 7, 7), (1, 64, 9, 30),
]


def case_id(c):
    return "x".join(str(i) for i in c)


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def geom(N, C, H, W, k=7, wC=None):
    return _lib.AggGeom(N, C, H, W, 1, C // 8 if wC is None else wC, k, k, 1, 1, k // 2, k // 2, 1, 1)


def lds_bytes(H, W):
    """the plan's LDS formula (lr7_plan): one lane per pixel, TR whole rows per tile, planes of W + 6 floats per row rounded up to an odd
    size; JC = 8 channels staged per pass where that fits 64 KiB, else 4 -> bytes at the JC chosen, or None where W > 256"""
    if W > 256:
        return None
    TR = max(1, min(H, 256 // W))
    full, rows = ((TR + 6) * (W + 6)) | 1, (TR * (W + 6)) | 1
    size = lambda JC: (2 * JC * full + 14 * rows + 256) * 4  # noqa: E731
    return size(8) if size(8) <= 64 * 1024 else size(4)


def fits(H, W):
    b = lds_bytes(H, W)
    return b is not None and b <= 64 * 1024


def boundary_width(H=3):
    """the widest W the plan accepts for one-row tiles, from the formula"""
    W = 129
    while fits(H, W + 1):
        W += 1
    assert fits(H, W) and not fits(H, W + 1) and all(fits(H, w) for w in range(129, W))
    return W


def nan_margined(t, margin):
    """a copy of `t` that sits inside a NaN-filled allocation (`margin` elements either side, 16-byte aligned start)"""
    lead = margin + (-margin) % 8
    flat = torch.full((t.numel() + 2 * lead + 8,), float("nan"), dtype=t.dtype, device=t.device)
    v = flat[lead:lead + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def margins_untouched(view):
    flat, lo = view._base, view.storage_offset()
    return flat[:lo].isnan().all().item() and flat[lo + view.numel():].isnan().all().item()


def inputs(N, C, H, W, dtype, seed, qs=0.5, ks=7, dev="cpu"):
    g = torch.Generator().manual_seed(seed)
    q, k, v, gout = (torch.randn(N, C, H, W, generator=g) for _ in range(4))
    pos = (torch.randn(C, ks, 1, generator=g) + torch.randn(C, 1, ks, generator=g)).reshape(C, ks * ks).contiguous()
    return [t.to(dev) for t in ((qs * q).to(dtype), (0.5 * k).to(dtype), v.to(dtype), gout.to(dtype), pos)]


def reference64(q, k, v, pos, gout, ks=7, dev="cpu"):
    """fp64, from unfold and einsum, differentiated by autograd (on the CPU; the large device cases pass dev = "cuda"), results on the CPU:
        logit[n,g,t,p] = sum_{j<8} q[n,8g+j,p] (uk[n,8g+j,t,p] + pos[8g+j,t])   uk = 0 outside the image: a padded tap keeps q * pos
        out[n,c,p]     = sum_t softmax_t(logit)[n, c mod G, t, p] v[n,c,p + off_t]
    -> (out, gq, gk, gv, gpos[C][ks ks], probs)"""
    N, C, H, W = q.shape
    G, T = C // 8, ks * ks
    q, k, v, pos = (t.detach().to(dev).double().requires_grad_(True) for t in (q, k, v, pos))
    uk = F.unfold(k, ks, 1, ks // 2, 1).view(N, G, 8, T, H, W)
    logit = torch.einsum("ngjhw,ngjthw->ngthw", q.view(N, G, 8, H, W), uk + pos.view(1, G, 8, T, 1, 1))
    a = torch.softmax(logit, 2)
    uv = F.unfold(v, ks, 1, ks // 2, 1).view(N, 8, G, T, H, W)  # channel c = g + j G takes head g = c mod G
    out = torch.einsum("ngthw,njgthw->njghw", a, uv).reshape(N, C, H, W)
    out.backward(gout.detach().to(dev).double())
    return tuple(t.cpu() for t in (out.detach(), q.grad, k.grad, v.grad, pos.grad, a.detach()))


def tolerances(dtype):
    return (2e-5 if dtype == torch.float32 else 4e-2), {"out": 1, "gv": 1, "gq": 4, "gk": 4}


def mismatches(got, want, dtype, report=None):
    """names of the outputs (out, gq, gk, gv, gpos) that are not finite or off the fp64 reference; `report` collects each output's worst
    ratio to its bound"""
    tol, factor = tolerances(dtype)
    bad = []
    for name, g, w in zip(("out", "gq", "gk", "gv"), got, want):
        g = g.detach().cpu()
        if not torch.isfinite(g).all().item():
            bad.append((name, "not finite"))
            continue
        err = (g.double() - w).abs()
        ratio = (err / (factor[name] * tol * (1 + w.abs()))).max().item()
        if report is not None:
            report[name] = max(report.get(name, 0.0), ratio)
        if not ratio <= 1:
            bad.append((name, err.max().item(), ratio))
    g, w = got[4].detach().cpu(), want[4]
    err = (g.double() - w).abs().max().item()
    ratio = err / (4 * tol * max(1.0, w.abs().max().item()))
    if report is not None:
        report["gpos"] = max(report.get("gpos", 0.0), ratio)
    if not torch.isfinite(g).all().item() or not ratio <= 1:
        bad.append(("gpos", err, ratio))
    return bad


def run(E, q, k, v, gout, pos, ks=7, null_probs=True, margin=None):
    """forward + backward through the C ABI of `E` on the operands' device -> ((out, gq, gk, gv, gpos), probs)"""
    N, C, H, W = q.shape
    T = ks * ks
    g, dt, dev = geom(N, C, H, W, ks), _lib.dtype_code(q.dtype), q.device
    margin = ks // 2 * (W + 1) + 1 if margin is None else margin  # a whole halo's reach before the first / after the last element
    q, k, v, gout = (nan_margined(t, margin) for t in (q, k, v, gout))
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=q.dtype, device=dev)  # noqa: E731
    plane = lambda: nan_margined(nan(N, C, H, W), 256 + margin)  # noqa: E731
    probs, out = nan_margined(nan(N, 1, C // 8, T, H, W), 256 + margin), plane()
    assert E.cot_local_relation_forward(P(q), P(k), P(v), P(pos), P(out), P(probs), ctypes.byref(g), dt, None) == 0, E.cot_last_error()
    assert E.cot_last_kernel().decode() == FWD
    if null_probs:  # the branch that stores no probabilities: the same bits in out
        out2 = plane()
        assert E.cot_local_relation_forward(P(q), P(k), P(v), P(pos), P(out2), None, ctypes.byref(g), dt, None) == 0, E.cot_last_error()
        assert torch.isfinite(out).all().item() and torch.equal(out, out2), "probs == NULL changes out"
        assert margins_untouched(out2), "write outside out (probs == NULL)"
    nb = int(E.cot_local_relation_workspace_bytes(ctypes.byref(g), dt))
    assert nb > 0, nb
    buf = torch.full((nb + 256,), 0x7f, dtype=torch.uint8, device=dev)
    gq, gk, gv = plane(), plane(), plane()
    gpos = torch.full((C, T), float("nan"), dtype=torch.float32, device=dev)
    rc = E.cot_local_relation_backward(P(gout), P(q), P(k), P(v), P(pos), P(probs), P(gq), P(gk), P(gv), P(gpos), P(buf[:nb]),
                                       ctypes.byref(g), dt, None)
    assert rc == 0, E.cot_last_error()
    assert E.cot_last_kernel().decode() == BWD
    assert (buf[nb:] == 0x7f).all().item(), "write past the reported workspace size"
    for name, t in (("out", out), ("probs", probs), ("gq", gq), ("gk", gk), ("gv", gv)):
        assert margins_untouched(t), f"write outside {name}"
    return (out, gq, gk, gv, gpos), probs


def directed(E, dev, N, C, H, W, dtype, qs=0.5, seed=0, report=None):
    """one geometry through `run` against the fp64 reference at the op's tolerances; the stored probabilities too (one storage rounding of
    the reference's: 2^-8 relative for bf16 covers the rounding and the bf16 bound above, 1e-5 (1 + a) absolute for fp32)"""
    q, k, v, gout, pos = inputs(N, C, H, W, dtype, seed, qs, dev=dev)
    got, probs = run(E, q, k, v, gout, pos)
    want = reference64(q, k, v, pos, gout)
    bad = mismatches(got, want, dtype, report)
    assert not bad, (N, C, H, W, dtype, bad)
    a = probs.detach().cpu().double().view(want[5].shape)
    assert ((a - want[5]).abs() <= (2e-5 if dtype == torch.float32 else 2.0 ** -7) * (1e-30 + want[5]) + 1e-7).all(), "probs"
    return got, want, probs


def saturated(E, dev, H, W, dtype, seed=6):
    """q x 6: most pixels put nearly all mass on one tap.  Everything finite; sum_t probs = 1 within storage rounding: each stored
    probability is one rounding of a_t (relative 2^-9 for bf16, 2^-24 for fp32, a few more ulp from exp and the division in fp32), and
    sum_t a_t = 1, so the sum moves by at most 2^-9 (bf16) -- bound 2^-8 -- and a few 2^-24 (fp32) -- bound 2e-6"""
    q, k, v, gout, pos = inputs(2, 24, H, W, dtype, seed, qs=6, dev=dev)
    got, probs = run(E, q, k, v, gout, pos)
    for name, t in zip(("out", "gq", "gk", "gv", "gpos"), got):
        assert torch.isfinite(t).all().item(), name
    assert torch.isfinite(probs).all().item()
    s = probs.detach().cpu().double().sum(3)
    assert (s - 1).abs().max().item() <= (2e-6 if dtype == torch.float32 else 2.0 ** -8), (s - 1).abs().max().item()
    assert (probs.detach().cpu().double().amax(3) > 0.99).float().mean().item() > 0.25  # the case is what it says: saturated


def refused_everywhere(E, g, dt):
    """-2 from all three entry points before any pointer is touched"""
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: the coverage check comes first
    assert E.cot_local_relation_workspace_bytes(ctypes.byref(g), dt) == -2
    assert E.cot_local_relation_forward(*([fake] * 6), ctypes.byref(g), dt, None) == -2
    assert E.cot_local_relation_backward(*([fake] * 11), ctypes.byref(g), dt, None) == -2


def lds_boundary(E, dev, dtype):
    W = boundary_width()
    dt = _lib.dtype_code(dtype)
    assert E.cot_local_relation_workspace_bytes(ctypes.byref(geom(2, 16, 3, W)), dt) > 0
    directed(E, dev, 2, 16, 3, W, dtype, seed=W)
    refused_everywhere(E, geom(2, 16, 3, W + 1), dt)
    assert b"not covered" in E.cot_last_error()


def refusals(E):
    refused_everywhere(E, geom(2, 64, 8, 8, k=5), _lib.COT_F32)            # 5x5 stays refused
    refused_everywhere(E, geom(2, 64, 8, 8), _lib.COT_F64)                 # fp64
    refused_everywhere(E, geom(2, 60, 8, 8, wC=15), _lib.COT_F32)          # C % 8
    refused_everywhere(E, geom(2, 64, 8, 8, wC=16), _lib.COT_F32)          # wC != C / 8
    g = geom(2, 64, 8, 8)
    g.ph = 2                                                               # 7x7 with another padding
    refused_everywhere(E, g, _lib.COT_F32)
    g = geom(2, 64, 8, 8)
    g.kw, g.pw = 3, 1                                                      # 7x3
    refused_everywhere(E, g, _lib.COT_F32)
    refused_everywhere(E, geom(2, 16, 3, 300), _lib.COT_BF16)              # wider than a workgroup


def misaligned(E, dev):
    """the C ABI takes 16-byte aligned pointers only: one operand one element off the grid is an invalid argument, before any kernel runs"""
    g, buf = geom(1, 8, 4, 12), torch.zeros(8 * 4 * 12 * 49 + 4, device=dev)
    ok, off = P(buf), ctypes.c_void_p(buf.data_ptr() + 4)
    for i in range(3):
        args = [ok] * 6
        args[i] = off
        assert E.cot_local_relation_forward(*args, ctypes.byref(g), _lib.COT_F32, None) == -1, i
    assert b"16-byte aligned" in E.cot_last_error()
    assert E.cot_local_relation_backward(*([off] + [ok] * 10), ctypes.byref(g), _lib.COT_F32, None) == -1


# ---- the random sweep.  Widths: 1; odd; W % 4 == 2; W % 4 == 0; the model's 7 / 14 / 28 / 56; one row per tile (W > 128) up to the widest
# the plan takes (224); two it refuses -- 2 of 27 widths, 7.4 %, so the rule alone stays under the 15 % cap
FUZZ_WIDTHS = [1, 3, 5, 7, 9, 13, 21, 2, 6, 10, 14, 30, 4, 8, 12, 16, 20, 28, 56, 100, 129, 130, 132, 171, 224, 225, 260]


def fuzz_case(E, dev, rng):
    N, C, H, W = rng.randint(1, 2), 8 * rng.choice([1, 2, 3, 5]), rng.randint(1, 16), rng.choice(FUZZ_WIDTHS)
    H = max(1, min(H, 12000 // (N * C * W)))  # one case stays fast on the emulator
    dtype = rng.choice(DTYPES)
    qs, null_probs = rng.choice([0.5, 2]), rng.random() < 0.25
    g, dt = geom(N, C, H, W), _lib.dtype_code(dtype)
    desc = ("local relation 7x7", N, C, H, W, str(dtype), qs, null_probs)
    if E.cot_local_relation_workspace_bytes(ctypes.byref(g), dt) == -2:
        try:
            refused_everywhere(E, g, dt)
        except AssertionError as e:
            return False, desc + (str(e)[:200],)
        return not fits(H, W), ("refused",) + desc[1:]
    q, k, v, gout, pos = inputs(N, C, H, W, dtype, rng.randint(0, 10 ** 6), qs, dev=dev)
    try:
        got, _ = run(E, q, k, v, gout, pos, null_probs=null_probs, margin=3 * (W + 1) + 1 + rng.randint(0, 9))
    except AssertionError as e:
        return False, desc + (str(e)[:200],)
    bad = mismatches(got, reference64(q, k, v, pos, gout), dtype)
    return fits(H, W) and not bad, desc + tuple(bad)
