"""Randomised differential test of the MFMA convolution / GroupNorm / pooling kernels (host-emulated) against torch:
random batch sizes, channel counts (multiples of 8), image sizes from 1x1 up, channel slabs, biases, forced split counts
and rows-per-wave overrides -- the shapes nobody would think of writing down.  (480 further cases ran clean offline in round 2,
1200 more -- with the LDS-staged grouped 3x3 weight gradient and the sub-sampling kernels added -- in round 3.)"""
import ctypes
import random

import pytest
import torch
import torch.nn.functional as F

from cotnet_amd import _lib
from tests import test_kernels_emulated as tke

pytestmark = pytest.mark.skipif(tke._EMUL is None, reason="host emulation build unavailable")
E = tke._EMUL
BF = 2  # COT_BF16
# tests/test_fuzz_gpu.py runs these cases on the device, where the compiler contracts a * b + c into one rounding: results that are the
# host model's bits here (same operations in the same order as the C oracle / as torch) are there within a few ulps of them
ON_DEVICE = False
SCALE = 1  # (scripts/fuzz_gpu.py --scale: larger planes on the device -- the 128-pixel-tile forms of the convolution kernels, H * W > 256)


@pytest.fixture(autouse=True)
def _library_defaults():
    """every case sets the keys it draws with _lib.tuned; whatever a failing one leaves behind ends here"""
    yield
    E.emul_set_dma_mode(0)
    _lib.reset_tuning(E)


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def close(a, b, tol=2e-2):
    a, b = a.float(), b.float()
    return ((a - b).abs() <= tol * (b.abs() + b.abs().mean() + 1e-3)).all().item()


def case_conv1x1(rng):
    N, Ci, Co = rng.randint(1, 3), 8 * rng.randint(1, 12), 8 * rng.randint(1, 12)
    H, W = rng.randint(1, 13 * SCALE), rng.randint(1, 13 * SCALE)
    split = rng.random() < 0.3 and Ci > 8
    bias = rng.random() < 0.5
    c1 = 8 * rng.randint(1, Ci // 8 - 1) if split else Ci
    rows, waves = rng.choice([0, 0, 2, 4]), rng.choice([2048, 2048, -2, -3])  # rows per wave; split count
    with _lib.tuned(E, C1_ROWS_PER_WAVE=rows, C1_WGRAD_WAVES=waves):  # (C1_WGRAD_WAVES sizes the workspace: set before it is asked for)
        x = torch.randn(N, Ci, H, W).bfloat16()
        w = (torch.randn(Co, Ci) / Ci ** 0.5).bfloat16()
        b = torch.randn(Co).bfloat16() if bias else None
        gy = torch.randn(N, Co, H, W).bfloat16()
        xf, wf = x.float().requires_grad_(True), w.float().requires_grad_(True)
        bf = b.float().requires_grad_(True) if bias else None
        yr = F.conv2d(xf, wf[:, :, None, None], bf)
        yr.backward(gy.float())
        x1 = x[:, :c1].contiguous() if split else x
        x2 = x[:, c1:].contiguous() if split else None
        y = torch.empty(N, Co, H, W).bfloat16()
        assert E.cot_conv1x1_forward(P(x1), P(x2), c1, P(w), P(b), P(y), N, Ci, Co, H * W, BF, None) == 0
        ws = torch.empty(E.cot_conv1x1_workspace(N, Ci, Co, H * W, 1 if bias else 0), dtype=torch.uint8)
        # accumulate bits: 1 = add into the first slab's buffer, 2 = into the second's (fp32 sum, one rounding)
        accumulate = rng.choice([0, 0, 1, 2, 3]) & (3 if split else 1)
        init1, init2 = torch.randn_like(x1.float()).bfloat16(), (torch.randn_like(x2.float()).bfloat16() if split else None)
        gx1, gx2 = init1.clone(), (init2.clone() if split else None)
        assert E.cot_conv1x1_backward_data(P(gy), P(w), P(gx1), P(gx2), c1, accumulate, P(ws), N, Ci, Co, H * W, BF, None) == 0
        gx = torch.cat([gx1, gx2], 1) if split else gx1
        add = [init1.float() if accumulate & 1 else torch.zeros_like(init1.float())]
        if split:
            add.append(init2.float() if accumulate & 2 else torch.zeros_like(init2.float()))
        xf.grad += torch.cat(add, 1)
        gw = torch.empty_like(w)
        gb = torch.empty_like(b) if bias else None
        assert E.cot_conv1x1_backward_weight(P(gy), P(x1), P(x2), c1, P(gw), P(gb), P(ws), N, Ci, Co, H * W, BF, None) == 0
        ok = close(y, yr.detach()) and close(gx, xf.grad, 3e-2) and close(gw, wf.grad) and (not bias or close(gb, bf.grad))
        return ok, ("conv1x1", N, Ci, Co, H, W, c1, bias)


def case_conv3x3(rng):
    G, Kc = rng.choice([1, 2, 4, 8]), 8 * rng.randint(1, 4)
    C, N, H, W = G * Kc, rng.randint(1, 2), rng.randint(1, 12 * SCALE), rng.randint(1, 12 * SCALE)
    with _lib.tuned(E, C1_WGRAD_WAVES=rng.choice([2048, -2])):
        x = torch.randn(N, C, H, W).bfloat16()
        w = (torch.randn(C, Kc, 3, 3) / (9 * Kc) ** 0.5).bfloat16()
        gy = torch.randn(N, C, H, W).bfloat16()
        xf, wf = x.float().requires_grad_(True), w.float().requires_grad_(True)
        yr = F.conv2d(xf, wf, None, 1, 1, 1, G)
        yr.backward(gy.float())
        masks = torch.empty(E.cot_conv3x3g_masks_bytes(H, W), dtype=torch.uint8)
        assert E.cot_conv3x3g_masks(P(masks), H, W, None) == 0
        ws = torch.empty(E.cot_conv3x3g_workspace(N, C, C, G, H, W), dtype=torch.uint8)
        y, gw = torch.empty_like(x), torch.empty_like(w)
        accumulate = rng.choice([0, 1])
        init = torch.randn_like(x.float()).bfloat16()
        gx = init.clone()
        assert E.cot_conv3x3g_forward(P(x), P(w), P(y), P(masks), P(ws), N, C, C, G, H, W, BF, None) == 0
        assert E.cot_conv3x3g_backward_data(P(gy), P(w), P(gx), accumulate, P(masks), P(ws), N, C, C, G, H, W, BF, None) == 0
        if accumulate:
            xf.grad += init.float()
        assert E.cot_conv3x3g_backward_weight(P(gy), P(x), P(gw), P(masks), P(ws), N, C, C, G, H, W, BF, None) == 0
        return close(y, yr.detach()) and close(gx, xf.grad, 3e-2) and close(gw, wf.grad), ("conv3x3g", N, C, G, H, W)


def case_group_norm(rng):
    N, G, H, W = rng.randint(1, 3), rng.randint(1, 4), rng.randint(1, 30), rng.randint(1, 30)
    C = 9 * G
    x = (torch.randn(N, C, H, W) * 1.5 + 0.3).bfloat16()
    ga, be = (1 + 0.3 * torch.randn(C)).bfloat16(), (0.2 * torch.randn(C)).bfloat16()
    dy = torch.randn(N, C, H, W).bfloat16()
    xf, gf, bf = (t.float().requires_grad_(True) for t in (x, ga, be))
    yr = F.group_norm(xf, G, gf, bf, 1e-5)
    yr.backward(dy.float())
    y, dx = torch.empty_like(x), torch.empty_like(x)
    m, r = torch.empty(N * G), torch.empty(N * G)
    dg, db, ws = torch.empty(C).bfloat16(), torch.empty(C).bfloat16(), torch.empty(2 * N * C)
    assert E.cot_group_norm9_forward(P(x), P(ga), P(be), P(y), P(m), P(r), N, C, H * W, 1e-5, BF, None) == 0
    assert E.cot_group_norm9_backward(P(dy), P(x), P(m), P(r), P(ga), P(dx), P(dg), P(db), P(ws), N, C, H * W, BF, None) == 0
    ok = H * W < 2 or (close(y, yr.detach(), 3e-2) and close(dx, xf.grad, 5e-2) and close(dg, gf.grad)
                       and close(db, bf.grad))
    return ok, ("group_norm9", N, G, H, W)


def case_pooling(rng):
    N, C, H, W = rng.randint(1, 3), rng.randint(1, 5), rng.randint(1, 17), rng.randint(1, 17)
    x = torch.relu(torch.randn(N, C, H, W)).bfloat16()  # post-ReLU: ties at zero everywhere
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    gy = torch.randn(N, C, Ho, Wo).bfloat16()
    ok = True
    for kind, mod in (("max", torch.nn.MaxPool2d(3, 2, 1)), ("avg", torch.nn.AvgPool2d(3, 2, padding=1))):
        xr = x.float().clone().requires_grad_(True)
        yr = mod(xr)
        yr.backward(gy.float())
        y, gx = torch.empty(N, C, Ho, Wo).bfloat16(), torch.empty_like(x)
        if kind == "max":
            assert E.cot_maxpool3x3s2_forward(P(x), P(y), N * C, H, W, BF, None) == 0
            assert E.cot_maxpool3x3s2_backward(P(gy), P(x), P(gx), N * C, H, W, BF, None) == 0
            ok = ok and torch.equal(y.float(), yr.detach())
        else:
            assert E.cot_avgpool3x3s2_forward(P(x), P(y), N * C, H, W, BF, None) == 0
            assert E.cot_avgpool3x3s2_backward(P(gy), P(gx), N * C, H, W, BF, None) == 0
        ok = ok and close(gx, xr.grad, 2e-2)
    return ok, ("pooling", N, C, H, W)


def case_conv3x3_guarded(rng):
    """the LDS-staged grouped 3x3 weight gradient (conv_wgrad2.hip TAPS form): x inside a NaN-margined allocation"""
    G = rng.choice([1, 2, 4])
    Kc, Mg = rng.choice([16, 16, 32, 64]), rng.choice([16, 32, 64, 128])
    N, H, W = rng.randint(1, 4), rng.randint(2, 15), rng.randint(2, 15)
    if H * W < 8:
        H = 4
    Ci, Co, HW = G * Kc, G * Mg, H * W
    guard = W + 1 + rng.randint(0, 9)
    lead = guard + (-guard) % 8
    flat = torch.full((N * Ci * HW + 2 * lead + 8,), float("nan")).bfloat16()
    x = flat[lead:lead + N * Ci * HW].view(N, Ci, H, W)
    x.copy_(torch.randn(N, Ci, H, W))
    gy = torch.randn(N, Co, H, W).bfloat16()
    wf = torch.zeros(Co, Kc, 3, 3, requires_grad=True)
    F.conv2d(x.float(), wf, None, 1, 1, 1, G).backward(gy.float())
    masks = torch.empty(E.cot_conv3x3g_masks_bytes(H, W), dtype=torch.uint8)
    assert E.cot_conv3x3g_masks(P(masks), H, W, None) == 0
    force = rng.choice([0, 0, 1, 2, 3, 7]) << 24  # forced slice counts (size the workspace afterwards)
    E.emul_set_dma_mode(rng.choice([0, 1]))
    with _lib.tuned(E, WGRAD2_BITS=force):
        ws = torch.full((E.cot_conv3x3g_workspace(N, Ci, Co, G, H, W),), 0x7f, dtype=torch.uint8)
        gw = torch.full((Co, Kc, 3, 3), float("nan")).bfloat16()
        assert E.cot_conv3x3g_backward_weight_guarded(P(gy), P(x), P(gw), P(masks), P(ws), N, Ci, Co, G, H, W, BF, guard, None) == 0
    E.emul_set_dma_mode(0)
    scale = wf.grad.abs().max().item()
    ok = (gw.float() - wf.grad).abs().max().item() <= 1e-2 * scale + 1e-2
    return ok, ("conv3x3 guarded wgrad", N, Ci, Co, G, H, W, guard)


def case_subsample(rng):
    N, C, H, W = rng.randint(1, 3), rng.randint(1, 9), 2 * rng.randint(1, 9), 2 * rng.randint(1, 9)
    x = torch.randn(N, C, H, W).bfloat16()
    y = torch.full((N, C, H // 2, W // 2), float("nan")).bfloat16()
    assert E.cot_subsample2_forward(P(x), P(y), N * C, H, W, BF, None) == 0
    gy = torch.randn(N, C, H // 2, W // 2).bfloat16()
    gx = torch.full_like(x, float("nan"))
    assert E.cot_subsample2_backward(P(gy), P(gx), N * C, H, W, BF, None) == 0
    ref = torch.zeros_like(x)
    ref[:, :, ::2, ::2] = gy
    return torch.equal(y, x[:, :, ::2, ::2]) and torch.equal(gx, ref), ("subsample2", N, C, H, W)



def _nan_margined(t, margin):
    """a copy of `t` that sits inside a NaN-filled allocation (`margin` elements either side, 16-byte aligned start)"""
    lead = margin + (-margin) % 8
    flat = torch.full((t.numel() + 2 * lead + 8,), float("nan"), dtype=t.dtype)
    v = flat[lead:lead + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def case_conv3x3_lds(rng):
    """round 4: the LDS-pipelined grouped 3x3 (conv_lds.hip), chunk-resident and per-step forms, one / two weight buffers,
    both tile planners, both K orders, both landing times of the LDS copies; operands inside NaN margins"""
    G = rng.choice([1, 2, 4, 8])
    Kc = rng.choice([16, 24, 32, 48, 64, 96, 128])
    while G * Kc > 512:
        G //= 2
    C, N = G * Kc, rng.randint(1, 3)
    H, W = rng.randint(3, 30 * min(SCALE, 2)), rng.randint(3, 30 * min(SCALE, 2))
    keys = dict(CONV3X3_RES=rng.choice([0, 1, 1, 2]), CONV3X3_WSINGLE=rng.choice([0, 1, 2]), CONV3X3_COLS=rng.choice([0, 1, 2]),
                CONV3X3_PERM=rng.choice([0, 1, 2]))
    dma = rng.choice([0, 1])
    x = _nan_margined(torch.randn(N, C, H, W).bfloat16(), W + 1 + rng.randint(0, 9))
    gy = _nan_margined(torch.randn(N, C, H, W).bfloat16(), W + 1 + rng.randint(0, 9))
    w = (torch.randn(C, Kc, 3, 3) / (9 * Kc) ** 0.5).bfloat16()
    xf, wf = x.float().requires_grad_(True), w.float()
    yr = F.conv2d(xf, wf, None, 1, 1, 1, G)
    yr.backward(gy.float())
    masks = torch.empty(E.cot_conv3x3g_masks_bytes(H, W), dtype=torch.uint8)
    assert E.cot_conv3x3g_masks(P(masks), H, W, None) == 0
    E.emul_set_dma_mode(dma)
    with _lib.tuned(E, **keys, CONV_LDS=1):
        ws = torch.full((E.cot_conv3x3g_workspace(N, C, C, G, H, W),), 0x7f, dtype=torch.uint8)
        y, init = torch.full_like(x, float("nan")), torch.randn(N, C, H, W).bfloat16()
        accumulate = rng.choice([0, 1])
        gx = init.clone() if accumulate else torch.full_like(x, float("nan"))
        assert E.cot_conv3x3g_forward(P(x), P(w), P(y), P(masks), P(ws), N, C, C, G, H, W, BF, None) == 0
        assert E.cot_conv3x3g_backward_data(P(gy), P(w), P(gx), accumulate, P(masks), P(ws), N, C, C, G, H, W, BF, None) == 0
    E.emul_set_dma_mode(0)
    want = xf.grad + (init.float() if accumulate else 0)
    return close(y, yr.detach()) and close(gx, want, 3e-2), ("conv3x3g lds", N, C, G, H, W, keys, dma, accumulate)


def case_bn(rng):
    """bn_act.hip: streaming / folded / channel-resident families, 7-element accesses on planes that are multiples of 7,
    ReLU sign mask against the saved-output path (bit-identical), against torch in fp32"""
    N, C = rng.randint(1, 40), rng.randint(1, 6)
    H, W = rng.choice([(1, 1), (2, 2), (7, 7), (7, 14), (14, 14), (4, 4), (8, 8), (3, 5), (5, 7), (28, 28), (6, 10)])
    if N * H * W < 2:
        N = 2
    dtype = rng.choice([torch.float32, torch.bfloat16])
    act, use_res = rng.choice([0, 1, 2]), rng.random() < 0.5
    keys = dict(BN_FOLD=rng.choice([0, 1]), BN_SMALL_M=rng.choice([0, 256]), BN_CHAN=rng.choice([0, 1]), BN_CHAN7=rng.choice([0, 1]))
    HW = H * W
    dt = tke._lib.dtype_code(dtype)
    x = (torch.randn(N, C, H, W) * 1.5 + 0.7).to(dtype)
    res = torch.randn(N, C, H, W).to(dtype) if use_res else None
    dy = torch.randn(N, C, H, W).to(dtype)
    gamma, beta = torch.rand(C) + 0.5, torch.randn(C) * 0.2
    xr = x.float().requires_grad_(True)
    rr = res.float().requires_grad_(True) if use_res else None
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    z = F.batch_norm(xr, torch.zeros(C), torch.ones(C), gr, br, True, 0.1, 1e-5)
    if use_res:
        z = z + rr
    yr = {0: lambda t: t, 1: torch.relu, 2: F.silu}[act](z)
    yr.backward(dy.float())
    with _lib.tuned(E, **keys):
        nb = E.cot_bn_relu_mask_bytes(N, C, HW, dt) if (act == 1 and use_res) else 0
        outs = []
        for use_mask in ([False, True] if nb else [False]):
            y = torch.full_like(x, float("nan"))
            mean, rstd, rm, rv = torch.empty(C), torch.empty(C), torch.zeros(C), torch.ones(C)
            nbt = torch.zeros((), dtype=torch.int64)
            ws = torch.empty(E.cot_bn_act_workspace(N, C))
            mask = torch.full((max(nb, 1),), 0xAA, dtype=torch.uint8)
            dx = torch.full_like(x, float("nan"))
            dres = torch.full_like(x, float("nan")) if use_res else None
            dg, db = torch.empty(C), torch.empty(C)
            if use_mask:
                assert E.cot_bn_act_forward_mask(P(x), P(res), P(y), P(mask), P(gamma), P(beta), P(mean), P(rstd), P(rm), P(rv), P(nbt),
                                                 P(ws), None, N, C, HW, 1e-5, 0.1, 1, dt, None) == 0
                assert E.cot_bn_act_backward_mask(P(dy), P(x), P(mask), P(dx), P(dres), P(gamma), P(beta), P(mean), P(rstd), P(dg),
                                                  P(db), P(ws), None, N, C, HW, 1, dt, None) == 0
            else:
                assert E.cot_bn_act_forward(P(x), P(res), P(y), P(gamma), P(beta), P(mean), P(rstd), P(rm), P(rv), P(nbt), P(ws),
                                            N, C, HW, 1e-5, 0.1, act, dt, None) == 0
                rc = E.cot_bn_act_backward(P(dy), P(x), P(y), P(dx), P(dres), P(gamma), P(beta), P(mean), P(rstd), P(dg), P(db),
                                           P(ws), N, C, HW, act, dt, None)
                assert rc == (-2 if act == 2 and use_res else 0)  # (SiLU after a residual add: forward only)
            outs.append((y, mean, rstd, dx, dres, dg, db))
    desc = ("bn", N, C, H, W, str(dtype), act, use_res, keys, bool(nb))
    if len(outs) == 2 and not all(torch.equal(a, b) for a, b in zip(*outs)):
        return False, desc
    y, mean, rstd, dx, dres, dg, db = outs[0]
    tol = 2e-5 if dtype == torch.float32 else 2e-2
    ok = ((y.float() - yr.detach()).abs() <= tol * (1 + yr.detach().abs())).all().item()
    if N * HW >= 8 and not (act == 1 and dtype == torch.bfloat16) and not (act == 2 and use_res):  # (tiny populations: 1/sigma amplifies the rounding; bf16 ReLU: see the directed test)
        gtol = 2e-4 if dtype == torch.float32 else 3e-2
        scale = 1 + xr.grad.abs().max().item()
        ok = ok and ((dx.float() - xr.grad).abs() <= gtol * scale).all().item()
        ok = ok and torch.allclose(dg, gr.grad, rtol=gtol * 10, atol=gtol * 10 * (1 + gr.grad.abs().max().item()))
        ok = ok and torch.allclose(db, br.grad, rtol=gtol * 10, atol=gtol * 10 * (1 + br.grad.abs().max().item()))
        if use_res:
            ok = ok and ((dres.float() - rr.grad).abs() <= gtol * (1 + rr.grad.abs())).all().item()
    return ok, desc


def case_stem(rng):
    """stem7x7.hip, LDS-staged and gather forms (tuning key 41), forward + weight gradient; input inside NaN margins"""
    N, H, W = rng.randint(1, 3), 2 * rng.randint(4, 24), 16 * rng.randint(1, 5)
    lds = rng.choice([0, 1])
    x = _nan_margined(torch.randn(N, 3, H, W).bfloat16(), 3 * W + 3 + rng.randint(0, 9))
    w = (torch.randn(64, 3, 7, 7) / 12).bfloat16()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    gy = _nan_margined(torch.randn(N, 64, Ho, Wo).bfloat16(), Wo + 1)
    wf = w.float().requires_grad_(True)
    yr = F.conv2d(x.float(), wf, None, 2, 3)
    yr.backward(gy.float())
    with _lib.tuned(E, STEM_LDS=lds):
        nb = E.cot_stem7x7s2_workspace(N, H, W)
        if nb == 0:
            return True, ("stem: geometry not covered", N, H, W)
        y = torch.full((N, 64, Ho, Wo), float("nan")).bfloat16()
        assert E.cot_stem7x7s2_forward(P(x), P(w), P(y), N, H, W, BF, None) == 0
        ws, gw = torch.full((nb,), 0x7f, dtype=torch.uint8), torch.full_like(w, float("nan"))
        assert E.cot_stem7x7s2_backward_weight(P(gy), P(x), P(gw), P(ws), N, H, W, BF, None) == 0
    ok = torch.allclose(y.float(), yr.detach(), atol=2e-2, rtol=2e-2)
    ok = ok and (gw.float() - wf.grad).abs().max().item() <= 1e-2 * wf.grad.abs().max().item() + 1e-2
    return ok, ("stem", N, H, W, lds)


def case_pool2(rng):
    """pool3x3.hip round-4 kernels: AvgPool2d(2, 2) (exact) and BlurPool in its per-pixel and row-block forms (same bits)"""
    from cotnet_amd.layers import BlurPool2d
    dtype = rng.choice([torch.float32, torch.bfloat16])
    dt = tke._lib.dtype_code(dtype)
    N, C = rng.randint(1, 3), rng.randint(1, 5)
    if rng.random() < 0.5:
        H, W = 2 * rng.randint(1, 15), 2 * rng.randint(1, 15)
        x, gy = torch.randn(N, C, H, W).to(dtype), torch.randn(N, C, H // 2, W // 2).to(dtype)
        xr = x.clone().requires_grad_(True)
        yr = torch.nn.AvgPool2d(2, 2, ceil_mode=True, count_include_pad=False)(xr)
        yr.backward(gy)
        y, gx = torch.full_like(yr, float("nan")), torch.full_like(x, float("nan"))
        assert E.cot_avgpool2x2s2_forward(P(x), P(y), N * C, H, W, dt, None) == 0
        assert E.cot_avgpool2x2s2_backward(P(gy), P(gx), N * C, H, W, dt, None) == 0
        return torch.equal(y, yr.detach()) and torch.equal(gx, xr.grad), ("avgpool2x2", N, C, H, W, str(dtype))
    H, W = rng.randint(2, 30), rng.randint(2, 30)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x, gy = torch.randn(N, C, H, W).to(dtype), torch.randn(N, C, Ho, Wo).to(dtype)
    xr = x.double().requires_grad_(True)
    yr = BlurPool2d(C)(xr)
    yr.backward(gy.double())
    outs = []
    for blk in (1, 0):
        with _lib.tuned(E, POOL_TILE=blk):
            y, gx = torch.full((N, C, Ho, Wo), float("nan")).to(dtype), torch.full_like(x, float("nan"))
            assert E.cot_blurpool3x3s2_forward(P(x), P(y), N * C, H, W, dt, None) == 0
            assert E.cot_blurpool3x3s2_backward(P(gy), P(gx), N * C, H, W, dt, None) == 0
            outs.append((y, gx))
    tol = 1e-6 if dtype == torch.float32 else 1.5e-2
    ok = torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    ok = ok and torch.allclose(outs[0][0].double(), yr.detach(), atol=tol, rtol=tol) and torch.allclose(outs[0][1].double(), xr.grad, atol=tol, rtol=tol)
    return ok, ("blurpool", N, C, H, W, str(dtype))


def case_conv1x1_stages(rng):
    """conv1x1_lds_fwd2 with three / six LDS stages on whole small images (tuning key 43), 64- / 128-row tiles (key 17), both
    landing times of the LDS copies: bit-identical to each other, close to torch; operands inside NaN margins"""
    N, Ci, Co = rng.randint(1, 6), 8 * rng.randint(2, 16), 8 * rng.randint(2, 40)
    H, W = rng.choice([(7, 7), (14, 14), (10, 10), (5, 9), (8, 8), (12, 16), (3, 3), (20, 20)])
    HW = H * W
    dma, k17 = rng.choice([0, 1]), rng.choice([0, 1 << 8])
    x = _nan_margined(torch.randn(N, Ci, H, W).bfloat16(), 8 + rng.randint(0, 30))
    gy = _nan_margined(torch.randn(N, Co, H, W).bfloat16(), 8 + rng.randint(0, 30))
    w = (torch.randn(Co, Ci) * Ci ** -0.5).bfloat16()
    ws = torch.empty(max(E.cot_conv1x1_workspace(N, Ci, Co, HW, 0), 256), dtype=torch.uint8)
    E.emul_set_dma_mode(dma)
    outs = []
    for ns3 in (2, 0):
        with _lib.tuned(E, CONV_LDS_BITS=k17, CONV_FLAT_NS3=ns3):
            y, gx = torch.full((N, Co, H, W), float("nan")).bfloat16(), torch.full((N, Ci, H, W), float("nan")).bfloat16()
            assert E.cot_conv1x1_forward(P(x), None, Ci, P(w), None, P(y), N, Ci, Co, HW, BF, None) == 0
            assert E.cot_conv1x1_backward_data(P(gy), P(w), P(gx), None, Ci, 0, P(ws), N, Ci, Co, HW, BF, None) == 0
            outs.append((y, gx))
    E.emul_set_dma_mode(0)
    ok = torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    ok = ok and close(outs[0][0], F.conv2d(x.float(), w.float()[:, :, None, None]))
    ok = ok and close(outs[0][1], F.conv2d(gy.float(), w.float().t().contiguous()[:, :, None, None]), 3e-2)
    return ok, ("conv1x1 stages", N, Ci, Co, H, W, dma, k17)


def case_agg_gn9(rng):
    """GroupNorm-9 in the aggregation's prologue (agg_nchw.hip forward, agg_dot2.hip backward) against the GroupNorm kernel
    followed by the plain aggregation on the same statistics: the same bits"""
    C = rng.choice([64, 128])
    Ch = C // 2
    H, W = rng.choice([(28, 28), (56, 56), (20, 40), (56, 28), (28, 56), (40, 40), (32, 32)])
    N = rng.randint(1, 2) if H * W < 2000 else 1
    HW, Ce, G = H * W, 9 * C // 8, C // 8
    if E.cot_gn9_fused_covers(Ch, Ch, 0, HW, W) != 1:
        return True, ("agg gn9: not covered", C, H, W)
    e3 = (torch.randn(N, Ce, H, W) * (0.5 + rng.random() * 2) + rng.random()).bfloat16()
    gamma, beta = (1 + 0.3 * torch.randn(Ce)).bfloat16(), (0.2 * torch.randn(Ce)).bfloat16()
    wn, mean, rstd = torch.empty_like(e3), torch.empty(N * G), torch.empty(N * G)
    assert E.cot_group_norm9_forward(P(e3), P(gamma), P(beta), P(wn), P(mean), P(rstd), N, Ce, HW, 1e-5, BF, None) == 0
    v, go = torch.randn(N, C, H, W).bfloat16(), torch.randn(N, C, H, W).bfloat16()
    geo = tke._lib.AggGeom(N, C, H, W, 1, G, 3, 3, 1, 1, 1, 1, 1, 1)
    a1, a2 = torch.full_like(v, float("nan")), torch.full_like(v, float("nan"))
    assert E.cot_agg_gn9_forward(P(v), P(e3), P(mean), P(rstd), P(gamma), P(beta), G, P(a1), ctypes.byref(geo), BF, None) == 0
    assert E.cot_agg_forward(P(v), P(wn), P(a2), ctypes.byref(geo), BF, 0, None) == 0
    gx1, gw1, gx2, gw2 = (torch.full_like(t, float("nan")) for t in (v, e3, v, e3))
    assert E.cot_agg_gn9_backward(P(go), P(v), P(e3), P(mean), P(rstd), P(gamma), P(beta), G, P(gx1), P(gw1), ctypes.byref(geo), BF, None) == 0
    assert E.cot_agg_backward(P(go), P(v), P(wn), P(gx2), P(gw2), ctypes.byref(geo), BF, 0, None) == 0
    return torch.equal(a1, a2) and torch.equal(gx1, gx2) and torch.equal(gw1, gw2), ("agg gn9", N, C, H, W)


def case_bn_ps(rng):
    """cot_bn_act_*_ps: y = act(s_n * bn(x) [+ residual]) with a per-sample scale (stochastic depth), every act / residual
    combination in fp32 against torch autograd; SiLU has no backward in this form (refused)"""
    N, C = rng.randint(2, 24), rng.randint(1, 5)
    H, W = rng.choice([(7, 7), (4, 4), (8, 8), (3, 5), (14, 14), (2, 2)])
    act, use_res, give_y = rng.choice([0, 1, 2]), rng.random() < 0.6, rng.random() < 0.5
    keys = dict(BN_FOLD=rng.choice([0, 1]), BN_SMALL_M=rng.choice([0, 256]), BN_CHAN=rng.choice([0, 1]), BN_CHAN7=rng.choice([0, 1]))
    HW, dt = H * W, tke._lib.dtype_code(torch.float32)
    x, dy = torch.randn(N, C, H, W) * 1.5 + 0.7, torch.randn(N, C, H, W)
    res = torch.randn(N, C, H, W) if use_res else None
    gamma, beta = torch.rand(C) + 0.5, torch.randn(C) * 0.2
    ps = (torch.rand(N) < 0.7).float() / 0.7
    xr = x.clone().requires_grad_(True)
    rr = res.clone().requires_grad_(True) if use_res else None
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    z = F.batch_norm(xr, None, None, gr, br, True, 0.1, 1e-5) * ps.view(N, 1, 1, 1)
    if use_res:
        z = z + rr
    yr = {0: lambda t: t, 1: torch.relu, 2: F.silu}[act](z)
    yr.backward(dy)
    with _lib.tuned(E, **keys):
        y, mean, rstd = torch.full_like(x, float("nan")), torch.empty(C), torch.empty(C)
        ws = torch.empty(E.cot_bn_act_workspace(N, C))
        assert E.cot_bn_act_forward_ps(P(x), P(res), P(y), P(gamma), P(beta), P(mean), P(rstd), None, None, None, P(ws), P(ps),
                                       N, C, HW, 1e-5, 0.1, act, dt, None) == 0
        dx, dres = torch.full_like(x, float("nan")), (torch.full_like(x, float("nan")) if use_res else None)
        dg, db = torch.empty(C), torch.empty(C)
        need_y = act == 1 and use_res
        rc = E.cot_bn_act_backward_ps(P(dy), P(x), P(y) if (need_y or give_y) else None, P(dx), P(dres), P(gamma), P(beta), P(mean),
                                      P(rstd), P(dg), P(db), P(ws), P(ps), N, C, HW, act, dt, None)
    desc = ("bn ps", N, C, H, W, act, use_res, give_y, keys)
    if act == 2:
        return rc == -2 and ((y - yr.detach()).abs() <= 2e-5 * (1 + yr.detach().abs())).all().item(), desc
    ok = rc == 0 and ((y - yr.detach()).abs() <= 2e-5 * (1 + yr.detach().abs())).all().item()
    ok = ok and ((dx - xr.grad).abs() <= 2e-4 * (1 + xr.grad.abs().max())).all().item()
    ok = ok and torch.allclose(dg, gr.grad, rtol=2e-3, atol=2e-3 * (1 + gr.grad.abs().max().item()))
    ok = ok and torch.allclose(db, br.grad, rtol=2e-3, atol=2e-3 * (1 + br.grad.abs().max().item()))
    if use_res:
        ok = ok and ((dres - rr.grad).abs() <= 2e-4 * (1 + rr.grad.abs())).all().item()
    return ok, desc


def case_aggregation(rng):
    """the operator itself (cupy_layers/aggregation_zeropad.py:20-110): random kernel / stride / padding / dilation (rectangular
    too), heads, weight sharing, both layouts, fused and split backward, fp64 / fp32 / bf16 storage against the C oracle --
    the k = 3 fast paths (LDS forward, dot2 backward at the widths it owns) and the generic kernels alike"""
    from oracle import unfold_oracle
    fast = rng.random() < 0.5
    if fast:  # k3 s1 p1 d1, one head, C / wC = 8: the CoT layer's form, plane sizes around the tuned ones
        k, s, p, d, heads = (3, 3), (1, 1), (1, 1), (1, 1), 1
        wC = rng.choice([1, 2, 4, 8, 16])
        C, H, W = 8 * wC, rng.randint(1, 30), rng.choice([1, 3, 7, 8, 14, 16, 20, 28, 31, 40, 56])
    else:
        k = (rng.choice([1, 3, 5, 7]), rng.choice([1, 3, 5]))
        s, d = (rng.randint(1, 3), rng.randint(1, 3)), (rng.randint(1, 2), rng.randint(1, 2))
        p = (rng.randint(0, 3), rng.randint(0, 3))
        heads, wC = rng.randint(1, 2), rng.randint(1, 4)
        C, H, W = wC * rng.randint(1, 4), rng.randint(1, 14), rng.randint(1, 14)
    N = rng.randint(1, 2)
    if (H + 2 * p[0] - d[0] * (k[0] - 1) - 1) < 0 or (W + 2 * p[1] - d[1] * (k[1] - 1) - 1) < 0:
        return True, ("aggregation: empty output", k, s, p, d, H, W)
    Ho, Wo = unfold_oracle.out_hw(H, W, k, s, p, d)
    dtype = rng.choice([torch.float64, torch.float32, torch.bfloat16] + [torch.bfloat16] * (2 if fast else 0))
    layout, fused = rng.choice([0, 0, 1]), rng.random() < 0.6
    x = torch.randn(N, C, H, W, dtype=torch.float64).to(dtype)
    w = torch.randn(N, heads, wC, k[0] * k[1], Ho, Wo, dtype=torch.float64).to(dtype)
    g = torch.randn(N, heads * C, Ho, Wo, dtype=torch.float64).to(dtype)
    y, gx, gw, fk, bk = tke.run(x, w, g, k, s, p, d, layout, fused)
    oy, ogx, ogw = tke.oracle_all(x.double(), w.double(), g.double(), k, s, p, d)
    taps = k[0] * k[1]
    tol = {torch.float64: 1e-12, torch.float32: 2e-5, torch.bfloat16: 1.2e-2}[dtype]
    def near(a, b, n):  # n terms of magnitude ~1 each
        return ((a.double() - b).abs() <= tol * (n ** 0.5 + b.abs())).all().item()
    ok = near(y, oy, taps) and near(gx, ogx, taps * heads) and near(gw, ogw, C // wC)
    return ok, ("aggregation", N, C, H, W, heads, wC, k, s, p, d, str(dtype), layout, fused, fk, bk)


def case_conv_general(rng):
    """conv_gen.hip and the routing around it: grouped 1x1 (any group width: tuned kernels group by group where they fit, the
    general kernels otherwise) and grouped 3x3 at widths off the tuned grid (12 / 20 / 40 ... per group, odd channel counts in
    fp32), fp32 and bf16, forward / data gradient (accumulate) / weight gradient (+ bias) against torch in fp64"""
    dtype = rng.choice([torch.float32, torch.bfloat16])
    dt = tke._lib.dtype_code(dtype)
    atol, rtol = tke._tol(dtype)
    G = rng.choice([1, 2, 3, 4, 8])
    N, H, W = rng.randint(1, 3), rng.randint(1, 11 * SCALE), rng.randint(1, 11 * SCALE)
    step = 1 if dtype == torch.float32 else 4
    if rng.random() < 0.5:   # grouped 1x1
        Ci, Co = G * step * rng.randint(1, 12), G * step * rng.randint(1, 12)
        if rng.random() < 0.3 and dtype == torch.bfloat16:
            Ci = G * 32 * rng.randint(1, 2)  # (the tuned kernels' grid)
            Co = G * 8 * rng.randint(1, 6)
        HW, bias, acc = H * W, rng.random() < 0.5, rng.choice([0, 1])
        x, gy = torch.randn(N, Ci, H, W).to(dtype), torch.randn(N, Co, H, W).to(dtype)
        w = (torch.randn(Co, Ci // G) / (Ci // G) ** 0.5).to(dtype)
        b = torch.randn(Co).to(dtype) if bias else None
        xf, wf = x.double().requires_grad_(True), w.double().requires_grad_(True)
        bf = b.double().requires_grad_(True) if bias else None
        yr = F.conv2d(xf, wf.view(Co, Ci // G, 1, 1), bf, 1, 0, 1, G)
        yr.backward(gy.double())
        y = torch.full((N, Co, H, W), float("nan")).to(dtype)
        desc = ("general 1x1", N, Ci, Co, G, H, W, str(dtype), bias, acc)
        rc = E.cot_conv1x1g_forward(P(x), P(w), P(b), P(y), N, Ci, Co, G, HW, dt, None)
        if rc == -2:
            return True, ("general 1x1: refused",) + desc[1:]
        init = torch.randn(N, Ci, H, W).to(dtype)
        gx = init.clone() if acc else torch.full_like(x, float("nan"))
        ok = rc == 0 and E.cot_conv1x1g_backward_data(P(gy), P(w), P(gx), acc, N, Ci, Co, G, HW, dt, None) == 0
        ws = torch.full((E.cot_convg_workspace(N, Ci, Co, G, HW, 1, 1) // 4,), float("nan"))
        gw, gb = torch.full_like(w, float("nan")), (torch.full_like(b, float("nan")) if bias else None)
        ok = ok and E.cot_conv1x1g_backward_weight(P(gy), P(x), P(gw), P(gb), P(ws), N, Ci, Co, G, HW, dt, None) == 0
        want = xf.grad + (init.double() if acc else 0)
        ok = ok and torch.allclose(y.double(), yr.detach(), atol=4 * atol, rtol=rtol)
        ok = ok and torch.allclose(gx.double(), want, atol=8 * atol, rtol=2 * rtol)
        ok = ok and (gw.double() - wf.grad.view(Co, Ci // G)).abs().max().item() <= rtol * wf.grad.abs().max().item() + atol
        if bias:
            ok = ok and (gb.double() - bf.grad).abs().max().item() <= rtol * bf.grad.abs().max().item() + atol
        return ok, desc
    C = G * step * rng.randint(1, 10)
    x, gy = torch.randn(N, C, H, W).to(dtype), torch.randn(N, C, H, W).to(dtype)
    w = (torch.randn(C, C // G, 3, 3) / (9 * C // G) ** 0.5).to(dtype)
    xf, wf = x.double().requires_grad_(True), w.double().requires_grad_(True)
    yr = F.conv2d(xf, wf, None, 1, 1, 1, G)
    yr.backward(gy.double())
    masks = torch.empty(E.cot_conv3x3g_masks_bytes(H, W), dtype=torch.uint8)
    assert E.cot_conv3x3g_masks(P(masks), H, W, None) == 0
    ws = torch.full((max(E.cot_conv3x3g_workspace(N, C, C, G, H, W), E.cot_convg_workspace(N, C, C, G, H, W, 3), 256) // 4,), float("nan"))
    y, gw, acc = torch.full_like(x, float("nan")), torch.full_like(w, float("nan")), rng.choice([0, 1])
    init = torch.randn(N, C, H, W).to(dtype)
    gx = init.clone() if acc else torch.full_like(x, float("nan"))
    desc = ("general 3x3", N, C, G, H, W, str(dtype), acc)
    rc = E.cot_conv3x3g_forward(P(x), P(w), P(y), P(masks), P(ws), N, C, C, G, H, W, dt, None)
    if rc == -2:
        return True, ("general 3x3: refused",) + desc[1:]
    ok = rc == 0 and E.cot_conv3x3g_backward_data(P(gy), P(w), P(gx), acc, P(masks), P(ws), N, C, C, G, H, W, dt, None) == 0
    ok = ok and E.cot_conv3x3g_backward_weight(P(gy), P(x), P(gw), P(masks), P(ws), N, C, C, G, H, W, dt, None) == 0
    want = xf.grad + (init.double() if acc else 0)
    ok = ok and torch.allclose(y.double(), yr.detach(), atol=4 * atol, rtol=rtol)
    ok = ok and torch.allclose(gx.double(), want, atol=8 * atol, rtol=2 * rtol)
    ok = ok and (gw.double() - wf.grad).abs().max().item() <= rtol * wf.grad.abs().max().item() + atol
    return ok, desc


def case_elementwise(rng):
    """the small per-plane kernels at random plane sizes: radix-2 tail (gap / mix / backward, models/cotnet.py:92-104), the SE
    gate of SplitAttn (radix 1), eval-mode BatchNorm + act + residual"""
    dtype = rng.choice([torch.float32, torch.bfloat16])
    dt, tol = tke._lib.dtype_code(dtype), (1e-5 if dtype == torch.float32 else 2e-2)
    B, C, H, W = rng.randint(1, 4), rng.randint(1, 12), rng.randint(1, 20), rng.randint(1, 20)
    planes, HW = B * C, H * W
    def near(a, b, f=1.0):
        return ((a.double() - b.double()).abs() <= f * tol * (1 + b.double().abs())).all().item()
    which = rng.choice(["radix", "se", "bn_eval"])
    desc = (which, B, C, H, W, str(dtype))
    if which == "radix":
        y, k, gout = (torch.randn(B, C, H, W).to(dtype) for _ in range(3))
        attn = torch.softmax(torch.randn(B, C, 2), dim=2).to(dtype)
        yr, kr, ar = y.float().requires_grad_(True), k.float().requires_grad_(True), attn.float().requires_grad_(True)
        x5 = torch.cat([yr.view(B, C, 1, H, W), kr.view(B, C, 1, H, W)], dim=2)
        gap_ref, out_ref = x5.sum(dim=2).mean((2, 3), keepdim=True), (x5 * ar.reshape(B, C, 2, 1, 1)).sum(dim=2)
        out_ref.backward(gout.float())
        gap, out = torch.full((B, C, 1, 1), float("nan")).to(dtype), torch.full_like(y, float("nan"))
        gy, gk, ga = torch.full_like(y, float("nan")), torch.full_like(k, float("nan")), torch.full_like(attn, float("nan"))
        ok = E.cot_radix_gap(P(y), P(k), P(gap), planes, HW, dt, None) == 0
        ok = ok and E.cot_radix_mix(P(y), P(k), P(attn), P(out), planes, HW, dt, None) == 0
        ok = ok and E.cot_radix_mix_backward(P(gout), P(y), P(k), P(attn), P(gy), P(gk), P(ga), planes, HW, dt, None) == 0
        ok = ok and near(gap, gap_ref.detach()) and near(out, out_ref.detach()) and near(gy, yr.grad) and near(gk, kr.grad)
        return ok and near(ga, ar.grad, 4 * max(1.0, HW ** 0.5 / 4)), desc
    if which == "se":
        x, g, logit = torch.randn(B, C, H, W).to(dtype), torch.randn(B, C, H, W).to(dtype), (2 * torch.randn(B, C)).to(dtype)
        xr, lr = x.double().requires_grad_(True), logit.double().requires_grad_(True)
        outr = xr * torch.sigmoid(lr)[:, :, None, None]
        outr.backward(g.double())
        gap, out = torch.full((B, C), float("nan")).to(dtype), torch.full_like(x, float("nan"))
        gx, gl = torch.full_like(x, float("nan")), torch.full_like(logit, float("nan"))
        ok = E.cot_se_gap(P(x), P(gap), planes, HW, dt, None) == 0 and E.cot_se_gate(P(x), P(logit), P(out), planes, HW, dt, None) == 0
        ok = ok and E.cot_se_gate_backward(P(g), P(x), P(logit), P(gx), P(gl), planes, HW, dt, None) == 0
        ok = ok and near(gap, x.double().mean((2, 3))) and near(out, outr.detach()) and near(gx, xr.grad)
        return ok and near(gl, lr.grad, 10 * max(1.0, HW ** 0.5 / 4)), desc
    act, use_res = rng.choice([0, 1, 2]), rng.random() < 0.5
    x = (torch.randn(B, C, H, W) * 1.5 + 0.7).to(dtype)
    res = torch.randn(B, C, H, W).to(dtype) if use_res else None
    gamma, beta, rm, rv = torch.rand(C) + 0.5, torch.randn(C) * 0.2, torch.randn(C) * 0.3, torch.rand(C) + 0.5
    z = F.batch_norm(x.float(), rm, rv, gamma, beta, False, 0.1, 1e-5)
    if use_res:
        z = z + res.float()
    yr = {0: lambda t: t, 1: torch.relu, 2: F.silu}[act](z)
    y = torch.full_like(x, float("nan"))
    ok = E.cot_bn_act_inference(P(x), P(res), P(y), P(gamma), P(beta), P(rm), P(rv), B, C, HW, 1e-5, act, dt, None) == 0
    return ok and near(y, yr, 2.0), desc + (act, use_res)


def case_optimizer_and_input(rng):
    """fused SGD step (any length: vector body + tail, n = 1 too) and the loader's uint8 -> float normalisation (exact)"""
    if rng.random() < 0.5:
        n = rng.choice([1, 2, 3, 7, 8, 9, 63, 64, 65, 255, 1023, 4096, rng.randint(1, 20000)])
        pdt, gdt = rng.choice([(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.bfloat16, torch.float32)])
        nesterov = rng.choice([0, 1])
        lr, mu, wd, gs = rng.random(), rng.choice([0.0, 0.9]), rng.choice([0.0, 1e-2]), rng.choice([1.0, 0.5])
        master, mom, grad = torch.randn(n), torch.randn(n) * 0.1, torch.randn(n).to(gdt)
        param = master.to(pdt)
        master_arg, ref_p = (None, param.clone()) if pdt == torch.float32 else (master.clone(), master.clone())
        gg = grad.float() * gs + wd * ref_p
        buf = mu * mom + gg
        ref_p = ref_p - lr * (gg + mu * buf if nesterov else buf)
        ok = E.cot_sgd_step(P(param), P(master_arg), P(mom), P(grad), n, lr, mu, wd, gs, nesterov, tke._lib.dtype_code(pdt),
                            tke._lib.dtype_code(gdt), None) == 0
        atol = 1e-6 if ON_DEVICE else 1e-7
        ok = ok and torch.allclose(mom, buf, rtol=1e-6, atol=atol)
        if master_arg is not None:
            ok = ok and torch.allclose(master_arg, ref_p, rtol=1e-6, atol=atol) and torch.equal(param, master_arg.to(pdt))
        else:
            ok = ok and torch.allclose(param, ref_p, rtol=1e-6, atol=atol)
        return ok, ("sgd", n, str(pdt), str(gdt), nesterov)
    shape = (rng.randint(1, 3), rng.randint(1, 4), rng.randint(1, 40), rng.randint(1, 40))
    x = torch.randint(0, 256, shape, dtype=torch.uint8)
    C = shape[1]
    mean, std = torch.tensor([123.675, 116.28, 103.53, 99.0][:C]), torch.tensor([58.395, 57.12, 57.375, 50.0][:C])
    dtype = rng.choice([torch.float32, torch.bfloat16, torch.float16])
    m, sd = (mean.half().float(), std.half().float()) if dtype == torch.float16 else (mean, std)
    y = torch.empty(shape, dtype=dtype)
    ok = E.cot_input_normalize(P(x), P(y), P(m), P(sd), shape[0] * C, C, shape[2] * shape[3], tke._lib.dtype_code(dtype), None) == 0
    if dtype == torch.float16:
        ref = x.half().sub_(m.half().view(1, C, 1, 1)).div_(sd.half().view(1, C, 1, 1))
    else:
        ref = x.float().sub_(m.view(1, C, 1, 1)).div_(sd.view(1, C, 1, 1)).to(dtype)
    return ok and torch.equal(y, ref), ("input normalise", shape, str(dtype))


# ---- the local-relation kernels (local_relation.hip) against a plain fp64 statement of the operation: rectangular planes, every loader
# width (W odd / W % 4 == 2 / W % 4 == 0), single-row tiles (W > 128) up to and beyond the LDS boundary, ragged last tiles, both backward routes
def lr_reference64(q, k, v, pos, gout, terms=False):
    """fp64, from unfold and einsum (the semantics in the header of local_relation.hip), differentiated by autograd:
        logit[n,g,t,p] = sum_{j<8} q[n,8g+j,p] (uk[n,8g+j,t,p] + pos[8g+j,t])   uk = 0 outside the image: a padded tap keeps q * pos
        out[n,c,p]     = sum_t softmax_t(logit)[n, c mod G, t, p] v[n,c,p + off_t]
    -> (out, gq, gk, gv, gpos[C][9]); with `terms` also, for the bounds on bf16 gk (gL = d loss / d logit, gA = d loss / d a):
        S[n,c,p'] = sum_t |gL_t q| at p' - off_t                                   the magnitudes of the products gk[n,c,p'] sums
        R[n,c,p'] = sum_t |q| (2 |gL_t| + a_t sum_u a_u |gA_u|) at p' - off_t      what a relative error of 1 in every a_u moves them by"""
    N, C, H, W = q.shape
    G = C // 8
    q, k, v, pos = (t.detach().double().requires_grad_(True) for t in (q, k, v, pos))
    uk = F.unfold(k, 3, 1, 1, 1).view(N, G, 8, 9, H, W)
    logit = torch.einsum("ngjhw,ngjthw->ngthw", q.view(N, G, 8, H, W), uk + pos.view(1, G, 8, 9, 1, 1))
    logit.retain_grad()
    a = torch.softmax(logit, 2)
    a.retain_grad()
    uv = F.unfold(v, 3, 1, 1, 1).view(N, 8, G, 9, H, W)  # channel c = g + j G takes head g = c mod G
    out = torch.einsum("ngthw,njgthw->njghw", a, uv).reshape(N, C, H, W)
    out.backward(gout.double())
    res = (out.detach(), q.grad, k.grad, v.grad, pos.grad)
    if terms:
        gather = lambda x: F.fold(x.reshape(N, C * 9, H * W), (H, W), 3, 1, 1, 1)  # noqa: E731  (the term at p lands on p + off_t)
        aq = q.detach().abs().view(N, G, 8, 1, H, W)
        gl, ad = logit.grad.abs(), a.detach()
        moved = 2 * gl + ad * (ad * a.grad.abs()).sum(2, keepdim=True)
        res += (gather(gl.view(N, G, 1, 9, H, W) * aq), gather(moved.view(N, G, 1, 9, H, W) * aq))
    return res


def lr_tolerances(dtype):
    """(name -> factor) on `tol (1 + |want|)` per element, tests/test_lrnet_emulated.py::test_forward_and_all_gradients_match_the_composition"""
    return (2e-5 if dtype == torch.float32 else 4e-2), {"out": 1, "gv": 1, "gq": 4, "gk": 4}


def lr_mismatches(got, want, dtype, skip=()):
    """names of the outputs (out, gq, gk, gv, gpos) that are not finite or off the fp64 reference; gpos against its own scale"""
    tol, factor = lr_tolerances(dtype)
    bad = []
    for name, g, w in zip(("out", "gq", "gk", "gv"), got, want):
        if not torch.isfinite(g).all().item():
            bad.append((name, "not finite"))
        elif name not in skip:
            err = (g.double() - w).abs()
            if not (err <= factor[name] * tol * (1 + w.abs())).all().item():
                bad.append((name, err.max().item()))
    g, w = got[4], want[4]
    err = (g.double() - w).abs().max().item()
    if not torch.isfinite(g).all().item() or not err <= 4 * tol * max(1.0, w.abs().max().item()):
        bad.append(("gpos", err))
    return bad


def lr_gk_ratio(gk, want, S):
    """bf16 gk under a saturated softmax: the error beyond the output rounding 2^-9 |want|, in units of 2^-8 S (S from lr_reference64:
    the magnitudes of the products the element sums)"""
    over = ((gk.double() - want).abs() - 2.0 ** -9 * want.abs()).clamp_min(0)
    return (over / (2.0 ** -8 * S).clamp_min(1e-300)).max().item()


def lr_gk_rounding_ratio(gk, want, R):
    """the same error in units of 2^-8 R + LR_GK_FLOOR.  The forward rounds each probability to bf16 once (a_u (1 + e_u), |e_u| <= 2^-8, the
    unit roundoff of 8 significant bits) and the backward stores gL_t = a_t (gA_t - sum_u a_u gA_u) in bf16, so to first order gL_t moves
    by at most 2^-8 (2 |gL_t| + a_t sum_u a_u |gA_u|).  The second term does not shrink with gL_t, which is why a saturated softmax
    (gL_t -> 0) leaves gk errors far above 2^-8 S.  The floor: a gL_t or a gk below the smallest normal number (1.2e-38) is flushed
    to zero, a relative error of 1 that no multiple of R covers; 9 such products with |q| of a few tens stay far below 1e-30."""
    over = ((gk.double() - want).abs() - 2.0 ** -9 * want.abs()).clamp_min(0)
    return (over / (2.0 ** -8 * R + LR_GK_FLOOR)).max().item()


LR_GK_FLOOR = 1e-30


def _margins_untouched(view):
    """`view` came from _nan_margined: everything around it in its allocation is still NaN"""
    flat, lo = view._base, view.storage_offset()
    return flat[:lo].isnan().all().item() and flat[lo + view.numel():].isnan().all().item()


def lr_geom(N, C, H, W):
    return tke._lib.AggGeom(N, C, H, W, 1, C // 8, 3, 3, 1, 1, 1, 1, 1, 1)


def lr_run(q, k, v, gout, pos, null_probs=False, margin=None):
    """forward + backward through the C ABI of `E`: q / k / v / gout / probs inside NaN margins, NaN-filled outputs inside NaN margins that
    must stay NaN (wide enough for a whole tile, at most 256 pixels, written past the end of the last plane: the row guard of a ragged last
    tile), the workspace at exactly the reported size, 0x7f-filled, with a guard behind it.  Every pointer is 16-byte aligned, which the C ABI
    requires (tests/test_lrnet_emulated.py::test_misaligned_pointers_are_refused) -> ((out, gq, gk, gv, gpos), probs, first backward kernel)"""
    N, C, H, W = q.shape
    g, dt = lr_geom(N, C, H, W), tke._lib.dtype_code(q.dtype)
    margin = W + 1 if margin is None else margin
    q, k, v, gout = (_nan_margined(t, margin) for t in (q, k, v, gout))
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=q.dtype)  # noqa: E731
    plane = lambda: _nan_margined(nan(N, C, H, W), 256 + W + 1)  # noqa: E731
    probs, out = _nan_margined(nan(N, 1, C // 8, 9, H, W), 256 + W + 1), plane()
    assert E.cot_local_relation_forward(P(q), P(k), P(v), P(pos), P(out), P(probs), ctypes.byref(g), dt, None) == 0, E.cot_last_error()
    if null_probs:  # the branch that stores no probabilities: the same bits in out
        out2 = plane()
        assert E.cot_local_relation_forward(P(q), P(k), P(v), P(pos), P(out2), None, ctypes.byref(g), dt, None) == 0, E.cot_last_error()
        assert torch.isfinite(out).all().item() and torch.equal(out, out2), "probs == NULL changes out"
        assert _margins_untouched(out2), "write outside out (probs == NULL)"
    nb = int(E.cot_local_relation_workspace_bytes(ctypes.byref(g), dt))
    assert nb > 0, nb
    buf = torch.full((nb + 256,), 0x7f, dtype=torch.uint8)
    gq, gk, gv, gpos = plane(), plane(), plane(), torch.full((C, 9), float("nan"), dtype=torch.float32)
    rc = E.cot_local_relation_backward(P(gout), P(q), P(k), P(v), P(pos), P(probs), P(gq), P(gk), P(gv), P(gpos), P(buf[:nb]),
                                       ctypes.byref(g), dt, None)
    assert rc == 0, E.cot_last_error()
    route = E.cot_last_kernel().decode().split("+")[0]
    assert (buf[nb:] == 0x7f).all().item(), "write past the reported workspace size"
    for name, t in (("out", out), ("probs", probs), ("gq", gq), ("gk", gk), ("gv", gv)):
        assert _margins_untouched(t), f"write outside {name}"
    return (out, gq, gk, gv, gpos), probs, route


# 1; odd (the V = 1 loader); W % 4 == 2 (V = 2); W % 4 == 0 (V = 4); the model's 28 / 56; one row per tile (W > 128) up to the widest
# width that fits LDS (211); two beyond it
LR_WIDTHS = [1, 3, 5, 7, 9, 13, 21, 2, 6, 10, 14, 30, 4, 8, 12, 16, 20, 28, 56, 100, 129, 130, 132, 171, 200, 211, 214, 260]


def case_local_relation(rng):
    N, C, H, W = rng.randint(1, 3), 8 * rng.choice([1, 2, 3, 5, 8, 16]), rng.randint(1, 28), rng.choice(LR_WIDTHS)
    if N * C * W > 60000:
        N = 1
    H = max(1, min(H, 60000 // (N * C * W)))  # one case stays fast on the emulator
    dtype = rng.choice([torch.float32, torch.bfloat16])
    qs, null_probs, margin = rng.choice([0.5, 2]), rng.random() < 0.25, W + 1 + rng.randint(0, 9)
    g, dt = lr_geom(N, C, H, W), tke._lib.dtype_code(dtype)
    desc = ("local relation", N, C, H, W, str(dtype), qs, null_probs)
    if E.cot_local_relation_workspace_bytes(ctypes.byref(g), dt) == -2:
        fake = ctypes.c_void_p(0x1000)  # never dereferenced: the coverage check comes first
        ok = E.cot_local_relation_forward(*([fake] * 6), ctypes.byref(g), dt, None) == -2
        ok = ok and E.cot_local_relation_backward(*([fake] * 11), ctypes.byref(g), dt, None) == -2
        return ok, ("local relation: refused",) + desc[1:]
    q, k, v, gout = (torch.randn(N, C, H, W) for _ in range(4))
    q, k, v, gout = (qs * q).to(dtype), (0.5 * k).to(dtype), v.to(dtype), gout.to(dtype)
    pos = (torch.randn(C, 3, 1) + torch.randn(C, 1, 3)).reshape(C, 9).contiguous()
    try:
        got, _, route = lr_run(q, k, v, gout, pos, null_probs, margin)
    except AssertionError as e:
        return False, desc + (str(e)[:200],)
    bad = lr_mismatches(got, lr_reference64(q, k, v, pos, gout), dtype)
    return not bad, desc + (route,) + tuple(bad)


CASES_LR = [case_local_relation]


def lr_check_kinds(descs):
    """the two conditions that keep the case from hiding a failure: few refusals, both backward routes well represented"""
    refused = [d for d in descs if d[0].endswith("refused")]
    accepted = [d for d in descs if not d[0].endswith("refused")]
    assert len(refused) <= 0.15 * len(descs), (len(refused), len(descs))
    for route in ("lr_softmax_bwd", "agg_bwd_nchw_k3_lds<softmax>"):
        n = sum(1 for d in accepted if route in d)
        assert n >= 0.2 * len(accepted), (route, n, len(accepted))


@pytest.mark.parametrize("seed", [71, 72])
def test_random_shapes_local_relation(seed):
    rng = random.Random(seed)
    torch.manual_seed(seed)
    failures, descs = [], []
    for _ in range(120):
        ok, desc = case_local_relation(rng)
        descs.append(desc)
        if not ok:
            failures.append(desc)
    assert not failures, failures
    lr_check_kinds(descs)


CASES = [case_conv1x1, case_conv1x1, case_conv3x3, case_conv3x3_guarded, case_group_norm, case_pooling, case_subsample]
CASES_R4 = [case_conv3x3_lds, case_conv3x3_lds, case_bn, case_bn, case_stem, case_pool2, case_conv1x1_stages, case_agg_gn9, case_bn_ps, case_aggregation, case_aggregation, case_conv_general, case_conv_general, case_elementwise, case_optimizer_and_input]


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_random_shapes(seed):
    rng = random.Random(seed)
    torch.manual_seed(seed)
    failures = []
    for _ in range(40):
        ok, desc = rng.choice(CASES)(rng)
        if not ok:
            failures.append(desc)
    assert not failures, failures


@pytest.mark.parametrize("seed", [41, 42])
def test_random_shapes_round4_kernels(seed):
    """(7300 further cases of this list ran clean offline in round 4; its first run found SiLU + residual: backward now refused)"""
    rng = random.Random(seed)
    torch.manual_seed(seed)
    failures = []
    for _ in range(30):
        ok, desc = rng.choice(CASES_R4)(rng)
        if not ok:
            failures.append(desc)
    assert not failures, failures


# ---- round 6: the LDS-tiled aggregation_zeropad_mix kernels against the C oracle (random storage types, plane sizes from 1 x 1 up, heads,
# channel groups, lanes per workgroup, pixels per lane) and the deep stem's first convolution against torch
def case_mix(rng):
    from oracle import cref
    dtype = rng.choice([torch.float64, torch.float32, torch.bfloat16])
    N, heads, wC, J = rng.randint(1, 2), rng.randint(1, 2), rng.choice([1, 2, 3, 4, 8]), rng.randint(1, 4)
    C, H, W = wC * J, rng.randint(1, 11), rng.randint(1, 12)
    lanes, ppl = rng.choice([64, 128, 256]), rng.choice([0, 0, 1, 2, 4])
    mk = lambda *s: torch.randn(*s, dtype=torch.float64).to(dtype)  # noqa: E731
    x, w1, w2 = mk(N, C, H, W), mk(N, heads, wC, 9, H, W), mk(N, heads, wC, 25, H, W)
    gout = mk(N, 2 * heads * C, H, W)
    with _lib.tuned(E, MIX_LANES=lanes, MIX_PPL=ppl):
        out, gx, gw1, gw2, names = tke._mix_run(E, x, w1, w2, gout)
    od = torch.float32 if dtype == torch.bfloat16 else dtype
    want = (cref.mix_forward(x.to(od), w1.to(od), w2.to(od), 1, 1, 2, 1),
            cref.mix_backward_input(gout.to(od), w1.to(od), w2.to(od), x.shape, 1, 1, 2, 1, False),
            *cref.mix_backward_weight(gout.to(od), x.to(od), w1.shape, w2.shape, 1, 1, 2, 1))
    ok = all(n.endswith("_tile") for n in names)
    for got, w in zip((out, gx, gw1, gw2), want):
        if dtype == torch.bfloat16:
            ok = ok and ((got.float() - w).abs() <= 2.0 ** -8 * w.abs() + 1e-6).all().item()
        elif ON_DEVICE:
            ok = ok and ((got - w).abs().max() <= (1e-5 if dtype == torch.float32 else 1e-13) * (1 + w.abs().max())).item()
        else:
            ok = ok and torch.equal(got, w)
    return ok, ("mix", str(dtype), N, heads, wC, J, H, W, lanes, ppl, names)


def case_stem3x3(rng):
    N, Co = rng.randint(1, 3), rng.choice([32, 64])
    Ho, Wo = rng.choice([(4, 8), (2, 16), (8, 8), (1, 32), (4, 24), (16, 8)])
    H, W = 2 * Ho - rng.randint(0, 1), 2 * Wo - rng.randint(0, 1)
    x = torch.randn(N, 3, H, W).bfloat16()
    w = (torch.randn(Co, 3, 3, 3) / 5).bfloat16()
    gy = torch.randn(N, Co, Ho, Wo).bfloat16()
    wf = w.float().requires_grad_(True)
    yr = F.conv2d(x.float(), wf, None, 2, 1)
    yr.backward(gy.float())
    y = torch.full((N, Co, Ho, Wo), float("nan")).bfloat16()
    ok = E.cot_stem3x3s2_forward(P(x), P(w), P(y), N, H, W, Co, BF, None) == 0
    ok = ok and ((y.float() - yr.detach()).abs() <= 2.0 ** -8 * yr.detach().abs() + 1e-5).all().item()
    ws = torch.empty(E.cot_stem3x3s2_workspace(N, H, W, Co), dtype=torch.uint8)
    gw = torch.full_like(w, float("nan"))
    ok = ok and E.cot_stem3x3s2_backward_weight(P(gy), P(x), P(gw), P(ws), N, H, W, Co, BF, None) == 0
    ok = ok and (gw.float() - wf.grad).abs().max().item() <= 1e-2 * wf.grad.abs().max().item() + 1e-2
    return ok, ("stem3x3", N, Co, H, W)


def _asserting(fn, desc):
    """the shared cases of tests/bn_tail_cases.py assert instead of returning a verdict; a refusal (COT_ERR_UNSUPPORTED) is not a failure"""
    if ON_DEVICE:
        torch.set_default_device("cpu")  # (those cases place their tensors themselves: operands on the device, references on the host)
    try:
        fn()
    except AssertionError as e:
        msg = str(e)
        if "not covered" in msg:
            return True, desc + ("refused",)
        import traceback
        where = traceback.extract_tb(e.__traceback__)[-1]
        return False, desc + (f"{where.filename.rsplit('/', 1)[-1]}:{where.lineno} {where.line} {msg[:200]}",)
    finally:
        if ON_DEVICE:
            torch.set_default_device("cuda")
    return True, desc


def case_bn_tail(rng):
    """BatchNorm + SiLU folded into the radix tail (radix_tail.hip cot_radix_*_bn; models/cotnet.py:89-104): random populations from two
    elements up, either statistics route, NCHW / channel-major k, both storage types"""
    from tests.bn_tail_cases import bn_tail_case
    N, C, H, W = rng.randint(1, 12), rng.randint(1, 20), rng.randint(1, 30), rng.randint(1, 30)
    if N * H * W < 4:
        N = 4
    dtype, lay_k, sums = rng.choice([torch.float32, torch.bfloat16]), rng.choice([0, 1]), rng.random() < 0.5
    desc = ("bn tail", N, C, H, W, str(dtype), lay_k, sums)
    with _lib.tuned(E, BN_FOLD=1):
        return _asserting(lambda: bn_tail_case(E, N, C, H, W, dtype, lay_k, sums, seed=rng.randint(0, 10 ** 6)), desc)


def case_rowstats(rng):
    """the aggregation forward that emits the following BatchNorm's row sums (agg_nchw.hip ST = 1) + their finalize"""
    from tests.bn_tail_cases import rowstats_case
    C, N = 8 * rng.choice([1, 2, 4, 8, 16, 24]), rng.randint(1, 3)
    H, W = rng.randint(1, 30), rng.choice([2, 4, 5, 7, 8, 10, 14, 16, 20, 28, 30, 40, 56])
    gn = rng.random() < 0.5 and W % 2 == 0
    return _asserting(lambda: rowstats_case(E, N, C, H, W, gn, seed=rng.randint(0, 10 ** 6)), ("rowstats", N, C, H, W, gn))


def case_relu_res(rng):
    """conv1's data gradient with the masked residual gradient added in the epilogue (conv_lds2.hip acc_src / acc_mask)"""
    from tests.bn_tail_cases import relu_res_case
    Ci, Co = 32 * rng.randint(1, 8), 32 * rng.randint(1, 4)
    N, HW = rng.randint(1, 6), 8 * rng.randint(1, 120)
    dt = tke._lib.COT_BF16
    if E.cot_conv1x1_backward_data_relu_res_covers(N, Ci, Co, HW, dt) != 1:
        return True, ("relu res: not covered", N, Ci, Co, HW)
    return _asserting(lambda: relu_res_case(E, N, Ci, Co, HW, seed=rng.randint(0, 10 ** 6)), ("relu res", N, Ci, Co, HW))


CASES_R6 = [case_mix, case_mix, case_stem3x3]
CASES_R6B = [case_bn_tail, case_bn_tail, case_rowstats, case_relu_res]  # (no oracle loop nests: fast)


@pytest.mark.parametrize("seed", [61, 62])
def test_random_shapes_round6_kernels(seed):
    """(300 further cases of this list ran clean offline in round 6)"""
    rng = random.Random(seed)
    torch.manual_seed(seed)
    failures = []
    for _ in range(10):  # (the oracle's loop nest on 2 x 11 x 12 planes is the slow part: 1-2 s per case)
        ok, desc = rng.choice(CASES_R6)(rng)
        if not ok:
            failures.append(desc)
    assert not failures, failures


@pytest.mark.parametrize("seed", [66, 67])
def test_random_shapes_round6_fused_kernels(seed):
    rng = random.Random(seed)
    torch.manual_seed(seed)
    failures = []
    for _ in range(12):
        ok, desc = rng.choice(CASES_R6B)(rng)
        if not ok:
            failures.append(desc)
    assert not failures, failures
