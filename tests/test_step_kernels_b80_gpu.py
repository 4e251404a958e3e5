"""Element-wise parity AT THE BENCHMARK BATCH (B = 80), through the C ABI, of the kernels of the measured step that
tests/test_dispatch_parity_gpu.py does not key:

  * cot_bn_act_forward_mask / _backward_mask  -- bn3 + residual + ReLU with the 1-bit sign mask: runs in every Bottleneck
    (models/cotnet.py:248-262); against fp32 torch relu(bn(x) + res) AND bit-identical with the unmasked entry points;
  * cot_bn_act_forward_ps / _backward_ps      -- the same with the per-sample stochastic-depth scale (models/cotnet.py:256-257);
  * cot_radix_gap_t / cot_radix_mix_logits / cot_radix_mix_backward_reduce / _apply -- the radix-2 tail (models/cotnet.py:92-104)
    at the four stage geometries (80, 64, 56) ... (80, 512, 7);
  * cot_stem7x7s2_forward / _backward_weight at N = 80 (models/resnet.py:539-555);
  * cot_agg_gn9_forward / _backward at both fused stages against the ORACLE on GroupNorm-ed weights (the unfused HIP composition is
    compared bit for bit in tests/test_gn_fusion_gpu.py).
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from cotnet_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = _lib.COT_BF16
B = 80


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _close(a, b, rel=1e-2):
    b = b.float()
    bad = (a.float() - b).abs() > rel * (b.abs() + b.abs().mean())
    assert not bad.any(), (int(bad.sum()), (a.float() - b).abs().max().item(), b.abs().mean().item())


def _rel(a, b, rel):
    b = b.float()
    e = (a.float() - b).abs().max().item()
    assert e <= rel * (b.abs().max().item() + 1e-6), (e, b.abs().max().item())


def _randn(*shape, seed=0, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, device=DEV, generator=g) * scale).bfloat16()


@pytest.fixture(autouse=True)
def _bench_tuning():
    with _lib.tuned(_lib.lib(), BN_FOLD=1):  # (bench.py's `new` set: finalize folded into the apply kernels)
        yield


# bn3 of every stage of CoTNet-50 at B = 80: (channels, plane)
BN3 = [(256, 3136), (512, 784), (1024, 196), (2048, 49)]


def _bn_operands(C, HW, seed):
    x = (_randn(B, C, HW, 1, seed=seed).float() * 1.5 + 0.25).bfloat16()
    res = _randn(B, C, HW, 1, seed=seed + 1)
    gamma = (torch.rand(C, device=DEV) + 0.5).float()
    beta = (torch.randn(C, device=DEV) * 0.2).float()
    return x, res, gamma, beta


def _bn_forward(L, entry, x, res, gamma, beta, C, HW, mask=None, ps=None):
    mean, rstd = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    ws = torch.full((max(int(L.cot_bn_act_workspace(B, C)), 1),), float("nan"), device=DEV)
    y = torch.full((B, C, HW, 1), float("nan"), device=DEV).bfloat16()
    if entry == "mask":
        rc = L.cot_bn_act_forward_mask(P(x), P(res), P(y), P(mask), P(gamma), P(beta), P(mean), P(rstd), P(rm), P(rv), P(nbt), P(ws),
                                       P(ps), B, C, HW, 1e-5, 0.1, 1, BF, _st())
    else:
        rc = L.cot_bn_act_forward_ps(P(x), P(res), P(y), P(gamma), P(beta), P(mean), P(rstd), P(rm), P(rv), P(nbt), P(ws), P(ps), B, C,
                                     HW, 1e-5, 0.1, 1, BF, _st())
    assert rc == 0, L.cot_last_error().decode()
    return y, mean, rstd, rm, rv


def _bn_backward(L, entry, dy, x, y_or_mask, gamma, beta, mean, rstd, C, HW, ps=None):
    dx, dres = (torch.full((B, C, HW, 1), float("nan"), device=DEV).bfloat16() for _ in range(2))
    dg, db = torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
    ws = torch.full((max(int(L.cot_bn_act_workspace(B, C)), 1),), float("nan"), device=DEV)
    fn = L.cot_bn_act_backward_mask if entry == "mask" else L.cot_bn_act_backward_ps
    rc = fn(P(dy), P(x), P(y_or_mask), P(dx), P(dres), P(gamma), P(beta), P(mean), P(rstd), P(dg), P(db), P(ws), P(ps), B, C, HW, 1, BF,
            _st())
    assert rc == 0, L.cot_last_error().decode()
    return dx, dres, dg, db


@pytest.mark.parametrize("C,HW", BN3, ids=[f"{c}x{hw}" for c, hw in BN3])
@pytest.mark.parametrize("drop", [False, True], ids=["plain", "drop_path"])
def test_bn3_residual_relu_with_the_sign_mask(C, HW, drop):
    L = _lib.lib()
    x, res, gamma, beta = _bn_operands(C, HW, seed=C + HW)
    ps = None
    if drop:  # stochastic depth: a sample's branch is dropped (0) or scaled by 1 / keep
        keep = 0.8
        ps = (torch.rand(B, device=DEV) < keep).float() / keep
    nb = int(L.cot_bn_relu_mask_bytes(B, C, HW, BF))
    assert (nb > 0) == (HW % 8 == 0), "planes that are multiples of 8 elements take the mask form, 7 x 7 planes the saved output"
    y, mean, rstd, rm, rv = _bn_forward(L, "ps", x, res, gamma, beta, C, HW, ps=ps)
    if nb:
        mask = torch.full((nb,), 0xAA, dtype=torch.uint8, device=DEV)
        y2, mean2, rstd2, rm2, rv2 = _bn_forward(L, "mask", x, res, gamma, beta, C, HW, mask=mask, ps=ps)
        torch.cuda.synchronize()
        # (1) the mask form IS the _ps form: same kernels, one more store
        assert torch.equal(y, y2) and torch.equal(mean, mean2) and torch.equal(rstd, rstd2) and torch.equal(rm, rm2) and torch.equal(rv, rv2)
        # (2) the mask is the sign of the rounded output, bit k of byte i = element 8 i + k
        bits = (y.flatten() > 0).view(-1, 8).to(torch.uint8)
        packed = (bits << torch.arange(8, device=DEV, dtype=torch.uint8)).sum(1).to(torch.uint8)
        assert torch.equal(mask[: packed.numel()], packed)
    # (3) against fp32 torch on the same bf16 operands
    xr = x.float().requires_grad_(True)
    rr = res.float().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm_r, rv_r = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    z = F.batch_norm(xr, rm_r, rv_r, gr, br, True, 0.1, 1e-5)
    if drop:
        z = z * ps.view(B, 1, 1, 1)
    yr = F.relu(z + rr)
    _close(y, yr.detach())
    _rel(mean, xr.detach().mean((0, 2, 3)), 1e-4)
    _rel(rm, rm_r, 1e-3)
    _rel(rv, rv_r, 1e-3)
    # ---- backward
    dy = _randn(B, C, HW, 1, seed=C + HW + 7)
    dx, dres, dg, db = _bn_backward(L, "ps", dy, x, y, gamma, beta, mean, rstd, C, HW, ps=ps)
    if nb:
        dx2, dres2, dg2, db2 = _bn_backward(L, "mask", dy, x, mask, gamma, beta, mean, rstd, C, HW, ps=ps)
        torch.cuda.synchronize()
        assert torch.equal(dx, dx2) and torch.equal(dres, dres2) and torch.equal(dg, dg2) and torch.equal(db, db2)
    # the kernels' ReLU mask is the sign of THEIR rounded output (where the pre-activation is within a rounding of zero the fp32
    # reference may decide differently, and with 3920 samples per channel a handful of such decisions moves dgamma by more than the
    # bar): the reference differentiates relu with the kernel's own sign decisions, so every element and every sum is comparable
    sign = (y.float() > 0).float()
    agree = ((z + rr).detach() > 0).float() == sign
    assert (~agree).float().mean().item() < 0.01
    ((z + rr) * sign).backward(dy.float())
    for got, ref in ((dx, xr.grad), (dres, rr.grad)):
        d = (got.float() - ref).abs()
        assert (d <= 1e-2 * (ref.abs() + ref.abs().mean())).all(), d.max().item()
    _rel(dg, gr.grad, 2e-3)
    _rel(db, br.grad, 2e-3)


STAGES = [(64, 56), (128, 28), (256, 14), (512, 7)]


@pytest.mark.parametrize("C,H", STAGES, ids=[f"{c}x{h}" for c, h in STAGES])
def test_radix_tail_kernels(C, H):
    """gapT = mean_hw(y + k) [C][N]; attn = softmax over the pair of logitsT[2c], logitsT[2c + 1]; out = y a0 + k a1; backward in two
    launches around the `se` branch (models/cotnet.py:92-104)"""
    L, HW, st = _lib.lib(), H * H, _st()
    y, k = _randn(B, C, HW, seed=C), _randn(B, C, HW, seed=C + 1)
    gapT = torch.full((C, B), float("nan"), device=DEV).bfloat16()
    assert L.cot_radix_gap_t(P(y), P(k), P(gapT), B, C, HW, BF, st) == 0, L.cot_last_error().decode()
    _close(gapT, (y.float() + k.float()).mean(2).t(), 5e-3)
    head = torch.full((C, B), float("nan"), device=DEV).bfloat16()  # (k == NULL: the classifier head's pooling)
    assert L.cot_radix_gap_t(P(y), None, P(head), B, C, HW, BF, st) == 0
    _close(head, y.float().mean(2).t(), 5e-3)

    logitsT = _randn(2 * C, B, seed=C + 2)
    out = torch.full((B, C, HW), float("nan"), device=DEV).bfloat16()
    attn = torch.full((B, C, 2), float("nan"), device=DEV).bfloat16()
    assert L.cot_radix_mix_logits(P(y), P(k), P(logitsT), P(out), P(attn), B, C, HW, BF, st) == 0, L.cot_last_error().decode()
    yr, kr = y.float().requires_grad_(True), k.float().requires_grad_(True)
    lr = logitsT.float().requires_grad_(True)
    ar = torch.softmax(lr.view(C, 2, B).permute(2, 0, 1), dim=2)           # [B][C][2]
    outr = yr * ar[:, :, 0:1] + kr * ar[:, :, 1:2]
    _close(attn, ar.detach(), 1e-2)
    _close(out, outr.detach())

    g = _randn(B, C, HW, seed=C + 3)
    glog = torch.full((2 * C, B), float("nan"), device=DEV).bfloat16()
    assert L.cot_radix_mix_backward_reduce(P(g), P(y), P(k), P(attn), P(glog), B, C, HW, BF, st) == 0, L.cot_last_error().decode()
    ggapT = _randn(C, B, seed=C + 4)
    gy, gk = (torch.full((B, C, HW), float("nan"), device=DEV).bfloat16() for _ in range(2))
    assert L.cot_radix_mix_backward_apply(P(g), P(attn), P(ggapT), P(gy), P(gk), B, C, HW, BF, st) == 0, L.cot_last_error().decode()
    # reference: the mix with the attention the KERNEL saved (bf16) so that both sides differentiate the same function
    a_saved = attn.float()
    gl_ref = torch.empty(2 * C, B, device=DEV)
    sy, sk = (g.float() * y.float()).sum(2), (g.float() * k.float()).sum(2)  # [B][C]
    d = a_saved[:, :, 0] * a_saved[:, :, 1] * (sy - sk)
    gl_ref[0::2], gl_ref[1::2] = d.t(), -d.t()
    _close(glog, gl_ref, 2e-2)
    add = ggapT.float().t().unsqueeze(2) / HW
    _close(gy, g.float() * a_saved[:, :, 0:1] + add)
    _close(gk, g.float() * a_saved[:, :, 1:2] + add)


def test_stem_convolution_at_the_benchmark_batch():
    L, st = _lib.lib(), _st()
    H = 224
    x = _randn(B, 3, H, H, seed=1)
    w = _randn(64, 3, 7, 7, seed=2, scale=(3 * 49) ** -0.5)
    y = torch.full((B, 64, 112, 112), float("nan"), device=DEV).bfloat16()
    assert L.cot_stem7x7s2_forward(P(x), P(w), P(y), B, H, H, BF, st) == 0, L.cot_last_error().decode()
    _close(y, F.conv2d(x.float(), w.float(), None, 2, 3))
    gy = _randn(B, 64, 112, 112, seed=3)
    ws = torch.empty(int(L.cot_stem7x7s2_workspace(B, H, H)), dtype=torch.uint8, device=DEV)
    ws.fill_(0xFF)
    gw = torch.full((64, 3, 7, 7), float("nan"), device=DEV).bfloat16()
    assert L.cot_stem7x7s2_backward_weight(P(gy), P(x), P(gw), P(ws), B, H, H, BF, st) == 0, L.cot_last_error().decode()
    ref = torch.nn.grad.conv2d_weight(x.float(), (64, 3, 7, 7), gy.float(), 2, 3)
    _close(gw, ref)


@pytest.mark.parametrize("C,H", [(64, 56), (128, 28), (256, 14), (512, 7)], ids=["64x56", "128x28", "256x14", "512x7"])
def test_aggregation_with_groupnorm_prologue_against_the_oracle(C, H):
    """cot_agg_gn9_*: weights = GroupNorm-9(logits) applied in the kernels' prologue.  Oracle: oracle/agg_oracle.c on the weight
    tensor csrc/group_norm9.hip writes for the same logits / statistics (itself keyed in the dispatch walk)."""
    from oracle import cref
    L, st = _lib.lib(), _st()
    HW, G, Ce = H * H, C // 8, 9 * C // 8
    if L.cot_gn9_fused_covers(C // 2, C // 2, 0, HW, H) != 1:
        pytest.skip("this geometry composes the three ops (cot_gn9_fused_covers == 0)")
    logits = _randn(B, Ce, H, H, seed=C)
    gamma, beta = (1 + 0.3 * torch.randn(Ce, device=DEV)).bfloat16(), (0.2 * torch.randn(Ce, device=DEV)).bfloat16()
    wn = torch.empty_like(logits)
    mean, rstd = torch.empty(B * G, device=DEV), torch.empty(B * G, device=DEV)
    assert L.cot_group_norm9_forward(P(logits), P(gamma), P(beta), P(wn), P(mean), P(rstd), B, Ce, HW, 1e-5, BF, st) == 0
    v, go = _randn(B, C, H, H, seed=C + 1), _randn(B, C, H, H, seed=C + 2)
    geo = _lib.AggGeom(B, C, H, H, 1, G, 3, 3, 1, 1, 1, 1, 1, 1)
    out = torch.full((B, C, H, H), float("nan"), device=DEV).bfloat16()
    assert L.cot_agg_gn9_forward(P(v), P(logits), P(mean), P(rstd), P(gamma), P(beta), G, P(out), ctypes.byref(geo), BF, st) == 0, \
        L.cot_last_error().decode()
    gx = torch.full((B, C, H, H), float("nan"), device=DEV).bfloat16()
    gw = torch.full((B, Ce, H, H), float("nan"), device=DEV).bfloat16()
    assert L.cot_agg_gn9_backward(P(go), P(v), P(logits), P(mean), P(rstd), P(gamma), P(beta), G, P(gx), P(gw), ctypes.byref(geo), BF,
                                  st) == 0, L.cot_last_error().decode()
    torch.cuda.synchronize()
    x_c, w_c, g_c = v.float().cpu(), wn.float().cpu().view(B, 1, G, 9, H, H), go.float().cpu()
    for got, ref in ((out, cref.forward(x_c, w_c, 3, 1, 1, 1)), (gx, cref.backward_input(g_c, w_c, x_c.shape, 3, 1, 1, 1)),
                     (gw.view(B, 1, G, 9, H, H), cref.backward_weight(g_c, x_c, w_c.shape, 3, 1, 1, 1))):
        got = got.float().cpu()
        assert ((got - ref).abs() <= 2.0 ** -8 * ref.abs() + 1e-5 * (1 + ref.abs().mean())).all(), (got - ref).abs().max().item()
