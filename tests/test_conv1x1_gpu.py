"""The NCHW-native MFMA 1x1-convolution kernels (csrc/conv1x1.hip behind cot_conv1x1_*, opt-in COT_CONV1X1=hip) on the
GPU against torch's own convolution evaluated in fp32 on the same bf16-rounded operands; composed blocks against an
fp32 truth (tests/truth.py)."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from cotnet_amd import conv1x1 as c1

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ref(xs, w, b, gy):
    """fp32 autograd reference on the bf16-rounded values; xs = list of channel slabs"""
    rs = [x.detach().float().requires_grad_(True) for x in xs]
    wf = w.detach().float().requires_grad_(True)
    bf = b.detach().float().requires_grad_(True) if b is not None else None
    y = F.conv2d(torch.cat(rs, 1) if len(rs) > 1 else rs[0], wf, bf)
    y.backward(gy.float())
    return y.detach(), [r.grad for r in rs], wf.grad, (bf.grad if bf is not None else None)


def _close(a, b, rel):
    # bf16 outputs of fp32-accumulated sums: error <= half an ulp of the result (2^-9 relative) + accumulation-order noise
    return ((a.float() - b).abs() <= rel * (b.abs() + b.abs().mean())).all()


# (N, Ci, Co, H, split, bias): the CoTNet-50 layer shapes (models/cotnet.py:51-62,:206-224) at a small batch + odd ones
CASES = [
    (4, 256, 64, 56, 0, False),    # Bottleneck.conv1, stage 1
    (4, 128, 32, 56, 64, False),   # CotLayer.embed[0] on [x | k]
    (4, 32, 72, 56, 0, True),      # CotLayer.embed[3] (bias; Co = 72)
    (4, 64, 64, 56, 0, False),     # CotLayer.conv1x1[0]
    (4, 64, 256, 56, 0, False),    # Bottleneck.conv3, stage 1
    (4, 128, 512, 28, 0, False),
    (4, 512, 128, 28, 256, False),
    (3, 256, 1024, 14, 0, False),  # 14x14: 8-byte pieces
    (3, 128, 288, 14, 0, True),
    (3, 512, 2048, 7, 0, False),   # 7x7: unaligned rows
    (3, 1024, 256, 7, 512, False),
    (2, 24, 40, 5, 8, True),       # nothing aligned, partial K step
    (1, 8, 8, 1, 0, False),        # a single pixel
]


@pytest.mark.parametrize("N,Ci,Co,H,split,bias", CASES)
def test_matches_torch_convolution(N, Ci, Co, H, split, bias, monkeypatch):
    monkeypatch.setattr(c1, "MODE", "hip")
    torch.manual_seed(Ci + Co + H)
    conv = nn.Conv2d(Ci, Co, 1, bias=bias).to(DEV).bfloat16()
    x = torch.randn(N, Ci, H, H, device=DEV).bfloat16()
    xs = [x[:, :split].contiguous(), x[:, split:].contiguous()] if split else [x]
    xs = [t.requires_grad_(True) for t in xs]
    gy = torch.randn(N, Co, H, H, device=DEV).bfloat16()
    assert c1.eligible_hip(conv, *xs)
    y = c1.conv1x1(conv, *xs)
    y.backward(gy)
    torch.cuda.synchronize()
    yr, gxr, gwr, gbr = _ref(xs, conv.weight, conv.bias, gy)
    assert _close(y, yr, 1e-2)
    for t, r in zip(xs, gxr):
        assert _close(t.grad, r, 1e-2)
    assert _close(conv.weight.grad, gwr, 1e-2)
    if bias:
        assert _close(conv.bias.grad, gbr, 1e-2)


def test_weight_gradient_is_deterministic(monkeypatch):
    monkeypatch.setattr(c1, "MODE", "hip")
    torch.manual_seed(0)
    conv = nn.Conv2d(64, 256, 1, bias=False).to(DEV).bfloat16()
    x = torch.randn(16, 64, 56, 56, device=DEV).bfloat16()
    gy = torch.randn(16, 256, 56, 56, device=DEV).bfloat16()
    grads = []
    for _ in range(3):
        conv.weight.grad = None
        c1.conv1x1(conv, x).backward(gy)
        grads.append(conv.weight.grad.clone())
    assert torch.equal(grads[0], grads[1]) and torch.equal(grads[0], grads[2])


def test_cot_layer_and_bottleneck_with_hip_convolutions():
    """whole Bottleneck forward+backward with COT_CONV1X1=hip: its distance from an fp32 evaluation of the same block
    must not exceed the default (MIOpen) path's distance (round 1 compared the two bf16 paths with each other at a 3 %
    bar -- below the bf16 noise floor of a BatchNorm block, whose input gradient sits ~10 % from the fp32 truth)"""
    from cotnet_amd.cotnet import Bottleneck
    from cotnet_amd.flat_sgd import to_mixed_bf16
    from tests import truth
    torch.manual_seed(1)
    ds = nn.Sequential(nn.Identity(), nn.Conv2d(128, 256, 1, bias=False), nn.BatchNorm2d(256))
    blk = to_mixed_bf16(Bottleneck(128, 64, downsample=ds).to(DEV)).train()
    with torch.no_grad():
        blk.bn3.weight.fill_(1.0)  # zero-init would hide conv3
    x = torch.randn(4, 128, 28, 28, device=DEV).bfloat16()
    gy = torch.randn(4, 256, 28, 28, device=DEV).bfloat16()
    rep = truth.check_against_truth(blk, x, gy, cand=dict(truth.ROUND1, conv1x1="hip"))
    print({k: (round(a, 4), round(b, 4)) for k, (a, b) in rep.items() if k in ("y", "gx")})


# every 1x1 shape of that Bottleneck / CotLayer(64) at 28x28 plus the se convolutions on a 1x1 map (verdict r1: the
# composed block uses shapes the op-level list did not have), with the workspace poisoned
BLOCK_CASES = [(4, 128, 64, 28, 0, False), (4, 64, 256, 28, 0, False), (4, 128, 256, 28, 0, False),
               (4, 128, 32, 28, 64, False), (4, 32, 72, 28, 0, True), (4, 64, 64, 28, 0, False),
               (1, 64, 32, 2, 0, True), (1, 32, 128, 2, 0, True)]


@pytest.mark.parametrize("N,Ci,Co,H,split,bias", BLOCK_CASES)
def test_block_shapes_with_poisoned_workspace(N, Ci, Co, H, split, bias, monkeypatch):
    monkeypatch.setattr(c1, "MODE", "hip")
    torch.manual_seed(Ci * 3 + Co + H)
    conv = nn.Conv2d(Ci, Co, 1, bias=bias).to(DEV).bfloat16()
    x = torch.randn(N, Ci, H, H, device=DEV).bfloat16()
    xs = [x[:, :split].contiguous(), x[:, split:].contiguous()] if split else [x]
    xs = [t.requires_grad_(True) for t in xs]
    gy = torch.randn(N, Co, H, H, device=DEV).bfloat16()
    real_empty = torch.empty

    def poisoned(*a, **k):  # every workspace / output the wrapper allocates starts as NaN (bytes 0xFF)
        t = real_empty(*a, **k)
        if t.is_cuda and t.numel():
            t.view(torch.uint8).fill_(0xFF)
        return t

    monkeypatch.setattr(torch, "empty", poisoned)
    y = c1.conv1x1(conv, *xs)
    y.backward(gy)
    monkeypatch.setattr(torch, "empty", real_empty)
    torch.cuda.synchronize()
    yr, gxr, gwr, gbr = _ref(xs, conv.weight, conv.bias, gy)
    assert _close(y, yr, 1e-2)
    for t, r in zip(xs, gxr):
        assert _close(t.grad, r, 1e-2)
    assert _close(conv.weight.grad, gwr, 1e-2)
    if bias:
        assert _close(conv.bias.grad, gbr, 1e-2)


def test_other_inputs_keep_the_module_path(monkeypatch):
    monkeypatch.setattr(c1, "MODE", "hip")
    conv = nn.Conv2d(16, 16, 1).to(DEV)
    x = torch.randn(2, 16, 8, 8, device=DEV)
    assert not c1.eligible_hip(conv, x) and c1.eligible_general(conv, x)    # fp32: the general kernels (conv_gen.hip)
    assert torch.allclose(c1.conv1x1(conv, x), conv(x), atol=1e-5, rtol=1e-5)
    xh = x.half()
    assert not c1.eligible_general(conv.half(), xh)          # fp16: the module
    assert torch.equal(c1.conv1x1(conv, xh), conv(xh))
    conv = conv.float()
    convb = nn.Conv2d(12, 16, 1).to(DEV).bfloat16()
    assert not c1.eligible_hip(convb, torch.zeros(2, 12, 8, 8, device=DEV).bfloat16())   # Ci % 8 != 0
    convs = nn.Conv2d(16, 16, 1, stride=2).to(DEV).bfloat16()
    assert not c1.eligible_hip(convs, x.bfloat16())


@pytest.mark.parametrize("N,Ci,Co,H", [(6, 512, 2048, 7), (6, 2048, 512, 7), (5, 256, 1024, 14)])
def test_deep_layers_with_both_channel_block_sizes(N, Ci, Co, H, monkeypatch):
    """the 7 x 7 / 14 x 14 layers run 64-channel blocks when a launch has few workgroups (the small batches of these tests
    always do) and 128-channel blocks otherwise (B = 80): both forms (cot_set_tuning(CONV_LDS_BITS) bits 8..) against the fp32
    reference (the two walk K from different staggered starting steps, so they agree to rounding, not bit for bit)"""
    from cotnet_amd import _lib
    monkeypatch.setattr(c1, "MODE", "hip")
    torch.manual_seed(Ci + H)
    conv = nn.Conv2d(Ci, Co, 1, bias=False).to(DEV).bfloat16()
    x = torch.randn(N, Ci, H, H, device=DEV).bfloat16()
    gy = torch.randn(N, Co, H, H, device=DEV).bfloat16()
    outs = []
    for key in (0, 256):
        with _lib.tuned(_lib.lib(), CONV_LDS_BITS=key):
            xi = x.clone().requires_grad_(True)
            conv.zero_grad()
            y = c1.conv1x1(conv, xi)
            y.backward(gy)
            outs.append((y.detach().clone(), xi.grad.clone(), conv.weight.grad.clone()))
    yr, gxr, gwr, _ = _ref([x], conv.weight, None, gy)
    for y, gx, gw in outs:
        assert _close(y, yr, 1e-2) and _close(gx, gxr[0], 1e-2) and _close(gw, gwr, 1e-2)
    assert _close(outs[0][0], outs[1][0].float(), 1e-2) and _close(outs[0][1], outs[1][1].float(), 1e-2)


@pytest.mark.parametrize("Ci,Co,NB", [(64, 32, 80), (32, 128, 80), (512, 256, 80), (256, 1024, 80), (128, 64, 24), (72, 40, 250)])
def test_one_image_convolutions_of_the_se_branch(Ci, Co, NB, monkeypatch):
    """the `se` branch's two 1x1 convolutions as the single-node layers issue them: ONE image whose pixels are the batch
    (csrc/conv_tiny.hip: a wave per 16 x 16 output tile, no LDS), against the fp32 reference, and the tiled kernels next to
    them (cot_set_tuning(_lib.TUNE.CONV_TINY, 0))"""
    from cotnet_amd import _lib
    monkeypatch.setattr(c1, "MODE", "hip")
    torch.manual_seed(Ci + Co)
    conv = nn.Conv2d(Ci, Co, 1, bias=True).to(DEV).bfloat16()
    x = torch.randn(1, Ci, 1, NB, device=DEV).bfloat16()
    gy = torch.randn(1, Co, 1, NB, device=DEV).bfloat16()
    yr, gxr, gwr, gbr = _ref([x], conv.weight, conv.bias, gy)
    for key in (1, 0):
        with _lib.tuned(_lib.lib(), CONV_TINY=key):
            xi = x.clone().requires_grad_(True)
            conv.zero_grad()
            y = c1.conv1x1(conv, xi)
            y.backward(gy)
            torch.cuda.synchronize()
            assert _close(y, yr, 1e-2) and _close(xi.grad, gxr[0], 1e-2)
            assert _close(conv.weight.grad, gwr, 1e-2) and _close(conv.bias.grad, gbr, 1e-2)


@pytest.mark.parametrize("N,Ci,Co,H", [(64, 48, 48, 56), (64, 96, 24, 56), (64, 96, 48, 28), (64, 96, 216, 14), (64, 192, 432, 7),
                                       (80, 32, 72, 56), (80, 64, 144, 28), (3, 24, 56, 28), (5, 40, 72, 20), (7, 56, 120, 7), (2, 8, 16, 16)])
def test_partial_last_k_step_on_the_lds_kernels(N, Ci, Co, H):
    """reduction depths on the 8-channel grid but off the 32-row K step -- one group of CoXtLayer's grouped 1x1s at the benchmark batch
    (models/cotnet.py:118-135: 48 -> 48, 96 -> 24 | 48, 96 -> 216, 192 -> 432 per group), CotLayer.embed[3]'s data gradient (72 / 144) and small
    ragged ones: conv_lds2.hip's KT instantiations through the C ABI, operands inside NaN margins, against torch in fp32 on the rounded
    operands and against the first-generation kernel (tuning key 54 = 0)"""
    import ctypes

    from cotnet_amd import _lib
    L = _lib.lib()
    torch.manual_seed(Ci + Co)
    HW, dt = H * H, _lib.COT_BF16
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def margined(t, m):
        flat = torch.full((t.numel() + 2 * m,), float("nan"), dtype=t.dtype, device=DEV)
        v = flat[m:m + t.numel()].view(t.shape)
        v.copy_(t)
        return v
    x, gy = margined(torch.randn(N, Ci, H, H, device=DEV).bfloat16(), 8), margined(torch.randn(N, Co, H, H, device=DEV).bfloat16(), 16)
    w = margined((torch.randn(Co, Ci, device=DEV) * Ci ** -0.5).bfloat16(), 8)
    ws = torch.empty(max(int(L.cot_conv1x1_workspace(N, Ci, Co, HW, 0)), 256), dtype=torch.uint8, device=DEV)
    yr = torch.einsum("oc,nchw->nohw", w.float(), x.float())
    gr = torch.einsum("oc,nohw->nchw", w.float(), gy.float())
    init = torch.randn(N, Ci, H, H, device=DEV).bfloat16()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    outs = {}
    for k54 in (1, 0):
        with _lib.tuned(L, CONV_K_TAIL=k54):
            y, gx, ga = torch.full_like(gy, float("nan")), torch.full_like(x, float("nan")), init.clone()
            assert L.cot_conv1x1_forward(P(x), None, Ci, P(w), None, P(y), N, Ci, Co, HW, dt, st) == 0, L.cot_last_error()
            assert L.cot_conv1x1_backward_data(P(gy), P(w), P(gx), None, Ci, 0, P(ws), N, Ci, Co, HW, dt, st) == 0, L.cot_last_error()
            assert L.cot_conv1x1_backward_data(P(gy), P(w), P(ga), None, Ci, 1, P(ws), N, Ci, Co, HW, dt, st) == 0, L.cot_last_error()
            torch.cuda.synchronize()
            outs[k54] = (y, gx, ga)
    assert L.cot_conv1x1_lds_covers(Ci, Ci, 0, HW) == 1 and L.cot_conv1x1_lds_covers(Co, Co, 0, HW) == 1
    y, gx, ga = outs[1]
    assert _close(y, yr, 2e-2) and _close(gx, gr, 2e-2) and _close(ga, gr + init.float(), 3e-2)
    for a, b, ref in zip(outs[1], outs[0], (yr, gr, gr)):
        assert (a.float() - b.float()).abs().max() <= 2e-2 * ref.abs().max()
