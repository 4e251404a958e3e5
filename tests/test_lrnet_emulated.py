"""Pre-GPU check of csrc/local_relation.hip: the SAME kernels compiled for the host (tests/emul), driven through the C ABI with CPU
pointers and compared with `local_relation_reference` (the reference's composition, models/lr_net.py:82-96) differentiated by
autograd in fp64 on the same (rounded) operands.  The parity gate is tests/test_lrnet_gpu.py on the MI355X."""
import ctypes

import pytest
import torch

import cotnet_amd.aggregation_zeropad as az
from cotnet_amd import _lib
from cotnet_amd.local_relation import local_relation_reference
from oracle import unfold_oracle
from tests.emul import build_emul

try:
    _EMUL = _lib.bind(ctypes.CDLL(build_emul.build()))
except FileNotFoundError:  # no host compiler: the GPU tests still gate parity
    _EMUL = None

pytestmark = pytest.mark.skipif(_EMUL is None, reason="host emulation build unavailable")


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def geom(N, C, H, W, k=3, wC=None):
    return _lib.AggGeom(N, C, H, W, 1, C // 8 if wC is None else wC, k, k, 1, 1, k // 2, k // 2, 1, 1)


def inputs(N, C, H, W, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    q, k, v, gout = (torch.randn(N, C, H, W, generator=g).to(dtype) for _ in range(4))
    pos_h, pos_w = torch.randn(C, 3, 1, generator=g), torch.randn(C, 1, 3, generator=g)
    return q, k, v, gout, pos_h, pos_w


def reference(q, k, v, gout, pos_h, pos_w, monkeypatch):
    """fp64 composition on the same operands, differentiated by autograd: (out, gq, gk, gv, gpos[C][9])"""
    monkeypatch.setattr(az, "aggregation_zeropad", lambda x, w, ks=3, s=1, p=0, d=1: unfold_oracle.aggregation_unfold(x, w, ks, s, p, d))
    q, k, v = (t.double().requires_grad_(True) for t in (q, k, v))
    pos = (pos_h + pos_w).reshape(-1, 9).double().requires_grad_(True)
    out = local_relation_reference(q, k, v, pos.view(-1, 3, 3), torch.zeros(pos.shape[0], 1, 1, dtype=torch.float64), 3)
    out.backward(gout.double())
    return out.detach(), q.grad, k.grad, v.grad, pos.grad


def run_emul(q, k, v, gout, pos):
    N, C, H, W = q.shape
    g = geom(N, C, H, W)
    dt = _lib.dtype_code(q.dtype)
    out, probs = torch.empty_like(v), torch.empty(N, 1, C // 8, 9, H, W, dtype=q.dtype)
    assert _EMUL.cot_local_relation_forward(P(q), P(k), P(v), P(pos), P(out), P(probs), ctypes.byref(g), dt, None) == 0, \
        _EMUL.cot_last_error()
    gq, gk, gv, gpos = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v), torch.empty(C, 9)
    ws = torch.empty(int(_EMUL.cot_local_relation_workspace_bytes(ctypes.byref(g), dt)), dtype=torch.uint8)
    rc = _EMUL.cot_local_relation_backward(P(gout), P(q), P(k), P(v), P(pos), P(probs), P(gq), P(gk), P(gv), P(gpos), P(ws),
                                           ctypes.byref(g), dt, None)
    assert rc == 0, _EMUL.cot_last_error()
    return out, probs, gq, gk, gv, gpos


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [16, 64])
@pytest.mark.parametrize("H", [7, 14])
def test_forward_and_all_gradients_match_the_composition(C, H, dtype, monkeypatch):
    q, k, v, gout, pos_h, pos_w = inputs(2, C, H, H, dtype, seed=C + H)
    q, k = q * 0.5, k * 0.5  # logits of a few units: the softmax is neither flat nor one-hot
    pos = (pos_h + pos_w).reshape(C, 9).contiguous()
    out, _, gq, gk, gv, gpos = run_emul(q, k, v, gout, pos)
    r_out, r_gq, r_gk, r_gv, r_gpos = reference(q, k, v, gout, pos_h, pos_w, monkeypatch)
    tol = 2e-5 if dtype == torch.float32 else 4e-2  # (tests/test_agg_gpu.py::test_fused_window_softmax)
    for name, got, want, f in (("out", out, r_out, 1), ("gv", gv, r_gv, 1), ("gq", gq, r_gq, 4), ("gk", gk, r_gk, 4)):
        err = (got.double() - want).abs()
        assert (err <= f * tol * (1 + want.abs())).all(), (name, err.max().item())
    # gpos sums N * H * W products: measured against the tensor's own scale
    assert (gpos.double() - r_gpos).abs().max().item() <= 4 * tol * max(1.0, r_gpos.abs().max().item()), \
        (gpos - r_gpos.float()).abs().max().item()


def test_results_are_bit_identical_run_to_run():
    q, k, v, gout, pos_h, pos_w = inputs(2, 64, 14, 14, torch.bfloat16, seed=5)
    pos = (pos_h + pos_w).reshape(64, 9).contiguous()
    a = run_emul(q, k, v, gout, pos)
    _EMUL.emul_set_order(2)  # a different lane schedule: the fixed-order reductions must not notice
    try:
        b = run_emul(q, k, v, gout, pos)
    finally:
        _EMUL.emul_set_order(0)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_the_direct_softmax_backward_is_taken_where_the_lds_kernel_is_not():
    """C = 16 at 7 x 7 in fp32: a weight plane group of 2 x 49 floats breaks the LDS kernel's 16-byte rule; gv / gL then come
    from lr_softmax_bwd -- same results as the case above checks, here the route itself"""
    q, k, v, gout, pos_h, pos_w = inputs(1, 16, 7, 7, torch.float32, seed=9)
    run_emul(q, k, v, gout, (pos_h + pos_w).reshape(16, 9).contiguous())
    assert _EMUL.cot_last_kernel().decode().startswith("lr_softmax_bwd")
    q, k, v, gout, pos_h, pos_w = inputs(1, 64, 14, 14, torch.float32, seed=9)
    run_emul(q, k, v, gout, (pos_h + pos_w).reshape(64, 9).contiguous())
    assert _EMUL.cot_last_kernel().decode().startswith("agg_bwd_nchw_k3_lds<softmax>")


@pytest.mark.parametrize("g", [geom(2, 64, 8, 8, k=5), geom(2, 60, 8, 8, wC=15), geom(2, 64, 8, 8, wC=16)],
                         ids=["k5", "C_not_multiple_of_8", "wC_not_C_over_8"])
def test_unsupported_geometry_returns_unsupported(g):
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: the coverage check comes first
    assert _EMUL.cot_local_relation_workspace_bytes(ctypes.byref(g), _lib.COT_F32) == -2
    assert _EMUL.cot_local_relation_forward(fake, fake, fake, fake, fake, fake, ctypes.byref(g), _lib.COT_F32, None) == -2
    assert _EMUL.cot_local_relation_backward(*([fake] * 11), ctypes.byref(g), _lib.COT_F32, None) == -2
    ok = geom(2, 64, 8, 8)
    assert _EMUL.cot_local_relation_forward(fake, fake, fake, fake, fake, fake, ctypes.byref(ok), _lib.COT_F64, None) == -2
