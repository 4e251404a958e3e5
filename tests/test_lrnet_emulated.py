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


# ---- directed edges, against a checker that shares no code with the product: lr_reference64 (tests/test_fuzz_emulated.py), fp64 from
# unfold and einsum.  tests/test_lrnet_gpu.py runs the same functions on the device.
from tests import test_fuzz_emulated as tfe  # noqa: E402

# bf16 gk under a saturated softmax, two bounds from the fp64 reference's own terms (scripts/lr_gk_ratio.py measures both ratios on the
# host emulator, random bf16 cases at q x 6):
#   |gk - want| <= GK_ROUNDING_C (2^-8 R + 1e-30) + 2^-9 |want|     R = sum_t |q| (2 |gL_t| + a_t sum_u a_u |gA_u|)  (tfe.lr_gk_rounding_ratio)
# the first-order effect of rounding each probability to bf16 once and of storing gL in bf16.  Worst ratio over two seeds of 2 400 cases (1.0853, 1.0897):
# GK_ROUNDING_RATIO; GK_ROUNDING_C is twice that.  An indexing error in the gather moves gk by O(|gL q|), some 2^8 / GK_ROUNDING_C times this.
#   |gk - want| <= GK_C 2^-8 S + 2^-9 |want|                        S = sum_t |gL q|                                  (tfe.lr_gk_ratio)
# the form that counts gL's storage rounding alone.  Its ratio has no natural scale (worst 2.86e6 and 1.06e7 over two seeds of 2 400
# cases; GK_C is twice the worst): gL_t = a_t (gA_t - sum_u a_u gA_u) is formed from the rounded probabilities, and the error of that
# difference does not shrink with the true gL_t, so where the softmax saturates S vanishes and the error does not.  It is kept as a
# coarse guard; the first bound is the one that tells a defect from rounding.
GK_ROUNDING_RATIO = 1.0897
GK_ROUNDING_C = 2 * GK_ROUNDING_RATIO
GK_RATIO = 1.06e7
GK_C = 2 * GK_RATIO
SOFTMAX_ROUTE = "lr_softmax_bwd+lr_bwd_rel+lr_gpos_reduce"
LDS_ROUTE = "agg_bwd_nchw_k3_lds<softmax>+lr_bwd_rel+lr_gpos_reduce"
RAGGED = [(5, 100), (3, 85), (1, 1), (40, 6), (9, 30)]  # (5, 100): two rows per tile, a last tile of one row


def lr_directed(N, C, H, W, dtype, qs=0.5, seed=0, skip=()):
    """one geometry through tfe.lr_run (NaN margins, NaN-filled outputs, exact workspace; probs == NULL must give the same bits in out)
    against the fp64 reference at the tolerances of the test above -> (results, reference + gk terms, last_kernel of the backward)"""
    torch.manual_seed(seed)
    q, k, v, gout = (torch.randn(N, C, H, W) for _ in range(4))
    q, k, v, gout = (qs * q).to(dtype), (0.5 * k).to(dtype), v.to(dtype), gout.to(dtype)
    pos = (torch.randn(C, 3, 1) + torch.randn(C, 1, 3)).reshape(C, 9).contiguous()
    got, _, _ = tfe.lr_run(q, k, v, gout, pos, null_probs=True, margin=W + 3)
    kernel = tfe.E.cot_last_kernel().decode()
    want = tfe.lr_reference64(q, k, v, pos, gout, terms=True)
    bad = tfe.lr_mismatches(got, want, dtype, skip)
    assert not bad, (N, C, H, W, dtype, kernel, bad)
    return got, want, kernel


def lds_boundary_case(dtype):
    """25 planes of 3 x (W + 2) floats + 360 floats in 64 KiB: W = 211 is the widest single-row tile, 212 the first refused"""
    dt = _lib.dtype_code(dtype)
    fits = lambda W: (25 * 3 * (W + 2) + 360) * 4 <= 64 * 1024  # noqa: E731
    assert fits(211) and not fits(212)
    assert tfe.E.cot_local_relation_workspace_bytes(ctypes.byref(geom(2, 16, 3, 211)), dt) > 0
    lr_directed(2, 16, 3, 211, dtype, seed=211)
    g, fake = geom(2, 16, 3, 212), ctypes.c_void_p(0x1000)
    assert tfe.E.cot_local_relation_workspace_bytes(ctypes.byref(g), dt) == -2
    assert tfe.E.cot_local_relation_forward(*([fake] * 6), ctypes.byref(g), dt, None) == -2
    assert tfe.E.cot_local_relation_backward(*([fake] * 11), ctypes.byref(g), dt, None) == -2


def backward_routes_case():
    """24 channels at 7 x 9 (three weight planes of 63 floats: off the LDS kernel's 16-byte rule) and at 8 x 12"""
    _, _, kernel = lr_directed(2, 24, 7, 9, torch.float32, seed=1)
    assert kernel == SOFTMAX_ROUTE
    _, _, kernel = lr_directed(2, 24, 8, 12, torch.float32, seed=2)
    assert kernel == LDS_ROUTE
    _, _, kernel = lr_directed(2, 24, 7, 9, torch.bfloat16, seed=3)
    assert kernel == SOFTMAX_ROUTE
    _, _, kernel = lr_directed(2, 24, 8, 12, torch.bfloat16, seed=4)
    assert kernel == LDS_ROUTE


def saturated_case(dtype, H, W, seed=6):
    """q x 6: most pixels put nearly all mass on one tap.  fp32: every output at the usual tolerances.  bf16: out / gv / gq / gpos at the
    usual tolerances, gk within the two bounds above"""
    got, want, _ = lr_directed(2, 24, H, W, dtype, qs=6, seed=seed, skip=("gk",) if dtype == torch.bfloat16 else ())
    if dtype == torch.bfloat16:
        rounding, ratio = tfe.lr_gk_rounding_ratio(got[2], want[2], want[6]), tfe.lr_gk_ratio(got[2], want[2], want[5])
        print(f"saturated bf16 gk at {H} x {W}: ratio to 2^-8 R {rounding:.4f} (bound {GK_ROUNDING_C}), to 2^-8 S {ratio:.4g} (bound {GK_C:g})")
        assert rounding <= GK_ROUNDING_C, (H, W, rounding)
        assert ratio <= GK_C, (H, W, ratio)


def test_misaligned_pointers_are_refused():
    """the C ABI takes 16-byte aligned pointers only (the vector loaders rely on it; the Python wrapper re-aligns its operands): one operand
    one element off the grid is an invalid argument, before any kernel runs"""
    g, buf = geom(1, 8, 4, 12), torch.zeros(8 * 4 * 12 * 9 + 4)
    ok, off = P(buf), ctypes.c_void_p(buf.data_ptr() + 4)
    for i in range(3):
        args = [ok] * 6
        args[i] = off
        assert _EMUL.cot_local_relation_forward(*args, ctypes.byref(g), _lib.COT_F32, None) == -1, i
    assert b"16-byte aligned" in _EMUL.cot_last_error()
    assert _EMUL.cot_local_relation_backward(*([off] + [ok] * 10), ctypes.byref(g), _lib.COT_F32, None) == -1


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_lds_boundary(dtype):
    lds_boundary_case(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H,W", RAGGED)
def test_rectangular_and_ragged_tiles(H, W, dtype):
    lr_directed(2, 24, H, W, dtype, seed=H + W)


def test_both_backward_routes_by_name():
    backward_routes_case()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H,W", [(9, 30), (5, 100), (7, 7), (2, 150)])
def test_saturated_softmax(H, W, dtype):
    saturated_case(dtype, H, W, seed=6)
