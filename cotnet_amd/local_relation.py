"""LR-Net's local relation (models/lr_net.py:82-96) on fused HIP kernels (csrc/local_relation.hip, include/cotnet_amd.h).

    local_relation(q, k, v, pos_h, pos_w, kernel_size)
        = aggregation_zeropad(v, softmax_t(sum_{8 channels} q * (unfold(k) + pos_h + pos_w)))

with G = C/8 heads of 8 consecutive q/k channels and the weights of channel c taken from head c mod G (:89-96).  `pos` is
formed here in torch, so pos_h / pos_w stay ordinary differentiable parameters (kept in fp32 by to_mixed_bf16); the fused
op takes it as fp32 [C][k k] and returns its gradient in fp32.

Route: the fused autograd Function for CUDA fp32 / bf16 tensors at k = 3 (the reference's two builders) or k = 7 (LR-Net's own
window, csrc/local_relation7.hip) whose geometry the library covers (C % 8 == 0, a tile that fits LDS).  Everything else -- CPU
tensors, fp64, any other window -- takes `local_relation_reference`, the reference's composition (unfold, + pos, product, head
sum, aggregation_zeropad_softmax).  A CUDA fp32 / bf16 tensor at k = 3 or 7 that the kernels do not cover is counted as a module
fallback (COT_STRICT_DISPATCH=1 makes it an error).
"""
import ctypes

import torch
import torch.nn.functional as F
from torch.autograd import Function

from . import _lib
from ._lib import ptr as _ptr, stream as _stream
from .aggregation_zeropad import _aligned, aggregation_zeropad_softmax

_DT = (torch.float32, torch.bfloat16)
_FUSED_WINDOWS = (3, 7)
_WS = _lib.register_cache({})  # ((N, C, H, W), dtype, window) -> workspace bytes (< 0: geometry off the fused kernels)


def _geom(q, kernel_size):
    N, C, H, W = q.shape
    return _lib.AggGeom(N, C, H, W, 1, C // 8, kernel_size, kernel_size, 1, 1, kernel_size // 2, kernel_size // 2, 1, 1)


def _ws_bytes(q, kernel_size):
    key = (tuple(q.shape), q.dtype, kernel_size)
    if key not in _WS:
        _WS[key] = int(_lib.lib().cot_local_relation_workspace_bytes(ctypes.byref(_geom(q, kernel_size)), _lib.dtype_code(q.dtype)))
    return _WS[key]


def _pos(pos_h, pos_w, kernel_size):
    """pos[c][k i + j] = pos_h[c][i][0] + pos_w[c][0][j]  (:87-88)"""
    return (pos_h + pos_w).reshape(pos_h.shape[0], kernel_size * kernel_size)


class _LocalRelation(Function):
    @staticmethod
    def forward(ctx, q, k, v, pos, kernel_size):
        q, k, v = (_aligned(t.detach().contiguous()) for t in (q, k, v))
        pos_dtype = pos.dtype
        pos = pos.detach().float().contiguous()
        N, C, H, W = q.shape
        geom = _geom(q, kernel_size)
        out = torch.empty_like(v)
        probs = torch.empty((N, 1, C // 8, kernel_size * kernel_size, H, W), dtype=q.dtype, device=q.device)
        _lib.api().cot_local_relation_forward(_ptr(q), _ptr(k), _ptr(v), _ptr(pos), _ptr(out), _ptr(probs),
                                              ctypes.byref(geom), _lib.dtype_code(q.dtype), _stream())
        ctx.geom, ctx.pos_dtype, ctx.kernel_size = geom, pos_dtype, kernel_size
        ctx.save_for_backward(q, k, v, pos, probs)
        return out

    @staticmethod
    def backward(ctx, gout):
        q, k, v, pos, probs = ctx.saved_tensors
        gout = _aligned(gout.contiguous())
        gq, gk, gv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        gpos = torch.empty_like(pos)
        ws = torch.empty(_ws_bytes(q, ctx.kernel_size), dtype=torch.uint8, device=q.device)
        _lib.api().cot_local_relation_backward(_ptr(gout), _ptr(q), _ptr(k), _ptr(v), _ptr(pos), _ptr(probs), _ptr(gq),
                                               _ptr(gk), _ptr(gv), _ptr(gpos), _ptr(ws), ctypes.byref(ctx.geom),
                                               _lib.dtype_code(q.dtype), _stream())
        return gq, gk, gv, gpos.to(ctx.pos_dtype), None


def local_relation_reference(q, k, v, pos_h, pos_w, kernel_size):
    """the reference's composition (:82-96): unfold(k) + pos, product with q, sum over each head's 8 channels, then the
    window softmax and the aggregation (aggregation_zeropad_softmax)"""
    B, C, H, W = q.shape
    T = kernel_size * kernel_size
    G = C // 8
    uk = F.unfold(k, kernel_size, 1, kernel_size // 2, 1).view(B, C, T, H, W)
    kp = uk + _pos(pos_h, pos_w, kernel_size).view(1, C, T, 1, 1)
    attn = (q.view(B, G, -1, 1, H, W) * kp.view(B, G, -1, T, H, W)).sum(2)
    w = attn.view(B, 1, -1, T, H, W).to(v.dtype)
    return aggregation_zeropad_softmax(v, w, kernel_size, 1, (kernel_size - 1) // 2, 1)


def fusable(q, k, v, kernel_size):
    return (q.is_cuda and kernel_size in _FUSED_WINDOWS and q.dim() == 4 and q.dtype in _DT and k.dtype == q.dtype
            and v.dtype == q.dtype and k.shape == q.shape and v.shape == q.shape and q.shape[1] % 8 == 0
            and _ws_bytes(q, kernel_size) >= 0)


def local_relation(q, k, v, pos_h, pos_w, kernel_size):
    """out[n,c,p] = sum_t softmax_t(logit[n, c mod G, :, p]) v[n, c, p + off_t]; see the module docstring"""
    if fusable(q, k, v, kernel_size):
        return _LocalRelation.apply(q, k, v, _pos(pos_h, pos_w, kernel_size), kernel_size)
    if q.is_cuda and kernel_size in _FUSED_WINDOWS and q.dtype in _DT:
        _lib.fallback("local_relation", q, f"window {kernel_size}, C {q.shape[1]}, dtypes {q.dtype} / {k.dtype} / {v.dtype}")
    return local_relation_reference(q, k, v, pos_h, pos_w, kernel_size)
