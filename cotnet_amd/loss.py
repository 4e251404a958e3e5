"""The recipe's losses on the device -- the reference's loss/cross_entropy.py (`SoftTargetCrossEntropy`, `LabelSmoothingCrossEntropy`).

The reference's training loss with mixup is `sum(-target * log_softmax(x), -1).mean()` against a dense [N, K] target that its collate
built from two one-hot tensors (datasets/mixup.py:22-27).  Here the target is never materialised: `cot_soft_target_ce_forward` /
`_backward` (csrc/mix_loss.hip) form it per element from the INTEGER labels, the pairing n <-> N-1-n and the (lam, 1 - lam) that
`cotnet_amd.mixup.DeviceMixup` keeps in device memory.  Forward is two launches (rows, then their mean in a fixed order -- no atomics),
backward one; nothing about the batch is a kernel argument, so a captured step follows new labels and a new lambda at every replay.

A caller that does hold a dense target (the reference's host collate, distillation) is served by the torch formula, counted through
`_lib.fallback` like every other wrapper's off-grid case.
"""
import torch
from torch import nn

from . import _lib
from .mixup import pack_params


class _SoftTargetCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, block, smoothing):
        N, K = logits.shape
        f32 = dict(dtype=torch.float32, device=logits.device)
        rows, lse, mean = torch.empty(N, **f32), torch.empty(4 * N, **f32), torch.empty((), **f32)  # (lse: the kernels' workspace, opaque)
        _lib.api().cot_soft_target_ce_forward(logits.data_ptr(), labels.data_ptr(), block.data_ptr(), smoothing, rows.data_ptr(),
                                              lse.data_ptr(), mean.data_ptr(), N, K, _lib.dtype_code(logits.dtype), _lib.stream())
        ctx.save_for_backward(logits, labels, block, lse)
        ctx.smoothing = smoothing
        return mean

    @staticmethod
    def backward(ctx, g):
        logits, labels, block, lse = ctx.saved_tensors
        N, K = logits.shape
        g = g.to(torch.float32).contiguous()  # one element on the device: the kernel reads it when it runs
        dx = torch.empty_like(logits)
        _lib.api().cot_soft_target_ce_backward(logits.data_ptr(), labels.data_ptr(), block.data_ptr(), ctx.smoothing, lse.data_ptr(),
                                               g.data_ptr(), dx.data_ptr(), N, K, _lib.dtype_code(logits.dtype), _lib.stream())
        return dx, None, None, None


def _block_of(mix):
    return getattr(mix, "params", mix)  # a DeviceMixup, or the int32[8] block itself


def _dense(logits, target):
    """the reference's formula (cross_entropy.py:35-36) for a caller-made dense target"""
    _lib.fallback("soft_target_cross_entropy", logits, "dense target")
    return torch.sum(-target * torch.nn.functional.log_softmax(logits, dim=-1), dim=-1).mean()


def soft_target_cross_entropy(logits, labels, mix, smoothing=0.1):
    """logits [N, K] fp32 / bf16; labels int64 [N]; mix: a DeviceMixup (or its int32[8] parameter block); -> the mean loss, fp32 scalar.
    The target of row n is lam*oh(y_n) + (1 - lam)*oh(y_{N-1-n}) with smoothed one-hots, as the reference's collate builds it.
    A floating-point `labels` of logits' shape is a dense target: the torch formula (counted as a module fallback)."""
    if labels.is_floating_point() and labels.shape == logits.shape:
        return _dense(logits, labels)
    if logits.dim() != 2 or labels.shape != logits.shape[:1] or labels.dtype != torch.int64:
        raise TypeError("soft_target_cross_entropy: logits [N, K] and int64 labels [N]")
    if logits.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"soft_target_cross_entropy: {logits.dtype} logits (float32 / bfloat16)")
    if _lib.DEVICE_ONLY and not logits.is_cuda:
        raise RuntimeError("soft_target_cross_entropy: cotnet_amd has no CPU path (logits must be on the GPU)")
    block = _block_of(mix)
    if block.dtype != torch.int32 or block.numel() < 8 or block.numel() % 8 or block.device != logits.device:
        raise ValueError("soft_target_cross_entropy: the parameter block is int32[8] (a PerSampleMixup's: int32[8 * (1 + capacity)]) on the "
                         "logits' device")
    return _SoftTargetCE.apply(logits.contiguous(), labels.contiguous(), block, float(smoothing))


class MixedSoftTargetCrossEntropy(nn.Module):
    """module form: `loss_fn = MixedSoftTargetCrossEntropy(mixup)`; `loss_fn(logits, labels)`.  smoothing defaults to the mixup's
    label_smoothing, as the reference passes it to mixup_target"""

    def __init__(self, mix, smoothing=None):
        super().__init__()
        self.mix = mix
        self.smoothing = float(mix.label_smoothing if smoothing is None else smoothing)

    def forward(self, x, target):
        return soft_target_cross_entropy(x, target, self.mix, self.smoothing)


class LabelSmoothingCrossEntropy(nn.Module):
    """the reference's signature (cross_entropy.py:6-26): NLL with label smoothing against hard labels -- the same kernels reading a
    constant block `mode 0, lam 1`"""

    def __init__(self, smoothing=0.1):
        super().__init__()
        assert smoothing < 1.0
        self.smoothing = smoothing
        self.confidence = 1. - smoothing
        self.register_buffer("params", pack_params(0, 1.), persistent=False)  # moves with .to(device)

    def forward(self, x, target):
        if self.params.device != x.device:
            self.params = self.params.to(x.device)
        return soft_target_cross_entropy(x, target, self.params, self.smoothing)
