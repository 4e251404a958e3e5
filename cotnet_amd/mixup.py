"""Batch-mode mixup / CutMix on the device -- the reference's `FastCollateMixup(mode='batch')` (datasets/mixup.py:223-317) moved out of the
host loader's collate.

The reference mixes uint8 batches on the host while collating (`_mix_batch_collate`, :282-299) and builds two dense [N, num_classes]
targets (`mixup_target`, :22-27).  Here the host only DRAWS the batch's parameters -- from `np.random`, with the same calls in the same
order as `_params_per_batch` + `cutmix_bbox_and_lam`, so one seed gives the reference's stream -- and writes them into a 32-byte block in
device memory (`cot_mix_params`, include/cotnet_amd.h).  Two consumers read that block when their kernels run:

  * `mix_normalize` (`cot_mix_normalize`): the mixing folded into the uint8 -> model-dtype normalisation pass, partner sample N-1-i read
    from the unmodified input (no clone of the batch);
  * `cotnet_amd.loss.soft_target_cross_entropy`: the loss against the mixed, smoothed targets, formed per element from the integer labels.

Because lambda and the box are device data, not kernel arguments, a HIP graph that captured the step follows every later `draw()`
(`FlatSGD(device_lr=True)` does the same for the learning rate).  `draw()` stages the eight words in pinned host memory and issues one
non-blocking copy on the current stream: no host synchronisation unless all `_SLOTS` staging copies are still outstanding (then it
waits for the oldest).  It must be called outside a capture.

`DeviceMixup` is `mode='batch'` (what every shipped recipe uses through the prefetcher).  `PerSampleMixup` is `mode='elem'` and
`mode='pair'` (`_mix_elem_collate`, :229-252; `_mix_pair_collate`, :254-280): every sample has a lambda and a box of its own, so the block
grows into a table -- a header `mode 3, R` and R records of the same eight words, record n mixing sample n with its partner N-1-n
(include/cotnet_amd.h).  Both kernels take the header-or-table decision on the device, so one capture serves either kind of block.
`create_mixup(mode, ...)` is where a recipe's `mixup_mode` goes.  'half' (its output batch is half its input) and `Mixup.__call__` on
normalised float tensors raise / do not exist.
"""
import numpy as np
import torch

from . import _lib

_SLOTS = 8  # pinned staging slots: a draw reuses a slot only after the copy issued from it eight draws ago has completed


def pack_params(mode, lam, box=(0, 0, 0, 0)):
    """the eight 32-bit words of `cot_mix_params` as an int32 tensor: lam = float32(lam), one_minus_lam = float32(1.0 - lam) with the
    subtraction in double, as the reference forms both (mixup.py:27, :296)"""
    words = np.zeros(8, dtype=np.int32)
    words[0] = mode
    words[1:3] = np.array([lam, 1.0 - float(lam)], dtype=np.float64).astype(np.float32).view(np.int32)
    words[3:7] = box
    return torch.from_numpy(words)


class DeviceMixup:
    """The reference's constructor (mixup.py:104-121) and `mixup_enabled`; `device`: where the parameter block lives.

    `self.params`: the block the loss reads (int32[8], its address never changes).  draw(img_shape) draws the next batch's parameters
    and writes them there (or into `block=`, see PrefetchLoader) -> (lam, use_cutmix, (yl, yh, xl, xh))."""

    def __init__(self, mixup_alpha=1., cutmix_alpha=0., cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode='batch', correct_lam=True,
                 label_smoothing=0.1, num_classes=1000, device="cuda"):
        if mode != 'batch':
            raise NotImplementedError(f"DeviceMixup: mode={mode!r} (only 'batch', the recipes' mode, runs on the device)")
        self.mixup_alpha, self.cutmix_alpha = mixup_alpha, cutmix_alpha
        self.cutmix_minmax = cutmix_minmax if cutmix_minmax is not None and len(cutmix_minmax) else None
        if self.cutmix_minmax is not None:
            assert len(self.cutmix_minmax) == 2
            self.cutmix_alpha = 1.0  # as the reference: min/max draws the box, alpha only keeps CutMix switched on
        self.mix_prob, self.switch_prob = prob, switch_prob
        self.label_smoothing, self.num_classes = label_smoothing, num_classes
        self.mode, self.correct_lam = mode, correct_lam
        self.mixup_enabled = True  # the training loop switches mixing off for the last epochs (train.py:243-245)
        self.device = torch.device(device)
        self.params = self.new_block()
        self._stage = [None] * _SLOTS  # (pinned int32[8], event of the copy that last read it)
        self._n = 0

    def new_block(self):
        """a parameter block on the device holding `mode 0, lam 1` (no mixing; the loss is label smoothing alone)"""
        return pack_params(0, 1.).to(self.device)

    # ---- the draw: np.random calls in the reference's order
    def _lam_and_switch(self):
        lam, use_cutmix = 1., False
        if self.mixup_enabled and np.random.rand() < self.mix_prob:
            if self.mixup_alpha > 0. and self.cutmix_alpha > 0.:
                use_cutmix = np.random.rand() < self.switch_prob
                a = self.cutmix_alpha if use_cutmix else self.mixup_alpha
            elif self.mixup_alpha > 0.:
                a = self.mixup_alpha
            elif self.cutmix_alpha > 0.:
                use_cutmix, a = True, self.cutmix_alpha
            else:
                raise ValueError("DeviceMixup: one of mixup_alpha > 0, cutmix_alpha > 0, cutmix_minmax must be set")
            lam = float(np.random.beta(a, a))
        return lam, bool(use_cutmix)

    def _box(self, H, W, lam):
        if self.cutmix_minmax is not None:
            lo, hi = self.cutmix_minmax
            cut_h = np.random.randint(int(H * lo), int(H * hi))
            cut_w = np.random.randint(int(W * lo), int(W * hi))
            yl = np.random.randint(0, H - cut_h)
            xl = np.random.randint(0, W - cut_w)
            yh, xh = yl + cut_h, xl + cut_w
        else:
            ratio = np.sqrt(1 - lam)
            cut_h, cut_w = int(H * ratio), int(W * ratio)
            cy = np.random.randint(0, H)
            cx = np.random.randint(0, W)
            yl, yh = np.clip(cy - cut_h // 2, 0, H), np.clip(cy + cut_h // 2, 0, H)
            xl, xh = np.clip(cx - cut_w // 2, 0, W), np.clip(cx + cut_w // 2, 0, W)
        if self.correct_lam or self.cutmix_minmax is not None:  # the box was clipped by the border, or drawn without lam
            lam = float(1. - (yh - yl) * (xh - xl) / float(H * W))
        return (int(yl), int(yh), int(xl), int(xh)), lam

    def sample(self, img_shape):
        """-> (lam, use_cutmix, box) for one batch of images `img_shape` ([..., H, W]); host only"""
        lam, use_cutmix = self._lam_and_switch()
        box = (0, 0, 0, 0)
        if use_cutmix:
            box, lam = self._box(int(img_shape[-2]), int(img_shape[-1]), lam)
        return lam, use_cutmix, box

    def draw(self, img_shape, block=None):
        """sample() and write the block on the current stream (pinned staging, non-blocking copy; the host waits only if all `_SLOTS`
        earlier copies are still outstanding) -> (lam, use_cutmix, box) of THIS draw"""
        if _lib.capturing():
            raise RuntimeError("DeviceMixup.draw inside a HIP-graph capture would record this batch's values into the graph: draw "
                               "between replays, the captured kernels read the block when they run")
        lam, use_cutmix, box = self.sample(img_shape)
        mode = 0 if lam == 1. else (2 if use_cutmix else 1)  # the reference mixes nothing at lam == 1 (mixup.py:291)
        self.write(pack_params(mode, lam, box if mode == 2 else (0, 0, 0, 0)), block)
        return lam, use_cutmix, box

    def write(self, words, block=None):
        block = self.params if block is None else block
        if block.device.type != "cuda":
            block.copy_(words)
            return
        slot = self._n % _SLOTS
        self._n += 1
        if self._stage[slot] is None:
            self._stage[slot] = (torch.empty(8, dtype=torch.int32).pin_memory(), torch.cuda.Event())
        pinned, done = self._stage[slot]
        done.synchronize()  # (returns at once unless eight draws are in flight)
        pinned.copy_(words)
        block.copy_(pinned, non_blocking=True)
        done.record()

    def mix_normalize(self, x, mean, std, dtype=torch.float32, out=None, block=None):
        """x: uint8 [N, C, H, W] (contiguous, N even); mean / std: fp32 tensors of C entries scaled by 255, as for
        input_pipeline.normalize_uint8 -> the batch mixed as the block says and normalised as `dtype`, one kernel on the current stream"""
        block = self.params if block is None else block
        if x.dtype != torch.uint8 or x.dim() != 4 or not x.is_contiguous():
            raise TypeError("mix_normalize: expects a contiguous uint8 NCHW tensor")
        if _lib.DEVICE_ONLY and not x.is_cuda:
            raise RuntimeError("mix_normalize: cotnet_amd has no CPU path (input must be on the GPU)")
        N, C, H, W = x.shape
        if mean.numel() != C or std.numel() != C or mean.dtype != torch.float32 or std.dtype != torch.float32:
            raise ValueError("mix_normalize: mean / std must be fp32 tensors with one entry per channel")
        y = torch.empty((N, C, H, W), dtype=dtype, device=x.device) if out is None else out
        if y.shape != x.shape or y.dtype != dtype or not y.is_contiguous():
            raise ValueError("mix_normalize: out must be a contiguous tensor of x's shape and the requested dtype")
        _lib.api().cot_mix_normalize(x.data_ptr(), y.data_ptr(), mean.data_ptr(), std.data_ptr(), block.data_ptr(), N, C, H, W,
                                     _lib.dtype_code(dtype), _lib.stream())
        return y


class PerSampleMixup(DeviceMixup):
    """The reference's constructor with mode 'elem' (a draw per sample) or 'pair' (a draw per pair n <-> N-1-n, applied to both), plus
    `capacity`: the records the block has room for (the largest batch it can serve).

    `self.params` / new_block(): int32[8 * (1 + capacity)], allocated once -- its address never changes.  draw(img_shape) draws for the
    N = img_shape[0] samples and writes the header and N records.  In these modes the reference keeps lambda as FLOAT32
    (`lam_mix.astype(np.float32)`, :140): the box comes from sqrt(1 - lam) in fp32, a corrected CutMix lambda is a double rounded to
    float32 when it is stored back, and both the pixel blend and the target use 1 - lam subtracted in fp32 -- not batch mode's double."""

    def __init__(self, mixup_alpha=1., cutmix_alpha=0., cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode='elem', correct_lam=True,
                 label_smoothing=0.1, num_classes=1000, device="cuda", capacity=1024):
        if mode not in ('elem', 'pair'):
            raise NotImplementedError(f"PerSampleMixup: mode={mode!r} ('elem' or 'pair'; 'batch' is DeviceMixup)")
        if capacity < 2:
            raise ValueError("PerSampleMixup: capacity is the largest batch size, at least 2")
        self.capacity = int(capacity)  # (before the base constructor: it allocates through new_block())
        super().__init__(mixup_alpha, cutmix_alpha, cutmix_minmax, prob, switch_prob, 'batch', correct_lam, label_smoothing, num_classes,
                         device)
        self.mode = mode

    def new_block(self):
        """a block of 8 * (1 + capacity) words on the device whose header says `mode 0, lam 1`"""
        blk = torch.zeros(8 * (1 + self.capacity), dtype=torch.int32)
        blk[:8] = pack_params(0, 1.)
        return blk.to(self.device)

    # ---- the draw: np.random calls in the order of _params_per_elem (:123-141), then cutmix_bbox_and_lam per CutMix element
    def _params_per_elem(self, n):
        lam = np.ones(n, dtype=np.float32)
        use_cutmix = np.zeros(n, dtype=bool)
        if self.mixup_enabled:
            if self.mixup_alpha > 0. and self.cutmix_alpha > 0.:
                use_cutmix = np.random.rand(n) < self.switch_prob
                lam_cut = np.random.beta(self.cutmix_alpha, self.cutmix_alpha, size=n)  # both are drawn for every element
                lam_mix = np.where(use_cutmix, lam_cut, np.random.beta(self.mixup_alpha, self.mixup_alpha, size=n))
            elif self.mixup_alpha > 0.:
                lam_mix = np.random.beta(self.mixup_alpha, self.mixup_alpha, size=n)
            elif self.cutmix_alpha > 0.:
                use_cutmix = np.ones(n, dtype=bool)
                lam_mix = np.random.beta(self.cutmix_alpha, self.cutmix_alpha, size=n)
            else:
                raise ValueError("PerSampleMixup: one of mixup_alpha > 0, cutmix_alpha > 0, cutmix_minmax must be set")
            lam = np.where(np.random.rand(n) < self.mix_prob, lam_mix.astype(np.float32), lam)
        return lam, use_cutmix

    def _box(self, H, W, lam):
        """rand_bbox on the float32 lambda: the ratio and its products with H, W stay in fp32; -> (box, corrected lam as a double)"""
        if self.cutmix_minmax is not None:
            return super()._box(H, W, lam)
        ratio = np.sqrt(np.float32(1) - np.float32(lam))
        cut_h, cut_w = int(np.float32(H) * ratio), int(np.float32(W) * ratio)
        cy = np.random.randint(0, H)
        cx = np.random.randint(0, W)
        yl, yh = np.clip(cy - cut_h // 2, 0, H), np.clip(cy + cut_h // 2, 0, H)
        xl, xh = np.clip(cx - cut_w // 2, 0, W), np.clip(cx + cut_w // 2, 0, W)
        if self.correct_lam:
            lam = 1. - float((yh - yl) * (xh - xl)) / float(H * W)
        return (int(yl), int(yh), int(xl), int(xh)), lam

    def sample(self, img_shape, N):
        """-> (lam float32 [N], use_cutmix bool [N], boxes int [N, 4]) for a batch of N images `img_shape` ([..., H, W]); host only.
        use_cutmix is the switch as drawn, also where lam is 1; a sample without a box has (0, 0, 0, 0)"""
        if N % 2:
            raise ValueError(f"PerSampleMixup: batch size {N} is odd: sample i is mixed with sample N-1-i")
        n = N // 2 if self.mode == 'pair' else N
        H, W = int(img_shape[-2]), int(img_shape[-1])
        lam, use_cutmix = self._params_per_elem(n)
        boxes = np.zeros((n, 4), dtype=np.int64)
        for i in range(n):
            if lam[i] != 1. and use_cutmix[i]:
                boxes[i], lam[i] = self._box(H, W, lam[i])  # (the corrected double is rounded to float32 here, as in lam_batch[i] = lam)
        if self.mode == 'pair':  # record N-1-i = record i
            lam, use_cutmix, boxes = (np.concatenate((a, a[::-1])) for a in (lam, use_cutmix, boxes))
        return lam, use_cutmix, boxes

    def pack(self, lam, use_cutmix, boxes):
        """the words of a table block: the header `mode 3, R = N`, then one record per sample -- mode 0 where lam is 1 (the reference
        mixes nothing there), one_minus_lam = float32(1) - lam in fp32"""
        N = len(lam)
        words = np.zeros((1 + N, 8), dtype=np.int32)
        words[0, 0], words[0, 3] = 3, N
        words[0, 1:3] = np.array([1., 0.], dtype=np.float32).view(np.int32)
        lam = np.asarray(lam, dtype=np.float32)
        cut = np.asarray(use_cutmix, dtype=bool) & (lam != 1.)
        words[1:, 0] = np.where(lam == 1., 0, np.where(cut, 2, 1))
        words[1:, 1] = lam.view(np.int32)
        words[1:, 2] = (np.float32(1) - lam).view(np.int32)
        words[1:, 3:7] = np.where(cut[:, None], np.asarray(boxes).reshape(N, 4), 0)
        return torch.from_numpy(words.reshape(-1))

    def draw(self, img_shape, block=None):
        """sample() for the N = img_shape[0] samples and write header + N records on the current stream (pinned staging, ONE non-blocking
        copy) -> (lam, use_cutmix, boxes) of THIS draw.  With mixup_enabled False: a `mode 0` header, nothing drawn"""
        if _lib.capturing():
            raise RuntimeError("PerSampleMixup.draw inside a HIP-graph capture would record this batch's values into the graph: draw "
                               "between replays, the captured kernels read the block when they run")
        N = int(img_shape[0])
        if N > self.capacity:
            raise ValueError(f"PerSampleMixup: a batch of {N} samples, the block holds capacity={self.capacity} records")
        if not self.mixup_enabled:
            self.write(pack_params(0, 1.), block)
            return np.ones(N, dtype=np.float32), np.zeros(N, dtype=bool), np.zeros((N, 4), dtype=np.int64)
        lam, use_cutmix, boxes = self.sample(img_shape, N)
        self.write(self.pack(lam, use_cutmix, boxes), block)
        return lam, use_cutmix, boxes

    def write(self, words, block=None):
        """the first len(words) words of the block (what lies behind them is never read: the header says how many records count)"""
        block = self.params if block is None else block
        n = words.numel()
        if block.device.type != "cuda":
            block[:n].copy_(words)
            return
        slot = self._n % _SLOTS
        self._n += 1
        if self._stage[slot] is None:
            self._stage[slot] = (torch.empty(8 * (1 + self.capacity), dtype=torch.int32).pin_memory(), torch.cuda.Event())
        pinned, done = self._stage[slot]
        done.synchronize()  # (returns at once unless eight draws are in flight)
        pinned[:n].copy_(words)
        block[:n].copy_(pinned[:n], non_blocking=True)
        done.record()


def create_mixup(mode='batch', **kw):
    """where a recipe's `cfg.augmentation.mixup_mode` goes: 'batch' -> DeviceMixup, 'elem' / 'pair' -> PerSampleMixup"""
    if mode == 'batch':
        return DeviceMixup(mode=mode, **kw)
    if mode in ('elem', 'pair'):
        return PerSampleMixup(mode=mode, **kw)
    if mode == 'half':
        raise NotImplementedError("create_mixup: mode='half' stays on the host -- its collate returns N/2 samples for N inputs and a float64 "
                                  "target, and cot_mix_normalize / cot_soft_target_ce_* take ONE batch size N for input, output and labels")
    raise ValueError(f"create_mixup: unknown mixup mode {mode!r} ('batch', 'elem', 'pair', 'half')")
