"""Mixed-precision parameters + fused flat SGD-nesterov ("training-loop glue on device").

The reference trains fp32 with `torch.optim.SGD(nesterov=True)` (optim/optim_factory.py:54-56), weight decay only on
>1-D parameters (:19-31), gradients synchronised by DDP (train.py:115), plus one elementwise op per tensor for EMA.
On MI355X the step is bound by HBM passes and launch count, so this module

  * keeps Conv2d / Linear weights and biases in bf16 (what the convolutions read) with fp32 MASTER copies, and the
    normalisation parameters in fp32 -- no per-step autocast casts (measured: ~530 cast launches per CoTNet-50 step);
  * lays parameters, gradients, masters and momentum out in a few flat buckets per (dtype, weight-decay) group
    (cotnet_amd.data_parallel.GradBucketReducer with flatten_params=True, grad_mode="copy": autograd's gradients are
    moved into the bucket with one multi-tensor copy, then all-reduced over RCCL on the side stream);
  * updates each bucket with ONE hand-written HIP kernel (`cot_sgd_step`, csrc/optim.hip; `cot_sgd_step_lr` with
    device_lr=True: the rate read from device memory, so that a step replayed from a HIP graph follows a schedule;
    `cot_sgd_step_clip` with clip_grad / skip_nonfinite: behind the gradients' global norm, formed on the device by
    `cot_grad_sumsq` + `cot_grad_clip_finish`, csrc/grad_clip.hip -- the reference's `dispatch_clip_grad`, train.py:269-274; with
    agc, one `cot_agc_clip` per bucket in front of it, csrc/agc.hip -- the same call's mode 'agc').

Arithmetic = torch.optim.SGD (dampening 0) evaluated in fp32 on the master weights; checked against it in
tests/test_flat_sgd_gpu.py.
"""
import contextlib
import math

import torch
from torch import nn

from . import _lib
from .data_parallel import GradBucketReducer


def to_mixed_bf16(model):
    """Conv2d / Linear / GroupNorm parameters -> bf16 (in place); BatchNorm parameters and all buffers stay fp32
    (torch's group_norm wants its affine parameters in the input dtype; batch_norm takes fp32 ones).  Returns the model."""
    for m in model.modules():
        if isinstance(m, (nn.Conv2d, nn.Linear, nn.GroupNorm)):
            for p in m.parameters(recurse=False):
                p.data = p.data.to(torch.bfloat16)
    return model


def _decay_group(name, p):
    # reference rule: no weight decay on 1-D parameters and biases (optim/optim_factory.py:19-31)
    return "no_decay" if (p.ndim <= 1 or name.endswith(".bias")) else "decay"


def _agc_unit_table(params, offs, n):
    """int64 [units, 2] = (start, len) in elements of a bucket whose parameter slots begin at `offs` (a CPU tensor): the reference's
    unitwise_norm (utils/clip_grad.py:3-9) -- a parameter with ndim <= 1 is one unit, any other is shape[0] units of numel / shape[0]
    consecutive elements.  The padding between the slots belongs to no unit.  Checked: len >= 1, ascending, disjoint, inside [0, n) --
    `cot_agc_clip` trusts the table's contents."""
    rows = []
    for p, off in zip(params, offs):
        if p.numel() == 0:
            continue
        if p.ndim <= 1:
            rows.append(torch.tensor([[off, p.numel()]], dtype=torch.int64))
        else:
            per = p.numel() // p.shape[0]
            start = off + per * torch.arange(p.shape[0], dtype=torch.int64)
            rows.append(torch.stack([start, torch.full_like(start, per)], dim=1))
    table = torch.cat(rows) if rows else torch.zeros((0, 2), dtype=torch.int64)
    start, length = table[:, 0], table[:, 1]
    ok = bool((length >= 1).all()) and bool((start >= 0).all()) and bool((start + length <= n).all())
    if not (ok and bool((start[1:] >= (start + length)[:-1]).all())):
        raise ValueError("FlatSGD(agc=...): the bucket's parameter slots do not give ascending, disjoint units inside the bucket")
    return table.contiguous()


class FlatSGD:
    def __init__(self, model, lr, momentum=0.9, weight_decay=0.0, nesterov=True, bucket_mb=10.0, process_group=None,
                 broadcast_params=True, ema_decay=None, force_collectives=False, grad_dtype=None, device_lr=False, clip_grad=None,
                 clip_mode="norm", skip_nonfinite=False, agc=None, agc_eps=1e-3, lookahead_k=None, lookahead_alpha=0.5):
        """bucket_mb: size of the flat gradient buckets.  10 MiB cuts CoTNet-50's 44 MB of bf16 weight gradients into five
        buckets in the order backward produces them (classifier and stage 4 first, the stem last), so four all-reduces are
        already on the communication stream when backward ends and only the last, small one is exposed; round 2's 48 MiB
        made ONE bucket whose last member is the stem's weight -- nothing could overlap (tests/test_data_parallel_cpu.py).
        A 10 MB ring all-reduce over 8 GPUs moves 17.5 MB per link direction: ~0.12 ms at xGMI's ~153 GB/s, well above the
        collective's fixed latency.
        grad_dtype: the arithmetic of the all-reduce.  None (default): the parameter's own (bf16 weights -> bf16 buckets, RCCL
        averages in bf16: one rounding of 2^-9 relative per ring hop, ~0.2 % over eight ranks -- the size of the bf16 gradients'
        own rounding; tests/test_data_parallel_cpu.py bounds it); torch.float32: the reference's arithmetic (DDP sums fp32
        gradients, train.py:112-115) at twice the bytes on the wire -- the gradients are produced in bf16 as always (kernels write
        them straight into the bucket slots) and each bucket is widened by one flat copy on the communication stream right before
        its all-reduce (GradBucketReducer reduce_dtype); the SGD kernel then reads the fp32 averages.
        ema_decay: also keep an exponential moving average of the weights (the reference's ModelEmaV2,
        utils/model_ema.py, `model_ema: True` / decay 0.9999 in its recipes): one flat kernel per bucket after the SGD
        kernel instead of one elementwise op per state_dict tensor; floating-point buffers (BatchNorm running statistics)
        are averaged with one multi-tensor lerp.  `ema_state_dict()` returns it under the model's state_dict keys.
        device_lr: False (default): `cot_sgd_step` takes the rate by value, so a HIP graph that captured step() keeps the rate it
        was captured with (set_lr).  True: the rate lives in `self.lr_dev`, one fp32 element on the parameters' device, allocated
        here once (its address never changes); step() issues `cot_sgd_step_lr`, whose kernel reads that element when it runs, so a
        capture bakes no rate and set_lr between replays moves the replayed step (lr_schedule.CosineSchedule.apply).  Same
        arithmetic on the same fp32 rate: the two forms are bit-equal (tests/test_sgd_device_lr_gpu.py).
        clip_grad: clip the gradients to this global L2 norm before the step, as the reference does between backward and
        optimizer.step() (train.py:269-274, `dispatch_clip_grad(..., mode='norm')` = torch.nn.utils.clip_grad_norm_); None or <= 0: no
        clipping (the reference's convention, train.py:270).  The norm runs over EVERY bucket, decay and no-decay alike, on the
        averaged gradients (after the all-reduce: the same coefficient on every rank).
        clip_mode: only "norm".  Of the reference's other two modes (utils/clip_grad.py:36-39), 'agc' is the keyword `agc` below and
        'value' is not built.
        skip_nonfinite: a step whose gradients hold an inf or a NaN (or whose sum of squares overflows) writes no parameter, master
        or momentum; the EMA still moves, as the reference's does behind a step its scaler skipped (train.py:276-277).
        With either, step() issues `cot_grad_sumsq` per bucket, one `cot_grad_clip_finish` and `cot_sgd_step_clip` per bucket
        (csrc/grad_clip.hip): norm, coefficient and skip flag stay in `self.clip_state` (int32[8] = cot_clip_state, allocated here
        once next to the partial sums; the addresses never change), nothing about a batch is a kernel argument, and one HIP-graph
        capture serves clipped, unclipped and skipped steps alike.  A non-finite step is ALWAYS skipped when clip_grad is set
        (torch's clip_grad_norm_ multiplies every gradient by the NaN coefficient, and the step then poisons every weight);
        skip_nonfinite=True alone asks for the guard with the coefficient 1.  `clip_stats()` reads the block.  With neither,
        nothing is allocated and the launches are the ones of the plain optimizer.
        agc: adaptive gradient clipping with this clip factor (the reference's `dispatch_clip_grad(..., mode='agc')` =
        adaptive_clip_grad, utils/clip_grad.py:3-24, whose default factor is 0.01); None or <= 0: off -- nothing is allocated and the
        launches are the ones of before.  Every output unit of every parameter (the reference's unitwise_norm: a parameter with
        ndim <= 1 is ONE unit, any other is shape[0] rows) is clipped against the L2 norm of its own fp32 weights, the master where
        the bucket has one: coef = gn < max(wn, agc_eps) * agc ? 1 : max(wn, agc_eps) * agc / max(gn, 1e-6), and a unit with coef < 1
        is scaled IN PLACE in the bucket.  step() issues one `cot_agc_clip` per bucket (csrc/agc.hip) on the averaged gradients, after
        the all-reduce (the same coefficients on every rank) and in front of everything else, so that the guard of skip_nonfinite
        sees the gradients the step will consume.  The unit tables (int64 (start, len) pairs from the buckets' slots, checked here
        on the host to be ascending, disjoint and in range, uploaded once) and the coefficient tensors (one float per unit) are
        allocated here and keep their addresses; the factor and agc_eps travel by value, so one HIP-graph capture serves every step.
        A unit whose weight or gradient norm is not finite is left as it is and marked coef = NaN (the reference would write NaN
        into it); with skip_nonfinite=True the guard then skips the step.  The reference's zero-initialised `bn3.weight`
        (cotnet.py:225-226) is a 1-D unit with wn = 0: it is clipped against agc_eps * agc, which is the reference's behaviour and
        is kept.  Not together with clip_grad: the reference runs one mode per step.  `agc_stats()` and `agc_coefficients()` read
        the last step's coefficients.
        agc_eps: the floor of the weight norm (the reference's eps = 1e-3).
        lookahead_k: Lookahead (the reference's `lookahead_` prefix, optim/optim_factory.py:116-118 -> optim/lookahead.py, whose
        defaults are k = 6 and alpha = 0.5); None (default): off -- nothing is allocated and the launches are the ones of before.
        An int >= 1: every k-th ACCEPTED step the fp32 weights are pulled back to slow weights, slow += alpha * (fast - slow);
        fast = slow (lookahead.py:29-39).  The slow weights (`"slow"` in each bucket's state, fp32, the bucket's length) and
        `self.lookahead_state` (int32[8] = cot_lookahead_state) are allocated here once and keep their addresses.  step() issues one
        `cot_lookahead_tick` behind the clip launches and the update rule's own tick -- it counts the step in device memory and
        decides -- and one `cot_lookahead_step` per bucket between the bucket's update kernel and its EMA launch (csrc/lookahead.hip),
        so the EMA averages the weights after the sync, as the reference's loop does, and one HIP-graph capture serves sync and
        non-sync steps alike; k and alpha travel by value.  As in the reference the slow weights are created at the FIRST sync as a
        copy of the fast ones (lookahead.py:34-36): step k moves no weight, step 2k is the first to interpolate.  Momentum and
        moments are never touched.  A step the non-finite guard skips is not counted (the block's `refused` counts it), as a step
        the reference's scaler skips never reaches optimizer.step() (train.py:276-277).  `sync_lookahead()` is the reference's
        end-of-epoch call (train.py:295-296), `lookahead_stats()` reads the block.
        lookahead_alpha: the slow weights' rate, in [0, 1]."""
        self.momentum, self.nesterov = float(momentum), nesterov
        self._setup(model, lr, weight_decay, bucket_mb, process_group, broadcast_params, ema_decay, force_collectives, grad_dtype,
                    device_lr, clip_grad, clip_mode, skip_nonfinite, agc, agc_eps, lookahead_k, lookahead_alpha)

    def _bucket_state(self, b):
        """what the update rule keeps per bucket next to the master: fp32 arrays of the bucket's length, allocated once"""
        return {"mom": torch.zeros(b.pflat.numel(), dtype=torch.float32, device=b.pflat.device)}

    @staticmethod
    def _weights(b, st):
        """the bucket's fp32 weights: the master, or the parameters themselves where there is none"""
        return st["master"] if st["master"] is not None else b.pflat

    def _device(self):
        """the device of the first bucket, else of the first parameter"""
        return self.reducer.buckets[0].pflat.device if self.reducer.buckets else next(self.model.parameters()).device

    def _setup(self, model, lr, weight_decay, bucket_mb, process_group, broadcast_params, ema_decay, force_collectives, grad_dtype,
               device_lr, clip_grad, clip_mode, skip_nonfinite, agc, agc_eps, lookahead_k=None, lookahead_alpha=0.5):
        """everything of the constructor that does not depend on the update rule (FlatAdamW, flat_adamw.py, shares it): the keywords'
        checks, the buckets and masters, the device-resident rate, the clip block, the AGC tables, the averages, Lookahead's slow
        weights and block"""
        name = type(self).__name__
        self.lookahead_k, self.lookahead_alpha = self._lookahead_checked(lookahead_k, lookahead_alpha, f"{name}(")
        self._captured_lookahead = None  # (k, alpha) a HIP-graph capture of step() baked into its lookahead launches
        if clip_mode != "norm":
            raise ValueError(f"{name}(clip_mode={clip_mode!r}): only 'norm' (clipping by the global L2 norm) is a value of clip_mode; "
                             "the reference's other modes 'value' and 'agc' are not values of clip_mode: adaptive clipping is "
                             f"{name}(agc=...), and clipping by value is not built")
        self.agc = float(agc) if agc is not None and agc > 0 else None
        self.agc_eps = float(agc_eps)
        if self.agc is not None:
            if clip_grad is not None and clip_grad > 0:
                raise ValueError(f"{name}(agc={agc!r}, clip_grad={clip_grad!r}): one clipping mode per step, as in the reference's "
                                 "dispatch_clip_grad -- give agc or clip_grad, not both")
            if not (math.isfinite(self.agc) and math.isfinite(self.agc_eps) and self.agc_eps > 0):
                raise ValueError(f"{name}(agc={agc!r}, agc_eps={agc_eps!r}): both must be finite and positive")
        self.lr, self.weight_decay = float(lr), float(weight_decay)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self._captured_lr = None  # the rate a HIP-graph capture of step() baked into its cot_sgd_step launches (set_lr)
        self.model = model
        # masters must be taken from the fp32 values BEFORE rounding when the caller converts later; here parameters
        # are already in their storage dtype, so the master starts as the (exact) up-cast of the working copy.
        self.reducer = GradBucketReducer(model, process_group=process_group, bucket_mb=bucket_mb,
                                         broadcast_params=broadcast_params, group_fn=_decay_group, grad_mode="copy",
                                         flatten_params=True, force_collectives=force_collectives, reduce_dtype=grad_dtype)
        self.state = []
        for b in self.reducer.buckets:
            master = b.pflat.float().clone() if b.pflat.dtype != torch.float32 else None
            st = {"master": master, **self._bucket_state(b)}
            if self.ema_decay is not None:
                st["ema"] = self._weights(b, st).float().clone()
            if self.lookahead_k is not None:  # zeros, not the weights: the slow weights are born at the first sync (lookahead.py:34-36)
                st["slow"] = torch.zeros(b.pflat.numel(), dtype=torch.float32, device=b.pflat.device)
            self.state.append(st)
        self.lookahead_state = None
        if self.lookahead_k is not None:
            self.lookahead_state = torch.zeros(8, dtype=torch.int32, device=self._device())  # cot_lookahead_state
        self.lr_dev = None
        if device_lr:
            self.lr_dev = torch.full((1,), self.lr, dtype=torch.float32, device=self._device())
        self.clip_grad = float(clip_grad) if clip_grad is not None and clip_grad > 0 else None
        self.skip_nonfinite = bool(skip_nonfinite)
        self.clip_state = self._clip_parts = None
        if self.clip_grad is not None or self.skip_nonfinite:
            dev = self._device()
            self.clip_state = torch.zeros(8, dtype=torch.int32, device=dev)
            self._clip_parts = torch.zeros(max(len(self.reducer.buckets), 1) * _lib.lib().cot_grad_norm_parts(), dtype=torch.float32,
                                           device=dev)
        self._agc_units = self._agc_coef = None
        if self.agc is not None:
            self._agc_units, self._agc_coef = [], []
            for b in self.reducer.buckets:
                table = _agc_unit_table(b.params, b.offs, b.pflat.numel())
                self._agc_units.append(table.to(b.pflat.device))
                self._agc_coef.append(torch.zeros(table.shape[0], dtype=torch.float32, device=b.pflat.device))
        if self.ema_decay is not None:
            self._buf_src = [bf for bf in model.buffers() if bf.is_floating_point()]
            self._buf_ema = [bf.detach().float().clone() for bf in self._buf_src]
        _lib.lib()

    def zero_grad(self):
        self.reducer.zero_grad()

    def step(self, deferred=False):
        """finish the gradient all-reduce (stream wait only) and update every bucket with one kernel each.
        deferred=True: the reducer ran with defer_comm (hooks only filled the buckets); all-reduce them now."""
        if deferred:
            self.reducer.allreduce_all()
        else:
            self.reducer.finish()
        L = _lib.api()
        stream = _lib.stream()
        # (with lr_dev the kernel reads the rate when it runs: a capture bakes none)
        if self.lr_dev is None and _lib.capturing():  # the rate travels by value: every replay of this capture steps with it (set_lr)
            self._captured_lr = self.lr
        if self.agc is not None:
            # unit-wise clipping of the AVERAGED gradients, in place in the buckets; what follows (guard, SGD) reads the clipped ones
            for b, st, units, coef in zip(self.reducer.buckets, self.state, self._agc_units, self._agc_coef):
                if units.shape[0] == 0:
                    continue
                g = self.reducer.reduced(b)
                weight = self._weights(b, st)
                L.cot_agc_clip(g.data_ptr(), weight.data_ptr(), units.data_ptr(), units.shape[0], g.numel(), self.agc, self.agc_eps,
                               coef.data_ptr(), _lib.dtype_code(g.dtype), stream)
        clipped = self.clip_state is not None and bool(self.reducer.buckets)
        if clipped:
            # the norm of the AVERAGED gradients over every bucket -> coefficient and skip flag in self.clip_state, which the update
            # kernels below read when they run
            parts = L.cot_grad_norm_parts()
            for i, b in enumerate(self.reducer.buckets):
                g = self.reducer.reduced(b)
                L.cot_grad_sumsq(g.data_ptr(), g.numel(), _lib.dtype_code(g.dtype), self._clip_parts.data_ptr() + 4 * parts * i, stream)
            L.cot_grad_clip_finish(self._clip_parts.data_ptr(), self._clip_parts.numel(),
                                   self.clip_grad if self.clip_grad is not None else float("inf"), self.clip_state.data_ptr(), stream)
        update = self._bucket_update(L, clipped, stream)
        sync = self._lookahead_update(L, clipped, stream)
        for b, st in zip(self.reducer.buckets, self.state):
            update(b, st, self.weight_decay if b.key == "decay" else 0.0)
            if sync is not None:  # in front of the EMA launch: the average follows the weights after the sync
                sync(b, st)
            if self.ema_decay is not None:
                src = self._weights(b, st)
                L.cot_ema_step(st["ema"].data_ptr(), src.data_ptr(), src.numel(),
                               self.ema_decay, _lib.dtype_code(src.dtype), stream)
        if self.ema_decay is not None and self._buf_src:
            torch._foreach_lerp_(self._buf_ema, [bf.float() if bf.dtype != torch.float32 else bf for bf in self._buf_src],
                                 1.0 - self.ema_decay)
        if self.reducer.buckets:  # the parameters changed behind torch's version counters: caches keyed on them move on
            from . import cot_layer_fused
            cot_layer_fused.after_optimizer_step(self.reducer.buckets[0].pflat.device)

    def _bucket_update(self, L, clipped, stream):
        """the update rule's launches: called once per step() behind the clip launches (`clipped`: the block was filled), returns
        update(bucket, its state, its weight decay), which step() calls per bucket in front of the bucket's EMA launch"""
        if clipped:
            sgd = L.cot_sgd_step_clip
            rate = (self.lr, self.lr_dev.data_ptr() if self.lr_dev is not None else None, self.clip_state.data_ptr())
        elif self.lr_dev is not None:
            sgd, rate = L.cot_sgd_step_lr, (self.lr_dev.data_ptr(),)
        else:
            sgd, rate = L.cot_sgd_step, (self.lr,)

        def update(b, st, wd):
            sgd(b.pflat.data_ptr(),
                st["master"].data_ptr() if st["master"] is not None else None,
                st["mom"].data_ptr(), self.reducer.reduced(b).data_ptr(),
                b.pflat.numel(), *rate, self.momentum, wd, 1.0, 1 if self.nesterov else 0,
                _lib.dtype_code(b.pflat.dtype), _lib.dtype_code(self.reducer.reduced(b).dtype), stream)
        return update

    # ---- Lookahead (the reference's optim/lookahead.py) on the device: csrc/lookahead.hip

    @staticmethod
    def _lookahead_checked(k, alpha, where):
        """(k, alpha) as stored -- (None, alpha) = off; the reference's checks (lookahead.py:14-17)"""
        alpha = float(alpha)
        if not 0.0 <= alpha <= 1.0:  # (a NaN fails it too)
            raise ValueError(f"{where}lookahead_alpha={alpha!r}): the slow update rate must lie in [0, 1]")
        if k is None:
            return None, alpha
        if isinstance(k, bool) or not isinstance(k, int) or k < 1:
            raise ValueError(f"{where}lookahead_k={k!r}): the number of lookahead steps must be an int >= 1 (None: no Lookahead)")
        return k, alpha

    def _lookahead_update(self, L, clipped, stream, force=0):
        """Lookahead's launches: called once per step() behind `_bucket_update` (whose tick, if it has one, is issued first) -- ONE
        cot_lookahead_tick, which reads the clip block's skip -- and returns sync(bucket, its state) = one cot_lookahead_step, which
        step() calls per bucket between the update kernel and the bucket's EMA launch.  None with Lookahead off."""
        if self.lookahead_k is None or not self.reducer.buckets:
            return None
        block = self.lookahead_state.data_ptr()
        k, alpha = self.lookahead_k, self.lookahead_alpha
        if _lib.capturing():  # k and alpha travel by value: every replay of this capture syncs with them
            self._captured_lookahead = (k, alpha)
        L.cot_lookahead_tick(block, self.clip_state.data_ptr() if clipped else None, k, force, stream)

        def sync(b, st):
            L.cot_lookahead_step(b.pflat.data_ptr(), st["master"].data_ptr() if st["master"] is not None else None, st["slow"].data_ptr(),
                                 b.pflat.numel(), alpha, block, _lib.dtype_code(b.pflat.dtype), stream)
        return sync

    def sync_lookahead(self):
        """the reference's end-of-epoch call (lookahead.py:41-43, train.py:295-296): the slow weights are updated and the fast weights
        set to them NOW, without counting a step -- one forced cot_lookahead_tick, one cot_lookahead_step per bucket.  Unborn slow
        weights are adopted and no weight moves, as in the reference.  It finishes no all-reduce, reads no gradient and not the clip
        block, and leaves momentum, moments and the EMA alone.  Refused while capturing.  Built without lookahead_k it returns at
        once: the reference guards its call with hasattr, and here the attribute is always there."""
        if self.lookahead_k is None:
            return
        self._not_while_capturing("sync_lookahead()")
        sync = self._lookahead_update(_lib.api(), False, _lib.stream(), force=1)
        if sync is None:
            return
        for b, st in zip(self.reducer.buckets, self.state):
            sync(b, st)
        from . import cot_layer_fused
        cot_layer_fused.after_optimizer_step(self.reducer.buckets[0].pflat.device)

    def lookahead_stats(self):
        """ONE host read of the block: dict(step, born, syncs, refused) -- accepted steps, whether the slow weights hold something, the
        syncs carried out, the steps the guard skipped.  Synchronises with the device; refused while capturing."""
        if self.lookahead_state is None:
            raise RuntimeError(f"{type(self).__name__}.lookahead_stats(): built without lookahead_k")
        self._not_while_capturing("lookahead_stats()")
        w = self.lookahead_state.cpu().tolist()
        return dict(step=w[0], born=w[2], syncs=w[3], refused=w[4])

    def _lookahead_saved(self, d):
        """state_dict()'s `d` with Lookahead's part: the reference's top-level order (lookahead.py:62-66) state, slow_state,
        param_groups, then cotnet_amd; slow_state[idx] = {'slow_buffer': fp32 clone} once born, {} before; lookahead_alpha, _k and
        _step in every group (lookahead.py:18-27); the block's eight words under cotnet_amd['lookahead'].  Off: `d` as it is."""
        if self.lookahead_k is None:
            return d
        words = self.lookahead_state.cpu().tolist()
        slow = self._slots("slow")
        members = [p for g in self._groups() for _, p in g]
        slow_state = {i: ({"slow_buffer": slow[p].detach().clone()} if words[2] else {}) for i, p in enumerate(members)}
        groups = [dict(g, lookahead_alpha=self.lookahead_alpha, lookahead_k=self.lookahead_k, lookahead_step=words[0])
                  for g in d["param_groups"]]
        return {"state": d["state"], "slow_state": slow_state, "param_groups": groups, "cotnet_amd": dict(d["cotnet_amd"], lookahead=words)}

    def _lookahead_plan(self, d):
        """load_state_dict()'s checks of Lookahead's part, all before anything is written: returns what `_lookahead_load` writes.
        (d['param_groups'] has been checked against this optimizer's groups.)"""
        name = type(self).__name__
        extra = d.get("cotnet_amd") or {}
        if self.lookahead_k is None:
            if "slow_state" in d or extra.get("lookahead") is not None:
                raise ValueError(f"{name}.load_state_dict(): the checkpoint carries Lookahead's slow weights and this optimizer was built "
                                 "without the keyword lookahead_k -- they would be dropped silently; build it with lookahead_k (and "
                                 "lookahead_alpha) as the checkpoint's groups say")
            return None
        theirs = d["param_groups"]
        said = {}
        for key in ("lookahead_step", "lookahead_k", "lookahead_alpha"):
            values = {g[key] for g in theirs if key in g}
            if len(values) > 1:
                raise ValueError(f"{name}.load_state_dict(): the groups' {key} are {sorted(values)}; this optimizer keeps ONE count, one k "
                                 "and one alpha in device memory for all of them")
            said[key] = values.pop() if values else None
        k, alpha = self._lookahead_checked(self.lookahead_k if said["lookahead_k"] is None else said["lookahead_k"],
                                           self.lookahead_alpha if said["lookahead_alpha"] is None else said["lookahead_alpha"],
                                           f"{name}.load_state_dict(")
        if self._captured_lookahead is not None and (k, alpha) != self._captured_lookahead:
            raise ValueError(f"{name}.load_state_dict(): step() was captured into a HIP graph with (lookahead_k, lookahead_alpha) = "
                             f"{self._captured_lookahead}, which travel by value and stay in its replays; the checkpoint says {(k, alpha)} "
                             "-- build the optimizer with the checkpoint's values before capturing")
        step = int(said["lookahead_step"] or 0)
        if step < 0:
            raise ValueError(f"{name}.load_state_dict(): negative lookahead_step {step}")
        buffers = None
        if "slow_state" in d:
            slow_state = d["slow_state"]
            indices = [i for g in theirs for i in g["params"]]
            if sorted(map(str, slow_state)) != sorted(map(str, indices)):
                raise ValueError(f"{name}.load_state_dict(): slow_state is keyed by {sorted(map(str, slow_state))[:4]}..., the groups list "
                                 f"the indices {indices}; a slow_state the reference's Lookahead wrote is keyed by id(tensor) of ITS "
                                 "process, which cannot be matched to any parameter here -- only a slow_state keyed by the groups' "
                                 "indices (as state_dict() of this package writes it) is read")
            buffers = {}
            for members, g in zip(self._groups(), theirs):
                for (pname, p), idx in zip(members, g["params"]):
                    s = slow_state.get(idx)
                    buf = (s if s is not None else slow_state.get(str(idx)) or {}).get("slow_buffer")
                    if buf is not None and tuple(buf.shape) != tuple(p.shape):
                        raise ValueError(f"{name}.load_state_dict(): slow_buffer of index {idx} has shape {tuple(buf.shape)}, parameter "
                                         f"'{pname}' at that place has {tuple(p.shape)}")
                    buffers[p] = buf
            held = [b is not None for b in buffers.values()]
            if any(held) and not all(held):
                raise ValueError(f"{name}.load_state_dict(): slow_state holds a slow_buffer for some indices and none for others; this "
                                 "optimizer's slow weights are born together, at the first sync")
            if not any(held):
                buffers = None
        words = extra.get("lookahead")
        if words is not None:
            words = [int(w) for w in words]
            if len(words) != 8 or bool(words[2]) != (buffers is not None):
                raise ValueError(f"{name}.load_state_dict(): cotnet_amd['lookahead'] = {words} is not a block of eight words whose `born` "
                                 f"agrees with slow_state ({'buffers' if buffers is not None else 'no buffers'})")
        else:
            words = [step, 0, 1 if buffers is not None else 0, 0, 0, 0, 0, 0]
        return dict(k=k, alpha=alpha, words=words, buffers=buffers)

    def _lookahead_load(self, plan):
        """write what `_lookahead_plan` returned, in place (inside torch.no_grad())"""
        if plan is None:
            return
        self.lookahead_k, self.lookahead_alpha = plan["k"], plan["alpha"]
        slow = self._slots("slow")
        for st in self.state:
            st["slow"].zero_()  # (padding, and everything where the checkpoint's slow weights are unborn)
        for p, buf in (plan["buffers"] or {}).items():
            slow[p].copy_(buf)
        self.lookahead_state.copy_(torch.tensor(plan["words"], dtype=torch.int32))

    def clip_stats(self):
        """ONE host read of the clip block: dict(total_norm, scale, skip, steps, clipped, skipped) -- the last step's norm, coefficient
        and skip flag, and the counts since construction (or since the caller last zeroed `self.clip_state`).  It synchronises with
        the device, so it belongs at a logging interval, not in every step; refused while a HIP graph is being captured (the read
        would see what the block held before the capture: recorded launches have not run)."""
        if self.clip_state is None:
            raise RuntimeError(f"{type(self).__name__}.clip_stats(): built with neither clip_grad nor skip_nonfinite")
        self._not_while_capturing("clip_stats()")
        w = self.clip_state.cpu()
        scale, total_norm = w[:2].view(torch.float32).tolist()
        skip, steps, clipped, skipped = w[2:6].tolist()
        return dict(total_norm=total_norm, scale=scale, skip=skip, steps=steps, clipped=clipped, skipped=skipped)

    def agc_stats(self):
        """ONE host read of the coefficient tensors: dict(units, clipped, nonfinite, min_coef) of the last step -- how many units
        there are, how many were scaled (coef < 1), how many were left alone because a norm was not finite (coef = NaN), and the
        smallest coefficient (1.0 when nothing clipped).  Like clip_stats() it synchronises with the device and is refused while a HIP
        graph is being captured."""
        if self._agc_coef is None:
            raise RuntimeError(f"{type(self).__name__}.agc_stats(): built without agc")
        self._not_while_capturing("agc_stats()")
        c = torch.cat(self._agc_coef).cpu() if self._agc_coef else torch.zeros(0)
        bad = torch.isnan(c)
        fin = c[~bad]
        return dict(units=c.numel(), clipped=int((fin < 1).sum()), nonfinite=int(bad.sum()),
                    min_coef=float(fin.min()) if fin.numel() else 1.0)

    def agc_coefficients(self):
        """{parameter: view of its coefficients in the bucket's tensor}, of shape [shape[0]], or [1] for a parameter with ndim <= 1:
        what the last step's `cot_agc_clip` launches left (1 = not clipped, NaN = a norm was not finite).  The views stay valid:
        the tensors are never reallocated."""
        if self._agc_coef is None:
            raise RuntimeError(f"{type(self).__name__}.agc_coefficients(): built without agc")
        out = {}
        for b, coef in zip(self.reducer.buckets, self._agc_coef):
            at = 0
            for p in b.params:
                k = 0 if p.numel() == 0 else (1 if p.ndim <= 1 else p.shape[0])
                out[p] = coef[at:at + k]
                at += k
        return out

    def ema_state_dict(self):
        """the averaged weights under the model's own state_dict keys (fp32; integer buffers are copied as they are) --
        what the reference stores as `state_dict_ema` (utils/checkpoint_saver.py:103-120)"""
        assert self.ema_decay is not None, f"{type(self).__name__} was built without ema_decay"
        by_param = self._slots("ema")
        by_buf = {id(bf): e for bf, e in zip(self._buf_src, self._buf_ema)}
        out = {}
        params = dict(self.model.named_parameters())
        bufs = dict(self.model.named_buffers())
        for k in self.model.state_dict().keys():
            if k in params:
                out[k] = by_param[params[k]].clone()
            else:
                bf = bufs[k]
                out[k] = by_buf[id(bf)].clone() if id(bf) in by_buf else bf.detach().clone()
        return out

    @contextlib.contextmanager
    def ema_weights(self):
        """`with opt.ema_weights(): evaler(epoch, model)`: run the AVERAGED weights through the model's own parameters -- what the
        reference does with a second model (`evaler(epoch, model_ema.module)`, train.py:352-355) and `ema_state_dict()` could only
        serve through a clone of every tensor, a second network and its own packings.

        On entry each bucket's flat parameters receive its fp32 average cast to the bucket's dtype (round to nearest even, as
        `.to(torch.bfloat16)` does) and every floating-point buffer its averaged value; the caches keyed on the parameters' version are
        moved on.  The parameters keep their addresses, so a HIP graph that captured the model's forward runs the average when it is
        replayed inside the context.  On exit everything is put back bit for bit and the caches are moved on again: buckets with a
        master from the master (the working copy is always the rounded master), fp32 buckets and the buffers from copies taken on
        entry.  Masters, momentum, the averages and integer buffers are never written.  No step() inside the context; refused while a
        HIP graph is being captured (the recorded copies would swap the weights at every replay)."""
        assert self.ema_decay is not None, f"{type(self).__name__} was built without ema_decay"
        if _lib.capturing():
            raise RuntimeError(f"{type(self).__name__}.ema_weights() inside a HIP-graph capture: the copies would be recorded and swap the weights at "
                               "every replay -- enter the context outside the capture (a captured forward reads the weights when it runs)")
        from . import cot_layer_fused
        buckets = self.reducer.buckets
        device = buckets[0].pflat.device if buckets else None
        kept = [b.pflat.clone() if st["master"] is None else None for b, st in zip(buckets, self.state)]
        kept_bufs = [bf.detach().clone() for bf in self._buf_src]
        with torch.no_grad():
            for b, st in zip(buckets, self.state):
                b.pflat.copy_(st["ema"])
            for bf, e in zip(self._buf_src, self._buf_ema):
                bf.copy_(e)
        if buckets:
            cot_layer_fused.after_optimizer_step(device)
        try:
            yield self
        finally:
            with torch.no_grad():
                for b, st, k in zip(buckets, self.state, kept):
                    b.pflat.copy_(st["master"] if k is None else k)
                for bf, k in zip(self._buf_src, kept_bufs):
                    bf.copy_(k)
            if buckets:
                cot_layer_fused.after_optimizer_step(device)

    def set_lr(self, lr):
        """the rate of the steps issued from here on.

        device_lr=False: cot_sgd_step takes it by value, so a HIP graph that captured step() keeps the rate it was captured with:
        a different rate after such a capture raises, and changes nothing, instead of leaving the replays silently at the old one
        (a schedule over a replayed step would otherwise train at a constant rate).  The captured rate itself is always accepted.
        To move on, capture the step again and call set_lr INSIDE that capture, before step(): while capturing, any rate is
        accepted, and the step() that follows records it.

        device_lr=True: never raises outside a capture.  The rate is written into `self.lr_dev` with one fill on the CURRENT stream
        (the value travels as that fill's kernel argument, rounded to fp32 as the by-value argument is: no host staging buffer that
        a second set_lr could overwrite before the first write ran).  Eager steps and replays issued afterwards read it -- the
        write is ordered on the current stream, so issue the step or the replay on that stream or on one that waits for it.
        WHILE capturing it raises and changes nothing: a recorded fill would put the captured rate back at every replay, the
        silent constant-rate training again -- set the rate outside the capture."""
        lr = float(lr)
        if self.lr_dev is not None:
            if _lib.capturing():
                raise RuntimeError(f"{type(self).__name__}.set_lr({lr:g}) inside a HIP-graph capture: the fill of the device-resident rate would be "
                                   "recorded and reset the rate at every replay -- set the rate outside the capture (replays read "
                                   "lr_dev when they run); the rate is left as it was")
            self.lr = lr
            self.lr_dev.fill_(self.lr)
            return
        if self._captured_lr is not None and lr != self._captured_lr and not _lib.capturing():
            raise RuntimeError(f"{type(self).__name__}.set_lr({lr:g}): step() was captured into a HIP graph at lr = {self._captured_lr:g}, and replays "
                               "keep the captured rate -- capture the step again and set the new rate inside that capture (its "
                               "step() records it); the rate is left as it was")
        self.lr = lr

    def master_parameters(self):
        """fp32 view of every parameter (master copy for bf16 parameters), in module.parameters() order of the buckets"""
        return self._slots("weights")

    # ---- the whole training state, out and in (the reference: CheckpointSaver._save, utils/checkpoint_saver.py:103-120, and
    # resume_checkpoint, models/helpers.py:51-88).  Everything below acts IN PLACE on the allocations made in __init__: no address
    # changes, so a HIP graph captured before a load replays the loaded state.  Everything is refused while capturing.

    STATE_FORMAT = 1

    def _not_while_capturing(self, what):
        if _lib.capturing():
            raise RuntimeError(f"{type(self).__name__}.{what} inside a HIP-graph capture: its copies and launches would be recorded and run again at "
                               "every replay, and a host read cannot be recorded -- save and load between replays (the state keeps its "
                               "addresses: a captured step replays what was loaded); nothing was changed")

    def _groups(self):
        """the reference's two parameter groups (optim/optim_factory.py:19-31): [[(name, parameter)] of no_decay, ... of decay], each in
        named_parameters() order"""
        in_bucket = {p: b.key for b in self.reducer.buckets for p in b.params}
        groups = {"no_decay": [], "decay": []}
        for name, p in self.model.named_parameters():
            if p in in_bucket:
                groups[in_bucket[p]].append((name, p))
        return [groups["no_decay"], groups["decay"]]

    def _slots(self, array):
        """{parameter: view of its slot in the buckets' `array`} ('weights': the master, or the fp32 parameters where there is none)"""
        out = {}
        for b, st in zip(self.reducer.buckets, self.state):
            flat = self._weights(b, st) if array == "weights" else st[array]
            for p, off in zip(b.params, b.offs):
                out[p] = flat[off:off + p.numel()].view_as(p)
        return out

    def model_state_dict(self):
        """the model's state_dict() keys with every parameter that has a master given as that fp32 master, every other parameter and
        buffer as it is (clones): what the reference stores under `state_dict` (utils/checkpoint_saver.py:107), at the precision the
        optimizer steps at.  `model.state_dict()` would hold the bf16 roundings."""
        self._not_while_capturing("model_state_dict()")
        weights = self._slots("weights")
        params = dict(self.model.named_parameters())
        out = {}
        for k, v in self.model.state_dict().items():
            p = params.get(k)
            out[k] = (weights[p] if p is not None and p in weights else v).detach().clone()
        return out

    @staticmethod
    def _strip(sd):
        return {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}

    def _check_keys(self, sd, strict, shapes):
        """missing / unexpected keys as nn.Module.load_state_dict reports them, and the shapes of those present"""
        keys = list(self.model.state_dict().keys())
        missing = [k for k in keys if k not in sd]
        unexpected = [k for k in sd if k not in shapes]
        errors = [f"size mismatch for {k}: copying a param with shape {tuple(sd[k].shape)} from checkpoint, the shape in current model is "
                  f"{tuple(shapes[k])}." for k in keys if k in sd and tuple(sd[k].shape) != tuple(shapes[k])]
        if strict:
            if unexpected:
                errors.insert(0, "Unexpected key(s) in state_dict: {}. ".format(", ".join(f'"{k}"' for k in unexpected)))
            if missing:
                errors.insert(0, "Missing key(s) in state_dict: {}. ".format(", ".join(f'"{k}"' for k in missing)))
        if errors:
            raise RuntimeError("Error(s) in loading state_dict for {}:\n\t{}".format(type(self.model).__name__, "\n\t".join(errors)))
        return nn.modules.module._IncompatibleKeys(missing, unexpected)

    def load_model_state_dict(self, sd, strict=True):
        """the inverse of model_state_dict(): the masters receive the fp32 values, each working copy its master rounded to the bucket's
        dtype (the invariant ema_weights() relies on), fp32 buckets and every other parameter and buffer the values themselves; the
        caches keyed on the parameters move on.  A `module.` prefix is stripped.  `model.load_state_dict` alone would write the working
        copies only, and the next step() would put the stale masters back over them.  strict: missing and unexpected keys raise, as
        nn.Module.load_state_dict's do, before anything is written."""
        self._not_while_capturing("load_model_state_dict()")
        sd = self._strip(sd)
        live = self.model.state_dict()
        keys = self._check_keys(sd, strict, {k: v.shape for k, v in live.items()})
        weights = self._slots("weights")
        params = dict(self.model.named_parameters())
        with torch.no_grad():
            for k, v in live.items():
                if k in sd:
                    p = params.get(k)
                    (weights[p] if p is not None and p in weights else v).copy_(sd[k])
            for b, st in zip(self.reducer.buckets, self.state):
                if st["master"] is not None:
                    b.pflat.copy_(st["master"])
        if self.reducer.buckets:
            from . import cot_layer_fused
            cot_layer_fused.after_optimizer_step(self.reducer.buckets[0].pflat.device)
        return keys

    def _clip_words(self):
        return self.clip_state.cpu().tolist() if self.clip_state is not None else None

    def state_dict(self):
        """torch.optim.SGD's own layout over the reference's groups (optim/optim_factory.py:19-31, :54-56): param_groups =
        [no_decay, decay], each listing its parameters in named_parameters() order with indices running on across the groups,
        state[idx] = {'momentum_buffer': fp32 tensor of the parameter's shape}, the hyper-parameters (lr, momentum, dampening 0,
        weight_decay, nesterov) in the groups -- torch.optim.SGD over the same groups of an fp32 twin loads its 'state' and
        'param_groups'.  One more top-level key, 'cotnet_amd', holds what that layout cannot: format, device_lr (whether the rate lives
        on the device) and clip_state (the eight words of the clip block: last coefficient and norm, the counters; None without one).
        Built with lookahead_k, Lookahead's part joins in the reference's layout (`_lookahead_saved`)."""
        self._not_while_capturing("state_dict()")
        momentum, groups, state, at = self._slots("mom"), [], {}, 0
        for members, wd in zip(self._groups(), (0.0, self.weight_decay)):
            idx = list(range(at, at + len(members)))
            at += len(members)
            groups.append(dict(lr=self.lr, momentum=self.momentum, dampening=0, weight_decay=wd, nesterov=bool(self.nesterov), params=idx))
            for i, (_, p) in zip(idx, members):
                state[i] = {"momentum_buffer": momentum[p].detach().clone()}
        extra = dict(format=self.STATE_FORMAT, device_lr=self.lr_dev is not None, clip_state=self._clip_words())
        return self._lookahead_saved({"state": state, "param_groups": groups, "cotnet_amd": extra})

    def load_state_dict(self, d):
        """the inverse of state_dict().  Parameters are matched by group ([no_decay, decay]) and position, their shapes checked, all
        before anything is written.  A dict without 'cotnet_amd' is accepted (a checkpoint the reference wrote): hyper-parameter keys a
        group lacks keep the constructor's values, an index without a momentum_buffer (torch before its first step) gives zero momentum
        -- with dampening 0 the same next step.  lr goes through set_lr (its rules hold).  Lookahead's part: `_lookahead_plan` -- a
        dict without slow_state loads unborn at the groups' lookahead_step; slow weights offered to an optimizer built without
        lookahead_k are refused, not dropped."""
        self._not_while_capturing("load_state_dict()")
        ours, theirs = self._groups(), d["param_groups"]
        if len(theirs) != 2 or [len(g["params"]) for g in theirs] != [len(g) for g in ours]:
            raise ValueError(f"FlatSGD.load_state_dict(): param_groups of {[len(g['params']) for g in theirs]} parameters, this optimizer "
                             f"has [no_decay, decay] = {[len(g) for g in ours]} (the reference's add_weight_decay order)")
        hp = {}
        for key, group, default in (("lr", 0, self.lr), ("momentum", 0, self.momentum), ("nesterov", 0, self.nesterov),
                                    ("weight_decay", 1, self.weight_decay)):
            hp[key] = theirs[group].get(key, default)
        if any(g.get("dampening", 0) != 0 for g in theirs) or theirs[0].get("weight_decay", 0.0) != 0.0 \
                or any(g.get(k, hp[k]) != hp[k] for g in theirs for k in ("lr", "momentum", "nesterov")):
            raise ValueError("FlatSGD.load_state_dict(): the step kernels take one lr / momentum / nesterov for both groups, dampening 0 and "
                             f"no weight decay on the first group; the checkpoint's groups say {[{k: v for k, v in g.items() if k != 'params'} for g in theirs]}")
        state = d.get("state", {})
        values = {}
        for members, g in zip(ours, theirs):
            for (name, p), idx in zip(members, g["params"]):
                buf = (state.get(idx) or state.get(str(idx)) or {}).get("momentum_buffer")
                if buf is not None and tuple(buf.shape) != tuple(p.shape):
                    raise ValueError(f"FlatSGD.load_state_dict(): momentum_buffer of index {idx} has shape {tuple(buf.shape)}, "
                                     f"parameter '{name}' at that place has {tuple(p.shape)}")
                values[p] = buf
        extra = d.get("cotnet_amd") or {}
        if extra and extra.get("format") != self.STATE_FORMAT:
            raise ValueError(f"FlatSGD.load_state_dict(): 'cotnet_amd' format {extra.get('format')!r}, this build reads {self.STATE_FORMAT}")
        lookahead = self._lookahead_plan(d)
        self.set_lr(hp["lr"])
        self.momentum, self.weight_decay, self.nesterov = float(hp["momentum"]), float(hp["weight_decay"]), bool(hp["nesterov"])
        mom = self._slots("mom")
        with torch.no_grad():
            self._lookahead_load(lookahead)
            for p, buf in values.items():
                mom[p].zero_() if buf is None else mom[p].copy_(buf)
            words = extra.get("clip_state")
            if self.clip_state is not None and words is not None:
                self.clip_state.copy_(torch.tensor(words, dtype=torch.int32))

    def load_ema_state_dict(self, sd=None):
        """the inverse of ema_state_dict(), averaged buffers included (a `module.` prefix is stripped; integer buffers belong to the model
        and are not touched).  sd None -- a checkpoint without `state_dict_ema` -- sets the average from the weights as they are now
        (load the model first), as the reference's load_checkpoint(model_ema.module, resume, use_ema=True) does when the key is missing
        (train.py:125-126, models/helpers.py:28-30)."""
        assert self.ema_decay is not None, f"{type(self).__name__} was built without ema_decay"
        self._not_while_capturing("load_ema_state_dict()")
        with torch.no_grad():
            if sd is None:
                for b, st in zip(self.reducer.buckets, self.state):
                    st["ema"].copy_(self._weights(b, st))
                for bf, e in zip(self._buf_src, self._buf_ema):
                    e.copy_(bf)
                return
            sd = self._strip(sd)
            live = self.model.state_dict()
            self._check_keys(sd, True, {k: v.shape for k, v in live.items()})
            ema = self._slots("ema")
            params = dict(self.model.named_parameters())
            by_buf = {id(bf): e for bf, e in zip(self._buf_src, self._buf_ema)}
            bufs = dict(self.model.named_buffers())
            for k in live:
                p = params.get(k)
                if p is not None and p in ema:
                    ema[p].copy_(sd[k])
                elif k in bufs and id(bufs[k]) in by_buf:
                    by_buf[id(bufs[k])].copy_(sd[k])
