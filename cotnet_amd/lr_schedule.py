"""The learning-rate schedule of the reference's recipes, on the host.

Every recipe (cot_experiments/*/config.yaml) trains on `sched: cosine` with a linear warm-up: 350 epochs, five warm-up epochs from
1e-4 up to 0.25, floor 1e-5, one cycle -- scheduler/cosine_lr.py:68-95 stepped once per epoch by train.py:139,:284,:361.  This module
restates what those recipes use of it: linear warm-up, ONE cosine cycle (`t_mul = 1`, `cycle_limit = 1`), `lr_min` once the cycle is
over.  Restarts, noise and the other schedulers are out of scope.  The doubles are the reference's, bit for bit
(tests/golden/lr_schedule_cosine.json): the order of operations below is its order.

The rate stays a host decision: `apply(opt, t)` hands it to `FlatSGD.set_lr`, which with `device_lr=True` writes it where the
replayed SGD kernels read it.
"""
import math


class CosineSchedule:
    def __init__(self, base_lr, t_initial, warmup_t=0, warmup_lr_init=0.0, lr_min=0.0):
        """`t` is whatever the caller counts -- epochs as in the reference, or updates"""
        assert t_initial > 0 and lr_min >= 0 and warmup_t >= 0
        self.base_lr, self.t_initial, self.warmup_t = base_lr, t_initial, warmup_t
        self.warmup_lr_init, self.lr_min = warmup_lr_init, lr_min
        self.warmup_step = (base_lr - warmup_lr_init) / warmup_t if warmup_t else 1

    def value(self, t):
        if t < self.warmup_t:
            return float(self.warmup_lr_init + t * self.warmup_step)
        if t >= self.t_initial:  # the one cycle is over
            return float(self.lr_min)
        # (no warm-up prefix: the cosine's clock is t itself, so the first step after the warm-up may jump, as in the reference)
        return float(self.lr_min + 0.5 * (self.base_lr - self.lr_min) * (1 + math.cos(math.pi * t / self.t_initial)))

    def apply(self, opt, t):
        """opt.set_lr(value(t)); returns the rate"""
        lr = self.value(t)
        opt.set_lr(lr)
        return lr
