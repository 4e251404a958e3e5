"""Learning-rate schedules, on the host: the reference's scheduler/ package restated over one rate.

Every recipe (cot_experiments/*/config.yaml) trains on `sched: cosine` with a linear warm-up: 350 epochs, five warm-up epochs from
1e-4 up to 0.25, floor 1e-5, one cycle -- scheduler/cosine_lr.py:68-95 stepped once per epoch by train.py:139,:284,:361.
`CosineSchedule` restates what those recipes use of it: linear warm-up, ONE cosine cycle (`t_mul = 1`, `cycle_limit = 1`), `lr_min`
once the cycle is over.  The rest of what `cfg.solver.sched` can name is below it:

    scheduler/cosine_lr.py    -> CosineLRSchedule    restarts (t_mul, cycle_limit), decay_rate per cycle, warm-up prefix
    scheduler/tanh_lr.py      -> TanhLRSchedule      the same clock under a tanh
    scheduler/step_lr.py      -> StepLRSchedule      base * decay_rate ** (t // decay_t)
    scheduler/plateau_lr.py   -> PlateauLRSchedule   torch's ReduceLROnPlateau rule on the validation metric; stateful
    scheduler/scheduler.py:87-105 (_add_noise)       the `noise_*` keywords of all four
    scheduler/scheduler_factory.py -> create_scheduler(sched, epochs=..., lr=..., ...) -> (schedule, num_epochs)

The doubles are the reference's, bit for bit (tests/golden/lr_schedule_cosine.json, tests/golden/lr_schedules.json): the order of
operations below is its order.  Not restated: `noise_type='uniform'`, which the reference's factory cannot reach.

ONE value per schedule: the reference keeps a rate per param group, all scaled from each group's own base; the flat optimizers
keep one rate for both of their groups (decay, no_decay), so each schedule yields one double.

The rate stays a host decision: `apply(opt, t)` hands it to `FlatSGD.set_lr`, which with `device_lr=True` writes it where the
replayed step kernels read it.  `Trainer` calls `apply(opt, t)`, and `apply(opt, t, metric)` where the class says `needs_metric`.
"""
import math

import torch


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


_NOISE = dict(noise_range_t=None, noise_pct=0.67, noise_std=1.0, noise_seed=42)


class _Noisy:
    """The `**noise` keywords every schedule below takes, and scheduler/scheduler.py:87-105: active when `lo <= t < hi` for a pair
    `noise_range_t`, or `t >= noise_range_t` for a scalar; a fresh `torch.Generator` seeded `noise_seed + t`; `torch.randn(1)` redrawn
    until `abs(noise) < noise_pct`; the rate becomes `lr + lr * noise`.  `noise_std` is accepted and unused, as in the reference.
    A pure function of (t, noise_seed): a resumed run draws the uninterrupted run's noise."""
    needs_metric = False

    def _init_noise(self, noise):
        unknown = set(noise) - set(_NOISE)
        if unknown:
            raise TypeError(f"{type(self).__name__}(): unexpected keyword(s) {sorted(unknown)}; the noise keywords are {sorted(_NOISE)}")
        noise = {**_NOISE, **noise}
        self.noise_range_t, self.noise_pct, self.noise_std = noise["noise_range_t"], noise["noise_pct"], noise["noise_std"]
        self.noise_seed = noise["noise_seed"] if noise["noise_seed"] is not None else 42

    def _noise_at(self, t):
        """-> the factor's noise at t, or None where the range leaves t out"""
        r = self.noise_range_t
        if r is None:
            return None
        if not (r[0] <= t < r[1] if isinstance(r, (list, tuple)) else t >= r):
            return None
        g = torch.Generator()
        g.manual_seed(self.noise_seed + t)
        while True:  # (resample what falls outside the limit, scheduler.py:97-101)
            noise = torch.randn(1, generator=g).item()
            if abs(noise) < self.noise_pct:
                return noise

    def _add_noise(self, lr, t):
        noise = self._noise_at(t)
        return lr if noise is None else lr + lr * noise

    def value(self, t):
        """the rate at t, noise included; nothing is kept between calls"""
        return float(self._add_noise(self._get_lr(t), t))

    def apply(self, opt, t, metric=None):
        """opt.set_lr(value(t)); returns the rate.  `metric` is ignored: only a schedule with `needs_metric` reads it."""
        lr = self.value(t)
        opt.set_lr(lr)
        return lr


class _Cyclic(_Noisy):
    """what scheduler/cosine_lr.py and scheduler/tanh_lr.py share: the warm-up, the cycle clock and get_cycle_length"""

    def _init_cycles(self, base_lr, t_initial, t_mul, lr_min, decay_rate, warmup_t, warmup_lr_init, warmup_prefix, cycle_limit, noise):
        assert t_initial > 0 and lr_min >= 0 and cycle_limit >= 0 and warmup_t >= 0
        self._init_noise(noise)
        self.base_lr, self.t_initial, self.t_mul, self.lr_min, self.decay_rate = base_lr, t_initial, t_mul, lr_min, decay_rate
        self.warmup_t, self.warmup_lr_init, self.warmup_prefix, self.cycle_limit = warmup_t, warmup_lr_init, warmup_prefix, cycle_limit

    def _cycle(self, t):
        """-> (i, t_i, t_curr): the cycle t falls in, its length and the time into it (cosine_lr.py:72-82), t past the warm-up"""
        if self.warmup_prefix:
            t = t - self.warmup_t
        if self.t_mul != 1:
            i = math.floor(math.log(1 - t / self.t_initial * (1 - self.t_mul), self.t_mul))
            t_i = self.t_mul ** i * self.t_initial
            t_curr = t - (1 - self.t_mul ** i) / (1 - self.t_mul) * self.t_initial
        else:
            i = t // self.t_initial
            t_i = self.t_initial
            t_curr = t - (self.t_initial * i)
        return i, t_i, t_curr

    def _running(self, i):
        return self.cycle_limit == 0 or (self.cycle_limit > 0 and i < self.cycle_limit)

    def get_cycle_length(self, cycles=0):
        """the epochs that `cycles` cycles (default: cycle_limit, at least one) take: cosine_lr.py:109-116"""
        if not cycles:
            cycles = self.cycle_limit
        cycles = max(1, cycles)
        if self.t_mul == 1.0:
            return self.t_initial * cycles
        return int(math.floor(-self.t_initial * (self.t_mul ** cycles - 1) / (1 - self.t_mul)))


class CosineLRSchedule(_Cyclic):
    """scheduler/cosine_lr.py:68-95: cosine decay with restarts (arXiv 1608.03983).  Cycle i is `t_mul ** i * t_initial` long and runs
    from `base_lr * decay_rate ** i` down to `lr_min * decay_rate ** i`; past `cycle_limit` cycles (0: no limit) the rate is the plain
    `lr_min`.  With `warmup_prefix` the cycles' clock starts behind the warm-up; without it the clock is t itself.  With t_mul = 1,
    cycle_limit = 1 and no noise this is `CosineSchedule`, bit for bit."""

    def __init__(self, base_lr, t_initial, t_mul=1., lr_min=0., decay_rate=1., warmup_t=0, warmup_lr_init=0, warmup_prefix=False,
                 cycle_limit=0, **noise):
        self._init_cycles(base_lr, t_initial, t_mul, lr_min, decay_rate, warmup_t, warmup_lr_init, warmup_prefix, cycle_limit, noise)
        self.warmup_step = (base_lr - warmup_lr_init) / warmup_t if warmup_t else 1

    def _get_lr(self, t):
        if t < self.warmup_t:
            return self.warmup_lr_init + t * self.warmup_step
        i, t_i, t_curr = self._cycle(t)
        gamma = self.decay_rate ** i
        lr_min = self.lr_min * gamma
        lr_max = self.base_lr * gamma
        if self._running(i):
            return lr_min + 0.5 * (lr_max - lr_min) * (1 + math.cos(math.pi * t_curr / t_i))
        return self.lr_min


class TanhLRSchedule(_Cyclic):
    """scheduler/tanh_lr.py:64-99: hyperbolic-tangent decay with restarts (arXiv 1806.01593), tanh taken over [lb, ub] across each
    cycle.  Two things differ from the cosine besides the curve: without `warmup_prefix` the warm-up climbs to the curve's own value
    at `warmup_t`, not to the base rate (:65-66), and past the cycle limit the rate is `lr_min * decay_rate ** cycle_limit` (:98)."""

    def __init__(self, base_lr, t_initial, lb=-6., ub=4., t_mul=1., lr_min=0., decay_rate=1., warmup_t=0, warmup_lr_init=0,
                 warmup_prefix=False, cycle_limit=0, **noise):
        assert lb < ub and warmup_lr_init >= 0
        self._init_cycles(base_lr, t_initial, t_mul, lr_min, decay_rate, warmup_t, warmup_lr_init, warmup_prefix, cycle_limit, noise)
        self.lb, self.ub = lb, ub
        if warmup_t:
            target = base_lr if warmup_prefix else self._get_lr(warmup_t)  # (t = warmup_t is past the warm-up: the curve's value)
            self.warmup_step = (target - warmup_lr_init) / warmup_t
        else:
            self.warmup_step = 1

    def _get_lr(self, t):
        if t < self.warmup_t:
            return self.warmup_lr_init + t * self.warmup_step
        i, t_i, t_curr = self._cycle(t)
        if self._running(i):
            gamma = self.decay_rate ** i
            lr_min = self.lr_min * gamma
            lr_max = self.base_lr * gamma
            tr = t_curr / t_i
            return lr_min + 0.5 * (lr_max - lr_min) * (1 - math.tanh(self.lb * (1. - tr) + self.ub * tr))
        return self.lr_min * (self.decay_rate ** self.cycle_limit)


class StepLRSchedule(_Noisy):
    """scheduler/step_lr.py:46-51: a linear warm-up, then `base_lr * decay_rate ** (t // decay_t)`.  `decay_t` may be a float
    (`decay_epochs: 2.4`): the floor division and the power are then the floats' own."""

    def __init__(self, base_lr, decay_t, decay_rate=1., warmup_t=0, warmup_lr_init=0, **noise):
        assert decay_t > 0 and warmup_t >= 0
        self._init_noise(noise)
        self.base_lr, self.decay_t, self.decay_rate, self.warmup_t, self.warmup_lr_init = base_lr, decay_t, decay_rate, warmup_t, warmup_lr_init
        self.warmup_step = (base_lr - warmup_lr_init) / warmup_t if warmup_t else 1

    def _get_lr(self, t):
        if t < self.warmup_t:
            return self.warmup_lr_init + t * self.warmup_step
        return self.base_lr * (self.decay_rate ** (t // self.decay_t))


class PlateauLRSchedule(_Noisy):
    """scheduler/plateau_lr.py:72-113 over the rule of `torch.optim.lr_scheduler.ReduceLROnPlateau` (threshold_mode 'rel', eps 1e-8),
    whose few lines are restated here over the one rate: STATEFUL, stepped once per epoch with the validation metric.

    `apply(opt, t, metric)`: while `t <= warmup_t` (inclusive, :73) the rate is `warmup_lr_init + t * warmup_step` and the plateau
    rule is not stepped.  Afterwards the previous call's noise is undone (`restore_lr`, :77-81); the rule judges the metric -- better
    than `best` by the relative threshold or one more bad epoch; more than `patience_t` of them multiply the CURRENT rate (not the base
    rate) by `decay_rate`, down to `lr_min`, and start `cooldown_t` epochs in which bad epochs do not count --; then noise is laid on
    top and the rate before it kept in `restore_lr` (:85-113).  `self.lr` is the rate last handed out.

    `apply(opt, t, None)` past the warm-up is the resume call (train.py:138-139, where the reference's would raise on float(None)):
    nothing is stepped and nothing is set; the optimizer's own rate, which a resume has just loaded, becomes the current one.
    DEPARTURE: with `warmup_t = 0` there is no warm-up branch at all.  The reference's `epoch <= 0` would set the rate to
    `warmup_lr_init` at epoch 0 for good -- a call its train.py never makes (`start_epoch > 0`, :138), and `Trainer.fit` always does.

    `state_dict()` / `load_state_dict()` carry best, last_epoch, num_bad_epochs, cooldown_counter, lr and restore_lr.  No checkpoint
    file stores them (the reference's stores no scheduler): a resumed run restarts the counters, as the reference's does."""
    needs_metric = True
    EPS = 1e-8  # ReduceLROnPlateau's: a smaller reduction is ignored
    STATE = ("best", "last_epoch", "num_bad_epochs", "cooldown_counter", "lr", "restore_lr")

    def __init__(self, base_lr, decay_rate=0.1, patience_t=10, threshold=1e-4, cooldown_t=0, warmup_t=0, warmup_lr_init=0, lr_min=0,
                 mode='max', **noise):
        if mode not in ("min", "max"):
            raise ValueError(f"PlateauLRSchedule(mode={mode!r}): 'min' or 'max'")
        if decay_rate >= 1.0:
            raise ValueError("PlateauLRSchedule(decay_rate=...): a factor < 1.0")
        self._init_noise(noise)
        self.base_lr, self.decay_rate, self.patience_t, self.threshold, self.cooldown_t = base_lr, decay_rate, patience_t, threshold, cooldown_t
        self.warmup_t, self.warmup_lr_init, self.lr_min, self.mode = warmup_t, warmup_lr_init, lr_min, mode
        self.warmup_step = (base_lr - warmup_lr_init) / warmup_t if warmup_t else 1
        self.best = math.inf if mode == "min" else -math.inf
        self.last_epoch = self.num_bad_epochs = self.cooldown_counter = 0
        self.lr = float(warmup_lr_init if warmup_t else base_lr)
        self.restore_lr = None

    def value(self, t):
        raise TypeError("PlateauLRSchedule has no value(t): its rate depends on the metrics it was stepped with -- "
                        "apply(opt, t, metric) returns the rate, and `lr` holds the last one")

    def _is_better(self, a):
        if self.mode == "min":
            rel_epsilon = 1.0 - self.threshold
            return a < self.best * rel_epsilon
        rel_epsilon = self.threshold + 1.0
        return a > self.best * rel_epsilon

    def _step_rule(self, metric, epoch):
        """ReduceLROnPlateau.step on self.lr"""
        current = float(metric)
        self.last_epoch = epoch
        if self._is_better(current):
            self.best = current
            self.num_bad_epochs = 0
        else:
            self.num_bad_epochs += 1
        if self.cooldown_counter > 0:
            self.cooldown_counter -= 1
            self.num_bad_epochs = 0  # (bad epochs in the cool-down do not count)
        if self.num_bad_epochs > self.patience_t:
            old_lr = float(self.lr)
            new_lr = max(old_lr * self.decay_rate, self.lr_min)
            if old_lr - new_lr > self.EPS:
                self.lr = new_lr
            self.cooldown_counter = self.cooldown_t
            self.num_bad_epochs = 0

    def apply(self, opt, t, metric=None):
        if self.warmup_t and t <= self.warmup_t:
            self.lr = self.warmup_lr_init + t * self.warmup_step
        elif metric is None:
            if hasattr(opt, "lr"):
                self.lr = opt.lr
            return self.lr
        else:
            if self.restore_lr is not None:
                self.lr = self.restore_lr
                self.restore_lr = None
            self._step_rule(metric, t)
            noise = self._noise_at(t)
            if noise is not None:
                old_lr = float(self.lr)
                self.restore_lr = old_lr
                self.lr = old_lr + old_lr * noise
        opt.set_lr(self.lr)
        return self.lr

    def state_dict(self):
        return {k: getattr(self, k) for k in self.STATE}

    def load_state_dict(self, state):
        missing = [k for k in self.STATE if k not in state]
        if missing:
            raise KeyError(f"PlateauLRSchedule.load_state_dict: missing {missing}")
        for k in self.STATE:
            setattr(self, k, state[k])


SCHEDULERS = ("cosine", "tanh", "step", "plateau")


def create_scheduler(sched, *, epochs, lr, min_lr=1e-5, warmup_lr=1e-4, warmup_epochs=0, decay_epochs=30, decay_rate=0.1,
                     patience_epochs=10, cooldown_epochs=0, lr_noise=None, lr_noise_pct=0.67, lr_noise_std=1.0, lr_cycle_mul=1.0,
                     lr_cycle_limit=1, seed=42, eval_metric='top1'):
    """scheduler/scheduler_factory.py:10-87 -> (schedule, num_epochs): the keywords are `cfg.solver`'s, plus `cfg.seed` and
    `cfg.eval.eval_metric`; every schedule counts epochs.

    `lr_noise` holds fractions of `epochs`: two make the pair `noise_range_t`, one a scalar, none (or None) no noise.  For cosine and
    tanh `num_epochs` is the cycles' length plus `cooldown_epochs` (:41, :57) -- train for THAT many; for step and plateau it is
    `epochs`.  As in the reference, the cosine takes `decay_rate`, the tanh does not, the plateau's mode is 'min' where 'loss' is in
    `eval_metric` and its cool-down is 0.
    DEPARTURE: `seed` goes through `int(seed)`.  The recipes carry `seed: 1.0`, which `Generator.manual_seed` refuses: in the
    reference `lr_noise` cannot run with the shipped configs."""
    num_epochs = epochs
    if lr_noise is not None and not isinstance(lr_noise, (list, tuple)):
        noise_range = lr_noise * num_epochs
    elif lr_noise is not None and len(lr_noise) > 0:
        noise_range = [n * num_epochs for n in lr_noise]
        if len(noise_range) == 1:
            noise_range = noise_range[0]
    else:
        noise_range = None
    noise = dict(noise_range_t=noise_range, noise_pct=lr_noise_pct, noise_std=lr_noise_std, noise_seed=int(seed))
    if sched == "cosine":
        schedule = CosineLRSchedule(lr, t_initial=num_epochs, t_mul=lr_cycle_mul, lr_min=min_lr, decay_rate=decay_rate,
                                    warmup_lr_init=warmup_lr, warmup_t=warmup_epochs, cycle_limit=lr_cycle_limit, **noise)
        num_epochs = schedule.get_cycle_length() + cooldown_epochs
    elif sched == "tanh":
        schedule = TanhLRSchedule(lr, t_initial=num_epochs, t_mul=lr_cycle_mul, lr_min=min_lr, warmup_lr_init=warmup_lr,
                                  warmup_t=warmup_epochs, cycle_limit=lr_cycle_limit, **noise)
        num_epochs = schedule.get_cycle_length() + cooldown_epochs
    elif sched == "step":
        schedule = StepLRSchedule(lr, decay_t=decay_epochs, decay_rate=decay_rate, warmup_lr_init=warmup_lr, warmup_t=warmup_epochs, **noise)
    elif sched == "plateau":
        mode = "min" if "loss" in eval_metric else "max"
        schedule = PlateauLRSchedule(lr, decay_rate=decay_rate, patience_t=patience_epochs, lr_min=min_lr, mode=mode,
                                     warmup_lr_init=warmup_lr, warmup_t=warmup_epochs, cooldown_t=0, **noise)
    else:
        raise ValueError(f"create_scheduler(sched={sched!r}): one of {', '.join(SCHEDULERS)}")
    return schedule, num_epochs
