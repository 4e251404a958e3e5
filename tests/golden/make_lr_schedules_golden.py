"""tests/golden/make_lr_schedules_golden.py -- the rates of all four schedulers FROM THE REFERENCE ITSELF, written next to this file.

The reference's own `CosineLRScheduler`, `TanhLRScheduler`, `StepLRScheduler` and `PlateauLRScheduler` (scheduler/*.py) are imported
where they lie and stepped over a `torch.optim.SGD` param group, `step(t)` for t = 0 ... count - 1 (the plateau: `step(t, metrics[t])`);
what each call leaves in `param_groups[0]["lr"]` is recorded as the `repr` of the double, so the fixture round-trips exactly.  Data
only: settings, metrics and rates.

    lr_schedules.json   {case: {"kind", "settings": {"lr", ...the scheduler's keywords}, "metrics": [...] (plateau only),
                                "cycle_length": int (cosine, tanh), "lr": [repr(rate at t) ...]}}

`PlateauLRScheduler.__init__` passes `verbose=` to `ReduceLROnPlateau`, which torch no longer takes: for the duration of that
construction, and here only, the class is wrapped so that the keyword is dropped.

    python tests/golden/make_lr_schedules_golden.py
"""
import contextlib
import json
import os
import sys
import warnings

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402

RESTARTS = dict(lr=0.1, t_initial=8, t_mul=1, lr_min=1e-3, decay_rate=0.5, warmup_t=2, warmup_lr_init=1e-4, cycle_limit=0)
TANH = dict(lr=0.1, t_initial=8, t_mul=1, lr_min=1e-3, decay_rate=0.5, warmup_t=3, warmup_lr_init=1e-4, cycle_limit=2)
STEP = dict(lr=0.1, decay_t=4, decay_rate=0.5, warmup_t=3, warmup_lr_init=1e-4)
PLATEAU = dict(lr=0.1, decay_rate=0.1, patience_t=2, cooldown_t=1, warmup_t=3, warmup_lr_init=1e-4, lr_min=1e-4, threshold=1e-4)
PAIR, SCALAR = dict(noise_range_t=[5, 14], noise_pct=0.67, noise_std=1.0, noise_seed=42), dict(noise_range_t=9, noise_pct=0.4, noise_seed=7)

# a top-1 that rises, stalls (three reductions, 0.1 -> 1e-4 = lr_min, each behind patience 2 and a cool-down of 1), recovers once within
# the relative threshold only (no improvement) and once for real, and stalls on at lr_min where nothing is left to reduce
TOP1 = [0., 0., 0., 0., 10., 20., 30., 30., 29., 30.002, 28., 31., 31., 30., 31., 30., 29., 31., 31., 31., 31., 30., 31., 40., 39., 38., 37., 36.,
        35., 34., 33., 32.]
LOSS = [9., 9., 9., 9., 5., 4., 3., 3., 3.1, 2.9998, 3.2, 2.5, 2.5, 2.6, 2.5, 2.6, 2.7, 2.5, 2.5, 2.5, 2.5, 2.6, 2.5, 1.0, 1.1, 1.2, 1.3, 1.4,
        1.5, 1.6, 1.7, 1.8]

CASES = {
    # name: (kind, settings, count[, metrics])
    "cosine_restarts": ("cosine", RESTARTS, 30),  # t_mul = 1, no cycle limit: the integer arithmetic, gamma per cycle
    "cosine_tmul2_limit3_prefix": ("cosine", dict(lr=0.1, t_initial=4, t_mul=2, lr_min=1e-3, decay_rate=0.5, warmup_t=3, warmup_lr_init=1e-4,
                                                  warmup_prefix=True, cycle_limit=3), 40),  # 3 + 4 + 8 + 16 = 31 < 40: past the last cycle
    "cosine_tmul1p5": ("cosine", dict(lr=0.1, t_initial=5, t_mul=1.5, lr_min=1e-3, decay_rate=0.8, cycle_limit=0), 36),
    "cosine_recipe": ("cosine", dict(lr=0.25, t_initial=350, t_mul=1.0, lr_min=1e-5, decay_rate=0.1, warmup_t=5, warmup_lr_init=1e-4,
                                     cycle_limit=1), 40),  # (t = 0 ... 351 of these settings: lr_schedule_cosine.json)
    "cosine_noise_pair": ("cosine", dict(RESTARTS, **PAIR), 30),
    "cosine_noise_scalar": ("cosine", dict(RESTARTS, **SCALAR), 30),
    "tanh_limit2_warmup": ("tanh", TANH, 24),  # no prefix: the warm-up climbs to the curve's value at warmup_t; past cycle 2
    "tanh_tmul2": ("tanh", dict(lr=0.1, t_initial=4, t_mul=2.0, lr_min=1e-3, decay_rate=0.7, warmup_t=2, warmup_lr_init=1e-4,
                                warmup_prefix=True, cycle_limit=0, lb=-5., ub=3.), 34),
    "tanh_noise_pair": ("tanh", dict(TANH, **PAIR), 24),
    "tanh_noise_scalar": ("tanh", dict(TANH, **SCALAR), 24),
    "step_int_warmup": ("step", STEP, 20),
    "step_float": ("step", dict(lr=0.1, decay_t=2.5, decay_rate=0.3), 20),
    "step_noise_pair": ("step", dict(STEP, **PAIR), 20),
    "step_noise_scalar": ("step", dict(STEP, **SCALAR), 20),
    "plateau_max": ("plateau", dict(PLATEAU, mode="max"), len(TOP1), TOP1),
    "plateau_min": ("plateau", dict(PLATEAU, mode="min"), len(LOSS), LOSS),
    "plateau_max_noise": ("plateau", dict(PLATEAU, mode="max", **dict(PAIR, noise_range_t=[6, 20])), len(TOP1), TOP1),  # restore_lr
    "plateau_min_noise_scalar": ("plateau", dict(PLATEAU, mode="min", **SCALAR), len(LOSS), LOSS),
}


@contextlib.contextmanager
def plateau_without_verbose():
    real = torch.optim.lr_scheduler.ReduceLROnPlateau

    def wrapped(optimizer, *a, verbose=None, **kw):
        return real(optimizer, *a, **kw)
    torch.optim.lr_scheduler.ReduceLROnPlateau = wrapped
    try:
        yield
    finally:
        torch.optim.lr_scheduler.ReduceLROnPlateau = real


def run(kind, settings, count, metrics=None):
    from scheduler.cosine_lr import CosineLRScheduler  # the reference's
    from scheduler.plateau_lr import PlateauLRScheduler
    from scheduler.step_lr import StepLRScheduler
    from scheduler.tanh_lr import TanhLRScheduler
    kw = dict(settings)
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=kw.pop("lr"), momentum=0.9, nesterov=True)
    out = {"kind": kind, "settings": settings}
    if kind == "plateau":
        with plateau_without_verbose():
            sched = PlateauLRScheduler(opt, verbose=False, **kw)
        out["metrics"] = list(metrics)
    else:
        sched = {"cosine": CosineLRScheduler, "tanh": TanhLRScheduler, "step": StepLRScheduler}[kind](opt, **kw)
        if kind != "step":
            out["cycle_length"] = sched.get_cycle_length()
    out["lr"] = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (ReduceLROnPlateau.step's `epoch` argument is deprecated; the reference passes it)
        for t in range(count):
            if kind == "plateau":
                sched.step(t, metrics[t])
            else:
                sched.step(t)
            out["lr"].append(repr(float(opt.param_groups[0]["lr"])))
    return out


if __name__ == "__main__":
    assert mg.build_ref.reference_available(), "the reference checkout is required to regenerate fixtures"
    mg.build_ref.install_stubs()  # (puts the reference on sys.path)
    fixture = {name: run(*case) for name, case in CASES.items()}
    with open(os.path.join(HERE, "lr_schedules.json"), "w") as f:
        json.dump(fixture, f, indent=0)
    for k, v in fixture.items():
        print(k, len(v["lr"]), v.get("cycle_length"), len(set(v["lr"])), v["lr"][:3], v["lr"][-1])
