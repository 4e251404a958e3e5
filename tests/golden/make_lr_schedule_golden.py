"""tests/golden/make_lr_schedule_golden.py -- learning rates FROM THE REFERENCE ITSELF, written next to this file.

The reference's own `CosineLRScheduler` (scheduler/cosine_lr.py) is imported where it lies and stepped over a `torch.optim.SGD`
param group; what `step(t)` leaves in `param_groups[0]["lr"]` is recorded as the `repr` of the double, so the fixture round-trips
exactly.  Data only: settings, `t` and rates.

    lr_schedule_cosine.json   {case: {"settings": {...}, "lr": [repr(rate at t) for t = 0 ... last]}}

    python tests/golden/make_lr_schedule_golden.py
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402

CASES = {
    # the recipes' settings (cot_experiments/*/config.yaml), t = 0 ... 351
    "recipe": (dict(lr=0.25, t_initial=350, warmup_t=5, warmup_lr_init=1e-4, lr_min=1e-5, decay_rate=0.1, cycle_limit=1), 352),
    # a short one, t = 0 ... 13
    "short": (dict(lr=0.25, t_initial=12, warmup_t=3, warmup_lr_init=1e-4, lr_min=1e-5, decay_rate=0.1, cycle_limit=1), 14),
}


def rates(settings, count):
    from scheduler.cosine_lr import CosineLRScheduler  # the reference's
    kw = dict(settings)
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=kw.pop("lr"), momentum=0.9, nesterov=True)
    sched = CosineLRScheduler(opt, **kw)
    out = []
    for t in range(count):
        sched.step(t)
        out.append(repr(float(opt.param_groups[0]["lr"])))
    return out


if __name__ == "__main__":
    assert mg.build_ref.reference_available(), "the reference checkout is required to regenerate fixtures"
    mg.build_ref.install_stubs()  # (puts the reference on sys.path)
    fixture = {name: {"settings": s, "lr": rates(s, n)} for name, (s, n) in CASES.items()}
    with open(os.path.join(HERE, "lr_schedule_cosine.json"), "w") as f:
        json.dump(fixture, f, indent=0)
    print({k: (len(v["lr"]), v["lr"][0], v["lr"][-1]) for k, v in fixture.items()})
