"""cotnet_amd.lr_schedule.CosineSchedule against the rates the reference's own CosineLRScheduler (scheduler/cosine_lr.py:68-95) set on a
torch.optim.SGD param group (tests/golden/lr_schedule_cosine.json, written by tests/golden/make_lr_schedule_golden.py; the rates are
stored as the `repr` of the doubles).  The schedule is a restatement in the reference's order of operations: the doubles are EQUAL."""
import json
import os

import pytest

from cotnet_amd.lr_schedule import CosineSchedule

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lr_schedule_cosine.json")) as fh:
    GOLDEN = json.load(fh)


def _schedule(settings):
    assert settings["cycle_limit"] == 1  # what the restatement covers: one cycle, no restarts
    return CosineSchedule(settings["lr"], settings["t_initial"], warmup_t=settings["warmup_t"],
                          warmup_lr_init=settings["warmup_lr_init"], lr_min=settings["lr_min"])


@pytest.mark.parametrize("case,count", [("recipe", 352), ("short", 14)])
def test_every_rate_equals_the_reference(case, count):
    fx = GOLDEN[case]
    assert len(fx["lr"]) == count
    sched = _schedule(fx["settings"])
    bad = [(t, sched.value(t), r) for t, r in enumerate(fx["lr"]) if sched.value(t) != float(r)]
    assert not bad, bad[:5]
    assert all(type(sched.value(t)) is float for t in range(count))


def test_recipe_settings_are_the_recipes():
    s = GOLDEN["recipe"]["settings"]
    assert (s["lr"], s["t_initial"], s["warmup_t"], s["warmup_lr_init"], s["lr_min"]) == (0.25, 350, 5, 1e-4, 1e-5)
    s = GOLDEN["short"]["settings"]
    assert (s["t_initial"], s["warmup_t"]) == (12, 3)


@pytest.mark.parametrize("case", ["recipe", "short"])
def test_rises_over_the_warm_up_falls_after_it_and_ends_at_the_floor(case):
    s = GOLDEN[case]["settings"]
    sched = _schedule(s)
    w, T = s["warmup_t"], s["t_initial"]
    v = [sched.value(t) for t in range(T + 10)]
    assert v[0] == s["warmup_lr_init"]
    assert all(a < b for a, b in zip(v[:w], v[1:w + 1]))    # rising, up to the first step of the cosine
    assert all(a > b for a, b in zip(v[w:T], v[w + 1:T + 1]))  # falling from there to the floor
    assert max(v) == v[w] <= s["lr"]
    assert all(x == s["lr_min"] for x in v[T:]) and sched.value(10 * T) == s["lr_min"]


def test_no_warm_up_starts_at_the_base_rate():
    sched = CosineSchedule(0.1, 10)
    assert sched.value(0) == 0.1 and sched.value(10) == 0.0 and sched.value(5) == pytest.approx(0.05, rel=1e-12)


def test_apply_hands_the_rate_to_the_optimizer():
    class Stub:
        def __init__(self):
            self.seen = []

        def set_lr(self, lr):
            self.seen.append(lr)
    opt, sched = Stub(), _schedule(GOLDEN["short"]["settings"])
    got = [sched.apply(opt, t) for t in (0, 2, 7, 13)]
    assert opt.seen == got == [sched.value(t) for t in (0, 2, 7, 13)]
