"""cotnet_amd.lr_schedule's four schedules, their noise and create_scheduler against the rates that the reference's own schedulers
(scheduler/*.py) set on a torch.optim.SGD param group (tests/golden/lr_schedules.json, written by
tests/golden/make_lr_schedules_golden.py; the rates are stored as the `repr` of the doubles).  The schedules restate the reference in
its order of operations: the doubles are EQUAL, so every comparison here is of `repr` strings or `==`."""
import json
import os
import random
import warnings

import pytest
import torch

import cotnet_amd
from cotnet_amd import (CosineLRSchedule, CosineSchedule, PlateauLRSchedule, StepLRSchedule, TanhLRSchedule, Trainer,
                        create_scheduler)

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN_DIR, "lr_schedules.json")) as fh:
    GOLDEN = json.load(fh)
with open(os.path.join(GOLDEN_DIR, "lr_schedule_cosine.json")) as fh:
    GOLDEN_COSINE = json.load(fh)

KINDS = {"cosine": CosineLRSchedule, "tanh": TanhLRSchedule, "step": StepLRSchedule, "plateau": PlateauLRSchedule}
STATELESS = sorted(k for k, v in GOLDEN.items() if v["kind"] != "plateau")
PLATEAU = sorted(k for k, v in GOLDEN.items() if v["kind"] == "plateau")
RECIPE = dict(t_initial=350, lr_min=1e-5, decay_rate=0.1, warmup_t=5, warmup_lr_init=1e-4, cycle_limit=1)


class Stub:
    """an optimizer as a schedule sees it: records set_lr"""

    def __init__(self):
        self.seen = []

    def set_lr(self, lr):
        self.seen.append(lr)


def build(case):
    kw = dict(GOLDEN[case]["settings"])
    return KINDS[GOLDEN[case]["kind"]](kw.pop("lr"), **kw)


def test_the_fixture_covers_what_it_is_meant_to():
    def s(case):
        return GOLDEN[case]["settings"]
    assert len(STATELESS) == 14 and len(PLATEAU) == 4
    assert (s("cosine_restarts")["t_mul"], s("cosine_restarts")["cycle_limit"], s("cosine_restarts")["decay_rate"]) == (1, 0, 0.5)
    c = s("cosine_tmul2_limit3_prefix")
    assert (c["t_mul"], c["cycle_limit"], c["warmup_prefix"], c["decay_rate"]) == (2, 3, True, 0.5)
    assert len(GOLDEN["cosine_tmul2_limit3_prefix"]["lr"]) > c["warmup_t"] + GOLDEN["cosine_tmul2_limit3_prefix"]["cycle_length"]
    assert {k: s("cosine_recipe")[k] for k in RECIPE} == RECIPE and s("cosine_recipe")["lr"] == 0.25
    t = s("tanh_limit2_warmup")
    assert (t["t_mul"], t["cycle_limit"], t["decay_rate"]) == (1, 2, 0.5) and t["warmup_t"] > 0 and "warmup_prefix" not in t
    assert len(GOLDEN["tanh_limit2_warmup"]["lr"]) > GOLDEN["tanh_limit2_warmup"]["cycle_length"]
    assert s("tanh_tmul2")["t_mul"] == 2
    assert isinstance(s("step_int_warmup")["decay_t"], int) and s("step_int_warmup")["warmup_t"] > 0 and s("step_float")["decay_t"] == 2.5
    for kind in ("cosine", "tanh", "step"):
        assert isinstance(s(kind + "_noise_pair")["noise_range_t"], list) and isinstance(s(kind + "_noise_scalar")["noise_range_t"], int)
        plain = {"cosine": "cosine_restarts", "tanh": "tanh_limit2_warmup", "step": "step_int_warmup"}[kind]
        for form in ("_noise_pair", "_noise_scalar"):  # the noise moved some rates and left the others alone
            moved = [a != b for a, b in zip(GOLDEN[kind + form]["lr"], GOLDEN[plain]["lr"])]
            assert any(moved) and not all(moved)
    for case in PLATEAU:
        p = s(case)
        assert (p["patience_t"], p["cooldown_t"], p["warmup_t"]) == (2, 1, 3)
    assert s("plateau_max")["mode"] == "max" and s("plateau_min")["mode"] == "min"
    for case in ("plateau_max", "plateau_min"):  # reduced, step by step, until lr_min stops it (within the rule's eps)
        rates = [float(r) for r in GOLDEN[case]["lr"]]
        assert rates[-1] - s(case)["lr_min"] < 1e-8 and len(set(rates[4:])) == 4
    assert "noise_range_t" in s("plateau_max_noise")
    assert all(len(v["lr"]) <= 40 for v in GOLDEN.values())


@pytest.mark.parametrize("case", STATELESS)
def test_every_rate_equals_the_reference(case):
    fx, sched = GOLDEN[case], build(case)
    got = [repr(sched.value(t)) for t in range(len(fx["lr"]))]
    bad = [(t, g, r) for t, (g, r) in enumerate(zip(got, fx["lr"])) if g != r]
    assert not bad, bad[:5]
    assert all(type(sched.value(t)) is float for t in range(len(fx["lr"])))
    assert not sched.needs_metric


@pytest.mark.parametrize("case", [c for c in STATELESS if "cycle_length" in GOLDEN[c]])
def test_cycle_length_equals_the_reference(case):
    assert build(case).get_cycle_length() == GOLDEN[case]["cycle_length"]


@pytest.mark.parametrize("case", STATELESS)
def test_value_is_pure(case):
    sched, n = build(case), len(GOLDEN[case]["lr"])
    forward = [sched.value(t) for t in range(n)]
    before = dict(vars(sched))
    order = list(range(n))
    random.Random(3).shuffle(order)
    shuffled = {t: sched.value(t) for t in order}
    assert [shuffled[t] for t in range(n)] == forward == [sched.value(t) for t in range(n)]
    assert vars(sched) == before
    state = torch.get_rng_state()  # (the noise has its own generator: torch's global one is left alone)
    sched.value(n // 2)
    assert torch.equal(torch.get_rng_state(), state)


@pytest.mark.parametrize("case", STATELESS[:3])
def test_apply_hands_the_rate_to_the_optimizer(case):
    opt, sched = Stub(), build(case)
    got = [sched.apply(opt, t) for t in (0, 2, 7, 13)] + [sched.apply(opt, 9, 1.0)]  # (a metric is accepted and ignored)
    assert opt.seen == got == [sched.value(t) for t in (0, 2, 7, 13, 9)]


def test_cosine_with_the_recipes_settings_is_the_recipes_schedule():
    new, old = CosineLRSchedule(0.25, **RECIPE), CosineSchedule(0.25, 350, warmup_t=5, warmup_lr_init=1e-4, lr_min=1e-5)
    fx = GOLDEN_COSINE["recipe"]["lr"]
    assert len(fx) == 352
    for t in range(352):
        assert repr(new.value(t)) == repr(old.value(t)) == fx[t], t
    assert new.get_cycle_length() == 350


def test_noise_keywords():
    with pytest.raises(TypeError, match="noise_rnge_t"):
        StepLRSchedule(0.1, 4, noise_rnge_t=3)
    s = StepLRSchedule(0.1, 100, noise_range_t=[2, 5], noise_seed=None)  # None: the reference's 42
    assert [s.value(t) != 0.1 for t in range(7)] == [False, False, True, True, True, False, False]
    assert [s.value(t) for t in range(7)] == [StepLRSchedule(0.1, 100, noise_range_t=[2, 5], noise_std=9.).value(t) for t in range(7)]
    assert all(abs(s.value(t) / 0.1 - 1) < 0.67 for t in range(2, 5))
    tight = StepLRSchedule(0.1, 100, noise_range_t=0, noise_pct=0.05)
    assert all(0 < abs(tight.value(t) / 0.1 - 1) < 0.05 for t in range(40))


# ---- plateau

@pytest.mark.parametrize("case", PLATEAU)
def test_plateau_equals_the_reference_through_apply(case):
    fx, sched, opt = GOLDEN[case], build(case), Stub()
    assert sched.needs_metric
    got = [repr(sched.apply(opt, t, m)) for t, m in enumerate(fx["metrics"])]
    bad = [(t, g, r) for t, (g, r) in enumerate(zip(got, fx["lr"])) if g != r]
    assert not bad, bad[:5]
    assert [repr(v) for v in opt.seen] == fx["lr"] and all(type(v) is float for v in opt.seen)
    with pytest.raises(TypeError, match="no value"):
        sched.value(3)


@pytest.mark.parametrize("case", PLATEAU)
@pytest.mark.parametrize("at", [2, 7, 12, 19])
def test_plateau_state_dict_continues_the_sequence(case, at):
    fx, first, opt = GOLDEN[case], build(case), Stub()
    for t in range(at):
        first.apply(opt, t, fx["metrics"][t])
    state = first.state_dict()
    assert set(state) == {"best", "last_epoch", "num_bad_epochs", "cooldown_counter", "lr", "restore_lr"}
    state = json.loads(json.dumps(state))  # (plain data: it survives a file)
    second = build(case)
    second.load_state_dict(state)
    got = [repr(second.apply(opt, t, fx["metrics"][t])) for t in range(at, len(fx["lr"]))]
    assert got == fx["lr"][at:]
    with pytest.raises(KeyError, match="restore_lr"):
        build(case).load_state_dict({k: v for k, v in state.items() if k != "restore_lr"})


@pytest.mark.parametrize("case", PLATEAU)
def test_plateau_without_a_metric_past_the_warm_up_changes_nothing(case):
    fx, sched, opt = GOLDEN[case], build(case), Stub()
    for t in range(12):
        sched.apply(opt, t, fx["metrics"][t])
    before, seen = sched.state_dict(), list(opt.seen)
    assert sched.apply(opt, 12, None) == sched.apply(opt, 12) == before["lr"] == float(fx["lr"][11])
    assert sched.state_dict() == before and opt.seen == seen
    assert repr(sched.apply(opt, 12, fx["metrics"][12])) == fx["lr"][12]  # and the sequence goes on as if it had not been called
    # inside the warm-up the rate is the warm-up's, metric or not
    fresh = build(case)
    assert [repr(fresh.apply(opt, t)) for t in range(4)] == fx["lr"][:4]


def test_plateau_resume_call_takes_the_rate_the_optimizer_was_resumed_with():
    class Resumed(Stub):
        lr = 0.003
    sched, opt = PlateauLRSchedule(0.1, patience_t=0, warmup_t=2, mode="min"), Resumed()
    assert sched.apply(opt, 5) == 0.003 and opt.seen == []
    assert sched.apply(opt, 6, 1.0) == 0.003 and sched.apply(opt, 7, 1.0) == 0.003 * 0.1  # the rule acts on the current rate
    assert opt.seen == [0.003, 0.003 * 0.1]


def test_plateau_without_a_warm_up_starts_at_the_base_rate():
    sched, opt = PlateauLRSchedule(0.1, patience_t=0, warmup_lr_init=1e-4), Stub()
    assert sched.apply(opt, 0) == 0.1 and sched.lr == 0.1 and opt.seen == []
    assert sched.apply(opt, 1, 5.0) == 0.1 and sched.apply(opt, 2, 5.0) == 0.1 * 0.1


@pytest.mark.parametrize("mode", ["min", "max"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_plateau_rule_equals_torchs_class(mode, seed):
    """random walks of a metric, no warm-up and no noise: the restated rule against torch's ReduceLROnPlateau on an SGD group"""
    rng = random.Random(seed)
    kw = dict(factor=0.5, patience=rng.choice([0, 1, 3]), threshold=rng.choice([1e-4, 0.05]), cooldown=rng.choice([0, 2]), min_lr=2e-3)
    sgd = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1)
    ref = torch.optim.lr_scheduler.ReduceLROnPlateau(sgd, mode=mode, **kw)
    sched = PlateauLRSchedule(0.1, decay_rate=kw["factor"], patience_t=kw["patience"], threshold=kw["threshold"], cooldown_t=kw["cooldown"],
                              lr_min=kw["min_lr"], mode=mode)
    opt, metric = Stub(), 10.0
    for t in range(1, 60):
        metric += rng.choice([-1.0, -0.01, 0.0, 0.0, 0.01, 1.0])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # (the `epoch` argument is deprecated; the reference passes it)
            ref.step(metric, t)
        assert repr(sched.apply(opt, t, metric)) == repr(float(sgd.param_groups[0]["lr"])), t
        assert (sched.best, sched.last_epoch, sched.num_bad_epochs, sched.cooldown_counter) == \
            (ref.best, ref.last_epoch, ref.num_bad_epochs, ref.cooldown_counter), t
    assert sched.lr < 0.1


def test_plateau_refuses_what_it_cannot_be():
    with pytest.raises(ValueError, match="'min' or 'max'"):
        PlateauLRSchedule(0.1, mode="top1")
    with pytest.raises(ValueError, match="< 1.0"):
        PlateauLRSchedule(0.1, decay_rate=1.0)


# ---- the factory

def test_factory_cosine_default_is_the_recipes_schedule():
    sched, num_epochs = create_scheduler("cosine", epochs=350, lr=0.25, warmup_epochs=5)
    assert type(sched) is CosineLRSchedule and num_epochs == 350
    fx = GOLDEN_COSINE["recipe"]["lr"]
    assert [repr(sched.value(t)) for t in range(352)] == fx
    assert cotnet_amd.create_scheduler is create_scheduler


def test_factory_names_and_what_each_gets():
    kw = dict(epochs=40, lr=0.2, min_lr=1e-3, warmup_lr=1e-2, warmup_epochs=4, decay_epochs=2.4, decay_rate=0.3, patience_epochs=7)
    cos, n = create_scheduler("cosine", **kw)
    assert type(cos) is CosineLRSchedule and n == 40
    assert (cos.base_lr, cos.t_initial, cos.t_mul, cos.lr_min, cos.decay_rate, cos.warmup_t, cos.warmup_lr_init, cos.warmup_prefix,
            cos.cycle_limit) == (0.2, 40, 1.0, 1e-3, 0.3, 4, 1e-2, False, 1)
    tanh, n = create_scheduler("tanh", **kw)
    assert type(tanh) is TanhLRSchedule and n == 40
    assert (tanh.base_lr, tanh.t_initial, tanh.lr_min, tanh.decay_rate, tanh.warmup_t, tanh.warmup_lr_init, tanh.cycle_limit, tanh.lb,
            tanh.ub) == (0.2, 40, 1e-3, 1., 4, 1e-2, 1, -6., 4.)  # (the reference's factory hands decay_rate to the cosine only)
    step, n = create_scheduler("step", cooldown_epochs=10, **kw)
    assert type(step) is StepLRSchedule and n == 40  # no cool-down is added for step and plateau
    assert (step.base_lr, step.decay_t, step.decay_rate, step.warmup_t, step.warmup_lr_init) == (0.2, 2.4, 0.3, 4, 1e-2)
    plat, n = create_scheduler("plateau", cooldown_epochs=10, **kw)
    assert type(plat) is PlateauLRSchedule and n == 40
    assert (plat.base_lr, plat.decay_rate, plat.patience_t, plat.lr_min, plat.mode, plat.warmup_t, plat.warmup_lr_init, plat.cooldown_t,
            plat.threshold) == (0.2, 0.3, 7, 1e-3, "max", 4, 1e-2, 0, 1e-4)
    assert [s.needs_metric for s in (cos, tanh, step, plat)] == [False, False, False, True]
    for s in (cos, tanh, step, plat):
        assert s.noise_range_t is None and s.noise_seed == 42


@pytest.mark.parametrize("sched", ["cosine", "tanh"])
def test_factory_num_epochs_covers_the_cycles_and_the_cool_down(sched):
    s, n = create_scheduler(sched, epochs=30, lr=0.1, lr_cycle_mul=2, lr_cycle_limit=3, cooldown_epochs=10)
    assert s.get_cycle_length() == 30 + 60 + 120 and n == 220
    assert (s.t_mul, s.cycle_limit) == (2, 3)
    s, n = create_scheduler(sched, epochs=30, lr=0.1, lr_cycle_limit=3, cooldown_epochs=10)
    assert n == 100


def test_factory_noise_range_forms():
    def noise(lr_noise, **kw):
        return create_scheduler("step", epochs=200, lr=0.1, lr_noise=lr_noise, **kw)[0]
    assert noise(None).noise_range_t is None and noise([]).noise_range_t is None and noise(()).noise_range_t is None
    assert noise([0.4, 0.9]).noise_range_t == [0.4 * 200, 0.9 * 200]
    assert noise([0.4]).noise_range_t == 0.4 * 200 and noise(0.4).noise_range_t == 0.4 * 200
    s = noise([0.4, 0.9], lr_noise_pct=0.3, lr_noise_std=0.5, seed=5)
    assert (s.noise_pct, s.noise_std, s.noise_seed) == (0.3, 0.5, 5)
    plain = create_scheduler("step", epochs=200, lr=0.1)[0]
    assert [s.value(t) != plain.value(t) for t in (0, 79, 80, 179, 180, 199)] == [False, False, True, True, False, False]
    for name in ("cosine", "tanh", "plateau"):
        assert create_scheduler(name, epochs=200, lr=0.1, lr_noise=[0.4, 0.9])[0].noise_range_t == [80.0, 180.0]


def test_factory_mode_follows_the_eval_metric():
    assert create_scheduler("plateau", epochs=10, lr=0.1)[0].mode == "max"
    assert create_scheduler("plateau", epochs=10, lr=0.1, eval_metric="top5")[0].mode == "max"
    assert create_scheduler("plateau", epochs=10, lr=0.1, eval_metric="loss")[0].mode == "min"
    assert create_scheduler("plateau", epochs=10, lr=0.1, eval_metric="eval_loss")[0].mode == "min"


def test_factory_takes_the_recipes_float_seed():
    s, _ = create_scheduler("cosine", epochs=20, lr=0.1, lr_noise=[0.5], seed=1.0)  # `seed: 1.0` in every shipped config
    assert s.noise_seed == 1 and type(s.noise_seed) is int
    assert s.value(15) == create_scheduler("cosine", epochs=20, lr=0.1, lr_noise=[0.5], seed=1)[0].value(15) != \
        create_scheduler("cosine", epochs=20, lr=0.1)[0].value(15)


def test_factory_refuses_an_unknown_name():
    with pytest.raises(ValueError, match="cosine, tanh, step, plateau"):
        create_scheduler("poly", epochs=10, lr=0.1)


# ---- Trainer

class SetLrSGD(torch.optim.SGD):
    """torch's SGD with the flat optimizers' `lr` / `set_lr`"""

    def __init__(self, params, lr):
        super().__init__(params, lr=lr)
        self.lr, self.seen = lr, []

    def set_lr(self, lr):
        self.lr = lr
        self.seen.append(lr)
        for g in self.param_groups:
            g["lr"] = lr


class Scripted:
    def __init__(self, metrics):
        self.metrics = metrics

    def __call__(self, epoch, model):
        return self.metrics[epoch], 0.0


def _pieces():
    torch.manual_seed(0)
    model = torch.nn.Linear(6, 3)
    batches = [(torch.randn(4, 6), torch.randint(0, 3, (4,))) for _ in range(2)]
    return model, SetLrSGD(model.parameters(), 0.1), torch.nn.CrossEntropyLoss(), batches


def test_trainer_refuses_a_plateau_schedule_it_cannot_feed():
    model, opt, loss_fn, batches = _pieces()
    plateau = PlateauLRSchedule(0.1)
    with pytest.raises(ValueError, match="no evaler"):
        Trainer(model, opt, loss_fn, batches, num_epochs=2, schedule=plateau)
    with pytest.raises(ValueError, match="none per update"):
        Trainer(model, opt, loss_fn, batches, num_epochs=2, schedule=plateau, evaler=Scripted([1., 1.]), schedule_unit="update")
    Trainer(model, opt, loss_fn, batches, num_epochs=2, schedule=plateau, evaler=Scripted([1., 1.]))
    for unit in ("epoch", "update"):  # every other schedule needs neither
        Trainer(model, opt, loss_fn, batches, num_epochs=2, schedule=StepLRSchedule(0.1, 1), schedule_unit=unit)
        Trainer(model, opt, loss_fn, batches, num_epochs=2, schedule=CosineSchedule(0.1, 2), schedule_unit=unit)


def test_trainer_steps_a_plateau_schedule_with_the_epochs_metric():
    fx = GOLDEN["plateau_max"]
    model, opt, loss_fn, batches = _pieces()
    epochs = 12
    trainer = Trainer(model, opt, loss_fn, batches, num_epochs=epochs, schedule=build("plateau_max"), evaler=Scripted(fx["metrics"][1:]))
    history = trainer.fit()
    assert [repr(h["lr"]) for h in history] == fx["lr"][:epochs]  # epoch e trains at the rate of the reference's step(e, metrics[e])
    assert [repr(v) for v in opt.seen] == fx["lr"][:epochs + 1]
    assert float(fx["lr"][epochs]) < float(fx["lr"][4])  # (the run covers a reduction)


def test_trainer_keeps_the_two_argument_call_for_every_other_schedule():
    class TwoArguments(CosineSchedule):
        def apply(self, opt, t):  # (a third argument would be a TypeError)
            return super().apply(opt, t)
    model, opt, loss_fn, batches = _pieces()
    sched = TwoArguments(0.1, 3)
    Trainer(model, opt, loss_fn, batches, num_epochs=3, schedule=sched, evaler=Scripted([1., 2., 3.])).fit()
    assert opt.seen == [sched.value(t) for t in range(4)]
