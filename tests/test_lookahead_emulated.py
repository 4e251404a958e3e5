"""Lookahead on the flat optimizers (cot_lookahead_tick, cot_lookahead_step, FlatSGD / FlatAdamW(lookahead_k=...)) -- on the host emulator.

The cases are tests/lookahead_cases.py's, the same list the device runs (tests/test_lookahead_gpu.py).  Left to the device only: the
size at which a lane makes a second trip of the grid-stride loop (2 M elements through the emulator take more than a few seconds) and
everything that replays a HIP graph."""
import pytest
import torch

from cotnet_amd import _lib
from tests import adamw_cases as adamw
from tests import lookahead_cases as cases
from tests.test_grad_clip_emulated import _EMUL, _counted, _emulated  # (ONE handle: _emulated puts that module's behind _lib.lib())

pytestmark = pytest.mark.skipif(_EMUL is None, reason="host emulation build unavailable")
CPU = torch.device("cpu")
MIXED, MIXED_IDS = [False, True], ["fp32", "mixed-bf16"]


def test_the_block_is_eight_words_and_the_entry_points_are_statuses():
    import os
    import re
    from tests.emul import build_emul
    hdr = open(os.path.join(build_emul.ROOT, "include", "cotnet_amd.h")).read()
    body = re.search(r"typedef struct cot_lookahead_state \{(.*?)\} cot_lookahead_state;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int32_t|float)\s+(\w+)(?:\[(\d+)\])?;", body)
    assert [f[1] for f in fields] == ["step", "action", "born", "syncs", "refused", "reserved"] and {f[0] for f in fields} == {"int32_t"}
    assert sum(int(f[2] or 1) for f in fields) == 8
    assert "cot_lookahead_tick" not in _lib.NOT_STATUS and "cot_lookahead_step" not in _lib.NOT_STATUS


@pytest.mark.parametrize("pdt", cases.FORMS, ids=cases.FORM_IDS)
@pytest.mark.parametrize("alpha", [0.5, 0.3])
@pytest.mark.parametrize("n", cases.SIZES)
def test_interpolation_against_the_formula(pdt, alpha, n):
    cases.check_interpolation(_EMUL, CPU, None, pdt, n, alpha)


@pytest.mark.parametrize("pdt", cases.FORMS, ids=cases.FORM_IDS)
def test_action_0_writes_nothing_and_action_1_only_adopts(pdt):
    cases.check_actions(_EMUL, CPU, None, pdt)


def test_tick():
    cases.check_tick(_EMUL, CPU, None)


def test_tick_behind_a_skip():
    cases.check_tick_skip(_EMUL, CPU, None)


@pytest.mark.parametrize("alpha", [0.5, 0.8])
@pytest.mark.parametrize("t", [3, 6, 8])
def test_the_reference_fixture(alpha, t):
    cases.check_fixture_sync(_EMUL, CPU, None, alpha, t)


def test_refusals_leave_everything_alone():
    cases.check_refusals(_EMUL, CPU, None)


@pytest.mark.parametrize("pdt", cases.FORMS, ids=cases.FORM_IDS)
def test_two_calls_give_equal_bits(pdt):
    cases.check_repeatable(_EMUL, CPU, None, pdt)


# ---- the optimizers

@pytest.mark.parametrize("mixed", MIXED, ids=MIXED_IDS)
@pytest.mark.parametrize("rule", cases.RULES)
def test_twin_protocol(mixed, rule, monkeypatch):
    _emulated(monkeypatch)
    cases.check_twin_protocol(CPU, mixed, rule)


@pytest.mark.parametrize("mixed", MIXED, ids=MIXED_IDS)
@pytest.mark.parametrize("rule", cases.RULES)
def test_the_average_follows_the_weights_after_the_sync(mixed, rule, monkeypatch):
    _emulated(monkeypatch)
    cases.check_ema_follows_the_sync(CPU, mixed, rule)


@pytest.mark.parametrize("mixed", MIXED, ids=MIXED_IDS)
@pytest.mark.parametrize("rule", cases.RULES)
def test_a_skipped_step_is_not_counted(mixed, rule, monkeypatch):
    _emulated(monkeypatch)
    cases.check_skipped_step(CPU, mixed, rule)


@pytest.mark.parametrize("mixed", MIXED, ids=MIXED_IDS)
@pytest.mark.parametrize("rule", cases.RULES)
def test_sync_lookahead(mixed, rule, monkeypatch):
    _emulated(monkeypatch)
    cases.check_sync_lookahead(CPU, mixed, rule)


@pytest.mark.parametrize("rule", cases.RULES)
def test_nothing_of_lookahead_inside_a_capture(rule, monkeypatch):
    _emulated(monkeypatch)
    model, opt = cases.build(CPU, True, rule, lookahead_k=2)
    adamw.train_step(model, opt, adamw.batches(CPU, True, 1)[0])
    monkeypatch.setattr(_lib, "capturing", lambda: True)
    for call in (opt.sync_lookahead, opt.lookahead_stats, opt.state_dict):
        with pytest.raises(RuntimeError, match="inside a HIP-graph capture"):
            call()
    adamw.train_step(model, opt, adamw.batches(CPU, True, 1)[0])  # (a step may be captured: it records k and alpha)
    monkeypatch.setattr(_lib, "capturing", lambda: False)
    assert opt._captured_lookahead == (2, 0.5) and opt.lookahead_stats()["step"] == 2
    sd = opt.state_dict()
    with pytest.raises(ValueError, match="captured into a HIP graph with \\(lookahead_k, lookahead_alpha\\)"):
        opt.load_state_dict(dict(sd, param_groups=[dict(g, lookahead_k=3) for g in sd["param_groups"]]))
    opt.load_state_dict(sd)


@pytest.mark.parametrize("mixed", MIXED, ids=MIXED_IDS)
@pytest.mark.parametrize("rule", cases.RULES)
@pytest.mark.parametrize("at", [2, 4], ids=["unborn", "born"])
def test_checkpoint_resumes_bit_equal(mixed, rule, at, monkeypatch):
    _emulated(monkeypatch)
    cases.check_checkpoint(CPU, mixed, rule, at)


@pytest.mark.parametrize("rule", cases.RULES)
@pytest.mark.parametrize("at", [2, 4], ids=["unborn", "born"])
def test_checkpoint_saver_round_trip(rule, at, monkeypatch, tmp_path):
    _emulated(monkeypatch)
    cases.check_checkpoint(CPU, True, rule, at, tmp_path=tmp_path, skip_nonfinite=True)


@pytest.mark.parametrize("rule", cases.RULES)
def test_load_state_dict_refusals(rule, monkeypatch):
    _emulated(monkeypatch)
    cases.check_load_refusals(CPU, True, rule)


# ---- launches

SGD_NAMES = ("cot_sgd_step", "cot_sgd_step_lr", "cot_sgd_step_clip")
NAMES = ("cot_agc_clip", "cot_grad_sumsq", "cot_grad_clip_finish", "cot_adam_tick", "cot_adamw_step", "cot_ema_step", "cot_lookahead_tick",
         "cot_lookahead_step") + SGD_NAMES


def _launches(monkeypatch, rule, **kw):
    """(optimizer, [(entry point, arguments)] of one step)"""
    order = []
    model, opt = cases.build(CPU, True, rule, **kw)
    with monkeypatch.context() as m:
        for name in NAMES:
            raw = getattr(_EMUL, name)
            m.setattr(_EMUL, name, lambda *a, _raw=raw, _name=name: (order.append((_name, a)), _raw(*a))[1])
        adamw.train_step(model, opt, adamw.batches(CPU, True, 1)[0])
    return opt, order


@pytest.mark.parametrize("rule", cases.RULES)
@pytest.mark.parametrize("kw", [dict(), dict(skip_nonfinite=True, ema_decay=0.9, device_lr=True)], ids=["plain", "guard-ema-device-lr"])
def test_lookahead_adds_one_tick_and_one_launch_per_bucket(rule, kw, monkeypatch):
    """off: the launch list is the one of before; on: the same list plus ONE tick behind the clip launches and the rule's own tick, and
    one cot_lookahead_step per bucket between the bucket's update and its EMA launch"""
    _emulated(monkeypatch)
    off, before = _launches(monkeypatch, rule, **kw)
    opt, after = _launches(monkeypatch, rule, lookahead_k=3, **kw)
    nb = len(opt.reducer.buckets)
    assert off.lookahead_state is None and all("slow" not in st for st in off.state)
    assert not any(n.startswith("cot_lookahead") for n, _ in before)
    assert [n for n, _ in after if not n.startswith("cot_lookahead")] == [n for n, _ in before]
    assert len(after) == len(before) + 1 + nb
    update = "cot_adamw_step" if rule == "adamw" else ("cot_sgd_step_clip" if kw else "cot_sgd_step")
    head = ["cot_grad_sumsq"] * nb + ["cot_grad_clip_finish"] if kw else []
    head += ["cot_adam_tick"] if rule == "adamw" else []
    per_bucket = [update, "cot_lookahead_step"] + (["cot_ema_step"] if kw else [])
    assert [n for n, _ in after] == head + ["cot_lookahead_tick"] + per_bucket * nb
    tick = next(a for n, a in after if n == "cot_lookahead_tick")
    assert tick[:4] == (opt.lookahead_state.data_ptr(), opt.clip_state.data_ptr() if kw else None, 3, 0)
    for (_, a), b, st in zip([o for o in after if o[0] == "cot_lookahead_step"], opt.reducer.buckets, opt.state):
        assert a[:7] == (b.pflat.data_ptr(), st["master"].data_ptr() if st["master"] is not None else None, st["slow"].data_ptr(),
                         b.pflat.numel(), 0.5, opt.lookahead_state.data_ptr(), _lib.dtype_code(b.pflat.dtype))
        assert st["slow"].dtype == torch.float32 and st["slow"].numel() == b.pflat.numel()


def test_sync_lookahead_launches_a_forced_tick_and_the_bucket_kernels_only(monkeypatch):
    _emulated(monkeypatch)
    model, opt = cases.build(CPU, True, "sgd", lookahead_k=3, skip_nonfinite=True, ema_decay=0.9)
    adamw.train_step(model, opt, adamw.batches(CPU, True, 1)[0])
    calls = {name: _counted(monkeypatch, name) for name in NAMES}
    opt.sync_lookahead()
    assert {k: len(v) for k, v in calls.items() if v} == {"cot_lookahead_tick": 1, "cot_lookahead_step": len(opt.reducer.buckets)}
    assert calls["cot_lookahead_tick"][0][:4] == (opt.lookahead_state.data_ptr(), None, 3, 1)
