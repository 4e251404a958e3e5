"""Fused Adam / AdamW (cot_adam_tick, cot_adamw_step, FlatAdamW, FlatAdam) -- on the host emulator.

The kernel cases are tests/adamw_cases.py's, the same list the device runs (tests/test_adamw_gpu.py).  Left to the device only: the size
at which a lane makes a second trip of the grid-stride loop (2 M elements through the emulator take more than a few seconds) and
everything that replays a HIP graph.  The emulator's pow is the host's own, so the tick's corrections are compared with no allowance."""
import pytest
import torch

from cotnet_amd import _lib
from tests import adamw_cases as cases
from tests import sgd_lr_cases as sgd
from tests.test_grad_clip_emulated import _EMUL, _counted, _emulated  # (ONE handle: _emulated puts that module's behind _lib.lib())

pytestmark = pytest.mark.skipif(_EMUL is None, reason="host emulation build unavailable")
CPU = torch.device("cpu")
FORMS, FORM_IDS = [False, True], ["fp32", "mixed-bf16"]


def test_the_block_is_eight_words_and_the_entry_points_are_statuses():
    import os
    import re
    from tests.emul import build_emul
    hdr = open(os.path.join(build_emul.ROOT, "include", "cotnet_amd.h")).read()
    body = re.search(r"typedef struct cot_adam_state \{(.*?)\} cot_adam_state;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int32_t|float)\s+(\w+)(?:\[(\d+)\])?;", body)
    assert [f[1] for f in fields] == ["step", "bc1", "sqrt_bc2", "refused", "reserved"]
    assert sum(int(f[2] or 1) for f in fields) == 8
    assert "cot_adam_tick" not in _lib.NOT_STATUS and "cot_adamw_step" not in _lib.NOT_STATUS


@pytest.mark.parametrize("pdt,gdt", sgd.DTYPE_PAIRS, ids=sgd.PAIR_IDS)
@pytest.mark.parametrize("decoupled", [0, 1])
@pytest.mark.parametrize("n", cases.SIZES)
def test_one_step_against_the_formula(pdt, gdt, decoupled, n):
    cases.check_step(_EMUL, CPU, None, pdt, gdt, decoupled, n)


@pytest.mark.parametrize("t", [1, 2, 3, 1000])
def test_the_reference_fixture(t):
    cases.check_fixture_step(_EMUL, CPU, None, t)


def test_l2_form_against_torch_adam():
    cases.check_l2_against_torch_adam(_EMUL, CPU, None)


def test_tick():
    cases.check_tick(_EMUL, CPU, None, exact=True)


def test_tick_behind_a_skip():
    cases.check_tick_skip(_EMUL, CPU, None)


@pytest.mark.parametrize("pdt,gdt", sgd.DTYPE_PAIRS, ids=sgd.PAIR_IDS)
def test_zero_gradient(pdt, gdt):
    cases.check_zero_gradient(_EMUL, CPU, None, pdt, gdt)


@pytest.mark.parametrize("pdt,gdt", sgd.DTYPE_PAIRS, ids=sgd.PAIR_IDS)
def test_rate_by_value_and_from_memory_give_equal_bits(pdt, gdt):
    cases.check_rate_sources(_EMUL, CPU, None, pdt, gdt)


@pytest.mark.parametrize("pdt,gdt", sgd.DTYPE_PAIRS, ids=sgd.PAIR_IDS)
def test_clip_block(pdt, gdt):
    cases.check_clip_block(_EMUL, CPU, None, pdt, gdt)


@pytest.mark.parametrize("pdt,gdt", sgd.DTYPE_PAIRS, ids=sgd.PAIR_IDS)
def test_two_calls_give_equal_bits(pdt, gdt):
    cases.check_repeatable(_EMUL, CPU, None, pdt, gdt)


def test_refusals_leave_everything_alone():
    cases.check_refusals(_EMUL, CPU, None)


# ---- FlatAdamW

@pytest.mark.parametrize("mixed", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("decoupled", [True, False], ids=["adamw", "adam"])
def test_flat_optimizer_follows_torch(mixed, decoupled, monkeypatch):
    _emulated(monkeypatch)
    cases.check_flat_against_torch(CPU, mixed, decoupled)


@pytest.mark.parametrize("mixed", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("kw", [dict(), dict(device_lr=True, clip_grad=0.05)], ids=["plain", "device-lr-clip"])
def test_checkpoint_resumes_bit_equal(mixed, kw, monkeypatch):
    _emulated(monkeypatch)
    cases.check_checkpoint(CPU, mixed, **kw)


@pytest.mark.parametrize("mixed", FORMS, ids=FORM_IDS)
def test_state_dict_goes_to_torch_adamw_and_back(mixed, monkeypatch):
    _emulated(monkeypatch)
    cases.check_torch_interop(CPU, mixed)


def test_checkpoint_saver_round_trip(monkeypatch, tmp_path):
    _emulated(monkeypatch)
    cases.check_saver_round_trip(CPU, True, tmp_path)


@pytest.mark.parametrize("mixed", FORMS, ids=FORM_IDS)
def test_a_non_finite_step_is_skipped_and_not_counted(mixed, monkeypatch):
    _emulated(monkeypatch)
    cases.check_skipped_step(CPU, mixed)


def test_launch_order(monkeypatch):
    """step(): AGC per bucket, the sums of squares per bucket, the finish, ONE tick, then per bucket the step and its EMA launch"""
    _emulated(monkeypatch)
    model, opt = cases.build(CPU, True, agc=1e-2, skip_nonfinite=True, ema_decay=0.9, device_lr=True)
    nb = len(opt.reducer.buckets)
    names = ("cot_agc_clip", "cot_grad_sumsq", "cot_grad_clip_finish", "cot_adam_tick", "cot_adamw_step", "cot_ema_step", "cot_sgd_step",
             "cot_sgd_step_lr", "cot_sgd_step_clip")
    order = []
    for name in names:
        raw = getattr(_EMUL, name)
        monkeypatch.setattr(_EMUL, name, lambda *a, _raw=raw, _name=name: (order.append((_name, a)), _raw(*a))[1])
    cases.train_step(model, opt, cases.batches(CPU, True, 1)[0])
    assert [n for n, _ in order] == ["cot_agc_clip"] * nb + ["cot_grad_sumsq"] * nb + ["cot_grad_clip_finish", "cot_adam_tick"] + \
        ["cot_adamw_step", "cot_ema_step"] * nb
    tick = order[2 * nb + 1][1]
    assert tick[0] == opt.adam_state.data_ptr() and tick[1] == opt.clip_state.data_ptr() and tick[2:4] == opt.betas
    for (_, a), b, st in zip([o for o in order if o[0] == "cot_adamw_step"], opt.reducer.buckets, opt.state):
        assert a[:5] == (b.pflat.data_ptr(), st["master"].data_ptr() if st["master"] is not None else None, st["exp_avg"].data_ptr(),
                         st["exp_avg_sq"].data_ptr(), opt.reducer.reduced(b).data_ptr())
        assert a[7:10] == (opt.lr_dev.data_ptr(), opt.adam_state.data_ptr(), opt.clip_state.data_ptr())
        assert a[13] == (0.05 if b.key == "decay" else 0.0) and a[15] == 1


def test_plain_optimizer_allocates_no_blocks_it_does_not_need(monkeypatch):
    _emulated(monkeypatch)
    model, opt = cases.build(CPU, False)
    assert opt.clip_state is None and opt.lr_dev is None and opt._agc_units is None
    assert opt.adam_state.dtype == torch.int32 and opt.adam_state.tolist() == [0] * 8
    assert all(set(st) == {"master", "exp_avg", "exp_avg_sq"} for st in opt.state)
    calls = _counted(monkeypatch, "cot_adamw_step")
    cases.train_step(model, opt, cases.batches(CPU, False, 1)[0])
    assert len(calls) == len(opt.reducer.buckets) and all(a[7] is None and a[9] is None for a in calls)


def test_set_lr_rules_are_flat_sgds(monkeypatch):
    _emulated(monkeypatch)
    model, opt = cases.build(CPU, True)
    monkeypatch.setattr(_lib, "capturing", lambda: True)
    cases.train_step(model, opt, cases.batches(CPU, True, 1)[0])
    for read in (opt.adam_stats, opt.state_dict, lambda: opt.load_state_dict({})):
        with pytest.raises(RuntimeError, match="FlatAdamW.*capture"):
            read()
    monkeypatch.setattr(_lib, "capturing", lambda: False)
    with pytest.raises(RuntimeError, match="FlatAdamW.set_lr.*captured"):
        opt.set_lr(opt.lr / 10)
    opt.set_lr(opt.lr)
