"""cotnet_amd.lr_schedule's schedules through cotnet_amd.trainer on the host emulator: tests/lr_schedules_cases.py's cases, the list the
device runs (tests/test_lr_schedules_gpu.py).  There is no graph here -- `graph=True` finds no GPU and steps eagerly -- so what this
file pins is the loop's order: where `apply` is called, with which `t` and which metric, and the resume."""
import pytest

from tests import lr_schedules_cases as cases
from tests.test_grad_clip_emulated import _EMUL, _emulated  # (ONE handle: _emulated puts that module's behind _lib.lib())

pytestmark = pytest.mark.skipif(_EMUL is None, reason="host emulation build unavailable")
CPU = "cpu"


def test_step_schedule_with_warm_up_and_noise_per_update(monkeypatch):
    _emulated(monkeypatch)
    cases.check_step_per_update(CPU, on_gpu=False)


def test_cosine_restart_per_epoch(monkeypatch):
    _emulated(monkeypatch)
    cases.check_cosine_restart_per_epoch(CPU, on_gpu=False)


def test_plateau_drops_where_the_fixture_says(monkeypatch):
    _emulated(monkeypatch)
    cases.check_plateau(CPU, on_gpu=False)


def test_resumed_run_with_a_noisy_step_schedule_is_bit_equal(monkeypatch, tmp_path):
    _emulated(monkeypatch)
    cases.check_resume(CPU, tmp_path, on_gpu=False)
