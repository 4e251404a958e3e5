"""cotnet_amd.trainer over the real pieces on the host emulator: tests/trainer_cases.py's cases, the list the device runs
(tests/test_trainer_gpu.py).  There is no graph here -- `graph=True` finds no GPU and says so -- so what this file pins is the loop:
Trainer against the hand-written loop bit for bit, the resume, and the meter's figures."""
import pytest

from tests import trainer_cases as cases
from tests.test_grad_clip_emulated import _EMUL, _emulated  # (ONE handle: _emulated puts that module's behind _lib.lib())

pytestmark = pytest.mark.skipif(_EMUL is None, reason="host emulation build unavailable")
CPU = "cpu"


@pytest.mark.parametrize("kind,epochs", [("sgd", 2), ("adamw", 1)])
def test_trainer_equals_the_hand_written_loop(kind, epochs, monkeypatch):
    _emulated(monkeypatch)
    cases.check_trainer_equals_the_hand_written_loop(CPU, kind, epochs, on_gpu=False)


def test_meter_equals_item_per_step(monkeypatch):
    _emulated(monkeypatch)
    cases.check_meter_against_item_per_step(CPU, "sgd", 2)


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_resume_is_bit_equal_to_the_uninterrupted_run(kind, monkeypatch, tmp_path):
    _emulated(monkeypatch)
    cases.check_resume(CPU, kind, tmp_path, on_gpu=False)

