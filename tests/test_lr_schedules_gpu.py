"""cotnet_amd.lr_schedule's schedules driving the replayed step on the device: tests/lr_schedules_cases.py's cases, which
tests/test_lr_schedules_emulated.py runs without a graph.  The rate reaches the captured step kernels through `opt.lr_dev` only, one
fill between replays: a hand-written loop, `Trainer(graph=False)` and `Trainer(graph=True)` end BIT FOR BIT in the same weights,
masters, momentum and EMA."""
import pytest

from tests import lr_schedules_cases as cases

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_step_schedule_with_warm_up_and_noise_per_update():
    cases.check_step_per_update(DEV, on_gpu=True)


def test_cosine_restart_per_epoch():
    cases.check_cosine_restart_per_epoch(DEV, on_gpu=True)


def test_plateau_drops_where_the_fixture_says_under_one_capture():
    cases.check_plateau(DEV, on_gpu=True)


def test_resumed_run_with_a_noisy_step_schedule_is_bit_equal(tmp_path):
    cases.check_resume(DEV, tmp_path, on_gpu=True)
