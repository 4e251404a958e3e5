"""cotnet_amd.checkpoint without a device: CheckpointSaver's file rotation against the reference's rules (utils/checkpoint_saver.py:60-157)
with a stub optimizer, what a file holds, and resume_checkpoint's return value and prefix handling."""
import os

import numpy as np
import torch
from torch import nn

from cotnet_amd import CheckpointSaver, resume_checkpoint


class _StubOptimizer:
    def __init__(self):
        self.loaded = None

    def state_dict(self):
        return {"state": {}, "param_groups": [{"lr": 0.1, "params": []}]}

    def load_state_dict(self, d):
        self.loaded = d


def _saver(tmp_path, **kw):
    torch.manual_seed(0)
    model = nn.Linear(3, 2)
    ck, rec = tmp_path / "ck", tmp_path / "rec"
    ck.mkdir()
    rec.mkdir()
    return model, CheckpointSaver(model, _StubOptimizer(), checkpoint_dir=str(ck), recovery_dir=str(rec), **kw), ck, rec


def _names(d):
    return sorted(os.listdir(d))


def test_the_best_two_are_kept_and_last_is_what_was_not(tmp_path):
    """max_history = 2, saves five epochs apart: a save is renamed tmp -> last -> checkpoint-N while the history has room or its metric
    beats the worst kept one, which then falls out; a save that does not stays as `last`"""
    model, saver, ck, _ = _saver(tmp_path, max_history=2)
    assert saver.save_checkpoint(0, 50.0) == (50.0, 0)
    assert _names(ck) == ["checkpoint-0.pth.tar"]  # (neither tmp nor last is left behind a kept save)
    assert saver.save_checkpoint(5, 60.0) == (60.0, 5)
    assert _names(ck) == ["checkpoint-0.pth.tar", "checkpoint-5.pth.tar"]
    assert saver.save_checkpoint(10, 40.0) == (60.0, 5)  # worse than both: not kept
    assert _names(ck) == ["checkpoint-0.pth.tar", "checkpoint-5.pth.tar", "last.pth.tar"]
    assert torch.load(str(ck / "last.pth.tar"), weights_only=False)["epoch"] == 10
    assert saver.save_checkpoint(15, 55.0) == (60.0, 5)  # beats the worst (50): epoch 0 falls out, and `last` moved on
    assert _names(ck) == ["checkpoint-15.pth.tar", "checkpoint-5.pth.tar"]
    assert [os.path.basename(p) for p, _ in saver.checkpoint_files] == ["checkpoint-5.pth.tar", "checkpoint-15.pth.tar"]
    assert saver.save_checkpoint(20, 70.0) == (70.0, 20)
    assert _names(ck) == ["checkpoint-20.pth.tar", "checkpoint-5.pth.tar"]


def test_a_lower_metric_is_better_when_decreasing(tmp_path):
    model, saver, ck, _ = _saver(tmp_path, max_history=2, decreasing=True)
    for epoch, loss in ((0, 3.0), (5, 2.0), (10, 2.5), (15, 4.0)):
        best = saver.save_checkpoint(epoch, loss)
    assert best == (2.0, 5)
    assert _names(ck) == ["checkpoint-10.pth.tar", "checkpoint-5.pth.tar", "last.pth.tar"]


def test_without_a_metric_nothing_is_best(tmp_path):
    model, saver, ck, _ = _saver(tmp_path, max_history=3)
    assert saver.save_checkpoint(0) == (None, None)
    assert _names(ck) == ["checkpoint-0.pth.tar"]


def test_the_recovery_rotation_keeps_two_files(tmp_path):
    model, saver, _, rec = _saver(tmp_path, recovery_prefix="rec")
    assert saver.find_recovery() == ""
    saver.save_recovery(1, 100)
    saver.save_recovery(1, 200)
    assert _names(rec) == ["rec-1-100.pth.tar", "rec-1-200.pth.tar"]
    saver.save_recovery(2, 0)
    assert _names(rec) == ["rec-1-200.pth.tar", "rec-2-0.pth.tar"]
    assert saver.find_recovery() == str(rec / "rec-1-200.pth.tar")  # the first by name, as in the reference
    saver.save_recovery(2, 50)
    assert _names(rec) == ["rec-2-0.pth.tar", "rec-2-50.pth.tar"]


def test_what_a_file_holds(tmp_path):
    class Cfg:
        model = "cotnet50"
    model, saver, ck, _ = _saver(tmp_path, cfg=Cfg(), rng=True)
    state = saver.state(7, metric=81.5)
    assert set(state) == {"epoch", "arch", "state_dict", "optimizer", "version", "metric", "args", "rng"}
    assert state["version"] == 2 and state["epoch"] == 7 and state["arch"] == "cotnet50" and state["metric"] == 81.5
    assert set(state["rng"]) == {"torch_cpu", "numpy"}
    assert all(v.device.type == "cpu" for v in state["state_dict"].values())
    plain = CheckpointSaver(model, _StubOptimizer(), checkpoint_dir=str(ck)).state(3)
    assert set(plain) == {"epoch", "arch", "state_dict", "optimizer", "version"} and plain["arch"] == "linear"


def test_resume_returns_the_epoch_strips_the_prefix_and_restores_the_generators(tmp_path):
    model, saver, ck, _ = _saver(tmp_path, rng=True)
    np.random.seed(4)
    torch.manual_seed(4)
    saver.save_checkpoint(12, 1.0)
    want = (np.random.rand(), float(torch.rand(())))
    path = str(ck / "checkpoint-12.pth.tar")
    file = torch.load(path, weights_only=False)
    file["state_dict"] = {"module." + k: v for k, v in file["state_dict"].items()}
    torch.save(file, path)
    other, opt = nn.Linear(3, 2), _StubOptimizer()
    assert not torch.equal(other.weight, model.weight)
    assert resume_checkpoint(other, path, optimizer=opt, log_info=False) == 12
    assert torch.equal(other.weight, model.weight) and torch.equal(other.bias, model.bias)
    assert opt.loaded == saver.optimizer.state_dict()
    assert (np.random.rand(), float(torch.rand(()))) == want
    third = nn.Linear(3, 2)
    assert resume_checkpoint(third, path, log_info=False) == 12 and torch.equal(third.weight, model.weight)  # (registry.load_checkpoint)
    bare = str(tmp_path / "bare.pth")
    torch.save(model.state_dict(), bare)
    assert resume_checkpoint(nn.Linear(3, 2), bare, log_info=False) is None
