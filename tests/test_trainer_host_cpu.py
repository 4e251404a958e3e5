"""cotnet_amd.trainer on the host: TrainMeter on CPU tensors against the reference's formulas (utils/meters.py:59-141, restated here from
its deque, numpy mean and Python-float sums), and the ORDER of `Trainer.fit` / `train_epoch` on recording stand-ins against the sequence
of the reference's train.py:243-364, written out below.  No GPU, no library call: the meter is plain torch and the stand-ins only log."""
import contextlib
import re
from collections import deque

import numpy as np
import pytest
import torch
from torch import nn

import cotnet_amd
from cotnet_amd import trainer as tr
from cotnet_amd.trainer import ReplayedStep, TrainMeter, Trainer, train_epoch


# ---- TrainMeter

class _RefMeter:
    """the reference's ScalarMeter + TrainMeter arithmetic on `loss.item()` values (utils/meters.py:62-84, :114-118)"""

    def __init__(self, window):
        self.deque, self.loss_total, self.num_samples = deque(maxlen=window), 0.0, 0

    def update_stats(self, loss, mb_size):
        self.deque.append(loss)
        self.loss_total += loss * mb_size
        self.num_samples += mb_size

    def get_win_avg(self):
        return np.mean(self.deque)


def _losses(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, generator=g) * 7).to(torch.float32)  # values whose fp32 sums round: an fp32 mean would differ from the double one


@pytest.mark.parametrize("window", [1, 2, 3, 5])
def test_window_mean_and_loss_avg_equal_the_references_formulas(window):
    losses, sizes = _losses(11, seed=window), [4, 4, 2, 4, 6, 4, 4, 2, 8, 4, 2]
    meter, ref = TrainMeter(window, 0, 1, len(losses), "cpu"), _RefMeter(window)
    meter.lr = "[0.1]"
    lines = 0
    for it, (v, mb) in enumerate(zip(losses, sizes)):
        meter.record(v, mb)
        ref.update_stats(v.item(), mb)
        before = meter.host_reads
        line = meter.log_iter_stats(0, it)
        if (it + 1) % window == 0:
            lines += 1
            assert meter.host_reads == before + 1
            assert line is not None and f"loss: {ref.get_win_avg():.4f}," in line
            assert float(np.mean(meter._window())) == float(ref.get_win_avg())  # equal, not close
        else:
            assert line is None and meter.host_reads == before, "a step that logs nothing read the host"
    reads = meter.host_reads
    out = meter.epoch_stats()
    assert meter.host_reads == reads + 1
    assert out == dict(updates=len(losses), samples=ref.num_samples, loss_avg=ref.loss_total / ref.num_samples)
    assert lines == len(losses) // window


def test_window_mean_before_the_ring_is_full_and_after_it_wrapped():
    losses = _losses(7, seed=9)
    meter, ref = TrainMeter(4, 0, 1, 7, "cpu"), _RefMeter(4)
    for k, v in enumerate(losses):
        meter.record(v, 2)
        ref.update_stats(v.item(), 2)
        got = meter.get_iter_stats(0, k)["loss"]  # (every k: 1, 2, 3 values, a full ring, and rings that wrapped by 1, 2, 3)
        assert got == float(ref.get_win_avg()), (k, got, float(ref.get_win_avg()))
        assert meter._window() == list(ref.deque)  # oldest first, as the deque holds them
    assert meter.host_reads == 2 * len(losses)


def test_reset_is_the_references():
    meter = TrainMeter(2, 0, 1, 4, "cpu")
    meter.lr = "[1]"
    meter.record(torch.tensor(3.0), 4)
    meter.reset()
    assert meter.lr is None and meter._window() == []
    assert meter.epoch_stats()["updates"] == 0 and meter.epoch_stats()["samples"] == 0
    meter.record(torch.tensor(1.5), 2)
    assert meter.epoch_stats() == dict(updates=1, samples=2, loss_avg=1.5)
    with pytest.raises(ValueError, match="log_interval"):
        TrainMeter(0, 0, 1, 4, "cpu")


def test_the_logged_line_is_the_references_format(caplog):
    assert tr.LOG_LINE == "Epoch: {:s}, Iter: {:s}, loss: {:.4f}, lr: {:s}, time_avg: {:.4f}, eta: {:s}, mem: {:d}"  # utils/meters.py:139
    meter = TrainMeter(2, 1, 3, 5, "cpu")  # epochs 1 and 2 of 3 are to run
    meter.lr = str([0.1])
    meter.record(torch.tensor(1.0), 4)
    meter.log_iter_stats(1, 0)
    meter.record(torch.tensor(1.4690001), 4)
    with caplog.at_level("INFO", logger="cotnet_amd.trainer"):
        line = meter.log_iter_stats(1, 1)
    want = float(np.mean([1.0, torch.tensor(1.4690001).item()]))
    m = re.fullmatch(r"Epoch: 2/3, Iter: 2/5, loss: (\d+\.\d{4}), lr: \[0\.1\], time_avg: (\d+\.\d{4}), eta: \d\d,\d\d:\d\d:\d\d, mem: 0", line)
    assert m, line
    assert m.group(1) == f"{want:.4f}"
    assert line == meter.last_line and line in caplog.text
    assert tr.time_string(3 * 86400 + 4 * 3600 + 5 * 60 + 6) == "03,04:05:06"
    stats = meter.get_iter_stats(1, 1)
    assert stats["epoch"] == "2/3" and stats["iter"] == "2/5" and stats["mem"] == 0


# ---- the order of the loop

class _Model(nn.Linear):
    def __init__(self, log):
        super().__init__(4, 3)
        self.log = log

    def train(self, mode=True):
        if hasattr(self, "log") and mode:
            self.log.append("model.train")
        return super().train(mode)

    def forward(self, x):
        self.log.append("forward")
        return super().forward(x)


class _Optimizer:
    """a recording stand-in; flat=True gives it what checkpoint._is_flat looks for"""

    def __init__(self, log, model, ema_decay=None, flat=False, lr_dev=None):
        self.log, self.model, self.lr, self.ema_decay, self.lr_dev = log, model, 0.5, ema_decay, lr_dev
        if flat:
            self.model_state_dict = self.load_model_state_dict = lambda *a: None

    def zero_grad(self):
        self.log.append("zero_grad")
        for p in self.model.parameters():
            p.grad = None

    def step(self):
        assert all(p.grad is not None for p in self.model.parameters()), "optimizer.step() in front of backward()"
        self.log.append("optimizer.step")

    def set_lr(self, lr):
        self.lr = lr

    def sync_lookahead(self):
        self.log.append("sync_lookahead")

    @contextlib.contextmanager
    def ema_weights(self):
        self.log.append("ema_weights enter")
        yield self
        self.log.append("ema_weights exit")


class _Schedule:
    def __init__(self, log):
        self.log = log

    def apply(self, opt, t):
        self.log.append(f"schedule.apply({t})")
        opt.set_lr(1.0 / (1 + t))
        return opt.lr


class _Sampler:
    def __init__(self, log):
        self.log = log

    def set_epoch(self, epoch):
        self.log.append(f"set_epoch({epoch})")


class _Loader:
    def __init__(self, log, batches=2, mixup=None):
        self.log, self.n, self.sampler, self._on = log, batches, _Sampler(log), True
        if mixup is not None:
            self.mixup = mixup

    @property
    def mixup_enabled(self):
        return self._on

    @mixup_enabled.setter
    def mixup_enabled(self, x):
        self.log.append(f"mixup_enabled = {x}")
        self._on = x

    def __len__(self):
        return self.n

    def __iter__(self):
        g = torch.Generator().manual_seed(3)
        for _ in range(self.n):
            yield torch.randn(4, 4, generator=g), torch.randint(0, 3, (4,), generator=g)


class _Evaler:
    def __init__(self, log, opt):
        self.log, self.opt, self.inside, self.last = log, opt, False, None

    def __call__(self, epoch, model):
        ema = self.log[-1] == "ema_weights enter"
        self.log.append(f"evaler({epoch})")
        self.last = dict(top1=0.75 if ema else 0.25, top5=0.9 if ema else 0.5, loss=1.0 if ema else 2.0)
        return self.last["top1"], self.last["top5"]


class _Saver:
    def __init__(self, log):
        self.log = log

    def save_recovery(self, epoch, batch_idx=0):
        self.log.append(f"save_recovery({epoch})")

    def save_checkpoint(self, epoch, metric=None):
        self.log.append(f"save_checkpoint({epoch}, metric={metric})")
        return metric, epoch


def _loss_fn(log):
    def loss_fn(out, target):
        log.append("loss_fn")
        return nn.functional.cross_entropy(out, target)
    return loss_fn


def _trainer(log, num_epochs=2, ema=0.99, **kw):
    model = _Model(log)
    opt = _Optimizer(log, model, ema_decay=ema)
    kw.setdefault("schedule", _Schedule(log))
    t = Trainer(model, opt, _loss_fn(log), kw.pop("loader", None) or _Loader(log), num_epochs=num_epochs, evaler=_Evaler(log, opt),
                saver=_Saver(log), log_interval=1, **kw)
    record, stats = t.meter.record, t.meter.log_iter_stats
    t.step.on_loss = lambda loss, n: (log.append(f"on_loss({n})"), record(loss, n))[1]  # (an eager step reads on_loss at every call)
    t.meter.log_iter_stats = lambda e, i: (log.append(f"log_iter_stats({e}, {i})"), stats(e, i))[1]
    return t


def _batch(n=4):
    return ["zero_grad", "forward", "loss_fn", "optimizer.step", f"on_loss({n})"]


def test_fit_runs_the_references_sequence():
    """train.py:314-364 around train.py:243-297, two epochs of two batches, everything on"""
    log = []
    t = _trainer(log, recovery_interval=1)
    history = t.fit()
    assert t.step.graph is False and "no flat optimizer" in t.step.graph_note
    want = ["schedule.apply(0)",                                                       # lr_scheduler.step(start_epoch), train.py:139
            # epoch 0
            "set_epoch(0)",                                                            # :339
            "model.train",                                                             # :250
            *_batch(), "log_iter_stats(0, 0)",                                         # :254-293
            *_batch(), "log_iter_stats(0, 1)",
            "sync_lookahead",                                                          # :295-296
            "evaler(0)",                                                               # :350
            "ema_weights enter", "evaler(0)", "ema_weights exit",                      # :352-355
            "save_recovery(1)",                                                        # :357-358
            "schedule.apply(1)",                                                       # :360-361
            "save_checkpoint(1, metric=0.75)",                                         # :363-364, the EMA's top-1
            # epoch 1
            "set_epoch(1)", "model.train",
            *_batch(), "log_iter_stats(1, 0)",
            *_batch(), "log_iter_stats(1, 1)",
            "sync_lookahead", "evaler(1)", "ema_weights enter", "evaler(1)", "ema_weights exit", "save_recovery(2)", "schedule.apply(2)",
            "save_checkpoint(2, metric=0.75)"]
    assert log == want, [(i, a, b) for i, (a, b) in enumerate(zip(log, want)) if a != b][:3] or (len(log), len(want))
    assert [h["epoch"] for h in history] == [0, 1]
    h = history[-1]
    assert (h["top1"], h["top5"], h["loss"], h["ema_top1"], h["ema_top5"], h["ema_loss"]) == (0.25, 0.5, 2.0, 0.75, 0.9, 1.0)
    assert (h["best_metric"], h["best_epoch"]) == (0.75, 2), "the EMA's top-1 is the metric"
    assert h["updates"] == 2 and h["samples"] == 8 and h["train_loss"] > 0 and h["lr"] == 0.5  # epoch 1 trained at schedule(1)
    assert t.meter.host_reads == 2 * (2 + 1)  # per epoch: two log lines and the read at its end


def test_recovery_interval_zero_is_off_and_two_divides_the_second_epoch():
    log = []
    _trainer(log, recovery_interval=0).fit()
    assert not [e for e in log if e.startswith("save_recovery")]
    log = []
    _trainer(log, recovery_interval=2).fit()
    assert [e for e in log if e.startswith("save_recovery")] == ["save_recovery(2)"]
    assert log.index("save_recovery(2)") < log.index("schedule.apply(2)") < log.index("save_checkpoint(2, metric=0.75)")


def test_without_an_ema_the_models_top1_is_the_metric():
    log = []
    history = _trainer(log, ema=None).fit()
    assert "ema_weights enter" not in log and [e for e in log if e.startswith("save_checkpoint")] == \
        ["save_checkpoint(1, metric=0.25)", "save_checkpoint(2, metric=0.25)"]
    assert history[-1]["ema_top1"] is None and history[-1]["best_metric"] == 0.25


def test_per_update_schedule_is_applied_in_front_of_every_step():
    log = []
    _trainer(log, schedule_unit="update").fit()
    sched = [e for e in log if e.startswith("schedule.apply")]
    assert sched == ["schedule.apply(0)"] + [f"schedule.apply({u})" for u in range(4)]  # start_epoch, then num_updates 0..3
    for u in range(4):
        at = [i for i, e in enumerate(log) if e == f"schedule.apply({u})"][-1]
        assert log[at + 1] == "zero_grad", "the rate is set in front of the step it belongs to"


def test_mixup_off_epoch_flips_the_loader_at_that_epoch():
    log = []
    _trainer(log, num_epochs=3, mixup_off_epoch=1).fit()
    flips = [i for i, e in enumerate(log) if e == "mixup_enabled = False"]
    assert len(flips) == 1, "flipped once: a loader that is off already is left alone (train.py:244)"
    assert log[flips[0] - 1] == "set_epoch(1)" and log[flips[0] + 1] == "model.train"  # train.py:243-250
    log = []
    _trainer(log, num_epochs=2, mixup_off_epoch=0).fit()
    assert "mixup_enabled = False" not in log  # 0 is off (train.py:243)


def test_a_resume_starts_at_the_stored_epoch(monkeypatch):
    log = []
    t = _trainer(log, num_epochs=4)

    def resume(model, path, optimizer):
        assert model is t.model and optimizer is t.optimizer, "the load goes through the optimizer"
        log.append(f"resume_checkpoint({path})")
        return 2
    monkeypatch.setattr(tr, "resume_checkpoint", resume)
    history = t.fit(resume="last.pth.tar")
    assert log[:4] == ["resume_checkpoint(last.pth.tar)", "schedule.apply(2)", "set_epoch(2)", "model.train"]
    assert [h["epoch"] for h in history] == [2, 3]
    assert [e for e in log if e.startswith("save_checkpoint")] == ["save_checkpoint(3, metric=0.75)", "save_checkpoint(4, metric=0.75)"]
    assert t.meter.start_epoch == 2 and t.meter.max_iter == 2 * 2


def test_keyboard_interrupt_ends_fit_cleanly():
    log = []
    t = _trainer(log, num_epochs=3)

    def interrupted(epoch, model):
        if epoch == 1:
            raise KeyboardInterrupt
        return 0.1, 0.2
    t.evaler = interrupted
    history = t.fit()
    assert [h["epoch"] for h in history] == [0]


def test_train_epoch_alone_feeds_a_meter_that_the_step_does_not():
    log = []
    model = _Model(log)
    opt = _Optimizer(log, model)
    meter = TrainMeter(2, 0, 1, 3, "cpu")
    step = ReplayedStep(model, opt, _loss_fn(log), graph=False)
    out = train_epoch(0, model, _Loader(log, batches=3), step, opt, meter=meter)
    assert out["updates"] == 3 and out["samples"] == 12 and out["loss_avg"] > 0
    assert meter.host_reads == 1 + 1 and "lr: [0.5]" in meter.last_line
    assert log[-1] == "sync_lookahead" and log[0] == "model.train"
    none = train_epoch(0, model, _Loader(log, batches=3), step, opt)
    assert none == dict(updates=3, samples=12, loss_avg=None)
    with pytest.raises(ValueError, match="schedule_unit"):
        train_epoch(0, model, _Loader(log), step, opt, schedule_unit="batch")


# ---- the refusals

def test_a_schedule_under_replay_needs_device_lr():
    log = []
    model = _Model(log)
    flat = _Optimizer(log, model, flat=True)
    loader = _Loader(log, mixup=cotnet_amd.DeviceMixup(device="cpu", num_classes=3))
    with pytest.raises(ValueError, match="device_lr=True"):
        Trainer(model, flat, _loss_fn(log), loader, num_epochs=1, schedule=_Schedule(log), graph=True)
    Trainer(model, flat, _loss_fn(log), loader, num_epochs=1, schedule=_Schedule(log), graph=False)
    Trainer(model, flat, _loss_fn(log), loader, num_epochs=1, schedule=None, graph=True)
    on_device = _Optimizer(log, model, flat=True, lr_dev=torch.zeros(1))
    Trainer(model, on_device, _loss_fn(log), loader, num_epochs=1, schedule=_Schedule(log), graph=True)


def test_replay_needs_the_mixup_on_the_device():
    log = []
    model = _Model(log)
    flat = _Optimizer(log, model, flat=True, lr_dev=torch.zeros(1))

    class HostMixup:
        mixup_enabled = True
    with pytest.raises(ValueError, match=r"graph=True.*not a DeviceMixup"):
        Trainer(model, flat, _loss_fn(log), _Loader(log, mixup=HostMixup()), num_epochs=1, graph=True)
    Trainer(model, flat, _loss_fn(log), _Loader(log, mixup=HostMixup()), num_epochs=1, graph=False)
    mix = cotnet_amd.DeviceMixup(device="cpu", num_classes=3)
    Trainer(model, flat, _loss_fn(log), _Loader(log, mixup=mix), num_epochs=1, graph=True)


def test_exports():
    for name in ("ReplayedStep", "TrainMeter", "train_epoch", "Trainer"):
        assert getattr(cotnet_amd, name) is getattr(tr, name)
