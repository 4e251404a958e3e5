"""Train for epochs -- the reference's `train_epoch` / `main` (train.py:238-364) and `TrainMeter` (utils/meters.py:59-141) over the pieces
this package already has, with the step replayed from ONE HIP graph and nothing in the batch loop that waits for the device.

No kernel lives here: every launch of the loop is one the pieces already make.  What lives here is the ORDER (DESIGN 5.9 lists it once):

  * the first `warmup` batches are eager steps; the next batch fixes the static buffers and the step is captured once, then replayed;
  * `schedule.apply` (FlatSGD.set_lr: one fill of `lr_dev`) and the loader's copy of the mixup draw into `mixup.params` are issued
    BETWEEN replays, on the training stream; neither is ever recorded;
  * a schedule under replay needs `device_lr=True` -- Trainer refuses the other form instead of training at the captured rate;
  * a resume goes through the optimizer (`resume_checkpoint(model, path, optimizer)`), in place: a step captured before it replays the
    resumed state;
  * the EMA weights are validated inside `optimizer.ema_weights()`; `sync_lookahead()` runs at the end of each epoch;
  * the loss stays on the device: `TrainMeter.record` is part of the captured step, and the host reads once per log line and once per
    epoch (`meter.host_reads`).

    step = ReplayedStep(model, opt, loss_fn, on_loss=meter.record)      # or: Trainer(model, opt, loss_fn, loader, num_epochs=...).fit()
    with step.stream_context():
        for epoch in range(num_epochs):
            train_epoch(epoch, model, loader, step, opt, meter=meter, schedule=schedule)
"""
import contextlib
import logging
import sys
import time

import numpy as np
import torch

from . import _lib
from .checkpoint import _is_flat, resume_checkpoint
from .mixup import DeviceMixup

_logger = logging.getLogger(__name__)
LOG_LINE = "Epoch: {:s}, Iter: {:s}, loss: {:.4f}, lr: {:s}, time_avg: {:.4f}, eta: {:s}, mem: {:d}"  # utils/meters.py:139


def time_string(seconds):
    """the reference's fixed-width days,hh:mm:ss (utils/meters.py:38-43)"""
    days, rem = divmod(int(seconds), 24 * 3600)
    hrs, rem = divmod(rem, 3600)
    mins, secs = divmod(rem, 60)
    return "{0:02},{1:02}:{2:02}:{3:02}".format(days, hrs, mins, secs)


def gpu_mem_usage(device=None):
    """the reference's figure (utils/meters.py:45-48): torch's peak allocation in MB; 0 for a CPU device"""
    if device is not None and torch.device(device).type != "cuda":
        return 0.0
    return torch.cuda.max_memory_allocated(device) / 1024 / 1024


class TrainMeter:
    """The reference's TrainMeter / ScalarMeter (utils/meters.py:59-141) with the numbers kept where the loss is.

    `record(loss, mb_size)` is the reference's `update_stats` without its `loss.item()` (train.py:290): plain torch ops on tensors
    allocated here once -- a ring of `log_interval` fp32 losses written at `counter % log_interval`, the counter itself (int64, on the
    device: a replayed step has no host code that could count), and fp64 `loss_total += loss * mb_size`, `num_samples += mb_size`
    (utils/meters.py:117-118).  It records into a HIP-graph capture like any other launch, so the step that ReplayedStep replays feeds
    the meter with no host work at all; mb_size is baked into a capture, which replays one batch shape only.

    `log_iter_stats(epoch, it)` returns at once unless `(it + 1) % log_interval == 0`; then ONE device-to-host copy (ring and counter;
    `host_reads` counts them) and the reference's line.  `loss` is `get_win_avg`: numpy's mean of the window's values as Python floats,
    oldest first -- the fp32 values widened exactly, so the figure EQUALS what a loop with `.item()` per step prints.  `lr` is
    `self.lr` (train_epoch sets `str([optimizer.lr])`), `mem` the reference's gpu_mem_usage.

    DEPARTURE: `time_avg` is the wall time since the previous log line (or `iter_tic()`) divided by the steps between them.  The
    reference times every step between two `torch.cuda.synchronize()` calls (train.py:282-293); that synchronisation is what this
    class removes, and without it a per-step timer would time the host's launch queue.

    With a process group the ring is mean-reduced once per log line (all-reduce, then 1 / world in fp32: the arithmetic of the
    reference's `scaled_all_reduce` per step, train.py:287), and `epoch_stats` sums `loss_total` and `num_samples` over the ranks.

    Plain torch: it works on CPU tensors too."""

    def __init__(self, log_interval, start_epoch, num_epochs, epoch_iters, device, process_group=None):
        if isinstance(log_interval, bool) or not isinstance(log_interval, int) or log_interval < 1:
            raise ValueError(f"TrainMeter(log_interval={log_interval!r}): an int >= 1")
        self.log_interval, self.epoch_iters = log_interval, epoch_iters
        self.device, self.process_group = torch.device(device), process_group
        self.set_range(start_epoch, num_epochs)
        self.ring = torch.zeros(log_interval, dtype=torch.float32, device=self.device)
        self.counter = torch.zeros(1, dtype=torch.int64, device=self.device)  # losses recorded since reset(); the slot is counter % L
        self.acc = torch.zeros(2, dtype=torch.float64, device=self.device)    # loss_total, num_samples
        self.lr = None
        self.host_reads = 0
        self.last_line = None
        self.iter_tic()

    def set_range(self, start_epoch, num_epochs):
        """the epochs the eta counts over (the reference fixes them at construction, utils/meters.py:89-98)"""
        self.start_epoch, self.max_epoch = start_epoch, num_epochs
        self.max_iter = (num_epochs - start_epoch) * self.epoch_iters

    def reset(self, timer=False):
        """utils/meters.py:100-106; three fills on the current stream.  Refused inside a capture: the recorded fills would empty the
        meter at every replay."""
        if _lib.capturing():
            raise RuntimeError("TrainMeter.reset() inside a HIP-graph capture: the fills would be recorded and empty the meter at every "
                               "replay -- reset between replays; the meter is left as it was")
        if timer:
            self.iter_tic()
        self.ring.zero_()
        self.counter.zero_()
        self.acc.zero_()
        self.lr = None

    def iter_tic(self):
        """start the window that the next log line's time_avg covers"""
        self._t0, self._steps = time.perf_counter(), 0

    def record(self, loss, mb_size):
        """loss: a 0-d tensor on the meter's device; six small launches, no host read"""
        v = loss.detach()
        self.ring.scatter_(0, torch.remainder(self.counter, self.log_interval), v.to(torch.float32).reshape(1))
        self.counter.add_(1)
        self.acc[0:1].add_(v.to(torch.float64).reshape(1), alpha=int(mb_size))  # (fp32 x a small integer is exact in fp64)
        self.acc[1:2].add_(int(mb_size))

    def _window(self):
        """THE host read of a log line -> the window's losses as Python floats, oldest first"""
        ring = self.ring
        dist = torch.distributed
        if self.process_group is not None and dist.is_available() and dist.is_initialized():
            ring = ring.clone()
            dist.all_reduce(ring, group=self.process_group)
            ring.mul_(1.0 / dist.get_world_size(self.process_group))
        host = torch.cat([ring.to(torch.float64), self.counter.to(torch.float64)]).cpu().tolist()
        self.host_reads += 1
        values, n = host[:-1], int(host[-1])
        if n <= self.log_interval:
            return values[:n]
        at = n % self.log_interval
        return values[at:] + values[:at]

    def get_iter_stats(self, cur_epoch, cur_iter):
        """utils/meters.py:120-133"""
        window = self._window()
        now = time.perf_counter()
        time_avg = (now - self._t0) / max(self._steps, 1)
        self._t0, self._steps = now, 0
        cur_iter_total = (cur_epoch - self.start_epoch) * self.epoch_iters + cur_iter + 1
        return {"epoch": "{}/{}".format(cur_epoch + 1, self.max_epoch), "iter": "{}/{}".format(cur_iter + 1, self.epoch_iters),
                "time_avg": time_avg, "eta": time_string(time_avg * (self.max_iter - cur_iter_total)),
                "loss": float(np.mean(window)) if window else float("nan"), "lr": self.lr,
                "mem": int(np.ceil(gpu_mem_usage(self.device)))}

    def log_iter_stats(self, cur_epoch, cur_iter):
        """call once per step.  -> the line it logged, or None"""
        self._steps += 1
        if (cur_iter + 1) % self.log_interval != 0:
            return None
        stats = self.get_iter_stats(cur_epoch, cur_iter)
        self.last_line = LOG_LINE.format(stats["epoch"], stats["iter"], stats["loss"], str(stats["lr"]), stats["time_avg"], stats["eta"],
                                         stats["mem"])
        _logger.info(self.last_line)
        return self.last_line

    def epoch_stats(self):
        """THE host read at the end of an epoch -> dict(updates, samples, loss_avg): the losses recorded since reset(), the samples
        they covered and loss_total / num_samples (with a process group: both summed over the ranks first)"""
        acc = self.acc
        dist = torch.distributed
        if self.process_group is not None and dist.is_available() and dist.is_initialized():
            acc = acc.clone()
            dist.all_reduce(acc, group=self.process_group)
        total, samples, updates = torch.cat([acc, self.counter.to(torch.float64)]).cpu().tolist()
        self.host_reads += 1
        return dict(updates=int(updates), samples=int(samples), loss_avg=total / samples if samples > 0 else float("nan"))


class ReplayedStep:
    """`step(input, target)` -> the loss, a 0-d tensor on the device: one training step, replayed from a HIP graph where it can be.

    ONE body serves the eager steps, the capture and the replays, in the reference's order (train.py:260-274):
    `optimizer.zero_grad()`, forward, `loss_fn`, `backward()`, `optimizer.step()`, then `on_loss(loss, batch_size)` (TrainMeter.record).

    graph=True, with a flat optimizer (FlatSGD, FlatAdam, FlatAdamW) whose model is on the GPU: the first `warmup` batches are real
    training steps issued eagerly (whatever a first call initialises must not happen while recording).  The next batch fixes shape and
    dtype of the static input and target buffers; the body is captured once (the capture records and does not run) and replayed for that
    batch and every later batch of the same shape, each copied into the static buffers first.  A batch of another shape -- a short last
    batch -- is stepped eagerly by the same body; a replay reads the weights when it runs, so the two mix freely.  A capture that fails
    leaves eager steps and says so (`graph_note`, a line on stderr).  Any other optimizer, or a model on the CPU, runs eagerly
    (`graph_note` says why).

    Everything runs on `self.stream`, the training stream (not the default stream: autograd's AccumulateGrad nodes remember the stream
    they were made under, and one made under the default stream aborts a capture).  `step()` called under another stream fences both
    ways; a loop enters `stream_context()` once and pays nothing per step.  What the captured kernels read from device memory is
    written BETWEEN replays on that stream: `optimizer.set_lr` (device_lr=True) and the mixup draw, which `PrefetchLoader` copies into
    `mixup.params` when it hands a batch over -- this class never calls `DeviceMixup.draw()`.

    The returned loss of a replay is the capture's own tensor: the next replay overwrites it (clone it to keep it).
    `on_loss` is read when the body runs; changing it after the capture does not change the replays."""

    def __init__(self, model, optimizer, loss_fn, *, graph=True, warmup=2, on_loss=None):
        self.model, self.optimizer, self.loss_fn, self.on_loss = model, optimizer, loss_fn, on_loss
        self.warmup = int(warmup)
        self.steps = self.replays = 0  # steps issued in all; those that were replays
        self.graph_note = None
        self.stream = self._graph = self._static = self._loss = None
        self._failed = False
        self.graph = bool(graph)
        if self.graph:
            first = next(iter(model.parameters()), None)
            if not _is_flat(optimizer):
                self.graph, self.graph_note = False, f"{type(optimizer).__name__} is no flat optimizer: eager steps"
            elif not (_lib.DEVICE_ONLY and first is not None and first.is_cuda):
                self.graph, self.graph_note = False, "the model is not on a GPU: eager steps"
            else:
                self.stream = torch.cuda.Stream(device=first.device)

    @contextlib.contextmanager
    def stream_context(self):
        """run the loop on the training stream: it waits for what the caller's stream holds on entry, and the caller's stream for it on
        exit.  A null context where there is no training stream."""
        if self.stream is None:
            yield
            return
        outer = torch.cuda.current_stream(self.stream.device)
        if outer == self.stream:
            yield
            return
        self.stream.wait_stream(outer)
        try:
            with torch.cuda.stream(self.stream):
                yield
        finally:
            outer.wait_stream(self.stream)

    def _body(self, x, y):
        self.optimizer.zero_grad()
        loss = self.loss_fn(self.model(x), y)
        loss.backward()
        self.optimizer.step()
        loss = loss.detach()
        if self.on_loss is not None:
            self.on_loss(loss, x.shape[0])
        return loss

    def _capture(self, x, y):
        sx, sy = x.clone(), y.clone()
        graph = torch.cuda.CUDAGraph()
        # (with a process group, the collectives' watchdog thread polls events while this thread records: bench.py, at its capture site)
        dist = torch.distributed
        mode = "thread_local" if (dist.is_available() and dist.is_initialized()) else "global"
        try:
            with torch.cuda.graph(graph, stream=self.stream, capture_error_mode=mode):
                loss = self._body(sx, sy)
        except Exception as e:  # the steps are then issued launch by launch
            self._failed = True
            self.graph_note = f"capture of the training step failed ({type(e).__name__}: {str(e)[:160]}); eager steps"
            print(f"[trainer] {self.graph_note}", file=sys.stderr, flush=True)
            torch.cuda.synchronize(x.device)
            self.optimizer.zero_grad()  # (bucket bookkeeping of the abandoned capture)
            return
        self._graph, self._static, self._loss = graph, (sx, sy), loss

    def _fits(self, x, y):
        sx, sy = self._static
        return x.shape == sx.shape and x.dtype == sx.dtype and y.shape == sy.shape and y.dtype == sy.dtype

    def _step(self, x, y):
        n = self.steps
        self.steps += 1
        if not self.graph or self._failed or n < self.warmup:
            return self._body(x, y)
        fresh = self._graph is None
        if fresh:
            self._capture(x, y)
            if self._graph is None:
                return self._body(x, y)
        elif not self._fits(x, y):
            return self._body(x, y)
        if not fresh:  # (the capture cloned this batch into the buffers)
            self._static[0].copy_(x)
            self._static[1].copy_(y)
        self._graph.replay()
        from . import cot_layer_fused
        cot_layer_fused.invalidate_packs()  # (the replayed update kernels moved the weights behind torch's version counters)
        self.replays += 1
        return self._loss

    def step(self, input, target):
        with self.stream_context():
            return self._step(input, target)

    __call__ = step


def train_epoch(epoch, model, loader, step, optimizer, *, meter=None, schedule=None, schedule_unit="epoch", mixup_off_epoch=0):
    """One epoch, train.py:243-297 in the reference's order: the `mixup_off_epoch` switch through `loader.mixup_enabled`, `model.train()`,
    per batch [with schedule_unit="update": `schedule.apply(optimizer, num_updates)`; `step(input, target)`; `meter.log_iter_stats`],
    then `optimizer.sync_lookahead()` where the optimizer has it and `meter.reset()`.

    step: a ReplayedStep, or any callable (input, target) -> loss on the device.  A ReplayedStep built with `on_loss=meter.record`
    feeds the meter from inside the step; for a step without an `on_loss` this function records the returned loss itself.
    DEPARTURE: the per-update schedule is applied IN FRONT of the step, step k trains at value(k); the reference's `step_update`
    behind the step (train.py:283-284) sets the next step's rate, so there step k trains at value(k - 1).

    -> dict(updates, samples, loss_avg): ONE host read at the end of the epoch (`meter.epoch_stats()`); without a meter, updates and
    samples are the host's own counts and loss_avg is None."""
    if schedule_unit not in ("epoch", "update"):
        raise ValueError(f"train_epoch(schedule_unit={schedule_unit!r}): 'epoch' or 'update'")
    if mixup_off_epoch and epoch >= mixup_off_epoch and getattr(loader, "mixup_enabled", False):
        loader.mixup_enabled = False
    model.train()
    num_updates = epoch * len(loader)
    feeds = meter is not None and getattr(step, "on_loss", None) is None  # nobody else feeds the meter
    stream_context = getattr(step, "stream_context", contextlib.nullcontext)
    updates = samples = 0
    with stream_context():
        if meter is not None:
            meter.iter_tic()
        for batch_idx, (input, target) in enumerate(loader):
            if schedule is not None and schedule_unit == "update":
                schedule.apply(optimizer, num_updates)
            loss = step(input, target)
            num_updates += 1
            updates += 1
            samples += input.shape[0]
            if meter is not None:
                if feeds:
                    meter.record(loss, input.shape[0])
                meter.lr = str([optimizer.lr]) if hasattr(optimizer, "lr") else \
                    str(list(set(g["lr"] for g in optimizer.param_groups)))  # (train.py:289)
                meter.log_iter_stats(epoch, batch_idx)
        if hasattr(optimizer, "sync_lookahead"):
            optimizer.sync_lookahead()
        if meter is None:
            return dict(updates=updates, samples=samples, loss_avg=None)
        out = meter.epoch_stats()
        meter.reset()
    return out


class Trainer:
    """The reference's `main` (train.py:314-364): `Trainer(model, optimizer, loss_fn, train_loader, num_epochs=...).fit(resume=None)`.

    fit: a resume through `resume_checkpoint(model, path, optimizer)` -- the stored epoch is the first one to run, the loop below saves
    `epoch + 1` --, `schedule.apply(optimizer, start_epoch)`, then per epoch, in this order: `sampler.set_epoch` where the loader has a
    sampler; `train_epoch`; `distribute_bn` where there is a process group and `dist_bn` is 'reduce' or 'broadcast'; `evaler(epoch,
    model)`; where `optimizer.ema_decay` is set, the same inside `optimizer.ema_weights()`, whose top-1 becomes the metric
    (train.py:352-355); `saver.save_recovery(epoch + 1)` when recovery_interval > 0 divides epoch + 1 (0, the reference's default, would divide
    by zero there: here it means off); with schedule_unit="epoch", `schedule.apply(optimizer, epoch + 1)` -- for a schedule whose class says `needs_metric`
    (PlateauLRSchedule) `schedule.apply(optimizer, epoch + 1, metric)`, the metric that the saver is about to get (DEPARTURE: the
    reference passes None there, train.py:361, on which its plateau scheduler raises) --; `saver.save_checkpoint(epoch
    + 1, metric=top1)`.  KeyboardInterrupt ends the loop cleanly.  -> `history`, one dict per epoch: epoch, train_loss, updates,
    samples, lr, top1 / top5 / loss of the model, ema_top1 / ema_top5 / ema_loss, best_metric, best_epoch (None where there is nothing
    to report).

    The whole of fit runs on the step's training stream (ReplayedStep.stream_context), validation and saves included.

    Refused at construction, because each would train silently wrong under replay: a schedule with graph=True on a flat optimizer built
    without `device_lr=True` (the capture would freeze the rate); graph=True with a train loader whose mixup is not a DeviceMixup (a
    capture reads the draw from `DeviceMixup.params`; a host-side mixup hands over dense targets that the captured loss cannot take).
    Refused too: a `needs_metric` schedule without an evaler, or with schedule_unit="update" -- there is no metric to step it with.
    NOT done here: `distribute_bn` of the EMA's averaged buffers (the reference's second call, train.py:353-354)."""

    def __init__(self, model, optimizer, loss_fn, train_loader, *, num_epochs, evaler=None, saver=None, schedule=None,
                 schedule_unit="epoch", log_interval=50, recovery_interval=0, mixup_off_epoch=0, graph=True, process_group=None,
                 dist_bn="reduce"):
        if schedule_unit not in ("epoch", "update"):
            raise ValueError(f"Trainer(schedule_unit={schedule_unit!r}): 'epoch' or 'update'")
        if dist_bn not in ("reduce", "broadcast", "", None, False):
            raise ValueError(f"Trainer(dist_bn={dist_bn!r}): 'reduce', 'broadcast' or '' (off)")
        flat = _is_flat(optimizer)
        if graph and flat and schedule is not None and getattr(optimizer, "lr_dev", None) is None:
            raise ValueError(f"Trainer(schedule=..., graph=True): {type(optimizer).__name__} was built without device_lr=True, so a captured "
                             "step keeps the rate it was captured with and the schedule would not reach the replays -- build the optimizer "
                             "with device_lr=True, or pass graph=False")
        if getattr(schedule, "needs_metric", False):
            if evaler is None:
                raise ValueError(f"Trainer(schedule={type(schedule).__name__}(...)): the schedule is stepped with the epoch's validation metric and "
                                 "there is no evaler to produce one -- pass evaler=..., or a schedule that needs no metric")
            if schedule_unit == "update":
                raise ValueError(f"Trainer(schedule={type(schedule).__name__}(...), schedule_unit='update'): the schedule is stepped with the "
                                 "epoch's validation metric, and there is none per update -- pass schedule_unit='epoch'")
        mixup = getattr(train_loader, "mixup", getattr(train_loader, "mixup_fn", None))
        if graph and flat and not isinstance(mixup, DeviceMixup) and (mixup is not None or getattr(train_loader, "mixup_enabled", False)):
            raise ValueError(f"Trainer(graph=True): the train loader's mixup is a {type(mixup).__name__}, not a DeviceMixup -- a captured step "
                             "reads the batch's draw from DeviceMixup.params on the device; build the loader with "
                             "PrefetchLoader(..., mixup=DeviceMixup(...)), or pass graph=False")
        self.model, self.optimizer, self.loss_fn, self.train_loader = model, optimizer, loss_fn, train_loader
        self.num_epochs, self.evaler, self.saver, self.schedule, self.schedule_unit = num_epochs, evaler, saver, schedule, schedule_unit
        self.recovery_interval, self.mixup_off_epoch = int(recovery_interval), mixup_off_epoch
        self.process_group, self.dist_bn = process_group, dist_bn
        first = next(iter(model.parameters()), None)
        device = first.device if first is not None else torch.device("cpu")
        self.meter = TrainMeter(log_interval, 0, num_epochs, len(train_loader), device, process_group)
        self.step = ReplayedStep(model, optimizer, loss_fn, graph=graph, on_loss=self.meter.record)
        self.history = []
        self.best_metric = self.best_epoch = None

    def _validate(self, epoch):
        top1, top5 = self.evaler(epoch, self.model)
        return dict(top1=top1, top5=top5, loss=(getattr(self.evaler, "last", None) or {}).get("loss"))

    def fit(self, resume=None):
        model, optimizer, loader = self.model, self.optimizer, self.train_loader
        with self.step.stream_context():
            start_epoch = 0
            if resume:
                start_epoch = resume_checkpoint(model, resume, optimizer) or 0
            if self.schedule is not None:
                self.schedule.apply(optimizer, start_epoch)
            self.meter.set_range(start_epoch, self.num_epochs)
            self.meter.reset(timer=True)
            history = self.history = []
            try:
                for epoch in range(start_epoch, self.num_epochs):
                    sampler = getattr(loader, "sampler", None)
                    if hasattr(sampler, "set_epoch"):
                        sampler.set_epoch(epoch)
                    trained = train_epoch(epoch, model, loader, self.step, optimizer, meter=self.meter, schedule=self.schedule,
                                          schedule_unit=self.schedule_unit, mixup_off_epoch=self.mixup_off_epoch)
                    row = dict(epoch=epoch, train_loss=trained["loss_avg"], updates=trained["updates"], samples=trained["samples"],
                               lr=getattr(optimizer, "lr", None), top1=None, top5=None, loss=None, ema_top1=None, ema_top5=None,
                               ema_loss=None)
                    if self.process_group is not None and self.dist_bn in ("reduce", "broadcast"):
                        from .data_parallel import distribute_bn
                        _logger.info("Distributing BatchNorm running means and vars")
                        distribute_bn(model, self.process_group, self.dist_bn == "reduce")
                    metric = None
                    if self.evaler is not None:
                        row.update(self._validate(epoch))
                        metric = row["top1"]
                        if getattr(optimizer, "ema_decay", None) is not None:
                            with optimizer.ema_weights():
                                ema = self._validate(epoch)
                            row.update(ema_top1=ema["top1"], ema_top5=ema["top5"], ema_loss=ema["loss"])
                            metric = ema["top1"]
                    if self.saver is not None and self.recovery_interval > 0 and (epoch + 1) % self.recovery_interval == 0:
                        self.saver.save_recovery(epoch + 1)
                    if self.schedule is not None and self.schedule_unit == "epoch":
                        if getattr(self.schedule, "needs_metric", False):
                            self.schedule.apply(optimizer, epoch + 1, metric)
                        else:
                            self.schedule.apply(optimizer, epoch + 1)
                    if self.saver is not None:
                        self.best_metric, self.best_epoch = self.saver.save_checkpoint(epoch + 1, metric=metric)
                    elif metric is not None and (self.best_metric is None or metric > self.best_metric):
                        self.best_metric, self.best_epoch = metric, epoch + 1
                    row.update(best_metric=self.best_metric, best_epoch=self.best_epoch)
                    history.append(row)
            except KeyboardInterrupt:
                pass
        if self.best_metric is not None:
            _logger.info("*** Best metric: {0} (epoch {1})".format(self.best_metric, self.best_epoch))
        return history
