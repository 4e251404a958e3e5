"""Validation on the device -- the reference's evaler/evaler.py (`Evaler`) and utils/meters.py (`accuracy`, `TestMeter`).

The reference scores a batch with `output.topk(5)`, a transpose, `eq` and two sums (utils/meters.py:12-19), hands the two counts to a host
meter (:154-157) and synchronises after every batch (evaler/evaler.py:50-52).  Here a batch is ONE call of `cot_eval_score`
(csrc/eval_score.hip): two launches that ADD the batch's samples, top-1 hits, top-5 hits and summed negative log-likelihood to a 32-byte
block in device memory.  The host reads the block once, at the end of the pass (`DeviceTestMeter.result`), so nothing in the batch loop
waits for the device, and -- nothing about the batch being a kernel argument -- forward plus scoring can be recorded into one HIP graph
and replayed on every batch of the validation set (`Evaler(graph=True)`); a short last batch is padded with the label -1, which the
kernel skips.

    evaler = Evaler(loader_eval, graph=True)
    top1, top5 = evaler(epoch, model)                  # the model's weights
    with opt.ema_weights():                            # FlatSGD(ema_decay=...): the average, through the model's own buckets
        top1_ema, top5_ema = evaler(epoch, model)      # (the number the reference reports, train.py:350-355)
"""
import contextlib
import sys
import weakref

import torch

from . import _lib


def _check(who, logits, labels):
    if not (isinstance(logits, torch.Tensor) and isinstance(labels, torch.Tensor)):
        raise TypeError(f"{who}: logits and labels are tensors")
    if logits.dim() != 2 or labels.shape != logits.shape[:1] or labels.dtype != torch.int64:
        raise TypeError(f"{who}: logits [N, K] and int64 labels [N]")
    if logits.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"{who}: {logits.dtype} logits (float32 / bfloat16)")
    if logits.shape[0] < 1 or logits.shape[1] < 1:
        raise ValueError(f"{who}: empty logits {tuple(logits.shape)}")
    if _lib.DEVICE_ONLY and not logits.is_cuda:
        raise RuntimeError(f"{who}: cotnet_amd has no CPU path (logits must be on the GPU)")
    if labels.device != logits.device:
        raise ValueError(f"{who}: labels on {labels.device}, logits on {logits.device}")


def _score(logits, labels, acc, rank=None, nll=None):
    N, K = logits.shape
    logits, labels = logits.contiguous(), labels.contiguous()
    _lib.api().cot_eval_score(logits.data_ptr(), labels.data_ptr(), acc.data_ptr(), _lib.ptr(rank), _lib.ptr(nll), N, K,
                              _lib.dtype_code(logits.dtype), _lib.stream())


def accuracy(output, target, topk=(1,)):
    """the reference's signature and return value (utils/meters.py:12-19): for every k the NUMBER of rows whose target is among the k
    largest logits, as fp32 0-dim tensors on the device, no host read.  Formed from the target's rank in a stable descending sort
    (`cot_eval_score`'s row_rank), so any k is served and equal logits are placed by column index, where topk picks as it pleases.
    A label outside [0, K) is no hit for any k."""
    _check("accuracy", output, target)
    acc = torch.zeros(4, dtype=torch.int64, device=output.device)
    rank = torch.empty(output.shape[0], dtype=torch.int32, device=output.device)
    _score(output, target, acc, rank=rank)
    return [((rank >= 0) & (rank < int(k))).sum().float() for k in topk]


class DeviceTestMeter:
    """the reference's TestMeter (utils/meters.py:143-177) with its three numbers, and the summed loss, in ONE `cot_eval_acc` block on the
    device: int64 samples, top1, top5 and an fp64 nll_sum.  `update` adds a batch without a host read; `result` is the only one."""

    def __init__(self, device):
        self.device = torch.device(device)
        if _lib.DEVICE_ONLY and self.device.type != "cuda":
            raise RuntimeError("DeviceTestMeter: cotnet_amd has no CPU path (the block lives on the GPU)")
        self.acc = torch.zeros(4, dtype=torch.int64, device=self.device)  # 32 bytes; [3] holds the bits of the fp64 nll_sum

    def reset(self):
        """zero the block with one fill on the current stream.  Refused inside a HIP-graph capture, for the reason FlatSGD.set_lr gives:
        the recorded fill would empty the block at every replay, and a pass would end with its last batch alone."""
        if _lib.capturing():
            raise RuntimeError("DeviceTestMeter.reset() inside a HIP-graph capture: the fill would be recorded and empty the block at every "
                               "replay -- reset outside the capture (replays add to the block when they run); the block is left as it was")
        self.acc.zero_()

    def update(self, logits, labels, row_rank=None, row_nll=None):
        """add one batch: logits [N, K] fp32 / bf16, labels int64 [N] (outside [0, K): the row is skipped).  One `cot_eval_score` call.
        row_rank (int32 [N]) / row_nll (fp32 [N]), if given, receive the rows' results."""
        _check("DeviceTestMeter.update", logits, labels)
        if logits.device != self.acc.device:
            raise ValueError(f"DeviceTestMeter.update: logits on {logits.device}, the block on {self.acc.device}")
        for t, dt, name in ((row_rank, torch.int32, "row_rank"), (row_nll, torch.float32, "row_nll")):
            if t is not None and (t.dtype != dt or t.numel() != logits.shape[0] or not t.is_contiguous() or t.device != logits.device):
                raise ValueError(f"DeviceTestMeter.update: {name} is a contiguous {dt} [N] on the logits' device")
        _score(logits, labels, self.acc, row_rank, row_nll)

    def result(self, process_group=None):
        """THE host read of a pass -> dict(samples, top1, top5, loss): top1 / top5 as fractions of the samples, loss = nll_sum / samples.
        With a process group the four sums are all-reduced once, as float64 (counts below 2^53 are exact) -- the reference's sum_tensor
        (utils/distributed.py:45-48) on its three counts (utils/meters.py:160-166)."""
        host = self.acc.cpu()
        sums = torch.tensor([float(v) for v in host[:3].tolist()] + [float(host[3:].view(torch.float64)[0])], dtype=torch.float64)
        if process_group is not None:
            import torch.distributed as dist
            sums = sums.to(self.device)
            dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=process_group)
            sums = sums.cpu()
        samples, top1, top5, nll = sums.tolist()
        n = samples if samples > 0 else float("nan")
        return dict(samples=int(samples), top1=top1 / n, top5=top5 / n, loss=nll / n)


class Evaler:
    """the reference's Evaler (evaler/evaler.py:11-58) over a loader that yields (input, target) already on the device (a
    PrefetchLoader): `evaler(epoch, model, amp_autocast=None)` -> (top1_acc, top5_acc); `evaler.last` holds the whole result
    (samples, top1, top5, loss).  No synchronisation and no host read inside the batch loop.

    graph=True: input and labels are copied into static buffers sized by the first batch, and forward plus scoring are captured once per
    (model, input shape) into a HIP graph and replayed for every batch, in this and later calls -- a captured forward reads the weights
    when it runs, so the graph follows training and `FlatSGD.ema_weights()`.  A smaller last batch is copied into the head of the buffers
    and the labels' tail set to -1: rows are independent in eval mode, so what the stale input tail computes is skipped.  A capture that
    fails falls back to eager batches and says so (`evaler.graph_note`).

    A short batch is scored at the first batch's size without a graph too (its tail: the rows of the latest full batch, labels -1).
    Rows of ONE batch size do not depend on their neighbours, bit for bit, but another batch size takes other kernels and tiles, and
    their rounding differs; so only by padding do eager and replayed passes give the same bits."""

    def __init__(self, loader, graph=False, process_group=None):
        self.loader, self.graph, self.process_group = loader, bool(graph), process_group
        self.last, self.graph_note = None, None
        self.meter = None  # the DeviceTestMeter of the last pass
        self._meters = {}  # device -> DeviceTestMeter
        self._graphs = {}  # (id(model), input shape, input dtype, device) -> [weakref(model), graph | None, static input, static labels]

    def _meter(self, device):
        m = self._meters.get(device)
        if m is None:
            m = self._meters[device] = DeviceTestMeter(device)
        return m

    def _captured(self, model, meter, x, y, full, autocast):
        """-> [weakref(model), graph or None, static input, static labels] for batches of `full` rows shaped like x, or None; the first
        full batch makes it: one eager forward (whatever a first call initialises must not happen while recording), then the capture"""
        key = (id(model), (full,) + tuple(x.shape[1:]), x.dtype, x.device)
        ent = self._graphs.get(key)
        if ent is not None and ent[0]() is model:
            return ent
        if x.shape[0] != full:
            return None
        sx, sy = x.clone(), y.clone()
        graph = torch.cuda.CUDAGraph()
        # (with a process group, the collectives' watchdog thread polls events while this thread records: bench.py, at its capture site)
        dist = torch.distributed
        mode = "thread_local" if (dist.is_available() and dist.is_initialized()) else "global"
        try:
            with autocast():
                model(sx)
            with torch.cuda.graph(graph, capture_error_mode=mode):
                with autocast():
                    out = model(sx)
                meter.update(out, sy)
        except Exception as e:  # the batches are then issued launch by launch
            graph = None
            self.graph_note = f"capture of forward + scoring failed ({type(e).__name__}: {str(e)[:160]}); eager batches"
            print(f"[evaler] {self.graph_note}", file=sys.stderr, flush=True)
            torch.cuda.synchronize(x.device)
        ent = self._graphs[key] = [weakref.ref(model), graph, sx, sy]
        return ent

    def __call__(self, epoch, model, amp_autocast=None):
        autocast = amp_autocast if amp_autocast is not None else contextlib.nullcontext
        was_training = model.training
        model.eval()
        meter = None
        try:
            with torch.no_grad():
                full = None     # the first batch's size: the static buffers'
                last_full = None  # the latest input of that size
                for x, y in self.loader:
                    if meter is None:
                        meter = self.meter = self._meter(x.device)
                        meter.reset()
                        full = x.shape[0]
                    n = x.shape[0]
                    ent = self._captured(model, meter, x, y, full, autocast) if (self.graph and _lib.DEVICE_ONLY and n <= full) else None
                    if ent is not None and ent[1] is not None:
                        ent[2][:n].copy_(x)
                        ent[3][:n].copy_(y)
                        if n < full:
                            ent[3][n:].fill_(-1)
                        ent[1].replay()
                    else:
                        if n < full and last_full is not None and x.shape[1:] == last_full.shape[1:] and x.dtype == last_full.dtype:
                            # the arithmetic of a forward depends on the batch size (other kernels, other tiles): a short batch is
                            # scored at the full size, as a replay scores it -- eager and replayed passes agree bit for bit
                            xp, yp = last_full.clone(), y.new_full((full,), -1)
                            xp[:n].copy_(x)
                            yp[:n].copy_(y)
                            x, y = xp, yp
                        with autocast():
                            out = model(x)
                        meter.update(out, y)
                    if n == full:
                        last_full = x
        finally:
            model.train(was_training)
        if meter is None:
            raise ValueError("Evaler: the loader yielded no batch")
        self.last = meter.result(self.process_group)
        return self.last["top1"], self.last["top5"]
