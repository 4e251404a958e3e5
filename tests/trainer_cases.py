"""cotnet_amd.trainer over the real pieces: the cases that tests/test_trainer_gpu.py runs on the device (replayed) and
tests/test_trainer_emulated.py on the host emulator (where `graph=True` finds no GPU and steps eagerly: the loop's order, the resume and
the meter are checked there, the replay only on the device).

Every comparison is BIT FOR BIT (torch.equal).  The model is tests/adamw_cases.small()'s kind on the flattened image -- a matrix, a bias
and BatchNorm vectors: both decay groups, buffers, bf16 and fp32 buckets -- because its torch operators are reproducible on the device
(adamw_cases.small records why torch convolutions are not); `runs()` asserts that first, on two identical hand-written loops.

Shapes: N = 4 images of 3 x 16 x 32 uint8, five batches per epoch of which the last has 2 rows, log_interval 2, warm-up 2.  So in the
first epoch batches 0 and 1 are eager, batch 2 is captured and replayed, 3 is replayed and 4 (short) is eager; later epochs replay four
and step the short one eagerly.

`hand_loop` is the reference's train.py:243-364 written out with the existing pieces -- and with `loss.item()` per step: the loop the
meter's figures are compared against."""
import functools
import os

import numpy as np
import torch
from torch import nn

from cotnet_amd import CheckpointSaver, DeviceMixup, Evaler, FlatAdamW, MixedSoftTargetCrossEntropy, Trainer
from cotnet_amd.flat_sgd import FlatSGD, to_mixed_bf16
from cotnet_amd.input_pipeline import IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD, PrefetchLoader
from cotnet_amd.lr_schedule import CosineSchedule

N, SHORT, IMG, CLASSES = 4, 2, (3, 16, 32), 16
BATCHES, LOG_INTERVAL, WARMUP = 5, 2, 2
SIZES = [N] * (BATCHES - 1) + [SHORT]
MIX = dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.8, switch_prob=0.5, label_smoothing=0.1, num_classes=CLASSES)
SEED = 20
COMMON = dict(device_lr=True, clip_grad=0.5, skip_nonfinite=True, ema_decay=0.9, lookahead_k=3)
OPTIMIZERS = {"sgd": lambda m: FlatSGD(m, lr=0.05, momentum=0.9, weight_decay=4e-5, nesterov=True, **COMMON),
              "adamw": lambda m: FlatAdamW(m, lr=2e-3, weight_decay=0.05, **COMMON)}
BASE_LR = {"sgd": 0.05, "adamw": 2e-3}


def host_batches(seed=1):
    """what a host DataLoader with fast_collate yields: uint8 images and integer labels on the CPU"""
    g = torch.Generator().manual_seed(seed)
    return [(torch.randint(0, 256, (n,) + IMG, generator=g, dtype=torch.uint8), torch.randint(0, CLASSES, (n,), generator=g)) for n in SIZES]


class HostLoader:
    """the emulator's stand-in for PrefetchLoader (which needs streams): the same draw per batch in the same order, the same two
    library calls, `mixup_enabled` and `len`"""

    def __init__(self, batches, mixup, dtype):
        self.batches, self.mixup, self.dtype = batches, mixup, dtype
        self.mean = torch.tensor([v * 255 for v in IMAGENET_DEFAULT_MEAN], dtype=torch.float32)
        self.std = torch.tensor([v * 255 for v in IMAGENET_DEFAULT_STD], dtype=torch.float32)

    mixup_enabled = PrefetchLoader.mixup_enabled

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        for x, y in self.batches:
            self.mixup.draw(x.shape)
            yield self.mixup.mix_normalize(x.contiguous(), self.mean, self.std, self.dtype), y


def train_loader(dev, mix):
    if torch.device(dev).type == "cuda":
        return PrefetchLoader(host_batches(), dtype=torch.bfloat16, device=dev, mixup=mix)
    return HostLoader(host_batches(), mix, torch.bfloat16)


def eval_batches(dev, seed=2):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn((N,) + IMG, generator=g).bfloat16().to(dev), torch.randint(0, CLASSES, (N,), generator=g).to(dev)) for _ in range(2)]


def make_model(dev, seed=0):
    torch.manual_seed(seed)
    m = nn.Sequential(nn.Flatten(), nn.Linear(IMG[0] * IMG[1] * IMG[2], CLASSES), nn.BatchNorm1d(CLASSES)).to(dev).train()
    return to_mixed_bf16(m)


class Rig:
    """one model with everything around it: optimizer, mixup, loss, loaders, schedule, evaler"""

    def __init__(self, dev, kind, epochs, seed=0, np_seed=SEED):
        np.random.seed(np_seed)  # the mixup draws
        torch.manual_seed(np_seed)
        self.dev, self.kind, self.epochs = dev, kind, epochs
        self.model = make_model(dev, seed)
        self.opt = OPTIMIZERS[kind](self.model)
        assert {b.key for b in self.opt.reducer.buckets} == {"decay", "no_decay"}
        self.mix = DeviceMixup(device=dev, **MIX)
        self.draws = []
        sample = self.mix.sample

        def logged(shape):
            out = sample(shape)
            self.draws.append(out)
            return out
        self.mix.sample = logged
        self.loss_fn = MixedSoftTargetCrossEntropy(self.mix)
        self.loader = train_loader(dev, self.mix)
        self.evaler = Evaler(eval_batches(dev), graph=False)
        # per update: three warm-up steps, then the cosine over the updates of three epochs (every step trains at another rate)
        self.schedule = CosineSchedule(BASE_LR[kind], 3 * BATCHES, warmup_t=3, warmup_lr_init=1e-4, lr_min=1e-5)

    def trainer(self, graph, tmp_path=None, epochs=None):
        saver = None
        if tmp_path is not None:
            os.makedirs(str(tmp_path), exist_ok=True)
            saver = CheckpointSaver(self.model, self.opt, checkpoint_dir=str(tmp_path), recovery_dir=str(tmp_path), rng=True)
        return Trainer(self.model, self.opt, self.loss_fn, self.loader, num_epochs=self.epochs if epochs is None else epochs,
                       evaler=self.evaler, saver=saver, schedule=self.schedule, schedule_unit="update", log_interval=LOG_INTERVAL, graph=graph)

    def state(self):
        d = {"param " + n: p.detach() for n, p in self.model.named_parameters()}
        d.update({"buffer " + n: b for n, b in self.model.named_buffers()})  # running_mean, running_var, num_batches_tracked
        for i, st in enumerate(self.opt.state):  # master, momentum / moments, ema, slow
            d.update({f"opt.state[{i}][{k}]": v for k, v in st.items() if v is not None})
        d.update({f"opt._buf_ema[{i}]": b for i, b in enumerate(self.opt._buf_ema)})
        d.update(clip_state=self.opt.clip_state, lookahead_state=self.opt.lookahead_state, lr_dev=self.opt.lr_dev, mix_params=self.mix.params)
        if hasattr(self.opt, "adam_state"):
            d["adam_state"] = self.opt.adam_state
        return {k: v.detach().clone().cpu() for k, v in d.items()}


def hand_loop(rig):
    """-> (history, per-step losses per epoch): train.py:243-364 with the existing pieces, eager, `.item()` per step"""
    model, opt, sched = rig.model, rig.opt, rig.schedule
    sched.apply(opt, 0)
    history, losses = [], []
    for epoch in range(rig.epochs):
        model.train()
        num_updates = epoch * len(rig.loader)
        losses.append([])
        for x, y in rig.loader:
            sched.apply(opt, num_updates)
            opt.zero_grad()
            loss = rig.loss_fn(model(x), y)
            loss.backward()
            opt.step()
            num_updates += 1
            losses[-1].append(loss.item())
        opt.sync_lookahead()
        top1, top5 = rig.evaler(epoch, model)
        row = dict(epoch=epoch, lr=opt.lr, top1=top1, top5=top5, loss=rig.evaler.last["loss"])
        with opt.ema_weights():
            top1, top5 = rig.evaler(epoch, model)
        row.update(ema_top1=top1, ema_top5=top5, ema_loss=rig.evaler.last["loss"])
        history.append(row)
    return history, losses


def same(a, b, what):
    assert a.keys() == b.keys(), (what, sorted(set(a) ^ set(b)))
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, f"{what}: {len(bad)} of {len(a)} tensors differ, first {bad[:4]}"


def reference_figures(losses):
    """what the reference's meters give over one epoch's `.item()` losses: (the window means it logs, loss_total / num_samples) --
    deque(maxlen=log_interval) + np.mean (utils/meters.py:62-81), Python-float sums (:117-118), a line when (it + 1) % log_interval == 0"""
    from collections import deque
    window, total, samples, means = deque(maxlen=LOG_INTERVAL), 0.0, 0, []
    for it, (v, mb) in enumerate(zip(losses, SIZES)):
        window.append(v)
        total += v * mb
        samples += mb
        if (it + 1) % LOG_INTERVAL == 0:
            means.append(float(np.mean(window)))
    return means, total / samples


def fit_logged(trainer, **kw):
    """trainer.fit() -> (history, the `loss` of every line the meter logged)"""
    means = []
    stats = trainer.meter.get_iter_stats

    def logged(epoch, it):
        out = stats(epoch, it)
        means.append(out["loss"])
        return out
    trainer.meter.get_iter_stats = logged
    return trainer.fit(**kw), means


@functools.lru_cache(maxsize=None)
def runs(dev, kind, epochs):
    """the four runs every comparison shares, computed once: the hand-written loop twice (the model's eager steps must be reproducible:
    asserted here, before anything is compared with them), Trainer(graph=False) and Trainer(graph=True)"""
    out = {}
    for name in ("hand", "hand again"):
        rig = Rig(dev, kind, epochs)
        history, losses = hand_loop(rig)
        out[name] = dict(rig=rig, state=rig.state(), history=history, losses=losses)
    same(out["hand"]["state"], out["hand again"]["state"], "two identical eager runs (the model is not reproducible: nothing below means anything)")
    assert out["hand"]["losses"] == out["hand again"]["losses"]
    for name, graph in (("eager", False), ("replayed", True)):
        rig = Rig(dev, kind, epochs)
        t = rig.trainer(graph)
        history, means = fit_logged(t)
        out[name] = dict(rig=rig, trainer=t, state=rig.state(), history=history, means=means)
    return out


def check_trainer_equals_the_hand_written_loop(dev, kind, epochs, on_gpu):
    r = runs(dev, kind, epochs)
    hand, eager, replayed = r["hand"], r["eager"], r["replayed"]
    flat = [v for e in hand["losses"] for v in e]
    assert len(flat) == epochs * BATCHES and len(set(flat)) == len(flat) and all(np.isfinite(flat)), flat  # (the steps do differ)
    same(hand["state"], eager["state"], "the hand-written loop vs Trainer(graph=False)")
    same(eager["state"], replayed["state"], "Trainer(graph=False) vs Trainer(graph=True)")
    assert eager["history"] == replayed["history"], (eager["history"], replayed["history"])
    for h, t in zip(hand["history"], replayed["history"]):
        assert all(t[k] == v for k, v in h.items()), (h, t)
    # who stepped what
    step = replayed["trainer"].step
    assert eager["trainer"].step.replays == 0 and eager["trainer"].step.steps == epochs * BATCHES == step.steps
    if on_gpu:
        assert step.graph and step.graph_note is None, step.graph_note
        assert step.replays == epochs * (BATCHES - 1) - WARMUP, "every full batch behind the warm-up is a replay; the short ones are eager"
    else:
        assert not step.graph and step.replays == 0 and "not on a GPU" in step.graph_note
    # everything was on
    stats = replayed["rig"].opt.clip_stats()
    assert stats["steps"] == epochs * BATCHES and stats["clipped"] > 0 and stats["skipped"] == 0, stats
    look = replayed["rig"].opt.lookahead_stats()
    assert look["step"] == epochs * BATCHES and look["syncs"] >= (epochs * BATCHES) // 3 and look["born"] == 1, look
    modes = {0 if lam == 1. else (2 if cut else 1) for lam, cut, _ in replayed["rig"].draws}
    assert modes == {0, 1, 2} or epochs == 1, modes  # unmixed, mixup and CutMix batches all went through the one capture
    assert replayed["rig"].draws == hand["rig"].draws and len(hand["rig"].draws) == epochs * BATCHES
    assert len({h["lr"] for h in replayed["history"]}) == epochs  # the per-update schedule reached the steps


def check_meter_against_item_per_step(dev, kind, epochs):
    """the logged window means and the epoch's loss_avg against the reference's meters fed with `loss.item()` per step"""
    r = runs(dev, kind, epochs)
    want_means, want_avg = [], []
    for e in r["hand"]["losses"]:
        means, avg = reference_figures(e)
        want_means += means
        want_avg.append(avg)
    for name in ("eager", "replayed"):
        assert r[name]["means"] == want_means, (name, r[name]["means"], want_means)  # equal, not close
        assert [h["train_loss"] for h in r[name]["history"]] == want_avg, (name, want_avg)
        assert [(h["updates"], h["samples"]) for h in r[name]["history"]] == [(BATCHES, sum(SIZES))] * epochs
        lines = epochs * (BATCHES // LOG_INTERVAL)
        assert len(want_means) == lines and r[name]["trainer"].meter.host_reads == lines + epochs, r[name]["trainer"].meter.host_reads


def check_resume(dev, kind, tmp_path, on_gpu):
    """three epochs uninterrupted against two epochs, then `fit(resume=<the last checkpoint>)` for the third in a fresh model, optimizer
    and trainer whose step was CAPTURED BEFORE the resume, on its own weights: every load is in place, so the replays train the resumed
    state.  The file carries the generators (rng=True): the third epoch draws the uninterrupted run's mixup parameters."""
    a = Rig(dev, kind, 3)
    ha = a.trainer(True, tmp_path / "a").fit()
    b = Rig(dev, kind, 3)
    hb = b.trainer(True, tmp_path / "b", epochs=2).fit()
    assert hb == ha[:2]
    path = tmp_path / "b" / "checkpoint-2.pth.tar"
    file = torch.load(str(path), map_location="cpu", weights_only=False)
    assert file["epoch"] == 2 and set(file["rng"]) >= {"torch_cpu", "numpy"} and "state_dict_ema" in file
    c = Rig(dev, kind, 3, seed=7, np_seed=99)  # other weights, other draws: a new process starts anywhere
    assert not torch.equal(c.model[1].weight, a.model[1].weight)
    t = c.trainer(True, tmp_path / "c")
    g = torch.Generator().manual_seed(5)
    for _ in range(WARMUP + 1):  # warm up and capture on C's own weights, on batches of the loader's shape that nobody else sees
        t.step(torch.randn((N,) + IMG, generator=g).bfloat16().to(dev), torch.randint(0, CLASSES, (N,), generator=g).to(dev))
    assert t.step.replays == (1 if on_gpu else 0) and not c.draws
    addresses = {k: v.data_ptr() for k, v in [("lr_dev", c.opt.lr_dev), ("clip", c.opt.clip_state)] + list(c.model.named_parameters())}
    hc = t.fit(resume=str(path))
    assert addresses == {k: v.data_ptr() for k, v in [("lr_dev", c.opt.lr_dev), ("clip", c.opt.clip_state)] + list(c.model.named_parameters())}
    assert [h["epoch"] for h in hc] == [2]
    if on_gpu:
        assert t.step.replays == 1 + (BATCHES - 1), "the resumed epoch was replayed from the capture made before the load"
    same(a.state(), c.state(), "uninterrupted vs resumed")
    best = ("best_metric", "best_epoch")  # (the resumed run's saver has seen one epoch; the reference does not restore it either)
    assert {k: v for k, v in hc[-1].items() if k not in best} == {k: v for k, v in ha[-1].items() if k not in best}, (hc[-1], ha[-1])
    assert hc[-1]["best_metric"] == hc[-1]["ema_top1"] and ha[-1]["best_metric"] == max(h["ema_top1"] for h in ha)
    assert c.draws == a.draws[2 * BATCHES:] and len(c.draws) == BATCHES, "the third epoch's mixup draws"
    assert a.draws[2 * BATCHES:] != a.draws[BATCHES:2 * BATCHES]
    assert a.opt.clip_stats() == c.opt.clip_stats() and a.opt.lookahead_stats() == c.opt.lookahead_stats()

