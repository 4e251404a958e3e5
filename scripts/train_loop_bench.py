"""What does the loop cost?  CoTNet-50 at 224^2, B = 80, mixed bf16, the recipe switches of `bench.py --recipe` (head dropout 0.25,
stochastic depth 0.1, EMA 0.9999, SGD-nesterov at 0.25 * B / 640), trained by cotnet_amd.trainer: PrefetchLoader with a DeviceMixup over a
synthetic uint8 loader that stays on the device, the soft-target loss, a per-update cosine schedule through `device_lr=True`, TrainMeter at
log_interval 50, the step replayed from one HIP graph.

Reported: steady-state images/s of whole epochs as `train_epoch` runs them with the Trainer's own step and meter -- wall time from the
call to the end-of-epoch host read, which waits for the training stream.  The first `--settle-epochs` epochs are not timed: they hold the
warm-up steps and the capture, and a fresh box runs its first seconds of sustained load slower (bench.py settles for the same reason).

Against `bench.py --recipe` of the same session (`--bench-json`: the file holding its JSON line), the loop ADDS per step: the uint8 ->
bf16 mix-normalise pass, the copy of the batch into the static buffers, the soft-target loss in place of F.cross_entropy, one fill of the
rate, one 32-byte copy of the mixup draw, six scalar launches of the meter.

    python bench.py --gpus 1 --steps 200 --warmup 20 --recipe > bench_recipe.json
    python scripts/train_loop_bench.py --bench-json bench_recipe.json --decompose 100

`--decompose K` says where a step's time goes and `--pad-streams N` moves the loader's per-epoch side stream among the hardware queues;
profiles/train_loop_bench.log holds both figures, their ratio and what these two options found.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class SyntheticLoader:
    """`steps` batches per epoch out of four uint8 batches that live on the device (PrefetchLoader's `.to(device)` is then no copy)"""

    def __init__(self, steps, batch, img, device):
        g = torch.Generator(device=device).manual_seed(7)
        self.steps = steps
        self.images = [torch.randint(0, 256, (batch, 3, img, img), device=device, generator=g, dtype=torch.uint8) for _ in range(4)]
        self.labels = [torch.randint(0, 1000, (batch,), device=device, generator=g) for _ in range(4)]

    def __len__(self):
        return self.steps

    def __iter__(self):
        for i in range(self.steps):
            yield self.images[i % 4], self.labels[i % 4]


def decompose(K, trainer, loader, schedule, mix, t):
    """ms per step of (a) the captured step replayed back to back, (b) the same with the loop's own device work in front of each replay
    (the rate's fill, the 32-byte draw, the batch copied into the static buffers), (c) the same as (a) with the host waiting 100 / 200 /
    400 us in front of each replay -- does host time between two replays show in the step? --, each twice, alternating; and (d) the
    host's own time per phase of a loop written out like train_epoch (loader, schedule, step call, meter)"""
    from cotnet_amd.cot_layer_fused import invalidate_packs
    step, opt, meter = trainer.step, trainer.optimizer, trainer.meter
    graph, (sx, sy) = step._graph, step._static
    x, y, block = sx.clone(), sy.clone(), mix.params.clone()

    def run(between):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(K):
            between()
            graph.replay()
            invalidate_packs()
        torch.cuda.synchronize()
        return round(1e3 * (time.perf_counter() - t0) / K, 4)

    def device_work():
        opt.set_lr(opt.lr)
        mix.params.copy_(block, non_blocking=True)
        sx.copy_(x)
        sy.copy_(y)

    def wait(us):
        def fn():
            end = time.perf_counter() + us * 1e-6
            while time.perf_counter() < end:
                pass
        return fn
    forms = {"replay_only": lambda: None, "replay_and_device_work": device_work, "replay_and_host_wait_100us": wait(100),
             "replay_and_host_wait_200us": wait(200), "replay_and_host_wait_400us": wait(400)}
    out = {k: [] for k in forms}
    with step.stream_context():
        for _ in range(2):
            for k, fn in forms.items():
                out[k].append(run(fn))
        host = dict(loader=0.0, schedule=0.0, step=0.0, meter=0.0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mark = [t0]

        def lap(phase):
            now = time.perf_counter()
            host[phase] += now - mark[0]
            mark[0] = now
        for i, (xb, yb) in enumerate(loader):
            lap("loader")
            schedule.apply(opt, t + i)
            lap("schedule")
            step(xb, yb)
            lap("step")
            meter.lr = str([opt.lr])
            meter.log_iter_stats(0, i)
            lap("meter")
        torch.cuda.synchronize()
        out["probe_epoch_ms_per_step"] = round(1e3 * (time.perf_counter() - t0) / len(loader), 4)
        out["host_us_per_step"] = {k: round(1e6 * v / len(loader), 1) for k, v in host.items()}
        meter.reset()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=80)
    ap.add_argument("--img", type=int, default=224)
    ap.add_argument("--steps", type=int, default=200, help="batches per epoch")
    ap.add_argument("--settle-epochs", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=3, help="timed epochs")
    ap.add_argument("--log-interval", type=int, default=50)
    ap.add_argument("--eager", action="store_true", help="Trainer(graph=False): every step issued launch by launch")
    ap.add_argument("--pad-streams", type=int, default=0, metavar="N",
                    help="take N idle streams from torch's pool in front of every epoch (PrefetchLoader takes a fresh side stream per "
                         "epoch; with N = 3 every epoch's lands on the same hardware queue of four)")
    ap.add_argument("--decompose", type=int, default=0, metavar="K",
                    help="after the timed epochs: where a step's time goes -- K replays of the loop's own graph back to back, with the "
                         "loop's device work between them, with a host wait between them, and the host's time per phase of the loop")
    ap.add_argument("--bench-json", default=None, help="file with the JSON line of `bench.py --recipe` from the same session")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_loop_bench.py needs an MI355X; there is no CPU path")

    import cotnet_amd
    from cotnet_amd import DeviceMixup, MixedSoftTargetCrossEntropy, Trainer, train_epoch
    from cotnet_amd.flat_sgd import FlatSGD, to_mixed_bf16
    from cotnet_amd.input_pipeline import PrefetchLoader
    from cotnet_amd.lr_schedule import CosineSchedule

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(1234)
    np.random.seed(1234)
    B, total = args.batch, args.settle_epochs + args.epochs
    model = to_mixed_bf16(cotnet_amd.create_model("cotnet50", num_classes=1000, drop_rate=0.25, drop_path_rate=0.1).to(dev)).train()
    lr = 0.25 * B / 640.0
    opt = FlatSGD(model, lr=lr, momentum=0.9, weight_decay=4e-5, nesterov=True, bucket_mb=25.0, ema_decay=0.9999, device_lr=True)
    mix = DeviceMixup(mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, label_smoothing=0.1, num_classes=1000, device=dev)
    loader = PrefetchLoader(SyntheticLoader(args.steps, B, args.img, dev), dtype=torch.bfloat16, device=dev, mixup=mix)
    schedule = CosineSchedule(lr, total * args.steps, warmup_t=args.steps, warmup_lr_init=1e-4, lr_min=1e-5)
    trainer = Trainer(model, opt, MixedSoftTargetCrossEntropy(mix), loader, num_epochs=total, schedule=schedule, schedule_unit="update",
                      log_interval=args.log_interval, graph=not args.eager)
    step, meter = trainer.step, trainer.meter
    epochs = []
    with step.stream_context():
        schedule.apply(opt, 0)
        meter.reset(timer=True)
        for epoch in range(total):
            torch.cuda.synchronize()
            idle = [torch.cuda.Stream(device=dev) for _ in range(args.pad_streams)]
            for s in idle:  # (a stream gets its hardware queue at its first launch)
                with torch.cuda.stream(s):
                    torch.zeros(1, device=dev)
            replays = step.replays
            t0 = time.perf_counter()
            out = train_epoch(epoch, model, loader, step, opt, meter=meter, schedule=schedule, schedule_unit="update")
            dt = time.perf_counter() - t0  # (the end-of-epoch read has waited for the training stream)
            epochs.append(dict(epoch=epoch, timed=epoch >= args.settle_epochs, seconds=round(dt, 4), images_per_s=round(out["samples"] / dt, 1),
                               ms_per_step=round(1e3 * dt / out["updates"], 3), replays=step.replays - replays, loss_avg=out["loss_avg"]))
            print(f"[train_loop_bench] {epochs[-1]}", file=sys.stderr, flush=True)
    timed = [e for e in epochs if e["timed"]]
    rate = sum(args.steps * B for _ in timed) / sum(e["seconds"] for e in timed)
    line = {"metric": "train_loop_images_per_s", "value": round(rate, 1), "ms_per_step": round(1e3 * B / rate, 3), "batch": B, "img": args.img,
            "steps_per_epoch": args.steps, "log_interval": args.log_interval, "graph": bool(step.graph and step.graph_note is None),
            "graph_note": step.graph_note, "host_reads": meter.host_reads, "epochs": epochs}
    if args.decompose and line["graph"]:
        line["decompose"] = decompose(args.decompose, trainer, loader, schedule, mix, total * args.steps)
    if args.bench_json:
        with open(args.bench_json) as fh:
            bench = [json.loads(row) for row in fh if row.lstrip().startswith("{")][-1]
        value = bench.get("value", bench.get("images_per_s"))
        line["bench_recipe_images_per_s"] = value
        line["ratio_loop_over_bench"] = round(rate / value, 4) if value else None
    print(json.dumps(line))


if __name__ == "__main__":
    main()
