#!/usr/bin/env python
"""What scoring a validation batch costs on the MI355X: `cot_eval_score` (DeviceTestMeter.update, two launches) at N = 128, K = 1000, bf16
logits against the torch composition it replaces -- the reference's `accuracy` (`topk(5)`, transpose, `eq`, two sums;
utils/meters.py:12-19) plus `F.cross_entropy(reduction='sum')`, the counts and the loss added to device tensors -- BOTH recorded into a
HIP graph and replayed, so that the host's launch cost is out of the figure (a validation pass replays them behind the forward).

One repeat = `--iters` back-to-back replays of ONE form between two device events; the forms alternate repeat by repeat in one process;
the first `--warmup` repeats of each are dropped.  Per form: median and min-max over the repeats, microseconds per batch.

    python scripts/eval_score_bench.py [--repeats 40] [--iters 50] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from cotnet_amd import DeviceTestMeter, _lib  # noqa: E402


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters  # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the device"
    dev = torch.device("cuda:0")
    _lib.lib()
    N, K = args.batch, 1000
    g = torch.Generator(device=dev).manual_seed(1)
    logits = (3 * torch.randn(N, K, device=dev, generator=g)).bfloat16()
    labels = torch.randint(0, K, (N,), device=dev, generator=g)
    logits[torch.arange(0, N, 3, device=dev), labels[::3]] += 9.0
    meter = DeviceTestMeter(dev)
    counts, loss = torch.zeros(2, device=dev), torch.zeros((), device=dev, dtype=torch.float64)

    def ours():
        meter.update(logits, labels)

    def composed():
        _, pred = logits.topk(5, 1, True, True)
        correct = pred.t().eq(labels.reshape(1, -1).expand(5, N))
        counts[0] += correct[:1].reshape(-1).float().sum(0)
        counts[1] += correct[:5].reshape(-1).float().sum(0)
        loss.add_(torch.nn.functional.cross_entropy(logits.float(), labels, reduction="sum"))

    graphs = {}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for name, fn in (("cot_eval_score", ours), ("torch composition", composed)):
            fn()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=s):
                fn()
            graphs[name] = gr
        meter.reset(), counts.zero_(), loss.zero_()
        graphs["cot_eval_score"].replay(), graphs["torch composition"].replay()
        torch.cuda.synchronize()
        r = meter.result()
        same = (r["top1"] * N, r["top5"] * N) == tuple(counts.tolist())
        lines = [f"# {torch.cuda.get_device_name(0)}; N = {N}, K = {K}, bf16 logits; {args.repeats} repeats of {args.iters} graph replays per form "
                 f"(first {args.warmup} dropped), forms alternating; microseconds per batch, device events",
                 f"# one batch: top-1 / top-5 hits {r['top1'] * N:.0f} / {r['top5'] * N:.0f}, the composition's {counts.tolist()} (equal: {same}); "
                 f"loss {r['loss']:.9f} against the composition's fp32 {float(loss) / N:.9f}"]
        times = {k: [] for k in graphs}
        for rep in range(args.repeats + args.warmup):
            for k, gr in graphs.items():
                t = timed(gr.replay, args.iters)
                if rep >= args.warmup:
                    times[k].append(t)
    torch.cuda.current_stream().wait_stream(s)
    for k, v in times.items():
        lines.append(f"{k:>20s} | median {statistics.median(v):8.2f} us  (min {min(v):8.2f}, max {max(v):8.2f})")
    lines.append(f"{'torch / ours':>20s} | {statistics.median(times['torch composition']) / statistics.median(times['cot_eval_score']):.2f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
