#!/usr/bin/env python
"""What the recipe's two new device passes cost on the MI355X, each against what a user had before them.

(i)  the loss: `soft_target_cross_entropy` forward + backward at B = 80, K = 1000, bf16 logits, against the torch composition it
     replaces -- two dense one-hot targets mixed as `mixup_target` does, `log_softmax`, product, sum, mean, autograd backward.
(ii) the input pass: `cot_mix_normalize` (mixup, CutMix and mode 0) at 80 x 3 x 224 x 224 uint8 -> bf16 against `cot_input_normalize`
     on the same buffers.  Bytes per pixel: 1 read + 2 written unmixed, 2 + 2 mixed, so a mixed pass that is purely HBM-bound takes
     4/3 of the unmixed one; the ratio measured against that is how far off the kernel is.  Inputs and outputs rotate through slots
     that together exceed the 256 MiB last-level cache, so every launch reads memory the cache no longer holds.

One repeat = `--iters` back-to-back calls of ONE form between two device events; the forms alternate repeat by repeat in one process;
the first `--warmup` repeats of each are dropped.  Per form: median and min-max over the repeats.  Writes profiles/recipe_loss_bench.log.

    python scripts/recipe_loss_bench.py [--repeats 40] [--iters 20]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from cotnet_amd import DeviceMixup, _lib, soft_target_cross_entropy  # noqa: E402
from cotnet_amd.input_pipeline import normalize_uint8  # noqa: E402
from cotnet_amd.mixup import pack_params  # noqa: E402


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters  # microseconds per call


def alternate(forms, repeats, warmup, iters):
    times = {k: [] for k in forms}
    for r in range(repeats + warmup):
        for k, fn in forms.items():
            t = timed(fn, iters)
            if r >= warmup:
                times[k].append(t)
    return times


def row(name, v):
    return f"{name:>34s} | median {statistics.median(v):9.2f} us  (min {min(v):9.2f}, max {max(v):9.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recipe_loss_bench.log"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the device"
    dev = torch.device("cuda:0")
    _lib.lib()
    lines = [f"# {torch.cuda.get_device_name(0)}; {args.repeats} repeats of {args.iters} calls per form (first {args.warmup} dropped), forms "
             "alternating; microseconds per call, device events"]

    # (i) loss forward + backward, B = 80, K = 1000, bf16
    B, K, lam, smoothing = 80, 1000, 0.37, 0.1
    g = torch.Generator(device=dev).manual_seed(1)
    logits = (3 * torch.randn(B, K, device=dev, generator=g)).bfloat16().requires_grad_(True)
    labels = torch.randint(0, K, (B,), device=dev, generator=g)
    mix = DeviceMixup(device=dev)
    mix.write(pack_params(1, lam))

    def ours(_):
        logits.grad = None
        soft_target_cross_entropy(logits, labels, mix, smoothing).backward()

    def composed(_):
        logits.grad = None
        off = smoothing / K
        on = 1. - smoothing + off
        y1 = torch.full((B, K), off, device=dev).scatter_(1, labels.view(-1, 1), on)
        y2 = torch.full((B, K), off, device=dev).scatter_(1, labels.flip(0).view(-1, 1), on)
        target = y1 * lam + y2 * (1. - lam)
        torch.sum(-target * torch.nn.functional.log_softmax(logits.float(), dim=-1), dim=-1).mean().backward()

    ours(0), composed(0)
    torch.cuda.synchronize()
    a, b = logits.grad.clone(), None
    composed(0)
    b = logits.grad.clone()
    lines.append(f"(i) loss forward + backward, B = {B}, K = {K}, bf16 logits (host launches included: eager calls, as a training loop issues them); "
                 f"largest gradient difference between the two forms {float((a.float() - b.float()).abs().max()):.3e}")
    t = alternate({"soft_target_cross_entropy": ours, "torch composition": composed}, args.repeats, args.warmup, args.iters)
    lines += [row(k, v) for k, v in t.items()]
    lines.append(f"{'ratio of medians (torch / ours)':>34s} | {statistics.median(t['torch composition']) / statistics.median(t['soft_target_cross_entropy']):.2f}")
    # the same two in captured graphs: device time without the host's launch cost
    graphs = {}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for name, fn in (("soft_target_cross_entropy", ours), ("torch composition", composed)):
            fn(0)
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=s):
                fn(0)
            graphs[name + " (graph replay)"] = (lambda _, gr=gr: gr.replay())
        t = alternate(graphs, args.repeats, args.warmup, args.iters)
    torch.cuda.current_stream().wait_stream(s)
    lines += [row(k, v) for k, v in t.items()]
    lines.append(f"{'ratio of medians (torch / ours)':>34s} | "
                 f"{statistics.median(t['torch composition (graph replay)']) / statistics.median(t['soft_target_cross_entropy (graph replay)']):.2f}")

    # (ii) input pass, 80 x 3 x 224 x 224 -> bf16
    shape = (80, 3, 224, 224)
    n = 80 * 3 * 224 * 224
    slots = 10  # 10 x (12 MB in + 24 MB out) = 361 MB: beyond the 256 MiB cache
    xs = [torch.randint(0, 256, shape, device=dev, dtype=torch.uint8, generator=g) for _ in range(slots)]
    ys = [torch.empty(shape, device=dev, dtype=torch.bfloat16) for _ in range(slots)]
    mean = torch.tensor([123.675, 116.28, 103.53], device=dev)
    std = torch.tensor([58.395, 57.12, 57.375], device=dev)
    blocks = {"mix mode 1 (mixup)": pack_params(1, lam).to(dev), "mix mode 2 (CutMix 112 x 112)": pack_params(2, 0.75, (50, 162, 37, 149)).to(dev),
              "mix mode 0": pack_params(0, 1.).to(dev)}
    forms = {"cot_input_normalize": lambda i: normalize_uint8(xs[i % slots], mean, std, torch.bfloat16, out=ys[i % slots])}
    for k, blk in blocks.items():
        forms[k] = (lambda i, blk=blk: mix.mix_normalize(xs[i % slots], mean, std, torch.bfloat16, out=ys[i % slots], block=blk))
    t = alternate(forms, args.repeats, args.warmup, args.iters)
    base = statistics.median(t["cot_input_normalize"])
    lines.append(f"(ii) input pass, {shape} uint8 -> bf16, {slots} rotating slots")
    for k, v in t.items():
        mixed = k in ("mix mode 1 (mixup)", "mix mode 2 (CutMix 112 x 112)")
        nbytes = n * (4 if mixed else 3)
        med = statistics.median(v)
        lines.append(row(k, v) + f" | {nbytes / med / 1e6:6.2f} TB/s | x{med / base:.3f} of cot_input_normalize (bytes alone: x{nbytes / (3 * n):.3f})")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
