#!/usr/bin/env python
"""What reading the rate from device memory costs the fused SGD kernel: `cot_sgd_step` (rate by value) against `cot_sgd_step_lr`
(one dependent scalar load in front of the loop) at CoTNet-50's actual bucket sizes, straight through the C ABI.

The bucket sizes come from a FlatSGD built on `cotnet50` in mixed precision (no forward is run).  Per bucket the operands are slots
of four pools that together exceed the 256 MiB last-level cache several times over; the launches walk the slots in order and wrap,
so every launch reads memory the cache no longer holds.  One repeat = `--iters` back-to-back launches of ONE form between two HIP
events; the forms alternate repeat by repeat in one process; the first `--warmup` repeats of each are dropped.  Per form: median and
min-max of the repeats, and the ratio of the medians.  Writes profiles/sgd_device_lr_ab.log.

    python scripts/sgd_device_lr_ab.py [--repeats 40] [--iters 20]
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import cotnet_amd  # noqa: E402
from cotnet_amd import _lib  # noqa: E402
from cotnet_amd.flat_sgd import FlatSGD, to_mixed_bf16  # noqa: E402

POOL_BYTES = 1 << 30  # all four pools together: four times the 256 MiB cache


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sgd_device_lr_ab.log"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the device"
    assert args.repeats >= 30
    dev = torch.device("cuda:0")
    L = _lib.api()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    opt = FlatSGD(to_mixed_bf16(cotnet_amd.create_model("cotnet50", num_classes=1000).to(dev)), lr=0.25, momentum=0.9,
                  weight_decay=4e-5, device_lr=True)
    buckets = [(b.key, b.pflat.dtype, opt.reducer.reduced(b).dtype, b.pflat.numel()) for b in opt.reducer.buckets]
    rate = opt.lr_dev
    del opt
    lines = [f"# {torch.cuda.get_device_name(0)}; {args.repeats} repeats of {args.iters} launches per form (first {args.warmup} dropped), "
             f"forms alternating, operands rotating through {POOL_BYTES >> 20} MiB; microseconds per launch",
             f"{'bucket':>26s} {'elements':>9s} | {'by value: median (min-max)':>30s} | {'from memory: median (min-max)':>30s} | ratio | inside"]
    print(lines[0], lines[1], sep="\n", flush=True)
    for key, pdt, gdt, n in buckets:
        pe, ge = torch.empty((), dtype=pdt).element_size(), torch.empty((), dtype=gdt).element_size()
        has_master = pdt != torch.float32
        stride = (n + 63) // 64 * 64  # elements between slots: every slot of every pool stays 16-byte aligned
        per_slot = stride * (pe + ge + 4 + (4 if has_master else 0))
        slots = max(2, POOL_BYTES // per_slot)
        param = torch.randn(slots * stride, device=dev).to(pdt)
        grad = (torch.randn(slots * stride, device=dev) * 1e-3).to(gdt)
        mom = torch.zeros(slots * stride, device=dev)
        master = param.float() if has_master else None
        pc, gc = _lib.dtype_code(pdt), _lib.dtype_code(gdt)
        slot = [0]

        def launch(form):
            k = slot[0] % slots
            slot[0] += 1
            args_ = (param.data_ptr() + k * stride * pe, master.data_ptr() + k * stride * 4 if has_master else None,
                     mom.data_ptr() + k * stride * 4, grad.data_ptr() + k * stride * ge, n)
            if form == 0:
                L.cot_sgd_step(*args_, 0.25, 0.9, 4e-5, 1.0, 1, pc, gc, stream)
            else:
                L.cot_sgd_step_lr(*args_, rate.data_ptr(), 0.9, 4e-5, 1.0, 1, pc, gc, stream)

        def repeat(form):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.iters):
                launch(form)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / args.iters * 1e3

        us = ([], [])
        for r in range(args.warmup + args.repeats):
            for form in ((0, 1) if r % 2 == 0 else (1, 0)):
                t = repeat(form)
                if r >= args.warmup:
                    us[form].append(t)
        med = [statistics.median(u) for u in us]
        inside = min(us[0]) <= med[1] <= max(us[0])
        row = (f"{key + ' ' + str(pdt)[6:] + '/' + str(gdt)[6:]:>26s} {n:9d} | "
               + " | ".join(f"{m:12.2f} ({min(u):7.2f}-{max(u):7.2f})" for m, u in zip(med, us))
               + f" | {med[1] / med[0]:5.3f} | {'yes' if inside else 'NO'}")
        print(row, flush=True)
        lines.append(row)
        del param, grad, mom, master
        torch.cuda.empty_cache()
    lines.append("# inside: the from-memory median lies within the by-value form's own min-max")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
