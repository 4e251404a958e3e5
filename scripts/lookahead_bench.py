#!/usr/bin/env python
"""What Lookahead costs on the MI355X, at CoTNet-50's real buckets (FlatSGD's buckets of the mixed-precision model, bf16 gradients).
Four forms, timed alternately in one process:

  sgd         one `cot_sgd_step` per bucket (csrc/optim.hip): the plain step, the baseline
  non-sync    one `cot_lookahead_tick`, then per bucket `cot_sgd_step` and `cot_lookahead_step` (csrc/lookahead.hip) behind a tick that
              decides 0: k - 1 of every k steps.  (The tick runs with a k no count reaches.)
  sync        the same launches behind a tick that decides 2: every k-th step.  (The tick runs with k = 1 on a born block.)
  sync alone  the tick and the `cot_lookahead_step` launches without the SGD kernels: per parameter with bf16 weights and an fp32 master
              4 + 4 B read and 4 + 4 + 2 B written, over the time, as a share of the measured copy rate

Operands rotate over copies of the buckets that together exceed 512 MB, so that every replay reads from HBM.  Every form is recorded into
HIP graphs and replayed.  One repeat = three untimed and then `--iters` timed back-to-back replays of ONE form between two device events;
the first `--warmup` repeats of each are dropped.  Per form: median and min-max over the repeats in microseconds.  The copy rate is a
512 MB device-to-device copy, bytes read plus bytes written over its time.

    python scripts/lookahead_bench.py [--repeats 10] [--iters 10] [--out FILE]
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch  # noqa: E402

import cotnet_amd  # noqa: E402
from cotnet_amd import _lib  # noqa: E402
from cotnet_amd.flat_sgd import FlatSGD, to_mixed_bf16  # noqa: E402
from agc_bench import alternate  # noqa: E402
from grad_clip_bench import graph_of, rotating, row  # noqa: E402

LR, MOMENTUM, WD, ALPHA = 0.1, 0.9, 4e-5, 0.5
NEVER = 1 << 30  # a k no step count reaches: the tick decides 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the device"
    dev = torch.device("cuda:0")
    L = _lib.lib()
    torch.manual_seed(0)
    model = to_mixed_bf16(cotnet_amd.create_model("cotnet50", num_classes=1000).to(dev).train())
    lines = [f"# {torch.cuda.get_device_name(0)}; cotnet50, FlatSGD's buckets; {args.repeats} repeats of {args.iters} graph replays per form "
             f"(first {args.warmup} dropped), forms alternating; microseconds, device events"]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        src = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        copy_us = alternate({"copy": lambda: dst.copy_(src)}, args)["copy"]
        copy_rate = 2 * src.numel() / (statistics.median(copy_us) * 1e-6)  # bytes per second, read + written
        lines.append(row("512 MB device copy", copy_us, f"  = {copy_rate / 1e12:.2f} TB/s read + written"))
        del src, dst
        opt = FlatSGD(model, lr=LR, momentum=MOMENTUM, weight_decay=WD, lookahead_k=6)
        buckets = opt.reducer.buckets
        shapes = [(b.pflat.numel(), b.pflat.dtype, opt.reducer.reduced(b).dtype, WD if b.key == "decay" else 0.0) for b in buckets]
        nparam = sum(n for n, *_ in shapes)
        g_b = sum(n * torch.empty((), dtype=gdt).element_size() for n, _, gdt, _ in shapes)
        w_b = 4 * nparam
        copy_b = sum(n * 2 for n, pdt, _, _ in shapes if pdt != torch.float32)
        moved = {"sgd": (g_b + 2 * w_b) + (2 * w_b + copy_b), "alone": 2 * w_b + (2 * w_b + copy_b)}
        per_set = g_b + 4 * w_b + copy_b
        copies = max(2, -(-(512 << 20) // per_set) + 1)
        gen = torch.Generator(device=dev).manual_seed(1)
        sets = []
        for _ in range(copies):
            st = []
            for n, pdt, gdt, wd in shapes:
                w = torch.randn(n, device=dev, generator=gen)
                st.append(dict(n=n, wd=wd, param=w.to(pdt), master=w if pdt != torch.float32 else None,
                               mom=0.1 * torch.randn(n, device=dev, generator=gen), slow=torch.randn(n, device=dev, generator=gen),
                               grad=(1e-3 * torch.randn(n, device=dev, generator=gen)).to(gdt)))
            sets.append(st)
        lines.append(f"# {len(buckets)} buckets of {[n for n, *_ in shapes]} elements = {nparam / 1e6:.2f} M parameters; per step SGD moves "
                     f"{moved['sgd'] / 1e6:.1f} MB, a sync {moved['alone'] / 1e6:.1f} MB more (read + written); rotating over {copies} copies of "
                     f"{per_set / 1e6:.1f} MB")
        idle = torch.zeros(8, dtype=torch.int32, device=dev)                                      # ticked with NEVER: action 0
        born = torch.tensor([0, 0, 1, 0, 0, 0, 0, 0], dtype=torch.int32, device=dev)             # ticked with k = 1: action 2

        def P(t):
            return t.data_ptr() if t is not None else None

        def step(st, block, k, sgd=True, lookahead=True):
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            if lookahead:
                assert L.cot_lookahead_tick(block.data_ptr(), None, k, 0, stream) == 0, L.cot_last_error()
            for o in st:
                if sgd:
                    rc = L.cot_sgd_step(P(o["param"]), P(o["master"]), P(o["mom"]), P(o["grad"]), o["n"], LR, MOMENTUM, o["wd"], 1.0, 1,
                                        _lib.dtype_code(o["param"].dtype), _lib.dtype_code(o["grad"].dtype), stream)
                    assert rc == 0, L.cot_last_error()
                if lookahead:
                    rc = L.cot_lookahead_step(P(o["param"]), P(o["master"]), P(o["slow"]), o["n"], ALPHA, block.data_ptr(),
                                              _lib.dtype_code(o["param"].dtype), stream)
                    assert rc == 0, L.cot_last_error()

        # every graph and everything a graph touches stays referenced until the forms have been timed (adamw_bench.py says why)
        graphs = {"sgd": [graph_of(lambda st=st: step(st, idle, NEVER, lookahead=False), s) for st in sets],
                  "non-sync": [graph_of(lambda st=st: step(st, idle, NEVER), s) for st in sets],
                  "sync": [graph_of(lambda st=st: step(st, born, 1), s) for st in sets],
                  "alone": [graph_of(lambda st=st: step(st, born, 1, sgd=False), s) for st in sets]}
        names = {"sgd": "cot_sgd_step per bucket", "non-sync": "tick + (sgd, lookahead) per bucket, action 0",
                 "sync": "tick + (sgd, lookahead) per bucket, action 2", "alone": "tick + cot_lookahead_step per bucket, action 2"}
        times = alternate({k: rotating(g) for k, g in graphs.items()}, args)
        torch.cuda.synchronize()
        words = idle.tolist(), born.tolist()
        assert words[0][1:4] == [0, 0, 0] and words[1][1:3] == [2, 1] and words[1][3] > 0, words  # the forms ran what their names say
        for k, v in times.items():
            extra = ""
            if k in moved:
                rate = moved[k] / (statistics.median(v) * 1e-6)
                extra = f"  {moved[k] / 1e6:.1f} MB read + written, {rate / 1e12:.2f} TB/s = {rate / copy_rate:.0%} of the copy rate"
            lines.append(row(names[k], v, extra))
        base, non, syn = (statistics.median(times[k]) for k in ("sgd", "non-sync", "sync"))
        spread = max(times["sgd"]) - min(times["sgd"])
        lines.append(f"# a non-sync step costs {non - base:+.2f} us over the plain step's {base:.2f} us ({(non - base) / base:+.1%}; the plain "
                     f"step's own min-max spread is {spread:.2f} us): one tick and {len(buckets)} launches that return at once")
        lines.append(f"# a sync step costs {syn - base:+.2f} us over the plain step ({(syn - base) / base:+.1%}); with k = 6 the average step "
                     f"costs {((5 * non + syn) / 6 - base) / base:+.1%}")
    torch.cuda.current_stream().wait_stream(s)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
