#!/usr/bin/env python
"""What the fused AdamW step costs on the MI355X, at CoTNet-50's real buckets (FlatAdamW's buckets of the mixed-precision model), for bf16
gradient buckets and for fp32 ones.  Three forms, timed alternately in one process:

  adamw   one `cot_adam_tick` and one `cot_adamw_step` per bucket (csrc/adamw.hip)
  sgd     one `cot_sgd_step` per bucket on the same buckets (csrc/optim.hip): the yardstick -- a streaming kernel of the same shape
  torch   torch.optim.AdamW on fp32 tensors of the same sizes, foreach=True, and fused=True where the installed torch accepts it on this
          device (capturable=True, so that its step can be recorded); the log says which ran, and whether captured or eager

Operands rotate over copies of the buckets that together exceed 512 MB, so that every replay reads from HBM.  Every form is recorded into
HIP graphs and replayed.  One repeat = three untimed and then `--iters` timed back-to-back replays of ONE form between two device events;
the first `--warmup` repeats of each are dropped.  Per form: median and min-max over the repeats in microseconds; for the two kernel
forms also the bytes they move (per parameter with bf16 weights and gradients and an fp32 master: AdamW 14 B read + 14 B written, SGD 10 +
10) over the time, as a share of the measured copy rate (a 512 MB device-to-device copy, bytes read plus bytes written over its time).

    python scripts/adamw_bench.py [--repeats 10] [--iters 10] [--out FILE]
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
from cotnet_amd.flat_adamw import FlatAdamW  # noqa: E402
from cotnet_amd.flat_sgd import to_mixed_bf16  # noqa: E402
from agc_bench import alternate  # noqa: E402
from grad_clip_bench import graph_of, rotating, row  # noqa: E402

LR, BETAS, EPS, WD, MOMENTUM = 1e-3, (0.9, 0.999), 1e-8, 0.05, 0.9


def esize(dt):
    return torch.empty((), dtype=dt).element_size()


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
    lines = [f"# {torch.cuda.get_device_name(0)}; cotnet50, FlatAdamW's buckets; {args.repeats} repeats of {args.iters} graph replays per form "
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
        opt = FlatAdamW(model, lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)
        buckets = opt.reducer.buckets
        block = torch.zeros(8, dtype=torch.int32, device=dev)
        for gd_name, gd in (("bf16 gradients", None), ("fp32 gradients", torch.float32)):
            shapes = [(b.pflat.numel(), b.pflat.dtype, opt.reducer.reduced(b).dtype if gd is None else gd, WD if b.key == "decay" else 0.0)
                      for b in buckets]
            nparam = sum(n for n, *_ in shapes)
            # bytes per parameter: the gradient and the weights (the fp32 master, or the fp32 parameters) read, the weights and a bf16
            # working copy written; AdamW reads and writes two fp32 moments, SGD one
            g_b = sum(n * esize(gdt) for n, _, gdt, _ in shapes)
            w_b = 4 * nparam
            copy_b = sum(n * 2 for n, pdt, _, _ in shapes if pdt != torch.float32)
            moved = {"adamw": (g_b + 3 * w_b) + (3 * w_b + copy_b), "sgd": (g_b + 2 * w_b) + (2 * w_b + copy_b)}
            per_set = g_b + 4 * w_b + copy_b
            copies = max(2, -(-(512 << 20) // per_set) + 1)
            gen = torch.Generator(device=dev).manual_seed(1)
            sets = []
            for _ in range(copies):
                st = []
                for n, pdt, gdt, wd in shapes:
                    w = torch.randn(n, device=dev, generator=gen)
                    st.append(dict(n=n, wd=wd, param=w.to(pdt), master=w if pdt != torch.float32 else None,
                                   m=0.1 * torch.randn(n, device=dev, generator=gen), v=(0.1 * torch.randn(n, device=dev, generator=gen)).square(),
                                   mom=0.1 * torch.randn(n, device=dev, generator=gen), grad=torch.randn(n, device=dev, generator=gen).to(gdt)))
                sets.append(st)
            lines.append(f"# {gd_name}: {len(buckets)} buckets of {[n for n, *_ in shapes]} elements = {nparam / 1e6:.2f} M parameters; per step "
                         f"AdamW moves {moved['adamw'] / 1e6:.1f} MB, SGD {moved['sgd'] / 1e6:.1f} MB (read + written); rotating over {copies} "
                         f"copies of {per_set / 1e6:.1f} MB")

            def P(t):
                return t.data_ptr() if t is not None else None

            def adamw(st):
                stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                assert L.cot_adam_tick(block.data_ptr(), None, BETAS[0], BETAS[1], stream) == 0, L.cot_last_error()
                for o in st:
                    rc = L.cot_adamw_step(P(o["param"]), P(o["master"]), P(o["m"]), P(o["v"]), P(o["grad"]), o["n"], LR, None, block.data_ptr(),
                                          None, BETAS[0], BETAS[1], EPS, o["wd"], 1.0, 1, _lib.dtype_code(o["param"].dtype),
                                          _lib.dtype_code(o["grad"].dtype), stream)
                    assert rc == 0, L.cot_last_error()

            def sgd(st):
                stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                for o in st:
                    rc = L.cot_sgd_step(P(o["param"]), P(o["master"]), P(o["mom"]), P(o["grad"]), o["n"], LR, MOMENTUM, o["wd"], 1.0, 1,
                                        _lib.dtype_code(o["param"].dtype), _lib.dtype_code(o["grad"].dtype), stream)
                    assert rc == 0, L.cot_last_error()

            # every graph and everything a graph touches stays referenced until the forms have been timed: each capture collects
            # garbage and empties the allocator's cache (torch.cuda.graph.__enter__), so an operand that lost its last reference is
            # unmapped by the next capture, and a graph replayed on it faults
            ag = [graph_of(lambda st=st: adamw(st), s) for st in sets]
            sg = [graph_of(lambda st=st: sgd(st), s) for st in sets]
            keep = [ag, sg]
            forms = {"adamw": rotating(ag), "sgd": rotating(sg)}
            names = {"adamw": "cot_adam_tick + cot_adamw_step per bucket", "sgd": "cot_sgd_step per bucket"}
            if gd is None:  # the torch form does not depend on the buckets' gradient dtype (fp32 tensors): timed once
                for label, kw in (("foreach", dict(foreach=True)), ("fused", dict(fused=True))):
                    try:
                        opts = []
                        for st in sets:
                            ps = [torch.nn.Parameter(torch.randn(o["n"], device=dev, generator=gen)) for o in st]
                            for p in ps:
                                p.grad = torch.randn(p.numel(), device=dev, generator=gen)
                            groups = [dict(params=[p], weight_decay=o["wd"]) for p, o in zip(ps, st)]
                            opts.append(torch.optim.AdamW(groups, lr=LR, betas=BETAS, eps=EPS, capturable=True, **kw))
                    except Exception as exc:
                        lines.append(f"# torch.optim.AdamW({label}=True) is not accepted here ({type(exc).__name__}: {str(exc)[:120]}): not timed")
                        continue
                    keep.append(opts)  # (the optimizers own the parameters, gradients and state their graphs step)
                    try:
                        tg = [graph_of(o.step, s) for o in opts]
                        keep.append(tg)
                        forms[label] = rotating(tg)
                        names[label] = f"torch.optim.AdamW({label}=True), fp32, captured"
                    except Exception as exc:
                        lines.append(f"# torch.optim.AdamW({label}=True) could not be captured ({type(exc).__name__}): timed EAGERLY, host cost included")
                        torch.cuda.synchronize()
                        forms[label] = rotating([type("E", (), {"replay": staticmethod(o.step)}) for o in opts])
                        names[label] = f"torch.optim.AdamW({label}=True), fp32, eager"
            times = alternate(forms, args)
            torch.cuda.synchronize()
            shares = {}
            for k, v in times.items():
                extra = ""
                if k in moved:
                    rate = moved[k] / (statistics.median(v) * 1e-6)
                    shares[k] = [moved[k] / (t * 1e-6) / copy_rate for t in v]
                    extra = (f"  {moved[k] / 1e6:.1f} MB read + written, {rate / 1e12:.2f} TB/s = {rate / copy_rate:.0%} of the copy rate "
                             f"(min-max {min(shares[k]):.0%} - {max(shares[k]):.0%})")
                elif "adamw" in times:
                    extra = f"  {statistics.median(v) / statistics.median(times['adamw']):.1f}x the fused step"
                lines.append(row(names[k], v, extra))
            a, b = statistics.median(shares["adamw"]), statistics.median(shares["sgd"])
            spread = max(max(shares[k]) - min(shares[k]) for k in shares)
            lines.append(f"# {gd_name}: AdamW reaches {a:.0%} of the copy rate, SGD {b:.0%}; the difference {b - a:+.1%} against the run's own "
                         f"min-max spread of {spread:.1%}: {'within' if b - a <= spread else 'BEYOND'} it")
            del forms, keep, sets, times
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
    torch.cuda.current_stream().wait_stream(s)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
