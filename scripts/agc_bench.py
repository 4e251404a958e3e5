#!/usr/bin/env python
"""What adaptive gradient clipping costs on the MI355X, at CoTNet-50's real buckets (FlatSGD's buckets of the mixed-precision model and
their unit tables), for bf16 gradient buckets and for fp32 ones:

  none    one `cot_agc_clip` per bucket with a factor so large that NO unit clips: a pure read of the gradients and the fp32 weights
  all     the same launches with a factor so small that EVERY unit clips: the read, the re-read of the gradients out of L2 and their
          store.  A clipped unit ends AT its threshold, so a second call with the same factor would clip only about half of the units:
          every replay of this form is a graph of its own whose factor is 0.8 times the one that last visited its operands (the
          norms stay far above the formula's 1e-6 floor of the gradient norm over all visits; the script asserts that every unit
          clipped in the last replay)
  torch   the reference's formula (utils/clip_grad.py:3-24) restated per parameter in torch on views of the same buffers: about eight
          launches per tensor, and a torch.where that rewrites every gradient whatever clips (run with the first form's factor, so that it
          hands every gradient through unchanged and leaves the second form's operands as they are: its work does not depend on the values)

Operands rotate over copies of the buckets (gradients and weights) that together exceed 512 MB, so that every replay reads from HBM.
Every form is recorded into HIP graphs and replayed (the host's launch cost is out of the figure, as in the replayed training step).
One repeat = three untimed and then `--iters` timed back-to-back replays of ONE form between two device events; the forms alternate repeat
by repeat in one process;
the first `--warmup` repeats of each are dropped.  Per form: median and min-max over the repeats in microseconds, and for the two
kernel forms the share of the measured copy rate (a 512 MB device-to-device copy, bytes read plus bytes written over its time) that the
bytes they move reach.

`--alt-libs A.so,B.so`: builds of the library with another COT_AGC_MAX_GROUPS, timed in the first form on the same operands in the same
process (how the header's value was chosen).

    python scripts/agc_bench.py [--repeats 10] [--iters 10] [--alt-libs ...] [--out FILE]
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
from grad_clip_bench import graph_of, rotating, row, timed  # noqa: E402

EPS = 1e-3
NONE, ALL0, SHRINK = 1e6, 0.5, 0.8  # factors: nothing clips / everything clips, times SHRINK per visit of a set of operands


def unitwise_norm(x):
    return x.norm(2.0) if x.ndim <= 1 else x.norm(2.0, dim=tuple(range(1, x.ndim)), keepdim=True)


PRE = 3  # untimed replays of a form in front of each of its timed windows


def alternate(forms, args):
    """{name: fn} -> {name: [microseconds per call]}; as grad_clip_bench.alternate, with PRE untimed calls of the form in front of every
    window: the torch form is 18 ms of small kernels, and the form that follows it would otherwise be timed while the clocks recover"""
    times = {k: [] for k in forms}
    for rep in range(args.repeats + args.warmup):
        for k, fn in forms.items():
            for _ in range(PRE):
                fn()
            t = timed(fn, args.iters)
            if rep >= args.warmup:
                times[k].append(t)
    return times


def in_turn(fns):
    """each call runs the next of `fns`; running out of them is an error, not a wrap-around"""
    state = [0]

    def fn():
        fns[state[0]]()
        state[0] += 1
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--alt-libs", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the device"
    dev = torch.device("cuda:0")
    L = _lib.lib()
    alt = {}
    for path in filter(None, args.alt_libs.split(",")):
        A = _lib.bind(ctypes.CDLL(os.path.abspath(path)), lenient=True)
        alt[f"cap {A.cot_agc_max_groups()} ({os.path.basename(path)})"] = A
    torch.manual_seed(0)
    model = to_mixed_bf16(cotnet_amd.create_model("cotnet50", num_classes=1000).to(dev).train())
    lines = [f"# {torch.cuda.get_device_name(0)}; cotnet50, FlatSGD's buckets and unit tables; {args.repeats} repeats of {args.iters} graph "
             f"replays per form (first {args.warmup} dropped), forms alternating; microseconds, device events"]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        src = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        copy_us = alternate({"copy": lambda: dst.copy_(src)}, args)["copy"]
        copy_rate = 2 * src.numel() / (statistics.median(copy_us) * 1e-6)  # bytes per second, read + written
        lines.append(row("512 MB device copy", copy_us, f"  = {copy_rate / 1e12:.2f} TB/s read + written"))
        del src, dst
        opt = FlatSGD(model, lr=0.0, momentum=0.9, weight_decay=4e-5, nesterov=True, agc=0.01)
        buckets, tables, coefs = opt.reducer.buckets, opt._agc_units, opt._agc_coef
        nunits = sum(t.shape[0] for t in tables)
        longest = max(int(t[:, 1].max()) for t in tables)
        for gd_name, gd in (("bf16 gradients", None), ("fp32 gradients", torch.float32)):
            shapes = [(b.pflat.numel(), opt.reducer.reduced(b).dtype if gd is None else gd) for b in buckets]
            g_bytes = sum(n * torch.empty((), dtype=dt).element_size() for n, dt in shapes)
            w_bytes = sum(4 * n for n, _ in shapes)
            copies = max(2, -(-(512 << 20) // (g_bytes + w_bytes)) + 1)
            gen = torch.Generator(device=dev).manual_seed(1)
            sets = []
            for _ in range(copies):
                gs = [(10.0 * torch.randn(n, device=dev, generator=gen)).to(dt) for n, dt in shapes]
                ws = [torch.randn(n, device=dev, generator=gen) for n, _ in shapes]
                sets.append((gs, ws))
            lines.append(f"# {gd_name}: {len(buckets)} buckets of {[n for n, _ in shapes]} elements, {nunits} units (longest {longest}); "
                         f"{g_bytes / 1e6:.1f} MB of gradients + {w_bytes / 1e6:.1f} MB of fp32 weights (randn; gradients 10 * randn); "
                         f"rotating over {copies} copies")

            def clip(st, factor, L=L):
                stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                for g, w, t, c in zip(st[0], st[1], tables, coefs):
                    rc = L.cot_agc_clip(g.data_ptr(), w.data_ptr(), t.data_ptr(), t.shape[0], g.numel(), factor, EPS, c.data_ptr(),
                                        _lib.dtype_code(g.dtype), stream)
                    assert rc == 0, L.cot_last_error()

            def torch_agc(st, factor):
                pairs = [(w[off:off + p.numel()].view_as(p), g[off:off + p.numel()].view_as(p))
                         for b, g, w in zip(buckets, st[0], st[1]) for p, off in zip(b.params, b.offs)]

                def fn():
                    for w, g in pairs:
                        max_norm = unitwise_norm(w).clamp_(min=EPS).mul_(factor)
                        gn = unitwise_norm(g)
                        g.copy_(torch.where(gn < max_norm, g, g * (max_norm / gn.clamp(min=1e-6))))
                return fn

            replays = (args.repeats + args.warmup) * (args.iters + PRE)
            keep = [graph_of(lambda st=st: clip(st, NONE), s) for st in sets]
            forms = {f"cot_agc_clip, no unit clips (cap {L.cot_agc_max_groups()}, this build)": rotating(keep)}
            for name, A in alt.items():
                ag = [graph_of(lambda st=st, A=A: clip(st, NONE, A), s) for st in sets]
                keep += ag
                forms[f"cot_agc_clip, no unit clips, {name}"] = rotating(ag)
            torch.cuda.synchronize()
            none_coef = torch.cat(coefs).cpu()
            for st in sets:  # visit 0 of every set, eagerly; the graphs below are only recorded, and replayed in this order
                clip(st, ALL0)
            torch.cuda.synchronize()
            every = []
            for k in range(replays):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=s):
                    clip(sets[k % copies], ALL0 * SHRINK ** (1 + k // copies))
                every.append(g)
            keep += every
            forms["cot_agc_clip, every unit clips"] = in_turn([g.replay for g in every])
            try:
                tg = [graph_of(torch_agc(st, NONE), s) for st in sets]
                keep += tg
                forms["the formula per parameter in torch"] = rotating(tg)
            except Exception as exc:  # not capturable on this torch: time it eagerly and say so
                lines.append(f"# the torch composition could not be captured ({type(exc).__name__}): timed EAGERLY, host launch cost included")
                torch.cuda.synchronize()
                forms["the formula per parameter in torch, eager"] = rotating([torch_agc(st, NONE) for st in sets])
            times = alternate(forms, args)
            torch.cuda.synchronize()
            all_coef = torch.cat(coefs).cpu()
            lines.append(f"# check: {int((none_coef == 1).sum())} of {nunits} coefficients are 1 after the first form's captures; "
                         f"{int((all_coef < 1).sum())} of {nunits} are < 1 after the last replay of the second")
            assert int((all_coef < 1).sum()) == nunits and int((none_coef == 1).sum()) == nunits, "a form did not run in its regime"
            moved = {k: (2 * g_bytes + w_bytes if "every" in k else g_bytes + w_bytes) for k in forms if k.startswith("cot_agc_clip")}
            tmed = statistics.median(next(v for k, v in times.items() if "torch" in k))
            for k, v in times.items():
                extra = ""
                if k in moved:
                    rate = moved[k] / (statistics.median(v) * 1e-6)
                    extra = (f"  {moved[k] / 1e6:.1f} MB read + written, {rate / 1e12:.2f} TB/s = {rate / copy_rate:.0%} of the copy rate; "
                             f"{tmed / statistics.median(v):.1f}x below torch")
                lines.append(row(k, v, extra))
            del forms, keep, every, sets, times
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
