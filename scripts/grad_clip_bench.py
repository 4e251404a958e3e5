#!/usr/bin/env python
"""What clipping by global norm costs on the MI355X, at CoTNet-50's real bucket sizes (FlatSGD's buckets of the mixed-precision model),
for bf16 gradient buckets and for grad_dtype=torch.float32:

  norm    the `cot_grad_sumsq` launches (one per bucket) plus `cot_grad_clip_finish`, against
          `torch.nn.utils.clip_grad_norm_(foreach=True)` on per-parameter views of the same buckets.  torch's call also SCALES the
          gradients (one more read and write of all of them: it multiplies by the clamped coefficient whatever it is); here the
          scaling is the `gscale` factor of the SGD kernel, which is the point of the comparison.  Reported with the share of the
          measured copy rate (a 512 MB device-to-device copy, bytes read plus bytes written over its time) that the bytes READ reach.
          "hot": the same buckets every replay (51 MB of bf16 gradients fit the 256 MB Infinity Cache); "rotating": over copies of the
          buckets that together exceed 512 MB, so that every replay reads from HBM.
  sgd     `cot_sgd_step_clip` (block {scale 0.5, skip 0}) against `cot_sgd_step` over all buckets, lr = 0.

Every form is recorded into a HIP graph and replayed (the host's launch cost is out of the figure, as in the replayed training step).
One repeat = `--iters` back-to-back replays of ONE form between two device events; the forms alternate repeat by repeat in one process;
the first `--warmup` repeats of each are dropped.  Per form: median and min-max over the repeats, microseconds.

`--alt-libs A.so,B.so`: builds of the library with another COT_GRAD_NORM_PARTS, timed on the same buckets in the same process (how
the header's value was chosen).

    python scripts/grad_clip_bench.py [--repeats 30] [--iters 20] [--alt-libs ...] [--out FILE]
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


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters  # microseconds per call


def graph_of(fn, s):
    fn()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        fn()
    return g


def rotating(graphs):
    state = [0]

    def fn():
        graphs[state[0] % len(graphs)].replay()
        state[0] += 1
    return fn


def alternate(forms, args):
    """{name: fn} -> {name: [microseconds per call]}"""
    times = {k: [] for k in forms}
    for rep in range(args.repeats + args.warmup):
        for k, fn in forms.items():
            t = timed(fn, args.iters)
            if rep >= args.warmup:
                times[k].append(t)
    return times


def row(name, v, extra=""):
    return f"{name:>44s} | median {statistics.median(v):9.2f} us  (min {min(v):9.2f}, max {max(v):9.2f}){extra}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--alt-libs", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the device"
    dev = torch.device("cuda:0")
    libs = {f"PARTS {_lib.lib().cot_grad_norm_parts()} (this build)": _lib.lib()}
    for path in filter(None, args.alt_libs.split(",")):
        L = _lib.bind(ctypes.CDLL(os.path.abspath(path)), lenient=True)
        libs[f"PARTS {L.cot_grad_norm_parts()} ({os.path.basename(path)})"] = L
    torch.manual_seed(0)
    model = to_mixed_bf16(cotnet_amd.create_model("cotnet50", num_classes=1000).to(dev).train())
    lines = [f"# {torch.cuda.get_device_name(0)}; cotnet50, FlatSGD's buckets; {args.repeats} repeats of {args.iters} graph replays per form "
             f"(first {args.warmup} dropped), forms alternating; microseconds, device events"]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        # the copy rate every share below refers to
        src = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        copy_us = alternate({"copy": lambda: dst.copy_(src)}, args)["copy"]
        copy_rate = 2 * src.numel() / (statistics.median(copy_us) * 1e-6)  # bytes per second, read + written
        lines.append(row("512 MB device copy", copy_us, f"  = {copy_rate / 1e12:.2f} TB/s read + written"))
        del src, dst
        for gd_name, gd in (("bf16 gradients", None), ("grad_dtype=float32", torch.float32)):
            opt = FlatSGD(model, lr=0.0, momentum=0.9, weight_decay=4e-5, nesterov=True)
            buckets = opt.reducer.buckets
            # (without a process group the reducer does not widen its buckets: the fp32 form gets buffers of its own, same sizes)
            reduced = [opt.reducer.reduced(b) if gd is None else torch.empty(b.pflat.numel(), dtype=gd, device=dev) for b in buckets]
            nbytes = sum(g.numel() * g.element_size() for g in reduced)
            copies = max(2, -(-(512 << 20) // nbytes) + 1)
            gen = torch.Generator(device=dev).manual_seed(1)
            sets = [reduced] + [[torch.empty_like(g) for g in reduced] for _ in range(copies - 1)]
            for st in sets:
                for g in st:
                    g.copy_(1e-2 * torch.randn(g.numel(), device=dev, generator=gen))
            lines.append(f"# {gd_name}: {len(buckets)} buckets of {[g.numel() for g in reduced]} elements, {nbytes / 1e6:.1f} MB; rotating over "
                         f"{copies} copies")
            state = torch.zeros(8, dtype=torch.int32, device=dev)
            forms, keep = {}, []
            for lname, L in libs.items():
                parts = L.cot_grad_norm_parts()
                partials = torch.zeros(len(reduced) * parts, dtype=torch.float32, device=dev)
                keep.append(partials)

                def norm(st, L=L, parts=parts, partials=partials):
                    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                    for i, g in enumerate(st):
                        rc = L.cot_grad_sumsq(g.data_ptr(), g.numel(), _lib.dtype_code(g.dtype), partials.data_ptr() + 4 * parts * i, stream)
                        assert rc == 0, L.cot_last_error()
                    rc = L.cot_grad_clip_finish(partials.data_ptr(), partials.numel(), 1.0, state.data_ptr(), stream)
                    assert rc == 0, L.cot_last_error()

                def finish_only(L=L, partials=partials):
                    rc = L.cot_grad_clip_finish(partials.data_ptr(), partials.numel(), 1.0, state.data_ptr(),
                                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
                    assert rc == 0, L.cot_last_error()
                gs = [graph_of(lambda st=st: norm(st), s) for st in sets]
                keep += gs
                forms[f"norm, hot, {lname}"] = gs[0].replay
                forms[f"norm, rotating, {lname}"] = rotating(gs)
                gf = graph_of(finish_only, s)
                keep.append(gf)
                forms[f"finish alone, {lname}"] = gf.replay
            next(iter(forms.values()))()  # (this build, the first set)
            torch.cuda.synchronize()
            ours = float(state[:2].view(torch.float32)[1])
            want = float(torch.sqrt(sum(g.double().square().sum() for g in sets[0])))
            lines.append(f"# norm of the first set: {ours:.9g}, fp64 torch {want:.9g}")

            def torch_clip(st):
                params = []
                for b, flat in zip(buckets, st):
                    for p, off in zip(b.params, b.offs):
                        q = torch.nn.Parameter(flat[off:off + p.numel()].view_as(p), requires_grad=True)
                        q.grad = flat[off:off + p.numel()].view_as(p)
                        params.append(q)
                return lambda: torch.nn.utils.clip_grad_norm_(params, 1e30, foreach=True)
            try:
                tg = [graph_of(torch_clip(st), s) for st in sets]
                keep += tg
                forms["clip_grad_norm_(foreach), hot"] = tg[0].replay
                forms["clip_grad_norm_(foreach), rotating"] = rotating(tg)
            except Exception as exc:  # not capturable on this torch: time it eagerly and say so
                lines.append(f"# clip_grad_norm_ could not be captured ({type(exc).__name__}): timed EAGERLY, host launch cost included")
                torch.cuda.synchronize()
                fns = [torch_clip(st) for st in sets]
                forms["clip_grad_norm_(foreach), eager, hot"] = fns[0]
            times = alternate(forms, args)
            for k, v in times.items():
                share = ""
                if k.startswith("norm"):
                    share = f"  {nbytes / (statistics.median(v) * 1e-6) / 1e12:.2f} TB/s read = {nbytes / (statistics.median(v) * 1e-6) / copy_rate:.0%} of the copy rate"
                lines.append(row(k, v, share))
            # the SGD kernel behind the block against the plain one
            L = _lib.lib()
            state[0:1].view(torch.float32)[0] = 0.5
            state[2] = 0

            def sgd(clip):
                stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                for b, st_, g in zip(buckets, opt.state, reduced):
                    head = (b.pflat.data_ptr(), st_["master"].data_ptr() if st_["master"] is not None else None, st_["mom"].data_ptr(),
                            g.data_ptr(), b.pflat.numel())
                    tail = (0.9, 4e-5 if b.key == "decay" else 0.0, 1.0, 1, _lib.dtype_code(b.pflat.dtype), _lib.dtype_code(g.dtype), stream)
                    rc = L.cot_sgd_step_clip(*head, 0.0, None, state.data_ptr(), *tail) if clip else L.cot_sgd_step(*head, 0.0, *tail)
                    assert rc == 0, L.cot_last_error()
            g_plain, g_clip = graph_of(lambda: sgd(False), s), graph_of(lambda: sgd(True), s)
            times = alternate({"cot_sgd_step, all buckets": g_plain.replay, "cot_sgd_step_clip, all buckets": g_clip.replay}, args)
            for k, v in times.items():
                lines.append(row(k, v))
            del forms, keep, sets, opt, g_plain, g_clip
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
