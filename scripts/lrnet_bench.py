"""A/B of LR-Net's local relation: the fused HIP op (cotnet_amd.local_relation, csrc/local_relation.hip; --window 7:
csrc/local_relation7.hip) against the reference's composition (`local_relation_reference`: unfold, + pos, product, head sum, window
softmax + aggregation), at every attention-layer geometry of LR-Net-50, B = 80, bf16; then the training step of lrnet50 (--window 3) or
lrnet50_k7 (--window 7) through bench.py, eager and replayed.

Per geometry: forward and forward + backward of each form, timed with device events in the same process, the two forms
alternated rep by rep (median of the reps).  Algorithmic bytes (what a kernel must move at least, e = bytes per element, T = k k
taps, so a tap tensor is T G HW = T/8 C HW):
  forward               q, k, v, out (4 C HW) + probs (T/8 C HW)             = 5.125 e C HW per image at 3x3, 10.125 at 7x7
  relation backward     gL (T/8 C HW) + q, k, gq, gk (4 C HW)                = the same
  aggregation backward  gout, v, gv (3 C HW) + probs, gL (2 T/8 C HW)        = 15.25 e C HW at 7x7 (lr7_bwd_agg; --window 7 only)
reported as a fraction of 8 TB/s over each fused kernel's time (kernel times from the library's per-launch recorder,
cot_profile_begin / _end).

    python scripts/lrnet_bench.py [--window 3|7] [--reps 20] [--no-model] [--steps 20 --warmup 5]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cotnet_amd import _lib  # noqa: E402
from cotnet_amd.aggregation_zeropad import profile_begin, profile_end  # noqa: E402
from cotnet_amd.local_relation import local_relation, local_relation_reference  # noqa: E402

STAGES = [(64, 56), (128, 56), (128, 28), (256, 28), (256, 14), (512, 14), (512, 7)]
PEAK = 8e12


def make(C, H, B, dev, ks=3):
    g = torch.Generator(device=dev).manual_seed(C + H)
    q, k = (0.5 * torch.randn(B, C, H, H, device=dev, generator=g, dtype=torch.bfloat16) for _ in range(2))
    v = torch.randn(B, C, H, H, device=dev, generator=g, dtype=torch.bfloat16)
    gout = torch.randn(B, C, H, H, device=dev, generator=g, dtype=torch.bfloat16)
    pos_h = torch.randn(C, ks, 1, device=dev, generator=g).requires_grad_(True)
    pos_w = torch.randn(C, 1, ks, device=dev, generator=g).requires_grad_(True)
    return [t.requires_grad_(True) for t in (q, k, v)], gout, pos_h, pos_w


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stage_ab(C, H, B, reps, dev, ks=3):
    (q, k, v), gout, ph, pw = make(C, H, B, dev, ks)
    forms = {"fused": local_relation, "composition": local_relation_reference}
    fwd = {f: [] for f in forms}
    fb = {f: [] for f in forms}

    def run_fwd(f):
        with torch.no_grad():
            forms[f](q, k, v, ph, pw, ks)

    def run_fb(f):
        y = forms[f](q, k, v, ph, pw, ks)
        torch.autograd.grad(y, (q, k, v, ph, pw), gout)
    for f in forms:  # warm-up (library load, workspace sizes, allocator)
        run_fwd(f)
        run_fb(f)
    torch.cuda.synchronize()
    for _ in range(reps):
        for f in forms:  # alternated
            fwd[f].append(timed(lambda: run_fwd(f)))
            fb[f].append(timed(lambda: run_fb(f)))
    # kernel times of the fused form from the library's per-launch recorder
    os.environ["COT_PROFILE_ALL"] = "1"
    profile_begin()
    for _ in range(5):
        run_fb("fused")
    torch.cuda.synchronize()
    recs = profile_end()
    kt = {}
    for r in recs:  # (kind, geometry, dtype, layout, ms, bytes, kernel)
        kt.setdefault(r[6], []).append(r[4])
    kms = {name: statistics.median(v) for name, v in kt.items()}
    e = 2
    taps = ks * ks / 8
    alg = (4 + taps) * e * C * H * H * B
    alg_agg = (3 + 2 * taps) * e * C * H * H * B
    stem = "lr_" if ks == 3 else "lr7_"
    fwd_k = next((v for n, v in kms.items() if stem + "fwd" in n), None)
    rel_k = next((v for n, v in kms.items() if stem + "bwd_rel" in n), None)
    agg_k = next((v for n, v in kms.items() if "lr7_bwd_agg" in n), None)
    med = {k2: {f: statistics.median(v) for f, v in d.items()} for k2, d in (("fwd", fwd), ("fwd_bwd", fb))}
    return {
        "C": C, "H": H, "B": B, "dtype": "bf16", "window": ks,
        "fwd_ms": med["fwd"], "fwd_bwd_ms": med["fwd_bwd"],
        "speedup_fwd": med["fwd"]["composition"] / med["fwd"]["fused"],
        "speedup_fwd_bwd": med["fwd_bwd"]["composition"] / med["fwd_bwd"]["fused"],
        "kernel_ms": kms,
        "alg_bytes_fwd": alg, "alg_bytes_rel_bwd": alg,
        "fwd_kernel_frac_8TBps": (alg / (fwd_k * 1e-3)) / PEAK if fwd_k else None,
        "rel_bwd_kernel_frac_8TBps": (alg / (rel_k * 1e-3)) / PEAK if rel_k else None,
        **({"alg_bytes_agg_bwd": alg_agg, "agg_bwd_kernel_frac_8TBps": (alg_agg / (agg_k * 1e-3)) / PEAK} if agg_k else {}),
    }


def model_line(steps, warmup, eager, model="lrnet50"):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--model", model, "--batch", "80", "--steps", str(steps),
           "--warmup", str(warmup)] + (["--eager"] if eager else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not lines:
        return {"error": r.returncode, "stderr": r.stderr[-2000:]}
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=int, default=3, choices=(3, 7), help="3: lrnet50's window; 7: LR-Net's own (lrnet50_k7)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=80)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    model = "lrnet50" if args.window == 3 else "lrnet50_k7"
    for C, H in STAGES:
        print(json.dumps(stage_ab(C, H, args.batch, args.reps, dev, args.window)), flush=True)
        torch.cuda.empty_cache()  # (the 7x7 composition's unfolded tensors: 1.6 GB each at the first stage)
    if not args.no_model:
        for eager in (True, False):
            res = model_line(args.steps, args.warmup, eager, model)
            print(json.dumps({"model": model, "img": 224, "batch": 80, "step": "eager" if eager else "replayed", "bench": res}),
                  flush=True)
    print(json.dumps({"module_fallbacks": _lib.FALLBACKS}))


if __name__ == "__main__":
    main()
