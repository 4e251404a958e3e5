#!/usr/bin/env python
"""What the table block (per-sample mixup / CutMix: `PerSampleMixup`, header mode 3) costs on the MI355X, and that the header modes it
sits next to cost what they did.

(i)   no regression: `cot_mix_normalize` under header modes 0, 1, 2 at 80 x 3 x 224 x 224 uint8 -> bf16 from THIS build and, with
      `--parent-lib`, from a libcotnet_hip.so built from the parent commit, both loaded into this one process and alternating.  The
      margin is the parent's own min-max spread over its repeats: the noise of the comparison.
(ii)  table mode on the same buffers: every sample mixup, every sample CutMix (a 112 x 112 box per sample, each at another place), and the
      recipe's 50 / 50 mixture, against header modes 1 and 2.  The bytes moved are the same (2 B read + 2 B written per pixel).
(iii) the loss, forward + backward at 80 x 1000 bf16, table block against header block (and the parent's).

The method is scripts/recipe_loss_bench.py's: inputs and outputs rotate through slots that together exceed the 256 MiB last-level cache;
one repeat = `--iters` back-to-back calls of ONE form between two device events; the forms alternate repeat by repeat; the first
`--warmup` repeats of each are dropped; median and min-max per form.  Every form is the bare C call on preallocated buffers, so that
the two libraries are called the same way.  Writes profiles/mix_modes_bench.log.

    python scripts/mix_modes_bench.py [--parent-lib /path/to/parent/libcotnet_hip.so] [--repeats 40] [--iters 20]
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cotnet_amd import PerSampleMixup, _lib  # noqa: E402
from cotnet_amd.mixup import pack_params  # noqa: E402
from scripts.recipe_loss_bench import alternate, row  # noqa: E402


def P(t):
    return ctypes.c_void_p(t.data_ptr())


def verdict(name, this, parent):
    med, lo, hi = statistics.median(this), min(parent), max(parent)
    inside = lo <= med <= hi
    return (f"{name:>34s} | this / parent medians x{med / statistics.median(parent):.4f}; this median {med:.2f} us "
            f"{'inside' if inside else 'OUTSIDE'} the parent's spread [{lo:.2f}, {hi:.2f}]")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libcotnet_hip.so built from the parent commit")
    ap.add_argument("--repeats", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mix_modes_bench.log"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the device"
    dev = torch.device("cuda:0")
    libs = {"this": _lib.lib()}
    if args.parent_lib:
        libs["parent"] = _lib.bind(ctypes.CDLL(args.parent_lib), lenient=True)
    st = _lib.stream()
    lines = [f"# {torch.cuda.get_device_name(0)}; {args.repeats} repeats of {args.iters} calls per form (first {args.warmup} dropped), forms "
             f"alternating; microseconds per call, device events; libraries: {', '.join(libs)}"]

    # (i) + (ii) the input pass
    N, C, H, W = shape = (80, 3, 224, 224)
    n = N * C * H * W
    slots = 10  # 10 x (12 MB in + 24 MB out) = 361 MB: beyond the 256 MiB cache
    g = torch.Generator(device=dev).manual_seed(1)
    xs = [torch.randint(0, 256, shape, device=dev, dtype=torch.uint8, generator=g) for _ in range(slots)]
    ys = [torch.empty(shape, device=dev, dtype=torch.bfloat16) for _ in range(slots)]
    mean = torch.tensor([123.675, 116.28, 103.53], device=dev)
    std = torch.tensor([58.395, 57.12, 57.375], device=dev)
    bf16 = _lib.dtype_code(torch.bfloat16)
    lam = 0.37
    rng = np.random.default_rng(2)
    lams = rng.random(N).astype(np.float32) * np.float32(0.98) + np.float32(0.01)
    corners = np.stack([rng.integers(0, H - 112, N), rng.integers(0, W - 112, N)], axis=1)
    boxes = np.stack([corners[:, 0], corners[:, 0] + 112, corners[:, 1], corners[:, 1] + 112], axis=1)
    packer = PerSampleMixup(device="cpu", capacity=N)
    half = np.arange(N) % 2 == 1
    header = {"header mode 0": pack_params(0, 1.), "header mode 1 (mixup)": pack_params(1, lam),
              "header mode 2 (CutMix 112 x 112)": pack_params(2, 0.75, (50, 162, 37, 149))}
    tables = {"table, every sample mixup": packer.pack(lams, np.zeros(N, dtype=bool), boxes),
              "table, every sample CutMix": packer.pack(np.full(N, 0.75, dtype=np.float32), np.ones(N, dtype=bool), boxes),
              "table, mixup / CutMix 50 / 50": packer.pack(np.where(half, np.float32(0.75), lams), half, boxes)}

    def mix_form(L, blk):
        blk = blk.to(dev)

        def call(i):
            rc = L.cot_mix_normalize(P(xs[i % slots]), P(ys[i % slots]), P(mean), P(std), P(blk), N, C, H, W, bf16, st)
            assert rc == 0, L.cot_last_error()
        return call
    forms = {f"{k} [{which}]": mix_form(L, blk) for k, blk in header.items() for which, L in libs.items()}
    forms.update({f"{k} [this]": mix_form(libs["this"], blk) for k, blk in tables.items()})
    t = alternate(forms, args.repeats, args.warmup, args.iters)
    lines.append(f"(i) + (ii) input pass, {shape} uint8 -> bf16, {slots} rotating slots")
    for k, v in t.items():
        nbytes = n * (3 if "mode 0" in k else 4)
        lines.append(row(k, v) + f" | {nbytes / statistics.median(v) / 1e6:6.2f} TB/s")
    if "parent" in libs:
        lines.append("(i) header modes, this build against the parent's (margin: the parent's own min-max spread)")
        lines += [verdict(k, t[f"{k} [this]"], t[f"{k} [parent]"]) for k in header]
    lines.append("(ii) table mode against the header mode that moves the same bytes (this build; margin: the header form's min-max spread)")
    for k, ref in (("table, every sample mixup", "header mode 1 (mixup)"), ("table, every sample CutMix", "header mode 2 (CutMix 112 x 112)"),
                   ("table, mixup / CutMix 50 / 50", "header mode 1 (mixup)"), ("table, mixup / CutMix 50 / 50", "header mode 2 (CutMix 112 x 112)")):
        a, b = t[f"{k} [this]"], t[f"{ref} [this]"]
        med = statistics.median(a)
        lines.append(f"{k:>34s} | x{med / statistics.median(b):.4f} of {ref}; median {med:.2f} us "
                     f"{'inside' if min(b) <= med <= max(b) else 'OUTSIDE'} its spread [{min(b):.2f}, {max(b):.2f}]")

    # (iii) the loss, forward + backward
    B, K = 80, 1000
    logits = (3 * torch.randn(B, K, device=dev, generator=g)).bfloat16()
    labels = torch.randint(0, K, (B,), device=dev, generator=g)
    f32 = dict(dtype=torch.float32, device=dev)
    rows, lse, mean_loss, gout, dx = torch.empty(B, **f32), torch.empty(4 * B, **f32), torch.empty(1, **f32), torch.ones(1, **f32), torch.empty_like(logits)

    def loss_form(L, blk):
        blk = blk.to(dev)

        def call(_):
            rc = L.cot_soft_target_ce_forward(P(logits), P(labels), P(blk), 0.1, P(rows), P(lse), P(mean_loss), B, K, bf16, st)
            rc = rc or L.cot_soft_target_ce_backward(P(logits), P(labels), P(blk), 0.1, P(lse), P(gout), P(dx), B, K, bf16, st)
            assert rc == 0, L.cot_last_error()
        return call
    forms = {f"header block [{which}]": loss_form(L, pack_params(1, lam)) for which, L in libs.items()}
    forms["table block [this]"] = loss_form(libs["this"], tables["table, every sample mixup"])
    t = alternate(forms, args.repeats, args.warmup, args.iters)
    lines.append(f"(iii) loss forward + backward (three launches), B = {B}, K = {K}, bf16 logits, eager calls")
    lines += [row(k, v) for k, v in t.items()]
    if "parent" in libs:
        lines.append(verdict("header block", t["header block [this]"], t["header block [parent]"]))
    a, b = t["table block [this]"], t["header block [this]"]
    lines.append(f"{'table block':>34s} | x{statistics.median(a) / statistics.median(b):.4f} of the header block; median {statistics.median(a):.2f} us "
                 f"{'inside' if min(b) <= statistics.median(a) <= max(b) else 'OUTSIDE'} its spread [{min(b):.2f}, {max(b):.2f}]")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
