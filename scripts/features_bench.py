#!/usr/bin/env python
"""What a feature backbone costs on the MI355X next to the classifier model's own `forward_features`.

cotnet50, mixed bf16, training mode, forward + backward, each form captured once into a HIP graph and replayed; B = 16 at 3 x 512 x 512
and B = 80 at 3 x 224 x 224.  Three forms, each on its own copy of the same weights, alternating in one process:

    forward_features   the classifier model's forward_features, loss = (y.float() * w).sum() on its output
    backbone (4,)      create_model(..., features_only=True, out_indices=(4,)), the same loss on its one tap -- the same launches
    backbone all       out_indices = (0, 1, 2, 3, 4), the same kind of loss summed over the five taps

One repeat = `--iters` back-to-back replays of ONE form between two device events; the forms alternate repeat by repeat; the first
`--warmup` repeats of each are dropped; median and min-max per form (scripts/recipe_loss_bench.py's method).  The yardstick for (4,) is
forward_features in the same run: a ratio of medians outside that form's own min-max spread is marked OUTSIDE and is a finding to
explain, not a threshold.  Next to the times: the library launches of one forward + backward per form (a dry run, cot_launch_log -- the
log is per thread, so the backward's part is drained by a hook that runs on the autograd thread), the node kinds that ran
(cot_layer_fused.NODE_COUNTS) and the module fallbacks (_lib.FALLBACKS) -- where a geometry no node covers would first show.
Writes profiles/features_bench.log.

    python scripts/features_bench.py [--repeats 15] [--iters 5]
"""
import argparse
import copy
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import cotnet_amd  # noqa: E402
from cotnet_amd import _lib, cot_layer_fused as clf  # noqa: E402
from cotnet_amd.features import FeatureListNet, load_classifier_state_dict  # noqa: E402
from cotnet_amd.flat_sgd import to_mixed_bf16  # noqa: E402
from scripts.recipe_loss_bench import alternate, row  # noqa: E402


class Form:
    def __init__(self, name, model, run, x):
        self.name, self.model, self.run, self.x = name, model, run, x
        self.w = None
        self.graph = None

    def step(self):
        self.model.zero_grad(set_to_none=True)
        outs = self.run(self.model, self.x)
        if self.w is None:
            g = torch.Generator(device=self.x.device).manual_seed(3)
            self.w = [torch.randn(t.shape, device=t.device, generator=g) for t in outs]
        loss = sum((t.float() * w).sum() for t, w in zip(outs, self.w))
        loss.backward()
        return loss

    def launches(self):
        """library launches of one forward + backward (dry run: nothing is launched by the library; what torch computes next to it is
        garbage and is thrown away).  The forward's lines are on this thread, the backward's on the autograd thread: a hook on the
        stem's weight gradient -- the last the backward produces -- drains those; one throw-away pass first, so that what the
        backward issues behind that hook is counted in the next pass, alike for every pass."""
        L = _lib.lib()
        buf = ctypes.create_string_buffer(1 << 22)
        seen = []

        def drain(_=None):
            L.cot_launch_log(buf, len(buf))
            seen.append(sum(1 for ln in buf.value.decode().splitlines() if ln))

        stem = next(p for p in self.model.parameters())
        handle = stem.register_hook(drain)
        counts = []
        with _lib.tuned(L, DRY_RUN=1):
            for _ in range(2):
                del seen[:]
                drain()
                del seen[:]
                self.step()
                drain()
                counts.append(sum(seen))
        handle.remove()
        self.model.zero_grad(set_to_none=True)
        return counts[-1]


def measure(shape, args, s, lines):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    base = cotnet_amd.create_model("cotnet50")
    with torch.no_grad():
        for m in base.modules():
            if hasattr(m, "bn3") and hasattr(m, "conv3"):
                m.bn3.weight.fill_(0.5)
    sd = base.state_dict()

    def backbone(idx):
        b = FeatureListNet(copy.deepcopy(base), out_indices=idx)
        load_classifier_state_dict(b, sd)
        return b
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(shape, device=dev, generator=g).bfloat16()
    forms = [Form("forward_features", copy.deepcopy(base), lambda m, t: [m.forward_features(t)], x),
             Form("backbone (4,)", backbone((4,)), lambda m, t: m(t), x),
             Form("backbone all five taps", backbone((0, 1, 2, 3, 4)), lambda m, t: m(t), x)]
    lines.append(f"== cotnet50, mixed bf16, train, forward + backward, replayed; input {tuple(shape)}")
    for f in forms:
        f.model = to_mixed_bf16(f.model.to(dev)).train()
        _lib.FALLBACKS.clear()
        for i in range(3):  # eager warm-up (and what the capture needs: caches filled, AccumulateGrad nodes made on this stream)
            clf.reset_node_counts()
            f.step()
        nodes = {k: v for k, v in clf.NODE_COUNTS.items() if v}
        fallbacks = {k: v // 3 for k, v in dict(_lib.FALLBACKS).items()}
        torch.cuda.synchronize()
        try:
            n_launch = f.launches()
        except Exception as e:  # noqa: BLE001  (a diagnostic next to the measurement: say so and go on)
            n_launch = f"unavailable ({type(e).__name__}: {e})"
        f.step()
        torch.cuda.synchronize()
        f.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(f.graph, stream=s):
            f.loss = f.step()
        f.graph.replay()
        torch.cuda.synchronize()
        lines.append(f"{f.name:>34s} | library launches per forward + backward {n_launch}; NODE_COUNTS {nodes}; module_fallbacks per step {fallbacks}; "
                     f"loss {float(f.loss.detach()):.6g}")
    assert float(forms[0].loss.detach()) == float(forms[1].loss.detach()), "forward_features and the (4,) backbone disagree"
    t = alternate({f.name: (lambda i, f=f: f.graph.replay()) for f in forms}, args.repeats, args.warmup, args.iters)
    lines += [row(k, v) for k, v in t.items()]
    ref = t["forward_features"]
    for k in ("backbone (4,)", "backbone all five taps"):
        med = statistics.median(t[k])
        lines.append(f"{k:>34s} | x{med / statistics.median(ref):.4f} of forward_features; median {med:.2f} us "
                     f"{'inside' if min(ref) <= med <= max(ref) else 'OUTSIDE'} its spread [{min(ref):.2f}, {max(ref):.2f}]")
    for f in forms:
        del f.graph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "features_bench.log"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the device"
    lines = [f"# {torch.cuda.get_device_name(0)}; {args.repeats} repeats of {args.iters} replays per form (first {args.warmup} dropped), forms "
             "alternating; microseconds per replayed forward + backward, device events"]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for shape in ((16, 3, 512, 512), (80, 3, 224, 224)):
            measure(shape, args, s, lines)
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
    torch.cuda.current_stream().wait_stream(s)
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
