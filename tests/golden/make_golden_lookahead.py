"""Fixture for Lookahead on the flat optimizers (csrc/lookahead.hip, FlatSGD(lookahead_k=...)), recorded from the reference's own wrapper.

    python tests/golden/make_golden_lookahead.py /path/to/reference

loads the reference's `optim/lookahead.py` where it lies, by file path (it imports only torch; on a current torch its `add_(alpha, t)`
raises a deprecation warning and computes the same), wraps torch.optim.SGD(nesterov=True, momentum 0.9) over four fp32 parameters of
shapes (8, 4, 3, 3), (8,), (5, 8) and (6, 147) in the reference's two groups -- the vector without weight decay, the others with 4e-5
-- with k = 3, takes 7 steps and then calls sync_lookahead() once, on the CPU, and writes DATA only, tests/golden/lookahead.npz.  Run
once with alpha 0.5 and once with alpha 0.8 (tag a50 / a80), same parameters and gradients.

  hp                        k, lr, momentum, weight decay as float64
  alphas                    [0.5, 0.8]
  steps                     [1 .. 7]; the final sync_lookahead() is recorded as step 8
  {tag}_lookahead_step      the groups' lookahead_step after each of the 8 records (the last one repeats 7: a sync counts nothing)
  {tag}_s{t}_before{i}      the fast weights before step t
  {tag}_s{t}_after{i}       the fast weights after it
  {tag}_s{t}_slow{i}        the slow buffer after it, from the step at which it exists
  {tag}_s{t}_fast{i}        at the syncs (t = 3, 6, 8): the fast weights as update_slow found them, behind the base step

The generator asserts the reference's quirk: no slow buffer before step 3, nothing moves at step 3 (the buffer is created as a copy
and interpolated with itself), fast equals slow after steps 3 and 6 and after the final sync, and at no other step.  About 270 KB.
Written with fixed zip timestamps: a second run gives the same bytes.
"""
import importlib.util
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_clip import write_npz  # noqa: E402

SHAPES = [(8, 4, 3, 3), (8,), (5, 8), (6, 147)]
NO_DECAY = [1]
K, LR, MOMENTUM, WD = 3, 0.1, 0.9, 4e-5
ALPHAS = [0.5, 0.8]
STEPS = 7
SYNCS = [3, 6, 8]


def load_lookahead(ref):
    spec = importlib.util.spec_from_file_location("ref_lookahead", os.path.join(ref, "optim", "lookahead.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.Lookahead


def run(Lookahead, alpha, tag, out):
    rng = np.random.Generator(np.random.PCG64(57))
    params = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(s)).float()) for s in SHAPES]
    groups = [dict(params=[params[i] for i in NO_DECAY], weight_decay=0.0),
              dict(params=[p for i, p in enumerate(params) if i not in NO_DECAY], weight_decay=WD)]
    opt = Lookahead(torch.optim.SGD(groups, lr=LR, momentum=MOMENTUM, nesterov=True), alpha=alpha, k=K)
    found = {}
    inner = opt.update_slow

    def update_slow(group):  # what update_slow finds: the fast weights behind the base step
        for p in group["params"]:
            found[id(p)] = p.detach().clone().numpy()
        inner(group)
    opt.update_slow = update_slow
    counts = []
    for t in range(1, STEPS + 2):
        found.clear()
        for i, p in enumerate(params):
            out[f"{tag}_s{t}_before{i}"] = p.detach().clone().numpy()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            if t <= STEPS:
                for i, p in enumerate(params):
                    p.grad = torch.from_numpy(rng.standard_normal(SHAPES[i])).float() * (0.1 if i == 3 else 1.0)
                opt.step()
            else:
                opt.sync_lookahead()
        steps = {g["lookahead_step"] for g in opt.param_groups}
        assert steps == {min(t, STEPS)}, steps
        counts.append(min(t, STEPS))
        assert bool(found) == (t in SYNCS), (t, "update_slow ran at an unexpected step")
        for i, p in enumerate(params):
            out[f"{tag}_s{t}_after{i}"] = p.detach().clone().numpy()
            slow = opt.state[p].get("slow_buffer")
            assert (slow is not None) == (t >= K), (t, "the slow buffer is created at the first sync, not before")
            if slow is not None:
                out[f"{tag}_s{t}_slow{i}"] = slow.clone().numpy()
                assert torch.equal(slow, p.detach()) == (t in SYNCS), (t, i, "fast equals slow after a sync and only then")
            if t in SYNCS:
                out[f"{tag}_s{t}_fast{i}"] = found[id(p)]
            if t == K:
                assert np.array_equal(found[id(p)], out[f"{tag}_s{t}_after{i}"]), "the first sync moved a weight"
            if t in SYNCS[1:]:
                assert not np.array_equal(found[id(p)], out[f"{tag}_s{t}_after{i}"]), "a later sync moved nothing"
    out[f"{tag}_lookahead_step"] = np.array(counts)


def main(ref):
    Lookahead = load_lookahead(ref)
    out = {"hp": np.array([K, LR, MOMENTUM, WD], dtype=np.float64), "alphas": np.array(ALPHAS), "steps": np.arange(1, STEPS + 1)}
    for alpha in ALPHAS:
        run(Lookahead, alpha, f"a{round(alpha * 100)}", out)
    path = os.path.join(HERE, "lookahead.npz")
    write_npz(path, out)
    print("lookahead.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
