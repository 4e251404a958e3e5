"""Fixture for fused AdamW (csrc/adamw.hip, FlatAdamW), recorded from the reference's own optimizer.

    python tests/golden/make_golden_adamw.py /path/to/reference

loads the reference's `optim/adamw.py` where it lies, by file path (it imports only math and torch; on a current torch its in-place calls
raise a deprecation warning and compute the same), steps four fp32 parameters of shapes (8, 4, 3, 3), (8,), (5, 8) and (6, 147) in the
reference's two groups -- the vector without weight decay, the others with 0.05 -- at lr 1e-2 on the CPU and writes DATA only,
tests/golden/adamw.npz.  Every gradient has elements that are exactly zero.  Steps 1, 2 and 3 follow each other; for step 1000 the state
dict of the optimizer after step 3 is loaded back with every `step` set to 999.

  hp               lr, beta1, beta2, eps as float64
  wd               the weight decay of each parameter's group
  steps            [1, 2, 3, 1000]
  p{i}             the parameters before step 1 (both moments are zero there)
  s{t}_g{i}        the gradient of step t
  s{t}_p{i}, s{t}_m{i}, s{t}_v{i}    parameter, exp_avg and exp_avg_sq AFTER step t

The state before step 2 is the state after step 1, and so on; before step 1000 it is the state after step 3.  About 80 KB: the shapes
are the other fixtures' (the stem's rows of 147 among them).  Written with fixed zip timestamps: a second run gives the same bytes.
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
LR, BETAS, EPS, WD = 1e-2, (0.9, 0.999), 1e-8, 0.05
STEPS = [1, 2, 3, 1000]


def load_adamw(ref):
    spec = importlib.util.spec_from_file_location("ref_adamw", os.path.join(ref, "optim", "adamw.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.AdamW


def main(ref):
    AdamW = load_adamw(ref)
    rng = np.random.Generator(np.random.PCG64(33))
    params = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(s)).float()) for s in SHAPES]
    groups = [dict(params=[params[i] for i in NO_DECAY], weight_decay=0.0),
              dict(params=[p for i, p in enumerate(params) if i not in NO_DECAY], weight_decay=WD)]
    opt = AdamW(groups, lr=LR, betas=BETAS, eps=EPS)
    out = {"hp": np.array([LR, BETAS[0], BETAS[1], EPS]), "wd": np.array([0.0 if i in NO_DECAY else WD for i in range(len(SHAPES))]),
           "steps": np.array(STEPS)}
    for i, p in enumerate(params):
        out[f"p{i}"] = p.detach().clone().numpy()
    for t in STEPS:
        if t == 1000:
            sd = opt.state_dict()
            for s in sd["state"].values():
                assert s["step"] == 3
                s["step"] = 999
            opt.load_state_dict(sd)
        for i, p in enumerate(params):
            g = torch.from_numpy(rng.standard_normal(SHAPES[i])).float() * (0.1 if i == 3 else 1.0)
            g.reshape(-1)[torch.from_numpy(rng.permutation(g.numel())[:max(2, g.numel() // 7)])] = 0.0
            p.grad = g
            out[f"s{t}_g{i}"] = g.clone().numpy()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            opt.step()
        for i, p in enumerate(params):
            st = opt.state[p]
            assert st["step"] == t
            out[f"s{t}_p{i}"] = p.detach().clone().numpy()
            out[f"s{t}_m{i}"] = st["exp_avg"].clone().numpy()
            out[f"s{t}_v{i}"] = st["exp_avg_sq"].clone().numpy()
            assert int((out[f"s{t}_g{i}"] == 0).sum()) >= 2
    path = os.path.join(HERE, "adamw.npz")
    write_npz(path, out)
    print("adamw.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
