"""Fixture for adaptive gradient clipping (csrc/agc.hip, FlatSGD(agc=...)), recorded from the reference's own code.

    python tests/golden/make_golden_agc.py /path/to/reference

loads the reference's `utils/clip_grad.py` where it lies, by file path (it imports only torch), calls
`dispatch_clip_grad(parameters, 0.01, mode='agc')` -- what its training step calls between backward and optimizer.step() -- on the CPU
and writes DATA only, tests/golden/agc.npz.  Four fp32 parameters of shapes (8, 4, 3, 3), (8,), (5, 8) and (6, 147) -- a convolution, a
BatchNorm vector that is all zeros (the reference's zero-initialised bn3.weight: one unit with a zero norm, clipped against eps * 0.01), a
classifier and the stem's rows of 147 -- with every unit's gradient scaled to 0.25, 0.8, 1.25 or 4 times the unit's max_norm in turn:

  w0 .. w3      the parameters
  g0 .. g3      the gradients as drawn and scaled
  out0 .. out3  the gradients the call left in `.grad`

The ratios are checked here, on the stored values in fp64, to be far from 1: the reference alone leaves no unit undecided.
The .npz is written with fixed zip timestamps: a second run gives the same bytes.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_clip import load_dispatch, write_npz  # noqa: E402

SHAPES = [(8, 4, 3, 3), (8,), (5, 8), (6, 147)]
ZEROS = 1  # the parameter that is all zeros
RATIOS = [0.25, 0.8, 1.25, 4.0]
FACTOR, EPS = 0.01, 1e-3  # the call's value and adaptive_clip_grad's default eps


def rows(t):
    """[units, elements per unit]: the reference's unitwise_norm"""
    return t.reshape(1, -1) if t.ndim <= 1 else t.reshape(t.shape[0], -1)


def main(ref):
    dispatch = load_dispatch(ref)
    rng = np.random.Generator(np.random.PCG64(21))
    out, unit = {}, 0
    params = []
    for i, shape in enumerate(SHAPES):
        w = torch.from_numpy(rng.standard_normal(shape)).float()
        if i == ZEROS:
            w.zero_()
        g = torch.from_numpy(rng.standard_normal(shape))
        max_norm = rows(w).double().norm(dim=1).clamp(min=EPS) * FACTOR
        want = torch.tensor([RATIOS[(unit + r) % len(RATIOS)] for r in range(rows(w).shape[0])], dtype=torch.float64) * max_norm
        g = (rows(g) * (want / rows(g).norm(dim=1))[:, None]).reshape(shape).float()
        ratio = rows(g).double().norm(dim=1) / max_norm
        assert bool(((ratio - 1).abs() > 0.1).all()), ratio  # decided by a wide margin: fp32 norms are good to ~1e-6
        unit += rows(w).shape[0]
        p = torch.nn.Parameter(w.clone())
        p.grad = g.clone()
        params.append(p)
        out[f"w{i}"], out[f"g{i}"] = w.numpy(), g.numpy()
    dispatch(params, FACTOR, mode="agc")
    clipped = 0
    for i, p in enumerate(params):
        assert torch.equal(p.detach(), torch.from_numpy(out[f"w{i}"]))
        out[f"out{i}"] = p.grad.detach().clone().numpy()
        clipped += int((rows(p.grad) != rows(torch.from_numpy(out[f"g{i}"]))).any(dim=1).sum())
    print(unit, "units,", clipped, "clipped by the reference")
    assert 0 < clipped < unit
    path = os.path.join(HERE, "agc.npz")
    write_npz(path, out)
    print("agc.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
