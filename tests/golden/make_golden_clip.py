"""Fixture for gradient clipping by global norm (csrc/grad_clip.hip, FlatSGD(clip_grad=...)), recorded from the reference's own code.

    python tests/golden/make_golden_clip.py /path/to/reference

loads the reference's `utils/clip_grad.py` where it lies, by file path (it imports only torch), calls
`dispatch_clip_grad(parameters, value, mode='norm')` -- what its training step calls between backward and optimizer.step() -- on the CPU
and writes DATA only, tests/golden/grad_clip.npz.  Per seeded gradient set (three fp32 tensors of shapes (8, 4, 3, 3), (8,) and (5, 8),
scaled so that the sets' norms differ by orders of magnitude):

  {set}__g0, g1, g2           the gradients as drawn
  {set}__total_norm           the norm the reference's call returns (fp32), the same for every max_norm
  {set}__max_norms            the values clipped to: fractions and multiples of the norm (both sides of it) and 1.0
  {set}__clipped{j}_g0 ..     the gradients the call left in `.grad` for max_norms[j]

The .npz is written with fixed zip timestamps: a second run gives the same bytes.
"""
import importlib.util
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(8, 4, 3, 3), (8,), (5, 8)]
SETS = [("unit", 11, 1.0), ("small", 12, 1e-3), ("large", 13, 40.0)]  # name, seed, scale of the standard normal draw
FACTORS = [0.25, 0.999, 1.001, 4.0]  # max_norm = factor * norm: two that clip, two that do not


def load_dispatch(ref):
    spec = importlib.util.spec_from_file_location("ref_clip_grad", os.path.join(ref, "utils", "clip_grad.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.dispatch_clip_grad


def write_npz(path, arrays):
    """np.savez_compressed with the zip members' timestamps fixed, so that the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def clip(dispatch, grads, value):
    """the reference's call on fresh parameters carrying `grads`; returns what it left in `.grad`"""
    params = [torch.nn.Parameter(torch.zeros_like(g)) for g in grads]
    for p, g in zip(params, grads):
        p.grad = g.clone()
    dispatch(params, value, mode="norm")
    return [p.grad.clone() for p in params]


def main(ref):
    dispatch = load_dispatch(ref)
    out = {}
    for name, seed, scale in SETS:
        rng = np.random.Generator(np.random.PCG64(seed))
        grads = [torch.from_numpy(scale * rng.standard_normal(s)).float() for s in SHAPES]
        # the norm as the reference's call computes it (clip_grad_norm_ returns it; dispatch_clip_grad drops the return value)
        params = [torch.nn.Parameter(torch.zeros_like(g)) for g in grads]
        for p, g in zip(params, grads):
            p.grad = g.clone()
        norm = torch.nn.utils.clip_grad_norm_(params, float("inf"), norm_type=2.0)
        assert all(torch.equal(p.grad, g) for p, g in zip(params, grads))
        max_norms = [float(np.float32(f * float(norm))) for f in FACTORS] + [1.0]
        for i, g in enumerate(grads):
            out[f"{name}__g{i}"] = g.numpy()
        out[f"{name}__total_norm"] = norm.numpy()
        out[f"{name}__max_norms"] = np.array(max_norms, dtype=np.float64)
        for j, v in enumerate(max_norms):
            for i, g in enumerate(clip(dispatch, grads, v)):
                out[f"{name}__clipped{j}_g{i}"] = g.numpy()
        print(name, "norm", float(norm), "max_norms", max_norms)
    path = os.path.join(HERE, "grad_clip.npz")
    write_npz(path, out)
    print("grad_clip.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
