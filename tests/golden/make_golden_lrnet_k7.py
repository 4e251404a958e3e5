"""tests/golden/make_golden_lrnet_k7.py -- fixtures of the reference's own SelfAttLayer(dim, 7, key_ks) (models/lr_net.py), written next to
this file.

The machinery is make_golden.py's and make_golden_lrnet.py's, imported, not copied: the reference's package is imported with the CuPy /
yacs stubs, its `aggregation_zeropad` runs the reference's own kernels compiled for the CPU, and the layer is the reference's module code,
unmodified -- only the window argument is 7, LR-Net's own, which none of the reference's builders passes.  Writes

    lrnet_k7_layer_<case>.npz        weights, x, gout and the fp32 results (y, gx, parameter gradients), eval and train
    lrnet_k7_layer_<case>.part2.npz  the fp64 results (every committed file stays under 1 MiB)

    python tests/golden/make_golden_lrnet_k7.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
import make_golden_lrnet as mgl  # noqa: E402

WINDOW = 7
LAYER_CASES = [
    # name, dim, B, H, W, key_ks, seed
    ("d32_k1", 32, 2, 10, 10, 1, 171),
    ("d32_k3", 32, 2, 10, 10, 3, 172),
    ("d64_7x7_k1", 64, 2, 7, 7, 1, 173),
    ("d64_7x7_k3", 64, 2, 7, 7, 3, 174),
]
LIMIT = 1 << 20


def make_layer_fixtures(ref_lr):
    for name, dim, B, H, W, key_ks, seed in LAYER_CASES:
        rng = np.random.Generator(np.random.PCG64(seed))
        torch.manual_seed(seed)
        layer = ref_lr.SelfAttLayer(dim, WINDOW, key_ks).float()
        mg.randomize_norm_state(layer, rng)
        state = {k: v.clone() for k, v in layer.state_dict().items()}
        x = mg.rng_tensor(rng, (B, dim, H, W), torch.float64)
        gout = mg.rng_tensor(rng, (B, dim, H, W), torch.float64)
        out = {}
        for mode in ("eval", "train"):
            for t, v in mgl.run(layer, state, x.float(), gout.float(), mode).items():
                out[f"{mode}_{t}"] = v.numpy().copy()
        layer64 = ref_lr.SelfAttLayer(dim, WINDOW, key_ks).double()
        state64 = {k: (v.double() if v.is_floating_point() else v) for k, v in state.items()}
        for mode in ("eval", "train"):
            for t, v in mgl.run(layer64, state64, x, gout, mode).items():
                out[f"{mode}_{t}_f64"] = v.numpy().copy()
        files = (f"lrnet_k7_layer_{name}.npz", f"lrnet_k7_layer_{name}.part2.npz")
        np.savez_compressed(os.path.join(HERE, files[0]), seed=np.int64(seed), x=x.numpy(), gout=gout.numpy(),
                            meta=json.dumps(dict(dim=dim, B=B, H=H, W=W, key_ks=key_ks, kernel_size=WINDOW)),
                            **{"sd__" + k: v.numpy() for k, v in state.items()},
                            **{k: v for k, v in out.items() if not k.endswith("_f64")})
        np.savez_compressed(os.path.join(HERE, files[1]), **{k: v for k, v in out.items() if k.endswith("_f64")})
        sizes = [os.path.getsize(os.path.join(HERE, f)) for f in files]
        assert max(sizes) < LIMIT, sizes
        print(f"lrnet_k7_layer_{name}: " + " + ".join(f"{s / 1e3:.0f} KB" for s in sizes))


if __name__ == "__main__":
    assert mg.build_ref.reference_available(), "the reference checkout is required to regenerate fixtures"
    mg.import_reference_models()
    import models.lr_net as ref_lr  # (the reference's models/__init__.py imports it already)
    make_layer_fixtures(ref_lr)
