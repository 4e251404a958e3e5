"""tests/golden/make_golden_lrnet.py -- LR-Net fixtures FROM THE REFERENCE ITSELF (models/lr_net.py), written next to this file.

Same machinery as make_golden.py (imported, not copied): the reference's package is imported with the CuPy / yacs stubs and its
`aggregation_zeropad` runs the reference's own kernels compiled for the CPU.  Everything else -- SelfAttLayer, Bottleneck,
Bottleneck_Ks3, ResNet -- is the reference's module code, unmodified.  Writes only lrnet_* files:

    lrnet_layer_<case>[.part2].npz full fixtures of one SelfAttLayer (weights, x, gout, y, gx and the parameter gradients),
                                   eval and train, in fp32 and fp64
    lrnet_layer_s<i>_<C>x<H>.npz   compact fixtures at LR-Net-50's stage geometries (weights from the seed, sampled outputs)
    lrnet_model_<name>.npz         fp64 logits of lrnet50 / lrnet50_ks3 at 64 x 64
    lrnet_state_dict_keys.json     {entry point: {key: shape}} in the reference's order

    python tests/golden/make_golden_lrnet.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402

LAYER_CASES = [
    # name, dim, B, H, W, key_ks, seed
    ("d32_k1", 32, 2, 10, 10, 1, 71),
    ("d32_k3", 32, 2, 10, 10, 3, 72),
    ("d64_7x7_k1", 64, 2, 7, 7, 1, 73),
    ("d64_7x7_k3", 64, 2, 7, 7, 3, 74),
]
# LR-Net-50's attention layers see the stage input's resolution (avd pools after conv2, models/lr_net.py:170-171); B = 2
REAL_LAYER_CASES = [
    ("s1_64x56", 64, 2, 56, 56, 1, 81),
    ("s2_128x28", 128, 2, 28, 28, 1, 82),
    ("s3_256x14", 256, 2, 14, 14, 1, 83),
    ("s4_512x7", 512, 2, 7, 7, 1, 84),
]
MODEL_CASES = [("lrnet50", 64, 91), ("lrnet50_ks3", 64, 92)]


def grads(layer):
    return {"g_convq_w": layer.conv_q[0].weight.grad, "g_convk_w": layer.conv_k[0].weight.grad,
            "g_convv_w": layer.conv_v[0].weight.grad, "g_pos_h": layer.pos_h.grad, "g_pos_w": layer.pos_w.grad,
            "g_bn_w": layer.bn.weight.grad}


def run(layer, state, x, gout, mode):
    layer.load_state_dict(state)
    layer.train(mode == "train")
    layer.zero_grad()
    xin = x.clone().requires_grad_(True)
    y = layer(xin)
    y.backward(gout)
    return {"y": y.detach(), "gx": xin.grad, **grads(layer)}


def make_layer_fixtures(ref_lr):
    for name, dim, B, H, W, key_ks, seed in LAYER_CASES:
        rng = np.random.Generator(np.random.PCG64(seed))
        torch.manual_seed(seed)
        layer = ref_lr.SelfAttLayer(dim, 3, key_ks).float()
        mg.randomize_norm_state(layer, rng)
        state = {k: v.clone() for k, v in layer.state_dict().items()}
        x = mg.rng_tensor(rng, (B, dim, H, W), torch.float64)
        gout = mg.rng_tensor(rng, (B, dim, H, W), torch.float64)
        out = {}
        for mode in ("eval", "train"):
            for t, v in run(layer, state, x.float(), gout.float(), mode).items():
                out[f"{mode}_{t}"] = v.numpy().copy()
        layer64 = ref_lr.SelfAttLayer(dim, 3, key_ks).double()
        state64 = {k: (v.double() if v.is_floating_point() else v) for k, v in state.items()}
        for mode in ("eval", "train"):
            for t, v in run(layer64, state64, x, gout, mode).items():
                out[f"{mode}_{t}_f64"] = v.numpy().copy()
        # (every committed file stays under 1 MiB: the fp64 results go to a second part, merged by tests/conftest.load_golden)
        np.savez_compressed(os.path.join(HERE, f"lrnet_layer_{name}.npz"), seed=np.int64(seed), x=x.numpy(), gout=gout.numpy(),
                            meta=json.dumps(dict(dim=dim, B=B, H=H, W=W, key_ks=key_ks)),
                            **{"sd__" + k: v.numpy() for k, v in state.items()},
                            **{k: v for k, v in out.items() if not k.endswith("_f64")})
        np.savez_compressed(os.path.join(HERE, f"lrnet_layer_{name}.part2.npz"), **{k: v for k, v in out.items() if k.endswith("_f64")})
        print(f"lrnet_layer_{name}: " + " + ".join(f"{os.path.getsize(os.path.join(HERE, f)) / 1e3:.0f} KB" for f in
                                                   (f"lrnet_layer_{name}.npz", f"lrnet_layer_{name}.part2.npz")))


def make_real_layer_fixtures(ref_lr):
    """compact: the weights come from the seed (same construction order), outputs at sampled positions + fp64 sums"""
    for name, dim, B, H, W, key_ks, seed in REAL_LAYER_CASES:
        rng = np.random.Generator(np.random.PCG64(seed))
        torch.manual_seed(seed)
        layer = ref_lr.SelfAttLayer(dim, 3, key_ks).float()
        mg.randomize_norm_state(layer, rng)
        state = {k: v.clone() for k, v in layer.state_dict().items()}
        probe = {k: float(v.double().sum()) for k, v in state.items() if v.is_floating_point()}
        x = mg.rng_tensor(rng, (B, dim, H, W), torch.float32)
        gout = mg.rng_tensor(rng, (B, dim, H, W), torch.float32)
        out = {}
        for mode in ("eval", "train"):
            for key, t in run(layer, state, x, gout, mode).items():
                flat = t.detach().reshape(-1)
                idx = mg.sample_idx(flat.numel(), mg.K_OUT if key in ("y", "gx") else mg.K_GRAD)
                out[f"{mode}_{key}"] = flat[idx].numpy().copy()
                out[f"{mode}_{key}_sum"] = np.float64(flat.double().sum().item())
                out[f"{mode}_{key}_absmax"] = np.float64(flat.abs().max().item())
        np.savez_compressed(os.path.join(HERE, f"lrnet_layer_{name}.npz"), seed=np.int64(seed),
                            meta=json.dumps(dict(dim=dim, B=B, H=H, W=W, key_ks=key_ks, compact=True, probe=probe)), **out)
        print(f"lrnet_layer_{name}: {os.path.getsize(os.path.join(HERE, f'lrnet_layer_{name}.npz')) / 1e3:.0f} KB")


def make_model_fixtures(models):
    keys = {}
    for name, size, seed in MODEL_CASES:
        torch.manual_seed(0)
        m = models.create_model(name)
        keys[name] = {k: list(v.shape) for k, v in m.state_dict().items()}
        print(f"state_dict {name}: {len(keys[name])} tensors, {sum(p.numel() for p in m.parameters()) / 1e6:.2f} M params")
        # fp64 and zero_init_last_bn=False, as make_golden.make_model_fixtures
        torch.manual_seed(seed)
        m = models.create_model(name, num_classes=10, zero_init_last_bn=False).double()
        rng = np.random.Generator(np.random.PCG64(seed))
        x = mg.rng_tensor(rng, (2, 3, size, size), torch.float64)
        probe = {k: float(v.double().sum()) for k, v in list(m.state_dict().items())[:8]}
        probe.update({k: float(v.double().sum()) for k, v in m.state_dict().items() if k.endswith(("pos_h", "pos_w"))})
        with torch.no_grad():
            logits = m.eval()(x)
            logits_train = m.train()(x)
        np.savez_compressed(os.path.join(HERE, f"lrnet_model_{name}.npz"), logits=logits.numpy(),
                            logits_train=logits_train.numpy(), seed=np.int64(seed),
                            meta=json.dumps(dict(size=size, num_classes=10, probe=probe)))
        print(f"lrnet_model_{name}: logits {tuple(logits.shape)} |max| {logits.abs().max():.4f}")
    with open(os.path.join(HERE, "lrnet_state_dict_keys.json"), "w") as f:
        json.dump(keys, f)


if __name__ == "__main__":
    assert mg.build_ref.reference_available(), "the reference checkout is required to regenerate fixtures"
    models, _, _ = mg.import_reference_models()
    import models.lr_net as ref_lr  # (the reference's models/__init__.py imports it already)
    make_layer_fixtures(ref_lr)
    make_real_layer_fixtures(ref_lr)
    make_model_fixtures(models)
