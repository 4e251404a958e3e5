"""LR-Net host-side logic on CPU: registry, state_dict contract and module wiring against fixtures made by the reference's own
models/lr_net.py (tests/golden/make_golden_lrnet.py).  As in test_models_cpu.py, the aggregation runs on the ORACLE (the
reference's nn.Unfold formula) because the product has no CPU path; the GPU twins are in test_lrnet_gpu.py."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cotnet_amd
from cotnet_amd import lr_net
from cotnet_amd.local_relation import local_relation, local_relation_reference
from oracle import unfold_oracle
from tests.conftest import GOLDEN, K_GRAD, K_OUT, load_golden, rng_tensor, sample_idx

LAYER = ["lrnet_layer_d32_k1", "lrnet_layer_d32_k3", "lrnet_layer_d64_7x7_k1", "lrnet_layer_d64_7x7_k3"]
REAL = ["lrnet_layer_s1_64x56", "lrnet_layer_s2_128x28", "lrnet_layer_s3_256x14", "lrnet_layer_s4_512x7"]
MODELS = ["lrnet50", "lrnet50_ks3"]
GRADS = {"g_convq_w": lambda m: m.conv_q[0].weight.grad, "g_convk_w": lambda m: m.conv_k[0].weight.grad,
         "g_convv_w": lambda m: m.conv_v[0].weight.grad, "g_pos_h": lambda m: m.pos_h.grad, "g_pos_w": lambda m: m.pos_w.grad,
         "g_bn_w": lambda m: m.bn.weight.grad}


@pytest.fixture
def oracle_aggregation(monkeypatch):
    import cotnet_amd.aggregation_zeropad as az

    def agg(input, weight, kernel_size=3, stride=1, padding=0, dilation=1):
        return unfold_oracle.aggregation_unfold(input, weight, kernel_size, stride, padding, dilation)

    monkeypatch.setattr(az, "aggregation_zeropad", agg)


def layer_from_fixture(gold, dtype):
    meta = json.loads(str(gold["meta"]))
    layer = lr_net.SelfAttLayer(meta["dim"], 3, meta["key_ks"])
    layer.load_state_dict({k[4:]: torch.from_numpy(gold[k]) for k in gold if k.startswith("sd__")}, strict=True)
    return meta, layer.to(dtype)


def run_layer(layer, x, gout, mode):
    layer.train(mode == "train")
    layer.zero_grad()
    xin = x.clone().requires_grad_(True)
    y = layer(xin)
    y.backward(gout)
    return {"y": y.detach(), "gx": xin.grad, **{k: f(layer) for k, f in GRADS.items()}}


def seeded_real_layer(gold):
    """same seed + same construction order -> the reference's initial weights (checked against the fixture's fp64 sums); norm
    state and inputs drawn from the stored numpy seed exactly as make_golden_lrnet drew them"""
    meta = json.loads(str(gold["meta"]))
    seed = int(gold["seed"])
    rng = np.random.Generator(np.random.PCG64(seed))
    torch.manual_seed(seed)
    layer = lr_net.SelfAttLayer(meta["dim"], 3, meta["key_ks"]).float()
    for m in layer.modules():  # make_golden.randomize_norm_state
        if isinstance(m, torch.nn.BatchNorm2d):
            with torch.no_grad():
                m.weight.copy_(torch.from_numpy(1.0 + 0.2 * rng.standard_normal(m.weight.shape)).float())
                m.bias.copy_(torch.from_numpy(0.1 * rng.standard_normal(m.bias.shape)).float())
                m.running_mean.copy_(torch.from_numpy(0.1 * rng.standard_normal(m.running_mean.shape)))
                m.running_var.copy_(torch.from_numpy(1.0 + 0.2 * rng.random(m.running_var.shape)))
    for k, v in layer.state_dict().items():
        if v.is_floating_point():
            want = meta["probe"][k]
            assert abs(float(v.double().sum()) - want) <= 1e-6 * max(1.0, abs(want)), f"weights differ from the reference's: {k}"
    x = rng_tensor(rng, (meta["B"], meta["dim"], meta["H"], meta["W"]), torch.float32)
    gout = rng_tensor(rng, (meta["B"], meta["dim"], meta["H"], meta["W"]), torch.float32)
    return meta, layer, x, gout


def check_compact(gold, mode, got, tol):
    for key, t in got.items():
        flat = t.detach().double().cpu().reshape(-1)
        idx = sample_idx(flat.numel(), K_OUT if key in ("y", "gx") else K_GRAD)
        scale = max(1.0, float(gold[f"{mode}_{key}_absmax"]))
        err = (flat[idx] - torch.from_numpy(gold[f"{mode}_{key}"]).double()).abs().max().item()
        assert err <= tol * scale, (mode, key, err, scale)
        dsum = abs(flat.sum().item() - float(gold[f"{mode}_{key}_sum"]))
        assert dsum <= tol * scale * max(1.0, flat.numel() ** 0.5), (mode, key, "sum", dsum)


def test_registry_has_both_lrnet_entrypoints():
    names = cotnet_amd.list_models()
    assert "lrnet50" in names and "lrnet50_ks3" in names
    m = cotnet_amd.create_model("lrnet50", num_classes=7)
    assert m.default_cfg["first_conv"] == "conv1" and m.fc.out_features == 7
    assert lr_net.default_cfgs["lrnet_basic"]["input_size"] == (3, 224, 224)


@pytest.mark.parametrize("name", MODELS)
def test_state_dict_keys_shapes_and_order_equal_reference(name):
    ref = json.load(open(os.path.join(GOLDEN, "lrnet_state_dict_keys.json")))[name]
    m = cotnet_amd.create_model(name)
    mine = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert list(mine.keys()) == list(ref.keys())
    assert mine == ref


def test_self_att_layer_attributes():
    layer = lr_net.SelfAttLayer(64, 3, 3)
    assert layer.head_num == 8 and layer.kernel_size == 3
    assert layer.conv_k[0].kernel_size == (3, 3) and layer.conv_k[0].padding == (1, 1)
    assert tuple(layer.pos_h.shape) == (64, 3, 1) and tuple(layer.pos_w.shape) == (64, 1, 3)
    assert isinstance(layer.local_conv, cotnet_amd.LocalConvolution) and layer.softmax.dim == 2
    blk = lr_net.Bottleneck_Ks3(256, 64, stride=2)
    assert blk.conv2.conv_k[0].kernel_size == (3, 3) and blk.avd is not None


@pytest.mark.parametrize("name", LAYER)
@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_layer_wiring_matches_reference_fixture(name, mode, dtype, oracle_aggregation):
    gold = load_golden(name)
    _, layer = layer_from_fixture(gold, dtype)
    x, gout = torch.from_numpy(gold["x"]).to(dtype), torch.from_numpy(gold["gout"]).to(dtype)
    got = run_layer(layer, x, gout, mode)
    sfx, tol = ("_f64", 1e-9) if dtype == torch.float64 else ("", 2e-4)
    for key, t in got.items():
        ref = torch.from_numpy(gold[f"{mode}_{key}{sfx}"]).to(dtype)
        scale = max(1.0, ref.abs().max().item())
        assert (t - ref).abs().max().item() <= tol * scale, (key, (t - ref).abs().max().item(), scale)


@pytest.mark.parametrize("name", REAL)
def test_layer_wiring_at_the_stage_geometries(name, oracle_aggregation):
    gold = load_golden(name)
    _, layer, x, gout = seeded_real_layer(gold)
    for mode in ("eval", "train"):
        check_compact(gold, mode, run_layer(layer, x, gout, mode), 1e-3)


@pytest.mark.parametrize("name", MODELS)
def test_model_wiring_matches_reference_fixture_fp64(name, oracle_aggregation):
    gold = load_golden(f"lrnet_model_{name}")
    meta = json.loads(str(gold["meta"]))
    torch.manual_seed(int(gold["seed"]))
    m = cotnet_amd.create_model(name, num_classes=meta["num_classes"], zero_init_last_bn=False).double()
    sd = m.state_dict()
    for k, want in meta["probe"].items():  # same construction order = the reference's initial weights
        assert abs(float(sd[k].double().sum()) - want) <= 1e-9 * max(1.0, abs(want)), k
    rng = np.random.Generator(np.random.PCG64(int(gold["seed"])))
    x = rng_tensor(rng, (2, 3, meta["size"], meta["size"]), torch.float64)
    with torch.no_grad():
        for key, mode in (("logits", False), ("logits_train", True)):
            y = m.train(mode)(x)
            ref = torch.from_numpy(gold[key])
            assert ((y - ref).abs().max() / ref.abs().max()).item() < 1e-7, key


def test_padded_taps_keep_their_logit_and_mass(oracle_aggregation):
    """k = 0 everywhere: every logit is sum_j q pos, INCLUDING the taps outside the image (unfold pads k, not the logit), so
    a corner pixel spreads probability over all nine taps and only the in-image ones (where v is not zero) contribute"""
    torch.manual_seed(0)
    B, C, H, W = 1, 16, 4, 5
    q, v = torch.randn(B, C, H, W, dtype=torch.float64), torch.randn(B, C, H, W, dtype=torch.float64)
    k = torch.zeros_like(q)
    pos_h, pos_w = torch.randn(C, 3, 1, dtype=torch.float64), torch.randn(C, 1, 3, dtype=torch.float64)
    out = local_relation(q, k, v, pos_h, pos_w, 3)
    G = C // 8
    pos = (pos_h + pos_w).reshape(C, 9)
    logit = torch.einsum("bgjhw,gjt->bgthw", q.view(B, G, 8, H, W), pos.view(G, 8, 9))
    a = torch.softmax(logit, dim=2)  # over all nine taps, padded ones included
    uv = F.unfold(v, 3, 1, 1, 1).view(B, C, 9, H, W)
    want = torch.einsum("bgthw,bjgthw->bjghw", a, uv.view(B, 8, G, 9, H, W)).reshape(B, C, H, W)  # channel c = g + j G
    assert torch.allclose(out, want, atol=1e-12)
    # the corner's in-image taps alone do NOT sum to one: the padded taps took their share
    assert a[0, :, [4, 5, 7, 8], 0, 0].sum(1).max().item() < 1 - 1e-3
    assert torch.allclose(local_relation_reference(q, k, v, pos_h, pos_w, 3), out)
