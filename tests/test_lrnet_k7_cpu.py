"""LR-Net's 7x7 window on the host: the `lrnet50_k7` builder, the wrapper's routing of CPU tensors, the reference's own
SelfAttLayer(dim, 7, key_ks) fixtures (tests/golden/make_golden_lrnet_k7.py) through the composition, and the check that sets the input
scale of tests/lr_k7_cases.py.  As in test_lrnet_cpu.py the aggregation runs on the unfold oracle: the product has no CPU path."""
import json
import os

import pytest
import torch

import cotnet_amd
import cotnet_amd.local_relation as lrmod
from cotnet_amd import lr_net
from cotnet_amd.local_relation import local_relation, local_relation_reference
from tests import lr_k7_cases as L7
from tests.conftest import GOLDEN, load_golden
from tests.test_lrnet_cpu import oracle_aggregation, run_layer  # noqa: F401  (the fixture is used by name)

LAYER = ["lrnet_k7_layer_d32_k1", "lrnet_k7_layer_d32_k3", "lrnet_k7_layer_d64_7x7_k1", "lrnet_k7_layer_d64_7x7_k3"]


def layer_from_fixture(gold, dtype):
    meta = json.loads(str(gold["meta"]))
    assert meta["kernel_size"] == 7
    layer = lr_net.SelfAttLayer(meta["dim"], 7, meta["key_ks"])
    layer.load_state_dict({k[4:]: torch.from_numpy(gold[k]) for k in gold if k.startswith("sd__")}, strict=True)
    return meta, layer.to(dtype)


def test_registry_has_the_k7_entrypoint_and_keeps_the_reference_ones():
    names = cotnet_amd.list_models()
    assert "lrnet50_k7" in names and "lrnet50" in names and "lrnet50_ks3" in names
    assert "not a reference entry point" in " ".join(lr_net.lrnet50_k7.__doc__.lower().split())


def test_k7_model_layout():
    m = cotnet_amd.create_model("lrnet50_k7", num_classes=7)
    assert [len(s) for s in (m.layer1, m.layer2, m.layer3, m.layer4)] == [3, 4, 6, 3] and m.fc.out_features == 7
    for stage, width in ((m.layer1, 64), (m.layer2, 128), (m.layer3, 256), (m.layer4, 512)):
        for blk in stage:
            assert isinstance(blk, lr_net.Bottleneck_K7)
            layer = blk.conv2
            assert layer.kernel_size == 7 and layer.head_num == width // 8 and layer.conv_k[0].kernel_size == (1, 1)
            assert tuple(layer.pos_h.shape) == (width, 7, 1) and tuple(layer.pos_w.shape) == (width, 1, 7)
    # the same tensors as lrnet50 in the same order; only the position tables are wider
    ref = {k: list(v.shape) for k, v in cotnet_amd.create_model("lrnet50", num_classes=7).state_dict().items()}
    mine = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert list(mine) == list(ref)
    assert {k for k in ref if mine[k] != ref[k]} == {k for k in ref if k.endswith(("pos_h", "pos_w"))}


def test_lrnet50_state_dict_keys_are_unchanged():
    ref = json.load(open(os.path.join(GOLDEN, "lrnet_state_dict_keys.json")))
    for name in ("lrnet50", "lrnet50_ks3"):
        m = cotnet_amd.create_model(name)
        assert {k: list(v.shape) for k, v in m.state_dict().items()} == ref[name]
        assert list(m.state_dict()) == list(ref[name])


def test_geometry_and_cache_key_carry_the_window():
    q = torch.zeros(2, 16, 5, 6)
    g7, g3 = lrmod._geom(q, 7), lrmod._geom(q, 3)
    assert (g7.kh, g7.kw, g7.ph, g7.pw, g7.wC, g7.heads) == (7, 7, 3, 3, 2, 1)
    assert (g3.kh, g3.kw, g3.ph, g3.pw, g3.wC, g3.heads) == (3, 3, 1, 1, 2, 1)
    assert not lrmod.fusable(q, q, q, 7) and not lrmod.fusable(q, q, q, 5)  # CPU tensors: the composition


@pytest.mark.parametrize("ks", [5, 7])
def test_cpu_tensors_take_the_composition(ks, oracle_aggregation, monkeypatch):  # noqa: F811
    monkeypatch.setattr(lrmod._LocalRelation, "apply", lambda *a: pytest.fail("the fused Function was called for CPU tensors"))
    g = torch.Generator().manual_seed(ks)
    q, k, v = (torch.randn(2, 16, 4, 5, generator=g, dtype=torch.float64) for _ in range(3))
    pos_h, pos_w = (torch.randn(s, generator=g, dtype=torch.float64) for s in ((16, ks, 1), (16, 1, ks)))
    before = dict(cotnet_amd._lib.FALLBACKS)
    out = local_relation(q, k, v, pos_h, pos_w, ks)
    assert dict(cotnet_amd._lib.FALLBACKS) == before  # not a module fallback: there is no CPU kernel to fall back from
    want = L7.reference64(q, k, v, (pos_h + pos_w).reshape(16, ks * ks), torch.ones_like(q), ks)[0]
    assert torch.allclose(out, want, atol=1e-12)


def test_fp32_composition_stays_inside_the_fp32_bound(oracle_aggregation, capsys):  # noqa: F811
    """what fixes the input scale of the directed cases: the reference's composition, evaluated in fp32 on the CPU over every directed
    input, must itself meet the fp32 tolerances against the fp64 checker -- else the inputs, not the bound, would have to change"""
    report = {}
    for case in L7.DIRECTED + [(2, 16, 3, L7.boundary_width())]:
        N, C, H, W = case
        q, k, v, gout, pos = L7.inputs(N, C, H, W, torch.float32, seed=sum(case))
        qa, ka, va, pa = (t.clone().requires_grad_(True) for t in (q, k, v, pos))
        out = local_relation_reference(qa, ka, va, pa.view(C, 7, 7), torch.zeros(C, 1, 1), 7)
        out.backward(gout)
        bad = L7.mismatches((out, qa.grad, ka.grad, va.grad, pa.grad), L7.reference64(q, k, v, pos, gout), torch.float32, report)
        assert not bad, (case, bad)
    with capsys.disabled():
        print("\nfp32 composition, worst ratio to the fp32 bound: " + ", ".join(f"{k} {v:.3f}" for k, v in report.items()))


@pytest.mark.parametrize("name", LAYER)
@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_layer_matches_the_reference_fixture(name, mode, dtype, oracle_aggregation):  # noqa: F811
    gold = load_golden(name)
    _, layer = layer_from_fixture(gold, dtype)
    x, gout = torch.from_numpy(gold["x"]).to(dtype), torch.from_numpy(gold["gout"]).to(dtype)
    got = run_layer(layer, x, gout, mode)
    sfx = "_f64" if dtype == torch.float64 else ""
    for key, t in got.items():
        ref = torch.from_numpy(gold[f"{mode}_{key}{sfx}"]).to(dtype)
        scale = max(1.0, ref.abs().max().item())
        assert (t - ref).abs().max().item() <= 1e-3 * scale, (key, (t - ref).abs().max().item(), scale)
