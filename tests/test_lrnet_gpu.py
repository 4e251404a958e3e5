"""LR-Net on the MI355X: the fused local-relation kernels (csrc/local_relation.hip) through the C ABI at every stage geometry of
LR-Net-50, the layer and model fixtures of the reference (tests/golden/make_golden_lrnet.py), mixed-precision training steps,
determinism and graph capture.  Run with `pytest -m gpu`."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cotnet_amd
import cotnet_amd.local_relation as lrmod
from cotnet_amd import _lib
from cotnet_amd.flat_sgd import to_mixed_bf16
from cotnet_amd.local_relation import local_relation, local_relation_reference
from tests.conftest import ROOT, load_golden, rng_tensor
from tests.test_lrnet_cpu import LAYER, MODELS, REAL, check_compact, layer_from_fixture, run_layer, seeded_real_layer

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
# (C, H) of LR-Net-50's attention layers: avd pools after conv2 (models/lr_net.py:170-171), so each stage's first layer runs at
# the previous stage's resolution
STAGES = [(64, 56), (128, 56), (128, 28), (256, 28), (256, 14), (512, 14), (512, 7)]


@pytest.fixture
def fused_calls(monkeypatch):
    """counts the calls that took the fused Function (and those that did not)"""
    calls = {"fused": 0, "other": 0}
    real = lrmod.fusable

    def spy(*a):
        ok = real(*a)
        calls["fused" if ok else "other"] += 1
        return ok
    monkeypatch.setattr(lrmod, "fusable", spy)
    return calls


def stage_inputs(C, H, dtype, seed, N=80):
    g = torch.Generator(device=DEV).manual_seed(seed)
    q, k = (0.5 * torch.randn(N, C, H, H, device=DEV, generator=g) for _ in range(2))
    v, gout = (torch.randn(N, C, H, H, device=DEV, generator=g) for _ in range(2))
    pos_h, pos_w = torch.randn(C, 3, 1, device=DEV, generator=g), torch.randn(C, 1, 3, device=DEV, generator=g)
    return [t.to(dtype) for t in (q, k, v, gout)] + [pos_h, pos_w]


def composition_grads(q, k, v, gout, pos_h, pos_w, dtype):
    """the reference's composition in `dtype` on the given operands, differentiated by autograd"""
    q, k, v = (t.detach().to(dtype).requires_grad_(True) for t in (q, k, v))
    ph, pw = (t.detach().to(dtype).requires_grad_(True) for t in (pos_h, pos_w))
    out = local_relation_reference(q, k, v, ph, pw, 3)
    out.backward(gout.to(dtype))
    return out.detach(), q.grad, k.grad, v.grad, (ph.grad, pw.grad)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C,H", STAGES)
def test_fused_op_at_the_stage_geometries(C, H, dtype):
    q, k, v, gout, pos_h, pos_w = stage_inputs(C, H, dtype, seed=C + H)
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    pha, pwa = pos_h.clone().requires_grad_(True), pos_w.clone().requires_grad_(True)
    y = local_relation(qa, ka, va, pha, pwa, 3)
    assert _lib.last_kernel() == "lr_fwd"
    y.backward(gout)
    assert "lr_bwd_rel" in _lib.last_kernel()
    torch.cuda.synchronize()
    # checker: the composition in fp64 (fp32 storage) / fp32 (bf16 storage) on the same rounded operands
    ref_dt = torch.float64 if dtype == torch.float32 else torch.float32
    r_y, r_gq, r_gk, r_gv, (r_gph, r_gpw) = composition_grads(q, k, v, gout, pos_h, pos_w, ref_dt)
    tol = 2e-5 if dtype == torch.float32 else 4e-2  # (tests/test_agg_gpu.py::test_fused_window_softmax)
    for name, got, want, f in (("y", y, r_y, 1), ("gv", va.grad, r_gv, 1), ("gq", qa.grad, r_gq, 4), ("gk", ka.grad, r_gk, 4)):
        err = (got.detach().to(ref_dt) - want).abs()
        bad = (err > f * tol * (1 + want.abs())).sum().item()
        assert bad == 0, (name, bad, err.max().item())
    for name, got, want in (("pos_h", pha.grad, r_gph), ("pos_w", pwa.grad, r_gpw)):  # sums over N * H * W products
        assert (got.to(ref_dt) - want).abs().max().item() <= 4 * tol * max(1.0, want.abs().max().item()), name


@pytest.mark.parametrize("name", LAYER)
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_layer_fixtures_through_the_fused_kernels_fp32(name, mode, fused_calls):
    gold = load_golden(name)
    _, layer = layer_from_fixture(gold, torch.float32)
    layer = layer.to(DEV)
    x, gout = torch.from_numpy(gold["x"]).float().to(DEV), torch.from_numpy(gold["gout"]).float().to(DEV)
    got = run_layer(layer, x, gout, mode)
    assert fused_calls == {"fused": 1, "other": 0}
    for key, t in got.items():
        ref = torch.from_numpy(gold[f"{mode}_{key}"])
        scale = max(1.0, ref.abs().max().item())
        assert (t.detach().cpu() - ref).abs().max().item() <= 1e-3 * scale, key


@pytest.mark.parametrize("name", REAL)
def test_compact_fixtures_at_the_stage_geometries_fp32(name, fused_calls):
    gold = load_golden(name)
    _, layer, x, gout = seeded_real_layer(gold)
    layer = layer.to(DEV)
    for mode in ("eval", "train"):
        check_compact(gold, mode, run_layer(layer, x.to(DEV), gout.to(DEV), mode), 1e-3)
    assert fused_calls["fused"] == 2 and fused_calls["other"] == 0


@pytest.mark.parametrize("name", MODELS)
def test_model_fixtures_fp64(name):
    gold = load_golden(f"lrnet_model_{name}")
    meta = json.loads(str(gold["meta"]))
    torch.manual_seed(int(gold["seed"]))
    m = cotnet_amd.create_model(name, num_classes=meta["num_classes"], zero_init_last_bn=False).double().to(DEV)
    rng = np.random.Generator(np.random.PCG64(int(gold["seed"])))
    x = rng_tensor(rng, (2, 3, meta["size"], meta["size"]), torch.float64).to(DEV)
    with torch.no_grad():
        for key, mode in (("logits", False), ("logits_train", True)):
            y = m.train(mode)(x).cpu()
            ref = torch.from_numpy(gold[key])
            assert ((y - ref).abs().max() / ref.abs().max()).item() < 1e-7, key


def _train_step(m, x, target):
    m.zero_grad()
    loss = torch.nn.functional.cross_entropy(m(x).float(), target)
    loss.backward()
    return loss


def test_bf16_training_step_tracks_its_fp32_twin(fused_calls, monkeypatch):
    """noise-relative: the bf16 step through the fused op is as far from the fp32 twin as the same bf16 step through the
    reference's composition (the softmax gradient sums to zero over the taps, so pos_h / pos_w gradients are small differences of
    large sums and carry bf16's noise at O(1) relative size in BOTH forms; a wiring defect would stand out against it)"""
    torch.manual_seed(0)
    m32 = cotnet_amd.create_model("lrnet50", num_classes=10, zero_init_last_bn=False).to(DEV).train()
    m16 = to_mixed_bf16(copy.deepcopy(m32))
    m16c = copy.deepcopy(m16)
    assert m16.layer1[0].conv2.pos_h.dtype == torch.float32  # bare parameters stay fp32
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(8, 3, 112, 112, device=DEV, generator=g)
    target = torch.randint(0, 10, (8,), device=DEV, generator=g)
    l32 = _train_step(m32, x, target)
    fused_calls.update(fused=0, other=0)
    l16 = _train_step(m16, x.bfloat16(), target)
    assert fused_calls == {"fused": 16, "other": 0}
    with monkeypatch.context() as mp:
        mp.setattr(lrmod, "fusable", lambda *a: False)
        l16c = _train_step(m16c, x.bfloat16(), target)
    torch.cuda.synchronize()
    assert abs(l16.item() - l32.item()) <= 2 * abs(l16c.item() - l32.item()) + 1e-2 * abs(l32.item())

    def rel(a, b):
        return ((a.float() - b.float()).norm() / b.float().norm()).item()
    for name, p32 in m32.named_parameters():
        r, rc = rel(m16.get_parameter(name).grad, p32.grad), rel(m16c.get_parameter(name).grad, p32.grad)
        assert r <= 2 * rc + 0.02, (name, r, rc)
    opt = torch.optim.SGD(m16.parameters(), lr=0.1, momentum=0.9)
    opt.step()
    assert torch.isfinite(_train_step(m16, x.bfloat16(), target)).item()


_STRICT_STEP = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
import cotnet_amd
from cotnet_amd import _lib
from cotnet_amd.flat_sgd import to_mixed_bf16
assert _lib.STRICT_DISPATCH
torch.manual_seed(0)
m = to_mixed_bf16(cotnet_amd.create_model(sys.argv[2]).cuda().train())
opt = torch.optim.SGD(m.parameters(), lr=0.1, momentum=0.9)
x = torch.randn(2, 3, 224, 224, device="cuda").bfloat16()
loss = torch.nn.functional.cross_entropy(m(x).float(), torch.tensor([1, 2], device="cuda"))
loss.backward()
opt.step()
torch.cuda.synchronize()
assert torch.isfinite(loss).item() and not _lib.FALLBACKS, _lib.FALLBACKS
print("strict ok", loss.item())
"""


@pytest.mark.parametrize("name", MODELS)
def test_bf16_step_with_no_module_fallback(name):
    env = dict(os.environ, COT_STRICT_DISPATCH="1")
    r = subprocess.run([sys.executable, "-c", _STRICT_STEP, ROOT, name], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "strict ok" in r.stdout, r.stderr[-3000:]


def test_two_runs_are_bit_identical():
    q, k, v, gout, pos_h, pos_w = stage_inputs(128, 28, torch.bfloat16, seed=7, N=16)
    res = []
    for _ in range(2):
        qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
        pha, pwa = pos_h.clone().requires_grad_(True), pos_w.clone().requires_grad_(True)
        y = local_relation(qa, ka, va, pha, pwa, 3)
        y.backward(gout)
        res.append([y.detach(), qa.grad, ka.grad, va.grad, pha.grad, pwa.grad])
    torch.cuda.synchronize()
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_graph_capture_of_forward_and_backward_replays_equal_to_eager():
    q, k, v, gout, pos_h, pos_w = stage_inputs(64, 56, torch.bfloat16, seed=11, N=8)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v, pos_h, pos_w)]

    def step():
        y = local_relation(*leaves, 3)
        return [y] + list(torch.autograd.grad(y, leaves, gout))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):  # warm-up off the capture stream (workspace-size cache, library load)
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    eager = [t.clone() for t in step()]
    with torch.no_grad():
        for t, src in zip(leaves, (q, k, v, pos_h, pos_w)):
            t.copy_(src * 1.0)  # same values, written in place: the replay reads the captured buffers
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(captured, eager):
        assert torch.equal(a, b)


# ---- the directed edges of tests/test_lrnet_emulated.py on the device (same functions, the device library in the emulator's place), then
# the Python wrapper off the happy path; checker: lr_reference64 (fp64 from unfold and einsum, no code shared with the product)
from tests import test_lrnet_emulated as tle  # noqa: E402
from tests.test_fuzz_gpu import device_fuzz  # noqa: E402


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_lds_boundary_on_the_device(dtype):
    with device_fuzz():
        tle.lds_boundary_case(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H,W", tle.RAGGED)
def test_rectangular_and_ragged_tiles_on_the_device(H, W, dtype):
    with device_fuzz():
        tle.lr_directed(2, 24, H, W, dtype, seed=H + W)


def test_both_backward_routes_by_name_on_the_device():
    with device_fuzz():
        tle.backward_routes_case()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("H,W", [(9, 30), (5, 100), (7, 7), (2, 150)])
def test_saturated_softmax_on_the_device(H, W, dtype):
    with device_fuzz():
        tle.saturated_case(dtype, H, W)


def _view(kind, base):
    """a [2, 24, H, W] view of `base` that the kernels cannot take as it is (differentiable: the gradient flows back to `base`)"""
    if kind == "channel_slice":  # base [2, 40, 6, 10]
        return base[:, 8:32]
    if kind == "transposed":     # base [2, 24, 10, 6]
        return base.transpose(2, 3)
    if kind == "offset":         # base [2, 24, 5, 12] (the four-element loader after the wrapper's copy): one element into a storage of its own
        return torch.cat([base.new_zeros(1), base.reshape(-1)])[1:].view(base.shape)
    return base                  # rectangular, [2, 24, 5, 100]


_BASE = {"channel_slice": (2, 40, 6, 10), "transposed": (2, 24, 10, 6), "offset": (2, 24, 5, 12), "rectangular": (2, 24, 5, 100)}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", list(_BASE))
def test_wrapper_views_and_bf16_positions(kind, dtype, fused_calls):
    from tests import test_fuzz_emulated as tfe
    g = torch.Generator(device=DEV).manual_seed(17)
    bases = [(f * torch.randn(_BASE[kind], device=DEV, generator=g)).to(dtype).requires_grad_(True) for f in (0.5, 0.5, 1)]
    q, k, v = (_view(kind, b) for b in bases)
    if kind == "offset":
        assert q.data_ptr() % 16 != 0
    elif kind != "rectangular":
        assert not q.is_contiguous()
    gout = torch.randn(q.shape, device=DEV, generator=g).to(dtype)
    pos_dt = torch.bfloat16 if dtype == torch.bfloat16 else torch.float32
    pha, pwa = (torch.randn(s, device=DEV, generator=g).to(pos_dt).requires_grad_(True) for s in ((24, 3, 1), (24, 1, 3)))
    y = local_relation(q, k, v, pha, pwa, 3)
    assert _lib.last_kernel() == "lr_fwd"
    y.backward(gout)
    torch.cuda.synchronize()
    assert fused_calls == {"fused": 1, "other": 0}
    assert pha.grad.dtype == pos_dt and pwa.grad.dtype == pos_dt
    pos = (pha.detach() + pwa.detach()).float().reshape(24, 9)  # (the sum is formed in the parameters' type, as the wrapper forms it)
    r_y, r_gq, r_gk, r_gv, r_gpos = tfe.lr_reference64(q, k, v, pos, gout)
    r_gq, r_gk, r_gv = torch.autograd.grad((q, k, v), bases, (r_gq.to(dtype), r_gk.to(dtype), r_gv.to(dtype)))  # back through the views
    tol = 2e-5 if dtype == torch.float32 else 4e-2
    for name, got, want, f in (("y", y, r_y, 1), ("gv", bases[2].grad, r_gv, 1), ("gq", bases[0].grad, r_gq, 4), ("gk", bases[1].grad, r_gk, 4)):
        assert torch.isfinite(got).all(), name
        err = (got.detach().double() - want.double()).abs()
        assert (err <= f * tol * (1 + want.double().abs())).all(), (name, err.max().item())
    r_gpos = r_gpos.view(24, 3, 3)
    for name, gr, w in (("pos_h", pha.grad, r_gpos.sum(2, keepdim=True)), ("pos_w", pwa.grad, r_gpos.sum(1, keepdim=True))):
        assert (gr.double() - w).abs().max().item() <= 4 * tol * max(1.0, w.abs().max().item()), name


def test_width_past_the_lds_boundary_takes_the_composition(fused_calls):
    g = torch.Generator(device=DEV).manual_seed(19)
    q, k, v = ((f * torch.randn(1, 8, 2, 212, device=DEV, generator=g)).bfloat16().requires_grad_(True) for f in (0.5, 0.5, 1))
    pos_h, pos_w = torch.randn(8, 3, 1, device=DEV, generator=g), torch.randn(8, 1, 3, device=DEV, generator=g)
    before = _lib.FALLBACKS.get("local_relation", 0)
    y = local_relation(q, k, v, pos_h, pos_w, 3)
    torch.cuda.synchronize()
    assert fused_calls == {"fused": 0, "other": 1}
    assert _lib.FALLBACKS.get("local_relation", 0) == before + 1, _lib.FALLBACKS
    from tests import test_fuzz_emulated as tfe
    want = tfe.lr_reference64(q, k, v, (pos_h + pos_w).reshape(8, 9), torch.ones_like(y))[0]
    assert ((y.detach().double() - want).abs() <= 4e-2 * (1 + want.abs())).all()


_STRICT_LR = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
from cotnet_amd import _lib
from cotnet_amd.local_relation import local_relation
assert _lib.STRICT_DISPATCH
q, k, v = (torch.randn(1, 8, 2, 212, device="cuda").bfloat16() for _ in range(3))
pos_h, pos_w = torch.randn(8, 3, 1, device="cuda"), torch.randn(8, 1, 3, device="cuda")
local_relation(q, k, v, pos_h, pos_w, 3)
print("no error raised")
"""


def test_width_past_the_lds_boundary_raises_under_strict_dispatch():
    env = dict(os.environ, COT_STRICT_DISPATCH="1")
    r = subprocess.run([sys.executable, "-c", _STRICT_LR, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "no error raised" not in r.stdout and "local_relation" in r.stderr, (r.stdout, r.stderr[-3000:])
