"""LR-Net's 7x7 local relation on the MI355X (csrc/local_relation7.hip): the directed cases of tests/lr_k7_cases.py through the C ABI of
the device library, the seven LR-Net-50 stage geometries through the Python wrapper, determinism, graph capture, views, the fallback past
the LDS boundary, the reference's SelfAttLayer(dim, 7, key_ks) fixtures on the fused route and one training step of lrnet50_k7.
Run with `pytest -m gpu`."""
import os
import subprocess
import sys

import pytest
import torch

import cotnet_amd.local_relation as lrmod
from cotnet_amd import _lib
from cotnet_amd.local_relation import local_relation
from tests import lr_k7_cases as L7
from tests.conftest import ROOT, load_golden
from tests.test_lrnet_cpu import run_layer
from tests.test_lrnet_k7_cpu import LAYER, layer_from_fixture

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture
def E():
    return _lib.lib()  # (raises when the HIP library is missing: no fallback)


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


# ---- the C ABI: the functions tests/test_lrnet_k7_emulated.py runs on the host emulator
@pytest.mark.parametrize("dtype", L7.DTYPES)
@pytest.mark.parametrize("case", L7.DIRECTED, ids=L7.case_id)
def test_directed_shapes_match_the_fp64_statement(case, dtype, E):
    """fails without the feature: all three entry points answer -2 at 7x7"""
    L7.directed(E, DEV, *case, dtype, seed=sum(case))


@pytest.mark.parametrize("dtype", L7.DTYPES)
def test_lds_boundary(dtype, E):
    L7.lds_boundary(E, DEV, dtype)


@pytest.mark.parametrize("dtype", L7.DTYPES)
@pytest.mark.parametrize("H,W", [(9, 30), (7, 7), (2, 150)])
def test_saturated_softmax(H, W, dtype, E):
    L7.saturated(E, DEV, H, W, dtype)


def test_other_windows_dtypes_and_paddings_are_refused(E):
    L7.refusals(E)


def test_misaligned_pointers_are_refused(E):
    L7.misaligned(E, DEV)


# ---- the wrapper
def wrapper_inputs(N, C, H, W, dtype, seed):
    q, k, v, gout, pos = L7.inputs(N, C, H, W, dtype, seed, dev=DEV)
    g = torch.Generator().manual_seed(seed + 1)
    pos_h, pos_w = torch.randn(C, 7, 1, generator=g).to(DEV), torch.randn(C, 1, 7, generator=g).to(DEV)
    return q, k, v, gout, pos_h, pos_w


def wrapper_step(q, k, v, gout, pos_h, pos_w):
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v, pos_h, pos_w)]
    y = local_relation(*leaves, 7)
    assert _lib.last_kernel() == L7.FWD
    y.backward(gout)
    assert _lib.last_kernel() == L7.BWD
    return [y.detach()] + [t.grad for t in leaves]


def check_against_reference(got, q, k, v, gout, pos_h, pos_w, dtype):
    y, gq, gk, gv, gph, gpw = got
    C = q.shape[1]
    pos = (pos_h + pos_w).float().reshape(C, 49)
    want = L7.reference64(q, k, v, pos, gout, dev=DEV)
    gpos = want[4].view(C, 7, 7)
    bad = L7.mismatches((y, gq, gk, gv, want[4]), want, dtype)  # (gpos reaches the caller as pos_h / pos_w gradients: below)
    assert not bad, bad
    tol = L7.tolerances(dtype)[0]
    for name, g, w in (("pos_h", gph, gpos.sum(2, keepdim=True)), ("pos_w", gpw, gpos.sum(1, keepdim=True))):
        assert (g.double().cpu() - w).abs().max().item() <= 4 * tol * max(1.0, w.abs().max().item()), name


@pytest.mark.parametrize("dtype", L7.DTYPES)
@pytest.mark.parametrize("C,H", L7.STAGES)
def test_fused_op_at_the_stage_geometries(C, H, dtype, fused_calls):
    args = wrapper_inputs(4, C, H, H, dtype, seed=C + H)
    got = wrapper_step(*args)
    assert fused_calls == {"fused": 1, "other": 0}
    check_against_reference(got, *args, dtype)


def test_two_runs_are_bit_identical():
    args = wrapper_inputs(4, 128, 28, 28, torch.bfloat16, seed=7)
    a, b = wrapper_step(*args), wrapper_step(*args)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_graph_capture_of_forward_and_backward_replays_equal_to_eager():
    q, k, v, gout, pos_h, pos_w = wrapper_inputs(4, 64, 56, 56, torch.bfloat16, seed=11)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v, pos_h, pos_w)]

    def step():
        y = local_relation(*leaves, 7)
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


def _view(kind, base):
    """a [2, 24, H, W] view of `base` that the kernels cannot take as it is (differentiable: the gradient flows back to `base`)"""
    if kind == "channel_slice":  # base [2, 40, 6, 10]
        return base[:, 8:32]
    if kind == "transposed":     # base [2, 24, 10, 6]
        return base.transpose(2, 3)
    if kind == "offset":         # base [2, 24, 5, 12]: one element into a storage of its own
        return torch.cat([base.new_zeros(1), base.reshape(-1)])[1:].view(base.shape)
    return base                  # rectangular, [2, 24, 5, 100]


_BASE = {"channel_slice": (2, 40, 6, 10), "transposed": (2, 24, 10, 6), "offset": (2, 24, 5, 12), "rectangular": (2, 24, 5, 100)}


@pytest.mark.parametrize("dtype", L7.DTYPES)
@pytest.mark.parametrize("kind", list(_BASE))
def test_wrapper_views_and_bf16_positions(kind, dtype, fused_calls):
    g = torch.Generator(device=DEV).manual_seed(17)
    bases = [(f * torch.randn(_BASE[kind], device=DEV, generator=g)).to(dtype).requires_grad_(True) for f in (0.5, 0.5, 1)]
    q, k, v = (_view(kind, b) for b in bases)
    if kind == "offset":
        assert q.data_ptr() % 16 != 0
    elif kind != "rectangular":
        assert not q.is_contiguous()
    gout = torch.randn(q.shape, device=DEV, generator=g).to(dtype)
    pos_dt = torch.bfloat16 if dtype == torch.bfloat16 else torch.float32
    pha, pwa = (torch.randn(s, device=DEV, generator=g).to(pos_dt).requires_grad_(True) for s in ((24, 7, 1), (24, 1, 7)))
    y = local_relation(q, k, v, pha, pwa, 7)
    assert _lib.last_kernel() == L7.FWD
    y.backward(gout)
    torch.cuda.synchronize()
    assert fused_calls == {"fused": 1, "other": 0}
    assert pha.grad.dtype == pos_dt and pwa.grad.dtype == pos_dt
    pos = (pha.detach() + pwa.detach()).float().reshape(24, 49)  # (the sum is formed in the parameters' type, as the wrapper forms it)
    r_y, r_gq, r_gk, r_gv, r_gpos, _ = L7.reference64(q, k, v, pos, gout)
    # back through the views, in fp64
    b64 = [b.detach().double().requires_grad_(True) for b in bases]
    r_gq, r_gk, r_gv = torch.autograd.grad([_view(kind, b) for b in b64], b64, [t.to(DEV) for t in (r_gq, r_gk, r_gv)])
    tol = L7.tolerances(dtype)[0]
    for name, got, want, f in (("y", y, r_y, 1), ("gv", bases[2].grad, r_gv, 1), ("gq", bases[0].grad, r_gq, 4), ("gk", bases[1].grad, r_gk, 4)):
        got, want = got.detach().double().cpu(), want.double().cpu()
        assert torch.isfinite(got).all(), name
        assert ((got - want).abs() <= f * tol * (1 + want.abs())).all(), (name, (got - want).abs().max().item())
    r_gpos = r_gpos.view(24, 7, 7)
    for name, gr, w in (("pos_h", pha.grad, r_gpos.sum(2, keepdim=True)), ("pos_w", pwa.grad, r_gpos.sum(1, keepdim=True))):
        assert (gr.double().cpu() - w).abs().max().item() <= 4 * tol * max(1.0, w.abs().max().item()), name


def test_width_past_the_lds_boundary_takes_the_composition(fused_calls):
    W = L7.boundary_width(2) + 1
    q, k, v, gout, pos_h, pos_w = wrapper_inputs(1, 8, 2, W, torch.bfloat16, seed=19)
    before = _lib.FALLBACKS.get("local_relation", 0)
    y = local_relation(q, k, v, pos_h, pos_w, 7)
    torch.cuda.synchronize()
    assert fused_calls == {"fused": 0, "other": 1}
    assert _lib.FALLBACKS.get("local_relation", 0) == before + 1, _lib.FALLBACKS
    want = L7.reference64(q, k, v, (pos_h + pos_w).reshape(8, 49), gout)[0]
    assert ((y.detach().double().cpu() - want).abs() <= 4e-2 * (1 + want.abs())).all()


def test_five_by_five_takes_the_composition_without_a_fallback_count(fused_calls):
    g = torch.Generator().manual_seed(23)
    q, k, v = ((0.5 * torch.randn(1, 8, 6, 8, generator=g)).to(DEV) for _ in range(3))
    pos_h, pos_w = torch.randn(8, 5, 1, generator=g).to(DEV), torch.randn(8, 1, 5, generator=g).to(DEV)
    before = _lib.FALLBACKS.get("local_relation", 0)
    y = local_relation(q, k, v, pos_h, pos_w, 5)
    assert fused_calls == {"fused": 0, "other": 1} and _lib.FALLBACKS.get("local_relation", 0) == before
    want = L7.reference64(q, k, v, (pos_h + pos_w).reshape(8, 25), torch.ones_like(q), ks=5)[0]
    assert ((y.double().cpu() - want).abs() <= 2e-5 * (1 + want.abs())).all()


_STRICT_LR = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
from cotnet_amd import _lib
from cotnet_amd.local_relation import local_relation
assert _lib.STRICT_DISPATCH
W = int(sys.argv[2])
q, k, v = (torch.randn(1, 8, 2, W, device="cuda").bfloat16() for _ in range(3))
pos_h, pos_w = torch.randn(8, 7, 1, device="cuda"), torch.randn(8, 1, 7, device="cuda")
local_relation(q, k, v, pos_h, pos_w, 7)
print("no error raised")
"""


def test_width_past_the_lds_boundary_raises_under_strict_dispatch():
    env = dict(os.environ, COT_STRICT_DISPATCH="1")
    r = subprocess.run([sys.executable, "-c", _STRICT_LR, ROOT, str(L7.boundary_width(2) + 1)], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0 and "no error raised" not in r.stdout and "local_relation" in r.stderr, (r.stdout, r.stderr[-3000:])


_STRICT_STEP = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
import cotnet_amd
from cotnet_amd import _lib
from cotnet_amd.flat_sgd import to_mixed_bf16
assert _lib.STRICT_DISPATCH
torch.manual_seed(0)
m = to_mixed_bf16(cotnet_amd.create_model("lrnet50_k7").cuda().train())
assert m.layer1[0].conv2.kernel_size == 7
opt = torch.optim.SGD(m.parameters(), lr=0.1, momentum=0.9)
x = torch.randn(2, 3, 224, 224, device="cuda").bfloat16()
loss = torch.nn.functional.cross_entropy(m(x).float(), torch.tensor([1, 2], device="cuda"))
loss.backward()
opt.step()
torch.cuda.synchronize()
grads = [p.grad for n, p in m.named_parameters() if n.endswith(("pos_h", "pos_w"))]
assert len(grads) == 32 and all(g is not None and torch.isfinite(g).all().item() for g in grads)
assert torch.isfinite(loss).item() and not _lib.FALLBACKS, _lib.FALLBACKS
print("strict ok", loss.item())
"""


def test_lrnet50_k7_bf16_step_with_no_module_fallback():
    env = dict(os.environ, COT_STRICT_DISPATCH="1")
    r = subprocess.run([sys.executable, "-c", _STRICT_STEP, ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "strict ok" in r.stdout, r.stderr[-3000:]


# ---- the reference's own SelfAttLayer(dim, 7, key_ks) on the fused route
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
