"""Caches that a kernel launch fills, while a HIP graph is being captured -- on the host emulator, with cot_layer_fused._capturing forced to
True.  A capture records launches and does not run them, so `_masks` and `_merged_weight` must serve the call and leave `_MASKS` / `_MERGED`
as they found them; the backward of a forward that made its own merged weight must still find it (tests/test_graph_replay_gpu.py runs the real
thing on the device)."""
import copy
import ctypes

import pytest
import torch

from cotnet_amd import _lib
from tests.emul import build_emul

try:
    _EMUL = _lib.bind(ctypes.CDLL(build_emul.build()))
except FileNotFoundError:
    _EMUL = None

pytestmark = pytest.mark.skipif(_EMUL is None, reason="host emulation build unavailable")


def _run(layer, x, g):
    xi = x.clone().requires_grad_(True)
    y = layer(xi)
    assert y.grad_fn.name().startswith("_CotLayerNode")
    y.backward(g)
    return [y.detach(), xi.grad] + [p.grad for p in layer.parameters()]


def test_masks_and_merged_weight_leave_their_caches_alone_while_capturing(monkeypatch):
    from cotnet_amd import conv3x3g as c3, cot_layer_fused as clf
    from cotnet_amd.cotnet import CoXtLayer
    from cotnet_amd.flat_sgd import to_mixed_bf16
    monkeypatch.setattr(_lib, "lib", lambda: _EMUL)
    monkeypatch.setattr(_lib, "DEVICE_ONLY", False)
    monkeypatch.setattr(clf, "ENABLED", True)
    monkeypatch.setattr(clf, "MERGE12", True)
    for mod, name in ((clf, "_SIZES"), (clf, "_MASKS"), (c3, "_MASKS")):  # fresh tables for this test; the process's own come back after it
        monkeypatch.setattr(mod, name, type(getattr(mod, name))())
    torch.manual_seed(12)
    N, C, H = 2, 96, 8
    layer = to_mixed_bf16(CoXtLayer(C, 3).train())  # 8 groups of 12 channels: the merged-weight branch
    conv = layer.key_embed[0]
    assert clf._merge12(C, conv.groups)
    x, g = torch.randn(N, C, H, H).bfloat16(), torch.randn(N, C, H, H).bfloat16()
    ref = _run(copy.deepcopy(layer), x, g)   # not capturing: fills the mask cache (and the copy's merged weight)
    assert len(clf._MASKS) == 1
    table = next(iter(clf._MASKS.values())).clone()
    clf._MASKS.clear()

    monkeypatch.setattr(clf, "_capturing", lambda: True)
    monkeypatch.setattr(_lib, "capturing", lambda: True)
    # cold caches: the calls are served, nothing is stored, and the backward runs on the merged weight its forward made
    m = clf._masks(_lib.api(), H, H, x.device)
    assert torch.equal(m, table) and not clf._MASKS
    assert torch.equal(c3._masks(H, H, x.device), table) and not c3._MASKS
    cold = copy.deepcopy(layer)
    got = _run(cold, x, g)
    assert not clf._MASKS and cold.key_embed[0] not in clf._MERGED
    assert all(torch.equal(a, b) for a, b in zip(ref, got))
    w1 = clf._merged_weight(conv, C, conv.groups, True)
    w2 = clf._merged_weight(conv, C, conv.groups, False)
    assert w1 is not w2 and torch.equal(w1, w2) and conv not in clf._MERGED
    assert clf._merged_weight(conv, C, conv.groups, False, own=w1) is w1

    # warm caches: the entries made outside a capture are used and stay the same objects
    monkeypatch.setattr(clf, "_capturing", lambda: False)
    monkeypatch.setattr(_lib, "capturing", lambda: False)
    warm = copy.deepcopy(layer)
    _run(warm, x, g)
    kept, merged = dict(clf._MASKS), clf._MERGED[warm.key_embed[0]][1]
    monkeypatch.setattr(clf, "_capturing", lambda: True)
    monkeypatch.setattr(_lib, "capturing", lambda: True)
    got = _run(warm, x, g)
    assert clf._MASKS.keys() == kept.keys() and all(clf._MASKS[k] is v for k, v in kept.items())
    assert clf._MERGED[warm.key_embed[0]][1] is merged
    assert all(torch.equal(a, b) for a, b in zip(ref[:2], got[:2]))


def test_set_lr_after_a_captured_step_raises_until_the_step_is_captured_again(monkeypatch):
    """cot_sgd_step takes the rate by value, so the replays of a captured step keep it: FlatSGD.set_lr to another rate raises and leaves
    the rate alone, the captured rate stays accepted, and a step captured at a new rate (set inside that capture) lifts the condition"""
    from cotnet_amd.flat_sgd import FlatSGD
    monkeypatch.setattr(_lib, "lib", lambda: _EMUL)
    monkeypatch.setattr(_lib, "DEVICE_ONLY", False)
    torch.manual_seed(1)
    m = torch.nn.Linear(8, 8)
    opt = FlatSGD(m, lr=0.1, momentum=0.9, weight_decay=4e-5, nesterov=True)

    def step(lr=None):
        if lr is not None:
            opt.set_lr(lr)
        opt.zero_grad()
        m(torch.randn(4, 8)).square().mean().backward()
        opt.step()
    step()
    opt.set_lr(0.05)  # nothing captured: silent
    w0 = m.weight.detach().clone()
    monkeypatch.setattr(_lib, "capturing", lambda: True)
    step()            # "captured" at 0.05
    monkeypatch.setattr(_lib, "capturing", lambda: False)
    assert not torch.equal(w0, m.weight)  # (the emulator ran the step)
    opt.set_lr(0.05)
    for _ in range(2):
        with pytest.raises(RuntimeError, match="replays keep the captured rate.*capture the step again"):
            opt.set_lr(0.005)
        assert opt.lr == 0.05  # a refused rate is not stored: eager steps and replays stay at one rate
    monkeypatch.setattr(_lib, "capturing", lambda: True)
    step(0.005)       # captured again; the new rate is set inside that capture
    monkeypatch.setattr(_lib, "capturing", lambda: False)
    assert opt.lr == 0.005
    opt.set_lr(0.005)
    with pytest.raises(RuntimeError, match="captured"):
        opt.set_lr(0.05)
    assert opt.lr == 0.005
