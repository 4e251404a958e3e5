"""What a module has to be for a single-node path to take it (cot_layer_fused.eligible / block_eligible / cm_block_eligible /
sa_block_eligible / eval_block_eligible), and the order in which a block tries the node kinds (cot_layer_fused.dispatch).

The training nodes normalise with batch statistics and overwrite the running ones, the eval node reads the running ones; so EVERY
BatchNorm a node's launch sequence touches has to be in the node's mode, and every parameter in the dtype the kernels read it as.  Each
plan lists both (`bns`, `lowp`); here each entry is put wrong alone and the predicate has to say no.  Before the plans listed them the
predicates checked hand-picked subsets: a training Bottleneck(256, 64) with bn3, conv2.embed.1, conv2.conv1x1.1, conv2.se.1 or
conv2.key_embed.1 frozen was taken by the block node (the last one not by the layer node), and a fp32 embed.0 / conv1x1.0 / se.0 /
se.3 went unnoticed.

CPU bf16 tensors with _lib.DEVICE_ONLY lifted; no kernel is launched.  Only the channel-major predicate asks the library (its
host-only *_covers queries), and only once everything cheaper has passed: every other predicate runs with a library handle that raises.
"""
import os

import pytest
import torch
from torch import nn

from cotnet_amd import _lib, cot_layer_fused as clf
from cotnet_amd.flat_sgd import to_mixed_bf16

N = 2


def _x(c, h):
    return torch.zeros(N, c, h, h, dtype=torch.bfloat16)


def _layer(cls, dim):
    def make():
        from cotnet_amd import cotnet
        m = to_mixed_bf16(getattr(cotnet, cls)(dim, 3).train())
        return m, _x(dim, 14), clf.eligible, clf._plan(m), True
    return make


def _identity(predicate, training=True):
    def make():
        from cotnet_amd.cotnet import Bottleneck
        m = to_mixed_bf16(Bottleneck(256, 64).train(training))
        return m, _x(256, 14), getattr(clf, predicate), clf._block_plan(m), training
    return make


def _opening():
    """a stage's stride-2 opening block: 3x3/2 average pooling in front of the layer, stride-2 projection shortcut"""
    from cotnet_amd.cotnet import Bottleneck
    from cotnet_amd.resnet import downsample_conv
    m = to_mixed_bf16(Bottleneck(256, 128, stride=2, downsample=downsample_conv(256, 512, 1, stride=2)).train())
    return m, _x(256, 28), clf.block_eligible, clf._block_plan(m), True


def _hybrid(block_idx):
    """SE-CoTNetD's third stage at 14 x 14 (its smallest SplitAttn shape): even blocks hold a CoT layer, odd ones a SplitAttnConv2d"""
    from cotnet_amd.cotnet_hybrid import CoTBottleneck
    from cotnet_amd.layers import get_act_layer
    return to_mixed_bf16(CoTBottleneck(block_idx, 1024, 256, conv_dim={64, 128}, c4_dim=256, c4_idx={0, 2, 4}, radix=1,
                                       act_layer=get_act_layer("swish")).train())


def _split_attn():
    m = _hybrid(1)
    return m, _x(1024, 14), clf.sa_block_eligible, clf._sa_plan(m), True


CASES = {
    "layer CotLayer(64)": _layer("CotLayer", 64),
    "layer CoXtLayer(96)": _layer("CoXtLayer", 96),
    "block identity": _identity("block_eligible"),
    "block stride-2 opening": _opening,
    "channel-major identity": _identity("cm_block_eligible"),
    "split-attn": _split_attn,
    "eval identity": _identity("eval_block_eligible", training=False),
}


class _Library:
    """stands where _lib.lib does: counts how often the library is asked for; passes the real one on, or raises when there is to be none"""

    def __init__(self, real):
        self.real, self.asked = real, 0

    def __call__(self):
        self.asked += 1
        if self.real is None:
            raise AssertionError("this predicate has no business with the library")
        return self.real()


@pytest.fixture
def case(request, monkeypatch):
    name = request.param
    cm = name.startswith("channel-major")
    if cm and not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libcotnet_hip.so not built")
    library = _Library(_lib.lib if cm else None)
    monkeypatch.setattr(_lib, "lib", library)
    monkeypatch.setattr(_lib, "DEVICE_ONLY", False)
    for switch in ("ENABLED", "CM_LAYOUT", "CM_OPENING"):
        monkeypatch.setattr(clf, switch, True)
    clf._CM_OK.clear()
    torch.manual_seed(0)
    mod, x, predicate, plan, training = CASES[name]()
    if training:
        yield mod, x, predicate, plan, training, library
    else:
        with torch.no_grad():
            yield mod, x, predicate, plan, training, library
    clf._CM_OK.clear()


every_case = pytest.mark.parametrize("case", list(CASES), indirect=True)


def _name(root, mod):
    return next(n for n, m in root.named_modules() if m is mod)


@every_case
def test_every_batchnorm_of_the_node_has_to_be_in_the_nodes_mode(case):
    mod, x, predicate, plan, training, library = case
    assert plan.bns and all(isinstance(bn, nn.BatchNorm2d) and bn.training == training for bn in plan.bns)
    assert predicate(mod, x)
    asked = library.asked  # (channel-major: the geometry query, answered once per shape)
    for bn in plan.bns:
        bn.train(not training)
        assert not predicate(mod, x), _name(mod, bn)
        assert library.asked == asked, _name(mod, bn)  # refused before the library is asked
        bn.train(training)
    assert predicate(mod, x)
    # ... and carry fp32 running statistics
    bn = plan.bns[-1]
    mean = bn.running_mean
    bn.running_mean = mean.bfloat16()
    assert not predicate(mod, x)
    bn.running_mean = None
    assert not predicate(mod, x)
    bn.running_mean = mean
    assert predicate(mod, x)


@every_case
def test_every_parameter_has_to_be_in_the_dtype_the_kernels_read(case):
    mod, x, predicate, plan, training, library = case
    assert plan.lowp and predicate(mod, x)
    asked = library.asked
    for m in plan.lowp:
        m.weight.data = m.weight.data.float()
        assert not predicate(mod, x), _name(mod, m)
        m.weight.data = m.weight.data.bfloat16()
    for m in (m for m in plan.lowp if m.bias is not None):
        m.bias.data = m.bias.data.float()
        assert not predicate(mod, x), _name(mod, m)
        m.bias.data = m.bias.data.bfloat16()
    for bn in plan.bns:
        for p in (bn.weight, bn.bias):
            p.data = p.data.bfloat16()
            assert not predicate(mod, x), _name(mod, bn)
            p.data = p.data.float()
    assert library.asked == asked
    assert predicate(mod, x)


@every_case
def test_bns_and_lowp_hold_exactly_the_modules_behind_params(case):
    mod, x, predicate, plan, training, library = case
    owner = {id(p): m for m in mod.modules() for p in m.parameters(recurse=False)}
    behind = {owner[id(p)] for p in plan.params}
    assert len(plan.params) == len({id(p) for p in plan.params})
    assert set(plan.bns) | set(plan.lowp) == behind
    assert len(plan.bns) + len(plan.lowp) == len(behind)  # (no module twice, none in both)
    assert not any(isinstance(m, nn.BatchNorm2d) for m in plan.lowp)
    # ... and params leaves no parameter of theirs out
    assert {id(p) for m in behind for p in m.parameters(recurse=False)} == {id(p) for p in plan.params}


# ---- dispatch
KINDS = ("eval_block", "cm_block", "block", "sa_block")


@pytest.fixture
def stubs(monkeypatch):
    """every NAME_forward replaced by one that says its name.  -> function that also replaces every NAME_eligible by a recorder with a
    given answer per kind and returns the list it records into"""
    monkeypatch.setattr(_lib, "DEVICE_ONLY", False)
    for switch in ("ENABLED", "CM_LAYOUT", "CM_OPENING"):
        monkeypatch.setattr(clf, switch, True)
    for kind in KINDS:
        monkeypatch.setattr(clf, kind + "_forward", lambda blk, x, kind=kind: kind)

    def answers(**yes):
        asked = []
        for kind in KINDS:
            monkeypatch.setattr(clf, kind + "_eligible", lambda blk, x, kind=kind: asked.append(kind) or yes.get(kind, False))
        return asked
    return answers


def test_dispatch_asks_the_kinds_in_the_order_the_block_class_states(stubs):
    from cotnet_amd.cotnet import Bottleneck
    from cotnet_amd.cotnet_hybrid import CoTBottleneck
    assert Bottleneck.node_kinds == ("eval_block", "cm_block", "block")
    assert CoTBottleneck.node_kinds == ("block", "sa_block")  # (neither the eval nor the channel-major node)
    blk, x = to_mixed_bf16(Bottleneck(256, 64).train()), _x(256, 14)
    asked = stubs()
    assert clf.dispatch(blk, x) is None and asked == ["eval_block", "cm_block", "block"]
    for yes, ran, upto in ((dict(eval_block=True, cm_block=True, block=True), "eval_block", 1),
                           (dict(cm_block=True, block=True), "cm_block", 2), (dict(block=True), "block", 3),
                           (dict(sa_block=True), None, 3)):
        asked = stubs(**yes)
        assert clf.dispatch(blk, x) == ran and asked == ["eval_block", "cm_block", "block"][:upto]
    for idx in (0, 1):
        hyb = _hybrid(idx)
        asked = stubs()
        assert clf.dispatch(hyb, _x(1024, 14)) is None and asked == ["block", "sa_block"]
        asked = stubs(eval_block=True, cm_block=True, block=True, sa_block=True)
        assert clf.dispatch(hyb, _x(1024, 14)) == "block" and asked == ["block"]
        asked = stubs(eval_block=True, cm_block=True, sa_block=True)
        assert clf.dispatch(hyb, _x(1024, 14)) == "sa_block" and asked == ["block", "sa_block"]


@pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libcotnet_hip.so not built")
def test_dispatch_with_the_real_predicates(stubs, monkeypatch):
    """a block that several kinds accept goes to the first of them; the forward of a module calls dispatch"""
    from cotnet_amd.cotnet import Bottleneck
    blk, x = to_mixed_bf16(Bottleneck(256, 64).train()), _x(256, 14)
    clf._CM_OK.clear()
    try:
        assert clf.cm_block_eligible(blk, x) and clf.block_eligible(blk, x) and not clf.eval_block_eligible(blk, x)
        assert clf.dispatch(blk, x) == "cm_block" and blk(x) == "cm_block"
        monkeypatch.setattr(clf, "CM_LAYOUT", False)
        assert clf.dispatch(blk, x) == "block" and blk(x) == "block"
        blk.bn3.eval()  # a frozen BatchNorm: no node takes the block
        assert clf.dispatch(blk, x) is None
        blk.eval()
        with torch.no_grad():
            assert clf.eval_block_eligible(blk, x) and clf.dispatch(blk, x) == "eval_block" and blk(x) == "eval_block"
        assert clf.dispatch(blk, x) is None  # (autograd on)
        # the hybrid block: the kind its conv2 calls for, and no other
        cot, sa, xh = _hybrid(0), _hybrid(1), _x(1024, 14)
        assert clf.block_eligible(cot, xh) and not clf.sa_block_eligible(cot, xh)
        assert clf.sa_block_eligible(sa, xh) and not clf.block_eligible(sa, xh)
        assert clf.dispatch(cot, xh) == "block" and cot(xh) == "block"
        assert clf.dispatch(sa, xh) == "sa_block" and sa(xh) == "sa_block"
        with torch.no_grad():
            assert clf.dispatch(cot.eval(), xh) is None  # (it has no eval node)
        monkeypatch.setattr(clf, "ENABLED", False)
        assert clf.dispatch(blk, x) is None and clf.dispatch(sa, xh) is None
    finally:
        clf._CM_OK.clear()
