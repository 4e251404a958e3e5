"""Shared cases of the feature-backbone tests (cotnet_amd/features.py): test_features_host_cpu.py (structure against the reference's
own wrappers, tests/golden/features_structure.json), test_features_emulated.py (a small ResNet on the host emulator) and
test_features_gpu.py (the registered models on the device).

The numerical criterion is transitive and exact: the classifier models are pinned to the reference by the existing suite, and a backbone
has to hand out, BIT FOR BIT, what the classifier model of the same weights computes at the tapped modules -- `hooked_forward` takes a
clone of each at the moment the module returns.  No tolerance anywhere in this file.

Tap 0 is what `act1` returns in the reference.  Here the stem's BatchNorm + ReLU is one fused pass (resnet.stem_forward) that never calls
the `act1` module, so a forward hook on it does not fire; the clone is then taken where that tensor is handed on -- at the max-pool's
call site (`resnet.pool`, ResNet) or by a forward-pre hook on `layer1` (CoTHybridNet, which has no max-pool).  Where the module path
does call `act1`, its hook is the one used.
"""
import contextlib
from collections import OrderedDict

import torch

MODELS = ("cotnet50", "cotnext50_2x48d", "se_cotnetd_50", "lrnet50")
OUT_INDICES = (None, (1, 2), (4,), (0, 3))  # None: the builder's default (0, 1, 2, 3, 4)
OUTPUT_STRIDES = (32, 16, 8)
STRUCTURE_CASES = [(m, o, s) for m in MODELS for o in OUT_INDICES for s in OUTPUT_STRIDES]
TAP_MODULES = ("act1", "layer1", "layer2", "layer3", "layer4")


def case_id(name, out_indices, output_stride):
    return f"{name}-{'default' if out_indices is None else '_'.join(map(str, out_indices))}-os{output_stride}"


def describe(net):
    """the structure of a feature wrapper (the reference's or this package's) as plain data"""
    fi = net.feature_info
    return dict(keys=list(net.keys()), return_layers=dict(net.return_layers), info=[dict(d) for d in fi.info],
                out_indices=list(fi.out_indices), channels=fi.channels(), reduction=fi.reduction(), module_name=fi.module_name(),
                state_dict=[f"{k} {'x'.join(map(str, v.shape))}" for k, v in sorted(net.state_dict().items())])


def pack(records):
    """{case: record} -> the JSON document: the state_dict listings (the same for every output stride of a model, ~30 kB each) are
    stored once each in a table and referred to by index"""
    table, out = [], {}
    for cid, rec in records.items():
        rec = dict(rec)
        sd = "\n".join(rec["state_dict"])
        if sd not in table:
            table.append(sd)
        rec["state_dict"] = table.index(sd)
        out[cid] = rec
    return dict(cases=out, state_dicts=table)


def unpack(doc):
    return {cid: dict(rec, state_dict=doc["state_dicts"][rec["state_dict"]].split("\n")) for cid, rec in doc["cases"].items()}


# ---- numerics: a classifier model and a backbone of the same weights
def perturb(model, seed):
    """off the initialisation's symmetries: 1-D parameters (BatchNorm / GroupNorm affine, biases) jittered, the zero-initialised last
    BatchNorm of every block at 0.5 (with zeros every residual branch and its gradients vanish)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in model.parameters():
            if p.ndim == 1:
                p.add_(0.3 * torch.randn(p.shape, generator=g))
        for m in model.modules():
            if hasattr(m, "bn3") and hasattr(m, "conv3"):
                m.bn3.weight.fill_(0.5)
    return model


def twins(build_classifier, build_backbone, device, mixed=True, train=True, seed=0):
    """-> (classifier model, backbone) built from one seed; the classifier's state_dict (perturbed) loaded into the backbone through the
    documented departure (keys of dropped modules ignored)"""
    from cotnet_amd.features import load_classifier_state_dict
    from cotnet_amd.flat_sgd import to_mixed_bf16
    torch.manual_seed(seed)
    clsf = perturb(build_classifier(), seed + 1)
    torch.manual_seed(seed)
    body = build_backbone()
    load_classifier_state_dict(body, clsf.state_dict())
    out = []
    for m in (clsf, body):
        m = m.to(device)
        out.append((to_mixed_bf16(m) if mixed else m).train(train))
    return out


class Hooked:
    """what the classifier model computed at the tapped modules: .live[i] the tensor itself (part of the autograd graph), .clone[i] a
    clone taken when the module returned, .counts[i] cot_layer_fused.NODE_COUNTS at that moment (cumulative), .out the model's output"""

    def __init__(self):
        self.live, self.clone, self.counts, self.out = {}, {}, {}, None


@contextlib.contextmanager
def _pool_call_site(fn):
    from cotnet_amd import resnet
    orig = resnet.pool

    def pool(module, x):
        fn(x)
        return orig(module, x)
    resnet.pool = pool
    try:
        yield
    finally:
        resnet.pool = orig


def hooked_forward(clsf, x, features_only=True):
    """run the classifier model's forward_features (or its whole forward) with a hook on each of TAP_MODULES"""
    from cotnet_amd import cot_layer_fused as clf
    h = Hooked()
    handles = []

    def take(i, t, by_act1=False):
        if i in h.live and not by_act1:   # (tap 0 from the act1 hook wins over the hand-on site)
            return
        h.live[i], h.clone[i], h.counts[i] = t, t.detach().clone(), dict(clf.NODE_COUNTS)

    for i, name in enumerate(TAP_MODULES):
        handles.append(getattr(clsf, name).register_forward_hook(lambda m, a, o, i=i: take(i, o, by_act1=(i == 0))))
    if not hasattr(clsf, "maxpool"):
        handles.append(clsf.layer1.register_forward_pre_hook(lambda m, a: take(0, a[0])))
    clf.reset_node_counts()
    with _pool_call_site(lambda t: take(0, t)):
        h.out = clsf.forward_features(x) if features_only else clsf(x)
    for hd in handles:
        hd.remove()
    assert sorted(h.live) == [0, 1, 2, 3, 4], sorted(h.live)
    return h


def backbone_forward(body, x):
    """-> (taps as {index: tensor}, NODE_COUNTS of this forward)"""
    from cotnet_amd import cot_layer_fused as clf
    clf.reset_node_counts()
    taps = body(x)
    if isinstance(taps, (dict, OrderedDict)):
        taps = list(taps.values())
    idx = sorted(body.feature_info.out_indices)
    assert len(taps) == len(idx)
    return dict(zip(idx, taps)), dict(clf.NODE_COUNTS)


def check_taps(taps, counts, h, dtype, report=None):
    """every tap bit-equal to the hook's clone, laid out as a tap has to be; the node counts those of the classifier's forward up to the
    last kept stage.  `report`: a list the per-kind counts are appended to (the odd-plane / dilated cases record which blocks ran as
    nodes; nothing here asserts that the counts are maximal)."""
    from cotnet_amd.cot_block_cm import _is_cm
    for i, t in taps.items():
        assert t.dtype == dtype and t.shape == h.clone[i].shape, (i, t.dtype, t.shape)
        assert t.is_contiguous() and not _is_cm(t) and t.data_ptr() % 16 == 0, (i, t.stride(), t.data_ptr() % 16)
        assert torch.equal(t.detach(), h.clone[i]), f"tap {i} differs from the classifier's {TAP_MODULES[i]} output"
    assert counts == h.counts[max(taps)], (counts, h.counts[max(taps)])
    if report is not None:
        report.append({k: v for k, v in counts.items() if v})


def tap_weights(taps, seed, device):
    g = torch.Generator().manual_seed(seed)
    return {i: torch.randn(t.shape, generator=g).to(device) for i, t in taps.items()}


def tap_loss(taps, w):
    return sum((taps[i].float() * w[i]).sum() for i in sorted(w))


def kept_parameters(body, clsf):
    """[(name, backbone parameter, the classifier's parameter of that name)]"""
    cp = dict(clsf.named_parameters())
    return [(n, p, cp[n]) for n, p in body.named_parameters()]


def check_gradients(body, clsf, taps, h, seed=5):
    """the same loss on the taps and on the tensors the classifier's hooks saw: the same graph, so the parameter gradients are
    bit-equal"""
    w = tap_weights(taps, seed, next(iter(taps.values())).device)
    for m in (body, clsf):
        m.zero_grad(set_to_none=True)
    tap_loss(taps, w).backward()
    tap_loss({i: h.live[i] for i in taps}, w).backward()
    bad = []
    for n, p, q in kept_parameters(body, clsf):
        assert p.grad is not None, f"{n}: no gradient in the backbone"
        assert q.grad is not None, f"{n}: no gradient in the classifier model"
        if not torch.equal(p.grad, q.grad):
            bad.append(n)
    assert not bad, f"{len(bad)} parameter gradients differ bit-wise, first {bad[:5]}"


def check_lifetime(body, clsf, x, x2):
    """the taps of one forward against clones of them taken right away: after a backward (1), after a second forward of the backbone on
    another input (2) and after the classifier model's forward (3) they still hold the same bits; the second call's taps are other
    tensors"""
    taps, _ = backbone_forward(body, x)
    keep = {i: t.detach().clone() for i, t in taps.items()}

    def intact(when):
        bad = [i for i, t in taps.items() if not torch.equal(t.detach(), keep[i])]
        assert not bad, f"taps {bad} changed {when}"

    w = tap_weights(taps, 9, x.device)
    tap_loss(taps, w).backward()
    intact("during the backward")
    taps2, _ = backbone_forward(body, x2)
    intact("during the next forward")
    for i in taps:
        assert taps2[i] is not taps[i] and taps2[i].data_ptr() != taps[i].data_ptr(), i
        assert not torch.equal(taps2[i].detach(), keep[i]), i
    clsf(x)
    intact("during the classifier model's forward")
    return taps
