"""Feature backbones on the device (cotnet_amd/features.py; the checks are tests/features_cases.py's).

The criterion is exact: a backbone built by `create_model(name, features_only=True, ...)` and loaded with a classifier model's
state_dict hands out, bit for bit, what forward hooks on that classifier model saw at act1 / layer1..4 for the same input in the same
mode, through the same nodes (cot_layer_fused.NODE_COUNTS per kind, up to the last kept stage); the parameter gradients of a loss on
the taps are bit-equal to those of the same loss on the hooked tensors; the taps stay intact through a backward, another forward and
the classifier model's forward; one FlatSGD step moves the kept weights alike; and a torch.cuda.graph capture of forward + loss +
backward replays bit-equal to the eager result.  The taps of a CAPTURED forward live in the graph's pool and are rewritten by the next
replay, like every tensor of a capture: read them before replaying again.

Inputs are the smallest where layout, aliasing or plane parity can still go wrong.  Planes below 7 x 7 are off the channel-major node's
geometries (cot_block_cm._cm_geometry_ok), so those cases run NCHW nodes; `test_channel_major_stages_at_224` is the one case at the
geometry where the deep stages do hand channel-major tensors from block to block.  The odd-plane and dilated cases print which node
kinds ran (pytest -s, and the `node_counts` property of the junit record); they do not assert that the counts are maximal.
"""
import pytest
import torch

import cotnet_amd
from tests import features_cases as fc, truth

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALL = (0, 1, 2, 3, 4)


@pytest.fixture(autouse=True)
def _reproducible_vendor_kernels():
    """Where a geometry is off the library's kernels the module path calls the vendor's convolution -- the 7 x 7 stem at 72 x 104 (its
    output width 52 is no multiple of 8: `stem_conv` falls back and counts it), SE-CoTNetD's strided 3 x 3 at small planes -- and that
    library's weight gradient is not reproducible call to call by default: on ONE model, one input, four backward passes, the stem's
    weight gradient at 72 x 104 came out in two different bit patterns (at 64 x 96, on the library's own kernel, in one).  With torch's
    deterministic switch the four are equal.  Bit-equality between two models is only defined over reproducible kernels, so these
    tests run with that switch on; it changes nothing in the library's own launches."""
    old = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = old


def _twins(name, out_indices=ALL, mixed=True, train=True, seed=0, **kw):
    return fc.twins(lambda: cotnet_amd.create_model(name, num_classes=10, **kw),
                    lambda: cotnet_amd.create_model(name, features_only=True, out_indices=out_indices, **kw), DEV, mixed, train, seed)


def _input(shape, seed, mixed=True):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(shape, device=DEV, generator=g)
    return x.bfloat16() if mixed else x


def _case(name, shape, out_indices=ALL, mixed=True, train=True, record=None, **kw):
    """hook equality, node counts, and -- in training mode -- bit-equal gradients; -> the backbone's node counts"""
    with truth.switches(**truth.SINGLE_NODE):
        clsf, body = _twins(name, out_indices, mixed, train, **kw)
        x = _input(shape, 7, mixed)
        with torch.enable_grad() if train else torch.no_grad():
            h = fc.hooked_forward(clsf, x)
            taps, counts = fc.backbone_forward(body, x)
            assert sorted(taps) == sorted(out_indices)
            report = []
            fc.check_taps(taps, counts, h, torch.bfloat16 if mixed else torch.float32, report)
            print(f"node counts {name} {tuple(shape)} {kw}: {report[0]}")
            if record is not None:
                record("node_counts", report[0])
            if train:
                assert all(t.requires_grad and t.grad_fn is not None for t in taps.values())
                fc.check_gradients(body, clsf, taps, h)
        torch.cuda.synchronize()
    return counts


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("out_indices", [ALL, (4,), (1, 2)], ids=["all", "4", "1_2"])
def test_cotnet50_even_planes(out_indices, train):
    """2 x 3 x 64 x 96: non-square, planes 32 x 48 ... 2 x 3, all even -- every kept block is node-eligible (eval: under no_grad, the
    inference call sequence)"""
    counts = _case("cotnet50", (2, 3, 64, 96), out_indices, train=train)
    blocks = sum([3, 4, 6, 3][:max(out_indices)])
    assert sum(counts.values()) == blocks and (train or counts["bottleneck_eval"] == blocks), counts
    if out_indices == (1, 2):
        body = cotnet_amd.create_model("cotnet50", features_only=True, out_indices=out_indices)
        assert not any(n.startswith("layer3") for n, _ in body.named_parameters())


def test_cotnet50_odd_planes(record_property):
    """2 x 3 x 72 x 104: planes 36 x 52, 18 x 26, 9 x 13, 5 x 7, 3 x 4 -- odd from layer2's output on, where a block with a pooled
    (avg_down) shortcut would fall off the even-plane rule of cot_layer_fused.block_eligible; cotnet50's strided 1 x 1 shortcuts do
    not, and all 16 blocks were seen to run as nodes.  What does leave the library here is the 7 x 7 stem (output width 52 is no
    multiple of 8: the vendor convolution, see _reproducible_vendor_kernels).  Equality is asserted whatever ran; the counts are
    recorded, not asserted."""
    _case("cotnet50", (2, 3, 72, 104), record=record_property)


@pytest.mark.parametrize("output_stride", [16, 8])
def test_cotnet50_dilated_stages(output_stride, record_property):
    """output_stride 16 / 8: layer4 (and layer3) at the plane size of the stage in front, stride-1 openers with dilated shortcuts"""
    _case("cotnet50", (2, 3, 64, 64), record=record_property, output_stride=output_stride)
    body = cotnet_amd.create_model("cotnet50", features_only=True, output_stride=output_stride)
    assert body.feature_info.reduction() == ([2, 4, 8, 16, 16] if output_stride == 16 else [2, 4, 8, 8, 8])


@pytest.mark.parametrize("name", ["cotnext50_2x48d", "se_cotnetd_50", "lrnet50_ks3"])
def test_other_families(name, record_property):
    """CoTNeXt's grouped layers, SE-CoTNetD's SplitAttn block nodes behind the deep stem with no max-pool, LR-Net's local relation"""
    _case(name, (2, 3, 64, 64), record=record_property)


def test_cotnet50_fp32_node_per_op():
    """fp32 parameters and input: no block is node-eligible, every op is its own autograd node"""
    counts = _case("cotnet50", (1, 3, 64, 64), mixed=False)
    assert not any(counts.values()), counts


def test_channel_major_stages_at_224():
    """2 x 3 x 224 x 224: layer3 / layer4 on the channel-major node (14 x 14, 7 x 7); their blocks hand channel-major tensors to their
    successors, and the last block of each stage writes the NCHW tensor that is the tap"""
    counts = _case("cotnet50", (2, 3, 224, 224))
    assert counts["bottleneck_channel_major"] >= 5 and sum(counts.values()) == 16, counts  # (B = 2: layer3; 2 * 49 pixels are off the rule)


def test_tap_lifetime():
    with truth.switches(**truth.SINGLE_NODE):
        clsf, body = _twins("cotnet50")
        fc.check_lifetime(body, clsf, _input((2, 3, 64, 96), 1), _input((2, 3, 64, 96), 2))
        torch.cuda.synchronize()


def test_tap_lifetime_channel_major():
    """the same where the deep stages run channel-major and reuse the most"""
    with truth.switches(**truth.SINGLE_NODE):
        clsf, body = _twins("cotnet50", (3, 4))
        fc.check_lifetime(body, clsf, _input((2, 3, 224, 224), 1), _input((2, 3, 224, 224), 2))
        torch.cuda.synchronize()


def test_dict_wrapper_with_out_map():
    from cotnet_amd.features import FeatureDictNet
    from cotnet_amd.registry import build_model_with_cfg
    with truth.switches(**truth.SINGLE_NODE):
        body = cotnet_amd.create_model("cotnet50", features_only=True, out_indices=(2, 4))
        sd = body.state_dict()
        from cotnet_amd.cotnet import Bottleneck, default_cfgs
        from cotnet_amd.resnet import ResNet
        dct = build_model_with_cfg(ResNet, "cotnet50", False, next(iter(default_cfgs.values())), features_only=True,
                                   feature_cfg=dict(feature_cls=FeatureDictNet, out_indices=(2, 4), out_map=("c3", "c5")),
                                   block=Bottleneck, layers=[3, 4, 6, 3])
        dct.load_state_dict(sd)
        from cotnet_amd.flat_sgd import to_mixed_bf16
        body, dct = (to_mixed_bf16(m.to(DEV)).train() for m in (body, dct))
        x = _input((2, 3, 64, 64), 3)
        a, b = body(x), dct(x)
        assert isinstance(a, list) and list(b) == ["c3", "c5"]
        assert torch.equal(a[0], b["c3"]) and torch.equal(a[1], b["c5"])
        torch.cuda.synchronize()


@pytest.mark.parametrize("out_indices", [ALL, (1, 2)], ids=["all", "1_2"])
def test_flat_sgd_step_moves_the_kept_weights_alike(out_indices):
    """FlatSGD on the backbone: the nodes write their weight gradients into its buckets (grad_sink); one step leaves the kept
    parameters bit-equal to those of the classifier model stepped by its own FlatSGD on the same loss"""
    from cotnet_amd.flat_sgd import FlatSGD
    with truth.switches(**truth.SINGLE_NODE):
        clsf, body = _twins("cotnet50", out_indices)
        before = {n: p.detach().clone() for n, p in body.named_parameters()}
        kw = dict(lr=0.1, momentum=0.9, weight_decay=4e-5, nesterov=True)
        oc, ob = FlatSGD(clsf, **kw), FlatSGD(body, **kw)
        x = _input((2, 3, 64, 96), 5)
        oc.zero_grad()
        ob.zero_grad()
        h = fc.hooked_forward(clsf, x)
        taps, _ = fc.backbone_forward(body, x)
        w = fc.tap_weights(taps, 6, DEV)
        fc.tap_loss({i: h.live[i] for i in taps}, w).backward()
        fc.tap_loss(taps, w).backward()
        oc.step()
        ob.step()
        torch.cuda.synchronize()
        bad = [n for n, p, q in fc.kept_parameters(body, clsf) if not torch.equal(p, q)]
        assert not bad, f"{len(bad)} parameters differ after the step, first {bad[:5]}"
        moved = sum(not torch.equal(p.detach(), before[n]) for n, p in body.named_parameters())
        assert moved >= len(before) // 2, (moved, len(before))  # (an update below half a bf16 ulp leaves a weight where it was)


def test_replayed_forward_loss_backward():
    """torch.cuda.graph capture of backbone forward + loss + backward at 2 x 3 x 64 x 96 after eager warm-up; three replays on new inputs
    written in place, each bit-equal -- taps, loss, every parameter gradient -- to the eager result on that input"""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with truth.switches(**truth.SINGLE_NODE), torch.cuda.stream(s):
        _, body = _twins("cotnet50")
        xs = [_input((2, 3, 64, 96), 20 + i) for i in range(4)]
        x = torch.empty_like(xs[0])
        w = None
        params = list(body.parameters())

        def step():
            body.zero_grad(set_to_none=True)
            taps = body(x)
            loss = sum((t.float() * wi).sum() for t, wi in zip(taps, w))
            loss.backward()
            return taps, loss

        eager = []
        for xi in xs:  # (the eager runs are the warm-up; no weight moves, and training-mode BatchNorm does not read its running statistics)
            x.copy_(xi)
            if w is None:
                w = [torch.randn(t.shape, device=DEV) for t in body(x)]
            taps, loss = step()
            eager.append(([t.detach().clone() for t in taps], loss.detach().clone(), [p.grad.clone() for p in params]))
        assert not torch.equal(eager[1][1], eager[2][1])
        g = torch.cuda.CUDAGraph()
        x.copy_(xs[0])
        with torch.cuda.graph(g, stream=s):
            taps, loss = step()
        for xi, (t_ref, l_ref, g_ref) in zip(xs[1:], eager[1:]):
            x.copy_(xi)
            g.replay()
            assert torch.equal(loss, l_ref)
            assert all(torch.equal(a.detach(), b) for a, b in zip(taps, t_ref))
            bad = [i for i, (p, r) in enumerate(zip(params, g_ref)) if not torch.equal(p.grad, r)]
            assert not bad, f"{len(bad)} parameter gradients differ between replay and eager, first {bad[:5]}"
        torch.cuda.synchronize()
        del g
    torch.cuda.current_stream().wait_stream(s)
