"""CotLayer / Bottleneck as ONE autograd node (cotnet_amd/cot_layer_fused.py, opt-in COT_FUSED_LAYER=1) on the GPU.
Each composed result is compared with an fp32 evaluation of the same module (tests/truth.py): the single-node path must
not sit further from that truth than the round-1 path (MIOpen convolutions, one node per op) does."""
import copy

import pytest
import torch

from cotnet_amd import cot_layer_fused as clf
from cotnet_amd.cotnet import Bottleneck, CotLayer
from cotnet_amd.flat_sgd import to_mixed_bf16
from tests import truth

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("cls,N,C,H", [("CotLayer", 8, 64, 56), ("CotLayer", 8, 128, 28), ("CotLayer", 8, 256, 14), ("CotLayer", 8, 512, 7),
                                       # CoTNeXt's layer at its four real widths (cotnext*_2x48d: 96 / 192 / 384 / 768)
                                       ("CoXtLayer", 8, 96, 56), ("CoXtLayer", 8, 192, 28), ("CoXtLayer", 8, 384, 14),
                                       ("CoXtLayer", 8, 768, 7)])
def test_single_node_layer_against_fp32_truth(cls, N, C, H):
    from cotnet_amd import cotnet as cn
    torch.manual_seed(C)
    layer = getattr(cn, cls)(C, 3).to(DEV).train()
    with torch.no_grad():
        for p in layer.parameters():
            if p.ndim == 1:
                p.add_(0.3 * torch.randn_like(p))
    layer = to_mixed_bf16(layer)
    x = torch.randn(N, C, H, H, device=DEV).bfloat16()
    g = torch.randn(N, C, H, H, device=DEV).bfloat16()
    truth.check_against_truth(layer, x, g, cand=truth.SINGLE_NODE)
    # the node really is the single one, it returns a gradient for every parameter, and the BatchNorm buffers move as
    # torch's do
    _, _, gf, mf, node = truth.run(layer, x, g, want_module=True, **truth.SINGLE_NODE)
    assert node.startswith("_CotLayerNode")
    _, _, gr, mr, node_r = truth.run(layer, x, g, want_module=True, **truth.ROUND1)
    assert not node_r.startswith("_CotLayerNode")
    assert set(gf) == set(gr) == {n for n, _ in layer.named_parameters()}
    # running statistics: against the fp32 truth's buffers (bf16 activations move a batch variance by ~0.5 %, i.e. the
    # running variance by ~5e-4 after one momentum-0.1 update: both paths must stay in that class)
    *_, mt, _ = truth.run(copy.deepcopy(layer).float(), x.float(), g.float(), want_module=True, **truth.PLAIN)
    for (n_, a), (_, b), (_, tb) in zip(mf.named_buffers(), mr.named_buffers(), mt.named_buffers()):
        ea, eb = (a.float() - tb.float()).abs().max().item(), (b.float() - tb.float()).abs().max().item()
        assert ea <= 2.0 * eb + 2e-3 * (1 + tb.float().abs().max().item()), (n_, ea, eb)


def test_ineligible_inputs_take_the_ordinary_forward(monkeypatch):
    monkeypatch.setattr(clf, "ENABLED", True)
    layer = to_mixed_bf16(CotLayer(64, 3).to(DEV))
    x = torch.randn(2, 64, 8, 8, device=DEV).bfloat16()
    assert clf.eligible(layer.train(), x)
    assert not clf.eligible(layer.eval(), x)                                  # inference
    assert not clf.eligible(layer.train(), x.to(memory_format=torch.channels_last))
    assert not clf.eligible(CotLayer(64, 3).to(DEV).train(), x.float())       # fp32 model
    y = layer.eval()(x)
    assert y.shape == x.shape


def test_a_frozen_batchnorm_keeps_a_training_block_off_the_block_nodes():
    """partial freezing: bn3.eval() inside a training Bottleneck.  The block nodes normalise every BatchNorm with batch statistics and
    overwrite its running statistics, so the block has to take the module path, which leaves bn3's buffers alone; back in train() the
    block is one node again"""
    torch.manual_seed(3)
    blk = to_mixed_bf16(Bottleneck(256, 64).to(DEV).train())
    with torch.no_grad():
        blk.bn3.weight.fill_(0.8)
        blk.bn3.running_mean.normal_(0, 0.3)
        blk.bn3.running_var.uniform_(0.5, 1.5)
    x = torch.randn(2, 256, 14, 14, device=DEV).bfloat16()
    g = torch.randn(2, 256, 14, 14, device=DEV).bfloat16()
    bns = {n: m for n, m in blk.named_modules() if isinstance(m, torch.nn.BatchNorm2d)}
    assert len(bns) == 7

    def step():
        before = {n: int(m.num_batches_tracked) for n, m in bns.items()}
        clf.reset_node_counts()
        xi = x.clone().requires_grad_(True)
        blk(xi).backward(g)
        torch.cuda.synchronize()
        assert xi.grad is not None and blk.conv1.weight.grad is not None and blk.conv3.weight.grad is not None
        return {n: int(m.num_batches_tracked) - before[n] for n, m in bns.items()}

    with truth.switches(**truth.SINGLE_NODE, cm=True):
        blk.bn3.eval()
        frozen = [t.clone() for t in (blk.bn3.running_mean, blk.bn3.running_var, blk.bn3.num_batches_tracked)]
        moved = step()
        assert clf.NODE_COUNTS["bottleneck"] == clf.NODE_COUNTS["bottleneck_channel_major"] == 0
        for a, b in zip(frozen, (blk.bn3.running_mean, blk.bn3.running_var, blk.bn3.num_batches_tracked)):
            assert torch.equal(a, b)
        assert moved == {n: (0 if n == "bn3" else 1) for n in bns}
        blk.bn3.train()
        moved = step()
        assert clf.NODE_COUNTS["bottleneck"] + clf.NODE_COUNTS["bottleneck_channel_major"] == 1
        assert moved == {n: 1 for n in bns}
        assert not torch.equal(frozen[0], blk.bn3.running_mean)


def test_bottleneck_trains_with_the_single_node_layer():
    """two SGD steps of a Bottleneck with the fused layer node inside: loss decreases, parameters stay finite"""
    torch.manual_seed(0)
    blk = Bottleneck(256, 64).to(DEV).train()
    with torch.no_grad():
        blk.bn3.weight.fill_(1.0)
    blk = to_mixed_bf16(blk)
    x = torch.randn(8, 256, 28, 28, device=DEV).bfloat16()
    tgt = torch.randn(8, 256, 28, 28, device=DEV).bfloat16()
    opt = torch.optim.SGD(blk.parameters(), lr=1e-2)
    losses = []
    with truth.switches(**truth.SINGLE_NODE):
        for _ in range(3):
            opt.zero_grad()
            loss = (blk(x).float() - tgt.float()).square().mean()
            loss.backward()
            opt.step()
            losses.append(loss.item())
    assert losses[-1] < losses[0]
    assert all(torch.isfinite(p.float()).all() for p in blk.parameters())


@pytest.mark.parametrize("kind", ["identity", "project", "stride2", "coxt-identity", "coxt-project", "coxt-stride2"])
def test_single_node_bottleneck_against_fp32_truth(kind):
    """the whole Bottleneck as one node (identity shortcut / 1x1 projection / stride-2 block with avd pooling); coxt-* = CoTNeXt's
    block (cardinality 2, base width 48: a CoXtLayer of width 96 inside)"""
    from cotnet_amd.resnet import downsample_conv
    torch.manual_seed(7)
    coxt = kind.startswith("coxt-")
    kind = kind[5:] if coxt else kind
    stride = 2 if kind == "stride2" else 1
    inpl = 256 if kind == "identity" else 128
    ds = None if kind == "identity" else downsample_conv(inpl, 256, 1, stride=stride)
    blk = Bottleneck(inpl, 64, stride=stride, downsample=ds, **(dict(cardinality=2, base_width=48) if coxt else {})).to(DEV).train()
    assert type(blk.conv2).__name__ == ("CoXtLayer" if coxt else "CotLayer")
    with torch.no_grad():
        blk.bn3.weight.fill_(0.8)
    blk = to_mixed_bf16(blk)
    x = torch.randn(8, inpl, 28, 28, device=DEV).bfloat16()
    g = torch.randn(8, 256, 28 // stride, 28 // stride, device=DEV).bfloat16()
    truth.check_against_truth(blk, x, g, cand=truth.SINGLE_NODE)
    *_, node = truth.run(blk, x, g, want_module=True, **truth.SINGLE_NODE)
    # (a stride-2 block whose layer runs on 14 x 14 planes is a deep stage's opening block: the channel-major node)
    assert node.startswith(("_BottleneckNode", "_BottleneckCMNode") if kind == "stride2" else "_BottleneckNode")


@pytest.mark.parametrize("inpl,planes,hw", [(256, 64, 40), (512, 128, 20), (1024, 256, 20)])
def test_single_node_split_attn_block_against_fp32_truth(inpl, planes, hw):
    """SE-CoTNetD's SplitAttnConv2d(radix=1) bottleneck (identity shortcut) as ONE node (cot_layer_fused._SplitAttnBlockNode) at the
    widths / maps of se_cotnetd_152_L (320 x 320 input): conv1 -> bn1+relu -> dense 3x3 -> bn0+swish -> SE gate -> conv3 -> bn3 +
    residual + relu, against the fp32 truth; 256 -> 256 at 20 x 20 runs the LDS 3x3 kernel with two 128-row blocks per group"""
    from cotnet_amd.cotnet_hybrid import CoTBottleneck
    from cotnet_amd.layers import get_act_layer
    torch.manual_seed(hw + planes)
    # (block index 1: in the 256-wide stage the even blocks are CoT layers, the odd ones SplitAttn convolutions -- c4_idx)
    blk = CoTBottleneck(1, inpl, planes, conv_dim={64, 128}, c4_dim=256, c4_idx={0, 2}, radix=1, act_layer=get_act_layer("swish")).to(DEV).train()
    assert type(blk.conv2).__name__ == "SplitAttnConv2d"
    with torch.no_grad():
        blk.bn3.weight.fill_(0.8)
    blk = to_mixed_bf16(blk)
    x = torch.randn(8, inpl, hw, hw, device=DEV).bfloat16()
    g = torch.randn(8, inpl, hw, hw, device=DEV).bfloat16()
    truth.check_against_truth(blk, x, g, cand=truth.SINGLE_NODE)
    *_, node = truth.run(blk, x, g, want_module=True, **truth.SINGLE_NODE)
    assert node.startswith("_SplitAttnBlockNode")


@pytest.mark.parametrize("kind,inpl,planes,hw", [("split_attn", 128, 64, 160), ("split_attn", 256, 128, 80), ("cot", 512, 256, 40),
                                                 ("cot", 1024, 512, 20)])
def test_se_cotnetd_stage_opening_blocks_as_single_nodes_against_fp32_truth(kind, inpl, planes, hw):
    """SE-CoTNetD-152's four stage-opening blocks at their real widths / maps (320 x 320 input): BlurPool2d behind conv2 (avd_first False,
    models/cotnet_hybrid.py:196-199) and the `avg_down` projection shortcut (models/resnet.py:380-394) inside the single-node paths"""
    from cotnet_amd.cotnet_hybrid import CoTBottleneck
    from cotnet_amd.layers import BlurPool2d, get_act_layer
    from cotnet_amd.resnet import downsample_avg
    torch.manual_seed(hw + planes)
    blk = CoTBottleneck(0, inpl, planes, stride=2, downsample=downsample_avg(inpl, planes * 4, 1, stride=2), aa_layer=BlurPool2d, radix=1,
                        avd=True, avd_first=False, conv_dim={64, 128}, c4_dim=256, c4_idx={0, 2}, act_layer=get_act_layer("swish")).to(DEV).train()
    assert type(blk.conv2).__name__ == ("SplitAttnConv2d" if kind == "split_attn" else "CoTLayer")
    with torch.no_grad():
        blk.bn3.weight.fill_(0.8)
    blk = to_mixed_bf16(blk)
    N = 4
    x = torch.randn(N, inpl, hw, hw, device=DEV).bfloat16()
    g = torch.randn(N, planes * 4, hw // 2, hw // 2, device=DEV).bfloat16()
    truth.check_against_truth(blk, x, g, cand=truth.SINGLE_NODE)
    *_, node = truth.run(blk, x, g, want_module=True, **truth.SINGLE_NODE)
    assert node.startswith("_SplitAttnBlockNode" if kind == "split_attn" else "_BottleneckNode"), node


class _FixedDropPath(torch.nn.Module):
    """stochastic depth with a GIVEN per-sample scale (0 or 1 / keep): what models/layers/drop.py:140-168 computes, minus the draw"""

    def __init__(self, scale, p):
        super().__init__()
        self.drop_prob = p
        self.register_buffer("fixed_scale", scale)

    def forward(self, x):
        return x * self.fixed_scale.view(-1, 1, 1, 1).to(x.dtype) if self.training else x


@pytest.mark.parametrize("kind,hw", [("identity", 28), ("project", 14), ("stride2", 28), ("identity", 7)])
def test_single_node_bottleneck_with_stochastic_depth_against_fp32_truth(kind, hw):
    """the reference recipe's drop_path (config.yaml:21-26) on the single-node path: the per-sample scale is folded into the
    bn3 + residual + ReLU kernels (cot_bn_act_*_ps: streaming at 28 x 28, channel-resident at 14 x 14 / 7 x 7); same mask in
    the fp32 truth, the baseline (module per op) and the candidate"""
    from cotnet_amd.resnet import downsample_conv
    torch.manual_seed(11)
    stride = 2 if kind == "stride2" else 1
    inpl = 256 if kind == "identity" else 128
    ds = None if kind == "identity" else downsample_conv(inpl, 256, 1, stride=stride)
    N, keep = 8, 0.75
    scale = torch.tensor([0, 1, 1, 0, 1, 1, 1, 0], dtype=torch.float32, device=DEV) / keep
    blk = Bottleneck(inpl, 64, stride=stride, downsample=ds, drop_path=_FixedDropPath(scale, 1 - keep)).to(DEV).train()
    with torch.no_grad():
        blk.bn3.weight.fill_(0.8)
    blk = to_mixed_bf16(blk)
    x = torch.randn(N, inpl, hw, hw, device=DEV).bfloat16()
    g = torch.randn(N, 256, hw // stride, hw // stride, device=DEV).bfloat16()
    truth.check_against_truth(blk, x, g, cand=truth.SINGLE_NODE)
    y, _, _, _, node = truth.run(blk, x, g, want_module=True, **truth.SINGLE_NODE)
    # (the 7 x 7 identity block is a deep-stage block: the channel-major node, its bn3 with the per-sample scale on cot_bn_act_*_lay)
    assert node.startswith("_BottleneckCMNode" if (kind, hw) in (("identity", 7), ("stride2", 28)) else "_BottleneckNode")
    if kind == "identity":  # a dropped sample passes relu(x) on
        assert torch.equal(y[0], torch.relu(x[0].float()))


def test_recipe_model_runs_on_the_single_node_path():
    """cotnet50 built with the reference recipe's regularisation (drop 0.25, drop_path 0.1): every Bottleneck is still one
    autograd node, the head applies its dropout on the library path, one step trains"""
    import cotnet_amd
    torch.manual_seed(0)
    model = to_mixed_bf16(cotnet_amd.create_model("cotnet50", num_classes=1000, drop_rate=0.25, drop_path_rate=0.1).to(DEV)).train()
    x = torch.randn(4, 3, 224, 224, device=DEV).bfloat16()
    t = torch.randint(0, 1000, (4,), device=DEV)
    with truth.switches(**truth.SINGLE_NODE):
        names = []
        hooks = [m.register_forward_hook(lambda mod, i, o: names.append(o.grad_fn.name() if o.grad_fn is not None else ""))
                 for m in model.modules() if isinstance(m, Bottleneck)]
        logits = model(x)
        loss = torch.nn.functional.cross_entropy(logits.float(), t)
        loss.backward()
        for h in hooks:
            h.remove()
    # (one node per block: the identity blocks of layer3 / layer4 on the channel-major node -- N = 4 at 14 x 14 / 7 x 7 is below the
    # channel-resident kernels' batch, so here they may also take the NCHW node)
    assert len(names) == 16 and all(n.startswith(("_BottleneckNode", "_BottleneckCMNode")) for n in names)
    assert torch.isfinite(loss) and all(p.grad is not None and torch.isfinite(p.grad.float()).all() for p in model.parameters())


@pytest.mark.parametrize("N,planes,H,blocks,coxt", [(80, 256, 14, 3, False), (80, 512, 7, 2, False), (8, 256, 14, 2, False),
                                                      (64, 256, 14, 2, True), (64, 512, 7, 2, True)])  # (CoTNeXt-101 2x48d: widths 384 / 768, B = 64)
def test_channel_major_deep_stage_blocks_against_fp32_truth(N, planes, H, blocks, coxt):
    """a run of identity Bottlenecks of layer3 / layer4 (models/cotnet.py:181-264) at the benchmark batch through the channel-major
    node (cot_layer_fused._BottleneckCMNode: NCHW in -> channel-major between the blocks -> NCHW out): no further from
    an fp32 evaluation of the same modules than the NCHW single-node path is, same gradients / buffers surface"""
    from torch import nn
    torch.manual_seed(planes + H)
    inpl = 4 * planes
    kw = dict(cardinality=2, base_width=48) if coxt else {}
    stage = nn.Sequential(*[Bottleneck(inpl, planes, **kw) for _ in range(blocks)]).to(DEV).train()
    assert type(stage[0].conv2).__name__ == ("CoXtLayer" if coxt else "CotLayer")
    with torch.no_grad():
        for p in stage.parameters():
            if p.ndim == 1:
                p.add_(0.3 * torch.randn_like(p))
        for b in stage:
            b.bn3.weight.fill_(0.8)
    stage = to_mixed_bf16(stage)
    with truth.switches(cm=True):
        clf.plan_stage_layouts(stage)
    assert [b._next_cm for b in stage] == [True] * (blocks - 1) + [False]
    x = torch.randn(N, inpl, H, H, device=DEV).bfloat16()
    g = torch.randn(N, inpl, H, H, device=DEV).bfloat16()
    cand, base = dict(truth.SINGLE_NODE, cm=True), dict(truth.SINGLE_NODE, cm=False)
    truth.check_against_truth(stage, x, g, cand=cand, base=base)
    yc, gxc, gc, mc, node = truth.run(stage, x, g, want_module=True, **cand)
    yb, gxb, gb, mb, node_b = truth.run(stage, x, g, want_module=True, **base)
    assert node.startswith("_BottleneckCMNode") and node_b.startswith("_BottleneckNode")
    assert set(gc) == set(gb) == {n for n, _ in stage.named_parameters()}
    # (CoXtLayer: the channel-major node runs embed[0] as two-slab kernels per group -- other summation order than the NCHW node's grouped
    # kernel on the interleaved tensor, so the two sit ~9 % apart while both are ~14 % from the fp32 evaluation, which check_against_truth
    # above bounds; profiles/r06_gx_slabs_errors.log)
    assert truth.err(yc, yb) < 2e-2 and truth.err(gxc, gxb) < (0.12 if coxt else 8e-2)
    for (n_, a), (_, b) in zip(mc.named_buffers(), mb.named_buffers()):
        assert torch.allclose(a.float(), b.float(), atol=2e-3, rtol=2e-3), n_


@pytest.mark.parametrize("kind,N,hw", [("identity", 80, 14), ("identity", 80, 7), ("stride2", 16, 28), ("project", 16, 56)])
def test_eval_mode_bottleneck_single_call_sequence_against_fp32(kind, N, hw):
    """BASELINE config 2 (forward only, eval mode): cot_layer_fused.eval_block_forward no further from an fp32 evaluation of the same
    block (running statistics) than the module path is"""
    from cotnet_amd.resnet import downsample_conv
    torch.manual_seed(5 + hw)
    stride = 2 if kind == "stride2" else 1
    planes = {14: 256, 7: 512}.get(hw, 64) if kind == "identity" else 64
    inpl = 4 * planes if kind == "identity" else 2 * planes
    ds = None if kind == "identity" else downsample_conv(inpl, 4 * planes, 1, stride=stride)
    blk = Bottleneck(inpl, planes, stride=stride, downsample=ds).to(DEV)
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.3)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.2)
    blk = to_mixed_bf16(blk).eval()
    x = torch.randn(N, inpl, hw, hw, device=DEV).bfloat16()
    with torch.no_grad():
        with truth.switches(**truth.PLAIN):
            yt = copy.deepcopy(blk).float()(x.float())
        with truth.switches(**truth.ALL_HIP):
            yb = blk(x).float()
        with truth.switches(**truth.SINGLE_NODE):
            assert clf.eval_block_eligible(blk, x)
            clf.reset_node_counts()
            yc = blk(x).float()
            assert clf.NODE_COUNTS["bottleneck_eval"] == 1
    torch.cuda.synchronize()
    assert truth.err(yc, yt) <= 1.5 * truth.err(yb, yt) + 2e-3, (truth.err(yc, yt), truth.err(yb, yt))


@pytest.mark.parametrize("N,planes,H", [(80, 256, 28), (80, 512, 14)])
def test_channel_major_stage_with_its_opening_block_against_fp32_truth(N, planes, H):
    """layer3 / layer4 of CoTNet-50 from their stride-2 opening block on (avd pooling, projection shortcut) at the benchmark batch: the
    opening block's layer / conv3 / bn3 / projection BatchNorm and the identity block behind it channel-major"""
    from torch import nn
    from cotnet_amd.resnet import downsample_conv
    torch.manual_seed(planes + H)
    inpl, outp = 2 * planes, 4 * planes
    stage = nn.Sequential(Bottleneck(inpl, planes, stride=2, downsample=downsample_conv(inpl, outp, 1, stride=2)), Bottleneck(outp, planes)).to(DEV).train()
    with torch.no_grad():
        for p in stage.parameters():
            if p.ndim == 1:
                p.add_(0.3 * torch.randn_like(p))
        for b in stage:
            b.bn3.weight.fill_(0.8)
    stage = to_mixed_bf16(stage)
    with truth.switches(cm=True):
        clf.plan_stage_layouts(stage)
    assert [b._next_cm for b in stage] == [True, False]
    x = torch.randn(N, inpl, H, H, device=DEV).bfloat16()
    g = torch.randn(N, outp, H // 2, H // 2, device=DEV).bfloat16()
    cand, base = dict(truth.SINGLE_NODE, cm=True), dict(truth.SINGLE_NODE, cm=False)
    truth.check_against_truth(stage, x, g, cand=cand, base=base)
    yc, gxc, gc, mc, node = truth.run(stage, x, g, want_module=True, **cand)
    yb, gxb, gb, mb, node_b = truth.run(stage, x, g, want_module=True, **base)
    assert node.startswith("_BottleneckCMNode") and node_b.startswith("_BottleneckNode")
    assert set(gc) == set(gb) == {n for n, _ in stage.named_parameters()}
    assert truth.err(yc, yb) < 2e-2 and truth.err(gxc, gxb) < 8e-2
    for (n_, a), (_, b) in zip(mc.named_buffers(), mb.named_buffers()):
        assert torch.allclose(a.float(), b.float(), atol=2e-3, rtol=2e-3), n_
