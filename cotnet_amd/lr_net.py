"""LR-Net on MI355X -- drop-in for the reference's models/lr_net.py.

`SelfAttLayer` (ref :39-100), `Bottleneck` (ref :103-189), `Bottleneck_Ks3` (ref :191-201) and the entry points `lrnet50` /
`lrnet50_ks3` (ref :203-215) keep the reference's constructor signatures, sub-module names, attributes and construction order,
so the same seed gives the same initial weights and a reference state_dict loads with strict=True.  The forward pass computes
the same function:

  * the local relation -- unfold(k) + pos, product with q, sum over each head's 8 channels, window softmax, aggregation of v
    (ref :82-96) -- is one fused HIP op each way (cotnet_amd.local_relation, csrc/local_relation.hip): the unfolded keys,
    the logits and the products are never materialised;
  * the convolutions and BatchNorms run through the package's wrappers (conv1x1, conv3x3, fused_bn_act, pool,
    run_downsample), as cotnet.Bottleneck does.

`Bottleneck_K7` / `lrnet50_k7` are this package's own: the same network at LR-Net's 7x7 window, which the reference's layer takes
but none of its builders uses.

Unlike CoTNet's Bottleneck, the stride-2 average pool `avd` runs AFTER the attention layer (ref :170-171), so the layer sees
the stage's input resolution.
"""
import math

import torch
from torch import nn

from .aggregation_zeropad import LocalConvolution
from .conv1x1 import conv1x1, run_downsample
from .conv3x3g import conv3x3
from .cotnet import _cfg, act_name
from .fused_bn import fused_bn_act
from .local_relation import local_relation
from .pool3x3 import pool
from .registry import build_model_with_cfg, register_model
from .resnet import ResNet

default_cfgs = {"lrnet_basic": _cfg(url="")}


class SelfAttLayer(nn.Module):
    def __init__(self, dim, kernel_size, key_ks):
        super(SelfAttLayer, self).__init__()
        rel_factor = 1
        in_planes = dim
        rel_planes = dim // rel_factor
        out_planes = dim
        self.head_num = dim // rel_factor // 8
        self.kernel_size = kernel_size

        self.conv_q = nn.Sequential(
            nn.Conv2d(in_planes, rel_planes, kernel_size=1, bias=False),
            nn.BatchNorm2d(rel_planes),
            nn.ReLU(inplace=True))
        self.conv_k = nn.Sequential(  # key_ks = 3 (Bottleneck_Ks3): a dense 3x3 convolution (ref :56-67)
            nn.Conv2d(in_planes, rel_planes, kernel_size=key_ks, padding=key_ks // 2, bias=False),
            nn.BatchNorm2d(rel_planes),
            nn.ReLU(inplace=True))
        self.conv_v = nn.Sequential(
            nn.Conv2d(in_planes, out_planes, kernel_size=1, bias=False),
            nn.BatchNorm2d(out_planes))

        self.pos_h = nn.Parameter(torch.randn(rel_planes, self.kernel_size, 1))
        self.pos_w = nn.Parameter(torch.randn(rel_planes, 1, self.kernel_size))
        self.unfold = torch.nn.Unfold(kernel_size, 1, kernel_size // 2, 1)
        self.softmax = nn.Softmax(dim=2)

        self.local_conv = LocalConvolution(dim, dim, kernel_size=self.kernel_size, stride=1,
                                           padding=(self.kernel_size - 1) // 2, dilation=1)
        self.bn = nn.BatchNorm2d(dim)
        self.act = nn.ReLU(inplace=True)

    def forward(self, x):
        q = fused_bn_act(conv1x1(self.conv_q[0], x), self.conv_q[1], "relu")
        kc = self.conv_k[0]
        k = fused_bn_act(conv3x3(kc, x) if kc.kernel_size == (3, 3) else conv1x1(kc, x), self.conv_k[1], "relu")
        v = fused_bn_act(conv1x1(self.conv_v[0], x), self.conv_v[1], None)
        y = local_relation(q, k, v, self.pos_h, self.pos_w, self.kernel_size)
        return fused_bn_act(y, self.bn, "relu")


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, cardinality=1, base_width=64, reduce_first=1,
                 dilation=1, first_dilation=None, act_layer=nn.ReLU, norm_layer=nn.BatchNorm2d, attn_layer=None,
                 aa_layer=None, drop_block=None, drop_path=None):
        super(Bottleneck, self).__init__()
        assert attn_layer is None, "attn_layer is unused by the LR-Net entry points"
        width = int(math.floor(planes * (base_width / 64)) * cardinality)
        first_planes = width // reduce_first
        outplanes = planes * self.expansion

        self.conv1 = nn.Conv2d(inplanes, first_planes, kernel_size=1, bias=False)
        self.bn1 = norm_layer(first_planes)
        self.act1 = act_layer(inplace=True)
        self.avd = nn.AvgPool2d(3, 2, padding=1) if stride > 1 else None
        self.conv2 = SelfAttLayer(width, kernel_size=3, key_ks=1)
        self.conv3 = nn.Conv2d(width, outplanes, kernel_size=1, bias=False)
        self.bn3 = norm_layer(outplanes)
        self.se = None
        self.act3 = act_layer(inplace=True)
        self.downsample = downsample
        self.stride = stride
        self.dilation = dilation
        self.drop_block = drop_block
        self.drop_path = drop_path

    def zero_init_last_bn(self):
        nn.init.zeros_(self.bn3.weight)

    def forward(self, x):
        residual = x
        a1, a3 = act_name(self.act1), act_name(self.act3)
        fusable = self.drop_block is None and a1 is not False and a3 is not False
        if fusable:
            x = fused_bn_act(conv1x1(self.conv1, x), self.bn1, a1)
        else:
            x = self.bn1(self.conv1(x))
            if self.drop_block is not None:
                x = self.drop_block(x)
            x = self.act1(x)
        x = self.conv2(x)
        if self.avd is not None:  # after the attention layer (ref :170-171)
            x = pool(self.avd, x)
        x = conv1x1(self.conv3, x)
        if fusable and self.drop_path is None:
            if self.downsample is not None:
                residual = run_downsample(self.downsample, residual)
            return fused_bn_act(x, self.bn3, a3, residual)  # bn3 + residual add + act3 in one pass
        x = self.bn3(x)
        if self.drop_block is not None:
            x = self.drop_block(x)
        if self.drop_path is not None:
            x = self.drop_path(x)
        if self.downsample is not None:
            residual = run_downsample(self.downsample, residual)
        x += residual
        return self.act3(x)


class Bottleneck_Ks3(Bottleneck):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, cardinality=1, base_width=64, reduce_first=1,
                 dilation=1, first_dilation=None, act_layer=nn.ReLU, norm_layer=nn.BatchNorm2d, attn_layer=None,
                 aa_layer=None, drop_block=None, drop_path=None):
        super(Bottleneck_Ks3, self).__init__(inplanes, planes, stride, downsample, cardinality, base_width, reduce_first,
                                             dilation, first_dilation, act_layer, norm_layer, attn_layer, aa_layer,
                                             drop_block, drop_path)
        # the parent's key_ks = 1 layer is built first and replaced (ref :198-201): same random draws, same key order
        width = int(math.floor(planes * (base_width / 64)) * cardinality)
        self.conv2 = SelfAttLayer(width, kernel_size=3, key_ks=3)


class Bottleneck_K7(Bottleneck):
    """the block with LR-Net's own 7x7 window (the layer is parametric in it; the reference builds only 3x3 networks)"""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, cardinality=1, base_width=64, reduce_first=1,
                 dilation=1, first_dilation=None, act_layer=nn.ReLU, norm_layer=nn.BatchNorm2d, attn_layer=None,
                 aa_layer=None, drop_block=None, drop_path=None):
        super(Bottleneck_K7, self).__init__(inplanes, planes, stride, downsample, cardinality, base_width, reduce_first,
                                            dilation, first_dilation, act_layer, norm_layer, attn_layer, aa_layer,
                                            drop_block, drop_path)
        # built the way Bottleneck_Ks3 replaces conv2: the parent's layer first, then this one in its place
        width = int(math.floor(planes * (base_width / 64)) * cardinality)
        self.conv2 = SelfAttLayer(width, kernel_size=7, key_ks=1)


def _create_lrnet(variant, pretrained=False, **kwargs):
    return build_model_with_cfg(ResNet, variant, default_cfg=default_cfgs[variant], pretrained=pretrained, **kwargs)


@register_model
def lrnet50(pretrained=False, **kwargs):
    return _create_lrnet("lrnet_basic", pretrained, block=Bottleneck, layers=[3, 4, 6, 3], **kwargs)


@register_model
def lrnet50_ks3(pretrained=False, **kwargs):
    return _create_lrnet("lrnet_basic", pretrained, block=Bottleneck_Ks3, layers=[3, 4, 6, 3], **kwargs)


@register_model
def lrnet50_k7(pretrained=False, **kwargs):
    """LR-Net-50 with the 7x7 local relation (SelfAttLayer(width, kernel_size=7, key_ks=1), layers [3, 4, 6, 3]).  NOT a
    reference entry point: models/lr_net.py builds lrnet50 and lrnet50_ks3 only, so there is no reference state_dict to load
    and no reference fixture of the whole model; the layer itself is the reference's (tests/golden/lrnet_k7_layer_*)."""
    return _create_lrnet("lrnet_basic", pretrained, block=Bottleneck_K7, layers=[3, 4, 6, 3], **kwargs)
