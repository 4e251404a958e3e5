"""Channel-major Bottlenecks of the 14 x 14 / 7 x 7 stages as ONE autograd node (split out of cot_layer_fused.py in round 6).
The node holds what is its own -- conv1 / bn1, conv3 / bn3, the shortcut, the layouts at its borders; the CoT layer between them is
cot_layer_fused._cot_forward / _cot_backward, called with the channel-major policy (rows 2-3 of the diagram below).
The switches (CM_LAYOUT, CM_OPENING, ENABLED, ...) stay attributes of cot_layer_fused and are read as clf.NAME at call time.
Imported by cot_layer_fused at its end: import THAT module.
"""
import torch
from torch.autograd import Function
from . import _lib
from ._lib import one_stream_query as _one_stream_query, ptr as _p, stream as _stream
from . import cot_layer_fused as clf
from .cot_layer_fused import (  # noqa: E402  (helpers; the switches are read as clf.NAME at call time: tests rebind them there)
    BF16, NODE_COUNTS, _Side, _block_plan, _bn_bwd, _bn_bwd_lay, _bn_fwd, _bn_fwd_lay, _conv1_bwd, _conv1x1_bwd, _conv1x1_dgrad,
    _conv1x1_wgrad, _cot_backward, _cot_forward, _drop_path_scale, _input_ok, _masks, _modes_ok, _new_guarded, _pack, _plan, _relu_mask,
    _unpack)

# ---- channel-major Bottlenecks for the 14 x 14 / 7 x 7 stages (round 5).  The layers of these stages spend their time in
# 1x1 convolutions and BatchNorms whose NCHW operands are N short rows per channel (392 / 98 bytes); stored channel-major --
# [C][N][HW], a channel = ONE row of N*HW elements -- the SAME kernels, called with N = 1 and HW' = N*HW, run 1.2-1.5x faster
# (profiles/r05_probe_cnhw.log).  So an identity-shortcut block keeps every operand of a 1x1 convolution channel-major and every
# operand of a plane kernel (grouped 3x3, aggregation) NCHW; the layout changes inside the BatchNorm / GroupNorm / radix kernels that
# sit between the two kinds anyway (cot_*_lay: one layout bit per tensor):
#     x -conv1-> c1 -bn1+relu-> a1 (NCHW, for the 3x3) + a1c (channel-major, for the 1x1s)
#     a1 -3x3-> k_pre (NCHW) -bn+relu-> k (cm);  [a1c | k] -1x1-> e0 -bn+relu-> e1 -1x1-> e3 (all cm) -GroupNorm-> w (NCHW)
#     a1c -1x1-> v_pre (cm) -bn-> v (NCHW);  aggregation(v, w) -> a -bn+silu-> y (NCHW);  radix tail(y, k) -> out (cm)
#     out -conv3-> c3 (cm) -bn3 + residual + relu-> block output (cm when the next block is one of these, else NCHW)
# The block's input / output tensor objects stay honest: a channel-major activation is a [N, C, H, W] tensor whose strides are
# (HW, N*HW, W, 1) -- any torch consumer computes the right thing with it.  Same parameters, buffers and state_dict as the module
# (models/cotnet.py:181-264).  COT_CM_LAYOUT=0 opts out.
_CM_SIZES = _lib.register_cache({})
_CM_OK = _lib.register_cache({})


def _is_cm(t):
    """[N, C, H, W] tensor stored [C][N][H][W] (dense)"""
    N, C, H, W = t.shape
    return N > 1 and C > 1 and t.stride() == (H * W, N * H * W, W, 1)


def _cm_view(buf):
    """dense [C, N, H, W] buffer -> the honest [N, C, H, W] tensor over it"""
    return buf.permute(1, 0, 2, 3)


def _cm_buf(t):
    """the dense [C, N, H, W] buffer under a channel-major [N, C, H, W] tensor"""
    return t.permute(1, 0, 2, 3)


def plan_stage_layouts(stage):
    """mark, once per stage, the blocks whose successor can take a channel-major input (so that they write one)"""
    blocks = list(stage.children())
    # the plan depends on both layout switches and on WHICH blocks the stage holds (a replaced block re-plans)
    key = (clf.CM_LAYOUT, clf.CM_OPENING, tuple(id(b) for b in blocks), tuple(b.training for b in blocks))
    if getattr(stage, "_cm_planned", None) == key:
        return
    for i, b in enumerate(blocks):
        nxt = blocks[i + 1] if i + 1 < len(blocks) else None
        # (an opening block takes NCHW: its conv1 / bn1 run at the input resolution, off the channel-resident kernels)
        # (... and only a successor in training mode runs the channel-major node: an eval-mode block inside a training stage would
        # take the module path on a strided tensor -- correct, but a silent performance cliff)
        b._next_cm = bool(clf.CM_LAYOUT and nxt is not None and nxt.training and _cm_static_ok(nxt) and not _block_plan(nxt).avd)
    stage._cm_planned = key


def _cm_static_ok(blk):
    from .cotnet import Bottleneck
    if not isinstance(blk, Bottleneck):
        return False
    bp = _block_plan(blk)
    identity = bp.ds_conv is None and not bp.avd and bp.conv1.in_channels == bp.conv3.out_channels
    # the stage's opening block (models/cotnet.py:228-264 with `avd` pooling in front of the layer and a stride-2 projection): conv1 /
    # bn1 / the pooling stay NCHW at the input resolution, the layer, conv3, bn3 and the projection's BatchNorm go channel-major
    opening = clf.CM_OPENING and bp.ds_conv is not None and bp.avd and bp.ds_stride == 2
    return bp.static_ok and (identity or opening)


@_lib.memo(_CM_SIZES)
def _cm_sizes(L, N, Cin, C, A, G, H, W, grouped=False, Cout=None):
    """Cin / Cout: the block's input / output channels (Cout given = the stage's opening block: conv1 on 2H x 2W NCHW planes, the
    projection on the sub-sampled input)"""
    HW, M = H * W, N * H * W
    gws = max(int(L.cot_convg_workspace(1, 2 * C, C // 2, 2, M, 1, 1)), int(L.cot_convg_workspace(1, C // 2, 9 * C // 8, 2, M, 1, 1)),
              int(L.cot_convg_workspace(1, C, C, 2, M, 1, 1))) if grouped else 0
    ws = max(gws, int(L.cot_conv3x3g_workspace(N, C, C, G, H, W)), int(L.cot_conv1x1_workspace(1, 2 * C, C // 2, M, 0)),
             int(L.cot_conv1x1_workspace(1, C // 2, 9 * C // 8, M, 1)), int(L.cot_conv1x1_workspace(1, C, C, M, 0)),
             int(L.cot_conv1x1_workspace(1, C, A, N, 1)), int(L.cot_conv1x1_workspace(1, A, 2 * C, N, 1)),
             int(L.cot_conv1x1_workspace(1, Cin, C, M, 0)), int(L.cot_conv1x1_workspace(1, C, Cout or Cin, M, 0)),
             int(L.cot_conv1x1_workspace(N, Cin, C, HW, 0)),
             *((int(L.cot_conv1x1_workspace(N, Cin, C, 4 * HW, 0)), int(L.cot_conv1x1_workspace(N, Cin, Cout, HW, 0))) if Cout else ()))
    return (ws, int(L.cot_bn_act_workspace(N, C)), int(L.cot_bn_act_workspace(1, C)), int(L.cot_bn_act_workspace(1, C // 2)),
            int(L.cot_bn_act_workspace(1, A)), int(L.cot_bn_act_workspace(1, Cout or Cin)))


@_lib.memo(_CM_OK)
def _cm_geometry_ok(L, N, Cin, C, H, W, grouped=False):
    HW = H * W
    v = bool(HW <= 256 and (N * HW) % 8 == 0 and N > 1 and C % 64 == 0
             and L.cot_bn_act_lay_covers(N, C, HW, BF16) and L.cot_bn_act_lay_covers(N, Cin, HW, BF16)
             and L.cot_conv1x1_lds_covers(Cin, Cin, 0, N * HW) and L.cot_conv1x1_lds_covers(C, C, 0, N * HW))
    if v and not grouped:
        v = bool(L.cot_conv1x1_lds_covers(2 * C, C, 1, N * HW) and L.cot_conv1x1_lds_covers(C // 2, C // 2, 0, N * HW))
    return v  # (CoXtLayer's grouped 1x1s: cot_conv1x1g_* routes each group to the tuned or the general kernels itself)


def cm_block_eligible(blk, x):
    """training-mode cotnet.Bottleneck of a deep stage (planes of at most 256 pixels, _cm_geometry_ok) on a tensor that is NCHW-contiguous
    or channel-major: an identity-shortcut block, or (CM_OPENING) the stage's stride-2 opening block on an NCHW tensor with even planes"""
    if not (clf.ENABLED and clf.CM_LAYOUT and blk.training and _input_ok(x, cm_allowed=True) and _cm_static_ok(blk)):
        return False
    bp = _block_plan(blk)
    N, Cin, H, W = x.shape
    if not (_modes_ok(bp, True) and Cin == bp.conv1.in_channels):
        return False
    if bp.avd:
        if not (x.is_contiguous() and H % 2 == 0 and W % 2 == 0):
            return False
        H, W = H // 2, W // 2
    # (the library is asked last: a block that fails a test above never touches it)
    return _cm_geometry_ok(_lib.lib(), N, bp.conv3.out_channels, bp.conv1.out_channels, H, W, _plan(bp.cot).grouped)


def cm_block_forward(blk, x):
    NODE_COUNTS["bottleneck_channel_major"] += 1
    return _BottleneckCMNode.apply(blk, x, *_block_plan(blk).params)


class _BottleneckCMNode(Function):
    @staticmethod
    @_one_stream_query
    def forward(ctx, blk, x, *params):
        L = _lib.api()
        bp = _block_plan(blk)
        pl = _plan(bp.cot)
        N, Cin, H0, W0 = x.shape
        opening = bp.avd   # the stage's first block: 3x3/2 average pooling in front of the layer, stride-2 projection shortcut
        H, W = (H0 // 2, W0 // 2) if opening else (H0, W0)
        C, A, G, Cout = bp.conv1.out_channels, pl.se0.out_channels, pl.ke0.groups, bp.conv3.out_channels
        HW, M = H * W, N * H * W
        dev, st = x.device, _stream()
        in_cm = _is_cm(x)
        out_cm = bool(getattr(blk, "_next_cm", False))
        # (CoXtLayer, models/cotnet.py:106-178: grouped 1x1s -- a group = a contiguous range of channel ROWS here --, [x, k] interleaved
        # row by row, the two groups folded into the batch for the aggregation: views of the NCHW tensors)
        ws_bytes, nws_c, nws_c1, nws_h1, nws_a, nws_o1 = _cm_sizes(L, N, Cin, C, A, G, H, W, pl.grouped, Cout if opening else None)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        masks = _masks(L, H, W, dev)
        nchw = lambda c: torch.empty((N, c, H, W), dtype=x.dtype, device=dev)  # noqa: E731
        cmj = lambda c: torch.empty((c, N, H, W), dtype=x.dtype, device=dev)   # noqa: E731  (dense channel-major buffers)
        stat = lambda c, nws: torch.empty(2 * c + nws, dtype=torch.float32, device=dev)  # noqa: E731
        xb = _cm_buf(x) if in_cm else x   # the dense buffer under x, either layout

        if opening:
            # conv1 -> bn1 + relu on the 2H x 2W input planes (NCHW, the ordinary kernels), pooled to H x W: a1 (NCHW with margins) and
            # its channel-major copy for the 1x1 convolutions
            c1 = torch.empty((N, C, H0, W0), dtype=x.dtype, device=dev)
            L.cot_conv1x1_forward(_p(xb), None, Cin, _p(bp.conv1.weight), None, _p(c1), N, Cin, C, H0 * W0, BF16, st)
            a1f = torch.empty_like(c1)
            s_1 = stat(C, nws_c)
            _bn_fwd(L, c1, a1f, bp.bn1, s_1, 2 * C, N, C, H0 * W0, 1)
            a1 = _new_guarded(N, C, H, W, x.dtype, dev)
            L.cot_avgpool3x3s2_forward(_p(a1f), _p(a1), N * C, H0, W0, BF16, st)
            a1c = a1.permute(1, 0, 2, 3).contiguous()
        else:
            # conv1 -> bn1 + relu -> a1 (NCHW with margins: the 3x3 weight gradient reads it shifted) and a1c (channel-major)
            c1 = cmj(C) if in_cm else nchw(C)
            n1, hw1 = (1, M) if in_cm else (N, HW)
            L.cot_conv1x1_forward(_p(xb), None, Cin, _p(bp.conv1.weight), None, _p(c1), n1, Cin, C, hw1, BF16, st)
            a1, a1c = _new_guarded(N, C, H, W, x.dtype, dev), cmj(C)
            s_1 = stat(C, 0)
            _bn_fwd_lay(L, c1, None, a1, a1c, bp.bn1, s_1, N, C, HW, 1, x_cm=in_cm, y2_cm=True)
        # the CoT layer (cot_layer_fused._cot_forward, channel-major policy): a1 for the 3x3, a1c for the 1x1s; its output channel-major
        cot_out, saved, geom = _cot_forward(L, bp.cot, a1, (a1c, ws, masks, nws_c, nws_h1, nws_a))
        # conv3 -> bn3 + residual + relu.  The residual: the block's input (identity) or bn(conv1x1(every second pixel of it))
        c3 = cmj(Cout)
        L.cot_conv1x1_forward(_p(cot_out), None, C, _p(bp.conv3.weight), None, _p(c3), 1, C, Cout, M, BF16, st)
        ps = _drop_path_scale(blk, N, dev)
        yb = cmj(Cout) if out_cm else nchw(Cout)
        if opening:
            xs = torch.empty((N, Cin, H, W), dtype=x.dtype, device=dev)
            L.cot_subsample2_forward(_p(xb), _p(xs), N * Cin, H0, W0, BF16, st)
            d0 = nchw(Cout)
            L.cot_conv1x1_forward(_p(xs), None, Cin, _p(bp.ds_conv.weight), None, _p(d0), N, Cin, Cout, HW, BF16, st)
            res_cm = out_cm  # (the projection's BatchNorm writes the layout bn3 writes)
            res = cmj(Cout) if res_cm else nchw(Cout)
            s_d = stat(Cout, 0)
            _bn_fwd_lay(L, d0, None, res, None, bp.ds_bn, s_d, N, Cout, HW, 0, y_cm=res_cm)
        else:
            xs = d0 = s_d = None
            res, res_cm = xb, in_cm
        m3 = None
        if res_cm and out_cm and ps is None:  # everything channel-major: the ordinary kernels on N*HW-element rows (16-byte accesses, sign mask)
            s_3 = stat(Cout, nws_o1)
            m3 = _relu_mask(L, 1, Cout, M, dev)
            _bn_fwd(L, c3, yb, bp.bn3, s_3, 2 * Cout, 1, Cout, M, 1, residual=res, mask=m3)
        else:
            s_3 = stat(Cout, 0)
            _bn_fwd_lay(L, c3, res, yb, None, bp.bn3, s_3, N, Cout, HW, 1, x_cm=True, res_cm=res_cm, y_cm=out_cm, ps=ps)
        ctx.blk, ctx.geom, ctx.flags = blk, geom, (in_cm, out_cm, res_cm)
        # (the layer's `x` is a1, its `xc` a1c)
        _pack(ctx, dict(saved, xb=xb, c1=c1, s_1=s_1, cot_out=cot_out, c3=c3, yb=yb, s_3=s_3, d0=d0, s_d=s_d, xs=xs, m3=m3, ps=ps))
        return _cm_view(yb) if out_cm else yb

    @staticmethod
    @_one_stream_query
    def backward(ctx, gout):
        L = _lib.api()
        blk = ctx.blk
        bp = _block_plan(blk)
        pl = _plan(bp.cot)
        s = _unpack(ctx)
        xb, c1, a1, c3, m3 = s.xb, s.c1, s.x, s.c3, s.m3
        in_cm, out_cm, res_cm = ctx.flags
        opening = bp.avd
        N, C, H, W = a1.shape
        Cin, Cout, A, G = bp.conv1.in_channels, c3.shape[0], pl.se0.out_channels, pl.ke0.groups
        HW, M = H * W, N * H * W
        H0, W0 = (xb.shape[2], xb.shape[3]) if opening else (H, W)
        dev, st = a1.device, _stream()
        ws_bytes, nws_c, nws_c1, nws_h1, nws_a, nws_o1 = _cm_sizes(L, N, Cin, C, A, G, H, W, pl.grouped, Cout if opening else None)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        masks = _masks(L, H, W, dev)
        side = _Side(dev, ws_bytes, ws, bp.params)
        nchw = lambda c: torch.empty((N, c, H, W), dtype=a1.dtype, device=dev)  # noqa: E731
        cmj = lambda c: torch.empty((c, N, H, W), dtype=a1.dtype, device=dev)   # noqa: E731
        # the upstream gradient in the layout the forward wrote its output in
        if out_cm:
            gb = _cm_buf(gout) if _is_cm(gout) else gout.permute(1, 0, 2, 3).contiguous()
        else:
            gb = gout.contiguous()
        # bn3 + residual + relu
        g_c3 = cmj(Cout)
        # identity shortcut, everything channel-major, a sign mask: the residual's gradient is folded into conv1's data gradient below
        fold = m3 is not None and in_cm and not opening and clf._res_fold_ok(L, 1, Cin, C, M)
        g_res = None if fold else (cmj(Cout) if res_cm else nchw(Cout))
        if m3 is not None:
            d_bn3_w, d_bn3_b = _bn_bwd(L, gb, c3, None, g_c3, bp.bn3, s.s_3, 1, Cout, M, 1, nws_o1, dres=g_res, mask=m3)
        else:
            d_bn3_w, d_bn3_b = _bn_bwd_lay(L, gb, None, c3, s.yb, g_c3, g_res, bp.bn3, s.s_3, N, Cout, HW, 1, dy_cm=out_cm, x_cm=True,
                                           y_cm=out_cm, dx_cm=True, dres_cm=res_cm, ps=s.ps)
        g_out = cmj(C)
        g_w3c, _ = _conv1x1_bwd(L, side, ws, bp.conv3, g_c3, s.cot_out, None, C, g_out, None, 0, 1, C, Cout, M)
        # the CoT layer: gxc = the 1x1s' channel-major contribution to da1, gx3 = the 3x3's NCHW one
        gxc, gx3, g_cot = _cot_backward(L, bp.cot, s, ctx.geom, g_out, side, (ws, masks, nws_c, nws_h1, nws_a))
        g_ds = ()
        if opening:
            # the pooled activation's gradient = the 3x3's NCHW contribution + the 1x1s' channel-major one (a strided add), back through the
            # pooling, bn1 and conv1 at the input resolution; the projection: its BatchNorm takes the residual gradient in bn3's layout
            gx3.add_(_cm_view(gxc))
            g_a1f = torch.empty((N, C, H0, W0), dtype=a1.dtype, device=dev)
            L.cot_avgpool3x3s2_backward(_p(gx3), _p(g_a1f), N * C, H0, W0, BF16, st)
            g_c1 = torch.empty_like(c1)
            d_bn1_w, d_bn1_b = _bn_bwd(L, g_a1f, c1, None, g_c1, bp.bn1, s.s_1, N, C, H0 * W0, 1, nws_c)
            g_d0 = nchw(Cout)
            d_ds_w, d_ds_b = _bn_bwd_lay(L, g_res, None, s.d0, None, g_d0, None, bp.ds_bn, s.s_d, N, Cout, HW, 0, dy_cm=res_cm)
            g_xs = torch.empty_like(s.xs)
            _conv1x1_dgrad(L, bp.ds_conv.weight, g_d0, g_xs, None, Cin, 0, ws, N, Cin, Cout, HW)
            gx = torch.empty_like(xb)
            L.cot_subsample2_backward(_p(g_xs), _p(gx), N * Cin, H0, W0, BF16, st)
            g_wd, _ = _conv1x1_wgrad(L, side, bp.ds_conv, g_d0, s.xs, None, Cin, N, Cin, Cout, HW)
            g_ds = (g_wd, d_ds_w, d_ds_b)
            gx, g_w1 = _conv1_bwd(L, side, ws, bp.conv1, g_c1, xb, gx, None, None, N, Cin, C, H0 * W0)
        else:
            # bn1: the two contributions to da1 (channel-major from the 1x1s, NCHW from the 3x3) meet in its backward
            g_c1 = cmj(C) if in_cm else nchw(C)
            d_bn1_w, d_bn1_b = _bn_bwd_lay(L, gxc, gx3, c1, None, g_c1, None, bp.bn1, s.s_1, N, C, HW, 1, dy_cm=True, x_cm=in_cm, dx_cm=in_cm)
            # identity shortcut: the residual's gradient is the first contribution to dx (None: folded into the data gradient)
            n1, hw1 = (1, M) if in_cm else (N, HW)
            gx, g_w1 = _conv1_bwd(L, side, ws, bp.conv1, g_c1, xb, g_res, gb, m3, n1, Cin, C, hw1)
        side.join()
        return (None, _cm_view(gx) if in_cm else gx, g_w1, d_bn1_w, d_bn1_b) + g_cot + (g_w3c, d_bn3_w, d_bn3_b) + g_ds
