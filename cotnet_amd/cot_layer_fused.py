"""CotLayer / CoXtLayer .forward -- and the Bottleneck around them -- as ONE autograd node (default on; COT_FUSED_LAYER=0 opts out).

Why: at the reference's batch (80 / GPU) the round-1 CoTNet-50 step on MI355X was bound by the host, not the device
(~3100 launches, ~38 ms of Python/dispatch per step against 36 ms of kernels).  One CotLayer is ~14 autograd
nodes forward and as many backward, plus the engine's gradient-accumulation adds wherever a tensor has several consumers
(x feeds key_embed, embed and conv1x1: two adds of C*H*W; k feeds embed and the radix tail: one more).  This module
evaluates the same function (models/cotnet.py:79-104) by calling the library's kernels back to back through the C ABI:

    forward   conv3x3g -> bn+relu -> conv1x1 on [x | k] (no cat) -> bn+relu -> conv1x1(+bias) -> GroupNorm
              -> conv1x1 -> bn -> aggregation -> bn+silu -> radix gap (channel-major) -> se branch as two 1x1
              convolutions over the batch axis with its BatchNorm+ReLU between them -> pair softmax + radix mix
    backward  the mirror image; the three contributions to dx and the two to dk are summed inside the data-gradient
              kernels (`accumulate`), not by separate add kernels.

Same parameters, buffers (running statistics, num_batches_tracked) and state_dict as the module it is applied to;
eligible in training mode for bf16 NCHW tensors with dim % 64 == 0 (every CoTNet stage; CoXtLayer -- CoTNeXt's grouped
variant, models/cotnet.py:106-178 -- with dim % 32 == 0: its grouped 1x1 convolutions run on cot_conv1x1g_*, [x, k] is
interleaved once and the group -> batch fold is a view); anything else takes the module's ordinary forward.  Verified against the unfused reference formula through the host-emulated kernels
(tests/test_kernels_emulated.py) and on the GPU against an fp32 truth by tests/test_fused_layer_gpu.py; round 2 on the
MI355X: ~1290 launches and 19.1 ms per step with every kernel from cotnet_amd/csrc.
"""
import ctypes
import os
import weakref
from types import SimpleNamespace

import torch
from torch import nn
from torch.autograd import Function

from . import _lib, grad_sink
from ._lib import one_stream_query as _one_stream_query, ptr as _p, stream as _stream

ENABLED = os.environ.get("COT_FUSED_LAYER", "1") != "0"  # default on; COT_FUSED_LAYER=0 = one autograd node per op
BF16 = _lib.COT_BF16


# ---- weight gradients on a side stream.  A parameter gradient is needed only when the step's backward is over, while the
# data-gradient chain it hangs off is the critical path: 100 weight-gradient launches (+ their split reduces) per CoTNet-50
# step, ~3 ms of device time in which 256-workgroup GEMM slices and their launch ramps sit between bandwidth-bound
# BatchNorm / data-gradient kernels that never need all the matrix pipes.  So every weight gradient of a node's backward is
# issued on ONE extra HIP stream per device: it waits (event) for what the compute stream has produced so far, runs beside
# the rest of the node's backward, and the compute stream joins it (event) before the node returns -- i.e. before autograd
# hands the gradients to anybody.  Rules that keep this race-free:
#   * a tensor read by a side-stream launch is never written again inside the node (no buffer reuse for them below) and is
#     kept referenced until the join (the caching allocator could otherwise hand its memory to a later compute-stream tensor);
#   * the side stream is in-order, so its launches share ONE persistent workspace of their own (partial sums are consumed by
#     the same launch's reduce); the compute stream's workspace is never touched by it.
# COT_WGRAD_STREAM=0 (or cot_layer_fused.SIDE_WGRAD = False) issues everything on the compute stream as before (A/B, tests).
#
# COT_WGRAD_LAZY=1 (default): the node's weight-gradient launches are QUEUED and issued together when its backward ends --
# one event pair for the node instead of one per launch (ten per Bottleneck: each pair is ~8 us of host time and a barrier
# packet on both queues) -- and the compute stream does not join them there: they run beside the NEXT node's backward.  The
# compute stream joins the side stream (a) at the next node's flush, which is also when the tensors the previous node's
# launches read are released, and (b) when the backward pass ends (autograd engine callback), i.e. before an optimizer or
# anybody else on the compute stream can see the gradients; a gradient bucket that launches its all-reduce mid-backward makes
# its communication stream wait for the side stream (grad_sink.producer_streams).  The un-joined form is taken ONLY by nodes
# whose parameter gradients are all flat-bucket aliases that autograd merely adopts (_Side.adopted_only: FlatSGD / the
# copy-mode reducer, the measured configuration); any node that hands autograd an ordinary gradient tensor, runs under
# create_graph or sees a foreign hook joins its side stream before it returns, exactly like COT_WGRAD_LAZY=0.
SIDE_WGRAD = os.environ.get("COT_WGRAD_STREAM", "1") != "0"
LAZY_WGRAD = os.environ.get("COT_WGRAD_LAZY", "1") != "0"
_SIDE_STREAMS = {}  # device index -> [torch.cuda.Stream, workspace tensor]
_SIDE_PENDING = {}  # device index -> {"keep": tensors read by launches the compute stream has not joined yet}


def _join_pending(dev_index):
    """the compute stream waits for everything issued on the side stream so far; the tensors those launches read are released"""
    ent, pend = _SIDE_STREAMS.get(dev_index), _SIDE_PENDING.get(dev_index)
    if ent is None or pend is None:
        return
    if pend["keep"]:
        cur = torch.cuda.current_stream(torch.device("cuda", dev_index))
        cur.wait_stream(ent[0])
        main = pend.get("main")  # the stream the node's backward ran on: the caller may sit on another one by now (backward
        if main is not None and main != cur:  # under a different ambient stream, re-entrant backward)
            main.wait_stream(ent[0])
        pend["keep"] = []


class _Side:
    """the side stream for one node's backward (or a pass-through onto the compute stream when switched off / on CPU tensors)"""
    __slots__ = ("on", "main", "stream", "st", "ws", "keep", "lazy", "queue", "dev", "fresh0", "params")

    def __init__(self, dev, ws_bytes, main_ws, params=()):
        self.on = SIDE_WGRAD and _lib.DEVICE_ONLY and dev.type == "cuda"
        self.lazy = self.on and LAZY_WGRAD
        self.keep, self.queue, self.dev = [], [], dev
        self.fresh0, self.params = grad_sink.fresh_count(), params
        if not self.on:
            self.st, self.ws = _stream(), main_ws
            return
        ent = _SIDE_STREAMS.get(dev.index)
        if ent is None:
            ent = _SIDE_STREAMS[dev.index] = [torch.cuda.Stream(device=dev), None]
        self.main = torch.cuda.current_stream(dev)
        self.stream = ent[0]
        if ent[1] is None or ent[1].numel() < ws_bytes:
            with torch.cuda.stream(self.stream):  # (owned by the side stream's pool; grown, never shrunk)
                ent[1] = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        self.ws = ent[1]
        self.st = ctypes.c_void_p(self.stream.cuda_stream)
        if self.lazy and dev.index not in _SIDE_PENDING:
            _SIDE_PENDING[dev.index] = {"keep": []}
            grad_sink.register_producer_stream(self.stream, lambda i=dev.index: _join_pending(i))

    def run(self, fn, *tensors):
        """fn(stream handle) launches ONE weight gradient that reads `tensors` (all of them final when this is called)"""
        if self.lazy:
            self.queue.append(fn)
            self.keep.extend(tensors)
        else:
            fn(self.ready(*tensors))

    def ready(self, *tensors):
        """call right before a side-stream launch that reads `tensors`: everything the compute stream has issued so far is
        ordered before it, and the tensors stay alive until join()"""
        if self.on:
            self.stream.wait_stream(self.main)
            self.keep.extend(tensors)
        return self.st

    def adopted_only(self):
        """True when nobody can READ this node's parameter gradients before the backward pass ends: every one of them is an
        alias of its flat-bucket slot (grad_sink: autograd adopts it, and the copy-mode reducer that owns the slot makes its
        communication stream wait for the side stream), no graph is being recorded (create_graph=True makes AccumulateGrad
        clone what it is handed) and no foreign tensor / post-accumulate hook sits on a parameter.  An ORDINARY gradient
        tensor is accumulated by autograd on the compute stream right after the node returns (`p.grad += g` when a gradient
        exists already: a second backward without zero_grad, micro-batches, a view-mode reducer, a parameter used twice) --
        while the side stream may still be writing it.  Only the first kind of node may leave its weight
        gradients un-joined."""
        if grad_sink.fresh_count() != self.fresh0 or torch.is_grad_enabled():
            return False
        for p in self.params:
            if p._backward_hooks:
                return False
            h = p._post_accumulate_grad_hooks
            if h is not None and len(h) > 1:  # (one = the reducer that registered the sink)
                return False
        return True

    def join(self):
        if self.lazy:
            pend = _SIDE_PENDING[self.dev.index]
            if pend["keep"]:  # the previous node's launches: long done by now; their inputs may go
                self.main.wait_stream(self.stream)
            pend["keep"], pend["main"] = self.keep, self.main
            self.stream.wait_stream(self.main)
            for fn in self.queue:
                fn(self.st)
            self.queue, self.keep = [], []
            if not self.adopted_only():  # somebody may read the gradients as soon as the node returns: join here
                self.main.wait_stream(self.stream)
                pend["keep"] = []
                return
            # join when the backward pass ends.  Queued by EVERY flush (the first callback to run joins, the others find nothing
            # pending): a flag "already queued" would survive a backward pass that died half-way and silence all later ones
            try:
                torch.autograd.Variable._execution_engine.queue_callback(lambda i=self.dev.index: _join_pending(i))
            except RuntimeError:  # (not inside the engine's backward: join now)
                _join_pending(self.dev.index)
        elif self.on:
            self.main.wait_stream(self.stream)
            self.keep.clear()


GN_FUSED = os.environ.get("COT_GN_FUSED", "1") != "0"  # GroupNorm-9 statistics in embed[3]'s epilogue + normalisation in the aggregation's prologue
_GN_OK = _lib.register_cache({})


@_lib.memo(_GN_OK)
def _gn_fused_ok(L, Ch, HW, W):
    return bool(L.cot_gn9_fused_covers(Ch, Ch, 0, HW, W))


# BatchNorm + SiLU of the aggregation's output folded into the radix tail (round 6; VERDICT r5 J1 / next #2b; models/cotnet.py:89-104):
# a statistics pass over `a`, then the pooling and the mix kernels normalise + activate as they load (cot_radix_*_bn) -- y = silu(bn(a))
# is never written; backward: two launches (reduce, apply) instead of four, the BatchNorm's channel sums out of the reduce kernel's
# plane sums.  COT_BN_TAIL=0 = the separate cot_bn_act_* kernels as before.
BN_TAIL = os.environ.get("COT_BN_TAIL", "1") != "0"


# ... and, opt-in (COT_AGG_ROWSTATS=1), its statistics out of the aggregation's own epilogue (cot_agg_forward_rowstats +
# cot_bn_rowstats_finalize) where the LDS forward kernel serves the geometry: no statistics pass over `a` at all.  Built, parity-green and
# measured: the epilogue costs the aggregation +5.7 / +3.0 / +1.7 / -0.8 us at 56 / 28 / 14 / 7 pixels and its finalize 6.4-7.4 us, against
# 10.3-14.9 us for cot_bn_batch_stats -- 37.1 -> 35.3, 26.6 -> 26.1, 20.5 -> 18.3, 20.7 -> 15.4 us per layer, and the step does not move
# (13.56 vs 13.56 ms, alternating; profiles/r06_rowstats_kernels.log, r06_rowstats_ab.log): default off.
AGG_ROWSTATS = os.environ.get("COT_AGG_ROWSTATS", "0") == "1"
_ROWSTATS_OK = _lib.register_cache({})


def _agg_fwd_stats(L, v, w_or_logits, a, gn, gn_mean, gn_rstd, geom, bn, stats, N, C, H, W):
    """a = aggregation(v, w) and what bn's batch statistics of a are made of.  -> True: mean / rstd are in stats[:C] / stats[C:2C] and
    the running statistics updated; False: stats[2C:] holds chunk sums that the pooling kernel's prologue finalizes (_tail_gap).  gn
    given: w_or_logits holds the raw logits and the GroupNorm is applied in the aggregation's prologue (cot_agg_gn9_forward's contract)."""
    st = _stream()
    key = (geom.N, geom.C, H, W, geom.wC, gn is not None)
    if AGG_ROWSTATS and _ROWSTATS_OK.get(key, True):
        rows = torch.empty(int(L.cot_agg_rowstats_floats(N, C, H)), dtype=torch.float32, device=a.device)
        try:
            L.cot_agg_forward_rowstats(_p(v), _p(w_or_logits), _p(a), _p(rows), _p(gn_mean) if gn is not None else None,
                                       _p(gn_rstd) if gn is not None else None, _p(gn.weight) if gn is not None else None,
                                       _p(gn.bias) if gn is not None else None, gn.num_groups if gn is not None else 0,
                                       ctypes.byref(geom), BF16, st)
        except _lib.CotError as e:
            if e.status != _lib.COT_ERR_UNSUPPORTED:
                raise
        else:
            L.cot_bn_rowstats_finalize(_p(rows), _p(stats), _p(stats[C:]), _p(bn.running_mean), _p(bn.running_var),
                                       _p(bn.num_batches_tracked), N, C, H, W, float(bn.eps), float(bn.momentum), st)
            return True
        _ROWSTATS_OK[key] = False  # (geometry off the LDS forward kernel: the plain forward + a statistics pass, from now on without asking)
    if gn is not None:
        L.cot_agg_gn9_forward(_p(v), _p(w_or_logits), _p(gn_mean), _p(gn_rstd), _p(gn.weight), _p(gn.bias), gn.num_groups, _p(a),
                              ctypes.byref(geom), BF16, st)
    else:
        L.cot_agg_forward(_p(v), _p(w_or_logits), _p(a), ctypes.byref(geom), BF16, _lib.COT_NCHW, st)
    L.cot_bn_stats_sums(_p(a), _p(stats[2 * C:]), N, C, H * W, BF16, st)
    return False


def _tail_gap(L, a, k, gapT, bn, stats, final, N, C, HW, lay):
    """gapT = mean_hw(silu(bn(a)) + k); final False: stats[2C:] holds cot_bn_stats_sums' chunk sums and this launch finalizes them"""
    L.cot_radix_gap_t_bn(_p(a), _p(k), _p(gapT), _p(bn.weight), _p(bn.bias), _p(stats), _p(stats[C:]), _p(bn.running_mean),
                         _p(bn.running_var), _p(bn.num_batches_tracked), None if final else _p(stats[2 * C:]), N, C, HW, float(bn.eps),
                         float(bn.momentum), lay, BF16, _stream())

_SIZES = _lib.register_cache({})  # (N, C, H, W, A) -> (workspace bytes, bn workspace floats for C, C/2 and the se branch's A channels)
_MASKS = {}


@_lib.memo(_SIZES)
def _sizes(L, N, C, H, W, A, G, grouped=False):
    HW = H * W
    if grouped:  # CoXtLayer: the three 1x1 convolutions of the layer are grouped (groups = 2): general kernels' workspace
        ws = max(int(L.cot_conv3x3g_workspace(N, C, C, G, H, W)), int(L.cot_conv3x3g_workspace(N, C, C, _conv3x3_ws_groups(C, G), H, W)),
                 int(L.cot_convg_workspace(N, 2 * C, C // 2, 2, H, W, 1)),
                 int(L.cot_convg_workspace(N, C // 2, 9 * C // 8, 2, H, W, 1)), int(L.cot_convg_workspace(N, C, C, 2, H, W, 1)),
                 int(L.cot_conv1x1_workspace(1, C, A, N, 1)), int(L.cot_conv1x1_workspace(1, A, 2 * C, N, 1)))
    else:
        ws = max(int(L.cot_conv3x3g_workspace(N, C, C, G, H, W)), int(L.cot_conv1x1_workspace(N, 2 * C, C // 2, HW, 0)),
                 int(L.cot_conv1x1_workspace(N, C // 2, 9 * C // 8, HW, 1)), int(L.cot_conv1x1_workspace(N, C, C, HW, 0)),
                 int(L.cot_conv1x1_workspace(1, C, A, N, 1)), int(L.cot_conv1x1_workspace(1, A, 2 * C, N, 1)))
    return ws, int(L.cot_bn_act_workspace(N, C)), int(L.cot_bn_act_workspace(N, C // 2)), int(L.cot_bn_act_workspace(1, A))


def _masks(L, H, W, device):
    k = (H, W, str(device))
    m = _MASKS.get(k)
    if m is None:
        m = torch.empty(int(L.cot_conv3x3g_masks_bytes(H, W)), dtype=torch.uint8, device=device)
        L.cot_conv3x3g_masks(_p(m), H, W, _stream())
        # a capture records the launch and does not run it: a table first made there serves this call (the replay fills it), and an eager
        # call afterwards must not find it in the cache with nothing written yet -- _pack_for's policy: cache nothing while capturing
        if not _capturing():
            _MASKS[k] = m
    return m


# ---- grouped 3x3 weights packed ahead of time (round 5).  The LDS kernels run on a re-ordered copy of the weights;
# the ordinary entry points make it per call (two 5 us launches per layer and step on the compute stream: 32 launches, 0.16 ms).  A
# layer's weights change once per optimizer step and each packing is used once per step, so nothing is saved in work -- but the packing
# need not sit on the critical path: right after the flat SGD kernels (FlatSGD.step -> after_optimizer_step) both packings of every
# layer seen in the last forward are made on the weight-gradient side stream, into persistent buffers, and the next step's forward /
# backward run `cot_conv3x3g_*_packed`.  Validity = (storage pointer, torch's version counter, the optimizer epoch below -- the flat
# SGD kernel writes through raw pointers, which torch's counter does not see --, geometry).  Never inside a graph capture (a replay
# would keep reading the packing of the capture): captured steps pack inline as before.  (Round 6 tried the scheme INSIDE a whole-step
# capture -- packings re-made behind the captured SGD kernels, read by the next replay; loss trajectory identical to eager -- and
# measured nothing: 13.82 / 13.80 ms with / without, profiles/r06_prepack_in_capture_ab.log; the inline packing launches are not on
# a replayed step's critical path.  Not kept.)  COT_PREPACK=0 opts out.
PREPACK = os.environ.get("COT_PREPACK", "1") != "0"
PARAM_EPOCH = [0]
_PACKS = weakref.WeakKeyDictionary()   # nn.Conv2d -> {"geom": (N, C, G, H, W), 0: (key, buffer), 1: (key, buffer)}
_PACK_EVENT = {}                       # device index -> event the compute stream has to wait for before its first packed launch


def _capturing():
    return _lib.capturing()


def _pack_for(L, conv, mode, N, C, G, H, W):
    """-> the valid packing of conv.weight for this call, or None (the caller then packs inline through the ordinary entry point).
    Also remembers the geometry for after_optimizer_step."""
    if not (PREPACK and _lib.DEVICE_ONLY):
        return None
    e = _PACKS.get(conv)
    if e is None:
        e = _PACKS[conv] = {}
    if _capturing():
        e.pop("geom", None)
        return None
    wt = conv.weight
    e["geom"] = (N, C, G, H, W)
    ent = e.get(mode)
    if ent is not None and ent[0] == (wt.data_ptr(), wt._version, PARAM_EPOCH[0], N, C, G, H, W):
        ev = _PACK_EVENT.pop(wt.device.index, None)
        if ev is not None:
            torch.cuda.current_stream(wt.device).wait_event(ev)
        return ent[1]
    return None


def invalidate_packs():
    """Every weight packing made ahead of time is stale from here on: the next packed call packs inline again.

    A packing is keyed on (storage pointer, torch's version counter, PARAM_EPOCH, geometry).  Two kinds of write move neither
    counter by themselves and MUST call this: (1) replaying a HIP graph that captured the optimizer's kernels (the flat SGD kernel
    writes through raw pointers; FlatSGD.step() bumps the epoch only when it runs in Python), (2) raw `.data` writes -- `p.data.
    copy_()`, a broadcast of the module's state, an EMA swap-in.  GradBucketReducer.broadcast_module_state and bench.py's replay
    loop call it; code that writes parameters behind torch's back has to as well."""
    PARAM_EPOCH[0] += 1
    _PACK_EVENT.clear()


def after_optimizer_step(device):
    """called by FlatSGD.step() once its kernels are issued: the parameters have changed (PARAM_EPOCH), and the 3x3 weights of the
    layers the last forward ran are packed for the next step on the side stream"""
    PARAM_EPOCH[0] += 1
    if not (PREPACK and ENABLED and SIDE_WGRAD and _lib.DEVICE_ONLY and device.type == "cuda") or _capturing():
        return
    ent = _SIDE_STREAMS.get(device.index)
    if ent is None or not _PACKS:
        return
    L = _lib.lib()  # (the raw handle: a status other than COT_OK is an answer here, not an error)
    side, cur = ent[0], torch.cuda.current_stream(device)
    side.wait_stream(cur)  # behind the SGD kernels (and with them behind the whole backward pass that read the old packings)
    st = ctypes.c_void_p(side.cuda_stream)
    done = False
    for conv, e in list(_PACKS.items()):
        g = e.get("geom")
        wt = conv.weight
        if g is None or wt.device != device or wt.dtype != torch.bfloat16:
            continue
        N, C, G, H, W = g
        key = (wt.data_ptr(), wt._version, PARAM_EPOCH[0], N, C, G, H, W)
        for mode in (0, 1):
            old = e.get(mode)
            buf = old[1] if old is not None else None
            if buf is None:
                nb = int(L.cot_conv3x3g_packed_bytes(C, C, G))
                if nb <= 0:
                    break
                buf = torch.empty(nb, dtype=torch.uint8, device=device)
            if L.cot_conv3x3g_pack(_p(wt), _p(buf), mode, N, C, C, G, H, W, BF16, st) == 0:
                e[mode] = (key, buf)
                done = True
            else:
                e.pop(mode, None)  # (geometry off the LDS kernels: they gather the weights in place)
    if done:
        ev = torch.cuda.Event()
        ev.record(side)
        _PACK_EVENT[device.index] = ev


# ---- groups of 12 channels (CoXtLayer(96).key_embed: 96 channels in 8 groups, models/cotnet.py:113-117): the LDS-pipelined 3x3 kernels take
# groups from 16 channels on, the general kernel (conv_gen.hip) runs this layer at 169 us per launch at 56 x 56, B = 64.  Two neighbouring
# groups ARE one group of 24 channels with a block-diagonal weight (the off-diagonal blocks zero), which the LDS kernels take: a copy of the
# 12 x 12 x 9 blocks onto the diagonal of a persistent zero-filled [C, 24, 3, 3] buffer per step (one small launch) instead.  The weight
# gradient keeps the module's grouping (its kernel merges neighbours itself).  COT_MERGE12=0 opts out.
MERGE12 = os.environ.get("COT_MERGE12", "1") != "0"
_MERGED = weakref.WeakKeyDictionary()  # nn.Conv2d -> [key, merged weight]


def _merge12(C, G):
    return MERGE12 and G % 2 == 0 and C == 12 * G


def _merged_weight(conv, C, G, refresh, own=None):
    """own: the merged weight the forward of this backward made for itself (_conv3x3_fwd's return value), used as it is"""
    if own is not None:
        return own
    w = conv.weight
    ent = _MERGED.get(conv)
    if ent is None or ent[1].device != w.device or ent[1].dtype != w.dtype:
        ent = [None, torch.zeros((C, 24, 3, 3), dtype=w.dtype, device=w.device)]
        # (a capture records the zero fill and does not run it: a buffer first made there is this call's own -- the replay fills it --
        # and never reaches the cache, where an eager call would read its off-diagonal blocks before anything wrote them)
        if not _capturing():
            _MERGED[conv] = ent
    key = (w.data_ptr(), w._version, PARAM_EPOCH[0])
    if refresh or ent[0] != key:  # (forward: always -- a replayed graph moves the weights behind every counter; backward: the forward's copy)
        G2 = G // 2
        ent[1].view(G2, 2, 12, 2, 12, 9).diagonal(dim1=1, dim2=3).copy_(w.detach().view(G2, 2, 12, 12, 9).permute(0, 2, 3, 4, 1))
        ent[0] = key
    return ent[1]


def _conv3x3_ws_groups(C, G):
    """the group count the 3x3 forward / data gradient are launched with (workspace sizing)"""
    return G // 2 if _merge12(C, G) else G


def _conv3x3_fwd(L, conv, x, y, masks, ws, N, C, G, H, W):
    """-> None, or the merged weight this call made for itself (groups of 12 first seen inside a capture: not in _MERGED): the
    backward of this forward is handed it (`own`)"""
    if _merge12(C, G):
        wm = _merged_weight(conv, C, G, True)
        L.cot_conv3x3g_forward(_p(x), _p(wm), _p(y), _p(masks), _p(ws), N, C, C, G // 2, H, W, BF16, _stream())
        ent = _MERGED.get(conv)
        return None if (ent is not None and ent[1] is wm) else wm
    pk = _pack_for(L, conv, 0, N, C, G, H, W)
    if pk is not None:
        L.cot_conv3x3g_forward_packed(_p(x), _p(pk), _p(y), N, C, C, G, H, W, BF16, _stream())
    else:
        L.cot_conv3x3g_forward(_p(x), _p(conv.weight), _p(y), _p(masks), _p(ws), N, C, C, G, H, W, BF16, _stream())


def _conv3x3_dgrad(L, conv, gy, gx, accumulate, masks, ws, N, C, G, H, W, own=None):
    if _merge12(C, G):
        wm = _merged_weight(conv, C, G, False, own)
        L.cot_conv3x3g_backward_data(_p(gy), _p(wm), _p(gx), accumulate, _p(masks), _p(ws), N, C, C, G // 2, H, W, BF16, _stream())
        return
    pk = _pack_for(L, conv, 1, N, C, G, H, W)
    if pk is not None:
        L.cot_conv3x3g_backward_data_packed(_p(gy), _p(pk), _p(gx), accumulate, N, C, C, G, H, W, BF16, _stream())
    else:
        L.cot_conv3x3g_backward_data(_p(gy), _p(conv.weight), _p(gx), accumulate, _p(masks), _p(ws), N, C, C, G, H, W, BF16, _stream())


class _Plan:
    """per-layer handles resolved once (nn.Sequential indexing and parameter walks cost more than a kernel launch)"""
    __slots__ = ("ke0", "ke1", "em0", "em1", "em3", "gn", "cv0", "cv1", "bn", "se0", "sebn", "se3", "params",
                 "static_ok", "grouped", "bns", "lowp", "handles")

    def __init__(self, layer):
        ke, em, cv = layer.key_embed, layer.embed, layer.conv1x1
        # CoXtLayer (models/cotnet.py:106-178): the 1x1 convolutions are grouped (dw_group = 2), the key embedding has 8
        # groups, [x, k] is channel-INTERLEAVED and the two groups are folded into the batch for the aggregation
        g1 = int(getattr(layer, "dw_group", 1))
        self.grouped = g1 == 2
        self.ke0, self.ke1, self.em0, self.em1, self.em3, self.gn = ke[0], ke[1], em[0], em[1], em[3], em[4]
        se = layer.se
        self.cv0, self.cv1, self.bn, self.se0, self.sebn, self.se3 = cv[0], cv[1], layer.bn, se[0], se[1], se[3]
        # what _modes_ok asks of the modules behind `params`: the BatchNorms the launch sequence normalises with, and the modules
        # whose weight (and bias) the kernels read as bf16
        self.bns = (ke[1], em[1], cv[1], layer.bn, se[1])
        self.lowp = (ke[0], em[0], em[3], em[4], cv[0], se[0], se[3])
        self.params = [ke[0].weight, ke[1].weight, ke[1].bias, em[0].weight, em[1].weight, em[1].bias, em[3].weight,
                       em[3].bias, em[4].weight, em[4].bias, cv[0].weight, cv[1].weight, cv[1].bias, layer.bn.weight,
                       layer.bn.bias, se[0].weight, se[0].bias, se[1].weight, se[1].bias, se[3].weight, se[3].bias]
        C = layer.dim
        self.static_ok = (
            g1 in (1, 2) and C % (16 * g1 if self.grouped else 64) == 0 and layer.kernel_size == 3
            and isinstance(layer.act, nn.SiLU) and layer.radix == 2
            and _conv_ok(ke[0], 3) and ke[0].bias is None and (self.grouped or (C // ke[0].groups) % 8 == 0)
            and isinstance(ke[2], nn.ReLU) and _conv_ok(em[0], 1, g1) and em[0].bias is None
            and isinstance(em[2], nn.ReLU) and _conv_ok(em[3], 1, g1) and em[3].bias is not None
            and isinstance(em[4], nn.GroupNorm) and em[4].num_groups * 9 == em[4].num_channels and em[4].affine
            and _conv_ok(cv[0], 1, g1) and cv[0].bias is None
            and len(se) == 4 and _conv_ok(se[0], 1, 1) and se[0].bias is not None and isinstance(se[2], nn.ReLU)
            and _conv_ok(se[3], 1, 1) and se[3].bias is not None and se[0].out_channels % 8 == 0
            and se[3].out_channels == 2 * C
            and all(_bn_static_ok(b) for b in (ke[1], em[1], cv[1], layer.bn, se[1])))


def _plans_of(cls):
    """-> the accessor module -> cls(module), made on first use.  The plans are kept out of the module's __dict__: deepcopy / pickling /
    state_dict never see them, and a copied module gets a plan of its own"""
    table = weakref.WeakKeyDictionary()

    def get(mod):
        p = table.get(mod)
        if p is None:
            p = table[mod] = cls(mod)
            # what _modes_ok reads on every call, resolved once like `params` (reading a parameter off an nn.Module costs more than testing
            # it): the BatchNorms' parameters, their buffer tables (module.to() REPLACES a buffer: looked up per call), `lowp`'s parameters
            p.handles = p.static_ok and (tuple(q for bn in p.bns for q in (bn.weight, bn.bias)), tuple(bn._buffers for bn in p.bns),
                                         tuple(q for m in p.lowp for q in (m.weight, m.bias) if q is not None))
        return p
    return get


_plan = _plans_of(_Plan)


def _new_guarded(N, C, H, W, dtype, dev):
    """[N, C, H, W] tensor with W + 1 (rounded up to 8) elements of the same allocation before and behind it: the grouped 3x3
    weight gradient's LDS-staged kernel copies x at pixel + tap offset in whole 16-byte pieces
    (cot_conv3x3g_backward_weight_guarded; what lies in the margins never reaches a sum)"""
    lead = (W + 1 + 7) // 8 * 8
    n = N * C * H * W
    flat = torch.empty(n + 2 * lead, dtype=dtype, device=dev)
    return flat[lead:lead + n].view(N, C, H, W)


def _guard_elems(t):
    """elements of t's own allocation before its first and behind its last element (0 for a tensor that fills its storage)"""
    if not t.is_contiguous():
        return 0
    total = t.untyped_storage().nbytes() // t.element_size()
    return max(0, min(t.storage_offset(), total - t.storage_offset() - t.numel()))


RELU_MASK = os.environ.get("COT_BN_RELU_MASK", "1") != "0"  # bn3 + residual + ReLU: backward reads a 1-bit sign mask, not y
# identity-shortcut blocks: the residual's gradient gout * [block output > 0] is not written by bn3's backward and read back by conv1's
# data gradient (`accumulate`) but formed in that data gradient's epilogue from gout and the sign mask (cot_conv1x1_backward_data_relu_res):
# one tensor write and most of one read per block less, one backward buffer less.  Opt-in (COT_RES_FOLD=1): bit-identical results, and the
# step does not move (13.556 vs 13.552 ms, alternating; profiles/r06_res_fold_ab.log) -- bn3's backward is not where these blocks wait.
RES_FOLD = os.environ.get("COT_RES_FOLD", "0") == "1"
_RES_FOLD_OK = _lib.register_cache({})


@_lib.memo(_RES_FOLD_OK)
def _res_fold_covers(L, N, Ci, Co, HW):
    return bool(L.cot_conv1x1_backward_data_relu_res_covers(N, Ci, Co, HW, BF16))


def _res_fold_ok(L, N, Ci, Co, HW):
    return RES_FOLD and _res_fold_covers(L, N, Ci, Co, HW)


_MASK_BYTES = _lib.register_cache({})


@_lib.memo(_MASK_BYTES)
def _relu_mask_bytes(L, N, C, HW):
    return int(L.cot_bn_relu_mask_bytes(N, C, HW, BF16))


def _relu_mask(L, N, C, HW, dev):
    """uint8 tensor for the ReLU sign mask of a bn + residual + ReLU over [N, C, HW] (cot_bn_act_*_mask), or None when the
    library does not take one for this geometry (then the backward reads the saved output as before)"""
    if not RELU_MASK:
        return None
    nb = _relu_mask_bytes(L, N, C, HW)
    return torch.empty(nb, dtype=torch.uint8, device=dev) if nb > 0 else None


def _bn_fwd(L, x, y, bn, stats, nws_off, N, C, HW, act, residual=None, ps=None, mask=None):
    """stats: fp32 [2*C + workspace] -> mean = stats[:C], rstd = stats[C:2C].  ps: per-sample scale of the normalised branch
    (stochastic depth: 0 or 1 / keep, fp32 [N]) or None.  mask: `_relu_mask` tensor to fill (act = ReLU with a residual)"""
    if mask is not None:
        L.cot_bn_act_forward_mask(_p(x), _p(residual), _p(y), _p(mask), _p(bn.weight), _p(bn.bias), _p(stats), _p(stats[C:]),
                                  _p(bn.running_mean), _p(bn.running_var), _p(bn.num_batches_tracked), _p(stats[nws_off:]),
                                  _p(ps), N, C, HW, float(bn.eps), float(bn.momentum), act, BF16, _stream())
        return
    if ps is not None:
        L.cot_bn_act_forward_ps(_p(x), _p(residual), _p(y), _p(bn.weight), _p(bn.bias), _p(stats), _p(stats[C:]),
                                _p(bn.running_mean), _p(bn.running_var), _p(bn.num_batches_tracked), _p(stats[nws_off:]),
                                _p(ps), N, C, HW, float(bn.eps), float(bn.momentum), act, BF16, _stream())
        return
    L.cot_bn_act_forward(_p(x), _p(residual), _p(y), _p(bn.weight), _p(bn.bias), _p(stats), _p(stats[C:]),
                         _p(bn.running_mean), _p(bn.running_var), _p(bn.num_batches_tracked), _p(stats[nws_off:]),
                         N, C, HW, float(bn.eps), float(bn.momentum), act, BF16, _stream())


# BatchNorm statistics out of the producing 1x1 convolution's epilogue (SURVEY 7.6 / DESIGN 4.9c; opt-in COT_BN_EPILOGUE=1): on
# planes of more than 256 pixels the convolution also writes per-tile sums of what it stores, a one-wave-per-channel finalize turns
# them into mean / rstd (+ running statistics), and the flat apply kernel normalises -- the statistics pass over the tensor is gone
BN_EPILOGUE = os.environ.get("COT_BN_EPILOGUE", "0") == "1"  # measured +0.63 ms per CoTNet-50 step (profiles/r05_bn_epilogue_stats_ab.log): off
_EPI_OK = _lib.register_cache({})


@_lib.memo(_EPI_OK)
def _epi_ok(L, Ci, c1, two, HW):
    return bool(L.cot_conv1x1_stats_covers(Ci, c1, 1 if two else 0, HW))


def _conv_bn_fwd(L, x1, x2, c1, conv, y_pre, y, bn, stats, nws_off, N, Ci, Co, HW, act, residual=None, ps=None, mask=None, epi=True):
    """y_pre = conv1x1([x1 | x2]); y = act(bn(y_pre) [+ residual]) -- the models' conv -> BatchNorm pairs (models/cotnet.py:51-62,
    :228-264).  stats: fp32 [2*Co + workspace] as for _bn_fwd.  epi False: never the epilogue statistics (channel rows)"""
    st = _stream()
    bias = conv.bias
    if epi and BN_EPILOGUE and ps is None and _epi_ok(L, Ci, c1, x2 is not None, HW):
        part = torch.empty(int(L.cot_gn9_stats_floats(N, Co, HW)), dtype=torch.float32, device=y.device)
        L.cot_conv1x1_forward_stats(_p(x1), _p(x2), c1, _p(conv.weight), _p(bias), _p(y_pre), _p(part), N, Ci, Co, HW, BF16, st)
        L.cot_bn_tile_stats_finalize(_p(part), _p(stats), _p(stats[Co:]), _p(bn.running_mean), _p(bn.running_var),
                                     _p(bn.num_batches_tracked), N, Co, HW, float(bn.eps), float(bn.momentum), st)
        L.cot_bn_act_apply_forward(_p(y_pre), _p(residual), _p(y), _p(mask), _p(bn.weight), _p(bn.bias), _p(stats), _p(stats[Co:]),
                                   N, Co, HW, act, BF16, st)
        return
    L.cot_conv1x1_forward(_p(x1), _p(x2), c1, _p(conv.weight), _p(bias), _p(y_pre), N, Ci, Co, HW, BF16, st)
    _bn_fwd(L, y_pre, y, bn, stats, nws_off, N, Co, HW, act, residual=residual, ps=ps, mask=mask)


def _bn_bwd(L, dy, x, y, dx, bn, stats, N, C, HW, act, nws, dres=None, ps=None, mask=None):
    """-> (dgamma, dbeta): the parameters' slots in the flat gradient buckets when registered (grad_sink), else fresh.
    mask: the sign mask the forward wrote (then `y` is not read)"""
    dg, db = grad_sink.out_like(bn.weight), grad_sink.out_like(bn.bias)
    ws = torch.empty(max(nws, 1), dtype=torch.float32, device=dy.device)
    if mask is not None:
        L.cot_bn_act_backward_mask(_p(dy), _p(x), _p(mask), _p(dx), _p(dres), _p(bn.weight), _p(bn.bias), _p(stats),
                                   _p(stats[C:]), _p(dg), _p(db), _p(ws), _p(ps), N, C, HW, act, BF16, _stream())
        return dg, db
    if ps is not None:
        L.cot_bn_act_backward_ps(_p(dy), _p(x), _p(y), _p(dx), _p(dres), _p(bn.weight), _p(bn.bias), _p(stats),
                                 _p(stats[C:]), _p(dg), _p(db), _p(ws), _p(ps), N, C, HW, act, BF16, _stream())
        return dg, db
    L.cot_bn_act_backward(_p(dy), _p(x), _p(y), _p(dx), _p(dres), _p(bn.weight), _p(bn.bias), _p(stats), _p(stats[C:]),
                          _p(dg), _p(db), _p(ws), N, C, HW, act, BF16, _stream())
    return dg, db


# ---- per-tensor layouts (include/cotnet_amd.h, "per-tensor layouts for the deep stages"): the `lay` argument of the cot_*_lay /
# cot_radix_*_bn entry points has one bit per plane tensor, set = that tensor is channel-major.  THE place that turns "which operands
# are channel-major" into that integer: the call sites say it per operand, in the entry point's bit order --
#     cot_bn_act_forward_lay   x, residual, y, y2             cot_bn_act_backward_lay      dy, dy2, x, y, dx, dresidual
#     cot_radix_gap_t*         y (a), k                       cot_radix_mix_logits*        y (a), k, out
#     cot_radix_mix_backward_reduce*  gout, y (a), k          cot_radix_mix_backward_apply*  gout, gy (a and ga), gk
#     cot_group_norm9_forward_lay     x, y                    cot_group_norm9_backward_lay   dy, x, dx
def _lay(*cm):
    m = 0
    for i, c in enumerate(cm):
        if c:
            m |= 1 << i
    return m


def _bn_fwd_lay(L, x, res, y, y2, bn, stats, N, C, HW, act, x_cm=False, res_cm=False, y_cm=False, y2_cm=False, ps=None):
    L.cot_bn_act_forward_lay(_p(x), _p(res), _p(y), _p(y2), _p(bn.weight), _p(bn.bias), _p(stats), _p(stats[C:]),
                             _p(bn.running_mean), _p(bn.running_var), _p(bn.num_batches_tracked), _p(ps), N, C, HW,
                             float(bn.eps), float(bn.momentum), act, _lay(x_cm, res_cm, y_cm, y2_cm), BF16, _stream())


def _bn_bwd_lay(L, dy, dy2, x, y, dx, dres, bn, stats, N, C, HW, act, dy_cm=False, dy2_cm=False, x_cm=False, y_cm=False, dx_cm=False,
                dres_cm=False, ps=None):
    dg, db = grad_sink.out_like(bn.weight), grad_sink.out_like(bn.bias)
    L.cot_bn_act_backward_lay(_p(dy), _p(dy2), _p(x), _p(y), _p(dx), _p(dres), _p(bn.weight), _p(bn.bias), _p(stats), _p(stats[C:]),
                              _p(dg), _p(db), _p(ps), N, C, HW, act, _lay(dy_cm, dy2_cm, x_cm, y_cm, dx_cm, dres_cm), BF16, _stream())
    return dg, db


# ---- the backward of a convolution: its data gradient on the compute stream, its weight (+ bias) gradient queued on the node's side
# stream (_Side's rules above: what the queued launch reads is final when it is queued and is kept referenced until the join -- the
# keep-alive list is derived from the operands here, once).  The pointer arguments are evaluated when the launch is QUEUED.
def _conv1x1_wgrad(L, side, conv, gy, x1, x2, c1, N, Ci, Co, HW, groups=1, gw=None):
    """queue d conv.weight (+ d conv.bias) of y = conv1x1([x1 | x2]) (c1: channels of x1; groups > 1: cot_conv1x1g_*, one slab) ->
    (gw, gb): the parameters' slots in the flat gradient buckets (grad_sink), lent here.  gw given: written instead (no bias)"""
    gb, keep = None, ((gy, x1) if x2 is None else (gy, x1, x2))
    if gw is None:
        gw = grad_sink.out_like(conv.weight)
        if conv.bias is not None:
            gb = grad_sink.out_like(conv.bias)
    else:
        keep += (gw,)
    if groups == 1:
        fn, a = L.cot_conv1x1_backward_weight, (_p(gy), _p(x1), _p(x2), c1, _p(gw), _p(gb), _p(side.ws), N, Ci, Co, HW, BF16)
    else:
        fn, a = L.cot_conv1x1g_backward_weight, (_p(gy), _p(x1), _p(gw), _p(gb), _p(side.ws), N, Ci, Co, groups, HW, BF16)
    side.run(lambda st_: fn(*a, st_), *keep)
    return gw, gb


def _conv1x1_dgrad(L, w, gy, gx1, gx2, c1, accumulate, ws, N, Ci, Co, HW, groups=1):
    """[gx1 | gx2] (+)= d / d[x1 | x2] of y = conv1x1([x1 | x2]; w); accumulate: bit 0 adds into gx1, bit 1 into gx2"""
    if groups == 1:
        L.cot_conv1x1_backward_data(_p(gy), _p(w), _p(gx1), _p(gx2), c1, accumulate, _p(ws), N, Ci, Co, HW, BF16, _stream())
    else:
        L.cot_conv1x1g_backward_data(_p(gy), _p(w), _p(gx1), accumulate, N, Ci, Co, groups, HW, BF16, _stream())


def _conv1x1_bwd(L, side, ws, conv, gy, x1, x2, c1, gx1, gx2, accumulate, N, Ci, Co, HW, groups=1, wgrad_first=False, w=None, gw=None):
    """both gradients of y = conv1x1([x1 | x2]) -> (gw, gb) as _conv1x1_wgrad.  (N, HW) = (1, N*HW) for channel-major operands.
    wgrad_first: the weight gradient is queued before the data gradient is issued (conv1: the two overlap).  w / gw: a re-ordered
    copy of the weight and the buffer for its gradient (the two-slab form of CoXtLayer.embed[0])"""
    if wgrad_first:
        g = _conv1x1_wgrad(L, side, conv, gy, x1, x2, c1, N, Ci, Co, HW, groups, gw)
    _conv1x1_dgrad(L, conv.weight if w is None else w, gy, gx1, gx2, c1, accumulate, ws, N, Ci, Co, HW, groups)
    if not wgrad_first:
        g = _conv1x1_wgrad(L, side, conv, gy, x1, x2, c1, N, Ci, Co, HW, groups, gw)
    return g


def _conv3x3_bwd(L, side, conv, gy, x, gx, accumulate, masks, ws, N, C, G, H, W, own=None):
    """the grouped 3x3: weight gradient queued (x carries margins: _new_guarded), then gx (+)= the data gradient -> gw.
    own: _conv3x3_fwd's return value"""
    gw = grad_sink.out_like(conv.weight)
    fn, a = L.cot_conv3x3g_backward_weight_guarded, (_p(gy), _p(x), _p(gw), _p(masks), _p(side.ws), N, C, C, G, H, W, BF16, _guard_elems(x))
    side.run(lambda st_: fn(*a, st_), gy, x, masks)
    _conv3x3_dgrad(L, conv, gy, gx, accumulate, masks, ws, N, C, G, H, W, own)
    return gw


def _gn9_wgrad(L, side, gn, gn_ws, N, C):
    """GroupNorm-9's dgamma / dbeta out of the partial sums its data gradient left in gn_ws: a launch of their own, beside the weight gradients"""
    gw, gb = grad_sink.out_like(gn.weight), grad_sink.out_like(gn.bias)
    fn, a = L.cot_group_norm9_backward_params, (_p(gn_ws), _p(gw), _p(gb), N, C, BF16)
    side.run(lambda st_: fn(*a, st_), gn_ws)
    return gw, gb


# ---- what a node keeps for its backward, by name.  Tensors go through ctx.save_for_backward (autograd's version checks); which names
# were None is remembered on ctx, and the backward gets every name back.
def _pack(ctx, saved):
    ctx.saved_names = tuple(saved)
    ctx.saved_present = present = tuple(n for n in saved if saved[n] is not None)
    ctx.save_for_backward(*[saved[n] for n in present])


def _unpack(ctx):
    d = dict.fromkeys(ctx.saved_names)
    d.update(zip(ctx.saved_present, ctx.saved_tensors))
    return SimpleNamespace(**d)


# ---- stochastic depth (models/cotnet.py:256-257; models/layers/drop.py:140-168: per sample, the block's branch is dropped with
# probability p and scaled by 1 / (1 - p) otherwise) inside the single-node Bottleneck: the per-sample scale goes into the
# bn3 + residual + ReLU kernels (cot_bn_act_*_ps).  One vectorised draw per step serves every block of a model
# (prepare_drop_path, called by ResNet.forward_features): 3 small launches per step instead of 4 per block.
_DP_PLANS = weakref.WeakKeyDictionary()  # model -> (blocks with an active DropPath, their keep probabilities on the device)


def prepare_drop_path(model, x):
    if not (ENABLED and model.training):
        return
    ent = _DP_PLANS.get(model)
    if ent is None or ent[1].device != x.device:
        blocks = [m for m in model.modules() if getattr(m, "drop_path", None) is not None and getattr(m.drop_path, "drop_prob", 0.0)]
        keep = torch.tensor([1.0 - float(b.drop_path.drop_prob) for b in blocks], dtype=torch.float32, device=x.device)
        ent = _DP_PLANS[model] = (blocks, keep)
    blocks, keep = ent
    if not blocks:
        return
    u = torch.rand((len(blocks), x.shape[0]), dtype=torch.float32, device=x.device)
    ps_all = u.add_(keep[:, None]).floor_().div_(keep[:, None])  # 0 or 1 / keep  (drop.py:165-167)
    for i, b in enumerate(blocks):
        b._ps_next = ps_all[i]


def _drop_path_scale(blk, N, dev):
    """this forward's per-sample scale for `blk` (None: no stochastic depth); consumes what prepare_drop_path laid out"""
    dp = blk.drop_path
    if dp is None or not dp.drop_prob or not blk.training:
        return None
    ps = getattr(dp, "fixed_scale", None)  # (tests: a module that applies a GIVEN per-sample scale)
    if ps is not None:
        return ps.to(device=dev, dtype=torch.float32).contiguous()
    ps = getattr(blk, "_ps_next", None)
    blk._ps_next = None
    if ps is None or ps.shape[0] != N or ps.device != dev:  # (block used outside a ResNet.forward: draw its own)
        keep = 1.0 - float(dp.drop_prob)
        ps = torch.rand(N, dtype=torch.float32, device=dev).add_(keep).floor_().div_(keep)
    return ps


def _gx_slabs_ok(L, C, Ch, M):
    """CoXtLayer.embed[0] as two two-slab 1x1 convolutions (one per group) on channel-major operands.  _cm_geometry_ok's C % 64 == 0 makes
    every slab (C/2 rows of x or k, Ch/2 = C/4 output rows) 16-byte aligned with a reduction count the 1x1 kernels take; CoTNeXt's widths
    (C = 384 / 768 at 14x14 / 7x7) land on the LDS kernels, narrower ones on the first-generation kernel"""
    return GX_SLABS and C % 64 == 0 and Ch * 2 == C


# ---- the CoT layer's launch sequence, stated once for both layouts.  `cm` None: every tensor NCHW (_CotLayerNode, _BottleneckNode).
# `cm` given (_BottleneckCMNode, cot_block_cm.py): the operands of the 1x1 convolutions are dense channel-major buffers [C][N][H][W] and
# those convolutions / their BatchNorm run on channel rows -- (N, HW) = (1, N*HW) --, the operands of the plane kernels (grouped 3x3,
# aggregation) stay NCHW, and the layout changes inside the BatchNorm / GroupNorm / radix kernels between the two kinds (cot_*_lay).
# What else the channel-major policy changes: no GroupNorm fusion (planes of at most 256 pixels), the two-slab embed[0] of a CoXtLayer
# (_gx_slabs_ok), statistics buffers without a workspace where a _lay kernel writes them, the block's workspace instead of one of the
# layer's own, and no buffer reuse backward (the gradients that meet are stored differently).
def _cot_forward(L, layer, x, cm=None):
    """the layer's forward on the library kernels -> (out, {name: tensor to keep for backward}, aggregation geometry).
    x: the layer's input, NCHW (the grouped 3x3 reads it).  cm: (x's channel-major copy, the block's workspace, its 3x3 masks, BatchNorm
    workspace floats for (N, C), (1, C/2) and the se branch) -- then `out` is channel-major too"""
    N, C, H, W = x.shape
    HW, Ch, Ce = H * W, C // 2, 9 * C // 8
    dev = x.device
    pl = _plan(layer)
    A, G = pl.se0.out_channels, pl.ke0.groups
    GX = pl.grouped
    if cm is None:
        ws_bytes, nws_c, nws_h, nws_a = _sizes(L, N, C, H, W, A, G, GX)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        masks = _masks(L, H, W, dev)
        x1, n1, hw1, nws_x = x, N, HW, nws_c
    else:
        x1, ws, masks, nws_c, nws_h, nws_a = cm
        n1, hw1, nws_x = 1, N * HW, 0  # (1x1 convolutions on channel rows; the _lay BatchNorms need no workspace)
    cm = cm is not None
    st = _stream()
    new = lambda c: torch.empty((N, c, H, W), dtype=x.dtype, device=dev)  # noqa: E731
    new1 = (lambda c: torch.empty((c, N, H, W), dtype=x.dtype, device=dev)) if cm else new  # noqa: E731  (operands of the 1x1 convolutions)
    stat = lambda c, nws: torch.empty(2 * c + nws, dtype=torch.float32, device=dev)  # noqa: E731

    # static context k = relu(bn(conv3x3_grouped(x)))                                             (ref :80)
    k_pre, k = new(C), new1(C)
    wm = _conv3x3_fwd(L, pl.ke0, x, k_pre, masks, ws, N, C, G, H, W)
    s_k = stat(C, nws_x)
    if cm:
        _bn_fwd_lay(L, k_pre, None, k, None, pl.ke1, s_k, N, C, HW, 1, y_cm=True)
    else:
        _bn_fwd(L, k_pre, k, pl.ke1, s_k, 2 * C, N, C, HW, 1)
    # attention logits from [x | k]                                                             (ref :81-85)
    e0, e1 = new1(Ch), new1(Ch)
    qk = None
    s_e = stat(Ch, nws_h)
    if GX and cm and _gx_slabs_ok(L, C, Ch, hw1):
        # CoXtLayer's embed[0] reads the row-INTERLEAVED [x0, k0, x1, k1, ...] in two groups (ref :153-154): group g sees the rows
        # g*C/2 .. of x and of k.  Channel-major, each of those is one contiguous slab, so a group is the two-slab 1x1 kernel on [x_g | k_g]
        # with the group's weight columns de-interleaved to match -- a copy of the (small) weight per step instead of a copy of the
        # activations (torch.stack: 2 C*M elements written and read) and, backward, two strided adds of C*M elements each
        qk = pl.em0.weight.view(Ch, C // 2, 2).permute(0, 2, 1).reshape(Ch, C)  # [Ch][x-part C/2 | k-part C/2], a copy (kept for the backward)
        Hc, Mg = C // 2, Ch // 2
        for g_ in range(2):
            L.cot_conv1x1_forward(_p(x1[g_ * Hc:]), _p(k[g_ * Hc:]), Hc, _p(qk[g_ * Mg:]), None, _p(e0[g_ * Mg:]), 1, C, Mg, hw1, BF16, st)
        _bn_fwd(L, e0, e1, pl.em1, s_e, 2 * Ch, n1, Ch, hw1, 1)
    elif GX:  # [x0, k0, x1, k1, ...] so that each of the two groups sees matching halves of x and k (ref :153-154)
        qk = torch.stack([x1, k], dim=1).view(2 * C, N, H, W) if cm else torch.stack([x, k], dim=2).view(N, 2 * C, H, W)
        L.cot_conv1x1g_forward(_p(qk), _p(pl.em0.weight), None, _p(e0), n1, 2 * C, Ch, 2, hw1, BF16, st)
        _bn_fwd(L, e0, e1, pl.em1, s_e, 2 * Ch, n1, Ch, hw1, 1)
    else:
        _conv_bn_fwd(L, x1, k, C, pl.em0, e0, e1, pl.em1, s_e, 2 * Ch, n1, 2 * C, Ch, hw1, 1, epi=not cm)
    e3 = new1(Ce)
    gn = pl.gn
    # GroupNorm of the logits fused into its neighbours: statistics out of embed[3]'s epilogue, normalisation in the
    # aggregation's prologue -- the normalised tensor `w` is never materialised (stages with planes of more than 256 pixels)
    fused_gn = GN_FUSED and not GX and not cm and _gn_fused_ok(L, Ch, HW, W)
    if GX:
        L.cot_conv1x1g_forward(_p(e1), _p(pl.em3.weight), _p(pl.em3.bias), _p(e3), n1, Ch, Ce, 2, hw1, BF16, st)
    elif fused_gn:
        part = torch.empty(int(L.cot_gn9_stats_floats(N, Ce, HW)), dtype=torch.float32, device=dev)
        L.cot_conv1x1_forward_gn9(_p(e1), None, Ch, _p(pl.em3.weight), _p(pl.em3.bias), _p(e3), _p(part), N, Ch, Ce, HW, BF16, st)
    else:
        L.cot_conv1x1_forward(_p(e1), None, Ch, _p(pl.em3.weight), _p(pl.em3.bias), _p(e3), n1, Ch, Ce, hw1, BF16, st)
    if fused_gn or HW <= 8192:
        gn_mean = torch.empty(2 * N * gn.num_groups, dtype=torch.float32, device=dev)
        gn_rstd = gn_mean[N * gn.num_groups:]
    if fused_gn:
        w = None
        L.cot_gn9_stats_finalize(_p(part), _p(gn_mean), _p(gn_rstd), N, Ce, HW, float(gn.eps), st)
    elif cm:  # the logits channel-major in, the aggregation's weights NCHW out
        w = new(Ce)
        L.cot_group_norm9_forward_lay(_p(e3), _p(gn.weight), _p(gn.bias), _p(w), _p(gn_mean), _p(gn_rstd), N, Ce, HW, float(gn.eps),
                                      _lay(True, False), BF16, st)
    elif HW <= 8192:  # one (image, group) fits a workgroup's registers: 1 read + 1 write (csrc/group_norm9.hip)
        w = new(Ce)
        L.cot_group_norm9_forward(_p(e3), _p(gn.weight), _p(gn.bias), _p(w), _p(gn_mean), _p(gn_rstd), N, Ce, HW,
                                  float(gn.eps), BF16, st)
    else:
        w, gn_mean, gn_rstd = torch.native_group_norm(e3, gn.weight, gn.bias, N, Ce, HW, gn.num_groups, gn.eps)
    # values; channel-major: 1x1 on channel rows, its BatchNorm writes NCHW                      (ref :87)
    v_pre, v = new1(C), new(C)
    s_v = stat(C, nws_x)
    if GX:
        L.cot_conv1x1g_forward(_p(x1), _p(pl.cv0.weight), None, _p(v_pre), n1, C, C, 2, hw1, BF16, st)
    elif cm:
        L.cot_conv1x1_forward(_p(x1), None, C, _p(pl.cv0.weight), None, _p(v_pre), n1, C, C, hw1, BF16, st)
    if cm:
        _bn_fwd_lay(L, v_pre, None, v, None, pl.cv1, s_v, N, C, HW, 0, x_cm=True)
    elif GX:
        _bn_fwd(L, v_pre, v, pl.cv1, s_v, 2 * C, N, C, HW, 0)
    else:
        _conv_bn_fwd(L, x, None, C, pl.cv0, v_pre, v, pl.cv1, s_v, 2 * C, N, C, C, HW, 0)
    # local aggregation, bn + swish (NCHW)                                                       (ref :88-90)
    # (CoXtLayer folds its two groups into the batch: [N, C] -> [2N, C/2], weights [2N, 1, C/16, 9]: views of the same memory)
    geom = _lib.AggGeom(2 * N, C // 2, H, W, 1, C // 16, 3, 3, 1, 1, 1, 1, 1, 1) if GX else \
        _lib.AggGeom(N, C, H, W, 1, C // 8, 3, 3, 1, 1, 1, 1, 1, 1)
    bn_tail = BN_TAIL
    a, y = new(C), (None if bn_tail else new(C))
    s_y = stat(C, nws_c)
    bnl = pl.bn
    y_final = False
    if bn_tail:  # (aggregation + the statistics of bn; bn + swish themselves happen inside the tail's kernels)
        y_final = _agg_fwd_stats(L, v, e3 if fused_gn else w, a, gn if fused_gn else None, gn_mean, gn_rstd, geom, bnl, s_y, N, C, H, W)
    else:
        if fused_gn:
            L.cot_agg_gn9_forward(_p(v), _p(e3), _p(gn_mean), _p(gn_rstd), _p(gn.weight), _p(gn.bias), gn.num_groups, _p(a),
                                  ctypes.byref(geom), BF16, st)
        else:
            L.cot_agg_forward(_p(v), _p(w), _p(a), ctypes.byref(geom), BF16, _lib.COT_NCHW, st)
        _bn_fwd(L, a, y, bnl, s_y, 2 * C, N, C, HW, 2)
    # radix-2 split attention; channel-major: y NCHW, k channel-major, the mix written channel-major for conv3   (ref :92-104)
    # descriptors are kept channel-major ([C][N]) so that the se branch runs on the 1x1-convolution / BatchNorm
    # kernels with the batch as the pixel axis
    row = lambda c: torch.empty((c, N), dtype=x.dtype, device=dev)  # noqa: E731
    gapT, hpre, h, logitsT = row(C), row(A), row(A), row(2 * C)
    if bn_tail:
        _tail_gap(L, a, k, gapT, bnl, s_y, y_final, N, C, HW, _lay(False, cm))
    elif cm:
        L.cot_radix_gap_t_lay(_p(y), _p(k), _p(gapT), N, C, HW, _lay(False, True), BF16, st)
    else:
        L.cot_radix_gap_t(_p(y), _p(k), _p(gapT), N, C, HW, BF16, st)
    L.cot_conv1x1_forward(_p(gapT), None, C, _p(pl.se0.weight), _p(pl.se0.bias), _p(hpre), 1, C, A, N, BF16, st)
    s_a = stat(A, nws_a)
    _bn_fwd(L, hpre, h, pl.sebn, s_a, 2 * A, 1, A, N, 1)
    L.cot_conv1x1_forward(_p(h), None, A, _p(pl.se3.weight), _p(pl.se3.bias), _p(logitsT), 1, A, 2 * C, N, BF16, st)
    attn = torch.empty((N, C, 2), dtype=x.dtype, device=dev)
    out = new1(C)
    if bn_tail:
        L.cot_radix_mix_logits_bn(_p(a), _p(k), _p(logitsT), _p(out), _p(attn), _p(bnl.weight), _p(bnl.bias), _p(s_y), _p(s_y[C:]),
                                  N, C, HW, _lay(False, cm, cm), BF16, st)
    elif cm:
        L.cot_radix_mix_logits_lay(_p(y), _p(k), _p(logitsT), _p(out), _p(attn), N, C, HW, _lay(False, True, True), BF16, st)
    else:
        L.cot_radix_mix_logits(_p(y), _p(k), _p(logitsT), _p(out), _p(attn), N, C, HW, BF16, st)
    return out, dict(x=x, xc=x1 if cm else None, k_pre=k_pre, k=k, e0=e0, e1=e1, e3=e3, w=w, gn_mean=gn_mean, gn_rstd=gn_rstd,
                     v_pre=v_pre, v=v, a=a, y=y, attn=attn, s_k=s_k, s_e=s_e, s_v=s_v, s_y=s_y, gapT=gapT, hpre=hpre, h=h, s_a=s_a,
                     qk=qk, wm=wm), geom


def _cot_backward(L, layer, s, geom, gout, side=None, cm=None):
    """-> (dx of the 1x1 convolutions' input, dx of the grouped 3x3's input, gradients of _Plan.params in that order).  NCHW: the two
    are ONE tensor (summed inside the data-gradient kernels, `accumulate`); channel-major: a channel-major and an NCHW buffer, for the
    caller to merge.  s: _cot_forward's tensors by name.  `side`: the caller's side stream for the weight gradients (a Bottleneck node
    passes its own and joins it itself); None = this call opens and joins one.  cm: (the block's workspace, its 3x3 masks, BatchNorm
    workspace floats as for _cot_forward); gout is then channel-major"""
    x, k_pre, k, e0, e1, e3, v_pre, v, a, y, attn, qk = s.x, s.k_pre, s.k, s.e0, s.e1, s.e3, s.v_pre, s.v, s.a, s.y, s.attn, s.qk
    gn_mean, gn_rstd, s_y = s.gn_mean, s.gn_rstd, s.s_y
    N, C, H, W = x.shape
    HW, Ch, Ce = H * W, C // 2, 9 * C // 8
    dev = x.device
    pl = _plan(layer)
    A, G = pl.se0.out_channels, pl.ke0.groups
    GX = pl.grouped
    if cm is None:
        ws_bytes, nws_c, nws_h, nws_a = _sizes(L, N, C, H, W, A, G, GX)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        masks = _masks(L, H, W, dev)
        x1, n1, hw1 = x, N, HW
    else:
        ws, masks, nws_c, nws_h, nws_a = cm
        x1, n1, hw1 = s.xc, 1, N * HW
    cm = cm is not None
    g1 = 2 if GX else 1
    st = _stream()
    own_side = side is None
    if own_side:
        side = _Side(dev, ws_bytes, ws, pl.params)
    ke0, ke1, em0, em1, em3, cv0, cv1 = pl.ke0, pl.ke1, pl.em0, pl.em1, pl.em3, pl.cv0, pl.cv1
    gout = gout.contiguous()
    new = lambda c: torch.empty((N, c, H, W), dtype=x.dtype, device=dev)  # noqa: E731
    new1 = (lambda c: torch.empty((c, N, H, W), dtype=x.dtype, device=dev)) if cm else new  # noqa: E731

    # radix mix -> pair-softmax backward -> se branch (two 1x1 convolutions over the batch axis) -> gap
    row = lambda c: torch.empty((c, N), dtype=x.dtype, device=dev)  # noqa: E731
    glogT, gh, ggapT = row(2 * C), row(A), row(C)
    bnl = pl.bn
    if y is None:  # (the forward folded bn + swish into the tail: so does the backward)
        tsum = torch.empty(N * C * 4, dtype=torch.float32, device=dev)
        L.cot_radix_mix_backward_reduce_bn(_p(gout), _p(a), _p(k), _p(attn), _p(glogT), _p(tsum), _p(bnl.weight), _p(bnl.bias),
                                           _p(s_y), _p(s_y[C:]), N, C, HW, _lay(cm, False, cm), BF16, st)
    elif cm:
        L.cot_radix_mix_backward_reduce_lay(_p(gout), _p(y), _p(k), _p(attn), _p(glogT), N, C, HW, _lay(True, False, True), BF16, st)
    else:
        L.cot_radix_mix_backward_reduce(_p(gout), _p(y), _p(k), _p(attn), _p(glogT), N, C, HW, BF16, st)
    g_w3, g_b3 = _conv1x1_bwd(L, side, ws, pl.se3, glogT, s.h, None, A, gh, None, 0, 1, A, 2 * C, N)
    ghpre = row(A)
    d_sa_w, d_sa_b = _bn_bwd(L, gh, s.hpre, None, ghpre, pl.sebn, s.s_a, 1, A, N, 1, nws_a)
    g_w0, g_b0 = _conv1x1_bwd(L, side, ws, pl.se0, ghpre, s.gapT, None, C, ggapT, None, 0, 1, C, A, N)
    # bn + swish, aggregation (NCHW)
    ga, gk = new(C), new1(C)
    if y is None:
        d_bn_w, d_bn_b = grad_sink.out_like(bnl.weight), grad_sink.out_like(bnl.bias)
        L.cot_radix_mix_backward_apply_bn(_p(gout), _p(a), _p(attn), _p(ggapT), _p(tsum), _p(ga), _p(gk), _p(bnl.weight), _p(bnl.bias),
                                          _p(s_y), _p(s_y[C:]), _p(d_bn_w), _p(d_bn_b), N, C, HW, _lay(cm, False, cm), BF16, st)
    else:
        gy = new(C)
        if cm:
            L.cot_radix_mix_backward_apply_lay(_p(gout), _p(attn), _p(ggapT), _p(gy), _p(gk), N, C, HW, _lay(True, False, True), BF16, st)
        else:
            L.cot_radix_mix_backward_apply(_p(gout), _p(attn), _p(ggapT), _p(gy), _p(gk), N, C, HW, BF16, st)
        d_bn_w, d_bn_b = _bn_bwd(L, gy, a, None, ga, bnl, s_y, N, C, HW, 2, nws_c)
    gv, gw = new(C), new(Ce)
    gn = pl.gn
    if s.w is None:  # (the forward normalised the logits inside the aggregation: so does the backward; gw = d / d normalised weights)
        L.cot_agg_gn9_backward(_p(ga), _p(v), _p(e3), _p(gn_mean), _p(gn_rstd), _p(gn.weight), _p(gn.bias), gn.num_groups,
                               _p(gv), _p(gw), ctypes.byref(geom), BF16, st)
    else:
        L.cot_agg_backward(_p(ga), _p(v), _p(s.w), _p(gv), _p(gw), ctypes.byref(geom), BF16, _lib.COT_NCHW, st)
    # values branch: bn, conv1x1 -> first contribution to dx (channel-major: NCHW gradient in, channel-major out)
    if cm:
        gv_pre = new1(C)
        d_cv_w, d_cv_b = _bn_bwd_lay(L, gv, None, v_pre, None, gv_pre, None, cv1, s.s_v, N, C, HW, 0, x_cm=True, dx_cm=True)
    else:
        gv_pre = ga  # (reuse: ga is dead)
        d_cv_w, d_cv_b = _bn_bwd(L, gv, v_pre, None, gv_pre, cv1, s.s_v, N, C, HW, 0, nws_c)
    gx1 = new1(C)
    g_wv, _ = _conv1x1_bwd(L, side, ws, cv0, gv_pre, x1, None, C, gx1, None, 0, n1, C, C, hw1, g1)
    # logits branch: GroupNorm, conv1x1(+bias), bn+relu, conv1x1 on [x | k] -> dx +=, dk +=
    if HW <= 8192:
        ge3 = new1(Ce)
        gn_ws = torch.empty(2 * N * Ce, dtype=torch.float32, device=dev)
        # (dx here; dgamma / dbeta -- a launch of their own -- beside the weight gradients)
        if cm:  # NCHW gradient in, channel-major out
            L.cot_group_norm9_backward_lay(_p(gw), _p(e3), _p(gn_mean), _p(gn_rstd), _p(gn.weight), _p(ge3), None, None, _p(gn_ws),
                                           N, Ce, HW, _lay(False, True, True), BF16, st)
        else:
            L.cot_group_norm9_backward(_p(gw), _p(e3), _p(gn_mean), _p(gn_rstd), _p(gn.weight), _p(ge3), None, None, _p(gn_ws), N, Ce, HW,
                                       BF16, st)
        g_gn_w, g_gn_b = _gn9_wgrad(L, side, gn, gn_ws, N, Ce)
    else:
        ge3, g_gn_w, g_gn_b = torch.ops.aten.native_group_norm_backward(
            gw, e3, gn_mean, gn_rstd, gn.weight, N, Ce, HW, gn.num_groups, [True, True, True])
        ge3 = ge3.contiguous()
    ge1 = new1(Ch)
    g_we3, g_be3 = _conv1x1_bwd(L, side, ws, em3, ge3, e1, None, Ch, ge1, None, 0, n1, Ch, Ce, hw1, g1)
    ge0 = new1(Ch)
    d_em_w, d_em_b = _bn_bwd(L, ge1, e0, None, ge0, em1, s.s_e, n1, Ch, hw1, 1, nws_h)  # (ReLU mask recomputed from e0)
    if GX and qk.dim() == 2:  # (the forward took the two-slab form: qk holds the de-interleaved weight)
        Hc, Mg = C // 2, Ch // 2
        g_we0 = grad_sink.out_like(em0.weight)
        gwp = torch.empty_like(qk)  # gradient w.r.t. the de-interleaved weight, re-interleaved into the parameter's slot below
        for g_ in range(2):
            _conv1x1_bwd(L, side, ws, em0, ge0[g_ * Mg:], x1[g_ * Hc:], k[g_ * Hc:], Hc, gx1[g_ * Hc:], gk[g_ * Hc:], 3, 1, C, Mg, hw1,
                         w=qk[g_ * Mg:], gw=gwp[g_ * Mg:])

        def _interleave(st_, dst=g_we0, src=gwp, side_=side):  # [Ch][2][C/2] -> [Ch][C/2][2], behind the two launches above on their stream
            if side_.on:
                with torch.cuda.stream(side_.stream):
                    dst.view(Ch, C // 2, 2).copy_(src.view(Ch, 2, C // 2).permute(0, 2, 1))
            else:
                dst.view(Ch, C // 2, 2).copy_(src.view(Ch, 2, C // 2).permute(0, 2, 1))
        side.run(_interleave, gwp)
    elif GX:  # gradient of the interleaved [x0, k0, x1, k1, ...]: de-interleaved into dx / dk (two strided adds)
        gqk = torch.empty_like(qk)
        _conv1x1_dgrad(L, em0.weight, ge0, gqk, None, 2 * C, 0, ws, n1, 2 * C, Ch, hw1, 2)
        gq5, d = (gqk.view(C, 2, N, H, W), 1) if cm else (gqk.view(N, C, 2, H, W), 2)
        gx1.add_(gq5.select(d, 0))
        gk.add_(gq5.select(d, 1))
        g_we0, _ = _conv1x1_wgrad(L, side, em0, ge0, qk, None, 2 * C, n1, 2 * C, Ch, hw1, 2)
    else:
        g_we0, _ = _conv1x1_bwd(L, side, ws, em0, ge0, x1, k, C, gx1, gk, 3, n1, 2 * C, Ch, hw1)
    # key branch: bn+relu, grouped 3x3 -> dx += (channel-major: channel-major gradient in, NCHW out: the NCHW contribution to dx)
    if cm:
        gk_pre, gx3 = new(C), new(C)
        d_ke_w, d_ke_b = _bn_bwd_lay(L, gk, None, k_pre, None, gk_pre, None, ke1, s.s_k, N, C, HW, 1, dy_cm=True)
    else:
        gk_pre, gx3 = gv, gx1  # (reuse: gv is dead)
        d_ke_w, d_ke_b = _bn_bwd(L, gk, k_pre, None, gk_pre, ke1, s.s_k, N, C, HW, 1, nws_c)
    g_wk = _conv3x3_bwd(L, side, ke0, gk_pre, x, gx3, 0 if cm else 1, masks, ws, N, C, G, H, W, s.wm)
    if own_side:
        side.join()
    # order = _Plan.params
    return gx1, gx3, (g_wk, d_ke_w, d_ke_b, g_we0, d_em_w, d_em_b, g_we3, g_be3, g_gn_w, g_gn_b, g_wv, d_cv_w, d_cv_b,
                      d_bn_w, d_bn_b, g_w0, g_b0, d_sa_w, d_sa_b, g_w3, g_b3)


class _CotLayerNode(Function):
    @staticmethod
    @_one_stream_query
    def forward(ctx, layer, x, *params):
        # params (_Plan.params) are only here so that autograd routes their gradients; values are read off `layer`
        out, saved, geom = _cot_forward(_lib.api(), layer, x)
        ctx.layer, ctx.geom = layer, geom
        _pack(ctx, saved)
        return out

    @staticmethod
    @_one_stream_query
    def backward(ctx, gout):
        gx, _, gparams = _cot_backward(_lib.api(), ctx.layer, _unpack(ctx), ctx.geom, gout)
        return (None, gx) + gparams


def _bn_static_ok(bn):
    return (isinstance(bn, nn.BatchNorm2d) and bn.affine and bn.track_running_stats and bn.momentum is not None
            and bn.num_batches_tracked is not None)


def _conv_ok(conv, k, groups=None):
    return (isinstance(conv, nn.Conv2d) and conv.kernel_size == (k, k) and conv.stride == (1, 1)
            and conv.padding == (k // 2, k // 2) and conv.dilation == (1, 1) and (groups is None or conv.groups == groups))


# ---- eligibility: what a module and its input have to be for a node to take them, stated once for every node kind.  A predicate is
# ENABLED, the module's own mode, _input_ok, its plan's static_ok, _modes_ok, then what only that node asks (shapes; library queries last).
def _input_ok(x, cm_allowed=False):
    """the tensor every node takes: bf16 [N, C, H, W] on the device (anywhere once the tests lift DEVICE_ONLY), 16-byte aligned and
    NCHW-contiguous -- or, cm_allowed, stored channel-major (_is_cm)"""
    return ((x.is_cuda or not _lib.DEVICE_ONLY) and x.dim() == 4 and x.dtype == torch.bfloat16 and x.data_ptr() % 16 == 0
            and (x.is_contiguous() or (cm_allowed and _is_cm(x))))


def _modes_ok(plan, training):
    """(plan.static_ok holds.)  Mixed precision as cotnet_amd.flat_sgd.to_mixed_bf16 sets it up -- fp32 BatchNorm parameters and running
    statistics, everything else bf16 --, and EVERY BatchNorm of the node in the node's mode.  A training node normalises with batch
    statistics and updates the running ones, the eval node reads the running ones: a BatchNorm in the other mode (a frozen one inside a
    training block, say) would be treated as what it is not, so such a module takes the module path"""
    f32, bf16 = torch.float32, torch.bfloat16
    fp32, stats, lowp = plan.handles
    if any(bn.training != training for bn in plan.bns) or any(p.dtype != f32 for p in fp32) or any(p.dtype != bf16 for p in lowp):
        return False
    for b in stats:
        mean, var = b["running_mean"], b["running_var"]
        if mean is None or var is None or mean.dtype != f32 or var.dtype != f32:
            return False
    return True


def eligible(layer, x):
    """training-mode CotLayer / CoXtLayer of a width the kernels cover (_Plan.static_ok) on a tensor of its width"""
    if not (ENABLED and layer.training and _input_ok(x)):
        return False
    pl = _plan(layer)
    return pl.static_ok and _modes_ok(pl, True) and x.shape[1] == layer.dim


# how many times each node kind ran since the last reset (bench.py reports what actually executed, per step)
NODE_COUNTS = {"cot_layer": 0, "bottleneck": 0, "bottleneck_channel_major": 0, "split_attn_block": 0, "bottleneck_eval": 0}


def reset_node_counts():
    for k in NODE_COUNTS:
        NODE_COUNTS[k] = 0


def cot_layer_forward(layer, x):
    """layer(x) through the single-node path; caller checks `eligible` first"""
    NODE_COUNTS["cot_layer"] += 1
    return _CotLayerNode.apply(layer, x, *_plan(layer).params)


# ---- the whole Bottleneck (models/cotnet.py:228-264; models/cotnet_hybrid.py:172-202 for SE-CoTNetD's CoT blocks, the same
# sequence) as one node: conv1 -> bn1+relu [-> 3x3/2 average pooling "avd"] ->
# CotLayer -> conv3 -> bn3 + residual + relu.  The residual branch may carry the stage's 1x1 projection (`downsample` =
# [Identity,] conv1x1, BatchNorm); in a stride-2 block that projection has stride 2 = the stride-1 convolution on every
# second pixel.  dx collects the residual gradient, the projection's and conv1's data gradients inside the kernels
# (`accumulate`).
class _BlockPlan:
    __slots__ = ("conv1", "bn1", "cot", "conv3", "bn3", "ds_conv", "ds_bn", "ds_stride", "avd", "avd_post", "ds_pool2", "params",
                 "static_ok", "bns", "lowp", "handles")

    def __init__(self, blk):
        from .cotnet import CotLayer, CoXtLayer
        self.conv1, self.bn1, self.cot, self.conv3, self.bn3 = blk.conv1, blk.bn1, blk.conv2, blk.conv3, blk.bn3
        ds = blk.downsample
        self.ds_conv = self.ds_bn = None
        self.ds_stride = 1
        from .layers import BlurPool2d
        avd = blk.avd
        # cotnet_hybrid.CoTBottleneck pools AFTER the layer when avd_first is False (models/cotnet_hybrid.py:196-199): SE-CoTNetD-152's
        # BlurPool2d(filt_size 3, stride 2) behind conv2 -- `avd_post`; cotnet.Bottleneck pools in front of it (3 x 3 / 2 average) -- `avd`
        post = (avd is not None and not getattr(blk, "avd_first", True) and isinstance(avd, BlurPool2d) and avd.filt_size == 3
                and avd.stride == 2)
        self.avd_post = post
        self.avd = avd is not None and not post
        avd_ok = avd is None or post or (isinstance(avd, nn.AvgPool2d) and avd.kernel_size == 3 and avd.stride == 2
                                         and avd.padding == 1 and not avd.ceil_mode and avd.count_include_pad
                                         and avd.divisor_override is None and getattr(blk, "avd_first", True))
        ds_ok = ds is None and avd is None
        self.ds_pool2 = False
        if isinstance(ds, nn.Sequential) and (len(ds) == 2 or (len(ds) == 3 and isinstance(ds[0], (nn.Identity, nn.AvgPool2d)))):
            self.ds_conv, self.ds_bn = ds[-2], ds[-1]  # models/resnet.py:364-394: [pool,] conv, norm
            c = ds[-2]
            pool = ds[0] if len(ds) == 3 and isinstance(ds[0], nn.AvgPool2d) else None
            # `avg_down` shortcut of a stride-2 block (models/resnet.py:380-394): AvgPool2d(2, 2) in front of a stride-1 projection
            self.ds_pool2 = (pool is not None and pool.kernel_size == 2 and pool.stride == 2 and pool.padding == 0
                             and pool.divisor_override is None)  # (ceil_mode / count_include_pad: no effect on even planes, checked at run time)
            self.ds_stride = 2 if (avd is not None and pool is None) else 1
            ds_ok = (isinstance(c, nn.Conv2d) and c.kernel_size == (1, 1) and c.padding == (0, 0) and c.groups == 1
                     and c.stride == (self.ds_stride, self.ds_stride) and c.bias is None and _bn_static_ok(ds[-1])
                     and (pool is None or (self.ds_pool2 and avd is not None)))
        self.static_ok, self.params, self.bns, self.lowp = False, [], (), ()
        if not isinstance(blk.conv2, (CotLayer, CoXtLayer)):  # (SE-CoTNetD's SplitAttn blocks: cot_block_sa.py)
            return
        pl = _plan(blk.conv2)
        self.static_ok = (
            ds_ok and avd_ok and blk.drop_block is None
            and (blk.drop_path is None or hasattr(blk.drop_path, "drop_prob")) and getattr(blk, "se", None) is None
            and isinstance(blk.act1, nn.ReLU)
            and isinstance(blk.act3, nn.ReLU) and _conv_ok(blk.conv1, 1, 1) and blk.conv1.bias is None
            and _conv_ok(blk.conv3, 1, 1) and blk.conv3.bias is None and _bn_static_ok(blk.bn1)
            and _bn_static_ok(blk.bn3) and blk.conv1.in_channels % 8 == 0 and blk.conv3.out_channels % 8 == 0
            and (self.ds_conv is not None or blk.conv1.in_channels == blk.conv3.out_channels)  # (no projection: `ds_ok` says no pooling)
            and pl.static_ok)
        ds = () if self.ds_conv is None else (self.ds_conv, self.ds_bn)
        self.params = [blk.conv1.weight, blk.bn1.weight, blk.bn1.bias] + pl.params + \
            [blk.conv3.weight, blk.bn3.weight, blk.bn3.bias] + \
            ([self.ds_conv.weight, self.ds_bn.weight, self.ds_bn.bias] if ds else [])
        self.bns = (blk.bn1,) + pl.bns + (blk.bn3,) + ds[1:]
        self.lowp = (blk.conv1,) + pl.lowp + (blk.conv3,) + ds[:1]


_block_plan = _plans_of(_BlockPlan)


_BSIZES = _lib.register_cache({})


@_lib.memo(_BSIZES)
def _block_sizes(L, N, Cin, Cw, Cout, HW):
    ws = max(int(L.cot_conv1x1_workspace(N, Cin, Cw, HW, 0)), int(L.cot_conv1x1_workspace(N, Cw, Cout, HW, 0)),
             int(L.cot_conv1x1_workspace(N, Cin, Cout, HW, 0)))
    return ws, int(L.cot_bn_act_workspace(N, Cw)), int(L.cot_bn_act_workspace(N, Cout))


# ---- the pieces every block node shares: the projection shortcut (`p`: a block plan with ds_conv, ds_bn, ds_pool2, ds_stride) and conv1's backward
def _shortcut_fwd(L, p, x, N, Cin, Cout, H, W, Ho, Wo, nws_o, epi=True):
    """res = bn(conv1x1(x')), x' = x, its 2 x 2 averages (`avg_down`) or every second pixel of it (stride 2) -> (x', conv output, res, statistics)"""
    dev, st = x.device, _stream()
    if p.ds_pool2:  # `avg_down`: 2 x 2 average pooling, then the stride-1 projection
        xs = torch.empty((N, Cin, H // 2, W // 2), dtype=x.dtype, device=dev)
        L.cot_avgpool2x2s2_forward(_p(x), _p(xs), N * Cin, H, W, BF16, st)
    elif p.ds_stride == 2 and H % 2 == 0 and W % 2 == 0:  # every second pixel: one pass, 16-byte accesses (pool3x3.hip)
        xs = torch.empty((N, Cin, H // 2, W // 2), dtype=x.dtype, device=dev)
        L.cot_subsample2_forward(_p(x), _p(xs), N * Cin, H, W, BF16, st)
    else:
        xs = x[:, :, ::2, ::2].contiguous() if p.ds_stride == 2 else x
    d0, res = (torch.empty((N, Cout, Ho, Wo), dtype=x.dtype, device=dev) for _ in range(2))
    s_d = torch.empty(2 * Cout + nws_o, dtype=torch.float32, device=dev)
    _conv_bn_fwd(L, xs, None, Cin, p.ds_conv, d0, res, p.ds_bn, s_d, 2 * Cout, N, Cin, Cout, Ho * Wo, 0, epi=epi)
    return xs, d0, res, s_d


def _shortcut_bwd(L, side, ws, p, g_res, g_c3, d0, s_d, xs, x, N, Cin, Cout, H, W, HWo, nws_o):
    """BatchNorm, 1x1 convolution [, pooling / sub-sampling] backwards -> (the first contribution to dx, (d weight, d gamma, d beta))"""
    st = _stream()
    # (g_c3 is still being read by conv3's weight gradient on the side stream: no reuse of its buffer then)
    g_d0 = torch.empty_like(g_c3) if side.on else g_c3
    d_ds_w, d_ds_b = _bn_bwd(L, g_res, d0, None, g_d0, p.ds_bn, s_d, N, Cout, HWo, 0, nws_o)
    gx = torch.zeros_like(x) if (p.ds_stride == 2 and (H % 2 or W % 2)) else torch.empty_like(x)
    if p.ds_pool2 or p.ds_stride == 2:
        g_xs = torch.empty_like(xs)
        _conv1x1_dgrad(L, p.ds_conv.weight, g_d0, g_xs, None, Cin, 0, ws, N, Cin, Cout, HWo)
        if p.ds_pool2:  # the projection saw 2 x 2 averages: its data gradient is spread over the four pixels of each window
            L.cot_avgpool2x2s2_backward(_p(g_xs), _p(gx), N * Cin, H, W, BF16, st)
        elif H % 2 == 0 and W % 2 == 0:  # it saw every second pixel: values back in place and the zeros around them in one pass
            L.cot_subsample2_backward(_p(g_xs), _p(gx), N * Cin, H, W, BF16, st)
        else:
            gx[:, :, ::2, ::2] = g_xs
    else:
        _conv1x1_dgrad(L, p.ds_conv.weight, g_d0, gx, None, Cin, 0, ws, N, Cin, Cout, HWo)
    g_wd, _ = _conv1x1_wgrad(L, side, p.ds_conv, g_d0, xs, None, Cin, N, Cin, Cout, HWo)
    return gx, (g_wd, d_ds_w, d_ds_b)


def _conv1_bwd(L, side, ws, conv, g_c1, x, gx, gout, m3, N, Cin, Cw, HW):
    """conv1's backward, the weight gradient queued before the data gradient is issued (the two overlap).  gx += the data gradient; gx
    None (identity shortcut, COT_RES_FOLD): the residual's gradient gout * [block output > 0] was never written and is formed in the
    data gradient's epilogue from gout and bn3's sign mask m3.  -> (dx, d weight)"""
    g_w1, _ = _conv1x1_wgrad(L, side, conv, g_c1, x, None, Cin, N, Cin, Cw, HW)
    if gx is None:
        gx = torch.empty_like(x)
        L.cot_conv1x1_backward_data_relu_res(_p(g_c1), _p(conv.weight), _p(gx), _p(gout), _p(m3), N, Cin, Cw, HW, BF16, _stream())
    else:
        _conv1x1_dgrad(L, conv.weight, g_c1, gx, None, Cin, 1, ws, N, Cin, Cw, HW)
    return gx, g_w1


class _BottleneckNode(Function):
    @staticmethod
    @_one_stream_query
    def forward(ctx, blk, x, *params):
        L = _lib.api()
        bp = _block_plan(blk)
        N, Cin, H, W = x.shape
        Cw, Cout = bp.conv1.out_channels, bp.conv3.out_channels
        Ho, Wo = ((H - 1) // 2 + 1, (W - 1) // 2 + 1) if (bp.avd or bp.avd_post) else (H, W)  # 3x3/2 pooling, padding 1 / BlurPool
        HW, HWo = H * W, Ho * Wo
        dev, st = x.device, _stream()
        _, nws_w, _ = _block_sizes(L, N, Cin, Cw, Cout, HW)
        _, _, nws_o = _block_sizes(L, N, Cin, Cw, Cout, HWo)
        new = lambda c, h, w: torch.empty((N, c, h, w), dtype=x.dtype, device=dev)  # noqa: E731
        stat = lambda c, nws: torch.empty(2 * c + nws, dtype=torch.float32, device=dev)  # noqa: E731
        # (the CoT layer's input -- a1, or its pooled version -- is what the grouped 3x3 weight gradient reads shifted: margins)
        c1, a1 = new(Cw, H, W), (new(Cw, H, W) if bp.avd else _new_guarded(N, Cw, H, W, x.dtype, dev))
        s_1 = stat(Cw, nws_w)
        _conv_bn_fwd(L, x, None, Cin, bp.conv1, c1, a1, bp.bn1, s_1, 2 * Cw, N, Cin, Cw, HW, 1)
        if bp.avd:
            p1 = _new_guarded(N, Cw, Ho, Wo, x.dtype, dev)
            L.cot_avgpool3x3s2_forward(_p(a1), _p(p1), N * Cw, H, W, BF16, st)
        else:
            p1 = a1
        cot_out, saved, geom = _cot_forward(L, bp.cot, p1)
        if bp.avd_post:  # anti-aliased down-sampling behind the layer (cotnet_hybrid.py:196-199; blur_pool.py:53-58)
            cot_full = cot_out
            cot_out = new(Cw, Ho, Wo)
            L.cot_blurpool3x3s2_forward(_p(cot_full), _p(cot_out), N * Cw, H, W, BF16, st)
        c3, y = new(Cout, Ho, Wo), new(Cout, Ho, Wo)
        if bp.ds_conv is not None:  # projection shortcut: bn(conv1x1(x)), on every second pixel in a stride-2 block
            xs, d0, res, s_d = _shortcut_fwd(L, bp, x, N, Cin, Cout, H, W, Ho, Wo, nws_o)
        else:
            xs, d0, res, s_d = None, None, x, None
        s_3 = stat(Cout, nws_o)
        ps = _drop_path_scale(blk, N, dev)  # stochastic depth: per-sample 0 or 1 / keep on the normalised branch
        m3 = _relu_mask(L, N, Cout, HWo, dev)
        _conv_bn_fwd(L, cot_out, None, Cw, bp.conv3, c3, y, bp.bn3, s_3, 2 * Cout, N, Cw, Cout, HWo, 1, residual=res, ps=ps, mask=m3)
        ctx.blk, ctx.geom = blk, geom
        _pack(ctx, dict(saved, x_in=x, c1=c1, a1=a1, s_1=s_1, cot_out=cot_out, c3=c3, y_out=y, s_3=s_3, d0=d0, s_d=s_d, xs=xs, m3=m3, ps=ps))
        return y

    @staticmethod
    @_one_stream_query
    def backward(ctx, gout):
        L = _lib.api()
        blk = ctx.blk
        bp = _block_plan(blk)
        s = _unpack(ctx)
        x, c1, a1, cot_out, c3, y, m3 = s.x_in, s.c1, s.a1, s.cot_out, s.c3, s.y_out, s.m3
        N, Cin, H, W = x.shape
        Cw, Cout = bp.conv1.out_channels, bp.conv3.out_channels
        Ho, Wo = y.shape[2], y.shape[3]
        HW, HWo = H * W, Ho * Wo
        dev, st = x.device, _stream()
        ws_a, nws_w, _ = _block_sizes(L, N, Cin, Cw, Cout, HW)
        ws_b, _, nws_o = _block_sizes(L, N, Cin, Cw, Cout, HWo)
        ws = torch.empty(max(ws_a, ws_b), dtype=torch.uint8, device=dev)
        cN, cC, cH, cW = s.x.shape
        cpl = _plan(bp.cot)
        side = _Side(dev, max(ws_a, ws_b, _sizes(L, cN, cC, cH, cW, cpl.se0.out_channels, cpl.ke0.groups, cpl.grouped)[0]), ws,
                     bp.params)
        gout = gout.contiguous()
        # bn3 + residual + relu: dx of the normalisation and the residual's gradient in one pass
        # identity shortcut with a sign mask: the residual's gradient is folded into conv1's data gradient below, never written
        fold = s.d0 is None and m3 is not None and not bp.avd and _res_fold_ok(L, N, Cin, Cw, HW)
        g_c3, g_res = torch.empty_like(c3), (None if fold else torch.empty_like(c3))
        d_bn3_w, d_bn3_b = _bn_bwd(L, gout, c3, y, g_c3, bp.bn3, s.s_3, N, Cout, HWo, 1, nws_o, dres=g_res, ps=s.ps, mask=m3)
        g_cot_out = torch.empty_like(cot_out)
        g_w3, _ = _conv1x1_bwd(L, side, ws, bp.conv3, g_c3, cot_out, None, Cw, g_cot_out, None, 0, N, Cw, Cout, HWo)
        if bp.avd_post:  # (cot_out at the output resolution was the pooled tensor: its gradient goes back through the blur)
            g_full = torch.empty((N, Cw, H, W), dtype=x.dtype, device=dev)
            L.cot_blurpool3x3s2_backward(_p(g_cot_out), _p(g_full), N * Cw, H, W, BF16, st)
            g_layer_out = g_full
        else:
            g_layer_out = g_cot_out
        g_p1, _, g_cot = _cot_backward(L, bp.cot, s, ctx.geom, g_layer_out, side)
        if bp.avd:
            g_a1 = torch.empty_like(a1)
            L.cot_avgpool3x3s2_backward(_p(g_p1), _p(g_a1), N * Cw, H, W, BF16, st)
            g_c1 = torch.empty_like(c1)
        else:
            g_a1 = g_p1
            g_c1 = g_layer_out  # (reuse: consumed by the layer's backward)
        d_bn1_w, d_bn1_b = _bn_bwd(L, g_a1, c1, None, g_c1, bp.bn1, s.s_1, N, Cw, HW, 1, nws_w)
        if s.d0 is not None:
            gx, g_ds = _shortcut_bwd(L, side, ws, bp, g_res, g_c3, s.d0, s.s_d, s.xs, x, N, Cin, Cout, H, W, HWo, nws_o)
        else:
            gx, g_ds = g_res, ()  # identity shortcut: the residual's gradient is the first contribution to dx (None: folded)
        gx, g_w1 = _conv1_bwd(L, side, ws, bp.conv1, g_c1, x, gx, gout, m3, N, Cin, Cw, HW)
        side.join()
        return (None, gx, g_w1, d_bn1_w, d_bn1_b) + g_cot + (g_w3, d_bn3_w, d_bn3_b) + g_ds


def block_eligible(blk, x):
    """training-mode cotnet.Bottleneck / cotnet_hybrid.CoTBottleneck around a CotLayer or CoXtLayer, every form _BlockPlan.static_ok
    admits: identity or projection shortcut (stride 2 or `avg_down`), average pooling in front of the layer or BlurPool behind it,
    stochastic depth"""
    if not (ENABLED and blk.training and _input_ok(x)):
        return False
    bp = _block_plan(blk)
    return (bp.static_ok and _modes_ok(bp, True) and x.shape[1] == bp.conv1.in_channels
            and not (bp.ds_pool2 and (x.shape[2] % 2 or x.shape[3] % 2)))  # (cot_avgpool2x2s2_*: even planes)


def block_forward(blk, x):
    NODE_COUNTS["bottleneck"] += 1
    return _BottleneckNode.apply(blk, x, *_block_plan(blk).params)


def dispatch(blk, x):
    """-> blk(x) by the first node kind that takes it, or None: the caller runs the module path.  A block class states the kinds it
    tries, in order, as `node_kinds` (cotnet.Bottleneck, cotnet_hybrid.CoTBottleneck); a kind is the NAME of this module's
    NAME_eligible / NAME_forward pair, looked up per call (tests rebind them)"""
    if ENABLED:
        g = globals()
        for kind in blk.node_kinds:
            if g[kind + "_eligible"](blk, x):
                return g[kind + "_forward"](blk, x)
    return None


# ---- the other node kinds live in their own modules (round 6 split): SplitAttn blocks, channel-major Bottlenecks, the
# eval-mode call sequence.  They import this module's helpers, so they are imported HERE, at its end, and re-exported under the names
# the wrappers, bench.py and the tests have always used.  The channel-major switches are attributes of THIS module (tests rebind them).
CM_LAYOUT = os.environ.get("COT_CM_LAYOUT", "1") != "0"
CM_OPENING = os.environ.get("COT_CM_OPENING", "1") != "0"  # the stage's stride-2 opening block on the channel-major node too (A/B switch)
GX_SLABS = os.environ.get("COT_GX_SLABS", "1") != "0"  # CoXtLayer.embed[0] in channel-major blocks: two-slab kernels per group instead of torch.stack (_cot_forward)
from .cot_block_sa import (_SABlockPlan, _SASIZES, _sa_plan, _sa_sizes, _SplitAttnBlockNode, sa_block_eligible,  # noqa: E402,F401
                           sa_block_forward)
from .cot_block_cm import (_CM_OK, _CM_SIZES, _BottleneckCMNode, _cm_buf, _cm_geometry_ok, _cm_sizes, _cm_static_ok, _cm_view,  # noqa: E402,F401
                           _is_cm, cm_block_eligible, cm_block_forward, plan_stage_layouts)
from .cot_block_eval import _bn_inf, eval_block_eligible, eval_block_forward  # noqa: E402,F401
