"""The call trace of the single-node paths: which C ABI entry points a node calls, in which order, with which arguments.

The host side of the training step (cot_layer_fused.py, cot_block_cm.py, cot_block_sa.py) is a long sequence of launches whose
correctness rests on details no numerical test isolates: which buffer a gradient is accumulated into, which one is reused, which
launches go to the weight-gradient side stream.  So the sequence is pinned: every node kind runs forward + backward on CPU tensors
against the REAL library in dry-run mode (cot_set_tuning(COT_TUNE_DRY_RUN, 1): no launch, no HIP call -- as tests/test_dispatch_table.py does; the
outputs are uninitialised memory, which the sequence does not depend on), a recorder in front of the library handle notes every call,
and the result is compared with tests/golden/node_call_trace.json: per case the number of calls and the SHA-256 of its lines, and for
one case of each node kind (FULL) the lines themselves, to be read.  `python tests/test_node_call_trace.py CASE` prints a trace; when a
digest differs, print the case at both commits and diff the two.  One line per call:

    entry(arg, arg, ...)      integers and floats as they are; a pointer as `-` (NULL) or `@i`, i = the index of the earliest call of
                              the trace that saw the same address (the call's own index: a buffer the library has not seen before), so
                              aliasing and buffer reuse are pinned without pinning addresses; a `cot_agg_geom` as {its fields}; the
                              stream as `c` (compute) or `s` (the weight-gradient side stream)

Two things besides the library handle are replaced while a case runs, both so that a CPU run says what a GPU run would do: `_Side` by
a subclass that is switched on without a device (its own workspace, a stream handle of its own, stream waits that do nothing) -- the
queueing, the keep-alive lists and the join logic are the real ones --, and `_lib.ptr` by one that also keeps every tensor it is asked
about alive until the case ends, so that an address can only re-appear because the node passes the same buffer again, never because
the allocator handed a freed block out a second time.

A deliberate change of the sequence = regenerate the fixture and read the diff:

    python tests/test_node_call_trace.py --write
"""
import ctypes
import hashlib
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "node_call_trace.json")
SIDE_HANDLE = 0x51DE0  # the side stream's handle: never dereferenced in dry-run mode


class _Recorder:
    """a library handle that notes every SYMBOLS call and passes it on"""

    def __init__(self, raw, symbols):
        self._raw, self._symbols = raw, symbols
        self.calls, self._seen = [], {}

    def __getattr__(self, name):
        fn = getattr(self._raw, name)
        sym = self._symbols.get(name)
        if sym is None:
            return fn
        argtypes = sym[1]

        def call(*args):
            assert len(args) == len(argtypes), (name, len(args), len(argtypes))
            idx, out = len(self.calls), []
            for i, (a, t) in enumerate(zip(args, argtypes)):
                if t is ctypes.c_void_p:
                    v = a.value if isinstance(a, ctypes.c_void_p) else a
                    if i == len(args) - 1 and name != "cot_profile_end":  # the stream
                        out.append("s" if v == SIDE_HANDLE else "c")
                        assert v in (None, 0, SIDE_HANDLE), (name, v)
                    elif not v:
                        out.append("-")
                    else:
                        out.append("@%d" % self._seen.setdefault(int(v), idx))
                elif isinstance(t, type) and issubclass(t, ctypes._Pointer):
                    g = a._obj
                    out.append("{" + " ".join(str(getattr(g, f)) for f, _ in g._fields_) + "}")
                elif t is ctypes.c_float:
                    out.append(repr(float(a)))
                elif t is ctypes.c_char_p:
                    out.append("buf")
                else:
                    out.append(str(int(a)))
            self.calls.append("%s(%s)" % (name, ",".join(out)))
            return fn(*args)
        return call


class _NoStream:
    def wait_stream(self, other):
        pass


def _install(mp, rec):
    """the recorder as THE library; _Side switched on without a device; ptr() keeping what it sees alive.  -> the keep-alive list"""
    from cotnet_amd import _lib, cot_layer_fused as clf
    real_side, real_ptr, pinned = clf._Side, _lib.ptr, []

    class _TraceSide(real_side):
        __slots__ = ()

        def __init__(self, dev, ws_bytes, main_ws, params=()):
            from cotnet_amd import grad_sink
            self.on, self.lazy = True, bool(clf.LAZY_WGRAD)
            self.keep, self.queue, self.dev = [], [], dev
            self.fresh0, self.params = grad_sink.fresh_count(), params
            self.main = self.stream = _NoStream()
            self.ws = torch.empty(max(int(ws_bytes), 16), dtype=torch.uint8)
            self.st = ctypes.c_void_p(SIDE_HANDLE)
            clf._SIDE_PENDING.setdefault(dev.index, {"keep": []})

    def ptr(t):
        if t is None:
            return None
        pinned.append(t)
        return t.data_ptr()

    mp.setattr(_lib, "lib", lambda: rec)
    mp.setattr(_lib, "DEVICE_ONLY", False)
    for name, mod in list(sys.modules.items()):
        if mod is None or not name.startswith("cotnet_amd"):
            continue
        for attr, val in list(vars(mod).items()):
            if val is real_side:
                mp.setattr(mod, attr, _TraceSide)
            elif val is real_ptr:
                mp.setattr(mod, attr, ptr)
    return pinned


def _tune(m):
    from cotnet_amd.flat_sgd import to_mixed_bf16
    return to_mixed_bf16(m.train())


class _FixedDropPath(torch.nn.Module):
    """stochastic depth with a GIVEN per-sample scale (cot_layer_fused._drop_path_scale reads `fixed_scale`)"""

    def __init__(self, scale, p):
        super().__init__()
        self.drop_prob = p
        self.register_buffer("fixed_scale", scale)

    def forward(self, x):
        return x * self.fixed_scale.view(-1, 1, 1, 1).to(x.dtype) if self.training else x


def _drop(n):
    return _FixedDropPath(torch.tensor([0.0 if i % 3 == 1 else 1.25 for i in range(n)]), 0.2)


def _x(*shape):
    return torch.zeros(shape, dtype=torch.bfloat16)


# ---- the cases: name -> function(clf) that runs forward + backward of one node (or of a short run of them); true stage geometries of
# CoTNet-50 / CoTNeXt-50 / SE-CoTNetD at a small batch
def _layer(cls, C, N, H):
    def run(clf):
        from cotnet_amd import cotnet
        layer = _tune(getattr(cotnet, cls)(C, 3))
        x = _x(N, C, H, H).requires_grad_(True)
        assert clf.eligible(layer, x)
        y = clf.cot_layer_forward(layer, x)
        assert y.grad_fn.name().startswith("_CotLayerNode")
        y.backward(_x(*y.shape))
    return run


def _bottleneck(inpl, planes, N, H, stride=1, project=False, drop=False, coxt=False):
    def run(clf):
        from cotnet_amd.cotnet import Bottleneck
        from cotnet_amd.resnet import downsample_conv
        ds = downsample_conv(inpl, planes * 4, 1, stride=stride) if (project or stride == 2) else None
        blk = Bottleneck(inpl, planes, stride=stride, downsample=ds, drop_path=_drop(N) if drop else None,
                         **(dict(cardinality=2, base_width=48) if coxt else {}))
        blk = _tune(blk)
        x = _x(N, inpl, H, H).requires_grad_(True)
        assert clf.block_eligible(blk, x)
        y = clf.block_forward(blk, x)
        assert y.grad_fn.name().startswith("_BottleneckNode")
        y.backward(_x(*y.shape))
    return run


def _hybrid(kind, N, H, opening):
    """SE-CoTNetD's blocks (cotnet_hybrid.CoTBottleneck): the SplitAttn kind, and the CoT kind with BlurPool behind the layer and the
    `avg_down` shortcut"""
    def run(clf):
        from cotnet_amd.cotnet_hybrid import CoTBottleneck
        from cotnet_amd.layers import BlurPool2d, get_act_layer
        from cotnet_amd.resnet import downsample_avg
        conv_dim = {64} if kind == "split_attn" else set()
        if opening:
            blk = CoTBottleneck(0, 128, 64, stride=2, downsample=downsample_avg(128, 256, 1, stride=2), aa_layer=BlurPool2d, radix=1,
                                avd=True, avd_first=False, conv_dim=conv_dim, c4_dim=-1, c4_idx=set(), act_layer=get_act_layer("swish"))
            inpl = 128
        else:
            blk = CoTBottleneck(1, 256, 64, conv_dim=conv_dim, c4_dim=256, c4_idx=set(), radix=1, act_layer=get_act_layer("swish"))
            inpl = 256
        blk = _tune(blk)
        x = _x(N, inpl, H, H).requires_grad_(True)
        if kind == "split_attn":
            assert clf.sa_block_eligible(blk, x)
            y = clf.sa_block_forward(blk, x)
            assert y.grad_fn.name().startswith("_SplitAttnBlockNode")
        else:
            assert clf.block_eligible(blk, x)
            y = clf.block_forward(blk, x)
            assert y.grad_fn.name().startswith("_BottleneckNode")
        y.backward(_x(*y.shape))
    return run


def _cm_stage(planes, N, H, blocks, opening=False, drop=False, coxt=False, gout_cm=True):
    """a run of channel-major blocks: the first takes NCHW, the last writes NCHW, the ones between are channel-major on both sides
    (blocks = 1: NCHW in and out); opening: the stage's stride-2 block in front.  gout_cm False: the middle gradient arrives NCHW"""
    def run(clf):
        from torch import nn
        from cotnet_amd.cotnet import Bottleneck
        from cotnet_amd.resnet import downsample_conv
        kw = dict(cardinality=2, base_width=48) if coxt else {}
        out = planes * 4
        stage = [Bottleneck(out, planes, drop_path=_drop(N) if drop else None, **kw) for _ in range(blocks)]
        if opening:
            stage.insert(0, Bottleneck(out // 2, planes, stride=2, downsample=downsample_conv(out // 2, out, 1, stride=2),
                                       drop_path=_drop(N) if drop else None, **kw))
        stage = _tune(nn.Sequential(*stage))
        clf.plan_stage_layouts(stage)
        assert [b._next_cm for b in stage] == [True] * (len(stage) - 1) + [False]
        h = _x(N, out // 2 if opening else out, 2 * H if opening else H, 2 * H if opening else H).requires_grad_(True)
        for i, b in enumerate(stage):
            assert clf.cm_block_eligible(b, h)
            h = clf.cm_block_forward(b, h)
            assert h.grad_fn.name().startswith("_BottleneckCMNode") and clf._is_cm(h) == (i + 1 < len(stage))
            if not gout_cm and i + 1 < len(stage):
                h = h + 0  # (an op between the blocks: its gradient reaches the node NCHW-contiguous)
                assert clf._is_cm(h)
        h.backward(_x(*h.shape))
    return run


COT_CASES = {
    "layer CotLayer(64) 56x56": _layer("CotLayer", 64, 2, 56),
    "layer CotLayer(256) 14x14": _layer("CotLayer", 256, 2, 14),
    "layer CoXtLayer(96) 56x56": _layer("CoXtLayer", 96, 2, 56),
    "bottleneck identity 256/64 56x56": _bottleneck(256, 64, 2, 56),
    "bottleneck identity 1024/256 14x14": _bottleneck(1024, 256, 2, 14),
    "bottleneck projection 64/64 56x56": _bottleneck(64, 64, 2, 56, project=True),
    "bottleneck stride-2 avd 256/128 56x56": _bottleneck(256, 128, 2, 56, stride=2),
    "bottleneck drop-path 512/128 28x28": _bottleneck(512, 128, 3, 28, drop=True),
    "bottleneck CoXt identity 256/64 56x56": _bottleneck(256, 64, 2, 56, coxt=True),
    "bottleneck CoXt stride-2 256/128 56x56": _bottleneck(256, 128, 2, 56, stride=2, coxt=True),
    "bottleneck hybrid opening (blur, avg_down) 128/64 40x40": _hybrid("cot", 2, 40, True),
    "cm NCHW in, NCHW out 1024/256 14x14": _cm_stage(256, 4, 14, 1),
    "cm stage of 3 1024/256 14x14": _cm_stage(256, 4, 14, 3),
    "cm stage of 2, NCHW gradient between 1024/256 14x14": _cm_stage(256, 4, 14, 2, gout_cm=False),
    "cm stage of 2 2048/512 7x7": _cm_stage(512, 8, 7, 2),
    "cm opening + identity 512->1024/256 28x28": _cm_stage(256, 4, 14, 1, opening=True),
    "cm opening alone 1024->2048/512 14x14": _cm_stage(512, 8, 7, 0, opening=True),
    "cm stage of 3 with drop-path 1024/256 14x14": _cm_stage(256, 6, 14, 3, drop=True),
    "cm opening + identity with drop-path 512->1024/256 28x28": _cm_stage(256, 4, 14, 1, opening=True, drop=True),
    "cm CoXt stage of 2 1024/256 14x14": _cm_stage(256, 4, 14, 2, coxt=True),
    "cm CoXt opening + identity 1024->2048/512 14x14": _cm_stage(512, 8, 7, 1, opening=True, coxt=True),
}
SA_CASES = {
    "split-attn identity 256/64 56x56": _hybrid("split_attn", 2, 56, False),
    "split-attn opening 128/64 40x40": _hybrid("split_attn", 2, 40, True),
}
# switch -> value: every CoT case runs once more with each (the side stream is always on in a trace; COT_WGRAD_LAZY = 0 issues each
# weight gradient where it is queued)
SWITCHES = [("BN_TAIL", False), ("GN_FUSED", False), ("RES_FOLD", True), ("AGG_ROWSTATS", True), ("BN_EPILOGUE", True),
            ("LAZY_WGRAD", False)]
# ... and the cases that a switch of their own changes (COT_GX_SLABS, COT_MERGE12)
EXTRA = [("GX_SLABS", False, "cm CoXt stage of 2 1024/256 14x14"), ("GX_SLABS", False, "cm CoXt opening + identity 1024->2048/512 14x14"),
         ("MERGE12", False, "layer CoXtLayer(96) 56x56"), ("MERGE12", False, "bottleneck CoXt identity 256/64 56x56")]


def _variants():
    for name in list(COT_CASES) + list(SA_CASES):
        yield name, None, None
    for sw, val in SWITCHES:
        for name in COT_CASES:
            yield name, sw, val
    for sw, val, name in EXTRA:
        yield name, sw, val


def _key(name, sw, val):
    return name if sw is None else "%s | %s=%d" % (name, sw, int(val))


def trace(name, sw=None, val=None):
    """-> the list of call lines of one case"""
    from cotnet_amd import _lib, cot_layer_fused as clf
    raw = _lib.lib()
    rec = _Recorder(raw, _lib.SYMBOLS)
    caches = [getattr(clf, n) for n in ("_SIZES", "_MASKS", "_BSIZES", "_CM_SIZES", "_CM_OK", "_SASIZES", "_RES_FOLD_OK", "_GN_OK",
                                        "_ROWSTATS_OK", "_EPI_OK", "_MASK_BYTES")]
    mp = pytest.MonkeyPatch()
    with _lib.tuned(raw, DRY_RUN=1):  # (also empties every registered shape cache)
        try:
            for c in caches:
                c.clear()
            pinned = _install(mp, rec)
            mp.setattr(clf, "ENABLED", True)
            for s, v in (("SIDE_WGRAD", True), ("LAZY_WGRAD", True), ("BN_TAIL", True), ("GN_FUSED", True), ("RES_FOLD", False),
                         ("AGG_ROWSTATS", False), ("BN_EPILOGUE", False), ("RELU_MASK", True), ("CM_LAYOUT", True), ("CM_OPENING", True),
                         ("GX_SLABS", True), ("MERGE12", True), ("PREPACK", True)):
                mp.setattr(clf, s, v)
            if sw is not None:
                mp.setattr(clf, sw, val)
            torch.manual_seed(0)
            (COT_CASES.get(name) or SA_CASES[name])(clf)
            assert pinned
        finally:
            mp.undo()
            clf._SIDE_PENDING.pop(None, None)
            for c in caches:
                c.clear()
    return rec.calls


# the cases whose lines the fixture holds in full, one of each node kind
FULL = ("layer CotLayer(256) 14x14", "bottleneck identity 1024/256 14x14", "cm NCHW in, NCHW out 1024/256 14x14",
        "split-attn identity 256/64 56x56")


def _digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def _have_lib():
    from cotnet_amd import _lib
    return os.path.exists(_lib.LIB_PATH)


@pytest.mark.skipif(not _have_lib(), reason="libcotnet_hip.so not built")
@pytest.mark.parametrize("name,sw,val", list(_variants()), ids=[_key(*v) for v in _variants()])
def test_node_call_trace_is_the_pinned_one(name, sw, val):
    fx = json.load(open(FIXTURE))
    key = _key(name, sw, val)
    got = trace(name, sw, val)
    want = fx["lines"].get(key)
    if want is not None:
        first = next((i for i, (a, b) in enumerate(zip(want, got)) if a != b), min(len(want), len(got)))
        assert got == want, "call %d of %d (pinned %d) differs:\n  pinned: %s\n  now:    %s" % (
            first, len(got), len(want), want[first] if first < len(want) else None, got[first] if first < len(got) else None)
    n, sha = fx["cases"][key]
    assert (len(got), _digest(got)) == (n, sha), "%d calls (pinned %d) or their arguments differ: print the case with `python " \
        "tests/test_node_call_trace.py %r` here and at the commit the fixture was written at and diff; regenerate with --write only " \
        "after reading that diff" % (len(got), n, key)


def test_fixture_holds_exactly_the_cases():
    fx = json.load(open(FIXTURE))
    assert sorted(fx["cases"]) == sorted(_key(*v) for v in _variants()) and sorted(fx["lines"]) == sorted(FULL)


def write_fixture(traces):
    """traces: {case key: lines}"""
    with open(FIXTURE, "w") as f:
        f.write('{"cases": {\n' + ",\n".join("%s: %s" % (json.dumps(k), json.dumps([len(v), _digest(v)])) for k, v in sorted(traces.items())))
        f.write('\n},\n"lines": {\n' + ",\n".join("%s: [\n%s\n]" % (json.dumps(k), ",\n".join(json.dumps(ln) for ln in traces[k])) for k in FULL))
        f.write("\n}}\n")


if __name__ == "__main__":
    if "--write" in sys.argv:
        traces = {_key(*v): trace(*v) for v in _variants()}
        write_fixture(traces)
        print("wrote %d cases, %d calls to %s" % (len(traces), sum(map(len, traces.values())), FIXTURE))
    else:
        arg = sys.argv[1] if len(sys.argv) > 1 else "bottleneck identity 256/64 56x56"
        name, _, sw = arg.partition(" | ")
        for ln in trace(name, *((sw.split("=")[0], bool(int(sw.split("=")[1]))) if sw else ())):
            print(ln)
