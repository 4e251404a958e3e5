"""Memory footprint and placement independence of the kernel entry points (include/cotnet_amd.h), shared by the host-emulated run
(tests/test_footprint_emulated.py) and the device run (tests/test_footprint_gpu.py).

Every case is a function `case(L, A, ...)` that builds its operands through an arena `A` and calls the library through a recording proxy
`L`.  run_case() runs it twice with the same values: on PLAIN operands (one fresh allocation each -- what the rest of the suite pins to
torch, the C oracle and the reference fixtures) and on MARGINED ones, each in an allocation of its own with a filled margin on both
sides, at an operand base = 0 or = 16 (mod 256 bytes).  Arena.check() then asserts that

  1. every margin of every operand still holds its fill, bit for bit (nothing was written outside a tensor: inputs, workspaces too),
  2. no `out` element still holds its fill and no `out` / `inout` element is NaN (every promised element was written, and no margin
     value was read and used: a NaN that enters an accumulation poisons the result),
  3. every `in` body is unchanged, bit for bit,
  4. outputs are bit-equal to the plain call's, the launches having gone to the same kernels (cot_last_kernel()).

The margins are at least 64 planes + one row + one element of the operand (and never under 2048 elements) wide -- one channel tile
past either end -- so that a plausible overrun lands in memory the test owns and is detected, not faulted on.

Fills.  `in`: NaN margins (integer inputs: byte 0xA5);  `out`: NaN everywhere (integer / byte / mask outputs: 0xA5);  `inout`: NaN
margins around finite values;  `ws`: every byte 0x7f (no kernel may count on a zeroed workspace).  One-byte outputs (sign masks, arg-max
taps) can legitimately hold the value 0xA5, so their "still holds its fill" check is made through (4): the plain run fills them with
0x5A, and a byte neither run wrote differs between the two.

BY_TOLERANCE lists the entry points whose kernel legitimately depends on the placement (none today)."""
import ctypes
import itertools

import torch

from cotnet_amd import _lib

F32, BF16, F16, F64 = torch.float32, torch.bfloat16, torch.float16, torch.float64
BF = _lib.COT_BF16
ROLES = ("in", "out", "inout", "ws")
MIN_MARGIN = 2048   # elements
MARGIN_PLANES = 64
# entry point -> (kernel on plain operands, kernel on margined ones, why the placement chooses): compared against the family's
# reference at its GPU test's tolerance instead of by bits.  Empty: every entry point takes the same kernel at every placement here.
BY_TOLERANCE = {}


def P(t):
    if t is None:
        return None
    return ctypes.c_void_p(getattr(t, "fp_ptr", None) or t.data_ptr())


def dt(dtype):
    return _lib.dtype_code(dtype)


def _fill(buf, dtype, role, plain):
    """the whole allocation `buf` (uint8) filled for an operand of `dtype` in `role`"""
    if role == "ws":
        buf.fill_(0x7f)
    elif dtype.is_floating_point:
        buf.view(dtype).fill_(float("nan"))
    else:
        buf.fill_(0x5A if (plain and role == "out") else 0xA5)


class Operand:
    def __init__(self, role, body, raw, off, nbytes, name):
        self.role, self.body, self.raw, self.off, self.nbytes, self.name = role, body, raw, off, nbytes, name
        self.snap = raw.clone()


class Arena:
    """place(t, role) -> the operand the kernel gets.  base None: plain operands (a fresh allocation each, no margins); base 0 / 16: each
    operand inside its own margined allocation with its first byte at `base` (mod 256).  Operands documented as 4- or 8-byte aligned
    blocks (align=4 / 8) sit at exactly that alignment, off any 16-byte boundary, when base is 16."""

    def __init__(self, dev="cpu", base=None):
        assert base in (None, 0, 16)
        self.dev, self.base = dev, base
        self.ops, self.kernels = [], []

    def place(self, t, role, plane=None, row=None, align=16, name=None, guard=0):
        """guard: elements before and behind the operand that its entry point documents as readable memory of the caller's allocation
        (cot_conv3x3g_backward_weight_guarded's x): the plain operand's allocation has exactly them (rounded up to 16 bytes, as
        conv3x3g.new_guarded allocates), filled like a margin; the margins are wider than any guard"""
        assert role in ROLES and align in (4, 8, 16)
        shape, dtype, item, n = tuple(t.shape), t.dtype, t.element_size(), t.numel()
        nbytes = n * item
        if plane is None:
            plane = shape[-1] * shape[-2] if len(shape) >= 4 else (shape[-1] if len(shape) >= 2 else 1)
        if row is None:
            row = shape[-1] if len(shape) >= 2 else 0
        if self.base is None:
            off = (guard * item + 15) // 16 * 16
            raw = torch.empty(max((nbytes + 15) // 16 * 16, 16) + 2 * off, dtype=torch.uint8, device=self.dev)
        else:
            margin = (max(MARGIN_PLANES * plane + row + 1, MIN_MARGIN, guard) * item + 255) // 256 * 256
            raw = torch.empty(2 * margin + (nbytes + 255) // 256 * 256 + 512, dtype=torch.uint8, device=self.dev)
            want = self.base if align == 16 else (align if self.base else 0)
            off = margin + (want - (raw.data_ptr() + margin)) % 256
            assert (raw.data_ptr() + off) % 256 == want and off >= margin and raw.numel() - off - nbytes >= margin
        assert raw.data_ptr() % 16 == 0 and off % item == 0
        _fill(raw, dtype, role, self.base is None)
        body = raw[off:off + nbytes].view(dtype).view(shape)
        if role in ("in", "inout"):
            body.copy_(t.to(self.dev))
        body.fp_ptr = raw.data_ptr() + off  # (an empty operand still has an address: a workspace query that answered 0)
        self.ops.append(Operand(role, body, raw, off, nbytes, name or f"#{len(self.ops)} {role} {dtype} {shape}"))
        return body

    def i(self, t, **kw):
        return self.place(t, "in", **kw)

    def io(self, t, **kw):
        return self.place(t, "inout", **kw)

    def o(self, shape, dtype=BF16, **kw):
        return self.place(torch.empty(tuple(shape) if not isinstance(shape, int) else (shape,), dtype=dtype), "out", **kw)

    def w(self, nbytes, **kw):
        return self.place(torch.empty(int(nbytes), dtype=torch.uint8), "ws", **kw)

    def check(self, plain=None):
        for op in self.ops:
            raw, snap, lo, hi = op.raw, op.snap, op.off, op.off + op.nbytes
            for what, a, b in (("before", raw[:lo], snap[:lo]), ("behind", raw[hi:], snap[hi:])):
                if not torch.equal(a, b):
                    at = int((a != b).nonzero()[0 if what == "behind" else -1])
                    where = at if what == "behind" else at - lo
                    raise AssertionError(f"{op.name}: the margin {what} the operand was written ({where:+d} bytes from its {'end' if what == 'behind' else 'start'})")
            if op.role == "in":
                assert torch.equal(raw[lo:hi], snap[lo:hi]), f"{op.name}: an input was modified"
            if op.role in ("out", "inout") and op.body.numel():
                if op.body.dtype.is_floating_point:
                    bad = torch.isnan(op.body)
                    if bool(bad.any()):
                        at = int(bad.reshape(-1).nonzero()[0])
                        raise AssertionError(f"{op.name}: element {at} is NaN ({int(bad.sum())} of {bad.numel()}): left unwritten, or a margin value was read and used")
                elif op.role == "out" and op.body.element_size() >= 4:
                    fill = torch.full_like(op.body, 0).view(torch.uint8).fill_(0xA5).view(op.body.dtype)
                    assert not bool((op.body == fill.view(op.body.shape)).any()), f"{op.name}: an element still holds its fill"
        if plain is None:
            return
        assert len(plain.ops) == len(self.ops), "the two runs of a case placed different operands"
        if self.kernels != plain.kernels:
            diff = [(a, b) for a, b in itertools.zip_longest(plain.kernels, self.kernels) if a != b]
            assert all(a and b and a[0] == b[0] and a[0] in BY_TOLERANCE for a, b in diff), f"another kernel by placement: {diff[:4]}"
            return  # (the case compares with its reference itself)
        for op, ref in zip(self.ops, plain.ops):
            if op.role in ("out", "inout"):
                same = torch.equal(op.body, ref.body) if not op.body.dtype.is_floating_point else \
                    torch.equal(op.body.view(torch.uint8), ref.body.view(torch.uint8))
                assert same, f"{op.name}: differs from the same call on plain operands"


class Recording:
    """the library with every call recorded: names into `names` (the completeness test), (name, cot_last_kernel()) into the arena's log;
    a cot_status other than COT_OK is an assertion failure.  soft(name, ...) returns COT_ERR_UNSUPPORTED instead of failing on it."""

    def __init__(self, L, arena=None, names=None):
        self.__dict__.update(_L=L, _arena=arena, _names=names if names is not None else set())

    def _call(self, name, args, soft):
        fn = getattr(self._L, name)
        self._names.add(name)
        rc = fn(*args)
        sym = _lib.SYMBOLS.get(name)
        if sym is not None and sym[0] is ctypes.c_int and name not in _lib.NOT_STATUS:
            if not (soft and rc == _lib.COT_ERR_UNSUPPORTED):
                assert rc == 0, (name, rc, self._L.cot_last_error())
            if self._arena is not None and not name.endswith("_tuning"):
                self._arena.kernels.append((name, rc, self._L.cot_last_kernel() if rc == 0 else b""))
        return rc

    def soft(self, name, *args):
        return self._call(name, args, True)

    def __getattr__(self, name):
        if not name.startswith("cot_"):
            return getattr(self._L, name)
        return lambda *args: self._call(name, args, False)


def _sync(dev):
    if str(dev).startswith("cuda"):
        torch.cuda.synchronize()


def run_case(L, case, args=(), base=0, names=None):
    """`case` on plain operands, then on margined ones at `base`; all four checks"""
    dev = getattr(L, "_test_device", "cpu")
    plain = Arena(dev, None)
    case(Recording(L, plain, names), plain, *args)
    _sync(dev)
    arena = Arena(dev, base)
    case(Recording(L, arena, names), arena, *args)
    _sync(dev)
    plain.check()
    arena.check(plain)
    return arena


def _gen(*seed):
    return torch.Generator().manual_seed(sum((i + 1) * int(s) for i, s in enumerate(seed)) + 1)


def _rn(g, *shape, dtype=BF16, scale=1.0, shift=0.0):
    return (torch.randn(*shape, generator=g) * scale + shift).to(dtype)


def _geom(N, C, H, W, heads=1, wC=None, k=(3, 3), s=(1, 1), p=(1, 1), d=(1, 1)):
    return _lib.AggGeom(N, C, H, W, heads, wC if wC is not None else C // 8, k[0], k[1], s[0], s[1], p[0], p[1], d[0], d[1])


# ---------------------------------------------------------------------------------------------------------------- aggregation

def case_agg(L, A, N, C, H, W, dtype):
    """cot_agg_* and cot_agg_softmax_* in the CoT layer's form (3x3, stride 1, pad 1, one head, C / wC = 8), NCHW"""
    g, d = _gen(N, C, H, W), dt(dtype)
    wC = C // 8
    x, w, go = A.i(_rn(g, N, C, H, W, dtype=dtype)), A.i(_rn(g, N, 1, wC, 9, H, W, dtype=dtype)), A.i(_rn(g, N, C, H, W, dtype=dtype))
    geo = _geom(N, C, H, W)
    G = ctypes.byref(geo)
    out = A.o((N, C, H, W), dtype)
    L.cot_agg_forward(P(x), P(w), P(out), G, d, 0, None)
    gx, gw = A.o(x.shape, dtype), A.o(w.shape, dtype)
    L.cot_agg_backward_input(P(go), P(w), P(gx), G, d, 0, None)
    L.cot_agg_backward_weight(P(go), P(x), P(gw), G, d, 0, None)
    for want_gx, want_gw, split in ((1, 1, 0), (1, 0, 0), (0, 1, 0), (1, 1, 1)):  # (split: tuning key 8, two launches)
        gx, gw = A.o(x.shape, dtype) if want_gx else None, A.o(w.shape, dtype) if want_gw else None
        with _lib.tuned(L, AGG_BWD_SPLIT=split):
            L.cot_agg_backward(P(go), P(x), P(w), P(gx), P(gw), G, d, 0, None)
    if dtype == BF16:  # (the fp32-unpacked LDS kernel behind the packed dot-product one)
        gx, gw = A.o(x.shape, dtype), A.o(w.shape, dtype)
        with _lib.tuned(L, DOT2=0):
            L.cot_agg_backward(P(go), P(x), P(w), P(gx), P(gw), G, d, 0, None)
    if (H, W) == (3, 10):  # (no LDS tile plan for this plane: refused before any launch, the caller composes softmax + cot_agg_forward)
        out, probs = A.i(_rn(g, N, C, H, W, dtype=dtype)), A.i(_rn(g, N, 1, wC, 9, H, W, dtype=dtype))  # (must stay as they are)
        assert L.soft("cot_agg_softmax_forward", P(x), P(w), P(out), P(probs), G, d, None) == _lib.COT_ERR_UNSUPPORTED
        return
    for with_probs in (1, 0):
        out, probs = A.o(x.shape, dtype), A.o(w.shape, dtype) if with_probs else None
        L.cot_agg_softmax_forward(P(x), P(w), P(out), P(probs), G, d, None)
        if with_probs:
            pin = A.i(probs.clone())
            gx, gl = A.o(x.shape, dtype), A.o(w.shape, dtype)
            L.cot_agg_softmax_backward(P(go), P(x), P(pin), P(gx), P(gl), G, d, None)


def case_agg_generic(L, A, dtype, layout):
    """the generic kernels: rectangular kernel, stride, heads, both layouts"""
    N, C, H, W, heads, wC, k, s, p = 2, 6, 9, 11, 2, 3, (3, 5), (2, 1), (1, 2)
    Ho, Wo = L.cot_agg_out_size(H, k[0], s[0], p[0], 1), L.cot_agg_out_size(W, k[1], s[1], p[1], 1)
    g, d = _gen(layout, 5), dt(dtype)
    kw = dict(plane=H * W, row=W)
    x = A.i(_rn(g, N * C * H * W, dtype=dtype), **kw)
    w = A.i(_rn(g, N * heads * wC * 15 * Ho * Wo, dtype=dtype), **kw)
    go = A.i(_rn(g, N * heads * C * Ho * Wo, dtype=dtype), **kw)
    geo = _geom(N, C, H, W, heads, wC, k, s, p)
    G = ctypes.byref(geo)
    out, gx, gw = A.o(go.shape, dtype, **kw), A.o(x.shape, dtype, **kw), A.o(w.shape, dtype, **kw)
    L.cot_agg_forward(P(x), P(w), P(out), G, d, layout, None)
    L.cot_agg_backward_input(P(go), P(w), P(gx), G, d, layout, None)
    L.cot_agg_backward_weight(P(go), P(x), P(gw), G, d, layout, None)
    gx, gw = A.o(x.shape, dtype, **kw), A.o(w.shape, dtype, **kw)
    L.cot_agg_backward(P(go), P(x), P(w), P(gx), P(gw), G, d, layout, None)


def case_agg_gn9(L, A, N, C, H, W):
    """GroupNorm-9 in the aggregation's prologue, both directions, and the forward that also emits the BatchNorm's row sums (with and
    without the prologue) + its finalize"""
    g = _gen(N, C, H, W)
    wC = C // 8
    x, go = A.i(_rn(g, N, C, H, W)), A.i(_rn(g, N, C, H, W))
    logits = A.i(_rn(g, N, 9 * wC, H, W, scale=0.4, shift=0.1))
    gm, gr = A.i(_rn(g, N * wC, dtype=F32, scale=0.1)), A.i(1 + 0.2 * torch.rand(N * wC, generator=g))
    gam, bet = A.i(_rn(g, 9 * wC, scale=0.3, shift=1.0)), A.i(_rn(g, 9 * wC, scale=0.2))
    geo = _geom(N, C, H, W)
    G = ctypes.byref(geo)
    if W % 2 == 0:
        out = A.o(x.shape)
        L.cot_agg_gn9_forward(P(x), P(logits), P(gm), P(gr), P(gam), P(bet), wC, P(out), G, BF, None)
        gx, gw = A.o(x.shape), A.o(logits.shape)
        rc = L.soft("cot_agg_gn9_backward", P(go), P(x), P(logits), P(gm), P(gr), P(gam), P(bet), wC, P(gx), P(gw), G, BF, None)
        assert rc == 0 or W != 20  # (the packed dot-product backward's widths; elsewhere refused before any launch)
        if rc:
            A.ops[-1].role = A.ops[-2].role = "in"  # (not the outputs of a refused call: they keep their fill)
    nrow = int(L.cot_agg_rowstats_floats(N, C, H))
    for gn in ((1, 0) if W % 2 == 0 else (0,)):
        out, rows = A.o(x.shape), A.o(nrow, F32)
        if gn:
            L.cot_agg_forward_rowstats(P(x), P(logits), P(out), P(rows), P(gm), P(gr), P(gam), P(bet), wC, G, BF, None)
        else:
            L.cot_agg_forward_rowstats(P(x), P(logits), P(out), P(rows), None, None, None, None, 0, G, BF, None)
        rin = A.i(rows.clone())
        for running in (1, 0):
            mean, rstd = A.o(C, F32), A.o(C, F32)
            rm, rv = (A.io(torch.zeros(C)), A.io(torch.ones(C))) if running else (None, None)
            nbt = A.io(torch.zeros((), dtype=torch.int64)) if running else None
            L.cot_bn_rowstats_finalize(P(rin), P(mean), P(rstd), P(rm), P(rv), P(nbt), N, C, H, W, 1e-5, 0.1, None)


def case_aggmix(L, A, N, C, wC, H, W, heads, dtype):
    """aggregation_zeropad_mix: the LDS-tiled kernels and (tuning key 51) the one-lane-per-element ones"""
    g, d = _gen(N, C, H, W, heads), dt(dtype)
    x = A.i(_rn(g, N, C, H, W, dtype=dtype))
    w1, w2 = A.i(_rn(g, N, heads, wC, 9, H, W, dtype=dtype)), A.i(_rn(g, N, heads, wC, 25, H, W, dtype=dtype))
    go = A.i(_rn(g, N, 2 * heads * C, H, W, dtype=dtype))
    geo = _geom(N, C, H, W, heads, wC)
    G = ctypes.byref(geo)
    for flat in (0, 1):
        with _lib.tuned(L, MIX_GENERIC=flat):
            out = A.o(go.shape, dtype)
            L.cot_aggmix_forward(P(x), P(w1), P(w2), P(out), G, 2, 2, d, None)
            for all_heads in (0, 1):
                gx = A.o(x.shape, dtype)
                L.cot_aggmix_backward_input(P(go), P(w1), P(w2), P(gx), G, 2, 2, all_heads, d, None)
            gw1, gw2 = A.o(w1.shape, dtype), A.o(w2.shape, dtype)
            L.cot_aggmix_backward_weight(P(go), P(x), P(gw1), P(gw2), G, 2, 2, d, None)


# ---------------------------------------------------------------------------------------------------------------- 1x1 convolutions

def case_conv1x1(L, A, N, Ci, Co, H, W, c1, dtype=BF16):
    """cot_conv1x1_*: one and two channel slabs, bias on / off, every accumulate combination of the data gradient, the weight gradient
    under forced split / slice counts and rows-per-wave overrides (workspace sized after the key is set)"""
    g, d, HW = _gen(N, Ci, Co, H, W, c1), dt(dtype), H * W
    bdt = dtype  # (fp32: the bias is fp32)
    x = _rn(g, N, Ci, H, W, dtype=dtype)
    cc1 = c1 or Ci
    x1 = A.i(x[:, :cc1].contiguous())
    x2 = A.i(x[:, cc1:].contiguous()) if c1 else None
    w, b = A.i(_rn(g, Co, Ci, dtype=dtype, scale=Ci ** -0.5)), A.i(_rn(g, Co, dtype=bdt))
    gy = A.i(_rn(g, N, Co, H, W, dtype=dtype))
    for bias, rows in ((1, 0), (0, 2), (0, 4)):
        y = A.o((N, Co, H, W), dtype)
        with _lib.tuned(L, C1_ROWS_PER_WAVE=rows):
            L.cot_conv1x1_forward(P(x1), P(x2), cc1, P(w), P(b) if bias else None, P(y), N, Ci, Co, HW, d, None)
    general = dtype == F32
    size = (lambda bias: L.cot_convg_workspace(N, Ci, Co, 1, HW, 1, 1)) if general else (lambda bias: L.cot_conv1x1_workspace(N, Ci, Co, HW, bias))
    for acc in range(4 if c1 else 2):
        ws = A.w(size(0))
        gx1 = A.io(_rn(g, N, cc1, H, W, dtype=dtype)) if acc & 1 else A.o((N, cc1, H, W), dtype)
        gx2 = None
        if c1:
            gx2 = A.io(_rn(g, N, Ci - cc1, H, W, dtype=dtype)) if acc & 2 else A.o((N, Ci - cc1, H, W), dtype)
        L.cot_conv1x1_backward_data(P(gy), P(w), P(gx1), P(gx2), cc1, acc, P(ws), N, Ci, Co, HW, d, None)
    for bias, k11, k25 in ((1, 2048, 0), (0, -2, 0), (1, -3, 0), (0, 2048, 3 << 24), (1, 2048, 7 << 24)):
        with _lib.tuned(L, C1_WGRAD_WAVES=k11, WGRAD2_BITS=k25):
            ws = A.w(size(bias))
            gw, gb = A.o((Co, Ci), dtype), A.o(Co, bdt) if bias else None
            L.cot_conv1x1_backward_weight(P(gy), P(x1), P(x2), cc1, P(gw), P(gb), P(ws), N, Ci, Co, HW, d, None)


def case_conv1x1_epilogues(L, A, N, Ci, Co, H, W, c1):
    """the 1x1 forward that also emits statistics (cot_conv1x1_forward_stats / _gn9: planes of more than 256 pixels), their two
    finalizes and the BatchNorm applied from them"""
    g, HW = _gen(N, Ci, Co, H, W), H * W
    x = _rn(g, N, Ci, H, W)
    cc1 = c1 or Ci
    x1 = A.i(x[:, :cc1].contiguous())
    x2 = A.i(x[:, cc1:].contiguous()) if c1 else None
    w, b = A.i(_rn(g, Co, Ci, scale=Ci ** -0.5)), A.i(_rn(g, Co))
    assert L.cot_conv1x1_stats_covers(Ci, cc1, 1 if c1 else 0, HW) == 1 and L.cot_gn9_fused_covers(Ci, cc1, 1 if c1 else 0, HW, W) in (0, 1)
    nst = int(L.cot_gn9_stats_floats(N, Co, HW))
    for name, bias in (("cot_conv1x1_forward_stats", 0), ("cot_conv1x1_forward_gn9", 1)):
        y, stats = A.o((N, Co, H, W)), A.o(nst, F32)
        getattr(L, name)(P(x1), P(x2), cc1, P(w), P(b) if bias else None, P(y), P(stats), N, Ci, Co, HW, BF, None)
    yin, sin = A.i(y.clone()), A.i(stats.clone())
    gmean, grstd = A.o(N * Co // 9, F32), A.o(N * Co // 9, F32)
    L.cot_gn9_stats_finalize(P(sin), P(gmean), P(grstd), N, Co, HW, 1e-5, None)
    for running in (1, 0):
        mean, rstd = A.o(Co, F32), A.o(Co, F32)
        rm, rv = (A.io(torch.zeros(Co)), A.io(torch.ones(Co))) if running else (None, None)
        nbt = A.io(torch.zeros((), dtype=torch.int64)) if running else None
        L.cot_bn_tile_stats_finalize(P(sin), P(mean), P(rstd), P(rm), P(rv), P(nbt), N, Co, HW, 1e-5, 0.1, None)
    m_in, r_in = A.i(mean.clone()), A.i(rstd.clone())
    gamma, beta = A.i(torch.rand(Co, generator=g) + 0.5), A.i(_rn(g, Co, dtype=F32, scale=0.2))
    res = A.i(_rn(g, N, Co, H, W))
    nb = int(L.cot_bn_relu_mask_bytes(N, Co, HW, BF))
    for act, with_res, with_mask in ((0, 0, 0), (1, 1, 1), (1, 1, 0), (2, 0, 0), (1, 0, 0)):
        z = A.o((N, Co, H, W))
        mk = A.o(nb, torch.uint8) if with_mask and nb else None
        L.cot_bn_act_apply_forward(P(yin), P(res) if with_res else None, P(z), P(mk), P(gamma), P(beta), P(m_in), P(r_in), N, Co, HW, act,
                                   BF, None)


def case_relu_res(L, A, N, Ci, Co, HW):
    """conv1's data gradient with the masked residual gradient folded in"""
    g = _gen(N, Ci, Co, HW)
    assert L.cot_conv1x1_backward_data_relu_res_covers(N, Ci, Co, HW, BF) == 1
    gy, w = A.i(_rn(g, N, Co, HW)), A.i(_rn(g, Co, Ci, scale=Co ** -0.5))
    gout = A.i(_rn(g, N, Ci, HW))
    bits = (torch.randn(N * Ci * HW // 8, 8, generator=g) > 0).to(torch.int32)
    mask = A.i((bits * (2 ** torch.arange(8, dtype=torch.int32))).sum(1).to(torch.uint8), plane=HW // 8, row=0)
    assert mask.numel() == int(L.cot_bn_relu_mask_bytes(N, Ci, HW, BF))
    gx = A.o((N, Ci, HW))
    L.cot_conv1x1_backward_data_relu_res(P(gy), P(w), P(gx), P(gout), P(mask), N, Ci, Co, HW, BF, None)


def case_conv1x1g(L, A, N, Ci, Co, G, H, W, dtype):
    """grouped 1x1 (conv_gen.hip, or the tuned kernels group by group)"""
    g, d, HW = _gen(N, Ci, Co, G, H, W), dt(dtype), H * W
    x, gy = A.i(_rn(g, N, Ci, H, W, dtype=dtype)), A.i(_rn(g, N, Co, H, W, dtype=dtype))
    w, b = A.i(_rn(g, Co, Ci // G, dtype=dtype, scale=(Ci // G) ** -0.5)), A.i(_rn(g, Co, dtype=dtype))
    for bias in (1, 0):
        y = A.o(gy.shape, dtype)
        L.cot_conv1x1g_forward(P(x), P(w), P(b) if bias else None, P(y), N, Ci, Co, G, HW, d, None)
    for acc in (0, 1):
        gx = A.io(_rn(g, N, Ci, H, W, dtype=dtype)) if acc else A.o(x.shape, dtype)
        L.cot_conv1x1g_backward_data(P(gy), P(w), P(gx), acc, N, Ci, Co, G, HW, d, None)
    for bias, k11 in ((1, 2048), (0, -2)):
        with _lib.tuned(L, C1_WGRAD_WAVES=k11):
            ws = A.w(L.cot_convg_workspace(N, Ci, Co, G, HW, 1, 1))
            gw, gb = A.o(w.shape, dtype), A.o(Co, dtype) if bias else None
            L.cot_conv1x1g_backward_weight(P(gy), P(x), P(gw), P(gb), P(ws), N, Ci, Co, G, HW, d, None)


# ---------------------------------------------------------------------------------------------------------------- 3x3 convolutions

def case_conv3x3(L, A, N, C, G, H, W, dtype=BF16):
    """cot_conv3x3g_*: masks, forward, data gradient (accumulate on / off), weight gradient (forced splits / slices), the guarded
    weight gradient with exactly the promised readable elements around x (they are NaN), the packed forms.  fp32 and group widths off
    the 8-channel grid take the general kernels (conv_gen.hip) on the same entry points"""
    g, d = _gen(N, C, G, H, W), dt(dtype)
    x, gy = A.i(_rn(g, N, C, H, W, dtype=dtype), guard=W + 1), A.i(_rn(g, N, C, H, W, dtype=dtype))
    w = A.i(_rn(g, C, C // G, 3, 3, dtype=dtype, scale=(9 * C // G) ** -0.5))
    masks = A.o(int(L.cot_conv3x3g_masks_bytes(H, W)), torch.uint8)
    L.cot_conv3x3g_masks(P(masks), H, W, None)
    mk = A.i(masks.clone())
    geo = (N, C, C, G, H, W)
    size = lambda: max(int(L.cot_conv3x3g_workspace(*geo)), int(L.cot_convg_workspace(*geo, 3)))  # noqa: E731
    ws, y = A.w(size()), A.o(x.shape, dtype)
    L.cot_conv3x3g_forward(P(x), P(w), P(y), P(mk), P(ws), *geo, d, None)
    for acc in (0, 1):
        ws = A.w(size())
        gx = A.io(_rn(g, N, C, H, W, dtype=dtype)) if acc else A.o(x.shape, dtype)
        L.cot_conv3x3g_backward_data(P(gy), P(w), P(gx), acc, P(mk), P(ws), *geo, d, None)
    for k11, k25 in ((2048, 0), (-2, 0), (2048, 2 << 24), (2048, 7 << 24)):
        with _lib.tuned(L, C1_WGRAD_WAVES=k11, WGRAD2_BITS=k25):
            ws, gw = A.w(size()), A.o(w.shape, dtype)
            L.cot_conv3x3g_backward_weight(P(gy), P(x), P(gw), P(mk), P(ws), *geo, d, None)
            for guard in (W + 1, 0):
                ws, gw = A.w(size()), A.o(w.shape, dtype)
                L.cot_conv3x3g_backward_weight_guarded(P(gy), P(x), P(gw), P(mk), P(ws), *geo, d, guard, None)
    if dtype != BF16:
        return
    nb = int(L.cot_conv3x3g_packed_bytes(C, C, G))
    for mode in (0, 1):
        packed = A.w(nb)
        if L.soft("cot_conv3x3g_pack", P(w), P(packed), mode, *geo, d, None) != 0:
            continue  # (not an LDS-kernel geometry: the ordinary entry points serve it)
        pk = A.i(packed.clone())
        if mode == 0:
            y = A.o(x.shape, dtype)
            L.cot_conv3x3g_forward_packed(P(x), P(pk), P(y), *geo, d, None)
        else:
            for acc in (0, 1):
                gx = A.io(_rn(g, N, C, H, W, dtype=dtype)) if acc else A.o(x.shape, dtype)
                L.cot_conv3x3g_backward_data_packed(P(gy), P(pk), P(gx), acc, *geo, d, None)


# ---------------------------------------------------------------------------------------------------------------- stems

def case_stem7(L, A, N, H, W, dtype):
    g, d = _gen(N, H, W), dt(dtype)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x, w = A.i(_rn(g, N, 3, H, W, dtype=dtype)), A.i(_rn(g, 64, 3, 7, 7, dtype=dtype, scale=1 / 12))
    gy = A.i(_rn(g, N, 64, Ho, Wo, dtype=dtype))
    for lds in (1, 0):
        with _lib.tuned(L, STEM_LDS=lds):
            y = A.o(gy.shape, dtype)
            L.cot_stem7x7s2_forward(P(x), P(w), P(y), N, H, W, d, None)
    ws, gw = A.w(L.cot_stem7x7s2_workspace(N, H, W)), A.o(w.shape, dtype)
    L.cot_stem7x7s2_backward_weight(P(gy), P(x), P(gw), P(ws), N, H, W, d, None)


def case_stem3(L, A, N, H, W, Co):
    g = _gen(N, H, W, Co)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x, w = A.i(_rn(g, N, 3, H, W)), A.i(_rn(g, Co, 3, 3, 3, scale=0.2))
    gy = A.i(_rn(g, N, Co, Ho, Wo))
    y = A.o(gy.shape)
    covered = Wo % 8 == 0 and (Ho * Wo) % 32 == 0
    rc = L.soft("cot_stem3x3s2_forward", P(x), P(w), P(y), N, H, W, Co, BF, None)
    nb = int(L.cot_stem3x3s2_workspace(N, H, W, Co))
    assert (rc == 0) == covered and (nb > 0) == covered  # (off the grid: refused before any launch, the caller keeps nn.Conv2d)
    ws, gw = A.w(nb), A.o(w.shape)
    rc = L.soft("cot_stem3x3s2_backward_weight", P(gy), P(x), P(gw), P(ws), N, H, W, Co, BF, None)
    assert (rc == 0) == covered
    if not covered:  # nothing may have been written: the outputs are not outputs of a refused call
        for op in A.ops:
            op.role = "in" if op.role == "out" else op.role  # (checked against the fill they were given)


# ---------------------------------------------------------------------------------------------------------------- poolings

def case_pools(L, A, N, C, H, W, dtype):
    """the 3x3 / stride-2 poolings (row-block and one-lane-per-pixel forms, tuning key 27), the taps forms, the blur pool and -- on even
    planes -- AvgPool2d(2, 2) and the sub-sampling"""
    g, d, planes = _gen(N, C, H, W), dt(dtype), N * C
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x = A.i(torch.relu(_rn(g, N, C, H, W)).to(dtype))  # (post-ReLU: ties at zero)
    gy = A.i(_rn(g, N, C, Ho, Wo, dtype=dtype))
    for blk in (1, 0):
        with _lib.tuned(L, POOL_TILE=blk):
            y, gx = A.o(gy.shape, dtype), A.o(x.shape, dtype)
            L.cot_maxpool3x3s2_forward(P(x), P(y), planes, H, W, d, None)
            L.cot_maxpool3x3s2_backward(P(gy), P(x), P(gx), planes, H, W, d, None)
            y, taps, gx = A.o(gy.shape, dtype), A.o(gy.shape, torch.uint8), A.o(x.shape, dtype)
            L.cot_maxpool3x3s2_forward_taps(P(x), P(y), P(taps), planes, H, W, d, None)
            tin = A.i(taps.clone())
            L.cot_maxpool3x3s2_backward_taps(P(gy), P(tin), P(gx), planes, H, W, d, None)
            y, gx = A.o(gy.shape, dtype), A.o(x.shape, dtype)
            L.cot_avgpool3x3s2_forward(P(x), P(y), planes, H, W, d, None)
            L.cot_avgpool3x3s2_backward(P(gy), P(gx), planes, H, W, d, None)
            if H >= 2 and W >= 2:
                y, gx = A.o(gy.shape, dtype), A.o(x.shape, dtype)
                L.cot_blurpool3x3s2_forward(P(x), P(y), planes, H, W, d, None)
                L.cot_blurpool3x3s2_backward(P(gy), P(gx), planes, H, W, d, None)
    if H % 2 == 0 and W % 2 == 0:
        for name in ("cot_avgpool2x2s2", "cot_subsample2"):
            y, gx = A.o(gy.shape, dtype), A.o(x.shape, dtype)
            getattr(L, name + "_forward")(P(x), P(y), planes, H, W, d, None)
            getattr(L, name + "_backward")(P(gy), P(gx), planes, H, W, d, None)


# ---------------------------------------------------------------------------------------------------------------- gate / radix tail

def case_tail(L, A, N, C, H, W, dtype):
    """cot_se_* and cot_radix_*: the [planes] forms and the channel-major-descriptor (_t) forms, k == NULL too"""
    g, d, HW, planes = _gen(N, C, H, W), dt(dtype), H * W, N * C
    y, k, go = (A.i(_rn(g, N, C, H, W, dtype=dtype)) for _ in range(3))
    lg = A.i(_rn(g, N, C, dtype=dtype, scale=2.0))
    gap, out = A.o((N, C), dtype), A.o(y.shape, dtype)
    L.cot_se_gap(P(y), P(gap), planes, HW, d, None)
    L.cot_se_gate(P(y), P(lg), P(out), planes, HW, d, None)
    gx, gl = A.o(y.shape, dtype), A.o((N, C), dtype)
    L.cot_se_gate_backward(P(go), P(y), P(lg), P(gx), P(gl), planes, HW, d, None)
    attn = A.i(torch.softmax(torch.randn(N, C, 2, generator=g), 2).to(dtype))
    gap, out = A.o((N, C), dtype), A.o(y.shape, dtype)
    L.cot_radix_gap(P(y), P(k), P(gap), planes, HW, d, None)
    L.cot_radix_mix(P(y), P(k), P(attn), P(out), planes, HW, d, None)
    gyy, gk, ga = A.o(y.shape, dtype), A.o(y.shape, dtype), A.o((N, C, 2), dtype)
    L.cot_radix_mix_backward(P(go), P(y), P(k), P(attn), P(gyy), P(gk), P(ga), planes, HW, d, None)
    logT, ggapT = A.i(_rn(g, 2 * C, N, dtype=dtype)), A.i(_rn(g, C, N, dtype=dtype, scale=0.5))
    for with_k in (1, 0):
        gapT = A.o((C, N), dtype)
        L.cot_radix_gap_t(P(y), P(k) if with_k else None, P(gapT), N, C, HW, d, None)
    out, at = A.o(y.shape, dtype), A.o((N, C, 2), dtype)
    L.cot_radix_mix_logits(P(y), P(k), P(logT), P(out), P(at), N, C, HW, d, None)
    ain = A.i(at.clone())
    glog = A.o((2 * C, N), dtype)
    L.cot_radix_mix_backward_reduce(P(go), P(y), P(k), P(ain), P(glog), N, C, HW, d, None)
    gyy, gk = A.o(y.shape, dtype), A.o(y.shape, dtype)
    L.cot_radix_mix_backward_apply(P(go), P(ain), P(ggapT), P(gyy), P(gk), N, C, HW, d, None)


def _cm(t):
    return t.transpose(0, 1).contiguous()


def case_tail_lay(L, A, N, C, H, W, k50):
    """cot_radix_*_lay at every lay bit combination (tests/layout_cases.py radix_case); the 7 x 7 eight-planes-per-wave form and one
    wave per plane (tuning key 50)"""
    g, HW = _gen(N, C, H, W), H * W
    hy, hk, hg = (_rn(g, N, C, H, W) for _ in range(3))
    logT, ggapT = A.i(_rn(g, 2 * C, N)), A.i(_rn(g, C, N, scale=0.5))
    ain = A.i(torch.softmax(torch.randn(N, C, 2, generator=g), 2).bfloat16())
    both = lambda t: (A.i(t), A.i(_cm(t)))  # noqa: E731
    y, k, go = both(hy), both(hk), both(hg)
    with _lib.tuned(L, RADIX_PACK7=k50):
        for b0, b1, b2 in itertools.product((0, 1), repeat=3):
            lay = b0 | (b1 << 1) | (b2 << 2)
            if not b2:
                gapT = A.o((C, N))
                L.cot_radix_gap_t_lay(P(y[b0]), P(k[b1]), P(gapT), N, C, HW, lay, BF, None)
                if not b1:
                    gapT = A.o((C, N))
                    L.cot_radix_gap_t_lay(P(y[b0]), None, P(gapT), N, C, HW, lay, BF, None)
            out, at = A.o(hy.shape), A.o((N, C, 2))
            L.cot_radix_mix_logits_lay(P(y[b0]), P(k[b1]), P(logT), P(out), P(at), N, C, HW, lay, BF, None)
            glog = A.o((2 * C, N))
            L.cot_radix_mix_backward_reduce_lay(P(go[b0]), P(y[b1]), P(k[b2]), P(ain), P(glog), N, C, HW, lay, BF, None)
            gyy, gk = A.o(hy.shape), A.o(hy.shape)
            L.cot_radix_mix_backward_apply_lay(P(go[b0]), P(ain), P(ggapT), P(gyy), P(gk), N, C, HW, lay, BF, None)


def case_tail_bn(L, A, N, C, H, W, dtype, lay_k, sums):
    """BatchNorm + SiLU folded into the radix tail: the statistics by their own launches (cot_bn_batch_stats) or as chunk sums finalized
    in the pooling kernel's prologue (cot_bn_stats_sums), running statistics given and NULL, k / out / gk channel-major or not"""
    g, d, HW = _gen(N, C, H, W, lay_k, sums), dt(dtype), H * W
    a = A.i(_rn(g, N, C, H, W, dtype=dtype, scale=1.3, shift=0.4))
    hk, hg = _rn(g, N, C, H, W, dtype=dtype), _rn(g, N, C, H, W, dtype=dtype)
    k, go = A.i(_cm(hk) if lay_k else hk), A.i(_cm(hg) if lay_k else hg)
    gamma, beta = A.i(1 + 0.3 * torch.randn(C, generator=g)), A.i(0.2 * torch.randn(C, generator=g))
    logT, ggapT = A.i(_rn(g, 2 * C, N, dtype=dtype)), A.i(_rn(g, C, N, dtype=dtype, scale=0.5))
    nws = 4 * max(int(L.cot_bn_act_workspace(N, C)), 1)
    for running in (1, 0):
        mean, rstd, ws = A.o(C, F32), A.o(C, F32), A.w(nws)
        rm, rv = (A.io(torch.zeros(C)), A.io(torch.ones(C))) if running else (None, None)
        nbt = A.io(torch.zeros((), dtype=torch.int64)) if running else None
        gapT = A.o((C, N), dtype)
        if sums:
            L.cot_bn_stats_sums(P(a), P(ws), N, C, HW, d, None)
            L.cot_radix_gap_t_bn(P(a), P(k), P(gapT), P(gamma), P(beta), P(mean), P(rstd), P(rm), P(rv), P(nbt), P(ws), N, C, HW, 1e-5, 0.1,
                                 2 if lay_k else 0, d, None)
        else:
            L.cot_bn_batch_stats(P(a), P(mean), P(rstd), P(rm), P(rv), P(nbt), P(ws), N, C, HW, 1e-5, 0.1, d, None)
            m_in, r_in = A.i(mean.clone()), A.i(rstd.clone())
            L.cot_radix_gap_t_bn(P(a), P(k), P(gapT), P(gamma), P(beta), P(m_in), P(r_in), None, None, None, None, N, C, HW, 1e-5, 0.1,
                                 2 if lay_k else 0, d, None)
    m_in, r_in = A.i(mean.clone()), A.i(rstd.clone())
    out, at = A.o(a.shape, dtype), A.o((N, C, 2), dtype)
    L.cot_radix_mix_logits_bn(P(a), P(k), P(logT), P(out), P(at), P(gamma), P(beta), P(m_in), P(r_in), N, C, HW, 6 if lay_k else 0, d, None)
    ain = A.i(at.clone())
    glog, tsum = A.o((2 * C, N), dtype), A.o(N * C * 4, F32)
    lay = 5 if lay_k else 0
    L.cot_radix_mix_backward_reduce_bn(P(go), P(a), P(k), P(ain), P(glog), P(tsum), P(gamma), P(beta), P(m_in), P(r_in), N, C, HW, lay, d, None)
    tin = A.i(tsum.clone())
    ga, gk, dg, db = A.o(a.shape, dtype), A.o(a.shape, dtype), A.o(C, F32), A.o(C, F32)
    L.cot_radix_mix_backward_apply_bn(P(go), P(a), P(ain), P(ggapT), P(tin), P(ga), P(gk), P(gamma), P(beta), P(m_in), P(r_in), P(dg), P(db),
                                      N, C, HW, lay, d, None)


# ---------------------------------------------------------------------------------------------------------------- GroupNorm-9

def case_gn9(L, A, N, G, H, W, dtype, k49=1):
    """cot_group_norm9_*: forward, backward, the backward as its two launches (dgamma == dbeta == NULL + cot_group_norm9_backward_params)
    and, in bf16, every lay bit combination"""
    g, d, C, HW = _gen(N, G, H, W), dt(dtype), 9 * G, H * W
    hx, hdy = _rn(g, N, C, H, W, dtype=dtype, scale=1.5, shift=0.3), _rn(g, N, C, H, W, dtype=dtype)
    x, dy = A.i(hx), A.i(hdy)
    gamma, beta = A.i(_rn(g, C, dtype=dtype, scale=0.3, shift=1.0)), A.i(_rn(g, C, dtype=dtype, scale=0.2))
    with _lib.tuned(L, GN9_PACK=k49):
        y, mean, rstd = A.o(x.shape, dtype), A.o(N * G, F32), A.o(N * G, F32)
        L.cot_group_norm9_forward(P(x), P(gamma), P(beta), P(y), P(mean), P(rstd), N, C, HW, 1e-5, d, None)
        m_in, r_in = A.i(mean.clone()), A.i(rstd.clone())
        dx, dg, db, ws = A.o(x.shape, dtype), A.o(C, dtype), A.o(C, dtype), A.w(8 * N * C)
        L.cot_group_norm9_backward(P(dy), P(x), P(m_in), P(r_in), P(gamma), P(dx), P(dg), P(db), P(ws), N, C, HW, d, None)
        if dtype != BF16:
            return
        dx, dg, db, ws = A.o(x.shape, dtype), A.o(C, dtype), A.o(C, dtype), A.w(8 * N * C)
        L.cot_group_norm9_backward(P(dy), P(x), P(m_in), P(r_in), P(gamma), P(dx), None, None, P(ws), N, C, HW, d, None)
        L.cot_group_norm9_backward_params(P(ws), P(dg), P(db), N, C, d, None)
        xs, dys = (x, A.i(_cm(hx))), (dy, A.i(_cm(hdy)))
        for b0, b1, b2 in itertools.product((0, 1), repeat=3):
            if not b2:
                y, mean, rstd = A.o(x.shape, dtype), A.o(N * G, F32), A.o(N * G, F32)
                L.cot_group_norm9_forward_lay(P(xs[b0]), P(gamma), P(beta), P(y), P(mean), P(rstd), N, C, HW, 1e-5, b0 | (b1 << 1), d, None)
            dx, dg, db, ws = A.o(x.shape, dtype), A.o(C, dtype), A.o(C, dtype), A.w(8 * N * C)
            L.cot_group_norm9_backward_lay(P(dys[b0]), P(xs[b1]), P(m_in), P(r_in), P(gamma), P(dx), P(dg), P(db), P(ws), N, C, HW,
                                           b0 | (b1 << 1) | (b2 << 2), d, None)


# ---------------------------------------------------------------------------------------------------------------- BatchNorm

_BN_COMBOS = ((0, 0), (1, 1), (2, 0), (1, 0), (0, 1))  # (activation, residual)


def case_bn(L, A, N, C, H, W, dtype, k21, k12):
    """cot_bn_act_*: streaming (tuning key 21 = 0) and channel-resident kernels, the finalize folded or not (key 12); activation codes,
    residual on / off, running statistics given and NULL; the _ps and _mask forms, inference, SiLU after a residual (forward only)"""
    g, d, HW = _gen(N, C, H, W), dt(dtype), H * W
    x = A.i(_rn(g, N, C, H, W, dtype=dtype, scale=1.5, shift=0.7))
    res, dy = A.i(_rn(g, N, C, H, W, dtype=dtype)), A.i(_rn(g, N, C, H, W, dtype=dtype))
    gamma, beta = A.i(torch.rand(C, generator=g) + 0.5), A.i(0.2 * torch.randn(C, generator=g))
    ps = A.i((torch.rand(N, generator=g) < 0.7).float() / 0.7)
    run_m, run_v = A.i(0.3 * torch.randn(C, generator=g)), A.i(torch.rand(C, generator=g) + 0.5)
    with _lib.tuned(L, BN_CHAN=k21, BN_FOLD=k12):
        nws = 4 * max(int(L.cot_bn_act_workspace(N, C)), 1)
        nb = int(L.cot_bn_relu_mask_bytes(N, C, HW, d))

        def stats(running=1):
            return (A.o(C, F32), A.o(C, F32), A.io(torch.zeros(C)) if running else None, A.io(torch.ones(C)) if running else None,
                    A.io(torch.zeros((), dtype=torch.int64)) if running else None, A.w(nws))
        for i, (act, with_res) in enumerate(_BN_COMBOS + ((2, 1),)):
            r = res if with_res else None
            mean, rstd, rm, rv, nbt, ws = stats(running=i != 2)
            y = A.o(x.shape, dtype)
            L.cot_bn_act_forward(P(x), P(r), P(y), P(gamma), P(beta), P(mean), P(rstd), P(rm), P(rv), P(nbt), P(ws), N, C, HW, 1e-5, 0.1, act,
                                 d, None)
            z = A.o(x.shape, dtype)
            L.cot_bn_act_inference(P(x), P(r), P(z), P(gamma), P(beta), P(run_m), P(run_v), N, C, HW, 1e-5, act, d, None)
            if act == 2 and with_res:
                continue  # (no backward in this form)
            yin, m_in, r_in = A.i(y.clone()), A.i(mean.clone()), A.i(rstd.clone())
            need_y = act == 1 and with_res
            for give_y in ((1,) if need_y else (1, 0)):
                dx, dres, dg, db, ws = A.o(x.shape, dtype), A.o(x.shape, dtype) if with_res else None, A.o(C, F32), A.o(C, F32), A.w(nws)
                L.cot_bn_act_backward(P(dy), P(x), P(yin) if give_y else None, P(dx), P(dres), P(gamma), P(beta), P(m_in), P(r_in), P(dg), P(db),
                                      P(ws), N, C, HW, act, d, None)
            # stochastic depth folded in
            mean, rstd, rm, rv, nbt, ws = stats()
            y = A.o(x.shape, dtype)
            L.cot_bn_act_forward_ps(P(x), P(r), P(y), P(gamma), P(beta), P(mean), P(rstd), P(rm), P(rv), P(nbt), P(ws), P(ps), N, C, HW, 1e-5,
                                    0.1, act, d, None)
            if act != 2:
                yin, m_in, r_in = A.i(y.clone()), A.i(mean.clone()), A.i(rstd.clone())
                dx, dres, dg, db, ws = A.o(x.shape, dtype), A.o(x.shape, dtype) if with_res else None, A.o(C, F32), A.o(C, F32), A.w(nws)
                L.cot_bn_act_backward_ps(P(dy), P(x), P(yin), P(dx), P(dres), P(gamma), P(beta), P(m_in), P(r_in), P(dg), P(db), P(ws), P(ps), N,
                                         C, HW, act, d, None)
            if act == 1 and with_res and nb:
                for with_ps in (0, 1):
                    mean, rstd, rm, rv, nbt, ws = stats()
                    y, mask = A.o(x.shape, dtype), A.o(nb, torch.uint8)
                    L.cot_bn_act_forward_mask(P(x), P(r), P(y), P(mask), P(gamma), P(beta), P(mean), P(rstd), P(rm), P(rv), P(nbt), P(ws),
                                              P(ps) if with_ps else None, N, C, HW, 1e-5, 0.1, 1, d, None)
                    mk, m_in, r_in = A.i(mask.clone()), A.i(mean.clone()), A.i(rstd.clone())
                    for with_dres in (1, 0):
                        dx, dres, dg, db, ws = A.o(x.shape, dtype), A.o(x.shape, dtype) if with_dres else None, A.o(C, F32), A.o(C, F32), A.w(nws)
                        L.cot_bn_act_backward_mask(P(dy), P(x), P(mk), P(dx), P(dres), P(gamma), P(beta), P(m_in), P(r_in), P(dg), P(db), P(ws),
                                                   P(ps) if with_ps else None, N, C, HW, 1, d, None)


def case_bn_lay(L, A, N, C, HW, act, with_res, two, with_ps, every):
    """cot_bn_act_*_lay at the lay bit combinations of tests/layout_cases.py (every: all of them; else those with all tensors alike)"""
    g = _gen(N, C, HW, act, with_res)
    assert L.cot_bn_act_lay_covers(N, C, HW, BF) == 1
    both = lambda t: (A.i(t), A.i(_cm(t)))  # noqa: E731
    hx = _rn(g, N, C, HW, scale=1.5, shift=0.3)
    x, res, dy, dy2 = both(hx), both(_rn(g, N, C, HW)), both(_rn(g, N, C, HW)), both(_rn(g, N, C, HW))
    gamma, beta = A.i(torch.rand(C, generator=g) + 0.5), A.i(0.2 * torch.randn(C, generator=g))
    ps = A.i((torch.rand(N, generator=g) < 0.7).float() / 0.7) if with_ps else None
    pick = lambda bits: every or len(set(bits)) == 1 or sum(bits) == 1  # noqa: E731
    last_by = 0
    for bits in itertools.product((0, 1), repeat=4):
        bx, br, by, by2 = bits
        if (not with_res and br) or (not two and by2) or not pick(bits):
            continue
        last_by = by
        mean, rstd = A.o(C, F32), A.o(C, F32)
        rm, rv, nbt = A.io(torch.zeros(C)), A.io(torch.ones(C)), A.io(torch.zeros((), dtype=torch.int64))
        y, y2 = A.o(hx.shape), A.o(hx.shape) if two else None
        L.cot_bn_act_forward_lay(P(x[bx]), P(res[br]) if with_res else None, P(y), P(y2), P(gamma), P(beta), P(mean), P(rstd), P(rm), P(rv),
                                 P(nbt), P(ps), N, C, HW, 1e-5, 0.1, act, bx | (br << 1) | (by << 2) | (by2 << 3), BF, None)
    if act == 2:
        return
    m_in, r_in = A.i(mean.clone()), A.i(rstd.clone())
    hy = y.clone().view(C, N, HW).transpose(0, 1).contiguous() if last_by else y.clone()  # (the last call's output, NCHW)
    ysave = both(hy) if (with_res and act == 1) else None
    for bits in itertools.product((0, 1), repeat=6):
        bdy, bdy2, bx, by, bdx, bdr = bits
        if (not two and bdy2) or (ysave is None and by) or (not with_res and bdr) or not pick(bits):
            continue
        dx, dres, dg, db = A.o(hx.shape), A.o(hx.shape) if with_res else None, A.o(C, F32), A.o(C, F32)
        L.cot_bn_act_backward_lay(P(dy[bdy]), P(dy2[bdy2]) if two else None, P(x[bx]), P(ysave[by]) if ysave is not None else None, P(dx),
                                  P(dres), P(gamma), P(beta), P(m_in), P(r_in), P(dg), P(db), P(ps), N, C, HW, act,
                                  bdy | (bdy2 << 1) | (bx << 2) | (by << 3) | (bdx << 4) | (bdr << 5), BF, None)


# ---------------------------------------------------------------------------------------------------------------- input, loss, score, EMA

_MEAN, _STD = torch.tensor([123.675, 116.28, 103.53, 99.0]), torch.tensor([58.395, 57.12, 57.375, 50.0])


def _mix_block(mode, lam, box=(0, 0, 0, 0)):
    blk = torch.zeros(8, dtype=torch.int32)
    blk[0] = mode
    blk[1:3] = torch.tensor([lam, 1.0 - lam], dtype=torch.float64).float().view(torch.int32)
    blk[3:7] = torch.tensor(box, dtype=torch.int32)
    return blk


def case_input(L, A, N, C, H, W):
    """cot_input_normalize and cot_mix_normalize (none / mixup / CutMix), the three output types; the parameter block 4-byte aligned"""
    g = _gen(N, C, H, W)
    x = A.i(torch.randint(0, 256, (N, C, H, W), dtype=torch.uint8, generator=g))
    for dtype in (F32, BF16, F16):
        m, s = (_MEAN[:C].half().float(), _STD[:C].half().float()) if dtype == F16 else (_MEAN[:C], _STD[:C])
        m, s = A.i(m.clone()), A.i(s.clone())
        y = A.o(x.shape, dtype)
        L.cot_input_normalize(P(x), P(y), P(m), P(s), N * C, C, H * W, dt(dtype), None)
        if N % 2:
            continue
        for blk in (_mix_block(0, 1.0), _mix_block(1, 0.3), _mix_block(2, 0.6, (H // 3, H, 0, max(W // 2, 1)))):
            params = A.i(blk, align=4)
            y = A.o(x.shape, dtype)
            L.cot_mix_normalize(P(x), P(y), P(m), P(s), P(params), N, C, H, W, dt(dtype), None)


def case_loss(L, A, N, K, dtype):
    """cot_soft_target_ce_* and cot_eval_score; the parameter block 4-byte, the accumulator block 8-byte aligned"""
    g, d = _gen(N, K), dt(dtype)
    logits = A.i(_rn(g, N, K, dtype=dtype, scale=3.0), plane=K, row=K)
    labels = A.i(torch.randint(0, K, (N,), generator=g))
    params = A.i(_mix_block(1, 0.35), align=4)
    gout = A.i(torch.tensor([0.5]))
    rows, lse, mean = A.o(N, F32), A.w(16 * N), A.o(1, F32)
    L.cot_soft_target_ce_forward(P(logits), P(labels), P(params), 0.1, P(rows), P(lse), P(mean), N, K, d, None)
    dl = A.o((N, K), dtype, plane=K, row=K)
    L.cot_soft_target_ce_backward(P(logits), P(labels), P(params), 0.1, P(lse), P(gout), P(dl), N, K, d, None)
    lab = labels.clone()
    lab[-1] = -1 if N > 1 else lab[-1]  # (a padded batch's tail: skipped)
    lab = A.i(lab.cpu())
    for with_rows in (1, 0):
        acc = A.io(torch.zeros(4, dtype=torch.int64), align=8)
        rank, nll = (A.o(N, torch.int32), A.o(N, F32)) if with_rows else (None, None)
        L.cot_eval_score(P(logits), P(lab), P(acc), P(rank), P(nll), N, K, d, None)


def case_ema(L, A, n, dtype):
    g = _gen(n)
    ema, src = A.io(_rn(g, n, dtype=F32)), A.i(_rn(g, n, dtype=dtype))
    L.cot_ema_step(P(ema), P(src), n, 0.999, dt(dtype), None)


# ---------------------------------------------------------------------------------------------------------------- the list

def _both(fn, shapes, *rest):
    return [(fn, s + (dtype,) + rest) for s in shapes for dtype in (BF16, F32)]


# the plane kernels' edges: HW = 1; 45 (5 x 9: scalar loads); 49 with N * C = 24 and 35 (packed 7 x 7 form, last wave partly dead); 196; 576;
# N in {1, 3, 9} (the prologue's loop over N has a tail when 8 lanes share a plane)
_PLANES = [(9, 2, 1, 1), (9, 4, 5, 9), (3, 8, 7, 7), (5, 7, 7, 7), (1, 6, 14, 14), (3, 2, 24, 24)]
CASES = {
    "agg": _both(case_agg, [(2, 16, 6, 56), (8, 64, 7, 7), (8, 8, 3, 10)]) + [(case_agg_generic, (dtype, lay)) for dtype in (BF16, F32) for lay in (0, 1)],
    "agg_gn9_rowstats": [(case_agg_gn9, s) for s in [(2, 16, 20, 20), (3, 64, 7, 7), (1, 128, 5, 8)]],
    "aggmix": _both(case_aggmix, [(2, 8, 4, 10, 6, 2), (1, 6, 2, 4, 7, 1)]),
    # HW = 196 (a 128-pixel tile + a ragged one), 400 (the > 256 form), 1 x 80 flat; reduction depths 64 / 40 / 24; Co = 72 / 40; two slabs
    # split at 8 and at 32; one image on the staging-free kernels; fp32 (general kernels)
    "conv1x1": [(case_conv1x1, s) for s in [(3, 64, 72, 14, 14, 32), (1, 64, 40, 20, 20, 0), (1, 96, 136, 1, 80, 0), (2, 40, 24, 6, 6, 0),
                                            (8, 24, 16, 7, 7, 8), (1, 16, 8, 3, 8, 0), (2, 64, 72, 20, 20, 8)]]
    + [(case_conv1x1, (2, 20, 12, 5, 5, 0, F32)), (case_conv1x1, (1, 7, 9, 14, 14, 0, F32))],
    "conv1x1_epilogues": [(case_conv1x1_epilogues, s) for s in [(2, 64, 72, 20, 20, 0), (1, 64, 72, 24, 24, 32)]]
    + [(case_relu_res, s) for s in [(5, 128, 64, 64), (20, 64, 32, 16), (1, 96, 64, 392)]],
    "conv1x1g": _both(case_conv1x1g, [(2, 128, 96, 2, 8, 8), (2, 48, 108, 2, 4, 6), (1, 16, 8, 2, 1, 8)]),
    "conv3x3": [(case_conv3x3, s) for s in [(1, 128, 4, 30, 20), (3, 256, 4, 7, 7), (1, 96, 2, 24, 16), (2, 96, 8, 6, 10), (2, 64, 4, 8, 16)]],
    # the general-kernel route of the same entry points: fp32, channel counts off the grid
    "conv3x3_general": [(case_conv3x3, s) for s in [(2, 16, 4, 4, 4, F32), (1, 15, 3, 5, 7, F32), (2, 72, 1, 2, 2, F32), (1, 20, 1, 6, 5, BF16)]],
    "stem7x7": _both(case_stem7, [(2, 32, 32), (1, 16, 64)]),
    "stem3x3": [(case_stem3, s) for s in [(2, 32, 32, 32), (1, 16, 64, 64), (1, 17, 23, 32), (1, 15, 63, 64)]],
    "pools": _both(case_pools, _PLANES + [(2, 3, 2, 2), (1, 5, 6, 10)]),
    "tail": _both(case_tail, _PLANES),
    "tail_lay": [(case_tail_lay, s + (k50,)) for s in [(3, 8, 7, 7), (5, 7, 7, 7), (9, 4, 5, 9), (1, 6, 14, 14)] for k50 in (1, 0)],
    "tail_bn": [(case_tail_bn, s + (dtype, lay_k, sums)) for s in [(3, 8, 7, 7), (9, 4, 5, 9), (1, 6, 14, 14), (5, 7, 7, 7)]
                for dtype in (BF16, F32) for lay_k in (0, 1) for sums in (0, 1)],
    "gn9": _both(case_gn9, [(2, 2, 8, 8), (8, 2, 7, 7), (9, 2, 5, 9), (3, 1, 1, 1), (1, 1, 24, 24), (3, 3, 14, 14)]) + [(case_gn9, (8, 2, 7, 7, BF16, 0))],
    "bn_streaming": _both(case_bn, [(3, 8, 7, 7), (9, 4, 5, 9), (1, 6, 14, 14), (9, 2, 1, 1), (3, 2, 24, 24)], 0, 1) + [(case_bn, (5, 7, 7, 7, BF16, 0, 0))],
    "bn_channel_resident": _both(case_bn, [(3, 8, 7, 7), (5, 7, 7, 7), (9, 4, 5, 9), (3, 2, 24, 24), (9, 2, 1, 1)], 1, 1) + [(case_bn, (3, 8, 7, 7, BF16, 1, 0))],
    # (the channel-resident kernels' tensors: more than 256 samples per channel)
    "bn_lay": [(case_bn_lay, (6, 4, 49, 1, 1, 1, 1, 1)), (case_bn_lay, (9, 8, 49, 0, 0, 0, 0, 1)), (case_bn_lay, (3, 2, 196, 2, 1, 1, 0, 0)),
               (case_bn_lay, (7, 5, 49, 1, 0, 1, 1, 0)), (case_bn_lay, (2, 4, 576, 0, 1, 0, 1, 0))],
    "input": [(case_input, s) for s in [(2, 3, 8, 8), (4, 3, 5, 9), (2, 1, 1, 1), (1, 3, 7, 7)]],
    "loss_score_ema": _both(case_loss, [(1, 1000), (5, 1000), (1, 7), (5, 7)]) + _both(case_ema, [(1,), (4097,)]),
}

# entry points the cases do not call, each with its reason: it launches nothing, or its margins and sentinels are pinned elsewhere
_QUERY = "a size, cover or version query: launches nothing"
_DEV = "a tuning, profiling or logging call: launches nothing on operands"
EXEMPT = {
    "cot_abi_version": _QUERY, "cot_last_error": _QUERY, "cot_last_kernel": _QUERY, "cot_status_string": _QUERY,
    "cot_local_relation_workspace_bytes": _QUERY, "cot_gn9_stats_floats": _QUERY, "cot_gn9_fused_covers": _QUERY,
    "cot_stem7x7s2_workspace": _QUERY, "cot_stem3x3s2_workspace": _QUERY, "cot_grad_norm_parts": _QUERY, "cot_agc_max_groups": _QUERY,
    "cot_conv1x1_workspace": _QUERY, "cot_conv1x1_backward_data_relu_res_covers": _QUERY, "cot_conv3x3g_masks_bytes": _QUERY,
    "cot_conv3x3g_workspace": _QUERY, "cot_conv3x3g_packed_bytes": _QUERY, "cot_convg_workspace": _QUERY, "cot_conv1x1_lds_covers": _QUERY,
    "cot_bn_act_workspace": _QUERY, "cot_bn_relu_mask_bytes": _QUERY, "cot_conv1x1_stats_covers": _QUERY, "cot_bn_act_lay_covers": _QUERY,
    "cot_agg_rowstats_floats": _QUERY, "cot_agg_out_size": _QUERY,
    "cot_set_tuning": _DEV, "cot_get_tuning": _DEV, "cot_reset_tuning": _DEV, "cot_tuning_name": _DEV, "cot_xchg_mode": _DEV + " (a 64-thread probe on library-owned memory)", "cot_launch_log": _DEV,
    "cot_profile_begin": _DEV, "cot_profile_end": _DEV,
    "cot_local_relation_forward": "operands and outputs inside NaN margins, output margins checked: tests/test_fuzz_emulated.py case_local_relation (tests/test_fuzz_gpu.py on the device)",
    "cot_local_relation_backward": "operands and outputs inside NaN margins, output margins checked: tests/test_fuzz_emulated.py case_local_relation (tests/test_fuzz_gpu.py on the device)",
    "cot_sgd_step": "NaN margins and sentinel words: tests/sgd_lr_cases.py",
    "cot_sgd_step_lr": "NaN margins and sentinel words: tests/sgd_lr_cases.py",
    "cot_grad_sumsq": "NaN margins and sentinel words: tests/grad_clip_cases.py",
    "cot_grad_clip_finish": "NaN margins and sentinel words: tests/grad_clip_cases.py",
    "cot_sgd_step_clip": "NaN margins and sentinel words: tests/grad_clip_cases.py",
    "cot_agc_clip": "NaN margins and sentinel words: tests/agc_cases.py",
    "cot_adam_tick": "NaN margins and sentinel words: tests/adamw_cases.py",
    "cot_adamw_step": "NaN margins and sentinel words: tests/adamw_cases.py",
    "cot_lookahead_tick": "NaN margins and sentinel words: tests/lookahead_cases.py",
    "cot_lookahead_step": "NaN margins and sentinel words: tests/lookahead_cases.py",
}


def uncovered(names, exported=None):
    """the entry points of _lib.SYMBOLS (those `exported` has, when given) that no case called and EXEMPT does not explain"""
    return sorted(n for n in _lib.SYMBOLS if n not in names and n not in EXEMPT and (exported is None or hasattr(exported, n)))
