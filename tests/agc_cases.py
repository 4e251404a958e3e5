"""Adaptive gradient clipping on the device (csrc/agc.hip: cot_agc_clip): the cases and criteria that tests/test_agc_emulated.py runs on
the host emulator and tests/test_agc_gpu.py on the device.

The bounds are DERIVED, not measured.  Every term of a sum of squares is >= 0, so the relative error of an fp32 sum is at most
(d + 1) * u, u = 2^-24, where d = agc_chain_length(start, len, V) is the longest chain of fp32 additions one square passes through (the
order stated at the top of agc.hip) and the + 1 is the square's own rounding; the square root halves it, and the root's own rounding and
the slack of the halving are covered by + 2:

    |norm - ref| <= ((d + 1) / 2 + 2) * u * ref,    ref = sqrt(sum(x.double() ** 2)) of the stored values

    coef    within norm_bound(weight, V = 4) + norm_bound(grad, V of its dtype) + 3 u of max_norm / gn in fp64: one u each for the
            maximum with eps, the multiply by the factor and the divide
    g'      a clipped element within that plus half a unit in the last place of the gradient's dtype (2^-24 fp32, 2^-8 bf16) of
            g * coef_ref in fp64.  (The maximum is exact; its u is what covers the fp32 rounding of the product in front of the
            rounding to bf16.)

`gn < max_norm` compares two rounded numbers, so only DECIDED units are judged: those whose fp64 ratio gn / max_norm is further from 1
than twice the coefficient bound.  Every case here places each unit at a ratio in RATIOS by scaling the unit's gradient, and asserts
that nothing is left undecided.

A case is one bucket: parameter shapes laid out as FlatSGD's buckets are (every slot starts on a 16-byte boundary of the narrower
operand), the padding between the slots filled with NaN in both operands -- it may neither reach a norm nor be written -- and all
operands inside NaN margins (tests/sgd_lr_cases.py), which must stay NaN."""
import ctypes
import math
import os

import numpy as np
import torch

from cotnet_amd import _lib
from tests import sgd_lr_cases as sgd

P = sgd.P
U = 2.0 ** -24
GRAD_DTYPES = [torch.float32, torch.bfloat16]
GRAD_IDS = ["f32", "bf16"]
HALF_ULP = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "agc.npz")
FACTOR, EPS = 0.01, 1e-3
FACTOR32, EPS32, FLOOR32 = float(np.float32(FACTOR)), float(np.float32(EPS)), float(np.float32(1e-6))  # what the kernel receives and holds
RATIOS = [0.25, 0.8, 1.25, 4.0]  # gn / max_norm a unit is placed at: two that do not clip, two that do
LENGTHS = [1, 3, 7, 8, 9, 63, 64, 65, 147, 511, 512, 513, 2048, 4099]


def vec(dt):
    """elements per 16 bytes"""
    return 16 // torch.empty((), dtype=dt).element_size()


def agc_chain_length(start, length, V):
    """the longest chain of fp32 additions a square passes through (agc.hip, "The chain")"""
    head = min(length, (-start) % V)
    nvec = (length - head) // V
    return -(-nvec // (64 * 4)) + 2 + int(math.log2(V)) + 2 + 6  # a lane's adds, the four sets, the slots, head and tail, the wave's stages


def norm_bound(start, length, V):
    """relative; see the module docstring"""
    return ((agc_chain_length(start, length, V) + 1) / 2 + 2) * U


def coef_bounds(units, gdt):
    """float64 [units]: the coefficient's relative bound per unit"""
    V = vec(gdt)
    return torch.tensor([norm_bound(s, n, 4) + norm_bound(s, n, V) + 3 * U for s, n in units.tolist()], dtype=torch.float64)


def layout(shapes, align):
    """(units int64 [U, 2], n): the reference's unitwise_norm over parameter slots that each start on a multiple of `align` elements --
    a parameter with ndim <= 1 is one unit, any other is shape[0] units of numel / shape[0] consecutive elements"""
    units, off = [], 0
    for shape in shapes:
        numel = int(np.prod(shape))
        if len(shape) <= 1:
            units.append((off, numel))
        else:
            per = numel // shape[0]
            units += [(off + r * per, per) for r in range(shape[0])]
        off += -(-numel // align) * align
    return torch.tensor(units, dtype=torch.int64), off


def cases(L):
    """{name: parameter shapes}"""
    many = 4 * L.cot_agc_max_groups() + 5  # a wave takes a second unit
    return {
        "lengths": [(n,) for n in LENGTHS],
        # rows of 147 and of 13 elements: starts at every phase of a 16-byte granule, of 4 floats and of 8 bf16 alike
        "rows-147": [(6, 147), (8, 13)],
        "padding": [(3, 5), (7,), (2, 3, 3), (1,), (5, 2, 1, 1)],
        "many-units": [(many, 3)],
        "single-unit": [(37,)],
    }


def expand(units):
    """(element index, unit index) of every element that belongs to a unit"""
    starts, lens = units[:, 0], units[:, 1]
    unit_of = torch.repeat_interleave(torch.arange(units.shape[0]), lens)
    first = torch.cumsum(lens, 0) - lens
    return starts[unit_of] + (torch.arange(int(lens.sum())) - first[unit_of]), unit_of


def unit_norms(x, units):
    """fp64 norm per unit of the stored values"""
    idx, unit_of = expand(units)
    return torch.zeros(units.shape[0], dtype=torch.float64).index_add_(0, unit_of, x[idx].double().square()).sqrt()


def reference(w, g, units):
    """the formula in fp64 on the stored values: dict(max_norm, gn, ratio, coef) per unit"""
    wn, gn = unit_norms(w, units), unit_norms(g, units)
    max_norm = wn.clamp(min=EPS32) * FACTOR32
    coef = torch.where(gn < max_norm, torch.ones_like(gn), max_norm / gn.clamp(min=FLOOR32))
    return dict(wn=wn, gn=gn, max_norm=max_norm, ratio=gn / max_norm, coef=coef)


def build(shapes, gdt, seed=0, weights=None, ratios=RATIOS):
    """CPU operands of one bucket: dict(w fp32 [n], g gdt [n], units, n).  Unit i's gradient is scaled to RATIOS[i % 4] times its
    max_norm; `weights(w, units)` may rewrite the weights first; the padding is NaN in both."""
    units, n = layout(shapes, vec(gdt))
    rng = torch.Generator().manual_seed(7000 + seed)
    w = torch.randn(n, generator=rng)
    g = torch.randn(n, generator=rng, dtype=torch.float64)
    if weights is not None:
        weights(w, units)
    idx, unit_of = expand(units)
    max_norm = unit_norms(w, units).clamp(min=EPS32) * FACTOR32
    want = torch.tensor(ratios, dtype=torch.float64)[torch.arange(units.shape[0]) % len(ratios)] * max_norm
    g[idx] *= (want / unit_norms(g, units))[unit_of]
    pad = torch.ones(n, dtype=torch.bool)
    pad[idx] = False
    w[pad] = float("nan")
    g[pad] = float("nan")
    return dict(w=w, g=g.to(gdt), units=units, n=n)


def decided(ref, bounds):
    return (ref["ratio"] - 1).abs() > 2 * bounds


def device_table(units, dev):
    """(buffer, view): the table between two sentinel pairs (-1, -1) -- a wave that read one would find a unit without elements"""
    buf = torch.full((units.numel() + 4,), -1, dtype=torch.int64)
    buf[2:-2] = units.reshape(-1)
    buf = buf.to(dev)
    return buf, buf[2:-2]


def run(L, dev, stream, ops, sync=lambda: None, factor=FACTOR, eps=EPS):
    """one cot_agc_clip on fresh device copies; returns the buffers (on the CPU) after the call"""
    wbuf, wv = sgd.margined(ops["w"].to(dev))
    gbuf, gv = sgd.margined(ops["g"].to(dev))
    tbuf, tv = device_table(ops["units"], dev)
    nunits = ops["units"].shape[0]
    cbuf, cv = sgd.margined(torch.full((nunits,), float("nan"), dtype=torch.float32, device=dev))  # every entry has to be written
    rc = L.cot_agc_clip(P(gv), P(wv), P(tv), nunits, ops["n"], factor, eps, P(cv), _lib.dtype_code(gv.dtype), stream)
    assert rc == 0, L.cot_last_error()
    sync()
    m = sgd.MARGIN
    out = dict(wbuf=wbuf.cpu(), gbuf=gbuf.cpu(), tbuf=tbuf.cpu(), cbuf=cbuf.cpu())
    out.update(g=out["gbuf"][m:-m], coef=out["cbuf"][m:-m])
    return out


def operands_untouched(ops, out, what):
    """the weights, the table, every margin, and the padding of the gradient"""
    assert sgd.same_bits(out["wbuf"], sgd.margined(ops["w"])[0]), f"the weights were written ({what})"
    assert torch.equal(out["tbuf"], device_table(ops["units"], "cpu")[0]), f"the table was written ({what})"
    assert sgd.margins_intact(out["gbuf"]) and sgd.margins_intact(out["cbuf"]), f"a NaN margin was written ({what})"
    idx, _ = expand(ops["units"])
    pad = torch.ones(ops["n"], dtype=torch.bool)
    pad[idx] = False
    assert bool(torch.isnan(out["g"][pad]).all()), f"the padding between the slots was written ({what})"


def check_units(ops, out, ref, bounds, gdt, what, skip=()):
    """coefficients and gradients of every unit not in `skip` against the fp64 formula; returns the worst observed errors relative to
    their bounds"""
    units = ops["units"]
    keep = torch.ones(units.shape[0], dtype=torch.bool)
    if skip:
        keep[list(skip)] = False
    coef = out["coef"].double()
    clips = ref["coef"] < 1
    assert bool((out["coef"][keep & ~clips] == 1.0).all()), f"an unclipped unit's coefficient is not exactly 1 ({what})"
    cerr = ((coef - ref["coef"]).abs() / ref["coef"])[keep & clips]
    assert bool((cerr <= bounds[keep & clips]).all()), (what, float(cerr.max()), "coefficient outside its bound")
    idx, unit_of = expand(units)
    before, after = ops["g"][idx], out["g"][idx]
    it = {2: torch.int16, 4: torch.int32}[before.element_size()]
    same = before.view(it) == after.view(it)
    e_keep, e_clip = keep[unit_of], clips[unit_of]
    assert bool(same[e_keep & ~e_clip].all()), f"an unclipped unit's gradient bits changed ({what})"
    want = before.double() * ref["coef"][unit_of]
    tol = (1 + bounds[unit_of]) * (1 + HALF_ULP[gdt]) - 1
    sel = e_keep & e_clip
    gerr = (after.double() - want).abs()[sel] / want.abs()[sel].clamp_min(1e-300)
    assert bool((gerr <= tol[sel]).all()), (what, float((gerr / tol[sel]).max()), "clipped element outside its bound")
    return (float((cerr / bounds[keep & clips]).max()) if cerr.numel() else 0.0,
            float((gerr / tol[sel]).max()) if gerr.numel() else 0.0)


def check_case(L, dev, stream, name, gdt, sync=lambda: None):
    """coefficients and clipped elements within the derived bounds, unclipped units bit for bit, two calls equal bits, nothing but the
    coefficients and the clipped units written"""
    ops = build(cases(L)[name], gdt, ratios=[4.0] if name == "single-unit" else RATIOS)  # (the one unit clips: the path that writes)
    bounds = coef_bounds(ops["units"], gdt)
    assert float(bounds.max()) < 2e-6, (name, float(bounds.max()))  # else the order of additions is too serial
    ref = reference(ops["w"], ops["g"], ops["units"])
    assert int((~decided(ref, bounds)).sum()) == 0
    nunits = ops["units"].shape[0]
    assert 0 < int((ref["coef"] < 1).sum()) < nunits or (nunits == 1 and float(ref["coef"][0]) < 1)
    what = f"{name}, {gdt}"
    out, again = run(L, dev, stream, ops, sync), run(L, dev, stream, ops, sync)
    assert sgd.same_bits(out["gbuf"], again["gbuf"]) and sgd.same_bits(out["cbuf"], again["cbuf"]), f"two calls on equal data differ ({what})"
    operands_untouched(ops, out, what)
    assert bool(torch.isfinite(out["coef"]).all()), f"a coefficient left unwritten ({what})"
    worst = check_units(ops, out, ref, bounds, gdt, what)
    print(f"{what}: {nunits} units, {int((ref['coef'] < 1).sum())} clip; worst coefficient error {worst[0]:.2f} of its bound "
          f"(largest bound {float(bounds.max()):.3e}), worst element error {worst[1]:.2f} of its bound")


def check_eps_floor(L, dev, stream, gdt, sync=lambda: None):
    """units with wn = 0 and wn = eps / 2 clip against eps * factor; so does a unit with wn a little above eps against its own norm"""
    def weights(w, units):
        fill = [0.0, EPS / 4, 0.0, EPS / 8, 0.0, EPS / 2, 0.0, 2 * EPS]  # lengths 5 4 9 16 1 1 3 7: wn = 0, eps/2, 0, eps/2, 0, eps/2, 0, > eps
        for (s, n), v in zip(units.tolist(), fill):
            w[s:s + n] = v
    ops = build([(5,), (4,), (9,), (16,), (1,), (1,), (3,), (7,)], gdt, seed=1, weights=weights)
    ref = reference(ops["w"], ops["g"], ops["units"])
    floor = torch.full((7,), EPS32 * FACTOR32, dtype=torch.float64)
    assert torch.allclose(ref["max_norm"][:7], floor, rtol=1e-12, atol=0) and float(ref["max_norm"][7]) > 2 * float(floor[0])
    assert bool((ref["wn"][[1, 3, 5]] - EPS / 2).abs().max() < 1e-9) and bool((ref["wn"][[0, 2, 4, 6]] == 0).all())
    bounds = coef_bounds(ops["units"], gdt)
    assert int((~decided(ref, bounds)).sum()) == 0
    out = run(L, dev, stream, ops, sync)
    operands_untouched(ops, out, f"eps floor, {gdt}")
    check_units(ops, out, ref, bounds, gdt, f"eps floor, {gdt}")
    assert (out["coef"] < 1).tolist() == [False, False, True, True] * 2


def check_zero_gradient(L, dev, stream, gdt, sync=lambda: None):
    """gn = 0 < max_norm: coef = 1 exactly and nothing written -- also where the weights are zero too"""
    def weights(w, units):
        s, n = units[3].tolist()
        w[s:s + n] = 0.0
    ops = build([(9,), (4, 6), (11,)], gdt, seed=2, weights=weights)
    for i in (1, 3, 5):
        s, n = ops["units"][i].tolist()
        ops["g"][s:s + n] = 0.0
    out = run(L, dev, stream, ops, sync)
    operands_untouched(ops, out, f"zero gradient, {gdt}")
    assert bool((out["coef"][[1, 3, 5]] == 1.0).all()), out["coef"]
    bounds = coef_bounds(ops["units"], gdt)
    check_units(ops, out, reference(ops["w"], ops["g"], ops["units"]), bounds, gdt, f"zero gradient, {gdt}")


NONFINITE = ["inf-gradient", "nan-gradient", "bf16-overflowing-squares", "nan-weight"]


def check_nonfinite(L, dev, stream, kind, gdt, sync=lambda: None):
    """ordinary arithmetic on an inf, a NaN or bf16 values whose squares overflow fp32, in ONE unit: that unit gets coef = NaN and keeps
    its gradient bits, every other unit is as in the finite run"""
    ops = build(cases(L)["rows-147"], gdt, seed=3)
    clean = run(L, dev, stream, ops, sync)
    bad = 3  # a row of 147 that starts off the 16-byte boundaries of both operands; placed at RATIOS[3]: the finite run clips it
    s, n = ops["units"][bad].tolist()
    planted = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in ops.items()}
    if kind == "inf-gradient":
        planted["g"][s + 1] = float("inf")
    elif kind == "nan-gradient":
        planted["g"][s + n - 1] = float("nan")
    elif kind == "nan-weight":
        planted["w"][s + 70] = float("nan")
    else:
        assert gdt == torch.bfloat16
        planted["g"][s:s + 3] = 3e38  # finite elements whose squares overflow fp32
        assert bool(torch.isfinite(planted["g"][s:s + n]).all())
    out = run(L, dev, stream, planted, sync)
    what = f"{kind}, {gdt}"
    operands_untouched(planted, out, what)
    assert math.isnan(float(out["coef"][bad])), (what, float(out["coef"][bad]))
    assert sgd.same_bits(out["g"][s:s + n], planted["g"][s:s + n]), f"the marked unit's gradient was written ({what})"
    others = torch.ones(ops["units"].shape[0], dtype=torch.bool)
    others[bad] = False
    assert sgd.same_bits(out["coef"][others], clean["coef"][others]), f"another unit's coefficient moved ({what})"
    elems = torch.ones(ops["n"], dtype=torch.bool)
    elems[s:s + n] = False
    assert sgd.same_bits(out["g"][elems], clean["g"][elems]), f"another unit's gradient differs from the finite run ({what})"
    assert int((clean["coef"] < 1).sum()) > 0 and bool(torch.isfinite(clean["coef"]).all())


def check_fixture(L, dev, stream, sync=lambda: None):
    """the reference's dispatch_clip_grad(params, 0.01, mode='agc') as recorded (tests/golden/make_golden_agc.py): its four tensors as ONE
    bucket; the gradients it left within the clipped-element bound plus one fp32 rounding, and bit for bit where it left a unit alone"""
    fix = np.load(GOLDEN)
    k = len([f for f in fix.files if f.startswith("w")])
    ws, gs, outs = ([torch.from_numpy(fix[f"{p}{i}"]) for i in range(k)] for p in ("w", "g", "out"))
    gdt = torch.float32
    units, n = layout([tuple(w.shape) for w in ws], vec(gdt))
    w, g, want = (torch.full((n,), float("nan")) for _ in range(3))
    off = 0
    for wi, gi, oi in zip(ws, gs, outs):
        for flat, t in ((w, wi), (g, gi), (want, oi)):
            flat[off:off + t.numel()] = t.reshape(-1)
        off += -(-wi.numel() // vec(gdt)) * vec(gdt)
    ops = dict(w=w, g=g, units=units, n=n)
    ref = reference(w, g, units)
    bounds = coef_bounds(units, gdt)
    assert int((~decided(ref, bounds)).sum()) == 0
    out = run(L, dev, stream, ops, sync)
    operands_untouched(ops, out, "fixture")
    idx, unit_of = expand(units)
    left_alone = torch.ones(units.shape[0], dtype=torch.bool)
    left_alone[unit_of[g[idx] != want[idx]]] = False  # (the reference's torch.where hands such a unit's gradient through)
    assert torch.equal(left_alone, ref["coef"] == 1) and 0 < int(left_alone.sum()) < units.shape[0]
    got, exp = out["g"][idx], want[idx]
    assert torch.equal(got[left_alone[unit_of]], exp[left_alone[unit_of]]), "a unit the reference left alone differs in its bits"
    tol = (1 + bounds[unit_of]) * (1 + HALF_ULP[gdt]) - 1 + U
    err = (got.double() - exp.double()).abs() / exp.double().abs().clamp_min(1e-300)
    err[exp == got] = 0.0
    print(f"fixture: {units.shape[0]} units, {int((~left_alone).sum())} clipped by the reference; worst element error "
          f"{float((err / tol).max()):.2f} of its allowance (largest allowance {float(tol.max()):.3e})")
    assert bool((err <= tol).all()), float((err / tol).max())


def check_refusals(L, dev, stream, sync=lambda: None):
    """each refused with its message before any device work: the operands, the table and the coefficients stay as they were"""
    gdt = torch.bfloat16
    ops = build([(3, 5), (7,)], gdt, seed=4)
    nunits, n = ops["units"].shape[0], ops["n"]
    wbuf, wv = sgd.margined(ops["w"].to(dev))
    gbuf, gv = sgd.margined(ops["g"].to(dev))
    tbuf, tv = device_table(ops["units"], dev)
    cbuf, cv = sgd.margined(torch.full((nunits,), float("nan"), dtype=torch.float32, device=dev))
    keep = [b.clone() for b in (wbuf, gbuf, tbuf)]

    def untouched():
        sync()
        return (sgd.same_bits(wbuf, keep[0]) and sgd.same_bits(gbuf, keep[1]) and torch.equal(tbuf, keep[2])
                and bool(torch.isnan(cbuf).all()))

    def refused(rc, message, status=-1):
        assert rc == status, (rc, L.cot_last_error())
        assert message in L.cot_last_error(), L.cot_last_error()
        assert untouched(), message

    def odd(t, by):
        return ctypes.c_void_p(t.data_ptr() + by)

    code = _lib.dtype_code(gdt)
    good = [P(gv), P(wv), P(tv), nunits, n, FACTOR, EPS, P(cv), code, stream]

    def call(**kw):
        names = ["grad", "weight", "units", "nunits", "n", "factor", "eps", "coef", "dtype", "stream"]
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        return L.cot_agc_clip(*a)

    refused(call(grad=None), b"NULL device pointer")
    refused(call(weight=None), b"NULL device pointer")
    refused(call(units=None), b"NULL units")
    refused(call(coef=None), b"NULL coef")
    refused(call(grad=odd(gv, 2)), b"16-byte")
    refused(call(weight=odd(wv, 4)), b"16-byte")
    refused(call(units=odd(tv, 4)), b"8-byte aligned")
    refused(call(coef=odd(cv, 2)), b"4-byte aligned")
    refused(call(nunits=0), b"unit count")
    refused(call(nunits=-3), b"unit count")
    refused(call(n=0), b"element count")
    for bad in (0.0, -0.01, float("nan"), float("inf"), float("-inf")):
        refused(call(factor=bad), b"clip_factor")
        refused(call(eps=bad), b"eps")
    refused(call(dtype=_lib.dtype_code(torch.float16)), b"dtype", _lib.COT_ERR_UNSUPPORTED)
    refused(call(dtype=_lib.dtype_code(torch.float64)), b"dtype", _lib.COT_ERR_UNSUPPORTED)
    assert call() == 0, L.cot_last_error()  # (the arguments the refusals were variations of are good ones)
    sync()
    assert bool(torch.isfinite(cv).all())
