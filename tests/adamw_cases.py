"""Fused Adam / AdamW on the device (csrc/adamw.hip: cot_adam_tick, cot_adamw_step): the cases and criteria that
tests/test_adamw_emulated.py runs on the host emulator and tests/test_adamw_gpu.py on the device.

The reference of a kernel step is THE FORMULA IN FP64 on the operands as stored and on the hyper-parameters as the caller holds them
(Python doubles).  The bounds are DERIVED, not measured: u = 2^-24, one u on the magnitude of its result for every fp32 operation in
the order stated at the top of adamw.hip (a fused multiply-add rounds once where two operations round twice: never more), one u for every
constant that reaches the kernel as an fp32 value (grad_scale, weight_decay, lr, eps, (float)beta, (float)(1 - beta), bc1, sqrt_bc2), and
errors carried from line to line by the line's own arithmetic.  With |x| the exact magnitudes:

    G  = grad * gs                       E_G  = 2u |G|                                   (the constant, the product)
    g  = G + wd * p   (L2 form)          E_g  = E_G + 2u |wd p| + u |g|                  (decoupled: g = G, E_g = E_G)
    p1 = p * (1 - lr * wd)  (decoupled)  E_p1 = |p| (3u lr wd + u (1 - lr wd)) + u |p1|  (lr, wd, their product; the subtraction; the product)
    m' = m b1 + o1 g                     E_m  = 2u |m b1| + 2u |o1 g| + o1 E_g + u |m'|
    v' = v b2 + (o2 g) g                 E_v  = 2u v b2 + 3u o2 g^2 + o2 (2 |g| E_g + E_g^2) + u v'
    s  = sqrt(v')                        E_s  = E_v / (s + sqrt(max(v' - E_v, 0))) + u s   (|sqrt a - sqrt b| = |a - b| / (sqrt a + sqrt b))
    d  = s / sqrt_bc2 + eps              E_d  = E_s / sqrt_bc2 + 2u s / sqrt_bc2 + u eps + u d
    r  = m' / d                          E_r  = (E_m + |r| E_d) / (d - E_d) + u |r|
    a  = lr / bc1                        E_a  = 3u a                                     (lr, bc1, the division)
    p' = p1 - a r                        E_p  = E_p1 + a E_r + E_a (|r| + E_r) + u |a r| + u |p'|

Each u |x| is taken on the exact |x|, not the computed one; what that leaves out is a product of two roundings, below 2^-20 of the
bound: every bound is multiplied by 1 + 2^-10.  E_m, E_v and E_p judge exp_avg, exp_avg_sq and the fp32 weights (the master, or the
fp32 parameters themselves: E_p's last term IS half a unit in their last place); a bf16 working copy is judged within
E_p + 2^-8 (|p'| + E_p), half a unit in ITS last place.  EVERY element is judged.  So that a sloppy derivation cannot hide a wrong
kernel, each case asserts that its largest E_p stays below 32 u times the operands' magnitude
|p| + a (|m b1| + o1 (|G| + |wd p|)) / d + a |r| sqrt(o2) (|G| + |wd p|) / (sqrt_bc2 d) -- the last term is the gradient's way into the
denominator, which counts where g cancels against wd p and v is small (counting the lines above gives at most ~25 u of it).
Bit-equality with torch is not the criterion: hipcc contracts to FMA.

The recorded fixture (tests/golden/adamw.npz, tests/golden/make_golden_adamw.py) and torch.optim.Adam stepped live are fp32 evaluations
of the same formula on the same doubles, each with its own roundings; they are judged with the same bounds plus one fp32 rounding of
their own result, u |ref|.

Operands sit inside NaN margins (tests/sgd_lr_cases.py) which must stay NaN; the two blocks sit between sentinel words."""
import ctypes
import math
import os

import numpy as np
import torch

from cotnet_amd import _lib
from tests import sgd_lr_cases as sgd

P = sgd.P
U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10
HALF_ULP = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8}  # (fp32: E_p's last term already is the working copy's rounding)
SIZES = sgd.SIZES  # 1, 3, 4, 5, 4003: tail only, body only, body + tail
SECOND_TRIP = 2048 * 256 * 4 + 4 * 256 + 3  # the smallest n at which a lane makes a second trip of the grid-stride loop, tail present
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adamw.npz")
HP = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, wd=0.05, gs=0.5)
STEP = 7  # the step the generic cases run as
SENTINEL = 0x7FC00BAD  # a NaN pattern: the words around a block


def f32(x):
    return float(np.float32(x))


def corrections(b1, b2, step):
    """(bc1, sqrt_bc2) as Python doubles: the reference's arithmetic (adamw.py:99-100, :111)"""
    return 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step)


def adam_block(step, b1, b2, dev, refused=0):
    """(buffer, view): int32[8] = cot_adam_state as `step` ticks leave it, between eight sentinel words on each side"""
    bc1, sbc2 = corrections(b1, b2, step) if step > 0 else (0.0, 0.0)
    buf = torch.full((24,), SENTINEL, dtype=torch.int32)
    buf[8:16] = 0
    buf[8], buf[11] = step, refused
    buf[9:11] = torch.tensor([bc1, sbc2], dtype=torch.float32).view(torch.int32)
    buf = buf.to(dev)
    return buf, buf[8:16]


def clip_block(scale, skip, dev):
    """(buffer, view): int32[8] = cot_clip_state {scale, total_norm 1, skip, steps 5, clipped 2, skipped 1}"""
    buf = torch.full((24,), SENTINEL, dtype=torch.int32)
    buf[8:16] = torch.tensor([0, 0, skip, 5, 2, 1, 0, 0], dtype=torch.int32)
    buf[8:10] = torch.tensor([scale, 1.0], dtype=torch.float32).view(torch.int32)
    buf = buf.to(dev)
    return buf, buf[8:16]


def read_block(view):
    w = view.cpu()
    return dict(step=int(w[0]), bc1=float(w[1:2].view(torch.float32)), sqrt_bc2=float(w[2:3].view(torch.float32)), refused=int(w[3]),
                reserved=w[4:].tolist())


def operands(pdt, gdt, n, dev, seed=0, zero_every=5):
    """{name: (buffer, view)} on `dev`, master None for fp32 parameters; every `zero_every`-th gradient element is exactly 0"""
    g = torch.Generator().manual_seed(9100 + seed + n % 1000)
    master = torch.randn(n, generator=g)
    m = torch.randn(n, generator=g) * 0.1
    v = (torch.randn(n, generator=g) * 0.1).square()
    grad = torch.randn(n, generator=g)
    if zero_every:
        grad[::zero_every] = 0.0
    return {"param": sgd.margined(master.to(pdt).to(dev)), "m": sgd.margined(m.to(dev)), "v": sgd.margined(v.to(dev)),
            "grad": sgd.margined(grad.to(gdt).to(dev)), "master": sgd.margined(master.to(dev)) if pdt != torch.float32 else None}


def views(ops):
    return {k: (x[1] if x is not None else None) for k, x in ops.items()}


def buffers_cpu(ops):
    return {k: (x[0].cpu().clone() if x is not None else None) for k, x in ops.items()}


def same(a, b):
    """two buffers_cpu() results equal bit for bit"""
    return all((a[k] is None and b[k] is None) or sgd.same_bits(a[k], b[k]) for k in a)


def call(L, stream, ops, n, block, pdt, gdt, decoupled, hp=HP, lr_dev=None, clip=None, **kw):
    """one cot_adamw_step; kw overrides one argument by name; returns the status"""
    v = views(ops)
    a = dict(param=P(v["param"]), master=P(v["master"]), m=P(v["m"]), v=P(v["v"]), grad=P(v["grad"]), n=n, lr=hp["lr"], lr_dev=lr_dev,
             block=P(block) if torch.is_tensor(block) else block, clip=clip, b1=hp["b1"], b2=hp["b2"], eps=hp["eps"], wd=hp["wd"], gs=hp["gs"], decoupled=decoupled,
             pcode=_lib.dtype_code(pdt), gcode=_lib.dtype_code(gdt), stream=stream)
    for k, x in kw.items():
        assert k in a, k
        a[k] = x
    return L.cot_adamw_step(*a.values())


def formula(p, m, v, g, hp, step, decoupled):
    """the step in fp64 and its bounds: dict(p, m, v, E_p, E_m, E_v, scale) of float64 tensors.  p, m, v: fp32 tensors as stored; g: the
    gradient as stored (any dtype); hp: the caller's doubles"""
    p, m, v, g = (t.double() for t in (p, m, v, g))
    lr, b1, b2, eps, wd, gs = (hp[k] for k in ("lr", "b1", "b2", "eps", "wd", "gs"))
    o1, o2 = 1.0 - b1, 1.0 - b2
    bc1, sbc2 = corrections(b1, b2, step)
    G = g * gs
    E_g = 2 * U * G.abs()
    if decoupled:
        gg, decay = G, 1.0 - lr * wd
        p1 = p * decay
        E_p1 = p.abs() * (3 * U * lr * wd + U * abs(decay)) + U * p1.abs()
        l2 = torch.zeros_like(p)
    else:
        l2 = (wd * p).abs()
        gg = G + wd * p
        E_g = E_g + 2 * U * l2 + U * gg.abs()
        p1, E_p1 = p, torch.zeros_like(p)
    m1 = m * b1 + o1 * gg
    E_m = 2 * U * (m * b1).abs() + 2 * U * (o1 * gg).abs() + o1 * E_g + U * m1.abs()
    v1 = v * b2 + o2 * gg * gg
    E_v = 2 * U * v * b2 + 3 * U * o2 * gg * gg + o2 * (2 * gg.abs() * E_g + E_g * E_g) + U * v1
    s = v1.sqrt()
    den = s + (v1 - E_v).clamp(min=0).sqrt()
    E_s = torch.where(den > 0, E_v / den.clamp(min=1e-300), torch.zeros_like(s)) + U * s
    d = s / sbc2 + eps
    E_d = E_s / sbc2 + 2 * U * s / sbc2 + U * eps + U * d
    r = m1 / d
    E_r = (E_m + r.abs() * E_d) / (d - E_d) + U * r.abs()
    a = lr / bc1
    E_a = 3 * U * a
    p2 = p1 - a * r
    E_p = E_p1 + a * E_r + E_a * (r.abs() + E_r) + U * (a * r).abs() + U * p2.abs()
    # the operands' magnitudes, each weighted by how far the result follows it: p itself; m b1 and o1 (|G| + |wd p|) through the
    # numerator; |G| + |wd p| through the denominator too (|d sqrt(v') / d g| <= sqrt(o2): where g cancels and v is small, the
    # denominator is as uncertain as g is, which is the formula's own conditioning and not the kernel's)
    scale = p.abs() + a * ((m * b1).abs() + o1 * (G.abs() + l2)) / d + a * r.abs() * math.sqrt(o2) * (G.abs() + l2) / (sbc2 * d)
    return dict(p=p2, m=m1, v=v1, E_p=E_p * SLACK, E_m=E_m * SLACK, E_v=E_v * SLACK, scale=scale)


def judge(got, ref, pdt, what, extra=0.0):
    """got: dict(weights fp32, param, m, v) CPU tensors; every element inside its bound (+ `extra` roundings of the reference's own
    result).  Prints the worst error as a share of its bound, then asserts."""
    worst = {}
    finite = torch.isfinite(ref["p"])  # (NaN padding between a fixture's slots is judged separately: it must stay NaN)
    checks = [("weights", got["weights"], ref["p"], ref["E_p"]), ("exp_avg", got["m"], ref["m"], ref["E_m"]),
              ("exp_avg_sq", got["v"], ref["v"], ref["E_v"]),
              ("param", got["param"], ref["p"], ref["E_p"] + HALF_ULP[pdt] * (ref["p"].abs() + ref["E_p"]))]
    for name, x, want, bound in checks:
        bound = bound + extra * U * want.abs()
        err = (x.double() - want).abs()[finite]
        b = bound[finite]
        ratio = torch.where(err == 0, torch.zeros_like(err), err / b.clamp(min=1e-300))
        worst[name] = float(ratio.max()) if ratio.numel() else 0.0
    tight = float((ref["E_p"] / ref["scale"])[finite].max()) / U
    print(f"{what}: worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f"; largest E_p = {tight:.1f} u of the magnitudes")
    assert tight < 32, (what, tight)
    for k, v in worst.items():
        assert v <= 1.0, (what, k, v)
    return worst


def collect(ops, pdt):
    v = views(ops)
    weights = v["master"] if v["master"] is not None else v["param"]
    return dict(weights=weights.cpu(), param=v["param"].cpu(), m=v["m"].cpu(), v=v["v"].cpu())


def margins_ok(ops):
    return all(x is None or sgd.margins_intact(x[0]) for x in ops.values())


def block_untouched(buf, before):
    return torch.equal(buf.cpu(), before)


def check_step(L, dev, stream, pdt, gdt, decoupled, n, sync=lambda: None):
    """one kernel step from a given state against the formula in fp64; the gradient, the block and every margin as they were"""
    ops = operands(pdt, gdt, n, dev)
    v0 = {k: (x.cpu().clone() if x is not None else None) for k, x in views(ops).items()}
    gbuf0 = ops["grad"][0].cpu().clone()
    bbuf, block = adam_block(STEP, HP["b1"], HP["b2"], dev)
    b0 = bbuf.cpu().clone()
    assert call(L, stream, ops, n, block, pdt, gdt, decoupled) == 0, L.cot_last_error()
    sync()
    what = f"n = {n}, {pdt}/{gdt}, decoupled = {decoupled}"
    assert margins_ok(ops), f"a NaN margin was written ({what})"
    assert sgd.same_bits(ops["grad"][0].cpu(), gbuf0), f"the gradient was written ({what})"
    assert block_untouched(bbuf, b0), f"the Adam block was written ({what})"
    weights0 = v0["master"] if v0["master"] is not None else v0["param"]
    ref = formula(weights0.float(), v0["m"], v0["v"], v0["grad"], HP, STEP, decoupled)
    got = collect(ops, pdt)
    judge(got, ref, pdt, what)
    if v0["master"] is not None:
        assert torch.equal(got["param"], got["weights"].to(pdt)), f"the working copy is not the rounded master ({what})"
    assert not torch.equal(got["weights"], weights0.float()), f"the step moved nothing ({what})"


# ---- the recorded fixture and torch.optim.Adam

def fixture():
    fix = np.load(GOLDEN)
    lr, b1, b2, eps = (float(x) for x in fix["hp"])
    k = len(fix["wd"])
    steps = [int(t) for t in fix["steps"]]
    states = {}
    prev = {"p": [torch.from_numpy(fix[f"p{i}"]) for i in range(k)]}
    prev["m"] = [torch.zeros_like(t) for t in prev["p"]]
    prev["v"] = [torch.zeros_like(t) for t in prev["p"]]
    for t in steps:
        after = {a: [torch.from_numpy(fix[f"s{t}_{a}{i}"]) for i in range(k)] for a in ("p", "m", "v")}
        states[t] = dict(before=prev, grad=[torch.from_numpy(fix[f"s{t}_g{i}"]) for i in range(k)], after=after)
        prev = after
    return dict(hp=dict(lr=lr, b1=b1, b2=b2, eps=eps, gs=1.0), wd=[float(x) for x in fix["wd"]], steps=steps, states=states)


def lay_out(tensors, order, align=4):
    """(flat fp32 with NaN between the slots, [(tensor index, offset, numel)]): the tensors in `order`, each slot on a 16-byte boundary"""
    slots, off = [], 0
    for i in order:
        slots.append((i, off, tensors[i].numel()))
        off += -(-tensors[i].numel() // align) * align + align  # (+ one whole vector of padding: NaN the body of the kernel passes through)
    flat = torch.full((off,), float("nan"))
    for i, o, n in slots:
        flat[o:o + n] = tensors[i].reshape(-1)
    return flat, slots


def check_fixture_step(L, dev, stream, t, sync=lambda: None):
    """the reference's step t as recorded.  Its four tensors lie in ONE buffer with NaN padding between the slots, the tensor without
    weight decay first; weight decay is an argument of the launch, so the buffer is stepped by two launches, [no_decay] and [decay], as
    FlatAdamW's two groups are.  The padding must stay NaN."""
    fx = fixture()
    st, hp0 = fx["states"][t], fx["hp"]
    order = sorted(range(len(fx["wd"])), key=lambda i: (fx["wd"][i] != 0.0, i))
    flats = {a: lay_out(st["before"][a], order)[0] for a in ("p", "m", "v")}
    flats["g"], slots = lay_out(st["grad"], order)
    want = {a: lay_out(st["after"][a], order)[0] for a in ("p", "m", "v")}
    ops = {"param": sgd.margined(flats["p"].to(dev)), "m": sgd.margined(flats["m"].to(dev)), "v": sgd.margined(flats["v"].to(dev)),
           "grad": sgd.margined(flats["g"].to(dev)), "master": None}
    bbuf, block = adam_block(t, hp0["b1"], hp0["b2"], dev)
    split = next(o for i, o, n in slots if fx["wd"][i] != 0.0)  # where the decay group begins
    total = flats["p"].numel()
    for lo, hi, wd in ((0, split, 0.0), (split, total, max(fx["wd"]))):
        part = {k: ((x[0], x[1][lo:hi]) if x is not None else None) for k, x in ops.items()}
        assert call(L, stream, part, hi - lo, block, torch.float32, torch.float32, 1, hp=dict(hp0, wd=wd)) == 0, L.cot_last_error()
    sync()
    assert margins_ok(ops), "a NaN margin was written"
    got = collect(ops, torch.float32)
    pad = torch.isnan(flats["p"])
    for k in ("weights", "m", "v"):
        assert bool(torch.isnan(got[k][pad]).all()) and bool(torch.isfinite(got[k][~pad]).all()), f"the padding did not stay NaN ({k})"
    wd_flat = torch.zeros(total, dtype=torch.float64)
    wd_flat[split:] = max(fx["wd"])
    worst = {}
    for wd, sel in ((0.0, wd_flat == 0), (max(fx["wd"]), wd_flat != 0)):
        ref = formula(flats["p"][sel], flats["m"][sel], flats["v"][sel], flats["g"][sel], dict(hp0, wd=wd), t, True)
        # the recorded result within ITS bound of the formula too (same count, + its own last rounding): the fixture is what it claims
        for a, e in (("p", "E_p"), ("m", "E_m"), ("v", "E_v")):
            ok = torch.isfinite(ref[a])
            assert bool(((want[a][sel].double() - ref[a]).abs() <= ref[e] + U * ref[a].abs())[ok].all()), (t, a, "the fixture is off the formula")
        worst[wd] = judge({k: x[sel] for k, x in got.items()}, ref, torch.float32, f"fixture step {t}, wd {wd}")
        # ... and against the recorded state itself: the same bounds plus one fp32 rounding for the reference's own result
        rec = dict(ref, p=want["p"][sel].double(), m=want["m"][sel].double(), v=want["v"][sel].double())
        judge({k: x[sel] for k, x in got.items()}, rec, torch.float32, f"fixture step {t}, wd {wd}, against the recorded state", extra=1.0)
    return worst


def check_l2_against_torch_adam(L, dev, stream, sync=lambda: None):
    """decoupled = 0 against torch.optim.Adam stepped live on the CPU from the same state (step 4 -> 5), weight_decay 0.05"""
    n, t = 4003, 5
    hp = dict(HP, gs=1.0)
    ops = operands(torch.float32, torch.float32, n, dev, seed=11)
    v0 = {k: (x.cpu().clone() if x is not None else None) for k, x in views(ops).items()}
    p = torch.nn.Parameter(v0["param"].clone())
    opt = torch.optim.Adam([p], lr=hp["lr"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"], weight_decay=hp["wd"], foreach=False)
    sd = opt.state_dict()
    sd["state"] = {0: {"step": torch.tensor(float(t - 1)), "exp_avg": v0["m"].clone(), "exp_avg_sq": v0["v"].clone()}}
    opt.load_state_dict(sd)
    p.grad = v0["grad"].clone()
    opt.step()
    assert int(opt.state[p]["step"]) == t
    bbuf, block = adam_block(t, hp["b1"], hp["b2"], dev)
    assert call(L, stream, ops, n, block, torch.float32, torch.float32, 0, hp=hp) == 0, L.cot_last_error()
    sync()
    assert margins_ok(ops)
    ref = formula(v0["param"], v0["m"], v0["v"], v0["grad"], hp, t, False)
    got = collect(ops, torch.float32)
    judge(got, ref, torch.float32, "L2 form, the formula")
    rec = dict(ref, p=p.detach().double(), m=opt.state[p]["exp_avg"].double(), v=opt.state[p]["exp_avg_sq"].double())
    judge(got, rec, torch.float32, "L2 form, torch.optim.Adam", extra=1.0)


# ---- the tick

def ulps32(a, b):
    x = torch.tensor([a, b], dtype=torch.float32).view(torch.int32)
    return abs(int(x[0]) - int(x[1]))


def check_tick(L, dev, stream, sync=lambda: None, exact=False):
    """k ticks from zero, k in 1, 2, 10, 1000: step = k and the corrections are the fp32 roundings of the Python doubles -- within ONE
    fp32 ulp on the device, whose pow may be one double ulp off Python's, which can move the fp32 rounding across a tie (exact=True, the
    emulator: the host's own pow, no allowance).  A block loaded at step = t (set to t - 1, ticked once: FlatAdamW.load_state_dict)
    equals one ticked t times bit for bit."""
    b1, b2 = HP["b1"], HP["b2"]
    bbuf, block = adam_block(0, b1, b2, dev)
    done, after = 0, {}
    for k in (1, 2, 10, 1000):
        for _ in range(k - done):
            assert L.cot_adam_tick(P(block), None, b1, b2, stream) == 0, L.cot_last_error()
        done = k
        sync()
        after[k] = bbuf.cpu().clone()
        got = read_block(block)
        bc1, sbc2 = corrections(b1, b2, k)
        assert got["step"] == k and got["refused"] == 0 and got["reserved"] == [0, 0, 0, 0], got
        allow = 0 if exact else 1
        assert ulps32(got["bc1"], bc1) <= allow and ulps32(got["sqrt_bc2"], sbc2) <= allow, (k, got, f32(bc1), f32(sbc2))
        assert bool((bbuf.cpu()[:8] == SENTINEL).all()) and bool((bbuf.cpu()[16:] == SENTINEL).all()), "a word next to the block was written"
    for t in (1, 2, 10, 1000):
        lbuf, loaded = adam_block(0, b1, b2, dev)
        loaded[0] = t - 1
        assert L.cot_adam_tick(P(loaded), None, b1, b2, stream) == 0, L.cot_last_error()
        sync()
        assert torch.equal(lbuf.cpu(), after[t]), f"a block loaded at step {t} differs from one ticked {t} times"


def check_tick_skip(L, dev, stream, sync=lambda: None):
    """a clip block that says skip: nothing but the refused count moves; one that does not: the tick is the plain one"""
    b1, b2 = HP["b1"], HP["b2"]
    bbuf, block = adam_block(3, b1, b2, dev)
    before = bbuf.cpu().clone()
    cbuf, clip = clip_block(0.0, 1, dev)
    c0 = cbuf.cpu().clone()
    for i in (1, 2):
        assert L.cot_adam_tick(P(block), P(clip), b1, b2, stream) == 0, L.cot_last_error()
        sync()
        want = before.clone()
        want[11] = i
        assert torch.equal(bbuf.cpu(), want), (bbuf.cpu().tolist(), want.tolist())
    assert torch.equal(cbuf.cpu(), c0), "the tick wrote the clip block"
    cbuf, clip = clip_block(0.5, 0, dev)
    plain_buf, plain = adam_block(3, b1, b2, dev, refused=2)
    assert L.cot_adam_tick(P(block), P(clip), b1, b2, stream) == 0 and L.cot_adam_tick(P(plain), None, b1, b2, stream) == 0
    sync()
    assert torch.equal(bbuf.cpu(), plain_buf.cpu()) and read_block(block)["step"] == 4


# ---- properties that are bits

def check_zero_gradient(L, dev, stream, pdt, gdt, sync=lambda: None):
    """zero gradient from zero moments: m and v stay exactly 0; p only decays in the decoupled form (p * (1 - lr wd), one product) and
    keeps its bits in the L2 form with weight_decay 0"""
    n = 4003
    for decoupled, wd in ((1, HP["wd"]), (0, 0.0)):
        ops = operands(pdt, gdt, n, dev, seed=3)
        for k in ("m", "v", "grad"):
            ops[k][1].zero_()
        before = buffers_cpu(ops)
        bbuf, block = adam_block(1, HP["b1"], HP["b2"], dev)
        assert call(L, stream, ops, n, block, pdt, gdt, decoupled, hp=dict(HP, wd=wd)) == 0, L.cot_last_error()
        sync()
        after = buffers_cpu(ops)
        for k in ("m", "v", "grad"):
            assert sgd.same_bits(after[k], before[k]), f"{k} moved under a zero gradient (decoupled = {decoupled})"
        wk = "master" if pdt != torch.float32 else "param"
        w0, w1 = before[wk][sgd.MARGIN:-sgd.MARGIN], after[wk][sgd.MARGIN:-sgd.MARGIN]
        if decoupled:
            decay = torch.tensor(1.0, dtype=torch.float32) - torch.tensor(HP["lr"], dtype=torch.float32) * torch.tensor(wd, dtype=torch.float32)
            assert torch.equal(w1, w0 * decay), "the decoupled form did not only decay"
            assert torch.equal(after["param"][sgd.MARGIN:-sgd.MARGIN], w1.to(pdt))
        else:
            assert same(after, before), "the L2 form with weight_decay 0 moved a weight under a zero gradient"


def check_rate_sources(L, dev, stream, pdt, gdt, sync=lambda: None):
    """lr by value and through lr_dev: equal bits; the rate tensor is left as it was"""
    for n in SIZES:
        for lr in sgd.RATES:
            base = operands(pdt, gdt, n, dev, seed=5)
            by_value, by_dev = sgd.clone_ops(base), sgd.clone_ops(base)
            rate = torch.tensor([lr], dtype=torch.float32).to(dev)
            bbuf, block = adam_block(STEP, HP["b1"], HP["b2"], dev)
            assert call(L, stream, by_value, n, block, pdt, gdt, 1, hp=dict(HP, lr=lr)) == 0, L.cot_last_error()
            assert call(L, stream, by_dev, n, block, pdt, gdt, 1, hp=dict(HP, lr=123.0), lr_dev=P(rate)) == 0, L.cot_last_error()
            sync()
            assert same(buffers_cpu(by_value), buffers_cpu(by_dev)), f"the two rate sources differ (n = {n}, lr = {lr!r})"
            assert float(rate.cpu()) == f32(lr)


def check_clip_block(L, dev, stream, pdt, gdt, sync=lambda: None):
    """skip = 1: no operand's bits change; scale = 0.5: the bits of a run with grad_scale halved (0.5 * gs is exact in fp32)"""
    for n in SIZES:
        base = operands(pdt, gdt, n, dev, seed=6)
        bbuf, block = adam_block(STEP, HP["b1"], HP["b2"], dev)
        b0 = bbuf.cpu().clone()
        skipped, scaled, halved = sgd.clone_ops(base), sgd.clone_ops(base), sgd.clone_ops(base)
        sbuf, skip = clip_block(0.5, 1, dev)
        cbuf, half = clip_block(0.5, 0, dev)
        c0 = cbuf.cpu().clone()
        for decoupled in (0, 1):
            assert call(L, stream, skipped, n, block, pdt, gdt, decoupled, clip=P(skip)) == 0, L.cot_last_error()
        assert call(L, stream, scaled, n, block, pdt, gdt, 1, clip=P(half)) == 0, L.cot_last_error()
        assert call(L, stream, halved, n, block, pdt, gdt, 1, hp=dict(HP, gs=HP["gs"] * 0.5)) == 0, L.cot_last_error()
        sync()
        assert same(buffers_cpu(skipped), buffers_cpu(base)), f"a skipped step wrote something (n = {n})"
        assert same(buffers_cpu(scaled), buffers_cpu(halved)), f"scale = 0.5 differs from grad_scale halved (n = {n})"
        assert not same(buffers_cpu(scaled), buffers_cpu(base))
        assert torch.equal(cbuf.cpu(), c0) and torch.equal(bbuf.cpu(), b0), "a block was written"


def check_repeatable(L, dev, stream, pdt, gdt, sync=lambda: None):
    base = operands(pdt, gdt, 4003, dev, seed=7)
    one, two = sgd.clone_ops(base), sgd.clone_ops(base)
    bbuf, block = adam_block(STEP, HP["b1"], HP["b2"], dev)
    for ops in (one, two):
        assert call(L, stream, ops, 4003, block, pdt, gdt, 1) == 0, L.cot_last_error()
    sync()
    assert same(buffers_cpu(one), buffers_cpu(two)), "two calls on equal data differ"


def check_refusals(L, dev, stream, sync=lambda: None):
    """each refused with its message before any device work: every operand and both blocks stay as they were"""
    pdt, gdt, n = torch.bfloat16, torch.bfloat16, 37
    ops = operands(pdt, gdt, n, dev, seed=8)
    bbuf, block = adam_block(STEP, HP["b1"], HP["b2"], dev)
    cbuf, clip = clip_block(0.5, 0, dev)
    rate = torch.tensor([0.01], dtype=torch.float32).to(dev)
    keep, b0, c0 = buffers_cpu(ops), bbuf.cpu().clone(), cbuf.cpu().clone()
    v = views(ops)

    def refused(rc, message, status=-1):
        assert rc == status, (rc, message, L.cot_last_error())
        assert message in L.cot_last_error(), (message, L.cot_last_error())
        sync()
        assert same(buffers_cpu(ops), keep) and torch.equal(bbuf.cpu(), b0) and torch.equal(cbuf.cpu(), c0), message

    def odd(t, by):
        return ctypes.c_void_p(t.data_ptr() + by)

    def step(**kw):
        a = dict(dict(clip=P(clip), lr_dev=P(rate)), **kw)
        return call(L, stream, ops, a.pop("n", n), a.pop("block", block), pdt, gdt, 1, **a)

    for k in ("param", "m", "v", "grad"):
        refused(step(**{k: None}), b"NULL device pointer")
    refused(step(block=None), b"NULL adam_state")
    refused(step(param=odd(v["param"], 2)), b"16-byte")
    refused(step(master=odd(v["master"], 4)), b"16-byte")
    refused(step(m=odd(v["m"], 4)), b"16-byte")
    refused(step(v=odd(v["v"], 8)), b"16-byte")
    refused(step(grad=odd(v["grad"], 2)), b"16-byte")
    refused(step(block=odd(block, 2)), b"adam_state")
    refused(step(clip=odd(clip, 2)), b"clip_state")
    refused(step(lr_dev=odd(rate, 2)), b"lr_dev")
    refused(step(n=0), b"element count")
    refused(step(n=-4), b"element count")
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        refused(step(b1=bad), b"beta1")
        refused(step(b2=bad), b"beta2")
    for bad in (0.0, -1e-8, float("nan"), float("inf")):
        refused(step(eps=bad), b"eps")
    for bad in (-1e-3, float("nan"), float("inf")):
        refused(step(lr=bad), b"lr")
        refused(step(wd=bad), b"weight_decay")
    refused(step(pcode=_lib.dtype_code(torch.float16)), b"not supported", _lib.COT_ERR_UNSUPPORTED)
    refused(step(gcode=_lib.dtype_code(torch.float64)), b"not supported", _lib.COT_ERR_UNSUPPORTED)
    refused(step(master=None), b"not supported", _lib.COT_ERR_UNSUPPORTED)  # (bf16 parameters need their master)
    refused(step(pcode=_lib.dtype_code(torch.float32)), b"not supported", _lib.COT_ERR_UNSUPPORTED)  # (fp32 parameters take none)
    # the tick
    refused(L.cot_adam_tick(None, P(clip), 0.9, 0.999, stream), b"NULL adam_state")
    refused(L.cot_adam_tick(odd(block, 2), P(clip), 0.9, 0.999, stream), b"adam_state")
    refused(L.cot_adam_tick(P(block), odd(clip, 2), 0.9, 0.999, stream), b"clip_state")
    for bad in (-0.1, 1.0, float("nan")):
        refused(L.cot_adam_tick(P(block), P(clip), bad, 0.999, stream), b"beta1")
        refused(L.cot_adam_tick(P(block), P(clip), 0.9, bad, stream), b"beta2")
    assert step() == 0, L.cot_last_error()  # (the arguments the refusals were variations of are good ones)
    sync()
    assert not same(buffers_cpu(ops), keep)


# ---- FlatAdamW: the small net of tests/test_flat_sgd_gpu.py's kind, shared by the emulated and the device tests

def bucket_grads(opt):
    """{parameter: clone of its gradient in the bucket, as the step will read it}"""
    return {p: opt.reducer.reduced(b)[off:off + p.numel()].clone().view_as(p)
            for b in opt.reducer.buckets for p, off in zip(b.params, b.offs)}


def opt_state(model, opt):
    """everything a step may write: working copies, masters, both moments, the block -- clones, in a fixed order"""
    out = [p.detach().clone() for p in model.parameters()]
    for st in opt.state:
        out += [st["exp_avg"].clone(), st["exp_avg_sq"].clone()] + ([st["master"].clone()] if st["master"] is not None else [])
    return out + [opt.adam_state.clone()]


def differing(a, b):
    """[(index, shape, dtype, elements that differ)] of the entries of two opt_state() / whole_state() lists that are not equal bit for bit"""
    def bits(t):
        return t.view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
    assert len(a) == len(b)
    return [(i, tuple(u.shape), str(u.dtype), int((bits(u) != bits(v)).sum())) for i, (u, v) in enumerate(zip(a, b))
            if not torch.equal(bits(u), bits(v))]


def states_equal(a, b):
    return not differing(a, b)


def check_against_torch(model, opt, inputs, loss_fn, decoupled):
    """four steps, each against torch.optim.AdamW / Adam on fp32 clones fed the gradients read from the buckets; the clones are set to
    our state after each comparison, so the per-step bounds apply (torch's result within the formula's bounds plus one rounding of its
    own, as for the fixture).  The working copy is the rounded master."""
    hp = dict(lr=opt.lr, b1=opt.betas[0], b2=opt.betas[1], eps=opt.eps, gs=1.0)
    params = list(model.parameters())
    wd_of = {p: (opt.weight_decay if b.key == "decay" else 0.0) for b in opt.reducer.buckets for p in b.params}
    clones = {p: torch.nn.Parameter(opt.master_parameters()[p].detach().float().cpu().clone()) for p in params}
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    ref = cls([dict(params=[clones[p] for p in params if wd_of[p] == 0.0], weight_decay=0.0),
               dict(params=[clones[p] for p in params if wd_of[p] != 0.0], weight_decay=opt.weight_decay)],
              lr=opt.lr, betas=opt.betas, eps=opt.eps, foreach=False)
    for t, x in enumerate(inputs, start=1):
        opt.zero_grad()
        loss_fn(model, x).backward()
        grads = bucket_grads(opt)
        before = {p: (opt.master_parameters()[p].detach().cpu().clone(), opt._slots("exp_avg")[p].cpu().clone(),
                      opt._slots("exp_avg_sq")[p].cpu().clone()) for p in params}
        opt.step()
        for p in params:
            clones[p].grad = grads[p].float().cpu()
        ref.step()
        for p in params:
            w0, m0, v0 = before[p]
            f = formula(w0.reshape(-1), m0.reshape(-1), v0.reshape(-1), grads[p].cpu().reshape(-1), dict(hp, wd=wd_of[p]), t, decoupled)
            got = dict(weights=opt.master_parameters()[p].detach().cpu().reshape(-1), param=p.detach().cpu().reshape(-1),
                       m=opt._slots("exp_avg")[p].cpu().reshape(-1), v=opt._slots("exp_avg_sq")[p].cpu().reshape(-1))
            what = f"step {t}, {tuple(p.shape)} {p.dtype}, decoupled = {decoupled}"
            judge(got, f, p.dtype, what)
            st = ref.state[clones[p]]
            rec = dict(f, p=clones[p].detach().double().reshape(-1), m=st["exp_avg"].double().reshape(-1), v=st["exp_avg_sq"].double().reshape(-1))
            judge(dict(got, param=got["weights"]), rec, torch.float32, what + ", torch", extra=1.0)
            assert torch.equal(p.detach().cpu(), opt.master_parameters()[p].detach().cpu().to(p.dtype)), "the working copy is not the rounded master"
            assert int(st["step"]) == t
            with torch.no_grad():  # re-synchronise: nothing compounds
                clones[p].copy_(opt.master_parameters()[p].detach().cpu())
                st["exp_avg"].copy_(opt._slots("exp_avg")[p].cpu())
                st["exp_avg_sq"].copy_(opt._slots("exp_avg_sq")[p].cpu())
    assert opt.adam_stats()["step"] == len(inputs)


# ---- FlatAdamW on a small net: what the emulated and the device tests share

def net():
    """tests/test_flat_sgd_gpu.py's small net: both decay groups, BatchNorm buffers, bf16 and fp32 buckets in the mixed form"""
    from torch import nn
    return nn.Sequential(nn.Conv2d(3, 16, 3, padding=1), nn.BatchNorm2d(16), nn.ReLU(), nn.Conv2d(16, 8, 1, bias=True),
                         nn.GroupNorm(2, 8), nn.AdaptiveAvgPool2d(1), nn.Flatten(), nn.Linear(8, 5))


def small():
    """tests/checkpoint_cases.py's model: a matrix, a bias and BatchNorm vectors -- both decay groups, buffers, and in the mixed form bf16
    and fp32 buckets.  It is the model of every case that compares two RUNS bit for bit: its torch operators are reproducible on the
    device in both forms (the existing checkpoint tests rest on that), while the fp32 backward of net()'s torch convolutions is not --
    two identical eager runs of it differed in the first step's gradient bucket (measured on the MI355X)."""
    from torch import nn
    return nn.Sequential(nn.Linear(8, 8), nn.BatchNorm1d(8))


def build(dev, mixed, seed=0, cls=None, conv=False, **kw):
    """(model, optimizer): small(), or with conv=True net() (for the cases judged by a bound)"""
    from cotnet_amd.flat_adamw import FlatAdamW
    from cotnet_amd.flat_sgd import to_mixed_bf16
    torch.manual_seed(seed)
    model = (net() if conv else small()).to(dev).train()
    if mixed:
        to_mixed_bf16(model)
    hp = dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    hp.update(kw)
    opt = (cls or FlatAdamW)(model, **hp)
    assert {b.key for b in opt.reducer.buckets} == {"decay", "no_decay"}
    return model, opt


def batches(dev, mixed, n, seed=1, conv=False):
    g = torch.Generator().manual_seed(seed)
    shape, classes = ((6, 3, 8, 8), 5) if conv else ((6, 8), 8)
    return [(torch.randn(shape, generator=g).to(torch.bfloat16 if mixed else torch.float32).to(dev),
             torch.randint(0, classes, (6,), generator=g).to(dev)) for _ in range(n)]


def loss_fn(model, batch):
    return torch.nn.functional.cross_entropy(model(batch[0]).float(), batch[1])


def train_step(model, opt, batch):
    opt.zero_grad()
    loss_fn(model, batch).backward()
    opt.step()


def whole_state(model, opt):
    """opt_state plus the buffers and, where kept, the averages"""
    out = opt_state(model, opt) + [b.detach().clone() for b in model.buffers()]
    if opt.ema_decay is not None:
        out += [st["ema"].clone() for st in opt.state] + [b.clone() for b in opt._buf_ema]
    if opt.clip_state is not None:
        out.append(opt.clip_state.clone())
    return out


def check_flat_against_torch(dev, mixed, decoupled):
    from cotnet_amd.flat_adamw import FlatAdam, FlatAdamW
    model, opt = build(dev, mixed, cls=FlatAdamW if decoupled else FlatAdam, conv=True)
    assert opt.decoupled == bool(decoupled)
    check_against_torch(model, opt, batches(dev, mixed, 4, conv=True), loss_fn, decoupled)


def pytest_raises(exc, match):
    import pytest
    return pytest.raises(exc, match=match)


def check_checkpoint(dev, mixed, captured=None, **kw):
    """three steps, state_dict + model_state_dict, loaded into a fresh model and optimizer (and, captured(model, opt) -> step function
    given, into one whose step was captured before the load); two more steps: bit-equal to five uninterrupted steps"""
    bs = batches(dev, mixed, 5)
    model, opt = build(dev, mixed, ema_decay=0.9, **kw)
    for b in bs[:3]:
        train_step(model, opt, b)
    sd, msd, esd = opt.state_dict(), opt.model_state_dict(), opt.ema_state_dict()
    assert all(s["step"] == 3 and isinstance(s["step"], int) for s in sd["state"].values())
    assert [g["amsgrad"] for g in sd["param_groups"]] == [False, False] and sd["param_groups"][0]["weight_decay"] == 0.0
    assert sd["cotnet_amd"]["decoupled"] is True and sd["cotnet_amd"]["refused"] == 0
    for b in bs[3:]:
        train_step(model, opt, b)
    want = whole_state(model, opt)
    assert opt.adam_stats()["step"] == 5
    # other weights, another rate; without a capture other betas, eps and weight decay too (those travel by value: a captured step keeps
    # its own, and load_state_dict refuses to change them behind it)
    other = dict(lr=0.5) if captured is not None else dict(lr=0.5, betas=(0.5, 0.5), eps=1e-3, weight_decay=0.3)
    fresh, fopt = build(dev, mixed, seed=5, ema_decay=0.9, **dict(kw, **other))
    step = (lambda b: train_step(fresh, fopt, b)) if captured is None else captured(fresh, fopt)
    if captured is not None:
        with pytest_raises(ValueError, "captured into a HIP graph"):
            fopt.load_state_dict(dict(sd, param_groups=[dict(g, eps=1e-3) for g in sd["param_groups"]]))
    addresses = [fopt.adam_state.data_ptr()] + [st[k].data_ptr() for st in fopt.state for k in ("exp_avg", "exp_avg_sq")]
    fopt.load_model_state_dict(msd)
    fopt.load_state_dict(sd)
    fopt.load_ema_state_dict(esd)
    assert addresses == [fopt.adam_state.data_ptr()] + [st[k].data_ptr() for st in fopt.state for k in ("exp_avg", "exp_avg_sq")]
    assert (fopt.lr, fopt.betas, fopt.eps, fopt.weight_decay) == (opt.lr, opt.betas, opt.eps, opt.weight_decay)
    assert fopt.adam_stats()["step"] == 3
    for b in bs[3:]:
        step(b)
    assert states_equal(want, whole_state(fresh, fopt)), "resumed and uninterrupted runs differ"


def _torch_groups(model, opt):
    names = [[n for n, _ in g] for g in opt._groups()]
    params = dict(model.named_parameters())
    return [dict(params=[params[n] for n in names[0]], weight_decay=0.0), dict(params=[params[n] for n in names[1]], weight_decay=0.05)]


def check_torch_interop(dev, mixed):
    """our dict loads into torch.optim.AdamW over the same groups of an fp32 twin (it turns the int step into its tensor and steps); a
    dict torch wrote (tensor steps, no 'cotnet_amd') loads here into the right slots, and the block is the one 2 ticks leave"""
    import copy
    bs = batches(dev, mixed, 3)
    model, opt = build(dev, mixed)
    for b in bs[:2]:
        train_step(model, opt, b)
    sd = opt.state_dict()
    twin = copy.deepcopy(model).float().cpu()
    ref = torch.optim.AdamW(_torch_groups(twin, opt), lr=1.0)
    ref.load_state_dict({"state": {k: {a: (v.cpu() if torch.is_tensor(v) else v) for a, v in s.items()} for k, s in sd["state"].items()},
                         "param_groups": sd["param_groups"]})
    g = ref.param_groups
    assert (g[0]["lr"], tuple(g[0]["betas"]), g[0]["eps"], g[1]["weight_decay"]) == (opt.lr, opt.betas, opt.eps, opt.weight_decay)
    flat = [p for grp in ref.param_groups for p in grp["params"]]
    ours = [p for grp in opt._groups() for _, p in grp]
    for q, p in zip(flat, ours):
        assert int(ref.state[q]["step"]) == 2 and torch.equal(ref.state[q]["exp_avg"], opt._slots("exp_avg")[p].cpu())
        q.grad = torch.zeros_like(q)
    ref.step()
    assert all(int(ref.state[q]["step"]) == 3 for q in flat)
    written = ref.state_dict()  # torch's own form: tensor steps
    assert all(torch.is_tensor(s["step"]) for s in written["state"].values()) and "cotnet_amd" not in written
    other, oopt = build(dev, mixed, seed=9, lr=0.7)
    oopt.load_state_dict(written)
    assert oopt.lr == opt.lr and oopt.adam_stats()["step"] == 3
    expect = adam_block(3, opt.betas[0], opt.betas[1], "cpu")[1]
    assert torch.equal(oopt.adam_state.cpu(), expect), (oopt.adam_state.cpu().tolist(), expect.tolist())
    for q, (_, p) in zip(flat, [m for grp in oopt._groups() for m in grp]):
        assert torch.equal(oopt._slots("exp_avg")[p].cpu(), ref.state[q]["exp_avg"]) and \
            torch.equal(oopt._slots("exp_avg_sq")[p].cpu(), ref.state[q]["exp_avg_sq"])


def check_saver_round_trip(dev, mixed, tmp_path):
    """CheckpointSaver writes a FlatAdamW, resume_checkpoint restores it into a fresh one: the next step is bit-equal"""
    from cotnet_amd import CheckpointSaver, resume_checkpoint
    bs = batches(dev, mixed, 3)
    model, opt = build(dev, mixed, ema_decay=0.9, skip_nonfinite=True)
    for b in bs[:2]:
        train_step(model, opt, b)
    saver = CheckpointSaver(model, opt, checkpoint_dir=str(tmp_path), recovery_dir=str(tmp_path))
    saver.save_checkpoint(1, metric=0.5)
    train_step(model, opt, bs[2])
    fresh, fopt = build(dev, mixed, seed=4, ema_decay=0.9, skip_nonfinite=True, lr=0.3)
    assert resume_checkpoint(fresh, str(tmp_path / "checkpoint-1.pth.tar"), optimizer=fopt, log_info=False) == 1
    assert fopt.adam_stats()["step"] == 2 and fopt.clip_stats()["steps"] == 2
    train_step(fresh, fopt, bs[2])
    assert states_equal(whole_state(model, opt), whole_state(fresh, fopt))


def check_skipped_step(dev, mixed):
    """eager: an inf planted in one gradient bucket before the second step -- no weight, no moment written, the count stays, refused = 1,
    the EMA still moves; the third step trains again as step 2"""
    bs = batches(dev, mixed, 3)
    model, opt = build(dev, mixed, skip_nonfinite=True, ema_decay=0.9)
    train_step(model, opt, bs[0])
    before, ema0 = opt_state(model, opt), [st["ema"].clone() for st in opt.state]
    opt.zero_grad()
    loss_fn(model, bs[1]).backward()
    b = opt.reducer.buckets[-1]
    opt.reducer.reduced(b)[b.offs[0] + 1] = float("inf")
    opt.step()
    after = opt_state(model, opt)
    assert states_equal(before[:-1], after[:-1]), "a skipped step wrote weights, masters or moments"
    s = opt.adam_stats()
    assert (s["step"], s["refused"]) == (1, 1) and opt.clip_stats()["skipped"] == 1, s
    assert torch.equal(before[-1][:3], after[-1][:3]) and after[-1][4:].tolist() == [0, 0, 0, 0]
    assert all(not torch.equal(e0, st["ema"]) for e0, st in zip(ema0, opt.state)), "the EMA did not move behind the skipped step"
    train_step(model, opt, bs[2])
    s = opt.adam_stats()
    assert (s["step"], s["refused"]) == (2, 1) and not states_equal(before[:-1], opt_state(model, opt)[:-1])
    assert ulps32(s["bc1"], corrections(*opt.betas, 2)[0]) <= 1  # (the second step ran as step 2, not 3)
