"""Lookahead on the device (csrc/lookahead.hip: cot_lookahead_tick, cot_lookahead_step; FlatSGD / FlatAdamW(lookahead_k=...)): the cases
and criteria that tests/test_lookahead_emulated.py runs on the host emulator and tests/test_lookahead_gpu.py on the device.

The kernel's sync is, per element in fp32, d = fast - slow; s = slow + alpha * d, with alpha the fp32 rounding of the caller's double
(the order is stated at the top of lookahead.hip).  With alpha = 0.5 the product is exact -- a fused multiply-add and the two separate
operations round the same value once -- so the result is compared BIT FOR BIT with `slow + 0.5 * (fast - slow)` evaluated on fp32
tensors on the CPU.  With any other alpha the reference is THE FORMULA IN FP64 on the operands as stored and on alpha as the caller
holds it, and the bound is DERIVED, not measured; u = 2^-24:

    d  = f - s                 one rounding:                            u |d|
    a  = (float)alpha          one rounding of the constant:            u alpha |d|      carried into the product
    q  = a * d                 one rounding (none when contracted):     u alpha |d|      and alpha times d's own: u alpha |d|
    s' = s + q                 one rounding:                            u |s'|

    E = (3 alpha |f - s| + |s'|) u (1 + 2^-10)

(with alpha <= 1 the rounding of d, carried through the product, is alpha u |d|; the factor 1 + 2^-10 covers the products of two
roundings, as in tests/adamw_cases.py).  EVERY element is judged.  The recorded fixture (tests/golden/lookahead.npz,
tests/golden/make_golden_lookahead.py) is an fp32 evaluation of the same formula with roundings of its own: it is judged with the same
bound plus one fp32 rounding of its own result, u |ref| -- and bit for bit where alpha is 0.5.

Operands sit inside NaN margins (tests/sgd_lr_cases.py) which must stay NaN; the block sits between sentinel words.

The optimizer cases run on adamw_cases.small(), the model of every case that compares two runs bit for bit."""
import copy
import ctypes
import os

import numpy as np
import torch

from cotnet_amd import _lib
from tests import adamw_cases as adamw
from tests import sgd_lr_cases as sgd

P = sgd.P
U = adamw.U
SLACK = adamw.SLACK
SENTINEL = adamw.SENTINEL
SIZES = sgd.SIZES  # 1, 3, 4, 5, 4003: tail only, body only, body + tail
SECOND_TRIP = adamw.SECOND_TRIP
FORMS = [torch.bfloat16, torch.float32]  # the parameters' dtype: bf16 with an fp32 master, fp32 without
FORM_IDS = ["bf16-master", "fp32"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lookahead.npz")
WORDS = ("step", "action", "born", "syncs", "refused")


# ---- the block

def la_block(dev, step=0, action=0, born=0, syncs=0, refused=0):
    """(buffer, view): int32[8] = cot_lookahead_state between eight sentinel words on each side"""
    buf = torch.full((24,), SENTINEL, dtype=torch.int32)
    buf[8:16] = torch.tensor([step, action, born, syncs, refused, 0, 0, 0], dtype=torch.int32)
    buf = buf.to(dev)
    return buf, buf[8:16]


def read_block(view):
    w = view.cpu().tolist()
    return dict(zip(WORDS, w[:5]), reserved=w[5:])


def sentinels_intact(buf):
    w = buf.cpu()
    return bool((w[:8] == SENTINEL).all()) and bool((w[16:] == SENTINEL).all())


# ---- cot_lookahead_step

def operands(pdt, n, dev, seed=0):
    """{name: (buffer, view)} on `dev`: param, master (None for fp32 parameters), slow"""
    g = torch.Generator().manual_seed(7300 + seed + n % 1000)
    fast = torch.randn(n, generator=g)
    slow = fast + torch.randn(n, generator=g) * torch.where(torch.arange(n) % 3 == 0, 1.0, 0.05)  # near and far
    return {"param": sgd.margined(fast.to(pdt).to(dev)), "master": sgd.margined(fast.to(dev)) if pdt != torch.float32 else None,
            "slow": sgd.margined(slow.to(dev))}


def call(L, stream, ops, n, block, pdt, alpha=0.5, **kw):
    """one cot_lookahead_step; kw overrides one argument by name; returns the status"""
    v = adamw.views(ops)
    a = dict(param=P(v["param"]), master=P(v["master"]), slow=P(v["slow"]), n=n, alpha=alpha,
             block=P(block) if torch.is_tensor(block) else block, pcode=_lib.dtype_code(pdt), stream=stream)
    for k, x in kw.items():
        assert k in a, k
        a[k] = x
    return L.cot_lookahead_step(*a.values())


def fast_of(values):
    """the fp32 weights among a {name: tensor} of views or their clones"""
    return values["master"] if values["master"] is not None else values["param"]


def bound(fast, slow, alpha):
    """(s' in fp64, E): the derivation in this module's docstring; fast, slow: fp32 tensors as stored; alpha: the caller's double"""
    f, s = fast.double(), slow.double()
    want = s + alpha * (f - s)
    return want, (3.0 * alpha * (f - s).abs() + want.abs()) * U * SLACK


def judge(got, want, E, what, extra=0.0):
    """every element of `got` within E (+ `extra` roundings of the reference's own result); prints the worst share, then asserts"""
    finite = torch.isfinite(want)
    err = (got.double() - want).abs()[finite]
    b = (E + extra * U * want.abs())[finite]
    ratio = torch.where(err == 0, torch.zeros_like(err), err / b.clamp(min=1e-300))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"{what}: worst error / bound {worst:.3f} over {int(finite.sum())} elements")
    assert worst <= 1.0, (what, worst)
    return worst


def check_interpolation(L, dev, stream, pdt, n, alpha, sync=lambda: None):
    """action 2 from a given state: the slow weights against the formula, the fast weights with their bits, the working copy their
    rounding; the block and every margin as they were"""
    ops = operands(pdt, n, dev)
    v0 = {k: (x.cpu().clone() if x is not None else None) for k, x in adamw.views(ops).items()}
    bbuf, block = la_block(dev, step=6, action=2, born=1, syncs=2)
    b0 = bbuf.cpu().clone()
    assert call(L, stream, ops, n, block, pdt, alpha=alpha) == 0, L.cot_last_error()
    sync()
    what = f"n = {n}, {pdt}, alpha = {alpha}"
    assert adamw.margins_ok(ops), f"a NaN margin was written ({what})"
    assert torch.equal(bbuf.cpu(), b0), f"the block was written ({what})"
    got = {k: (x.cpu() if x is not None else None) for k, x in adamw.views(ops).items()}
    f0, s0 = fast_of(v0).float(), v0["slow"]
    if alpha == 0.5:
        assert sgd.same_bits(got["slow"], s0 + 0.5 * (f0 - s0)), f"alpha 0.5 is exact: slow differs from the fp32 expression ({what})"
    else:
        want, E = bound(f0, s0, alpha)
        judge(got["slow"], want, E, what)
    assert sgd.same_bits(fast_of(got), got["slow"]), f"the fast weights do not have the slow weights' bits ({what})"
    assert torch.equal(got["param"], got["slow"].to(pdt)), f"the working copy is not the rounded slow weights ({what})"
    assert not torch.equal(got["slow"], s0), f"the sync moved nothing ({what})"


def check_actions(L, dev, stream, pdt, sync=lambda: None):
    """action 0 leaves every buffer as it was; action 1 gives slow the fast weights' bits and writes nothing else"""
    for n in SIZES:
        base = operands(pdt, n, dev, seed=2)
        keep = adamw.buffers_cpu(base)
        idle, adopt = sgd.clone_ops(base), sgd.clone_ops(base)
        zbuf, zero = la_block(dev, step=4, action=0, born=1, syncs=1)
        obuf, one = la_block(dev, step=3, action=1, born=1, syncs=1)
        z0, o0 = zbuf.cpu().clone(), obuf.cpu().clone()
        assert call(L, stream, idle, n, zero, pdt) == 0 and call(L, stream, adopt, n, one, pdt) == 0, L.cot_last_error()
        sync()
        assert adamw.same(adamw.buffers_cpu(idle), keep), f"action 0 wrote something (n = {n})"
        after = adamw.buffers_cpu(adopt)
        for k in ("param", "master"):
            assert after[k] is None or sgd.same_bits(after[k], keep[k]), f"action 1 wrote {k} (n = {n})"
        fast = fast_of({k: (x[1].cpu() if x is not None else None) for k, x in adopt.items()})
        assert sgd.same_bits(adopt["slow"][1].cpu(), fast.float()), f"action 1 did not copy the fast weights (n = {n})"
        assert sgd.margins_intact(adopt["slow"][0]), f"action 1 wrote a margin (n = {n})"
        assert torch.equal(zbuf.cpu(), z0) and torch.equal(obuf.cpu(), o0), "a block was written"


def check_repeatable(L, dev, stream, pdt, sync=lambda: None):
    base = operands(pdt, 4003, dev, seed=3)
    one, two = sgd.clone_ops(base), sgd.clone_ops(base)
    bbuf, block = la_block(dev, step=6, action=2, born=1, syncs=2)
    for ops in (one, two):
        assert call(L, stream, ops, 4003, block, pdt, alpha=0.3) == 0, L.cot_last_error()
    sync()
    assert adamw.same(adamw.buffers_cpu(one), adamw.buffers_cpu(two)), "two calls on equal data differ"
    assert not adamw.same(adamw.buffers_cpu(one), adamw.buffers_cpu(base))


# ---- cot_lookahead_tick

def tick(L, stream, block, k, force=0, clip=None):
    assert L.cot_lookahead_tick(P(block), clip, k, force, stream) == 0, L.cot_last_error()


def check_tick(L, dev, stream, sync=lambda: None):
    """from zero with k = 3: actions 0 0 1 0 0 2 0, two syncs; k = 1: 1 2 2; a forced tick keeps the count; the words around stay"""
    for k, want in ((3, [0, 0, 1, 0, 0, 2, 0]), (1, [1, 2, 2])):
        bbuf, block = la_block(dev)
        got = []
        for i in range(len(want)):
            tick(L, stream, block, k)
            sync()
            got.append(read_block(block))
        assert [g["action"] for g in got] == want, (k, got)
        assert [g["step"] for g in got] == list(range(1, len(want) + 1))
        assert [g["born"] for g in got] == [1 if any(want[:i + 1]) else 0 for i in range(len(want))]
        last = got[-1]
        assert last["syncs"] == sum(1 for a in want if a) and last["refused"] == 0 and last["reserved"] == [0, 0, 0], last
        assert sentinels_intact(bbuf), "a word next to the block was written"
    # forced (sync_lookahead): unborn adopts, born interpolates, the count stays -- also where step % k == 0 would not sync
    bbuf, block = la_block(dev, step=4)
    tick(L, stream, block, 3, force=1)
    sync()
    assert read_block(block) == dict(step=4, action=1, born=1, syncs=1, refused=0, reserved=[0, 0, 0])
    tick(L, stream, block, 3, force=1)
    sync()
    assert read_block(block) == dict(step=4, action=2, born=1, syncs=2, refused=0, reserved=[0, 0, 0])
    tick(L, stream, block, 3)
    sync()
    assert read_block(block) == dict(step=5, action=0, born=1, syncs=2, refused=0, reserved=[0, 0, 0]) and sentinels_intact(bbuf)


def check_tick_skip(L, dev, stream, sync=lambda: None):
    """behind a clip block that says skip: refused grows, the action BECOMES 0 even when it was 2, the count stays; behind one that
    does not, the tick is the plain one"""
    bbuf, block = la_block(dev, step=5, action=2, born=1, syncs=1)
    cbuf, clip = adamw.clip_block(0.0, 1, dev)
    c0 = cbuf.cpu().clone()
    for i in (1, 2):
        tick(L, stream, block, 3, clip=P(clip))  # (step 6 would have been a sync)
        sync()
        assert read_block(block) == dict(step=5, action=0, born=1, syncs=1, refused=i, reserved=[0, 0, 0])
    tick(L, stream, block, 3, force=1, clip=P(clip))  # a forced tick behind a skip is refused the same way
    sync()
    assert read_block(block) == dict(step=5, action=0, born=1, syncs=1, refused=3, reserved=[0, 0, 0])
    assert torch.equal(cbuf.cpu(), c0), "the tick wrote the clip block"
    okbuf, ok = adamw.clip_block(0.5, 0, dev)
    tick(L, stream, block, 3, clip=P(ok))
    sync()
    assert read_block(block) == dict(step=6, action=2, born=1, syncs=2, refused=3, reserved=[0, 0, 0]) and sentinels_intact(bbuf)


# ---- the recorded fixture

def fixture():
    fix = np.load(GOLDEN)
    k = int(fix["hp"][0])
    n = 4
    out = {"k": k, "alphas": [float(a) for a in fix["alphas"]], "runs": {}}
    for alpha in out["alphas"]:
        tag = f"a{round(alpha * 100)}"
        counts = [int(c) for c in fix[f"{tag}_lookahead_step"]]
        rec = {}
        for t in range(1, len(counts) + 1):
            rec[t] = {a: [torch.from_numpy(fix[f"{tag}_s{t}_{a}{i}"]) for i in range(n)]
                      for a in ("before", "after", "slow", "fast") if f"{tag}_s{t}_{a}0" in fix}
        out["runs"][alpha] = dict(counts=counts, rec=rec)
    return out


def check_fixture_sync(L, dev, stream, alpha, t, sync=lambda: None):
    """the reference's sync at record t (3: the adoption, 6: the first interpolation, 8: the final sync_lookahead) from the recorded
    fast and slow weights.  The four tensors lie in ONE buffer with NaN padding between the slots; the decision comes from
    cot_lookahead_tick on a block as the steps before left it.  alpha 0.5: bit for bit; else the bound plus one rounding of the
    reference's own result.  The padding stays NaN."""
    fx = fixture()
    run, k = fx["runs"][alpha], fx["k"]
    rec = run["rec"][t]
    syncs = [s for s in run["rec"] if "fast" in run["rec"][s]]
    assert syncs == [3, 6, 8] and run["counts"] == [1, 2, 3, 4, 5, 6, 7, 7], (syncs, run["counts"])
    assert all(("slow" in run["rec"][s]) == (s >= k) for s in run["rec"]), "the recorded slow buffers appear at the first sync"
    earlier = [s for s in syncs if s < t]
    order = [1, 0, 2, 3]  # the vector without weight decay first, as FlatSGD's groups are
    fast, slots = adamw.lay_out(rec["fast"], order)
    slow0 = adamw.lay_out(run["rec"][earlier[-1]]["slow"], order)[0] if earlier else torch.zeros_like(fast)
    want_slow, want_fast = adamw.lay_out(rec["slow"], order)[0], adamw.lay_out(rec["after"], order)[0]
    pad = torch.isnan(fast)
    ops = {"param": sgd.margined(fast.to(dev)), "master": None, "slow": sgd.margined(slow0.to(dev))}
    forced = t == 8
    bbuf, block = la_block(dev, step=run["counts"][t - 1] - (0 if forced else 1), born=1 if earlier else 0, syncs=len(earlier))
    tick(L, stream, block, k, force=1 if forced else 0)
    assert call(L, stream, ops, fast.numel(), block, torch.float32, alpha=alpha) == 0, L.cot_last_error()
    sync()
    blk = read_block(block)
    assert (blk["step"], blk["action"], blk["born"], blk["syncs"]) == (run["counts"][t - 1], 2 if earlier else 1, 1, len(earlier) + 1), blk
    assert adamw.margins_ok(ops), "a NaN margin was written"
    got_slow, got_fast = ops["slow"][1].cpu(), ops["param"][1].cpu()
    what = f"fixture alpha {alpha}, record {t}"
    if not earlier:  # the adoption: slow = fast, padding included; the fast weights keep their bits
        assert sgd.same_bits(got_slow, fast) and sgd.same_bits(got_fast, fast), what
        assert torch.equal(got_slow[~pad], want_slow[~pad]) and torch.equal(got_fast[~pad], want_fast[~pad]), what
        return
    for name, got in (("slow", got_slow), ("fast", got_fast)):
        assert bool(torch.isnan(got[pad]).all()) and bool(torch.isfinite(got[~pad]).all()), f"the padding did not stay NaN ({name}, {what})"
    assert sgd.same_bits(got_slow, got_fast), what
    assert torch.equal(want_slow[~pad], want_fast[~pad]), "the fixture's fast weights are not its slow weights after a sync"
    if alpha == 0.5:
        assert torch.equal(got_slow[~pad], want_slow[~pad]), f"alpha 0.5 is exact: not the recorded bits ({what})"
    else:
        ref, E = bound(fast, slow0, alpha)
        # the recorded result within the bound of the formula too (+ its own last rounding): the fixture is what it claims
        judge(want_slow, ref, E, what + ", the fixture against the formula", extra=1.0)
        judge(got_slow, ref, E, what + ", the formula")
        rec64 = torch.where(pad, torch.full_like(ref, float("nan")), want_slow.double())
        judge(got_slow, rec64, E, what + ", against the recorded state", extra=1.0)


# ---- refusals

def check_refusals(L, dev, stream, sync=lambda: None):
    """each refused with its message before any device work: every operand and both blocks stay as they were"""
    pdt, n = torch.bfloat16, 37
    ops = operands(pdt, n, dev, seed=8)
    bbuf, block = la_block(dev, step=6, action=2, born=1, syncs=2)
    cbuf, clip = adamw.clip_block(0.5, 0, dev)
    keep, b0, c0 = adamw.buffers_cpu(ops), bbuf.cpu().clone(), cbuf.cpu().clone()
    v = adamw.views(ops)

    def refused(rc, message, status=-1):
        assert rc == status, (rc, message, L.cot_last_error())
        assert message in L.cot_last_error(), (message, L.cot_last_error())
        sync()
        assert adamw.same(adamw.buffers_cpu(ops), keep) and torch.equal(bbuf.cpu(), b0) and torch.equal(cbuf.cpu(), c0), message

    def odd(t, by):
        return ctypes.c_void_p(t.data_ptr() + by)

    def step(**kw):
        return call(L, stream, ops, kw.pop("n", n), kw.pop("block", block), pdt, **kw)

    for k in ("param", "slow"):
        refused(step(**{k: None}), b"NULL device pointer")
    refused(step(block=None), b"NULL lookahead_state")
    refused(step(param=odd(v["param"], 2)), b"16-byte")
    refused(step(master=odd(v["master"], 4)), b"16-byte")
    refused(step(slow=odd(v["slow"], 8)), b"16-byte")
    refused(step(block=odd(block, 2)), b"lookahead_state")
    refused(step(n=0), b"element count")
    refused(step(n=-4), b"element count")
    for bad in (-0.1, 1.0000001, 2.0, float("nan"), float("inf"), float("-inf")):
        refused(step(alpha=bad), b"alpha")
    refused(step(pcode=_lib.dtype_code(torch.float16)), b"not supported", _lib.COT_ERR_UNSUPPORTED)
    refused(step(pcode=_lib.dtype_code(torch.float64)), b"not supported", _lib.COT_ERR_UNSUPPORTED)
    refused(step(master=None), b"not supported", _lib.COT_ERR_UNSUPPORTED)  # (bf16 parameters need their master)
    refused(step(pcode=_lib.dtype_code(torch.float32)), b"not supported", _lib.COT_ERR_UNSUPPORTED)  # (fp32 parameters take none)
    # the tick
    refused(L.cot_lookahead_tick(None, P(clip), 3, 0, stream), b"NULL lookahead_state")
    refused(L.cot_lookahead_tick(odd(block, 2), P(clip), 3, 0, stream), b"lookahead_state")
    refused(L.cot_lookahead_tick(P(block), odd(clip, 2), 3, 0, stream), b"clip_state")
    for bad in (0, -1, -6):
        refused(L.cot_lookahead_tick(P(block), P(clip), bad, 0, stream), b"lookahead k")
        refused(L.cot_lookahead_tick(P(block), P(clip), bad, 1, stream), b"lookahead k")
    for good in (0.0, 1.0):  # (the ends of the range are values)
        assert step(alpha=good) == 0, L.cot_last_error()
    sync()
    assert not adamw.same(adamw.buffers_cpu(ops), keep)


# ---- the optimizers: adamw_cases.small() under FlatSGD and FlatAdamW

RULES = ["sgd", "adamw"]
RULE_ARRAYS = {"sgd": ("mom",), "adamw": ("exp_avg", "exp_avg_sq")}
K = 3
STEPS = 7


def build(dev, mixed, rule, seed=0, **kw):
    """(model, optimizer): adamw_cases.small() under FlatSGD (nesterov) or FlatAdamW"""
    from cotnet_amd.flat_adamw import FlatAdamW
    from cotnet_amd.flat_sgd import FlatSGD, to_mixed_bf16
    torch.manual_seed(seed)
    model = adamw.small().to(dev).train()
    if mixed:
        to_mixed_bf16(model)
    if rule == "sgd":
        opt = FlatSGD(model, **dict(dict(lr=0.1, momentum=0.9, weight_decay=4e-5, nesterov=True), **kw))
    else:
        opt = FlatAdamW(model, **dict(dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05), **kw))
    assert {b.key for b in opt.reducer.buckets} == {"decay", "no_decay"}
    return model, opt


def weights(opt):
    """clones of the buckets' fp32 weights, whole buckets"""
    return [opt._weights(b, st).detach().clone() for b, st in zip(opt.reducer.buckets, opt.state)]


def rule_state(opt, rule):
    return [st[k].clone() for st in opt.state for k in RULE_ARRAYS[rule]]


def whole_state(model, opt, rule):
    """everything a step, a sync or a load may write, in a fixed order: working copies, fp32 weights, the rule's arrays, the slow
    weights, the blocks, the buffers, the averages"""
    out = [p.detach().clone() for p in model.parameters()] + weights(opt) + rule_state(opt, rule)
    if opt.lookahead_state is not None:
        out += [st["slow"].clone() for st in opt.state] + [opt.lookahead_state.clone()]
    if rule == "adamw":
        out.append(opt.adam_state.clone())
    out += [b.detach().clone() for b in model.buffers()]
    if opt.ema_decay is not None:
        out += [st["ema"].clone() for st in opt.state] + [b.clone() for b in opt._buf_ema]
    if opt.clip_state is not None:
        out.append(opt.clip_state.clone())
    return out


def without_lookahead(sd):
    """our state dict as an optimizer built without Lookahead reads it: no slow_state, no block (the groups' extra keys are ignored)"""
    extra = {k: v for k, v in sd["cotnet_amd"].items() if k != "lookahead"}
    return {"state": sd["state"], "param_groups": sd["param_groups"], "cotnet_amd": extra}


def working_copies_are_rounded(opt):
    return all(st["master"] is None or torch.equal(b.pflat, st["master"].to(b.pflat.dtype)) for b, st in zip(opt.reducer.buckets, opt.state))


def check_twin_protocol(dev, mixed, rule):
    """k = 3, seven steps.  Before each step a plain twin -- built without Lookahead, from other weights -- is loaded from the
    Lookahead optimizer's model and optimizer state, and both take the same batch.  After every step but the 6th (the 3rd included:
    the adoption moves nothing) the two are bit-equal; after the 6th the fp32 weights are s + 0.5 * (twin's weights - s), bit for bit,
    s the slow weights as step 3 left them.  Momentum / moments are the twin's throughout."""
    bs = adamw.batches(dev, mixed, STEPS)
    model, opt = build(dev, mixed, rule, lookahead_k=K)
    tmodel, twin = build(dev, mixed, rule, seed=5)
    assert twin.lookahead_state is None and all("slow" not in st for st in twin.state)
    for t, batch in enumerate(bs, start=1):
        twin.load_model_state_dict(opt.model_state_dict())
        twin.load_state_dict(without_lookahead(opt.state_dict()))
        slow0 = [st["slow"].clone() for st in opt.state]
        adamw.train_step(model, opt, batch)
        adamw.train_step(tmodel, twin, batch)
        what = f"step {t}, {rule}, mixed = {mixed}"
        assert adamw.states_equal(rule_state(opt, rule), rule_state(twin, rule)), f"a sync touched the rule's own state ({what})"
        stats = opt.lookahead_stats()
        assert stats == dict(step=t, born=1 if t >= K else 0, syncs=t // K, refused=0), (what, stats)
        slow = [st["slow"] for st in opt.state]
        if t == 2 * K:
            want = [s.cpu() + 0.5 * (w.cpu() - s.cpu()) for s, w in zip(slow0, weights(twin))]
            assert adamw.states_equal([w.cpu() for w in weights(opt)], want), f"the interpolation is not s + 0.5 (fast - s) ({what})"
            assert not adamw.states_equal(weights(opt), weights(twin)), what
        else:
            assert adamw.states_equal(weights(opt), weights(twin)), f"a non-interpolating step differs from the plain optimizer ({what})"
            assert adamw.states_equal([p.detach() for p in model.parameters()], [p.detach() for p in tmodel.parameters()]), what
        if t % K == 0:
            assert adamw.states_equal(slow, weights(opt)), f"fast is not slow after a sync ({what})"
        elif t < K:
            assert all(not bool(s.any()) for s in slow), f"the slow weights were written before the first sync ({what})"
        else:
            assert adamw.states_equal(slow, slow0), f"a non-sync step wrote the slow weights ({what})"
        assert working_copies_are_rounded(opt), what
        if rule == "adamw":
            assert torch.equal(opt.adam_state, twin.adam_state), what


def check_ema_follows_the_sync(dev, mixed, rule):
    """k = 1, two steps: the second interpolates.  The average after it is ONE cot_ema_step from the average before it on the weights
    AFTER the sync (the launch sits behind the bucket's cot_lookahead_step) -- and not on the ones before it"""
    bs = adamw.batches(dev, mixed, 2)
    model, opt = build(dev, mixed, rule, lookahead_k=1, ema_decay=0.9)
    tmodel, twin = build(dev, mixed, rule, seed=5, ema_decay=0.9)
    adamw.train_step(model, opt, bs[0])
    twin.load_model_state_dict(opt.model_state_dict())
    twin.load_state_dict(without_lookahead(opt.state_dict()))
    twin.load_ema_state_dict(opt.ema_state_dict())
    ema0 = [st["ema"].clone() for st in opt.state]
    assert adamw.states_equal(ema0, [st["ema"] for st in twin.state])
    adamw.train_step(model, opt, bs[1])
    adamw.train_step(tmodel, twin, bs[1])
    assert opt.lookahead_stats()["syncs"] == 2 and not adamw.states_equal(weights(opt), weights(twin))
    L, stream = _lib.api(), _lib.stream()
    for e, w in zip(ema0, weights(opt)):
        L.cot_ema_step(e.data_ptr(), w.data_ptr(), w.numel(), 0.9, _lib.dtype_code(w.dtype), stream)
    assert adamw.states_equal(ema0, [st["ema"] for st in opt.state]), "the average did not follow the weights after the sync"
    assert not adamw.states_equal(ema0, [st["ema"] for st in twin.state]), "the case cannot tell the two orders apart"


def plant_inf(opt):
    b = opt.reducer.buckets[-1]
    opt.reducer.reduced(b)[b.offs[0] + 1] = float("inf")


def check_skipped_step(dev, mixed, rule):
    """an inf planted at what would be step 3 (k = 3), skip_nonfinite=True: no sync, the count stays 2, refused = 1, nothing is born;
    the adoption happens at the next accepted step"""
    bs = adamw.batches(dev, mixed, 4)
    model, opt = build(dev, mixed, rule, lookahead_k=K, skip_nonfinite=True)
    for b in bs[:2]:
        adamw.train_step(model, opt, b)
    before = weights(opt) + rule_state(opt, rule)
    opt.zero_grad()
    adamw.loss_fn(model, bs[2]).backward()
    plant_inf(opt)
    opt.step()
    assert opt.lookahead_stats() == dict(step=2, born=0, syncs=0, refused=1)
    assert int(opt.lookahead_state[1]) == 0 and all(not bool(st["slow"].any()) for st in opt.state)
    assert adamw.states_equal(weights(opt) + rule_state(opt, rule), before), "a skipped step wrote weights, momentum or moments"
    adamw.train_step(model, opt, bs[3])
    assert opt.lookahead_stats() == dict(step=3, born=1, syncs=1, refused=1)
    assert adamw.states_equal([st["slow"] for st in opt.state], weights(opt)), "the adoption did not happen at the next accepted step"


def check_sync_lookahead(dev, mixed, rule):
    """unborn: it adopts and no weight moves; born: it interpolates without counting a step; momentum / moments stay"""
    bs = adamw.batches(dev, mixed, 2)
    model, opt = build(dev, mixed, rule, lookahead_k=K)
    adamw.train_step(model, opt, bs[0])
    w0, r0, p0 = weights(opt), rule_state(opt, rule), [p.detach().clone() for p in model.parameters()]
    opt.sync_lookahead()
    assert opt.lookahead_stats() == dict(step=1, born=1, syncs=1, refused=0)
    assert adamw.states_equal(weights(opt), w0) and adamw.states_equal([p.detach() for p in model.parameters()], p0)
    assert adamw.states_equal([st["slow"] for st in opt.state], w0), "an unborn sync_lookahead() did not adopt"
    adamw.train_step(model, opt, bs[1])
    w1, r1 = weights(opt), rule_state(opt, rule)
    assert opt.lookahead_stats() == dict(step=2, born=1, syncs=1, refused=0) and not adamw.states_equal(w1, w0)
    opt.sync_lookahead()
    assert opt.lookahead_stats() == dict(step=2, born=1, syncs=2, refused=0), "sync_lookahead() counted a step"
    want = [s.cpu() + 0.5 * (w.cpu() - s.cpu()) for s, w in zip(w0, w1)]
    assert adamw.states_equal([w.cpu() for w in weights(opt)], want) and adamw.states_equal([st["slow"] for st in opt.state], weights(opt))
    assert adamw.states_equal(rule_state(opt, rule), r1) and not adamw.states_equal(r1, r0) and working_copies_are_rounded(opt)
    # built without Lookahead the method is there and returns at once
    model, plain = build(dev, mixed, rule)
    adamw.train_step(model, plain, bs[0])
    w = weights(plain)
    assert plain.sync_lookahead() is None and adamw.states_equal(weights(plain), w)


def addresses(opt, rule):
    return [opt.lookahead_state.data_ptr()] + [st[k].data_ptr() for st in opt.state for k in ("slow",) + RULE_ARRAYS[rule]]


def check_layout(sd, opt, model, born, step):
    """section 3's layout: the reference's key order, index-keyed slow_state, the three keys in every group, the block's words"""
    assert list(sd) == ["state", "slow_state", "param_groups", "cotnet_amd"]
    members = [p for g in opt._groups() for _, p in g]
    assert list(sd["slow_state"]) == list(range(len(members))) == [i for g in sd["param_groups"] for i in g["params"]]
    slow = opt._slots("slow")
    for i, p in enumerate(members):
        if born:
            buf = sd["slow_state"][i]["slow_buffer"]
            assert list(sd["slow_state"][i]) == ["slow_buffer"] and buf.dtype == torch.float32 and buf.shape == p.shape
            assert torch.equal(buf, slow[p]) and buf.data_ptr() != slow[p].data_ptr()
        else:
            assert sd["slow_state"][i] == {}
    for g in sd["param_groups"]:
        assert (g["lookahead_alpha"], g["lookahead_k"], g["lookahead_step"]) == (opt.lookahead_alpha, opt.lookahead_k, step)
    words = sd["cotnet_amd"]["lookahead"]
    assert words == opt.lookahead_state.cpu().tolist() and len(words) == 8 and (words[0], words[2]) == (step, 1 if born else 0)


def torch_loads(sd, model, opt, rule):
    """torch.optim.SGD / AdamW over the same groups of an fp32 twin load 'state' + 'param_groups' of our dict"""
    twin = copy.deepcopy(model).float().cpu()
    names = [[n for n, _ in g] for g in opt._groups()]
    params = dict(twin.named_parameters())
    groups = [dict(params=[params[n] for n in names[0]]), dict(params=[params[n] for n in names[1]])]
    ref = torch.optim.SGD(groups, lr=1.0, momentum=0.5) if rule == "sgd" else torch.optim.AdamW(groups, lr=1.0)
    ref.load_state_dict({"state": {k: {a: (v.cpu() if torch.is_tensor(v) else v) for a, v in s.items()} for k, s in sd["state"].items()},
                         "param_groups": sd["param_groups"]})
    assert all(g["lr"] == opt.lr and g["lookahead_k"] == opt.lookahead_k for g in ref.param_groups)
    key = "momentum_buffer" if rule == "sgd" else "exp_avg"
    ours = opt._slots(RULE_ARRAYS[rule][0])
    for q, p in zip([q for g in ref.param_groups for q in g["params"]], [p for g in opt._groups() for _, p in g]):
        assert torch.equal(ref.state[q][key], ours[p].cpu())


def check_checkpoint(dev, mixed, rule, at, captured=None, tmp_path=None, **kw):
    """saved after step `at` (2: unborn, 4: born), through state_dict / model_state_dict -- or, tmp_path given, CheckpointSaver /
    resume_checkpoint -- into a fresh optimizer built from other weights (captured(model, opt) -> step function given: one whose step
    was captured before the load): the remaining steps to 7 are bit-equal to the uninterrupted run, the whole block included"""
    import pytest
    bs = adamw.batches(dev, mixed, STEPS)
    model, opt = build(dev, mixed, rule, lookahead_k=K, ema_decay=0.9, **kw)
    for b in bs[:at]:
        adamw.train_step(model, opt, b)
    born = at >= K
    if tmp_path is None:
        sd, msd, esd = opt.state_dict(), opt.model_state_dict(), opt.ema_state_dict()
        check_layout(sd, opt, model, born, at)
        torch_loads(sd, model, opt, rule)
    else:
        from cotnet_amd import CheckpointSaver, resume_checkpoint
        saver = CheckpointSaver(model, opt, checkpoint_dir=str(tmp_path), recovery_dir=str(tmp_path))
        saver.save_checkpoint(1, metric=0.5)
    for b in bs[at:]:
        adamw.train_step(model, opt, b)
    want = whole_state(model, opt, rule)
    assert opt.lookahead_stats() == dict(step=STEPS, born=1, syncs=2, refused=0)
    fresh, fopt = build(dev, mixed, rule, seed=5, lookahead_k=K, ema_decay=0.9, **dict(kw, lr=0.5))
    step = (lambda b: adamw.train_step(fresh, fopt, b)) if captured is None else captured(fresh, fopt)
    if captured is not None:
        for key, value in (("lookahead_k", 2), ("lookahead_alpha", 0.25)):
            with pytest.raises(ValueError, match="captured into a HIP graph with \\(lookahead_k, lookahead_alpha\\)"):
                fopt.load_state_dict(dict(sd, param_groups=[dict(g, **{key: value}) for g in sd["param_groups"]]))
    held = addresses(fopt, rule)
    if tmp_path is None:
        fopt.load_model_state_dict(msd)
        fopt.load_state_dict(sd)
        fopt.load_ema_state_dict(esd)
    else:
        assert resume_checkpoint(fresh, str(tmp_path / "checkpoint-1.pth.tar"), optimizer=fopt, log_info=False) == 1
    assert held == addresses(fopt, rule), "a load moved an allocation"
    assert fopt.lr == opt.lr and fopt.lookahead_stats() == dict(step=at, born=1 if born else 0, syncs=1 if born else 0, refused=0)
    for b in bs[at:]:
        step(b)
    diff = adamw.differing(want, whole_state(fresh, fopt, rule))
    assert not diff, ("resumed and uninterrupted runs differ", diff)


def check_load_refusals(dev, mixed, rule):
    """what load_state_dict refuses of Lookahead's part, each before anything is written; and what it accepts without slow_state"""
    import pytest
    bs = adamw.batches(dev, mixed, 4)
    model, opt = build(dev, mixed, rule, lookahead_k=K)
    for b in bs:
        adamw.train_step(model, opt, b)
    sd = opt.state_dict()
    fresh, fopt = build(dev, mixed, rule, seed=5, lookahead_k=K)
    adamw.train_step(fresh, fopt, bs[0])
    before = whole_state(fresh, fopt, rule)

    def refused(target, tmodel, d, match, keep):
        with pytest.raises(ValueError, match=match):
            target.load_state_dict(d)
        assert adamw.states_equal(keep, whole_state(tmodel, target, rule)), f"a refused load wrote something ({match})"

    members = [p for g in opt._groups() for _, p in g]
    by_id = dict(sd, slow_state={id(p): v for p, v in zip(members, sd["slow_state"].values())})
    refused(fopt, fresh, by_id, "id\\(tensor\\)", before)
    refused(fopt, fresh, dict(sd, slow_state={k: v for k, v in sd["slow_state"].items() if k != 0}), "keyed by", before)
    bad = copy.deepcopy(sd)
    bad["slow_state"][3]["slow_buffer"] = torch.zeros(3, 3)
    refused(fopt, fresh, bad, "slow_buffer of index 3 has shape", before)
    bad = copy.deepcopy(sd)
    bad["slow_state"][1] = {}
    refused(fopt, fresh, bad, "some indices and none for others", before)
    for key, value in (("lookahead_step", 5), ("lookahead_k", 4), ("lookahead_alpha", 0.25)):
        groups = [dict(sd["param_groups"][0]), dict(sd["param_groups"][1], **{key: value})]
        refused(fopt, fresh, dict(sd, param_groups=groups), f"the groups' {key} are", before)
    for key, value, match in (("lookahead_k", 0, "lookahead_k=0"), ("lookahead_alpha", 1.5, "lookahead_alpha=1.5")):
        refused(fopt, fresh, dict(sd, param_groups=[dict(g, **{key: value}) for g in sd["param_groups"]]), match, before)
    # into an optimizer built without Lookahead: refused, naming the keyword -- with slow_state, and with the block alone
    pmodel, plain = build(dev, mixed, rule, seed=6)
    pkeep = whole_state(pmodel, plain, rule)
    refused(plain, pmodel, sd, "lookahead_k", pkeep)
    refused(plain, pmodel, {k: v for k, v in sd.items() if k != "slow_state"}, "lookahead_k", pkeep)
    # a checkpoint without Lookahead loads unborn, the count from the groups' lookahead_step, or 0
    plain_sd = without_lookahead(sd)
    fopt.load_state_dict(plain_sd)
    assert fopt.lookahead_stats() == dict(step=4, born=0, syncs=0, refused=0) and all(not bool(st["slow"].any()) for st in fopt.state)
    bare = dict(plain_sd, param_groups=[{k: v for k, v in g.items() if not k.startswith("lookahead_")} for g in plain_sd["param_groups"]])
    fopt.load_state_dict(bare)
    assert fopt.lookahead_stats() == dict(step=0, born=0, syncs=0, refused=0) and (fopt.lookahead_k, fopt.lookahead_alpha) == (K, 0.5)
    # the whole dict loads, k and alpha following the checkpoint where nothing was captured
    other, oopt = build(dev, mixed, rule, seed=7, lookahead_k=5, lookahead_alpha=0.25)
    oopt.load_state_dict(sd)
    assert (oopt.lookahead_k, oopt.lookahead_alpha) == (K, 0.5) and torch.equal(oopt.lookahead_state, opt.lookahead_state)
    assert adamw.states_equal([st["slow"] for st in oopt.state], [st["slow"] for st in opt.state])
