"""Gradient clipping by global norm on the device (csrc/grad_clip.hip: cot_grad_sumsq, cot_grad_clip_finish; optim.hip: cot_sgd_step_clip):
the cases and criteria that tests/test_grad_clip_emulated.py runs on the host emulator and tests/test_grad_clip_gpu.py on the device.

The norm's bound is DERIVED, not measured.  Every term of a sum of squares is >= 0, so the relative error of the fp32 partial sums is at
most (d + 1) * u, u = 2^-24, where d = chain_length(n, V, parts) is the longest chain of fp32 additions one square passes through (the
loop structure stated at the top of grad_clip.hip) and the + 1 is the square's own rounding; the square root halves it; the fp64 finish,
the root and the rounding of the root to fp32 are covered by + 2:

    |norm - ref| <= ((d + 1) / 2 + 2) * u * ref,    ref = sqrt(sum(g.double() ** 2)) of the stored values.

Operands are views into buffers with NaN margins (tests/sgd_lr_cases.py), which must stay NaN."""
import math
import os

import numpy as np
import torch

from cotnet_amd import _lib
from tests import sgd_lr_cases as sgd

P = sgd.P
U = 2.0 ** -24
BLOCK = 256  # lanes per workgroup of cot_grad_sumsq
GRAD_DTYPES = [torch.float32, torch.bfloat16]
GRAD_IDS = ["f32", "bf16"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grad_clip.npz")
CLIP_COEFS = [1.0, 0.5, 0.02751363255083561]  # the last one is a double that is no fp32 value


def vec(gdt):
    """elements per 16-byte load of a lane"""
    return 16 // torch.empty((), dtype=gdt).element_size()


def chain_length(n, V, parts):
    """the longest chain of fp32 additions a square passes through (grad_clip.hip, "The chain")"""
    rounds = -(-(n // V) // (parts * BLOCK))  # a lane's sequential adds, one sum per vector slot
    return rounds + int(math.log2(V)) + 1 + 6 + 3  # + the slots pairwise, the tail element, the wave's stages (cot_reduce.h: wave_allsum), the four waves


def norm_bound(n, V, parts):
    """relative; see the module docstring"""
    return ((chain_length(n, V, parts) + 1) / 2 + 2) * U


def sizes(parts, V):
    """tail only, body only, body + tail, a few workgroups, one full sweep of the grid minus one element, one full sweep plus a tail
    and a second round, and 2^20 + 5 -- the issue's list is stated for V = 4; with 8 elements per load the same places are added"""
    out = [1, 3, 4, 5, 4003, parts * BLOCK * 4 - 1, parts * BLOCK * 4 + 5, 2 ** 20 + 5]
    if V == 8:
        out += [7, 8, 9, parts * BLOCK * 8 - 1, parts * BLOCK * 8 + 5]
    return sorted(set(out))


def share(n, V, parts):
    """indices of the workgroups that own at least one element of a bucket of n"""
    nvec = n // V
    own = set(range(min(parts, -(-nvec // BLOCK))))
    if n % V:
        own.add(0)
    return own


def owner(e, n, V, parts):
    """the workgroup that reads element e"""
    if e >= (n // V) * V:
        return 0
    return ((e // V) % (parts * BLOCK)) // BLOCK


def gradient(n, gdt, dev, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(1000 * seed + n % 997)
    return (scale * torch.randn(n, generator=g)).to(gdt).to(dev)


def new_partials(dev, count):
    """(buffer, view): `count` floats of NaN inside NaN margins -- every one of them has to be written"""
    return sgd.margined(torch.full((count,), float("nan"), dtype=torch.float32, device=dev))


def new_state(dev, scale=0.0, skip=0, fill=0):
    st = torch.full((8,), fill, dtype=torch.int32, device=dev)
    if fill == 0:
        st[0:1].view(torch.float32)[0] = scale
        st[2] = skip
    return st


def read_state(st):
    w = st.cpu()
    scale, norm = w[:2].view(torch.float32)
    return dict(scale=scale.clone(), total_norm=norm.clone(), skip=int(w[2]), steps=int(w[3]), clipped=int(w[4]), skipped=int(w[5]),
                reserved=(int(w[6]), int(w[7])))


def coefficient(total_norm, max_norm):
    """torch's clip_grad_norm_ formula in fp32, from an fp32 0-dim tensor"""
    c = torch.tensor(max_norm, dtype=torch.float32) / (total_norm + torch.tensor(1e-6, dtype=torch.float32))
    return torch.where(c < 1, c, torch.ones_like(c))


def run_norm(L, stream, grads, partials, state, max_norm):
    """cot_grad_sumsq per gradient into consecutive slices of `partials`, then cot_grad_clip_finish"""
    parts = L.cot_grad_norm_parts()
    assert partials.numel() == parts * len(grads)
    for i, g in enumerate(grads):
        rc = L.cot_grad_sumsq(P(g), g.numel(), _lib.dtype_code(g.dtype), P(partials[i * parts:(i + 1) * parts]), stream)
        assert rc == 0, L.cot_last_error()
    rc = L.cot_grad_clip_finish(P(partials), partials.numel(), max_norm, P(state), stream)
    assert rc == 0, L.cot_last_error()


def reference_norm(grads):
    return math.sqrt(sum(float(g.double().square().sum()) for g in grads))


def check_norm(L, dev, stream, gdt, n, sync=lambda: None):
    """norm within the derived bound, coefficient bit-equal to the formula, workgroups without a share write 0, two calls equal bits,
    nothing but the partials and the block written"""
    parts, V = L.cot_grad_norm_parts(), vec(gdt)
    bound = norm_bound(n, V, parts)
    assert bound < 2e-6, (n, V, chain_length(n, V, parts))  # else the structure has too long a serial chain
    gbuf, g = sgd.margined(gradient(n, gdt, dev))
    keep = gbuf.clone()
    ref = reference_norm([g])
    max_norm = float(np.float32(0.5 * ref))  # clips
    runs = []
    for _ in range(2):
        pbuf, pv = new_partials(dev, parts)
        st = new_state(dev)
        run_norm(L, stream, [g], pv, st, max_norm)
        runs.append((pbuf, pv, st))
    sync()
    (pbuf, pv, st), (pbuf2, _, st2) = runs
    what = f"n = {n}, {gdt}"
    assert sgd.same_bits(pbuf, pbuf2) and torch.equal(st, st2), f"two calls on the same data differ ({what})"
    assert sgd.margins_intact(pbuf) and bool(torch.isfinite(pv).all()), f"partials: a margin written or a partial left unwritten ({what})"
    assert sgd.same_bits(gbuf, keep), f"the gradient was written ({what})"
    idle = [i for i in range(parts) if i not in share(n, V, parts)]
    assert bool((pv.cpu()[idle] == 0).all()), f"a workgroup without a share wrote something else than 0 ({what})"
    s = read_state(st)
    err = abs(float(s["total_norm"]) - ref) / ref
    print(f"{what}: chain {chain_length(n, V, parts)}, |norm - ref| / ref = {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (what, err, bound)
    assert torch.equal(s["scale"], coefficient(s["total_norm"], max_norm)), (what, s)
    assert float(s["scale"]) < 1 and (s["skip"], s["steps"], s["clipped"], s["skipped"], s["reserved"]) == (0, 1, 1, 0, (0, 0)), (what, s)


def check_zero_gradient(L, dev, stream, gdt, sync=lambda: None):
    parts = L.cot_grad_norm_parts()
    g = torch.zeros(4003, dtype=gdt, device=dev)
    pbuf, pv = new_partials(dev, parts)
    st = new_state(dev)
    run_norm(L, stream, [g], pv, st, 1.0)
    sync()
    s = read_state(st)
    assert float(s["total_norm"]) == 0.0 and float(s["scale"]) == 1.0, s
    assert (s["skip"], s["steps"], s["clipped"], s["skipped"]) == (0, 1, 0, 0), s
    assert bool((pv == 0).all()) and sgd.margins_intact(pbuf)


NONFINITE = ["inf-first", "nan-last-of-body", "nan-in-tail", "minus-inf", "bf16-overflowing-squares"]


def check_nonfinite(L, dev, stream, kind, gdt, sync=lambda: None):
    """skip = 1, scale = 0, `skipped` advances, the untouched workgroups' partials stay finite -- and the next, finite call clears skip"""
    parts, V = L.cot_grad_norm_parts(), vec(gdt)
    n = 4003  # a body of several workgroups and a tail of three
    g = gradient(n, gdt, dev, seed=2)
    body = (n // V) * V
    if kind == "inf-first":
        where, value = [0], float("inf")
    elif kind == "nan-last-of-body":
        where, value = [body - 1], float("nan")
    elif kind == "nan-in-tail":
        where, value = [n - 1], float("nan")
    elif kind == "minus-inf":
        where, value = [1500], float("-inf")
    else:
        assert gdt == torch.bfloat16
        where, value = [16, 17, 2000], 3e38  # finite elements whose squares overflow fp32
    clean = g.clone()
    g[where] = value
    assert kind != "bf16-overflowing-squares" or bool(torch.isfinite(g).all())
    pbuf, pv = new_partials(dev, parts)
    st = new_state(dev)
    run_norm(L, stream, [g], pv, st, 1.0)
    sync()
    s = read_state(st)
    assert (s["skip"], float(s["scale"]), s["steps"], s["clipped"], s["skipped"]) == (1, 0.0, 1, 0, 1), (kind, s)
    assert not math.isfinite(float(s["total_norm"])), (kind, s)
    touched = {owner(e, n, V, parts) for e in where}
    bad = {i for i, ok in enumerate(torch.isfinite(pv).tolist()) if not ok}
    assert bad == touched, f"{kind}: non-finite partials of workgroups {sorted(bad)}, the value sits in {sorted(touched)}"
    assert sgd.margins_intact(pbuf)
    run_norm(L, stream, [clean], pv, st, float("inf"))  # guard only
    sync()
    s = read_state(st)
    assert (s["skip"], float(s["scale"]), s["steps"], s["clipped"], s["skipped"]) == (0, 1.0, 2, 0, 1), (kind, s)


def check_several_buckets(L, dev, stream, sync=lambda: None):
    """three buckets of two dtypes in one partials array: the joint norm; a NaN only in the last bucket skips"""
    parts = L.cot_grad_norm_parts()
    shapes = [(4003, torch.float32), (1001, torch.bfloat16), (5, torch.float32)]
    grads = [gradient(n, dt, dev, seed=3 + i, scale=10.0 ** -i) for i, (n, dt) in enumerate(shapes)]
    bound = max(norm_bound(n, vec(dt), parts) for n, dt in shapes)  # every bucket's sum is within its own bound, so is their sum
    ref = reference_norm(grads)
    pbuf, pv = new_partials(dev, parts * len(grads))
    st = new_state(dev)
    max_norm = float(np.float32(2.0 * ref))  # does not clip
    run_norm(L, stream, grads, pv, st, max_norm)
    sync()
    s = read_state(st)
    err = abs(float(s["total_norm"]) - ref) / ref
    print(f"three buckets: |norm - ref| / ref = {err:.3e}, bound {bound:.3e}")
    assert err <= bound and sgd.margins_intact(pbuf) and bool(torch.isfinite(pv).all())
    single = reference_norm(grads[:1])
    assert abs(float(s["total_norm"]) - single) / single > 100 * bound  # (the other buckets do count)
    assert torch.equal(s["scale"], coefficient(s["total_norm"], max_norm)) and float(s["scale"]) == 1.0
    assert (s["skip"], s["steps"], s["clipped"], s["skipped"]) == (0, 1, 0, 0), s
    grads[-1][4] = float("nan")
    run_norm(L, stream, grads, pv, st, max_norm)
    sync()
    s = read_state(st)
    assert (s["skip"], float(s["scale"]), s["steps"], s["skipped"]) == (1, 0.0, 2, 1), s
    assert bool(torch.isfinite(pv[:2 * parts]).all())


def check_counters(L, dev, stream, sync=lambda: None):
    """a scripted sequence of clipped, unclipped and skipped steps; the reserved words are written 0"""
    parts = L.cot_grad_norm_parts()
    g = gradient(4003, torch.float32, dev, seed=5)
    bad = g.clone()
    bad[77] = float("nan")
    ref = reference_norm([g])
    _, pv = new_partials(dev, parts)
    st = new_state(dev)
    st[6:] = 7  # (garbage in the reserved words)
    script = [(g, 0.5 * ref, "clipped"), (g, 2 * ref, "unclipped"), (bad, 0.5 * ref, "skipped"), (g, float("inf"), "unclipped"),
              (bad, float("inf"), "skipped"), (g, 0.25 * ref, "clipped")]
    want = dict(clipped=0, unclipped=0, skipped=0)
    for i, (grad, max_norm, kind) in enumerate(script):
        run_norm(L, stream, [grad], pv, st, float(np.float32(max_norm)))
        sync()
        want[kind] += 1
        s = read_state(st)
        assert (s["steps"], s["clipped"], s["skipped"], s["reserved"]) == (i + 1, want["clipped"], want["skipped"], (0, 0)), (i, kind, s)
        assert s["skip"] == (kind == "skipped") and (float(s["scale"]) < 1) == (kind != "unclipped"), (i, kind, s)
        if kind != "skipped":
            assert torch.equal(s["scale"], coefficient(s["total_norm"], float(np.float32(max_norm)))), (i, kind, s)


def sgd_clip_call(L, ops, n, lr, lr_dev, state, nesterov, pdt, gdt, stream, momentum=sgd.MU, wd=sgd.WD, gs=sgd.GS):
    v = {k: (x[1] if x is not None else None) for k, x in ops.items()}
    return L.cot_sgd_step_clip(P(v["param"]), P(v["master"]), P(v["mom"]), P(v["grad"]), n, lr, lr_dev, state, momentum, wd, gs, nesterov,
                               _lib.dtype_code(pdt), _lib.dtype_code(gdt), stream)


def check_sgd_clip(L, dev, stream, pdt, gdt, nesterov, ns, sync=lambda: None):
    """a block {scale = c, skip = 0} equals today's entry points with grad_scale' = fp32(grad_scale * c) (c = 1: the unclipped step);
    skip = 1 leaves everything as it was -- for both rate sources"""
    lr = 0.24987413835233163
    for n in ns:
        base = sgd.operands(pdt, gdt, n, dev)
        rate = torch.tensor([lr], dtype=torch.float32).to(dev)
        for by_dev in (False, True):
            for c in CLIP_COEFS:
                what = f"n = {n}, c = {c!r}, lr_dev {by_dev}"
                want, got = sgd.clone_ops(base), sgd.clone_ops(base)
                c32 = torch.tensor(c, dtype=torch.float32)
                gs = float(torch.tensor(sgd.GS, dtype=torch.float32) * c32)
                assert c != 1.0 or gs == sgd.GS
                if by_dev:
                    assert sgd.call(L, "cot_sgd_step_lr", want, n, P(rate), nesterov, pdt, gdt, stream, gs=gs) == 0, L.cot_last_error()
                else:
                    assert sgd.call(L, "cot_sgd_step", want, n, lr, nesterov, pdt, gdt, stream, gs=gs) == 0, L.cot_last_error()
                st = new_state(dev, scale=float(c32), skip=0)
                st0 = st.clone()
                # (with lr_dev given, `lr` is ignored: hand over another number)
                rc = sgd_clip_call(L, got, n, 123.0 if by_dev else lr, P(rate) if by_dev else None, P(st), nesterov, pdt, gdt, stream)
                assert rc == 0, L.cot_last_error()
                sync()
                for k in ("param", "master", "mom"):
                    if base[k] is None:
                        continue
                    assert torch.equal(want[k][1], got[k][1]), f"{k} differs from today's entry point ({what})"
                    assert sgd.margins_intact(got[k][0]), f"{k}: a NaN margin was written ({what})"
                k = "master" if base["master"] is not None else "param"
                assert not torch.equal(got[k][1], base[k][1]), f"the step moved nothing ({what})"
                assert sgd.same_bits(got["grad"][0], base["grad"][0]) and torch.equal(st, st0), f"gradient or block written ({what})"
            skipped = sgd.clone_ops(base)
            st = new_state(dev, scale=0.5, skip=1)  # (the flag is what counts, not a zero coefficient)
            st0 = st.clone()
            rc = sgd_clip_call(L, skipped, n, lr, P(rate) if by_dev else None, P(st), nesterov, pdt, gdt, stream)
            assert rc == 0, L.cot_last_error()
            sync()
            for k in ("param", "master", "mom", "grad"):
                if base[k] is not None:
                    assert sgd.same_bits(skipped[k][0], base[k][0]), f"{k} was written by a skipped step (n = {n}, lr_dev {by_dev})"
                    assert sgd.margins_intact(skipped[k][0])
            assert torch.equal(st, st0) and torch.equal(rate.cpu(), torch.tensor([lr], dtype=torch.float32))


def check_fixture(L, dev, stream, sync=lambda: None):
    """the reference's dispatch_clip_grad(mode='norm') as recorded (tests/golden/make_golden_clip.py): its total_norm and its clipped
    gradients within the derived bound plus one fp32 rounding.  The three tensors are three buckets; the clipped gradient is read off
    a step with p = 0, no momentum, no decay and lr = 1: p' = -(g * scale)."""
    fix = np.load(GOLDEN)
    parts = L.cot_grad_norm_parts()
    worst = 0.0
    for name in sorted({k.split("__")[0] for k in fix.files}):
        grads = [torch.from_numpy(fix[f"{name}__g{i}"]).reshape(-1).to(dev) for i in range(3)]
        tol = max(norm_bound(g.numel(), 4, parts) for g in grads) + U
        ref = float(fix[f"{name}__total_norm"])
        for j, max_norm in enumerate(fix[f"{name}__max_norms"].tolist()):
            _, pv = new_partials(dev, 3 * parts)
            st = new_state(dev)
            run_norm(L, stream, grads, pv, st, max_norm)
            outs = []
            for g in grads:
                p, mom = torch.zeros_like(g), torch.zeros_like(g)
                rc = L.cot_sgd_step_clip(P(p), None, P(mom), P(g), g.numel(), 1.0, None, P(st), 0.0, 0.0, 1.0, 0, _lib.COT_F32, _lib.COT_F32,
                                         stream)
                assert rc == 0, L.cot_last_error()
                outs.append(p)
            sync()
            s = read_state(st)
            err = abs(float(s["total_norm"]) - ref) / ref
            worst = max(worst, err)
            assert err <= tol, (name, max_norm, err, tol)
            clips = max_norm < ref
            assert (float(s["scale"]) < 1) == clips and s["clipped"] == int(clips), (name, max_norm, s)
            for i, p in enumerate(outs):
                want = torch.from_numpy(fix[f"{name}__clipped{j}_g{i}"]).reshape(-1)
                got = -p.cpu()
                e = float(((got - want).abs() / want.abs().clamp_min(1e-30)).max())
                worst = max(worst, e)
                if not clips:
                    assert torch.equal(got, want), (name, max_norm, i)
                assert e <= tol, (name, max_norm, i, e, tol)
    print(f"fixture: worst relative difference {worst:.3e}, allowance {tol:.3e}")


def check_refusals(L, dev, stream, sync=lambda: None):
    """each refused with its message before any device work: the operands, the partials and the block stay as they were"""
    parts = L.cot_grad_norm_parts()
    pdt = gdt = torch.bfloat16
    n = 37
    ops = sgd.operands(pdt, gdt, n, dev)
    keep = sgd.clone_ops(ops)
    g = ops["grad"][1]
    pbuf, pv = new_partials(dev, parts + 1)
    st = new_state(dev, fill=5)
    rate = torch.tensor([0.1], dtype=torch.float32).to(dev)

    def untouched():
        sync()
        return (all(sgd.same_bits(ops[k][0], keep[k][0]) for k in ops) and bool(torch.isnan(pbuf).all()) and bool((st == 5).all())
                and rate.item() == torch.tensor(0.1, dtype=torch.float32).item())

    def refused(rc, message, status=-1):
        assert rc == status, (rc, L.cot_last_error())
        assert message in L.cot_last_error(), L.cot_last_error()
        assert untouched(), message

    def odd(t, by=2):
        import ctypes
        return ctypes.c_void_p(t.data_ptr() + by)

    code = _lib.dtype_code
    # cot_grad_sumsq
    refused(L.cot_grad_sumsq(None, n, code(gdt), P(pv), stream), b"NULL")
    refused(L.cot_grad_sumsq(P(g), n, code(gdt), None, stream), b"NULL partials")
    refused(L.cot_grad_sumsq(P(g), n, code(gdt), odd(pv), stream), b"4-byte aligned")
    refused(L.cot_grad_sumsq(P(g[1:]), n - 1, code(gdt), P(pv), stream), b"16-byte")
    refused(L.cot_grad_sumsq(P(g), 0, code(gdt), P(pv), stream), b"element count")
    refused(L.cot_grad_sumsq(P(g), n, code(torch.float16), P(pv), stream), b"dtype", _lib.COT_ERR_UNSUPPORTED)
    # cot_grad_clip_finish
    refused(L.cot_grad_clip_finish(None, parts, 1.0, P(st), stream), b"NULL partials")
    refused(L.cot_grad_clip_finish(P(pv), parts, 1.0, None, stream), b"NULL clip_state")
    refused(L.cot_grad_clip_finish(odd(pv), parts, 1.0, P(st), stream), b"4-byte aligned")
    refused(L.cot_grad_clip_finish(P(pv), parts, 1.0, odd(st), stream), b"4-byte aligned")
    refused(L.cot_grad_clip_finish(P(pv), 0, 1.0, P(st), stream), b"partial count")
    for bad in (0.0, -1.0, float("nan"), float("-inf")):
        refused(L.cot_grad_clip_finish(P(pv), parts, bad, P(st), stream), b"max_norm")
    # cot_sgd_step_clip
    refused(sgd_clip_call(L, ops, n, 0.1, None, None, 1, pdt, gdt, stream), b"NULL clip_state")
    refused(sgd_clip_call(L, ops, n, 0.1, None, odd(st), 1, pdt, gdt, stream), b"clip_state")
    refused(sgd_clip_call(L, ops, n, 0.1, odd(rate), P(st), 1, pdt, gdt, stream), b"lr_dev")
    refused(sgd_clip_call(L, ops, 0, 0.1, None, P(st), 1, pdt, gdt, stream), b"element count")
    refused(sgd_clip_call(L, ops, n, 0.1, None, P(st), 1, torch.float16, gdt, stream), b"not supported", _lib.COT_ERR_UNSUPPORTED)
    refused(sgd_clip_call(L, dict(ops, master=None), n, 0.1, None, P(st), 1, pdt, gdt, stream), b"master", _lib.COT_ERR_UNSUPPORTED)
    misaligned = dict(ops, mom=(ops["mom"][0], ops["mom"][1][1:]))
    refused(sgd_clip_call(L, misaligned, n - 1, 0.1, None, P(st), 1, pdt, gdt, stream), b"16-byte")
