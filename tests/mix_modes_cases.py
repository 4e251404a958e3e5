"""cot_mix_normalize and cot_soft_target_ce_* reading a TABLE block (header `mode 3, R` + R records, include/cotnet_amd.h) through the C ABI,
against the reference's own `FastCollateMixup(mode='elem' | 'pair')` results (tests/golden/mix_modes.npz, written by
tests/golden/make_golden_mix_modes.py): what tests/test_mix_modes_emulated.py runs on the host emulator and tests/test_mix_modes_gpu.py on
the device.  The helpers and the criteria are tests/mix_loss_cases.py's:

Mixing: the kernel's output equals normalize_uint8's arithmetic applied to the reference's mixed uint8 batch, bit for bit, inside NaN margins.
Loss: against the reference in fp64, allowance = 4 x the reference's own fp32-versus-fp64 error from the fixture, per quantity.

The blocks are built HERE from the fixture's per-sample (lam, use_cutmix, box) by the header's rule -- `table()` below, not the package's
packer -- so the kernels are held to the documented format; tests/test_mix_modes_host_cpu.py holds the package's packer to the same words.
"""
import json

import numpy as np
import torch

from cotnet_amd import _lib
from tests import footprint_cases as fp
from tests.conftest import load_golden
from tests.mix_loss_cases import MEAN, P, STD, allowances, check_bf16_grad, compare, loss, margined, mix, normalized

GOLD = load_golden("mix_modes")
META = json.loads(str(GOLD["meta"]))
CASES = sorted(META)
SENTINEL = 0x7fffffff


def gold(name, key):
    return torch.from_numpy(GOLD[f"{name}__{key}"])


def record(mode, lam, oml, box=(0, 0, 0, 0)):
    w = np.zeros(8, dtype=np.int32)
    w[0] = mode
    w[1:3] = np.array([lam, oml], dtype=np.float32).view(np.int32)
    w[3:7] = box
    return w


def table(lam, cut, boxes, R=None, says=None, behind=0, fill=0):
    """the words of a table block: header {3, 1, 0, R}, then records 0 .. R-1 (R defaults to all), `behind` further records' worth of
    words holding `fill`.  A record: mode 0 where lam == 1, 2 with the box where CutMix, else 1; one_minus_lam = 1.0f - lam in fp32.
    `says`: the R the header states when it is not the number of records present"""
    lam = np.asarray(lam, dtype=np.float32)
    R = len(lam) if R is None else R
    w = [record(3, 1., 0., (R if says is None else says, 0, 0, 0))]
    for i in range(R):
        if lam[i] == 1.:
            w.append(record(0, 1., 0.))
        elif cut[i]:
            w.append(record(2, lam[i], np.float32(1) - lam[i], [int(v) for v in boxes[i]]))
        else:
            w.append(record(1, lam[i], np.float32(1) - lam[i]))
    w.append(np.full(8 * behind, fill, dtype=np.int64).astype(np.int32))
    return torch.from_numpy(np.concatenate(w))


def table_of(name, dev="cpu", **kw):
    return table(GOLD[f"{name}__lam"], GOLD[f"{name}__use_cutmix"], GOLD[f"{name}__boxes"], **kw).to(dev)


def kinds(name):
    """the record modes a case's table holds"""
    return set(int(v) for v in table_of(name).view(-1, 8)[1:, 0])


def check_mix_case(L, dev, stream, name, sync=lambda: None):
    x, mixed = gold(name, "x"), gold(name, "mixed")
    assert not torch.equal(x, mixed)  # (the reference did mix this batch)
    blk = table_of(name, dev)
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        rc, y, intact = mix(L, dev, stream, x, blk, dtype, sync)
        assert rc == 0, L.cot_last_error()
        assert intact, f"{name} {dtype}: a NaN margin was written"
        assert torch.equal(y, normalized(mixed, dtype)), f"{name} {dtype}: differs from the reference's mixed batch, normalised"


def refs(name):
    f = lambda k: gold(name, f"soft_{k}")  # noqa: E731
    return (f("loss_f32"), f("rows_f32"), f("grad_f32")), (f("loss_f64"), f("rows_f64"), f("grad_f64"))


def smoothing(name):
    return META[name]["kwargs"]["label_smoothing"]


def check_loss_case(L, dev, stream, name, sync=lambda: None):
    r32, r64 = refs(name)
    run = lambda **kw: loss(L, dev, stream, gold(name, "logits"), gold(name, "labels"), table_of(name, dev), smoothing(name), sync=sync, **kw)  # noqa: E731
    got = run()
    compare(got, *r64, allowances(*r32, *r64), f"{name} soft target, table block")
    again = run()
    assert all(torch.equal(got[k], again[k]) for k in got), f"{name}: two runs differ"
    half = run(g=0.5)
    assert torch.equal(half["grad"], got["grad"] * 0.5)


def check_bf16_case(L, dev, stream, name, sync=lambda: None):
    got = loss(L, dev, stream, gold(name, "logits").bfloat16(), gold(name, "labels"), table_of(name, dev), smoothing(name), sync=sync)
    assert got["grad"].dtype == torch.bfloat16
    check_bf16_grad(got["grad"], gold(name, "soft_grad_bf16_f64"), f"{name}, table block")


def check_short_table(L, dev, stream, name, sync=lambda: None):
    """R = N/2: samples and rows >= R are not mixed and take the target (1, 0).  The words behind the R records are never read: sentinel
    garbage there, or nothing there at all, changes no bit.  An R larger than N counts as N."""
    N = META[name]["N"]
    R = N // 2
    x, mixed, logits, labels = gold(name, "x"), gold(name, "mixed"), gold(name, "logits"), gold(name, "labels")
    want = torch.cat([mixed[:R], x[R:]])
    blocks = dict(zeros=table_of(name, dev, R=R, behind=N - R), garbage=table_of(name, dev, R=R, behind=N - R, fill=SENTINEL),
                  nothing=table_of(name, dev, R=R))
    full = loss(L, dev, stream, logits, labels, table_of(name, dev), smoothing(name), sync=sync)
    hard = loss(L, dev, stream, logits, labels, torch.from_numpy(record(0, 1., 0.)), smoothing(name), sync=sync)  # header mode 0, lam 1
    for what, blk in blocks.items():
        for dtype in (torch.float32, torch.bfloat16):
            rc, y, intact = mix(L, dev, stream, x, blk, dtype, sync)
            assert rc == 0 and intact, (what, L.cot_last_error())
            assert torch.equal(y, normalized(want, dtype)), f"{name}, R = {R}, {what} behind the records"
        got = loss(L, dev, stream, logits, labels, blk, smoothing(name), sync=sync)
        for k in ("rows", "grad"):
            assert torch.equal(got[k][:R], full[k][:R]), f"{name} {k}: rows under the table, {what}"
            assert torch.equal(got[k][R:], hard[k][R:]), f"{name} {k}: rows past the table, {what}"
    # the header may state more records than samples: min(R, N) of them count
    over = table_of(name, dev, says=SENTINEL)
    rc, y, intact = mix(L, dev, stream, x, over, torch.float32, sync)
    assert rc == 0 and intact and torch.equal(y, normalized(mixed, torch.float32))
    got = loss(L, dev, stream, logits, labels, over, smoothing(name), sync=sync)
    assert all(torch.equal(got[k], full[k]) for k in got)
    # a negative R: no record counts
    none = table_of(name, dev, says=-1)
    rc, y, intact = mix(L, dev, stream, x, none, torch.float32, sync)
    assert rc == 0 and intact and torch.equal(y, normalized(x, torch.float32))
    got = loss(L, dev, stream, logits, labels, none, smoothing(name), sync=sync)
    assert all(torch.equal(got[k], hard[k]) for k in got)


def check_other_header_modes(L, dev, stream, name, sync=lambda: None):
    """a header mode outside 0-3 is still `as 0`: nothing is mixed, whatever follows it; the loss reads the header's lam as under mode 0"""
    x, logits, labels = gold(name, "x"), gold(name, "logits"), gold(name, "labels")
    for mode in (7, -3, 4):
        blk = table_of(name, dev)
        blk[0] = mode
        blk[1:3] = torch.from_numpy(np.array([0.3, 0.7], dtype=np.float32).view(np.int32)).to(dev)
        rc, y, intact = mix(L, dev, stream, x, blk, torch.float32, sync)
        assert rc == 0 and intact and torch.equal(y, normalized(x, torch.float32)), mode
        got = loss(L, dev, stream, logits, labels, blk, smoothing(name), sync=sync)
        as0 = loss(L, dev, stream, logits, labels, torch.from_numpy(record(0, 0.3, 0.7)), smoothing(name), sync=sync)
        assert all(torch.equal(got[k], as0[k]) for k in got), mode


def check_odd_batch_is_refused(L, dev):
    x = torch.zeros(3, 3, 16, 32, dtype=torch.uint8, device=dev)
    buf, y = margined((3, 3, 16, 32), torch.float32, dev)
    blk = table([0.5, 0.5, 0.5], [False] * 3, np.zeros((3, 4), dtype=np.int64)).to(dev)
    m, sd = MEAN.to(dev), STD.to(dev)
    rc = L.cot_mix_normalize(P(x), P(y), P(m), P(sd), P(blk), 3, 3, 16, 32, _lib.dtype_code(torch.float32), None)
    assert rc == -1 and b"odd" in L.cot_last_error()  # COT_ERR_INVALID_ARG
    assert bool(torch.isnan(buf).all())  # (refused before any launch)


def case_table(L, A, name, dtype, R):
    """footprint case: the table block as a 4-byte-aligned `in` operand inside filled margins, both kernels' families, every output"""
    x = A.i(gold(name, "x"))
    N, C, H, W = x.shape
    m, s = (MEAN.half().float(), STD.half().float()) if dtype == torch.float16 else (MEAN, STD)
    m, s = A.i(m.clone()), A.i(s.clone())
    params = A.i(table_of(name, R=R), align=4)
    y = A.o(x.shape, dtype)
    L.cot_mix_normalize(P(x), P(y), P(m), P(s), P(params), N, C, H, W, fp.dt(dtype), None)
    if dtype == torch.float16:
        return
    K = META[name]["K"]
    logits = A.i(gold(name, "logits").to(dtype), plane=K, row=K)
    labels = A.i(gold(name, "labels"))
    gout = A.i(torch.tensor([0.5]))
    rows, lse, mean = A.o(N, torch.float32), A.w(16 * N), A.o(1, torch.float32)
    L.cot_soft_target_ce_forward(P(logits), P(labels), P(params), 0.1, P(rows), P(lse), P(mean), N, K, fp.dt(dtype), None)
    dl = A.o((N, K), dtype, plane=K, row=K)
    L.cot_soft_target_ce_backward(P(logits), P(labels), P(params), 0.1, P(lse), P(gout), P(dl), N, K, fp.dt(dtype), None)


FOOTPRINT = [(name, dtype, R) for name in ("elem_vec", "elem_odd") for dtype in (torch.float32, torch.bfloat16, torch.float16)
             for R in (None, META[name]["N"] // 2)]


def check_footprint(L, name, dtype, R):
    for base in (0, 16):
        fp.run_case(L, case_table, (name, dtype, R), base=base)
