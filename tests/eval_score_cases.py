"""cot_eval_score through the C ABI against the reference's own results (tests/golden/eval_score.npz, written by
tests/golden/make_golden_eval.py): what tests/test_eval_score_emulated.py runs on the host emulator and tests/test_eval_score_gpu.py on the device.

Counts: samples, top1, top5 and row_rank equal the reference's `accuracy` counts and the rule below, exactly.  The fixture's seeded cases
hold no value equal to a target (in fp32 or rounded to bf16), so the reference's topk and the rule cannot differ on them.

The rule (`rule`, torch on the caller's device): with y the label and t = logit[n, y],
    rank = #{j : greater(logit_j, t)} + #{j < y : same(logit_j, t)}        the target's place in a stable descending sort
    greater(a, b) = a > b or (isnan(a) and not isnan(b));   same(a, b) = a == b or (isnan(a) and isnan(b))     NaN sorts first
    top1 = rank == 0, top5 = rank < 5;   a label outside [0, K) skips the row: nothing counted, row_rank -1, row_nll +0.0.

Loss: nll_sum and row_nll are compared with torch's fp64 cross entropy.  The allowance is MEASURED, not chosen: the error of torch's own fp32
evaluation against its fp64 one on the same inputs (both in the fixture), times 4 -- the margin for another summation order over K terms,
the reasoning and the factor of tests/mix_loss_cases.py -- per quantity: the sum against 4 x the error of the fp32 sum, the rows against
4 x the largest error of the fp32 rows.

Every output sits inside NaN margins that must stay NaN.
"""
import json

import torch

from cotnet_amd import _lib
from tests.conftest import load_golden
from tests.mix_loss_cases import FACTOR, P, margined, margins_intact

GOLD = load_golden("eval_score")
META = json.loads(str(GOLD["meta"]))
CASES = sorted(META)
TAGS = {"f32": torch.float32, "bf16": torch.bfloat16}
NAN = float("nan")


def gold(name, key):
    return torch.from_numpy(GOLD[f"{name}__{key}"])


def rule(logits, labels):
    """-> (rank int64 [N], -1 on skipped rows; nll fp64 [N], 0 on skipped rows), on the inputs' device (module docstring)"""
    x = logits.float()
    K = x.shape[1]
    valid = (labels >= 0) & (labels < K)
    y = labels.clamp(0, K - 1).view(-1, 1)
    t = x.gather(1, y)
    xn, tn = torch.isnan(x), torch.isnan(t)
    greater = (x > t) | (xn & ~tn)
    same = (x == t) | (xn & tn)
    cols = torch.arange(K, device=x.device).view(1, -1)
    rank = (greater | (same & (cols < y))).sum(1)
    nll = torch.logsumexp(x.double(), 1) - t.double()[:, 0]
    return torch.where(valid, rank, torch.full_like(rank, -1)), torch.where(valid, nll, torch.zeros_like(nll))


def new_block(dev):
    """-> (buffer with margins, the zeroed 32-byte block inside it as int64[4])"""
    buf, view = margined((4,), torch.float64, dev)
    acc = view.view(torch.int64)
    acc.zero_()
    assert acc.data_ptr() % 8 == 0
    return buf, acc


def read_block(acc):
    """-> (samples, top1, top5, nll_sum as a Python float): read back exactly"""
    host = acc.cpu()
    return int(host[0]), int(host[1]), int(host[2]), float(host[3:].view(torch.float64)[0])


def score(L, dev, stream, logits, labels, acc=None, rows=True, sync=lambda: None):
    """one cot_eval_score call on a fresh block (or adding to `acc`) -> dict(block=(samples, top1, top5, nll_sum), rank, nll);
    rows=False passes NULL for row_rank and row_nll"""
    N, K = logits.shape
    x, lab = logits.to(dev).contiguous(), labels.to(dev)
    abuf = None
    if acc is None:
        abuf, acc = new_block(dev)
    rbuf, rank = margined((N,), torch.float32, dev)  # (int32 results inside float NaN margins)
    nbuf, nll = margined((N,), torch.float32, dev)
    rc = L.cot_eval_score(P(x), P(lab), P(acc), P(rank) if rows else None, P(nll) if rows else None, N, K, _lib.dtype_code(logits.dtype), stream)
    assert rc == 0, L.cot_last_error()
    sync()
    assert all(margins_intact(b) for b in (abuf, rbuf, nbuf) if b is not None), "a NaN margin was written"
    assert torch.equal(x.cpu(), logits) or bool(torch.isnan(logits).any()), "the logits were written"
    assert torch.equal(lab.cpu(), labels), "the labels were written"
    if not rows:
        assert bool(torch.isnan(rank).all()) and bool(torch.isnan(nll).all()), "a row output was written through a NULL pointer's neighbour"
    return dict(block=read_block(acc), rank=rank.view(torch.int32).cpu().clone().long(), nll=nll.cpu().clone())


def check_counts(got, logits, labels, what):
    """the block and row_rank against the rule, exactly"""
    rank, _ = rule(logits, labels)
    assert torch.equal(got["rank"], rank), f"{what}: row_rank {got['rank'].tolist()} != the rule's {rank.tolist()}"
    want = (int((rank >= 0).sum()), int((rank == 0).sum()), int(((rank >= 0) & (rank < 5)).sum()))
    assert got["block"][:3] == want, f"{what}: (samples, top1, top5) {got['block'][:3]} != {want}"
    return rank


def check_case(L, dev, stream, name, tag, sync=lambda: None):
    """a fixture case in fp32 or bf16: counts against the reference and the rule, loss against the fp64 evaluation"""
    logits, labels = gold(name, "logits").to(TAGS[tag]), gold(name, "labels")
    got = score(L, dev, stream, logits, labels, sync=sync)
    check_counts(got, logits, labels, f"{name} {tag}")
    ref = (len(labels), int(gold(name, f"{tag}_top1")), int(gold(name, f"{tag}_top5")))
    assert got["block"][:3] == ref, f"{name} {tag}: (samples, top1, top5) {got['block'][:3]} != the reference's {ref}"
    sum64, rows64 = gold(name, f"{tag}_ce_sum_f64"), gold(name, f"{tag}_ce_rows_f64")
    a_sum = FACTOR * abs(float(gold(name, f"{tag}_ce_sum_f32")) - float(sum64))
    a_rows = FACTOR * float((gold(name, f"{tag}_ce_rows_f32").double() - rows64).abs().max())
    e_sum = abs(got["block"][3] - float(sum64))
    e_rows = float((got["nll"].double() - rows64).abs().max())
    print(f"{name} {tag}: nll_sum error {e_sum:.3e} (allowance {a_sum:.3e}); row_nll error {e_rows:.3e} (allowance {a_rows:.3e})")
    assert e_sum <= a_sum, f"{name} {tag}: nll_sum error {e_sum:.3e} over the allowance {a_sum:.3e}"
    assert e_rows <= a_rows, f"{name} {tag}: row_nll error {e_rows:.3e} over the allowance {a_rows:.3e}"
    # without the row outputs: the same block
    bare = score(L, dev, stream, logits, labels, rows=False, sync=sync)
    assert bare["block"] == got["block"]
    return got


def check_ties(L, dev, stream, dtype, sync=lambda: None):
    """the fixture's hand-made rows whose target is tied at, across and away from the fifth place: the rule exactly, and the reference's
    counts (topk places a tied target as it pleases) bracketed by strictly-greater hits below and greater-or-equal hits above"""
    logits, labels = gold("ties", "logits").to(dtype), gold("ties", "labels")
    got = score(L, dev, stream, logits, labels, sync=sync)
    rank = check_counts(got, logits, labels, f"ties {dtype}")
    assert rank.tolist() == [5, 4, 6, 3, 1, 0, 0, 2]  # (worked out by hand: the rows' comments in make_golden_eval.py)
    x, t = logits.float(), logits.float().gather(1, labels.view(-1, 1))
    ge, gt = (x >= t).sum(1) - 1, (x > t).sum(1)  # the target's worst and best place
    for k, key, mine in ((1, "top1", got["block"][1]), (5, "top5", got["block"][2])):
        lo, hi, ref = int((ge < k).sum()), int((gt < k).sum()), int(gold("ties", key))
        assert lo <= ref <= hi and lo <= mine <= hi, (key, lo, ref, mine, hi)
        assert lo < hi  # (the rows do leave topk a choice)


def check_nan(L, dev, stream, dtype, sync=lambda: None):
    """NaN sorts first, as in torch's descending sort: a NaN target, NaNs in front of and behind it, a NaN elsewhere"""
    rows = [(2, [1., 5., NAN, 3., 0., -1.], 0),    # the target is the only NaN: first
            (4, [1., NAN, 3., 0., NAN, NAN], 1),   # a NaN target behind another NaN, in front of a third
            (0, [2., NAN, 3., 0., 1., NAN], 3),    # NaNs elsewhere count as greater: 2 NaN + one larger value
            (3, [NAN, NAN, NAN, 7., NAN, NAN], 5),  # five NaNs above the target: a top-5 miss
            (1, [0., 7., NAN, 1., 2., 3.], 1)]
    logits = torch.tensor([r for _, r, _ in rows]).to(dtype)
    labels = torch.tensor([y for y, _, _ in rows])
    got = score(L, dev, stream, logits, labels, sync=sync)
    rank = check_counts(got, logits, labels, f"NaN rows {dtype}")
    assert rank.tolist() == [w for _, _, w in rows]
    place = [int((torch.sort(x, descending=True, stable=True).indices == y).nonzero()[0, 0]) for x, y in zip(logits.float(), labels)]
    assert rank.tolist() == place  # ... and torch's own stable descending sort puts the targets there
    assert bool(torch.isnan(got["nll"]).all()) and got["block"][3] != got["block"][3]  # (as torch's cross entropy of such rows)


def check_skipped(L, dev, stream, sync=lambda: None):
    """labels -1, K and far outside: nothing added, row_rank -1, row_nll +0.0; the rows between them are scored as if alone"""
    g = torch.Generator().manual_seed(7)
    logits = 3.0 * torch.randn(6, 37, generator=g)
    labels = torch.tensor([4, -1, 36, 37, 2 ** 40, 0])
    got = score(L, dev, stream, logits, labels, sync=sync)
    check_counts(got, logits, labels, "skipped rows")
    keep = torch.tensor([0, 2, 5])
    alone = score(L, dev, stream, logits[keep], labels[keep], sync=sync)
    assert got["block"] == alone["block"] and got["block"][0] == 3
    assert [got["rank"][i].item() for i in (1, 3, 4)] == [-1, -1, -1]
    skipped = got["nll"][[1, 3, 4]]
    assert torch.equal(skipped.view(torch.int32), torch.zeros(3, dtype=torch.int32)), "row_nll of a skipped row is +0.0"
    assert torch.equal(got["nll"][keep], alone["nll"])
    # a batch of skipped rows only
    none = score(L, dev, stream, logits, torch.full((6,), -1), sync=sync)
    assert none["block"] == (0, 0, 0, 0.0) and none["rank"].tolist() == [-1] * 6


def check_accumulation(L, dev, stream, sync=lambda: None):
    """three calls into one block = the three single-call blocks added, nll_sum in call order, bit for bit; two runs give equal bits"""
    batches = [(gold(n, "logits"), gold(n, "labels")) for n in ("n7_k37", "n3_k5", "n4_k1000")]

    def run():
        buf, acc = new_block(dev)
        for x, y in batches:
            score(L, dev, stream, x, y, acc=acc, sync=sync)
        assert margins_intact(buf)
        return read_block(acc)
    total, again = run(), run()
    singles = [score(L, dev, stream, x, y, sync=sync)["block"] for x, y in batches]
    assert total[:3] == tuple(sum(s[i] for s in singles) for i in range(3))
    want = 0.0
    for s in singles:
        want = want + s[3]  # fp64 additions in call order
    assert total[3] == want, (total[3], want)
    assert total == again, "two runs differ"


def check_refusals(L, dev):
    fake = 0x1000  # never dereferenced: validation fails first
    f32, bf16 = _lib.dtype_code(torch.float32), _lib.dtype_code(torch.bfloat16)
    call = lambda *a: L.cot_eval_score(*a)  # noqa: E731
    assert call(None, fake, fake, None, None, 2, 10, f32, None) == -1
    assert call(fake, None, fake, None, None, 2, 10, f32, None) == -1
    assert call(fake, fake, None, None, None, 2, 10, f32, None) == -1 and b"acc" in L.cot_last_error()
    assert call(fake, fake, fake, None, None, 0, 10, f32, None) == -1
    assert call(fake, fake, fake, None, None, 2, 0, bf16, None) == -1
    assert call(fake, fake, fake + 4, None, None, 2, 10, f32, None) == -1 and b"8-byte" in L.cot_last_error()
    for dt in (_lib.dtype_code(torch.float64), _lib.dtype_code(torch.float16), 99):
        assert call(fake, fake, fake, None, None, 2, 10, dt, None) == _lib.COT_ERR_UNSUPPORTED
    assert b"dtype" in L.cot_last_error()
    # ... and real buffers are left alone by a refused call
    buf, acc = new_block(dev)
    x, y = torch.zeros(2, 10, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
    assert call(P(x), P(y), P(acc), None, None, 2, 10, 99, None) == _lib.COT_ERR_UNSUPPORTED
    assert read_block(acc) == (0, 0, 0, 0.0) and margins_intact(buf)
