"""Validation scoring (csrc/eval_score.hip) on the device: the cases and criteria of tests/test_eval_score_emulated.py
(tests/eval_score_cases.py) against the HIP library; the row lengths at which the kernels change path; the workload's rows (N = 128 and 80,
K = 1000, bf16); `update` recorded into a HIP graph and replayed; `Evaler` eager, replayed and by hand on cotnet50; `FlatSGD.ema_weights()`
against a second model that loaded `ema_state_dict()`, and the training step after it against a twin that never entered it."""
import pytest
import torch

import cotnet_amd
from cotnet_amd import DeviceTestMeter, Evaler, _lib
from cotnet_amd.flat_sgd import to_mixed_bf16
from tests import eval_score_cases as cases
from tests import truth
from tests.test_graph_replay_gpu import _Twin, _batches, _model, _stream, xent

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def run(check, *a):
    return check(_lib.lib(), DEV, _lib.stream(), *a, sync=torch.cuda.synchronize)


@pytest.mark.parametrize("tag", sorted(cases.TAGS))
@pytest.mark.parametrize("name", cases.CASES)
def test_counts_and_loss_against_the_reference(name, tag):
    run(cases.check_case, name, tag)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ties_follow_the_stable_order_and_bracket_the_reference(dtype):
    run(cases.check_ties, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_nan_sorts_first(dtype):
    run(cases.check_nan, dtype)


def test_skipped_rows_add_nothing():
    run(cases.check_skipped)


def test_calls_accumulate_in_call_order():
    run(cases.check_accumulation)


def test_refusals_come_before_any_launch():
    cases.check_refusals(_lib.lib(), DEV)


def _against_the_rule(logits, labels, what):
    """counts and row_rank exactly; row_nll = the fp64 value rounded once (half an fp32 ulp; the fp64 evaluations themselves differ by
    some 2^-53 per term, far below it); nll_sum against the fp64 sum of the rule's rows: N * K terms of 2^-53 relative each is below
    1e-12 at these sizes"""
    got = run(cases.score, logits, labels)
    rank = cases.check_counts(got, logits, labels, what)
    _, nll = cases.rule(logits.to(DEV), labels.to(DEV))
    nll = nll.cpu()
    valid = rank >= 0
    if bool(valid.any()):
        assert float(((got["nll"].double() - nll).abs()[valid] / nll[valid].abs()).max()) <= 2.0 ** -24 * 1.001, what
        want = float(nll.sum())
        assert abs(got["block"][3] - want) <= 1e-12 * abs(want), (what, got["block"][3], want)
    return got, rank


@pytest.mark.parametrize("K", [1, 4, 5, 63, 64, 65, 1000, 1001, 1024, 1025])
def test_row_length_edges(K):
    """K around the wave (63 / 64 / 65), the workload's and one more, K < 5 (every valid row is a top-5 hit), and 1024 / 1025: the last row
    length the lanes hold in registers and the first that is walked twice"""
    g = torch.Generator().manual_seed(K)
    for N in (1, 3):
        for dtype in (torch.float32, torch.bfloat16):
            logits = (3.0 * torch.randn(N, K, generator=g)).to(dtype)
            if K > 1:  # (K = 1: the only logit is the target, the loss exactly 0)
                logits[0, K - 1] = logits[0].float().max() + 1  # the last column wins row 0
            labels = torch.tensor([K - 1, 0, K // 2][:N])
            if K == 1:
                got = run(cases.score, logits, labels)
                assert got["block"] == (N, N, N, 0.0) and got["rank"].tolist() == [0] * N
                continue
            got, rank = _against_the_rule(logits, labels, f"N = {N}, K = {K}, {dtype}")
            assert rank[0] == 0
            if K < 5:
                assert got["block"][2] == N


def test_more_rows_than_one_launch_pair_holds():
    """4096 rows pass between the two launches at a time: 4096 + 3 rows are served in two slices, in row order"""
    N, K = 4096 + 3, 4
    g = torch.Generator().manual_seed(4099)
    logits = torch.randn(N, K, generator=g)
    labels = torch.randint(-1, K + 1, (N,), generator=g)  # skipped rows among them
    labels[-3:] = torch.tensor([0, K - 1, -1])
    _against_the_rule(logits, labels, "N = 4099")


@pytest.mark.parametrize("N", [128, 80])
def test_workload_rows_bf16(N):
    g = torch.Generator().manual_seed(N)
    K = 1000
    logits = (3.0 * torch.randn(N, K, generator=g)).bfloat16()
    labels = torch.randint(0, K, (N,), generator=g)
    hit = torch.arange(0, N, 3)  # as a trained model: a third of the targets raised into the first places
    logits[hit, labels[hit]] += 9.0
    got, rank = _against_the_rule(logits, labels, f"N = {N}, K = 1000 bf16")
    assert 0 < got["block"][1] < got["block"][2] < N
    again = run(cases.score, logits, labels)
    assert again["block"] == got["block"] and torch.equal(again["nll"], got["nll"])


def test_update_replays_on_new_batches():
    """`update` captured once over static logits and labels; three replays on different batches, the last with a padded tail of -1, leave
    the block bit-equal to the eager calls"""
    N, K = 6, 1000
    g = torch.Generator().manual_seed(66)
    batches = []
    for i in range(4):
        x = (3.0 * torch.randn(N, K, generator=g)).bfloat16()
        y = torch.randint(0, K, (N,), generator=g)
        x[0, y[0]] += 12.0
        batches.append((x.to(DEV), y.to(DEV)))
    batches[3][1][4:] = -1
    s = _stream()
    with torch.cuda.stream(s):
        eager, replayed = DeviceTestMeter(DEV), DeviceTestMeter(DEV)
        for x, y in batches[1:]:
            eager.update(x, y)
        sx, sy = batches[0][0].clone(), batches[0][1].clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            replayed.update(sx, sy)
            with pytest.raises(RuntimeError, match="inside a HIP-graph capture"):
                replayed.reset()
        assert cases.read_block(replayed.acc) == (0, 0, 0, 0.0)  # a capture records, it does not run
        for x, y in batches[1:]:
            sx.copy_(x)
            sy.copy_(y)
            graph.replay()
        a, b = cases.read_block(eager.acc), cases.read_block(replayed.acc)
        assert a == b and a[0] == 3 * N - 2 and a[1] >= 3, (a, b)
        assert eager.result() == replayed.result()
        del graph
    torch.cuda.current_stream().wait_stream(s)


def _sync_mode_is_honoured():
    """whether this torch build raises on a synchronising call under set_sync_debug_mode("error")"""
    t = torch.ones(1, device=DEV)
    torch.cuda.set_sync_debug_mode("error")
    try:
        t.item()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode("default")


def test_evaler_eager_replayed_and_by_hand():
    """cotnet50 in mixed precision, B = 2 at 224 x 224, three batches and a last one of a single sample: graph=True, graph=False and the
    eager logits scored by hand give the same block, bit for bit; the eager batch loop makes no synchronising call.

    The single sample is scored as row 0 of a batch of two in all three, each with ANOTHER tail -- the replay's stale buffer, the eager
    pass's copy of the latest full batch, zeros by hand: rows of one batch size do not depend on their neighbours.  They do depend on
    the batch size: alone (N = 1) the same sample takes other kernels, and on this untrained network their rounding grows to a largest
    logit difference of 14.0 at |logit| <= 96.5, nll 137.46 against 143.00 (measured on the MI355X; plain torch modules: 27.95 at 61.5)
    -- which is why Evaler scores a short batch at the full size with and without a graph."""
    s = _stream()
    data = [(x, t) for x, t in _batches((2, 3, 224, 224), (2,), 97, classes=1000, n=4)]
    data[3] = (data[3][0][:1].clone(), data[3][1][:1].clone())
    assert _sync_mode_is_honoured()

    def loop_without_syncs():
        torch.cuda.set_sync_debug_mode("error")
        try:
            yield from data
        finally:
            torch.cuda.set_sync_debug_mode("default")
    with truth.switches(**truth.SINGLE_NODE), torch.cuda.stream(s):
        model = _model("cotnet50")()
        with torch.no_grad():
            model.eval()
            padded = torch.zeros_like(data[0][0])
            padded[:1] = data[3][0]
            logits = [model(x).clone() for x in [d[0] for d in data[:3]] + [padded]]
            model.train()
        by_hand = DeviceTestMeter(DEV)
        for out, t in zip(logits, [d[1] for d in data[:3]] + [torch.cat([data[3][1], data[3][1].new_full((1,), -1)])]):
            by_hand.update(out, t)
        want = cases.read_block(by_hand.acc)
        assert want[0] == 7 and want[3] > 0
        eager = Evaler(loop_without_syncs(), graph=False)
        top1, top5 = eager(0, model)
        assert model.training and cases.read_block(eager.meter.acc) == want
        assert (top1, top5) == (want[1] / 7, want[2] / 7) and eager.last == by_hand.result()
        replayed = Evaler(data, graph=True)
        for epoch in range(2):  # the second pass replays the first one's capture
            assert replayed(epoch, model) == (top1, top5)
            assert replayed.graph_note is None and len(replayed._graphs) == 1
            assert cases.read_block(replayed.meter.acc) == want
        del replayed
    torch.cuda.current_stream().wait_stream(s)


def test_ema_weights_against_a_second_model_and_a_twin_that_never_entered():
    """two training steps of cotnet50 at B = 2 with ema_decay = 0.5; inside the context the logits equal, bit for bit, those of a fresh
    model that loaded ema_state_dict() and went through to_mixed_bf16; after it a third step equals the twin's (loss, every parameter)"""
    s = _stream()
    batches = _batches((2, 3, 224, 224), (2,), 131, classes=1000, n=3)
    with truth.switches(**truth.SINGLE_NODE), torch.cuda.stream(s):
        model = _model("cotnet50")()
        a, b = (_Twin(model, xent, batches[0], 0.05, ema_decay=0.5) for _ in range(2))
        for tw in (a, b):
            for bt in batches[:2]:
                tw.load(bt)
                tw.step()
        with a.opt.ema_weights(), torch.no_grad():
            a.m.eval()
            inside = a.m(batches[2][0]).clone()
            a.m.train()
        fresh = cotnet_amd.create_model("cotnet50", num_classes=1000).to(DEV)
        fresh.load_state_dict(a.opt.ema_state_dict())
        fresh = to_mixed_bf16(fresh).eval()
        with torch.no_grad():
            want = fresh(batches[2][0])
            a.m.eval()
            own = a.m(batches[2][0]).clone()
            a.m.train()
        assert torch.equal(inside, want)
        assert not torch.equal(inside, own)  # (the average is not the model)
        for tw in (a, b):
            tw.load(batches[2])
        la, lb = a.step(), b.step()
        assert torch.equal(la, lb) and bool(torch.isfinite(la))
        sa, sb = a.state(), b.state()
        bad = [k for k in sa if not torch.equal(sa[k], sb[k])]
        assert sa.keys() == sb.keys() and not bad, bad[:4]
    torch.cuda.current_stream().wait_stream(s)
