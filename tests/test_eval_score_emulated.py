"""Validation scoring (csrc/eval_score.hip) on the host emulator, through the C ABI, against the reference's own counts and torch's fp64 cross
entropy -- the cases and criteria are in tests/eval_score_cases.py (tests/test_eval_score_gpu.py runs the same on the device) -- and the
Python surface (cotnet_amd.evaler, FlatSGD.ema_weights) on top of the emulated library."""
import ctypes

import pytest
import torch
from torch import nn

from cotnet_amd import _lib
from tests import eval_score_cases as cases
from tests.emul import build_emul

try:
    _EMUL = _lib.bind(ctypes.CDLL(build_emul.build()))
except FileNotFoundError:
    _EMUL = None

pytestmark = pytest.mark.skipif(_EMUL is None, reason="host emulation build unavailable")
CPU = torch.device("cpu")


def test_fixture_holds_the_cases_it_is_meant_to():
    assert {(v["N"], v["K"]) for v in cases.META.values()} == {(4, 1000), (7, 37), (3, 5), (2, 1001)}
    seen = set()
    for name, m in cases.META.items():
        labels = cases.gold(name, "labels")
        assert 0 in labels.tolist() and m["K"] - 1 in labels.tolist()
        for dtype in cases.TAGS.values():
            x = cases.gold(name, "logits").to(dtype).float()
            t = x.gather(1, labels.view(-1, 1))
            assert int((x == t).sum()) == m["N"], f"{name} {dtype}: a value equal to its row's target"  # (topk has no choice to make)
            rank, _ = cases.rule(x, labels)
            assert all(w is None or w == r for w, r in zip(m["want_ranks"], rank.tolist()))
            seen |= set(rank.tolist())
    assert seen >= {0, 1, 4, 5, 6}
    # bf16 rounding does produce duplicates in a row of 1000 (none of them the target's): the property had to be searched for
    x = cases.gold("n4_k1000", "logits").bfloat16().float()
    assert any(len(torch.unique(r)) < r.numel() for r in x)


@pytest.mark.parametrize("tag", sorted(cases.TAGS))
@pytest.mark.parametrize("name", cases.CASES)
def test_counts_and_loss_against_the_reference(name, tag):
    cases.check_case(_EMUL, CPU, None, name, tag)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ties_follow_the_stable_order_and_bracket_the_reference(dtype):
    cases.check_ties(_EMUL, CPU, None, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_nan_sorts_first(dtype):
    cases.check_nan(_EMUL, CPU, None, dtype)


def test_skipped_rows_add_nothing():
    cases.check_skipped(_EMUL, CPU, None)


def test_calls_accumulate_in_call_order():
    cases.check_accumulation(_EMUL, CPU, None)


def test_refusals_come_before_any_launch():
    cases.check_refusals(_EMUL, CPU)


def test_rows_longer_than_the_lanes_hold():
    """K = 1024 is the last row read once (16 columns per lane), K = 1025 the first walked twice: the rule on both sides"""
    g = torch.Generator().manual_seed(1024)
    for K in (1024, 1025):
        logits = 3.0 * torch.randn(3, K, generator=g)
        labels = torch.tensor([K - 1, 0, 640])
        got = cases.score(_EMUL, CPU, None, logits, labels)
        cases.check_counts(got, logits, labels, f"K = {K}")
        _, nll = cases.rule(logits, labels)
        # row_nll is the fp64 value rounded once: half an fp32 ulp, plus fp64 noise (1000 terms of 2^-53 each) far below it
        assert float(((got["nll"].double() - nll).abs() / nll.abs()).max()) <= 2.0 ** -24 * 1.001


# ---- the Python surface on the emulated library

def _emulated(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: _EMUL)
    monkeypatch.setattr(_lib, "DEVICE_ONLY", False)


def test_accuracy_has_the_reference_signature_and_counts(monkeypatch):
    from cotnet_amd import accuracy
    _emulated(monkeypatch)
    for name in cases.CASES:
        logits, labels = cases.gold(name, "logits"), cases.gold(name, "labels")
        got = accuracy(logits, labels, topk=(1, 5))
        assert [g.dtype for g in got] == [torch.float32] * 2 and all(g.dim() == 0 for g in got)
        assert [int(g) for g in got] == [int(cases.gold(name, "f32_top1")), int(cases.gold(name, "f32_top5"))]
        rank, _ = cases.rule(logits, labels)
        ks = (1, 2, 6, 7, 1000)  # any k
        assert [int(g) for g in accuracy(logits, labels, topk=ks)] == [int((rank < k).sum()) for k in ks]
    assert len(accuracy(logits, labels)) == 1
    assert int(accuracy(logits, torch.full_like(labels, -1), topk=(5,))[0]) == 0  # a skipped row is no hit
    with pytest.raises(TypeError):
        accuracy(logits, labels.int())
    with pytest.raises(TypeError):
        accuracy(logits.half(), labels)
    with pytest.raises(TypeError):
        accuracy(logits[0], labels)


def test_accuracy_refuses_cpu_tensors_on_the_product_path():
    from cotnet_amd import accuracy
    with pytest.raises(RuntimeError, match="no CPU path"):
        accuracy(torch.zeros(2, 5), torch.zeros(2, dtype=torch.int64))


def test_meter_reset_update_result(monkeypatch):
    from cotnet_amd import DeviceTestMeter
    with pytest.raises(RuntimeError, match="no CPU path"):
        DeviceTestMeter("cpu")
    _emulated(monkeypatch)
    m = DeviceTestMeter("cpu")
    assert m.result() == dict(samples=0, top1=pytest.approx(float("nan"), nan_ok=True), top5=pytest.approx(float("nan"), nan_ok=True),
                              loss=pytest.approx(float("nan"), nan_ok=True))
    total = [0, 0, 0, 0.0]
    for name in cases.CASES:
        logits, labels = cases.gold(name, "logits"), cases.gold(name, "labels")
        m.update(logits, labels)
        one = cases.score(_EMUL, CPU, None, logits, labels)["block"]
        total = [total[i] + one[i] for i in range(4)]
    r = m.result()
    assert r == dict(samples=total[0], top1=total[1] / total[0], top5=total[2] / total[0], loss=total[3] / total[0])
    assert r["samples"] == 16 and 0 < r["top1"] < r["top5"] < 1
    # the rows' outputs, on request
    rank, nll = torch.empty(4, dtype=torch.int32), torch.empty(4)
    logits, labels = cases.gold("n4_k1000", "logits"), cases.gold("n4_k1000", "labels")
    m.update(logits, labels, row_rank=rank, row_nll=nll)
    assert torch.equal(rank.long(), cases.rule(logits, labels)[0])
    with pytest.raises(ValueError, match="row_rank"):
        m.update(logits, labels, row_rank=torch.empty(4, dtype=torch.int64))
    m.reset()
    assert m.result()["samples"] == 0
    # reset inside a capture is refused and changes nothing
    m.update(logits, labels)
    monkeypatch.setattr(_lib, "capturing", lambda: True)
    with pytest.raises(RuntimeError, match="inside a HIP-graph capture"):
        m.reset()
    assert m.result()["samples"] == 4


def test_evaler_over_four_batches_the_last_one_short(monkeypatch):
    """a small Linear model over 3 batches of 4 and a last batch of 2, against counts worked out with torch by hand (the short batch at
    the full size, as Evaler scores it: its tail is zeros here, the latest full batch's rows there)"""
    from cotnet_amd import Evaler
    _emulated(monkeypatch)
    torch.manual_seed(3)
    model = nn.Sequential(nn.Linear(6, 9), nn.Dropout(0.5)).train()  # (dropout: eval mode must be on inside, and off again after)
    data = [(torch.randn(n, 6), torch.randint(0, 9, (n,))) for n in (4, 4, 4, 2)]
    ev = Evaler(data)
    top1, top5 = ev(0, model)
    assert model.training
    with torch.no_grad():
        model.eval()
        out = torch.cat([model(x) for x, _ in data[:3]] + [model(torch.cat([data[3][0], torch.zeros(2, 6)]))[:2]])
        model.train()
    y = torch.cat([t for _, t in data])
    order = torch.sort(out, dim=1, descending=True, stable=True).indices
    place = (order == y.view(-1, 1)).int().argmax(1)
    want = dict(samples=14, top1=int((place == 0).sum()) / 14, top5=int((place < 5).sum()) / 14)
    assert (top1, top5) == (want["top1"], want["top5"]) and ev.last["samples"] == 14
    ce = float(torch.nn.functional.cross_entropy(out.double(), y, reduction="sum")) / 14
    assert abs(ev.last["loss"] - ce) <= 1e-12 * ce  # fp64 on both sides, another order of 9 terms
    assert 0 < want["top1"] < want["top5"] < 1
    # eval-mode models stay in eval mode, amp_autocast is entered per batch, and a second pass starts from zero
    entered = []

    class Ctx:
        def __enter__(self):
            entered.append(1)

        def __exit__(self, *a):
            return False
    model.eval()
    assert ev(1, model, amp_autocast=Ctx) == (top1, top5) and not model.training and len(entered) == 4
    with pytest.raises(ValueError, match="no batch"):
        Evaler([])(0, model)


# ---- FlatSGD.ema_weights()

def _snapshot(model, opt):
    d = {"param " + n: p.detach().clone() for n, p in model.named_parameters()}
    d.update({"buffer " + n: b.clone() for n, b in model.named_buffers()})
    for i, st in enumerate(opt.state):
        d.update({f"state[{i}][{k}]": v.clone() for k, v in st.items() if v is not None})
    d.update({f"buf_ema[{i}]": b.clone() for i, b in enumerate(opt._buf_ema)})
    return d


def test_ema_weights_swaps_in_and_restores_bit_for_bit(monkeypatch):
    from cotnet_amd import cot_layer_fused, flat_sgd
    _emulated(monkeypatch)
    torch.manual_seed(5)
    model = flat_sgd.to_mixed_bf16(nn.Sequential(nn.Conv2d(4, 8, 3, padding=1), nn.BatchNorm2d(8), nn.ReLU(), nn.Conv2d(8, 6, 1))).train()
    opt = flat_sgd.FlatSGD(model, lr=0.05, momentum=0.9, weight_decay=1e-4, ema_decay=0.5, broadcast_params=False)
    x = torch.randn(5, 4, 6, 6).bfloat16()
    for _ in range(2):
        opt.zero_grad()
        model(x).float().square().mean().backward()
        opt.step()
    before, ema = _snapshot(model, opt), opt.ema_state_dict()
    assert {p.dtype for p in model.parameters()} == {torch.bfloat16, torch.float32}  # a bucket with a master and one without
    epoch = cot_layer_fused.PARAM_EPOCH[0]
    ptrs = [p.data_ptr() for p in model.parameters()]
    with opt.ema_weights() as o:
        assert o is opt and cot_layer_fused.PARAM_EPOCH[0] == epoch + 1
        assert [p.data_ptr() for p in model.parameters()] == ptrs  # in place: a captured forward follows
        changed = 0
        for k, v in model.state_dict().items():
            assert torch.equal(v, ema[k].to(v.dtype)), k  # (.to(bfloat16): round to nearest even)
            changed += int(not torch.equal(v, before[("param " if "param " + k in before else "buffer ") + k]))
        assert changed >= 6  # the average is not the model
        inside = _snapshot(model, opt)
        for k in inside:  # masters, momentum, the averages: not written
            if k.startswith(("state", "buf_ema")):
                assert torch.equal(inside[k], before[k]), k
        y_ema = model.eval()(x).float()
        model.train()
    assert cot_layer_fused.PARAM_EPOCH[0] == epoch + 2
    after = _snapshot(model, opt)
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)
    # ... the logits inside were those of a second model that loaded ema_state_dict(): what the context replaces
    twin = nn.Sequential(nn.Conv2d(4, 8, 3, padding=1), nn.BatchNorm2d(8), nn.ReLU(), nn.Conv2d(8, 6, 1))
    twin.load_state_dict(ema)
    assert torch.equal(flat_sgd.to_mixed_bf16(twin).eval()(x).float(), y_ema)
    # restored on an exception too; refused inside a capture and without ema_decay
    with pytest.raises(KeyError):
        with opt.ema_weights():
            raise KeyError("x")
    assert all(torch.equal(before[k], v) for k, v in _snapshot(model, opt).items())
    monkeypatch.setattr(_lib, "capturing", lambda: True)
    with pytest.raises(RuntimeError, match="inside a HIP-graph capture"):
        with opt.ema_weights():
            pass
    assert all(torch.equal(before[k], v) for k, v in _snapshot(model, opt).items())
    monkeypatch.setattr(_lib, "capturing", lambda: False)
    plain = flat_sgd.FlatSGD(flat_sgd.to_mixed_bf16(nn.Sequential(nn.Conv2d(4, 8, 1))), lr=0.1, broadcast_params=False)
    with pytest.raises(AssertionError, match="ema_decay"):
        with plain.ema_weights():
            pass
