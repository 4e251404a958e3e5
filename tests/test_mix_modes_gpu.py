"""Per-sample mixup / CutMix (a table block: the reference's mode='elem' / 'pair') on the device: the cases and criteria of
tests/test_mix_modes_emulated.py (tests/mix_modes_cases.py) against the HIP library, and what only the device can show -- one capture
replayed under table blocks and a batch-mode block, `PrefetchLoader` handing every batch over with its own table, and `Trainer` replaying
its step under `PerSampleMixup`."""
import numpy as np
import pytest
import torch

from cotnet_amd import MixedSoftTargetCrossEntropy, PerSampleMixup, _lib, soft_target_cross_entropy
from cotnet_amd.input_pipeline import PrefetchLoader
from cotnet_amd.mixup import pack_params
from tests import mix_loss_cases as base
from tests import mix_modes_cases as cases
from tests import trainer_cases as tc
from tests.test_graph_replay_gpu import _stream

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
MIX = dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.6, switch_prob=0.5, label_smoothing=0.1, num_classes=37)
SHAPE = (4, 3, 16, 32)


class _DeviceLib:
    _test_device = "cuda"

    def __getattr__(self, name):
        return getattr(_lib.lib(), name)


def run(check, *a):
    return check(_lib.lib(), DEV, _lib.stream(), *a, sync=torch.cuda.synchronize)


@pytest.mark.parametrize("name", cases.CASES)
def test_mix_equals_the_reference_collate_then_normalize(name):
    run(cases.check_mix_case, name)


@pytest.mark.parametrize("name", cases.CASES)
def test_soft_target_loss_and_gradient(name):
    run(cases.check_loss_case, name)


@pytest.mark.parametrize("name", cases.CASES)
def test_bf16_gradient_within_one_ulp(name):
    run(cases.check_bf16_case, name)


@pytest.mark.parametrize("name", ["elem_vec", "elem_rows", "elem_odd", "pair_vec"])
def test_rows_past_the_table_are_unmixed_and_nothing_behind_it_is_read(name):
    run(cases.check_short_table, name)


@pytest.mark.parametrize("name", ["elem_vec", "elem_odd"])
def test_other_header_modes_are_still_mode_0(name):
    run(cases.check_other_header_modes, name)


def test_odd_batch_is_refused():
    cases.check_odd_batch_is_refused(_lib.lib(), DEV)


@pytest.mark.parametrize("name,dtype,R", cases.FOOTPRINT, ids=[f"{n}-{str(d)[6:]}-R{r}" for n, d, r in cases.FOOTPRINT])
def test_footprint_and_placement_of_the_table_block(name, dtype, R):
    cases.check_footprint(_DeviceLib(), name, dtype, R)
    torch.cuda.synchronize()


# ---- one capture, every kind of block

def _kinds(words, N):
    return set(int(v) for v in words.view(-1, 8)[1:1 + N, 0])


def _seed(mode, n, shape=SHAPE):
    """the first seed whose n draws hold between them a mixup record, a CutMix record with a box, and an unmixed one, no two draws alike"""
    m = PerSampleMixup(device="cpu", mode=mode, capacity=shape[0], **MIX)
    for s in range(10000):
        np.random.seed(s)
        packs = [m.pack(*m.sample(shape, shape[0])) for _ in range(n)]
        boxes_ok = all((r[4] > r[3] and r[6] > r[5]) for p in packs for r in p.view(-1, 8)[1:].tolist() if r[0] == 2)
        if set().union(*(_kinds(p, shape[0]) for p in packs)) == {0, 1, 2} and boxes_ok and \
                all(not torch.equal(packs[i], packs[i + 1]) for i in range(n - 1)):
            return s
    raise RuntimeError("no seed found")


def test_one_capture_follows_tables_and_a_batch_mode_header():
    N, C, H, W = SHAPE
    K = 37
    seed = _seed("elem", 4)
    s = _stream()
    with torch.cuda.stream(s):
        gen = torch.Generator().manual_seed(11)
        x = torch.randint(0, 256, SHAPE, dtype=torch.uint8, generator=gen).to(DEV)
        logits = (3 * torch.randn(N, K, generator=gen)).to(DEV).requires_grad_(True)
        labels = torch.tensor([1, 5, 9, 5], device=DEV)
        mean, std = base.MEAN.to(DEV), base.STD.to(DEV)
        mix = PerSampleMixup(device=DEV, capacity=N, **MIX)
        out = torch.empty(SHAPE, dtype=torch.bfloat16, device=DEV)

        def step(y):
            logits.grad = None
            mix.mix_normalize(x, mean, std, torch.bfloat16, out=y)
            loss = soft_target_cross_entropy(logits, labels, mix, 0.1)
            loss.backward()
            return loss.detach(), logits.grad

        step(out)  # (warm-up outside the capture, under the fresh block: mode 0)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            loss, grad = step(out)
        address = mix.params.data_ptr()
        np.random.seed(seed)
        seen, losses = set(), []

        def replay_and_compare(what):
            g.replay()
            got = (out.clone(), loss.clone(), grad.clone())
            eager = torch.empty_like(out)
            want_loss, want_grad = step(eager)
            torch.cuda.synchronize()
            assert torch.equal(got[0], eager), f"{what}: the replayed batch differs from the eager one"
            assert torch.equal(got[1], want_loss) and torch.equal(got[2], want_grad), f"{what}: the replayed loss differs from the eager one"
            losses.append(float(got[1]))
            return got

        for i in range(4):
            lam, cut, boxes = mix.draw(SHAPE)
            words = mix.params.cpu()
            assert torch.equal(words[:8 * (1 + N)], cases.table(lam, cut, boxes))
            seen |= _kinds(words, N)
            got = replay_and_compare(f"draw {i}")
            # and it IS this draw's batch: the collate's arithmetic, sample by sample
            want = x.cpu().clone()
            for n in range(N):
                a, b = x[n].cpu().numpy(), x[N - 1 - n].cpu().numpy()
                if lam[n] != 1. and cut[n]:
                    yl, yh, xl, xh = boxes[n]
                    want[n, :, yl:yh, xl:xh] = torch.from_numpy(b[:, yl:yh, xl:xh])
                elif lam[n] != 1.:
                    m = a.astype(np.float32) * lam[n] + b.astype(np.float32) * (1 - lam[n])
                    want[n] = torch.from_numpy(np.rint(m).astype(np.uint8))
            assert torch.equal(got[0].cpu(), base.normalized(want, torch.bfloat16)), f"draw {i}"
        assert seen == {0, 1, 2}
        # a batch-mode header in the same block: the records behind it are not looked at
        for mode, lam, box in ((1, 0.3, (0, 0, 0, 0)), (2, 0.75, (2, 10, 5, 21)), (0, 1.0, (0, 0, 0, 0))):
            mix.write(pack_params(mode, lam, box))
            assert int(mix.params[0]) == mode and int(mix.params[8]) in (0, 1, 2)  # (the last table's records are still there)
            got = replay_and_compare(f"header mode {mode}")
            ref = base.mix(_lib.lib(), DEV, _lib.stream(), x.cpu(), pack_params(mode, lam, box).to(DEV), torch.bfloat16, torch.cuda.synchronize)
            assert torch.equal(got[0].cpu(), ref[1])
        assert mix.params.data_ptr() == address and len(set(losses)) == len(losses), losses
        del g
    torch.cuda.current_stream().wait_stream(s)


# ---- the loader (the pattern of tests/test_prefetch_mixup_gpu.py)

@pytest.mark.parametrize("mode", ["elem", "pair"])
def test_loader_hands_each_batch_over_with_its_own_table(mode):
    batches, N = 4, SHAPE[0]
    seed = _seed(mode, batches)
    host_mix = PerSampleMixup(device="cpu", mode=mode, capacity=6, **MIX)
    np.random.seed(seed)
    want = [host_mix.sample(SHAPE, N) for _ in range(batches)]
    g = torch.Generator().manual_seed(3)
    host = [(torch.randint(0, 256, SHAPE, dtype=torch.uint8, generator=g), torch.randint(0, 37, (N,), generator=g)) for _ in range(batches)]
    logits = (3 * torch.randn(batches, N, 37, generator=g)).to(DEV)
    mix = PerSampleMixup(device=DEV, mode=mode, capacity=6, **MIX)
    loader = PrefetchLoader(host, mean=[v / 255 for v in base.MEAN.tolist()], std=[v / 255 for v in base.STD.tolist()],
                            dtype=torch.float32, mixup=mix)
    address = mix.params.data_ptr()
    got = []
    np.random.seed(seed)
    for k, (inp, tgt) in enumerate(loader):
        got.append((inp, tgt, mix.params.clone(), soft_target_cross_entropy(logits[k], tgt, mix, 0.1)))  # enqueued, not waited for
    assert len(got) == batches and mix.params.data_ptr() == address
    torch.cuda.synchronize()
    for k, (inp, tgt, block, loss) in enumerate(got):
        words = cases.table(*want[k])
        assert torch.equal(block.cpu()[:8 * (1 + N)], words), f"batch {k}: mixup.params did not hold the batch's own table"
        rc, ref, _ = base.mix(_lib.lib(), DEV, _lib.stream(), host[k][0], words.to(DEV), torch.float32, torch.cuda.synchronize)
        assert rc == 0 and torch.equal(inp.cpu(), ref), f"batch {k} is not the eager mix under table {k}"
        assert torch.equal(tgt.cpu(), host[k][1])
        assert torch.equal(loss, soft_target_cross_entropy(logits[k], tgt, words.to(DEV), 0.1)), f"batch {k}: the loss read another table"
    assert set().union(*(_kinds(cases.table(*w), N) for w in want)) == {0, 1, 2}


# ---- the trainer: tests/trainer_cases.py's rig with the per-sample mixup in the DeviceMixup's place

class _Rig(tc.Rig):
    def __init__(self, dev, kind, epochs):
        super().__init__(dev, kind, epochs)  # (seeds np.random; nothing has been drawn yet)
        self.mix = PerSampleMixup(device=dev, mode="elem", capacity=tc.N, **tc.MIX)
        sample = self.mix.sample

        def logged(shape, n):
            out = sample(shape, n)
            self.draws.append(self.mix.pack(*out))
            return out
        self.mix.sample = logged
        self.loss_fn = MixedSoftTargetCrossEntropy(self.mix)
        self.loader = tc.train_loader(dev, self.mix)


def test_trainer_replays_its_step_under_per_sample_mixup():
    epochs = 2
    hand = _Rig("cuda", "sgd", epochs)
    history, losses = tc.hand_loop(hand)
    out = {}
    for name, graph in (("eager", False), ("replayed", True)):
        rig = _Rig("cuda", "sgd", epochs)
        t = rig.trainer(graph)
        out[name] = dict(rig=rig, trainer=t, history=t.fit(), state=rig.state())
    tc.same(hand.state(), out["eager"]["state"], "the hand-written loop vs Trainer(graph=False)")
    tc.same(out["eager"]["state"], out["replayed"]["state"], "Trainer(graph=False) vs Trainer(graph=True)")
    assert out["eager"]["history"] == out["replayed"]["history"]
    for h, t in zip(history, out["replayed"]["history"]):
        assert all(t[k] == v for k, v in h.items()), (h, t)
    flat = [v for e in losses for v in e]
    assert len(flat) == epochs * tc.BATCHES and len(set(flat)) == len(flat) and all(np.isfinite(flat)), flat
    step = out["replayed"]["trainer"].step
    assert step.graph and step.graph_note is None, step.graph_note
    assert step.replays == epochs * (tc.BATCHES - 1) - tc.WARMUP and out["eager"]["trainer"].step.replays == 0
    draws = out["replayed"]["rig"].draws
    assert len(draws) == epochs * tc.BATCHES and all(torch.equal(a, b) for a, b in zip(draws, hand.draws))
    assert [len(d) // 8 - 1 for d in draws] == tc.SIZES * epochs  # the short last batch wrote a shorter table
    assert set().union(*(_kinds(d, len(d) // 8 - 1) for d in draws)) >= {1, 2}
    assert int(hand.mix.params[0]) == 3 and int(hand.mix.params[3]) == tc.SHORT
