"""A training step with the recipe's mixup / CutMix and soft-target loss, captured ONCE into a HIP graph and replayed while labels, lambda,
the mode and the box change -- against the same steps issued eagerly, BIT FOR BIT (torch.equal, no tolerance: the loss kernels have no
atomics and add the rows in a fixed order).

The step: `cot_mix_normalize` of a static uint8 batch, the forward of a small mixed-precision model (one CoT bottleneck and global pooling,
the first 37 pooled channels as logits), `soft_target_cross_entropy` reading the DeviceMixup's block, backward, FlatSGD.  Between replays new labels are copied into the
static buffer and `draw()` writes the next batch's parameters; the np.random seed is found so that the three replayed draws are a mixup, a
CutMix and a `lam == 1` batch.  Built like tests/test_graph_replay_gpu.py (twins on static buffers, one non-default stream)."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

from cotnet_amd import DeviceMixup, _lib, cot_layer_fused as clf, soft_target_cross_entropy
from cotnet_amd.cotnet import Bottleneck
from cotnet_amd.flat_sgd import FlatSGD, to_mixed_bf16
from cotnet_amd.mixup import pack_params
from tests import mix_loss_cases as cases, truth
from tests.test_graph_replay_gpu import NCHW, _stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
WARM, K = 2, 3
CLASSES, N = 37, 4
MIX = dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.5, switch_prob=0.5, label_smoothing=0.1, num_classes=CLASSES)
IMG = (N, 3, 16, 32)


class Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.stage = nn.Sequential(Bottleneck(256, 64))

    def forward(self, x):  # the first CLASSES pooled channels are the logits: every kernel of the step is the library's
        return self.stage(x).mean((2, 3))[:, :CLASSES]


def _modes(seed, n):
    m = DeviceMixup(device="cpu", **MIX)
    np.random.seed(seed)
    out = []
    for _ in range(n):
        lam, cut, _ = m.sample(IMG)
        out.append(0 if lam == 1. else (2 if cut else 1))
    return out


def _seed():
    """the first seed whose draws WARM .. WARM + 2 are a mixup, a CutMix and a lam == 1 batch"""
    return next(s for s in range(100000) if _modes(s, WARM + K)[WARM:] == [1, 2, 0])


class _Twin:
    def __init__(self, model):
        self.m = copy.deepcopy(model)
        self.opt = FlatSGD(self.m, lr=0.05, momentum=0.9, weight_decay=4e-5, nesterov=True)
        self.mix = DeviceMixup(device=DEV, **MIX)
        self.x = torch.empty(N, 256, 14, 14, device=DEV, dtype=torch.bfloat16)
        self.img = torch.empty(IMG, device=DEV, dtype=torch.uint8)
        self.img_out = torch.empty(IMG, device=DEV, dtype=torch.bfloat16)
        self.t = torch.empty(N, device=DEV, dtype=torch.int64)
        self.mean, self.std = cases.MEAN.to(DEV), cases.STD.to(DEV)

    def load(self, batch):
        self.x.copy_(batch[0])
        self.img.copy_(batch[1])
        self.t.copy_(batch[2])
        self.mix.draw(IMG)

    def step(self):
        self.opt.zero_grad()
        self.mix.mix_normalize(self.img, self.mean, self.std, torch.bfloat16, out=self.img_out)
        loss = soft_target_cross_entropy(self.m(self.x), self.t, self.mix, 0.1)
        loss.backward()
        self.opt.step()
        return loss.detach()

    def state(self):
        d = {"param " + n: p.detach() for n, p in self.m.named_parameters()}
        d.update({"buffer " + n: b for n, b in self.m.named_buffers()})
        for i, st in enumerate(self.opt.state):
            d.update({f"opt.state[{i}][{k}]": v for k, v in st.items() if v is not None})
        d["img_out"] = self.img_out
        return {k: v.clone() for k, v in d.items()}


def _batches(n):
    g = torch.Generator(device=DEV).manual_seed(17)
    return [(torch.randn(N, 256, 14, 14, device=DEV, generator=g).bfloat16(),
             torch.randint(0, 256, IMG, device=DEV, generator=g, dtype=torch.uint8),
             torch.randint(0, CLASSES, (N,), device=DEV, generator=g)) for _ in range(n)]


def _same(a, b, what):
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert a.keys() == b.keys() and not bad, f"{what}: {len(bad)} of {len(a)} tensors differ, first {bad[:4]}"


def test_replayed_recipe_step_follows_labels_and_draws():
    seed = _seed()
    assert _modes(seed, WARM + K)[WARM:] == [1, 2, 0]
    s = _stream()
    batches = _batches(WARM + K)
    _lib.FALLBACKS.clear()
    with truth.switches(**NCHW), torch.cuda.stream(s):
        torch.manual_seed(2)
        model = Net().to(DEV).train()
        with torch.no_grad():
            model.stage[0].bn3.weight.fill_(0.8)  # (off the zero initialisation: the branch's gradients are not zeros)
        model = to_mixed_bf16(model)
        clf.plan_stage_layouts(model.stage)
        a, b = _Twin(model), _Twin(model)
        np.random.seed(seed)
        want, seen = [], []
        for bt in batches:
            a.load(bt)
            seen.append(int(a.mix.params[0]))
            want.append((a.step().clone(), a.state()))
        assert seen[WARM:] == [1, 2, 0], seen
        np.random.seed(seed)
        for bt in batches[:WARM]:
            b.load(bt)
            b.step()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out = b.step()
        for i, bt in enumerate(batches[WARM:], start=WARM):
            b.load(bt)  # new input, new labels, a new draw: all into the buffers the graph reads
            g.replay()
            clf.invalidate_packs()
            torch.cuda.synchronize()
            assert torch.equal(out, want[i][0]), f"step {i} (mode {seen[i]}): loss {float(out)!r} replayed, {float(want[i][0])!r} eager"
            _same(want[i][1], b.state(), f"after step {i} (mode {seen[i]})")
        assert len({float(w[0]) for w in want}) == len(want) and all(torch.isfinite(w[0]) for w in want)
        assert not _lib.FALLBACKS, dict(_lib.FALLBACKS)
        del g
    torch.cuda.current_stream().wait_stream(s)


def test_replayed_loss_changes_when_only_lambda_changes():
    """what fails if a capture baked lambda in: the same graph, the same logits and labels, another lambda in the block"""
    s = _stream()
    with torch.cuda.stream(s):
        gen = torch.Generator(device=DEV).manual_seed(5)
        logits = (3 * torch.randn(N, CLASSES, device=DEV, generator=gen)).bfloat16().requires_grad_(True)
        labels = torch.tensor([1, 5, 9, 30], device=DEV)
        mix = DeviceMixup(device=DEV, **MIX)
        mix.write(pack_params(1, 0.3))

        def run():
            logits.grad = None
            loss = soft_target_cross_entropy(logits, labels, mix, 0.1)
            loss.backward()
            return loss.detach(), logits.grad

        run()  # (warm-up outside the capture)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            out, grad = run()
        got = []
        for lam in (0.3, 0.7, 1.0):
            mix.write(pack_params(0 if lam == 1.0 else 1, lam))
            g.replay()
            replayed = (out.clone(), grad.clone())
            eager = run()
            torch.cuda.synchronize()
            assert torch.equal(replayed[0], eager[0]) and torch.equal(replayed[1], eager[1]), lam
            got.append(replayed)
        assert len({float(v[0]) for v in got}) == 3, [float(v[0]) for v in got]
        assert not torch.equal(got[0][1], got[1][1])
        del g
    torch.cuda.current_stream().wait_stream(s)
