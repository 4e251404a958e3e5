"""`PrefetchLoader(..., mixup=DeviceMixup(...))`: the host loader yields plain uint8 batches and integer labels, the side stream draws and
mixes one batch AHEAD, and the loss of the batch in hand must still find that batch's parameters in `mixup.params`.

Nothing in the loop below waits for the device: at every yield a copy of `mixup.params` and a loss that reads it are only enqueued on the
consumer's stream, so a block rewritten too early, or handed over too late, shows in what they return.  Everything is compared after the
loop: the k-th batch against the reference collate's arithmetic in numpy with the k-th draw, the k-th snapshot of the block against that draw,
the loss against the same loss on an explicit block.  The draws come from a host-only DeviceMixup under the same np.random seed."""
import numpy as np
import pytest
import torch

from cotnet_amd import DeviceMixup, soft_target_cross_entropy
from cotnet_amd.input_pipeline import PrefetchLoader
from cotnet_amd.mixup import pack_params
from tests import mix_loss_cases as cases
from tests.test_mix_loss_gpu import _mixed_numpy

pytestmark = pytest.mark.gpu
DEV = "cuda"
MIX = dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.5, switch_prob=0.5, label_smoothing=0.1, num_classes=37)
SHAPE = (4, 3, 16, 32)
BATCHES = 5


def _mode(lam, cut):
    return 0 if lam == 1. else (2 if cut else 1)


def _draws(seed):
    m = DeviceMixup(device="cpu", **MIX)
    np.random.seed(seed)
    return [m.sample(SHAPE) for _ in range(BATCHES)]


def _seed():
    """the first seed whose draws hold a mixup, a CutMix with a box and an unmixed batch, and no two neighbours alike"""
    for s in range(100000):
        d = _draws(s)
        modes = [_mode(lam, cut) for lam, cut, _ in d]
        if set(modes) == {0, 1, 2} and all(d[i] != d[i + 1] for i in range(BATCHES - 1)) and \
                all(b[1] > b[0] and b[3] > b[2] for lam, cut, b in d if _mode(lam, cut) == 2):
            return s


def test_loader_hands_each_batch_over_with_its_own_draw():
    seed = _seed()
    want = _draws(seed)
    g = torch.Generator().manual_seed(3)
    host = [(torch.randint(0, 256, SHAPE, dtype=torch.uint8, generator=g), torch.randint(0, 37, (SHAPE[0],), generator=g))
            for _ in range(BATCHES)]
    logits = (3 * torch.randn(BATCHES, SHAPE[0], 37, generator=g)).to(DEV)
    mix = DeviceMixup(device=DEV, **MIX)
    issued = []
    real_draw = mix.draw
    mix.draw = lambda *a, **k: issued.append(real_draw(*a, **k)) or issued[-1]
    loader = PrefetchLoader(host, mean=[v / 255 for v in cases.MEAN.tolist()], std=[v / 255 for v in cases.STD.tolist()],
                            dtype=torch.float32, mixup=mix)
    assert len(loader) == BATCHES and loader.mixup_enabled
    address = mix.params.data_ptr()
    got = []
    np.random.seed(seed)
    for k, (inp, tgt) in enumerate(loader):
        assert len(issued) == min(k + 2, BATCHES), f"batch {k}: {len(issued)} draws issued"  # one batch ahead, on the side stream
        assert issued[k] == want[k]
        assert tgt.dtype == torch.int64 and tgt.is_cuda and inp.is_cuda and inp.dtype == torch.float32
        got.append((inp, tgt, mix.params.clone(), soft_target_cross_entropy(logits[k], tgt, mix, 0.1)))  # enqueued, not waited for
    assert len(got) == BATCHES and issued == want and mix.params.data_ptr() == address
    torch.cuda.synchronize()
    mean, std = loader.mean.cpu(), loader.std.cpu()
    for k, (inp, tgt, block, loss) in enumerate(got):
        lam, cut, box = want[k]
        mode = _mode(lam, cut)
        words = pack_params(mode, lam, box if mode == 2 else (0, 0, 0, 0))
        assert torch.equal(block.cpu(), words), f"batch {k}: mixup.params held {block.tolist()}, the batch's draw is {words.tolist()}"
        mixed = _mixed_numpy(host[k][0], mode, lam, box) if mode else host[k][0]
        ref = mixed.float().sub_(mean.view(1, 3, 1, 1)).div_(std.view(1, 3, 1, 1))
        assert torch.equal(inp.cpu(), ref), f"batch {k} (mode {mode}) is not the collate's arithmetic with draw {k}"
        assert torch.equal(tgt.cpu(), host[k][1])
        assert torch.equal(loss, soft_target_cross_entropy(logits[k], tgt, words.to(DEV), 0.1)), f"batch {k}: the loss read another draw"
    assert {_mode(lam, cut) for lam, cut, _ in want} == {0, 1, 2}


def test_disabled_loader_passes_batches_unmixed():
    g = torch.Generator().manual_seed(4)
    host = [(torch.randint(0, 256, SHAPE, dtype=torch.uint8, generator=g), torch.randint(0, 37, (SHAPE[0],), generator=g)) for _ in range(3)]
    mix = DeviceMixup(device=DEV, **dict(MIX, prob=1.0))
    loader = PrefetchLoader(host, dtype=torch.bfloat16, mixup=mix)
    loader.mixup_enabled = False
    state = np.random.get_state()[1].copy()
    for (inp, tgt), (x, y) in zip(loader, host):
        assert torch.equal(mix.params.cpu(), pack_params(0, 1.))
        ref = x.float().sub_(loader.mean.cpu().view(1, 3, 1, 1)).div_(loader.std.cpu().view(1, 3, 1, 1)).bfloat16()
        assert torch.equal(inp.cpu(), ref) and torch.equal(tgt.cpu(), y)
    assert np.array_equal(state, np.random.get_state()[1])  # nothing was drawn
