"""cotnet_amd.mixup.DeviceMixup's host side: its draws against the reference's `FastCollateMixup(mode='batch')` under the same np.random
seed (tests/golden/recipe_draws.json, recorded by tests/golden/make_golden_recipe.py), and the words it writes into the parameter block."""
import json
import os

import numpy as np
import pytest
import torch

from cotnet_amd.mixup import DeviceMixup, pack_params
from tests.conftest import GOLDEN

DRAWS = json.load(open(os.path.join(GOLDEN, "recipe_draws.json")))


def _mixup(kwargs):
    return DeviceMixup(device="cpu", **kwargs)


def _block(m):
    w = m.params.numpy()
    return int(w[0]), float(w[1:3].view(np.float32)[0]), float(w[1:3].view(np.float32)[1]), tuple(int(v) for v in w[3:7]), int(w[7])


@pytest.mark.parametrize("setting", sorted(DRAWS["settings"]))
def test_draws_equal_the_reference_stream(setting):
    rec = DRAWS["settings"][setting]
    m = _mixup(rec["kwargs"])
    np.random.seed(DRAWS["seed"])
    kinds = set()
    for i, (lam, use_cutmix, box, _) in enumerate(rec["draws"]):
        got = m.draw(DRAWS["img_shape"])
        assert got == (lam, use_cutmix, tuple(box)), f"{setting}, batch {i}: {got} != {(lam, use_cutmix, box)}"
        mode = 0 if lam == 1.0 else (2 if use_cutmix else 1)
        kinds.add(mode)
        want = (mode, float(np.float32(lam)), float(np.float32(1.0 - lam)), tuple(box) if mode == 2 else (0, 0, 0, 0), 0)
        assert _block(m) == want, f"{setting}, batch {i}"
    assert kinds == ({0, 1, 2} if setting == "prob_half" else {1, 2})
    # the generator is where the reference left it: the next number is the same
    state = np.random.get_state()[1].copy()
    np.random.seed(DRAWS["seed"])
    ref = _mixup(rec["kwargs"])
    for _ in rec["draws"]:
        ref.sample(DRAWS["img_shape"])
    assert np.array_equal(state, np.random.get_state()[1])


def test_one_minus_lam_is_subtracted_in_double():
    lam = 0.5315061016529674
    w = pack_params(1, lam).numpy()[1:3].view(np.float32)
    assert w[0] == np.float32(lam) and w[1] == np.float32(1.0 - lam)
    lams = np.random.default_rng(0).random(10000)
    assert any(np.float32(1.0 - v) != np.float32(1.0) - np.float32(v) for v in lams)  # (fp32 subtraction is another number)


def test_disabled_draws_nothing():
    m = _mixup(dict(mixup_alpha=0.8, cutmix_alpha=1.0))
    assert m.mixup_enabled is True
    m.mixup_enabled = False
    np.random.seed(3)
    before = np.random.get_state()[1].copy()
    assert m.draw((2, 3, 8, 8)) == (1.0, False, (0, 0, 0, 0))
    assert np.array_equal(before, np.random.get_state()[1])
    assert _block(m) == (0, 1.0, 0.0, (0, 0, 0, 0), 0)


def test_fresh_block_is_no_mixing():
    m = _mixup({})
    assert m.params.dtype == torch.int32 and m.params.shape == (8,) and _block(m) == (0, 1.0, 0.0, (0, 0, 0, 0), 0)
    address = m.params.data_ptr()
    np.random.seed(0)
    m.draw((2, 3, 8, 8))
    assert m.params.data_ptr() == address and _block(m)[0] == 1  # (the defaults: mixup alone)


@pytest.mark.parametrize("mode", ["elem", "pair", "half"])
def test_other_modes_raise(mode):
    with pytest.raises(NotImplementedError, match="batch"):
        _mixup(dict(mode=mode))


def test_reference_constructor_and_defaults():
    import inspect
    names = list(inspect.signature(DeviceMixup.__init__).parameters)[1:]
    assert names[:9] == ["mixup_alpha", "cutmix_alpha", "cutmix_minmax", "prob", "switch_prob", "mode", "correct_lam", "label_smoothing",
                         "num_classes"]
    m = _mixup({})
    assert (m.mixup_alpha, m.cutmix_alpha, m.cutmix_minmax, m.mix_prob, m.switch_prob, m.mode, m.correct_lam, m.label_smoothing,
            m.num_classes) == (1., 0., None, 1.0, 0.5, "batch", True, 0.1, 1000)
    assert _mixup(dict(cutmix_minmax=[0.2, 0.8])).cutmix_alpha == 1.0
    with pytest.raises(ValueError):
        _mixup(dict(mixup_alpha=0., cutmix_alpha=0.)).sample((2, 3, 8, 8))


def test_exports():
    import cotnet_amd
    for n in ("DeviceMixup", "soft_target_cross_entropy", "MixedSoftTargetCrossEntropy", "LabelSmoothingCrossEntropy"):
        assert hasattr(cotnet_amd, n)


def test_loader_forwards_mixup_enabled():
    """the training loop's `loader.mixup_enabled = False` (reference train.py:243-245) reaches the DeviceMixup; a loader built without
    one accepts False and refuses True"""
    from cotnet_amd.input_pipeline import PrefetchLoader
    m = _mixup({})
    loader = PrefetchLoader([], device="cpu", mixup=m)
    assert loader.mixup_enabled is True
    loader.mixup_enabled = False
    assert m.mixup_enabled is False and loader.mixup_enabled is False
    loader.mixup_enabled = True
    assert m.mixup_enabled is True
    plain = PrefetchLoader([], device="cpu")
    assert plain.mixup is None and plain.mixup_enabled is False
    plain.mixup_enabled = False
    with pytest.raises(AssertionError, match="without a mixup"):
        plain.mixup_enabled = True
