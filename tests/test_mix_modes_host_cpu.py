"""cotnet_amd.mixup.PerSampleMixup's host side: its draws against the reference's `FastCollateMixup(mode='elem' | 'pair')` under the same
np.random seed (tests/golden/mix_modes_draws.json, recorded by tests/golden/make_golden_mix_modes.py), the words it writes into the table
block against the header's rule and the reference's dense target, and `create_mixup`'s routing."""
import json
import os

import numpy as np
import pytest
import torch

from cotnet_amd import _lib
from cotnet_amd.mixup import DeviceMixup, PerSampleMixup, create_mixup
from tests import mix_modes_cases as cases
from tests.conftest import GOLDEN

DRAWS = json.load(open(os.path.join(GOLDEN, "mix_modes_draws.json")))


def _mixup(kwargs, **kw):
    return PerSampleMixup(device="cpu", **dict(kwargs, **kw))


@pytest.mark.parametrize("setting", sorted(DRAWS["settings"]))
def test_draws_equal_the_reference_stream(setting):
    rec = DRAWS["settings"][setting]
    m = _mixup(rec["kwargs"])
    N = DRAWS["img_shape"][0]
    np.random.seed(DRAWS["seed"])
    for i, want in enumerate(rec["draws"]):
        lam, use_cutmix, boxes = m.sample(DRAWS["img_shape"], N)
        assert lam.dtype == np.float32 and len(lam) == N
        got = dict(lam_bits=[int(v) for v in lam.view(np.int32)], use_cutmix=[bool(v) for v in use_cutmix],
                   boxes=[[int(v) for v in b] for b in boxes])
        assert got == want, f"{setting}, batch {i}: {got} != {want}"
    # the generator is where the reference left it: the next number is the same as after the same draws written into a block
    state = np.random.get_state()[1].copy()
    np.random.seed(DRAWS["seed"])
    again = _mixup(rec["kwargs"])
    for want in rec["draws"]:
        lam, use_cutmix, boxes = again.draw(DRAWS["img_shape"])
        assert torch.equal(again.params[:8 * (1 + N)], cases.table(lam, use_cutmix, boxes))
        assert [int(v) for v in lam.view(np.int32)] == want["lam_bits"]
    assert np.array_equal(state, np.random.get_state()[1])


def test_the_recorded_draws_hold_every_kind():
    s = DRAWS["settings"]
    one = 0x3f800000
    assert sorted(s) == sorted(f"{m}_{k}" for m in ("elem", "pair") for k in ("recipe", "prob_half", "minmax", "mixup_only", "cutmix_only"))
    assert all(len(v["draws"]) == 32 and all(len(b["lam_bits"]) == 6 for b in v["draws"]) for v in s.values())
    for mode in ("elem", "pair"):
        assert any(one in b["lam_bits"] for b in s[f"{mode}_prob_half"]["draws"])
        assert not any(any(b["use_cutmix"]) for b in s[f"{mode}_mixup_only"]["draws"])
        assert all(all(b["use_cutmix"]) for b in s[f"{mode}_cutmix_only"]["draws"])
        assert any(len(set(b["use_cutmix"])) == 2 for b in s[f"{mode}_recipe"]["draws"])  # mixup and CutMix within one batch
    for v in (s[k] for k in s if k.startswith("pair")):  # the mirrored half
        assert all(b["lam_bits"] == b["lam_bits"][::-1] and b["boxes"] == b["boxes"][::-1] for b in v["draws"])


def _decode_target(words, labels, K, smoothing):
    """the target the loss kernels form from a table block (include/cotnet_amd.h): (on|off)*lam + (on|off)*one_minus_lam in fp32, the two
    products rounded separately, with on / off formed in double and rounded once"""
    w = words.numpy().reshape(-1, 8)
    assert w[0, 0] == 3
    R, N = int(w[0, 3]), len(labels)
    off = np.float32(smoothing / K)
    on = np.float32(1. - smoothing + smoothing / K)
    lam, oml = np.ones(N, dtype=np.float32), np.zeros(N, dtype=np.float32)
    n = min(R, N)
    lam[:n], oml[:n] = w[1:1 + n, 1].view(np.float32), w[1:1 + n, 2].view(np.float32)
    y1 = np.full((N, K), off, dtype=np.float32)
    y2 = y1.copy()
    y1[np.arange(N), labels] = on
    y2[np.arange(N), labels[::-1]] = on
    return y1 * lam[:, None] + y2 * oml[:, None]


@pytest.mark.parametrize("name", cases.CASES)
def test_the_words_draw_writes_give_the_reference_target(name):
    meta = cases.META[name]
    m = _mixup(meta["kwargs"], capacity=6)
    assert m.params.shape == (8 * 7,) and m.params.dtype == torch.int32
    assert [int(v) for v in m.params[:8]] == [0, 0x3f800000, 0, 0, 0, 0, 0, 0] and not m.params[8:].any()  # fresh: no mixing
    address = m.params.data_ptr()
    np.random.seed(meta["seed"])
    N = meta["N"]
    lam, use_cutmix, boxes = m.draw((N, 3, meta["H"], meta["W"]))
    assert m.params.data_ptr() == address
    G = cases.GOLD
    assert np.array_equal(lam.view(np.int32), G[f"{name}__lam"].view(np.int32))
    assert np.array_equal(use_cutmix, G[f"{name}__use_cutmix"]) and np.array_equal(boxes, G[f"{name}__boxes"])
    words = m.params[:8 * (1 + N)]
    assert torch.equal(words, cases.table_of(name))  # the header's rule, record by record
    assert not m.params[8 * (1 + N):].any()  # nothing written behind the N records
    target = _decode_target(words, G[f"{name}__labels"], meta["K"], meta["kwargs"]["label_smoothing"])
    assert np.array_equal(target.view(np.int32), G[f"{name}__target"].view(np.int32)), f"{name}: the target differs from the reference's in some bit"


def test_one_minus_lam_is_subtracted_in_fp32():
    lams = np.random.default_rng(0).random(10000).astype(np.float32)
    m = _mixup({}, capacity=len(lams))
    w = m.pack(lams, np.zeros(len(lams), dtype=bool), np.zeros((len(lams), 4), dtype=np.int64)).numpy().reshape(-1, 8)
    assert np.array_equal(w[1:, 1].view(np.float32), lams) and np.array_equal(w[1:, 2].view(np.float32), np.float32(1) - lams)
    assert (w[1:, 0] == 1).all() and w[0].tolist() == [3, 0x3f800000, 0, len(lams), 0, 0, 0, 0]


def test_create_mixup_routes_the_recipe_switch():
    kw = dict(mixup_alpha=0.8, cutmix_alpha=1.0, device="cpu")
    b = create_mixup(**kw)
    assert type(b) is DeviceMixup and b.mode == "batch" and type(create_mixup("batch", **kw)) is DeviceMixup
    for mode in ("elem", "pair"):
        m = create_mixup(mode, **kw)
        assert type(m) is PerSampleMixup and isinstance(m, DeviceMixup) and m.mode == mode and m.capacity == 1024
        assert m.params.shape == (8 * 1025,) and m.new_block().shape == (8 * 1025,)
        assert (m.mixup_alpha, m.cutmix_alpha, m.mix_prob, m.switch_prob, m.label_smoothing, m.num_classes) == (0.8, 1.0, 1.0, 0.5, 0.1, 1000)
    with pytest.raises(ValueError):
        create_mixup("rows", **kw)


def test_half_stays_on_the_host():
    with pytest.raises(NotImplementedError, match="half"):
        create_mixup("half", device="cpu")
    for mode in ("half", "batch"):
        with pytest.raises(NotImplementedError):
            PerSampleMixup(mode=mode, device="cpu")


def test_draw_inside_a_capture_raises(monkeypatch):
    m = _mixup({})
    monkeypatch.setattr(_lib, "capturing", lambda: True)
    before = m.params.clone()
    np.random.seed(1)
    state = np.random.get_state()[1].copy()
    with pytest.raises(RuntimeError, match="between replays"):
        m.draw((2, 3, 8, 8))
    assert torch.equal(m.params, before) and np.array_equal(state, np.random.get_state()[1])


def test_a_batch_over_the_capacity_or_odd_raises():
    m = _mixup({}, capacity=4)
    before = m.params.clone()
    with pytest.raises(ValueError, match="capacity"):
        m.draw((6, 3, 8, 8))
    with pytest.raises(ValueError, match="odd"):
        m.draw((3, 3, 8, 8))
    assert torch.equal(m.params, before)
    m.draw((4, 3, 8, 8))
    assert int(m.params[0]) == 3 and int(m.params[3]) == 4


def test_disabled_writes_a_mode_0_header_and_draws_nothing():
    m = _mixup(dict(mixup_alpha=0.8, cutmix_alpha=1.0), capacity=4)
    np.random.seed(3)
    m.draw((4, 3, 8, 8))
    assert int(m.params[0]) == 3
    m.mixup_enabled = False
    before = np.random.get_state()[1].copy()
    lam, use_cutmix, boxes = m.draw((4, 3, 8, 8))
    assert np.array_equal(before, np.random.get_state()[1])
    assert (lam == 1).all() and not use_cutmix.any() and not boxes.any()
    assert [int(v) for v in m.params[:8]] == [0, 0x3f800000, 0, 0, 0, 0, 0, 0]


def test_exports():
    import cotnet_amd
    assert cotnet_amd.PerSampleMixup is PerSampleMixup and cotnet_amd.create_mixup is create_mixup
