"""Per-sample mixup / CutMix (a table block: the reference's mode='elem' / 'pair') on the host emulator, through the C ABI, against the
reference's own collate and loss -- the cases and criteria are in tests/mix_modes_cases.py (tests/test_mix_modes_gpu.py runs the same on the
device) -- and `PerSampleMixup` with the loss modules on top of the emulated library."""
import ctypes

import numpy as np
import pytest
import torch

from cotnet_amd import _lib
from tests import mix_modes_cases as cases
from tests.emul import build_emul
from tests.mix_loss_cases import MEAN, STD, loss, normalized

try:
    _EMUL = _lib.bind(ctypes.CDLL(build_emul.build()))
except FileNotFoundError:
    _EMUL = None

pytestmark = pytest.mark.skipif(_EMUL is None, reason="host emulation build unavailable")
CPU = torch.device("cpu")


def test_fixture_holds_the_cases_it_is_meant_to():
    m, G = cases.META, cases.GOLD
    assert {(v["mode"], v["N"], v["H"], v["W"]) for v in m.values()} >= {("elem", 6, 16, 32), ("elem", 6, 8, 24), ("elem", 4, 7, 9),
                                                                         ("pair", 4, 16, 32), ("pair", 2, 7, 9)}
    assert {v["K"] for v in m.values()} == {37, 1000}
    # elem_vec: a mixup row, a row left alone, and a CutMix row whose box the border clipped, xl and xh inside a 16-pixel vector
    assert cases.kinds("elem_vec") == {0, 1, 2}
    (i,) = np.flatnonzero(G["elem_vec__use_cutmix"] & (G["elem_vec__lam"] != 1.))
    yl, yh, xl, xh = G["elem_vec__boxes"][i]
    assert yh == 16 and xl % 16 and xh % 16 and G["elem_vec__lam"][i] == np.float32(1.0 - (yh - yl) * (xh - xl) / 512.0)
    lab = G["elem_vec__labels"]
    assert lab[0] == lab[5] and lab[1] != lab[4]
    # elem_rows: 24-pixel rows under 16-pixel vectors, at least two different boxes
    assert len({tuple(b) for b in G["elem_rows__boxes"] if b.any()}) >= 2
    assert cases.kinds("elem_odd") >= {1, 2} and cases.kinds("pair_vec") == {1, 2}
    for name in ("pair_vec", "pair_odd"):  # record N-1-n = record n
        t = cases.table_of(name).view(-1, 8)[1:]
        assert torch.equal(t, t.flip(0))
    # an empty box: CutMix was drawn, the corrected lam is 1
    e = G["elem_empty_box__use_cutmix"] & (G["elem_empty_box__lam"] == 1.)
    assert e.any() and all((b[1] - b[0]) * (b[3] - b[2]) == 0 for b in G["elem_empty_box__boxes"][e])


@pytest.mark.parametrize("name", cases.CASES)
def test_mix_equals_the_reference_collate_then_normalize(name):
    cases.check_mix_case(_EMUL, CPU, None, name)


@pytest.mark.parametrize("name", cases.CASES)
def test_soft_target_loss_and_gradient(name):
    cases.check_loss_case(_EMUL, CPU, None, name)


@pytest.mark.parametrize("name", cases.CASES)
def test_bf16_gradient_within_one_ulp(name):
    cases.check_bf16_case(_EMUL, CPU, None, name)


@pytest.mark.parametrize("name", ["elem_vec", "elem_rows", "elem_odd", "pair_vec"])
def test_rows_past_the_table_are_unmixed_and_nothing_behind_it_is_read(name):
    cases.check_short_table(_EMUL, CPU, None, name)


@pytest.mark.parametrize("name", ["elem_vec", "elem_odd"])
def test_other_header_modes_are_still_mode_0(name):
    cases.check_other_header_modes(_EMUL, CPU, None, name)


def test_odd_batch_is_refused():
    cases.check_odd_batch_is_refused(_EMUL, CPU)


@pytest.mark.parametrize("name,dtype,R", cases.FOOTPRINT, ids=[f"{n}-{str(d)[6:]}-R{r}" for n, d, r in cases.FOOTPRINT])
def test_footprint_and_placement_of_the_table_block(name, dtype, R):
    cases.check_footprint(_EMUL, name, dtype, R)


# ---- the Python surface on the emulated library

def _emulated(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: _EMUL)
    monkeypatch.setattr(_lib, "DEVICE_ONLY", False)


@pytest.mark.parametrize("name", cases.CASES)
def test_per_sample_mixup_and_loss_modules(name, monkeypatch):
    from cotnet_amd import MixedSoftTargetCrossEntropy, create_mixup
    _emulated(monkeypatch)
    meta = cases.META[name]
    m = create_mixup(device="cpu", capacity=8, **meta["kwargs"])
    assert m.params.shape == (8 * 9,) and m.params.dtype == torch.int32
    address = m.params.data_ptr()
    np.random.seed(meta["seed"])
    x = cases.gold(name, "x")
    lam, cut, boxes = m.draw(x.shape)
    assert m.params.data_ptr() == address
    assert np.array_equal(lam.view(np.int32), cases.GOLD[f"{name}__lam"].view(np.int32))
    y = m.mix_normalize(x, MEAN, STD, torch.float32)
    assert torch.equal(y, normalized(cases.gold(name, "mixed"), torch.float32))
    # the loss reads the same block; autograd gives the kernel's gradient
    logits = cases.gold(name, "logits").requires_grad_(True)
    out = MixedSoftTargetCrossEntropy(m)(logits, cases.gold(name, "labels"))
    (2 * out).backward()
    raw = loss(_EMUL, CPU, None, logits.detach(), cases.gold(name, "labels"), cases.table_of(name), 0.1, g=2.0)
    assert torch.equal(out.detach(), raw["mean"][0]) and torch.equal(logits.grad, raw["grad"])
    # switched off (the last epochs): a mode-0 header, and the batch passes unmixed
    m.mixup_enabled = False
    m.draw(x.shape)
    assert torch.equal(m.mix_normalize(x, MEAN, STD, torch.float32), normalized(x, torch.float32))


def test_the_loss_refuses_a_block_that_is_no_multiple_of_eight_words(monkeypatch):
    from cotnet_amd import soft_target_cross_entropy
    _emulated(monkeypatch)
    logits, labels = cases.gold("pair_odd", "logits"), cases.gold("pair_odd", "labels")
    for n in (0, 4, 12):
        with pytest.raises(ValueError, match="parameter block"):
            soft_target_cross_entropy(logits, labels, torch.zeros(n, dtype=torch.int32))
    soft_target_cross_entropy(logits, labels, cases.table_of("pair_odd"))
