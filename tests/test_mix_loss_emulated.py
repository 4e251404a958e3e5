"""The recipe's mixup / CutMix pass and soft-target loss (csrc/mix_loss.hip) on the host emulator, through the C ABI, against the reference's
own results -- the cases and criteria are in tests/mix_loss_cases.py (tests/test_mix_loss_gpu.py runs the same on the device) -- and the
Python surface (cotnet_amd.mixup, cotnet_amd.loss) on top of the emulated library."""
import ctypes

import numpy as np
import pytest
import torch

from cotnet_amd import _lib
from tests import mix_loss_cases as cases
from tests.emul import build_emul

try:
    _EMUL = _lib.bind(ctypes.CDLL(build_emul.build()))
except FileNotFoundError:
    _EMUL = None

pytestmark = pytest.mark.skipif(_EMUL is None, reason="host emulation build unavailable")
CPU = torch.device("cpu")


@pytest.mark.parametrize("name", cases.CASES)
def test_mix_equals_the_reference_collate_then_normalize(name):
    cases.check_mix_case(_EMUL, CPU, None, name)


def test_fixture_holds_the_cases_it_is_meant_to():
    m = cases.META
    assert {(v["N"], v["H"], v["W"]) for v in m.values()} >= {(4, 16, 32), (4, 7, 9), (2, 16, 32)}
    assert {(v["N"], v["K"]) for v in m.values()} >= {(4, 1000), (4, 37), (2, 10)}
    yl, yh, xl, xh = m["cutmix_vec"]["box"]
    assert m["cutmix_vec"]["use_cutmix"] and xl % 16 and xh % 16 and yh == 16  # clipped by the border, edges inside a 16-pixel vector
    assert m["cutmix_vec"]["lam"] == 1.0 - (yh - yl) * (xh - xl) / 512.0
    assert m["lam1_n2"]["lam"] == 1.0 and not m["mixup_vec"]["use_cutmix"] and m["mixup_vec"]["lam"] < 1
    lab = cases.gold("mixup_vec", "labels")
    assert lab[0] == lab[3] and lab[1] != lab[2]


def test_refusals_come_before_any_launch():
    cases.check_mix_refusals(_EMUL, CPU)


@pytest.mark.parametrize("name", cases.CASES)
def test_soft_target_loss_and_gradient(name):
    cases.check_soft_case(_EMUL, CPU, None, name)


@pytest.mark.parametrize("name", cases.CASES)
def test_label_smoothing_is_mode_0(name):
    cases.check_label_smoothing_case(_EMUL, CPU, None, name)


@pytest.mark.parametrize("name", cases.CASES)
def test_plain_cross_entropy_is_mode_0_without_smoothing(name):
    cases.check_plain_ce_case(_EMUL, CPU, None, name)


@pytest.mark.parametrize("name", cases.CASES)
def test_bf16_gradient_within_one_ulp(name):
    cases.check_bf16_case(_EMUL, CPU, None, name)


def test_out_of_range_labels_match_no_column():
    cases.out_of_range_labels(_EMUL, CPU, None)


# ---- the Python surface on the emulated library

def _emulated(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: _EMUL)
    monkeypatch.setattr(_lib, "DEVICE_ONLY", False)


def test_device_mixup_and_loss_modules(monkeypatch):
    from cotnet_amd import DeviceMixup, LabelSmoothingCrossEntropy, MixedSoftTargetCrossEntropy, soft_target_cross_entropy
    _emulated(monkeypatch)
    name = "cutmix_vec"
    meta = cases.META[name]
    kw = {k: v for k, v in meta["kwargs"].items()}
    m = DeviceMixup(device="cpu", **kw)
    np.random.seed(meta["seed"])
    x = cases.gold(name, "x")
    assert m.draw(x.shape) == (meta["lam"], meta["use_cutmix"], tuple(meta["box"]))
    y = m.mix_normalize(x, cases.MEAN, cases.STD, torch.float32)
    assert torch.equal(y, cases.normalized(cases.gold(name, "mixed"), torch.float32))
    out = torch.empty_like(y)
    assert m.mix_normalize(x, cases.MEAN, cases.STD, torch.float32, out=out) is out and torch.equal(out, y)
    with pytest.raises(_lib.CotError, match="odd"):
        m.mix_normalize(x[:3].contiguous(), cases.MEAN, cases.STD)
    # the loss reads the same block; autograd gives the kernel's gradient
    logits = cases.gold(name, "logits").requires_grad_(True)
    loss_fn = MixedSoftTargetCrossEntropy(m)
    assert loss_fn.smoothing == 0.1
    loss = loss_fn(logits, cases.gold(name, "labels"))
    (2 * loss).backward()
    raw = cases.loss(_EMUL, CPU, None, logits.detach(), cases.gold(name, "labels"), m.params, 0.1, g=2.0)
    assert torch.equal(loss.detach(), raw["mean"][0]) and torch.equal(logits.grad, raw["grad"])
    # label smoothing: the reference's signature
    ls = LabelSmoothingCrossEntropy(0.1)
    assert (ls.smoothing, ls.confidence) == (0.1, 0.9)
    got = ls(cases.gold(name, "logits"), cases.gold(name, "labels"))
    assert abs(float(got) - float(cases.gold(name, "ls_loss_f64"))) <= 1e-5
    # a dense target is the torch formula (counted on the device only: tests/test_mix_loss_gpu.py)
    dense = soft_target_cross_entropy(cases.gold(name, "logits"), cases.gold(name, "target"), m)
    assert torch.equal(dense, cases.gold(name, "soft_loss_f32"))
    with pytest.raises(TypeError):
        soft_target_cross_entropy(cases.gold(name, "logits"), cases.gold(name, "labels").int(), m)


def test_draw_inside_a_capture_raises(monkeypatch):
    from cotnet_amd import DeviceMixup
    _emulated(monkeypatch)
    m = DeviceMixup(device="cpu")
    monkeypatch.setattr(_lib, "capturing", lambda: True)
    before = m.params.clone()
    with pytest.raises(RuntimeError, match="between replays"):
        m.draw((2, 3, 8, 8))
    assert torch.equal(m.params, before)
