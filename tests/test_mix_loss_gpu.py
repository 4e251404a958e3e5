"""The recipe's mixup / CutMix pass and soft-target loss (csrc/mix_loss.hip) on the device: the cases and criteria of
tests/test_mix_loss_emulated.py (tests/mix_loss_cases.py) against the HIP library, one loss case at the recipe's own row length and batch
parity (N = 80, K = 1000, bf16), and two mixing cases at sizes the fixture does not hold: 4 x 3 x 224 x 224, and one whose vector count
exceeds the grid (4096 blocks x 256 lanes), so that lanes take a second round of the grid-stride loop."""
import numpy as np
import pytest
import torch

from cotnet_amd import _lib
from cotnet_amd.mixup import pack_params
from tests import mix_loss_cases as cases

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def run(check, *a):
    return check(_lib.lib(), DEV, _lib.stream(), *a, sync=torch.cuda.synchronize)


@pytest.mark.parametrize("name", cases.CASES)
def test_mix_equals_the_reference_collate_then_normalize(name):
    run(cases.check_mix_case, name)


def test_refusals_come_before_any_launch():
    cases.check_mix_refusals(_lib.lib(), DEV)


@pytest.mark.parametrize("name", cases.CASES)
def test_soft_target_loss_and_gradient(name):
    run(cases.check_soft_case, name)


@pytest.mark.parametrize("name", cases.CASES)
def test_label_smoothing_is_mode_0(name):
    run(cases.check_label_smoothing_case, name)


@pytest.mark.parametrize("name", cases.CASES)
def test_plain_cross_entropy_is_mode_0_without_smoothing(name):
    run(cases.check_plain_ce_case, name)


@pytest.mark.parametrize("name", cases.CASES)
def test_bf16_gradient_within_one_ulp(name):
    run(cases.check_bf16_case, name)


def test_out_of_range_labels_match_no_column():
    run(cases.out_of_range_labels)


def test_dense_target_is_the_torch_formula_and_is_counted(monkeypatch):
    """a caller-made dense [N, K] target: the reference's formula in torch, counted per site, an error under COT_STRICT_DISPATCH"""
    from cotnet_amd import soft_target_cross_entropy
    name = "cutmix_vec"
    logits, target = cases.gold(name, "logits").to(DEV), cases.gold(name, "target").to(DEV)
    blk = pack_params(0, 1.).to(DEV)
    _lib.FALLBACKS.clear()
    got = soft_target_cross_entropy(logits, target, blk)
    assert _lib.FALLBACKS == {"soft_target_cross_entropy": 1}
    want = torch.sum(-target * torch.log_softmax(logits, dim=-1), dim=-1).mean()
    assert torch.equal(got, want)
    soft_target_cross_entropy(logits, cases.gold(name, "labels").to(DEV), blk)  # integer labels: the kernels, not counted
    assert _lib.FALLBACKS == {"soft_target_cross_entropy": 1}
    monkeypatch.setattr(_lib, "STRICT_DISPATCH", True)
    with pytest.raises(RuntimeError, match="COT_STRICT_DISPATCH"):
        soft_target_cross_entropy(logits, target, blk)
    _lib.FALLBACKS.clear()


def _dense_target(labels, K, lam, smoothing):
    """mixup_target's formula (datasets/mixup.py:22-27) in fp32 torch"""
    off = smoothing / K
    on = 1. - smoothing + off
    y1 = torch.full((len(labels), K), off).scatter_(1, labels.view(-1, 1), on)
    y2 = torch.full((len(labels), K), off).scatter_(1, labels.flip(0).view(-1, 1), on)
    return y1 * lam + y2 * (1. - lam)


def _soft(logits, target, dtype):
    x = logits.detach().clone().to(dtype).requires_grad_(True)
    rows = torch.sum(-target.to(dtype) * torch.log_softmax(x, dim=-1), dim=-1)
    rows.mean().backward()
    return rows.mean().detach(), rows.detach(), x.grad


def test_recipe_batch_80_by_1000_bf16():
    """no fixture at this size: the reference's formulas in torch on the CPU, fp32 against fp64 for the allowance as everywhere"""
    g = torch.Generator().manual_seed(80)
    N, K, lam = 80, 1000, 0.37281
    logits = (3.0 * torch.randn(N, K, generator=g)).bfloat16()
    labels = torch.randint(0, K, (N,), generator=g)
    labels[N - 1 - 5] = labels[5]  # one pair with equal labels
    target = _dense_target(labels, K, lam, 0.1)
    r32, r64 = _soft(logits.float(), target, torch.float32), _soft(logits.float(), target, torch.float64)
    got = run(cases.loss, logits, labels, pack_params(1, lam), 0.1)
    cases.check_bf16_grad(got["grad"], r64[2], "N = 80, K = 1000")
    a_mean, a_rows, _ = cases.allowances(*r32, *r64)
    e_mean = abs(float(got["mean"]) - float(r64[0]))
    e_rows = float((got["rows"].double() - r64[1]).abs().max())
    print(f"N = 80, K = 1000 bf16: mean loss error {e_mean:.3e} (allowance {a_mean:.3e}), row loss error {e_rows:.3e} (allowance {a_rows:.3e})")
    assert e_mean <= a_mean and e_rows <= a_rows
    again = run(cases.loss, logits, labels, pack_params(1, lam), 0.1)
    assert all(torch.equal(got[k], again[k]) for k in got)


def _mixed_numpy(x, mode, lam, box):
    """_mix_batch_collate's arithmetic (datasets/mixup.py:288-298) on the whole batch"""
    a, b = x.numpy(), x.flip(0).numpy()
    if mode == 1:
        m = a.astype(np.float32) * lam + b.astype(np.float32) * (1 - lam)
        np.rint(m, out=m)
        return torch.from_numpy(m.astype(np.uint8))
    out = a.copy()
    yl, yh, xl, xh = box
    out[:, :, yl:yh, xl:xh] = b[:, :, yl:yh, xl:xh]
    return torch.from_numpy(out)


@pytest.mark.parametrize("shape,mode", [((4, 3, 224, 224), 1), ((4, 3, 224, 224), 2), ((2, 3, 1680, 1680), 1), ((2, 3, 1680, 1680), 2)],
                         ids=["224-mixup", "224-cutmix", "second-round-mixup", "second-round-cutmix"])
def test_mix_at_image_sizes(shape, mode):
    N, C, H, W = shape
    if H == 1680:
        assert N * C * H * W // 16 > 4096 * 256  # more vectors than lanes in the grid
    g = torch.Generator().manual_seed(H + mode)
    x = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
    lam, box = 0.6180339887498949, (H // 3 + 1, H - 5, 37, W - 19)  # box edges inside 16-pixel vectors
    rc, y, intact = cases.mix(_lib.lib(), DEV, _lib.stream(), x, pack_params(mode, lam, box).to(DEV), torch.bfloat16,
                              torch.cuda.synchronize)
    assert rc == 0 and intact
    assert torch.equal(y, cases.normalized(_mixed_numpy(x, mode, lam, box), torch.bfloat16))
