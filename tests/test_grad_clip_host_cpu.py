"""FlatSGD's clipping arguments on the host: what is refused, what means "off", what is allocated -- against the real library on CPU
tensors (construction launches nothing; cot_grad_norm_parts makes no HIP call), and the binding of the new entry points."""
import ctypes

import pytest
import torch
from torch import nn

from cotnet_amd import _lib
from cotnet_amd.flat_sgd import FlatSGD, to_mixed_bf16


def _model():
    torch.manual_seed(3)
    return to_mixed_bf16(nn.Sequential(nn.Linear(8, 8), nn.BatchNorm1d(8)).train())


def _opt(**kw):
    return FlatSGD(_model(), lr=0.1, momentum=0.9, weight_decay=4e-5, nesterov=True, **kw)


@pytest.mark.parametrize("mode", ["agc", "value", "Norm", None])
def test_other_clip_modes_raise_and_name_what_is_not_built(mode):
    with pytest.raises(ValueError, match="'value' and 'agc'"):
        _opt(clip_grad=1.0, clip_mode=mode)
    with pytest.raises(ValueError, match="only 'norm'"):
        _opt(clip_mode=mode)  # (also without clipping: a recipe that names another mode is told so)


@pytest.mark.parametrize("value", [None, 0, 0.0, -1, -1.0])
def test_none_zero_and_negative_clip_grad_mean_off(value):
    opt = _opt(clip_grad=value, clip_mode="norm")
    assert opt.clip_grad is None and opt.clip_state is None and opt._clip_parts is None and opt.skip_nonfinite is False
    with pytest.raises(RuntimeError, match="neither clip_grad nor skip_nonfinite"):
        opt.clip_stats()


@pytest.mark.parametrize("kw,clip", [(dict(clip_grad=2.5), 2.5), (dict(skip_nonfinite=True), None), (dict(clip_grad=-1, skip_nonfinite=True), None),
                                     (dict(clip_grad=3, skip_nonfinite=True, device_lr=True), 3.0)])
def test_either_request_allocates_the_block_and_the_partials_once(kw, clip):
    opt = _opt(**kw)
    parts = _lib.lib().cot_grad_norm_parts()
    assert parts >= 1 and opt.clip_grad == clip
    assert opt.clip_state.dtype == torch.int32 and opt.clip_state.shape == (8,) and not bool(opt.clip_state.any())
    assert opt._clip_parts.dtype == torch.float32 and opt._clip_parts.shape == (len(opt.reducer.buckets) * parts,)
    assert opt.clip_state.device == opt._clip_parts.device == opt.reducer.buckets[0].pflat.device
    assert opt.clip_state.data_ptr() % 4 == 0 and opt._clip_parts.data_ptr() % 4 == 0
    assert opt.clip_stats() == dict(total_norm=0.0, scale=0.0, skip=0, steps=0, clipped=0, skipped=0)


def test_clip_stats_is_refused_while_capturing(monkeypatch):
    opt = _opt(clip_grad=1.0)
    monkeypatch.setattr(_lib, "capturing", lambda: True)
    for _ in range(2):
        with pytest.raises(RuntimeError, match="inside a HIP-graph capture"):
            opt.clip_stats()
    monkeypatch.setattr(_lib, "capturing", lambda: False)
    assert opt.clip_stats()["steps"] == 0


def test_clip_stats_decodes_the_block():
    opt = _opt(clip_grad=1.0)
    opt.clip_state[:2] = torch.tensor([0.25, 4.0]).view(torch.int32)
    opt.clip_state[2:] = torch.tensor([1, 9, 4, 2, 0, 0], dtype=torch.int32)
    assert opt.clip_stats() == dict(total_norm=4.0, scale=0.25, skip=1, steps=9, clipped=4, skipped=2)


def test_the_new_entry_points_are_bound():
    L = _lib.lib()
    assert L.cot_abi_version() == 1
    assert "cot_grad_norm_parts" in _lib.NOT_STATUS and L.cot_grad_norm_parts() > 0
    for name in ("cot_grad_sumsq", "cot_grad_clip_finish", "cot_sgd_step_clip"):
        assert name in _lib.SYMBOLS and name not in _lib.NOT_STATUS and getattr(L, name).restype is ctypes.c_int
    # refused before any device work, so callable without a device
    assert L.cot_grad_clip_finish(None, 1, 1.0, None, None) == -1 and b"NULL" in L.cot_last_error()
    assert L.cot_grad_sumsq(None, 1, _lib.COT_F32, None, None) == -1
    assert L.cot_sgd_step_clip(None, None, None, None, 1, 0.1, None, None, 0.9, 0.0, 1.0, 1, _lib.COT_F32, _lib.COT_F32, None) == -1
