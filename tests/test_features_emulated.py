"""Feature backbones on the host emulator: a small ResNet of CoT Bottlenecks (one block per stage) through the checks of
tests/features_cases.py -- every tap bit-equal to what a hook on the classifier model of the same weights saw, the node counts those of the classifier's forward up to the last kept stage, bit-equal
parameter gradients, and the taps intact after a backward, another forward and the classifier's forward."""
import ctypes

import pytest
import torch

from cotnet_amd import _lib
from tests import features_cases as fc
from tests.emul import build_emul

try:
    _EMUL = _lib.bind(ctypes.CDLL(build_emul.build()))
except FileNotFoundError:
    _EMUL = None

pytestmark = pytest.mark.skipif(_EMUL is None, reason="host emulation build unavailable")
LAYERS = [1, 1, 1, 1]  # (planes of 4 x 6 and 2 x 3 pixels are off the channel-major node's geometries: NCHW nodes; the device tests cover it)


def _small():
    from cotnet_amd.cotnet import Bottleneck
    from cotnet_amd.resnet import ResNet
    return ResNet(Bottleneck, LAYERS, num_classes=10)


@pytest.fixture
def emulated(monkeypatch):
    import cotnet_amd.aggregation_zeropad as az
    from cotnet_amd import (cot_layer_fused as clf, conv1x1 as c1, conv3x3g as c3, fused_bn, group_norm9 as g9, head_fused as hf,
                            pool3x3 as p3, stem7x7 as s7)
    from tests.test_kernels_emulated import _EmulAggregation
    monkeypatch.setattr(_lib, "lib", lambda: _EMUL)
    monkeypatch.setattr(_lib, "DEVICE_ONLY", False)
    monkeypatch.setattr(az, "aggregation_zeropad", lambda i, w, kernel_size=3, stride=1, padding=0, dilation=1: _EmulAggregation.apply(i, w))
    monkeypatch.setattr(clf, "ENABLED", True)
    monkeypatch.setattr(clf, "CM_LAYOUT", True)
    for mod in (c1, c3, g9, p3, hf, s7):
        monkeypatch.setattr(mod, "MODE", "hip")
    caches = (clf._SIZES, clf._MASKS, clf._BSIZES, clf._CM_SIZES, clf._CM_OK, c1._WS, c3._WS, c3._MASKS, fused_bn._WS, hf._WS)
    for cache in caches:
        cache.clear()
    yield clf
    for cache in caches:
        cache.clear()


def _twins(out_indices, train=True):
    from cotnet_amd.features import FeatureListNet
    return fc.twins(_small, lambda: FeatureListNet(_small(), out_indices=out_indices), "cpu", mixed=True, train=train, seed=11)


@pytest.mark.parametrize("out_indices", [(0, 1, 2, 3, 4), (1, 2)])  # ((4,) runs on the device: the emulator's time goes into the stem)
def test_taps_and_gradients_equal_the_classifiers(emulated, out_indices):
    torch.manual_seed(3)
    x = torch.randn(2, 3, 64, 96).bfloat16()
    clsf, body = _twins(out_indices)
    h = fc.hooked_forward(clsf, x)
    taps, counts = fc.backbone_forward(body, x)
    assert sorted(taps) == sorted(out_indices)
    fc.check_taps(taps, counts, h, torch.bfloat16)
    assert sum(counts.values()) == sum(LAYERS[:max(out_indices)]), counts  # (even planes throughout: every kept block ran as a node)
    fc.check_gradients(body, clsf, taps, h)
    for (n, p, q), (_, b) in zip(fc.kept_parameters(body, clsf), body.named_parameters()):
        assert p is b
    for n, b in body.named_buffers():  # training-mode statistics moved the same way
        assert torch.equal(b, dict(clsf.named_buffers())[n]), n


def test_tap_lifetime(emulated):
    torch.manual_seed(4)
    x, x2 = torch.randn(2, 3, 64, 64).bfloat16(), torch.randn(2, 3, 64, 64).bfloat16()
    clsf, body = _twins((0, 1, 2, 3, 4))
    fc.check_lifetime(body, clsf, x, x2)


def test_dict_wrapper_and_eval_mode(emulated):
    from cotnet_amd.features import FeatureDictNet
    torch.manual_seed(5)
    x = torch.randn(2, 3, 64, 64).bfloat16()
    clsf, body = fc.twins(_small, lambda: FeatureDictNet(_small(), out_indices=(1, 3), out_map=("c2", "c4")), "cpu", train=False, seed=12)
    with torch.no_grad():
        h = fc.hooked_forward(clsf, x)
        out = body(x)
        assert list(out) == ["c2", "c4"]
        taps, counts = fc.backbone_forward(body, x)
    fc.check_taps(taps, counts, h, torch.bfloat16)
    assert counts["bottleneck_eval"] == sum(LAYERS[:3]), counts
    assert torch.equal(out["c2"], taps[1]) and torch.equal(out["c4"], taps[3])
