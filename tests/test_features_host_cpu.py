"""Feature backbones, host side (no compute): the structure of `create_model(..., features_only=True)` against what the reference's own
wrappers gave for the same cases (tests/golden/features_structure.json, written by tests/golden/make_features_golden.py), FeatureInfo's
accessors and checks, the keywords that are not provided, and the one departure in loading: a classifier checkpoint into a backbone."""
import json
import os

import pytest
import torch

import cotnet_amd
from cotnet_amd.features import FeatureDictNet, FeatureInfo, FeatureListNet, load_classifier_state_dict
from tests import features_cases as fc

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "features_structure.json")) as _fh:
    GOLDEN = fc.unpack(json.load(_fh))


def _meta(name, **kw):
    """built on the meta device: shapes and names without the initialisation's arithmetic"""
    with torch.device("meta"):
        return cotnet_amd.create_model(name, **kw)


def test_golden_covers_the_cases():
    assert sorted(GOLDEN) == sorted(fc.case_id(*c) for c in fc.STRUCTURE_CASES) and len(GOLDEN) == 48


@pytest.mark.parametrize("name,out_indices,output_stride", fc.STRUCTURE_CASES, ids=[fc.case_id(*c) for c in fc.STRUCTURE_CASES])
def test_structure_is_the_references(name, out_indices, output_stride):
    kw = {} if out_indices is None else {"out_indices": out_indices}
    net = _meta(name, features_only=True, output_stride=output_stride, **kw)
    assert isinstance(net, FeatureListNet)
    want = GOLDEN[fc.case_id(name, out_indices, output_stride)]
    got = fc.describe(net)
    got["default_cfg_keys"] = sorted(net.default_cfg)
    assert got.keys() == want.keys()
    for k in want:
        assert got[k] == want[k], k
    # the classifier model's keys for the kept modules, unchanged
    clsf = _meta(name, output_stride=output_stride)
    kept = {k: tuple(v.shape) for k, v in clsf.state_dict().items() if k.split(".")[0] in net.keys()}
    assert kept == {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert set(net.dropped_modules) == {n for n, _ in clsf.named_children()} - set(net.keys())


def test_default_indices_keep_everything_but_the_head():
    net = _meta("cotnet50", features_only=True)
    assert list(net.keys()) == ["conv1", "bn1", "act1", "maxpool", "layer1", "layer2", "layer3", "layer4"]
    assert net.dropped_modules == ("global_pool", "fc")
    net = _meta("cotnet50", features_only=True, out_indices=(1, 2))
    assert list(net.keys()) == ["conv1", "bn1", "act1", "maxpool", "layer1", "layer2"]
    assert not any(n.startswith(("layer3", "layer4", "fc")) for n, _ in net.named_parameters())
    assert _meta("cotnet50", features_only=True, output_stride=16).feature_info.reduction() == [2, 4, 8, 16, 16]
    assert _meta("cotnet50", features_only=True, output_stride=8).feature_info.reduction() == [2, 4, 8, 8, 8]
    assert _meta("se_cotnetd_50", features_only=True).feature_info.reduction() == [2, 4, 8, 16, 32]


@pytest.mark.parametrize("name", sorted(cotnet_amd.list_models()))
def test_every_entry_point_builds_a_backbone(name):
    net = _meta(name, features_only=True)
    assert isinstance(net, FeatureListNet) and net.feature_info.module_name() == list(fc.TAP_MODULES)
    assert "num_classes" not in net.default_cfg and "classifier" not in net.default_cfg and "crop_pct" not in net.default_cfg
    assert "input_size" in net.default_cfg and "mean" in net.default_cfg


def test_out_map_and_dict_wrapper():
    from cotnet_amd.cotnet import Bottleneck
    from cotnet_amd.resnet import ResNet
    with torch.device("meta"):
        net = FeatureDictNet(ResNet(Bottleneck, [1, 1, 1, 1]), out_indices=(1, 3), out_map=("c2", "c4"), feature_concat=True)
    assert net.return_layers == {"layer1": "c2", "layer3": "c4"} and "layer4" not in net.keys()
    with torch.device("meta"):
        net = FeatureDictNet(ResNet(Bottleneck, [1, 1, 1, 1]), out_indices=(0, 4))
    assert net.return_layers == {"act1": "0", "layer4": "4"}


def test_feature_cfg_of_the_builder():
    from cotnet_amd.cotnet import Bottleneck, default_cfgs
    from cotnet_amd.registry import build_model_with_cfg
    from cotnet_amd.resnet import ResNet
    CFG = next(iter(default_cfgs.values()))
    args = dict(block=Bottleneck, layers=[1, 1, 1, 1])
    with torch.device("meta"):
        cfg = {"out_indices": (2, 3), "feature_cls": FeatureDictNet, "out_map": ("a", "b")}
        net = build_model_with_cfg(ResNet, "cotnet50", False, CFG, feature_cfg=cfg, features_only=True, **args)
        assert type(net) is FeatureDictNet and net.return_layers == {"layer2": "a", "layer3": "b"}
        assert set(cfg) == {"out_indices", "feature_cls", "out_map"}  # (the caller's dict is left alone)
        net = build_model_with_cfg(ResNet, "cotnet50", False, CFG, feature_cfg={"out_indices": (2, 3)},
                                   features_only=True, out_indices=(4,), **args)  # the keyword overrides feature_cfg
        assert net.feature_info.out_indices == (4,)
        plain = build_model_with_cfg(ResNet, "cotnet50", False, CFG, feature_cfg={"out_indices": (2,)}, **args)
        assert isinstance(plain, ResNet) and "num_classes" in plain.default_cfg


def test_what_is_not_provided_says_so():
    from cotnet_amd.cotnet import Bottleneck, default_cfgs
    from cotnet_amd.registry import build_model_with_cfg
    from cotnet_amd.resnet import ResNet
    CFG = next(iter(default_cfgs.values()))
    with torch.device("meta"):
        with pytest.raises(NotImplementedError, match="flatten_sequential"):
            FeatureListNet(ResNet(Bottleneck, [1, 1, 1, 1]), flatten_sequential=True)
        with pytest.raises(NotImplementedError, match="feature_cls"):
            build_model_with_cfg(ResNet, "cotnet50", False, CFG, feature_cfg={"feature_cls": "hook"},
                                 features_only=True, block=Bottleneck, layers=[1, 1, 1, 1])
        with pytest.raises(NotImplementedError, match="pruned"):
            cotnet_amd.create_model("cotnet50", pruned=True)
        with pytest.raises(NotImplementedError, match="pruned"):
            cotnet_amd.create_model("cotnet50", features_only=True, pruned=True)


INFO = [dict(num_chs=64, reduction=2, module="act1"), dict(num_chs=256, reduction=4, module="layer1", extra="x"),
        dict(num_chs=512, reduction=8, module="layer2")]


def test_feature_info_accessors():
    fi = FeatureInfo([dict(d) for d in INFO], (0, 2))
    assert len(fi) == 3 and fi[1]["module"] == "layer1"
    assert fi.get("num_chs") == [64, 512] and fi.get("num_chs", 1) == 256 and fi.get("num_chs", (2, 0)) == [512, 64]
    assert fi.get("module", [1]) == ["layer1"]
    assert fi.channels() == [64, 512] and fi.reduction() == [2, 8] and fi.module_name() == ["act1", "layer2"]
    assert fi.channels(1) == 256 and fi.reduction((0, 1)) == [2, 4] and fi.module_name(2) == "layer2"
    assert fi.get_dicts() == [INFO[0], INFO[2]]
    assert fi.get_dicts(keys=("module",)) == [{"module": "act1"}, {"module": "layer2"}]
    assert fi.get_dicts(idx=1) == INFO[1] and fi.get_dicts(keys=("num_chs", "extra"), idx=1) == {"num_chs": 256, "extra": "x"}
    assert fi.get_dicts(idx=(1, 0)) == [INFO[1], INFO[0]]
    assert fi.get_dicts(keys=["reduction"], idx=[2]) == [{"reduction": 8}]
    other = fi.from_other((1,))
    assert other.out_indices == (1,) and other.info == fi.info and other.info is not fi.info and other.info[0] is not fi.info[0]
    assert other.channels() == [256] and fi.out_indices == (0, 2)


@pytest.mark.parametrize("bad", [dict(reduction=2, module="a"), dict(num_chs=0, reduction=2, module="a"), dict(num_chs=8, module="a"),
                                 dict(num_chs=8, reduction=2)])
def test_feature_info_checks_the_mandatory_fields(bad):
    with pytest.raises(AssertionError):
        FeatureInfo([bad], (0,))


def test_feature_info_wants_ascending_reductions():
    with pytest.raises(AssertionError):
        FeatureInfo([dict(num_chs=8, reduction=4, module="a"), dict(num_chs=8, reduction=2, module="b")], (0,))
    FeatureInfo([dict(num_chs=8, reduction=4, module="a"), dict(num_chs=8, reduction=4, module="b")], (0,))  # (dilated stages: equal)


def test_missing_tap_module_is_refused():
    from cotnet_amd.cotnet import Bottleneck
    from cotnet_amd.resnet import ResNet
    with torch.device("meta"):
        m = ResNet(Bottleneck, [1, 1, 1, 1])
    m.feature_info = [dict(num_chs=64, reduction=2, module="nowhere")]
    with pytest.raises(AssertionError, match="not present"):
        FeatureListNet(m, out_indices=(0,))


# ---- the checkpoint departure
def _small():
    from cotnet_amd.cotnet import Bottleneck
    from cotnet_amd.resnet import ResNet
    return ResNet(Bottleneck, [1, 1, 1, 1], num_classes=10)


@pytest.mark.parametrize("out_indices", [(0, 1, 2, 3, 4), (1, 2)])
def test_classifier_checkpoint_loads_into_a_backbone(tmp_path, out_indices):
    torch.manual_seed(1)
    clsf = fc.perturb(_small(), 2)
    sd = clsf.state_dict()
    path = str(tmp_path / "classifier.pth.tar")
    torch.save({"state_dict": {"module." + k: v for k, v in sd.items()}, "epoch": 3}, path)
    torch.manual_seed(3)
    body = FeatureListNet(_small(), out_indices=out_indices)
    assert not torch.equal(body.state_dict()["conv1.weight"], sd["conv1.weight"])
    cotnet_amd.load_checkpoint(body, path)
    got = body.state_dict()
    assert got and all(torch.equal(v, sd[k]) for k, v in got.items())
    assert ("layer3.0.conv1.weight" in got) == (out_indices != (1, 2))

    missing = {k: v for k, v in sd.items() if k != "layer1.0.bn1.weight"}
    torch.save({"state_dict": missing}, path)
    with pytest.raises(RuntimeError, match="Missing key.*layer1.0.bn1.weight"):
        cotnet_amd.load_checkpoint(body, path)
    foreign = dict(sd, **{"neck.weight": torch.zeros(1)})
    torch.save({"state_dict": foreign}, path)
    with pytest.raises(RuntimeError, match="Unexpected key.*neck.weight"):
        cotnet_amd.load_checkpoint(body, path)
    inside = dict(sd, **{"layer2.0.extra": torch.zeros(1)})  # a foreign key under a KEPT module
    with pytest.raises(RuntimeError, match="Unexpected key.*layer2.0.extra"):
        load_classifier_state_dict(body, inside)


def test_create_model_loads_a_classifier_checkpoint(tmp_path):
    """through the factory: create_model(name, features_only=True, checkpoint_path=p) on the smallest registered CoT model's keys (the
    meta device would not load, so this one builds lrnet50 -- no CoT layers to initialise, the cheapest entry point)"""
    torch.manual_seed(4)
    clsf = cotnet_amd.create_model("lrnet50", num_classes=7)
    path = str(tmp_path / "lrnet50.pth.tar")
    torch.save({"state_dict": clsf.state_dict()}, path)
    body = cotnet_amd.create_model("lrnet50", features_only=True, out_indices=(2,), checkpoint_path=path)
    sd = clsf.state_dict()
    assert list(body.keys())[-1] == "layer2" and all(torch.equal(v, sd[k]) for k, v in body.state_dict().items())
    # a backbone's own state_dict loads back strictly
    cotnet_amd.create_model("lrnet50", features_only=True, out_indices=(2,)).load_state_dict(body.state_dict())


def test_exports():
    assert cotnet_amd.FeatureInfo is FeatureInfo and cotnet_amd.FeatureListNet is FeatureListNet
    assert cotnet_amd.FeatureDictNet is FeatureDictNet and issubclass(FeatureListNet, FeatureDictNet)
    assert issubclass(FeatureDictNet, torch.nn.ModuleDict)
