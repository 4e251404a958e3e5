"""CoT models as feature backbones -- drop-in for the part of the reference's models/features.py the CoT entry points use.

    FeatureInfo                      reference :20-81, the same semantics
    FeatureDictNet, FeatureListNet   reference :153-232: an nn.ModuleDict over the wrapped model's own top-level children, in
                                     registration order, cut off behind the last module a requested tap needs; state_dict keys are
                                     the classifier model's keys for the kept modules

One departure: the forward.  The reference's `for name, module in self.items(): x = module(x)` would walk past everything that makes
these models fast here (stem_forward, pool, prepare_drop_path, plan_stage_layouts), so a wrapper runs `resnet.walk_features` -- the
call sequence `forward_features` of the wrapped class runs, with the class's own `walk_args` -- over the modules it kept and collects
the taps on the way.  Same launches as the classifier up to the last kept stage.

A tap is the tensor the tapped module returned: NCHW-contiguous, the model's activation dtype, part of the autograd graph, in storage
no later node, backward or forward writes (DESIGN 5.10 goes through every producer); `_tap` checks the layout and refuses anything else
instead of copying it quietly.  Under torch.cuda.graph capture the taps live in the graph's pool like every other tensor of the
capture: the next replay rewrites them.

`flatten_sequential=True` and `feature_cls='hook'` (FeatureHookNet) are not provided: no registered entry point uses either.
"""
from collections import OrderedDict
from copy import deepcopy

from torch import nn

from .resnet import walk_features


class FeatureInfo:
    def __init__(self, feature_info, out_indices):
        prev_reduction = 1
        for fi in feature_info:
            # the mandatory fields (a model may add more)
            assert "num_chs" in fi and fi["num_chs"] > 0
            assert "reduction" in fi and fi["reduction"] >= prev_reduction
            prev_reduction = fi["reduction"]
            assert "module" in fi
        self.out_indices = out_indices
        self.info = feature_info

    def from_other(self, out_indices):
        return FeatureInfo(deepcopy(self.info), out_indices)

    def get(self, key, idx=None):
        """idx None: the value at every output index; an int: at that feature index; a list / tuple: at each of those feature
        indices (both ignoring out_indices)"""
        if idx is None:
            return [self.info[i][key] for i in self.out_indices]
        if isinstance(idx, (tuple, list)):
            return [self.info[i][key] for i in idx]
        return self.info[idx][key]

    def get_dicts(self, keys=None, idx=None):
        """the info dicts, restricted to `keys` when given, at the indices `get` would use"""
        def pick(i):
            return self.info[i] if keys is None else {k: self.info[i][k] for k in keys}
        if idx is None:
            return [pick(i) for i in self.out_indices]
        if isinstance(idx, (tuple, list)):
            return [pick(i) for i in idx]
        return pick(idx)

    def channels(self, idx=None):
        return self.get("num_chs", idx)

    def reduction(self, idx=None):
        return self.get("reduction", idx)

    def module_name(self, idx=None):
        return self.get("module", idx)

    def __getitem__(self, item):
        return self.info[item]

    def __len__(self):
        return len(self.info)


def _get_feature_info(net, out_indices):
    feature_info = getattr(net, "feature_info")
    if isinstance(feature_info, FeatureInfo):
        return feature_info.from_other(out_indices)
    assert isinstance(feature_info, (list, tuple)), "Provided feature_info is not valid"
    return FeatureInfo(net.feature_info, out_indices)


def _get_return_layers(feature_info, out_map):
    return {name: (out_map[i] if out_map is not None else feature_info.out_indices[i])
            for i, name in enumerate(feature_info.module_name())}


def _tap(name, x):
    from .cot_block_cm import _is_cm
    if _is_cm(x) or not x.is_contiguous():
        raise RuntimeError(f"feature tap '{name}' is not NCHW-contiguous (strides {tuple(x.stride())}): the last block of a stage "
                           "writes NCHW, so this is a layout-planning bug")
    return x


class FeatureDictNet(nn.ModuleDict):
    """model -> OrderedDict of the feature maps at `out_indices` (into model.feature_info), keyed by str(index) or by `out_map`.
    The wrapped model has to be one of the classes `resnet.walk_features` runs (it states how as `walk_args`); it is taken apart:
    use the wrapper, not the model, afterwards.  `feature_concat` is accepted and has no effect (no CoT tap is a tuple)."""

    def __init__(self, model, out_indices=(0, 1, 2, 3, 4), out_map=None, feature_concat=False, flatten_sequential=False):
        super().__init__()
        if flatten_sequential:
            raise NotImplementedError("flatten_sequential=True is not provided: the stages run as whole nn.Sequential children")
        if not hasattr(model, "walk_args"):
            raise TypeError(f"{type(model).__name__} does not state how resnet.walk_features runs it (walk_args)")
        self.feature_info = _get_feature_info(model, out_indices)
        self.concat = feature_concat
        self.walk_args = dict(model.walk_args)
        self.return_layers = {}
        return_layers = _get_return_layers(self.feature_info, out_map)
        remaining = set(return_layers.keys())
        layers = OrderedDict()
        for name, module in model.named_children():
            layers[name] = module
            if name in remaining:
                self.return_layers[name] = str(return_layers[name])  # (the reference keeps the ids str: torchscript)
                remaining.remove(name)
            if not remaining:
                break
        assert not remaining and len(self.return_layers) == len(return_layers), \
            f"Return layers ({remaining}) are not present in model"
        self.update(layers)
        # (what a classifier checkpoint may hold beyond this wrapper's own keys: load_classifier_state_dict)
        self.dropped_modules = tuple(n for n, _ in model.named_children() if n not in layers)

    def _collect(self, x):
        out = OrderedDict()

        def tap(name, t):
            if name in self.return_layers:
                out[self.return_layers[name]] = _tap(name, t)
        walk_features(self, x, tap, **self.walk_args)
        return out

    def forward(self, x):
        return self._collect(x)


class FeatureListNet(FeatureDictNet):
    """the same, returning the list of the feature maps (in the order the modules run, as the reference's does)"""

    def forward(self, x):
        return list(self._collect(x).values())


def default_cfg_for_features(default_cfg):
    """the classifier's default_cfg without the fields that mean nothing for a backbone (reference helpers.py:253-260)"""
    default_cfg = deepcopy(default_cfg)
    for k in ("num_classes", "crop_pct", "classifier"):
        default_cfg.pop(k, None)
    return default_cfg


def load_classifier_state_dict(wrapper, state_dict):
    """a CLASSIFIER model's state_dict into a backbone: keys of top-level modules the wrapper dropped (fc.*, a dropped layerN.*,
    ...) are ignored -- they are told from foreign keys by `wrapper.dropped_modules`, the wrapped model's children that were not
    kept; every other unexpected key and every missing key raises, as a strict load does"""
    dropped = tuple(n + "." for n in getattr(wrapper, "dropped_modules", ()))
    kept = OrderedDict((k, v) for k, v in state_dict.items() if not (dropped and k.startswith(dropped)))
    return wrapper.load_state_dict(kept, strict=True)
