"""tests/golden/make_features_golden.py -- features_structure.json FROM THE REFERENCE ITSELF.

Builds the reference's own models with `features_only=True` on the CPU (the absent CuPy / yacs modules stubbed as
tests/golden/make_golden.py does, through oracle.build_ref.install_stubs) and records DATA only, per case: the wrapper's module keys in
order, `return_layers`, the whole `feature_info.info`, channels() / reduction() / module_name(), the sorted state_dict keys with their
shapes and the keys of the backbone's default_cfg.  No forward runs.  Runs only where the reference checkout exists.

The reference's build_model_with_cfg (models/helpers.py:311-357) defines `default_cfg_for_features` (:253-260) but leaves the
classifier's default_cfg on the model it wraps, which the wrapper then takes apart; the keys recorded here are that function applied to
the wrapped model's own default_cfg -- what cotnet_amd puts on the wrapper.

    python tests/golden/make_features_golden.py        # rewrites tests/golden/features_structure.json
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import build_ref  # noqa: E402
from tests.features_cases import STRUCTURE_CASES, case_id, describe, pack  # noqa: E402


def main():
    assert build_ref.reference_available(), "the reference checkout is required to regenerate fixtures"
    build_ref.install_stubs()
    import models  # noqa: F401  (the reference's package)
    from models.helpers import default_cfg_for_features
    import models.helpers as helpers

    seen = {}
    built = helpers.build_model_with_cfg

    def recording(model_cls, variant, pretrained, default_cfg, **kw):  # (the default_cfg the entry point hands over)
        seen["cfg"] = default_cfg
        return built(model_cls, variant, pretrained, default_cfg, **kw)

    out = {}
    for name, out_indices, output_stride in STRUCTURE_CASES:
        kw = {} if out_indices is None else {"out_indices": out_indices}
        for mod in list(sys.modules.values()):  # every module of the reference that imported the builder by name
            if getattr(mod, "build_model_with_cfg", None) is built and getattr(mod, "__name__", "").startswith("models."):
                mod.build_model_with_cfg = recording
        net = models.create_model(name, features_only=True, output_stride=output_stride, **kw)
        rec = describe(net)
        rec["default_cfg_keys"] = sorted(default_cfg_for_features(seen["cfg"]).keys())
        out[case_id(name, out_indices, output_stride)] = rec
    path = os.path.join(HERE, "features_structure.json")
    with open(path, "w") as fh:
        json.dump(pack(out), fh, sort_keys=True, separators=(",", ":"))
    print(f"features_structure: {len(out)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
