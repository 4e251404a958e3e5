"""ctypes binding of libcotnet_hip.so (the C ABI in include/cotnet_amd.h).

This is the only place the shared library is opened.  There is NO fallback: if the library is missing
or a call fails, a RuntimeError is raised (the product path must fail loudly, never silently compute
on the CPU).  The reference's equivalent is cupy_layers/utils.py:14-18 (`load_kernel`).
"""
import contextlib
import ctypes
import functools
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# COT_LIB_PATH: developer A/B of two builds of the library on one box (scripts/gpu_session.sh); the product loads the in-tree one
LIB_PATH = os.environ.get("COT_LIB_PATH") or os.path.join(_HERE, "lib", "libcotnet_hip.so")

COT_F32, COT_F64, COT_BF16, COT_F16 = 0, 1, 2, 3
COT_NCHW, COT_NHWC = 0, 1
COT_ERR_UNSUPPORTED = -2  # (cot_status, include/cotnet_amd.h)

_lib = None
_SHAPE_CACHES = []  # dicts of shape -> workspace size held by the Python wrappers (see register_cache)


def register_cache(d):
    """Workspace sizes are pure functions of (shape, tuning state).  The wrappers cache them per shape; every cache is
    registered here and emptied whenever a tuning key changes (several keys -- 11, 15, 17, 19, 20 -- change what
    cot_conv1x1_workspace / cot_conv3x3g_workspace return: a stale, smaller size would let a weight-gradient kernel write
    its partial sums past the end of the workspace; the ABI has no size argument to catch that)."""
    _SHAPE_CACHES.append(d)
    return d


def memo(cache):
    """decorator: fn(L, *key) answered out of `cache` (a register_cache dictionary) from the second call with a key on; the
    library handle L is passed on and is not part of the key"""
    def deco(fn):
        @functools.wraps(fn)
        def wrapped(L, *key):
            v = cache.get(key)
            if v is None:
                v = cache[key] = fn(L, *key)
            return v
        return wrapped
    return deco


class AggGeom(ctypes.Structure):
    """mirror of `cot_agg_geom`"""
    _fields_ = [(n, ctypes.c_int32) for n in (
        "N", "C", "H", "W", "heads", "wC", "kh", "kw", "sh", "sw", "ph", "pw", "dh", "dw")]


class ProfileRec(ctypes.Structure):
    """mirror of `cot_profile_rec`"""
    _fields_ = [("kernel", ctypes.c_char * 48), ("kind", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("dtype", ctypes.c_int32), ("layout", ctypes.c_int32), ("geom", AggGeom), ("ms", ctypes.c_float)]


# every symbol include/cotnet_amd.h declares: (restype, argtypes)
_P, _I = ctypes.c_void_p, ctypes.c_int
_G = ctypes.POINTER(AggGeom)
SYMBOLS = {
    "cot_abi_version": (_I, []),
    "cot_last_error": (ctypes.c_char_p, []),
    "cot_last_kernel": (ctypes.c_char_p, []),
    "cot_status_string": (ctypes.c_char_p, [_I]),
    "cot_agg_out_size": (_I, [_I] * 5),
    "cot_agg_forward": (_I, [_P, _P, _P, _G, _I, _I, _P]),
    "cot_agg_backward_input": (_I, [_P, _P, _P, _G, _I, _I, _P]),
    "cot_agg_backward_weight": (_I, [_P, _P, _P, _G, _I, _I, _P]),
    "cot_agg_backward": (_I, [_P, _P, _P, _P, _P, _G, _I, _I, _P]),
    "cot_agg_softmax_forward": (_I, [_P, _P, _P, _P, _G, _I, _P]),
    "cot_agg_softmax_backward": (_I, [_P, _P, _P, _P, _P, _G, _I, _P]),
    "cot_local_relation_workspace_bytes": (ctypes.c_int64, [_G, _I]),
    "cot_local_relation_forward": (_I, [_P] * 6 + [_G, _I, _P]),
    "cot_local_relation_backward": (_I, [_P] * 11 + [_G, _I, _P]),
    "cot_aggmix_forward": (_I, [_P, _P, _P, _P, _G, _I, _I, _I, _P]),
    "cot_aggmix_backward_input": (_I, [_P, _P, _P, _P, _G, _I, _I, _I, _I, _P]),
    "cot_aggmix_backward_weight": (_I, [_P, _P, _P, _P, _G, _I, _I, _I, _P]),
    "cot_set_tuning": (_I, [_I, _I]),
    "cot_get_tuning": (_I, [_I, ctypes.POINTER(_I)]),
    "cot_reset_tuning": (_I, []),
    "cot_tuning_name": (ctypes.c_char_p, [_I]),
    "cot_xchg_mode": (_I, []),
    "cot_launch_log": (_I, [ctypes.c_char_p, _I]),
    "cot_radix_gap": (_I, [_P, _P, _P, ctypes.c_int64, _I, _I, _P]),
    "cot_radix_mix": (_I, [_P, _P, _P, _P, ctypes.c_int64, _I, _I, _P]),
    "cot_radix_mix_backward": (_I, [_P] * 7 + [ctypes.c_int64, _I, _I, _P]),
    "cot_radix_gap_t": (_I, [_P, _P, _P, _I, _I, _I, _I, _P]),
    "cot_radix_mix_logits": (_I, [_P] * 5 + [_I, _I, _I, _I, _P]),
    "cot_radix_mix_backward_reduce": (_I, [_P] * 5 + [_I, _I, _I, _I, _P]),
    "cot_radix_mix_backward_apply": (_I, [_P] * 5 + [_I, _I, _I, _I, _P]),
    "cot_group_norm9_forward": (_I, [_P] * 6 + [_I, _I, _I, ctypes.c_float, _I, _P]),
    "cot_group_norm9_backward": (_I, [_P] * 9 + [_I, _I, _I, _I, _P]),
    "cot_gn9_stats_floats": (ctypes.c_int64, [_I, _I, _I]),
    "cot_gn9_fused_covers": (_I, [_I] * 5),
    "cot_conv1x1_forward_gn9": (_I, [_P, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "cot_gn9_stats_finalize": (_I, [_P, _P, _P, _I, _I, _I, ctypes.c_float, _P]),
    "cot_agg_gn9_forward": (_I, [_P] * 6 + [_I, _P, _G, _I, _P]),
    "cot_agg_gn9_backward": (_I, [_P] * 7 + [_I, _P, _P, _G, _I, _P]),
    "cot_subsample2_forward": (_I, [_P, _P, ctypes.c_int64, _I, _I, _I, _P]),
    "cot_subsample2_backward": (_I, [_P, _P, ctypes.c_int64, _I, _I, _I, _P]),
    "cot_avgpool2x2s2_forward": (_I, [_P, _P, ctypes.c_int64, _I, _I, _I, _P]),
    "cot_avgpool2x2s2_backward": (_I, [_P, _P, ctypes.c_int64, _I, _I, _I, _P]),
    "cot_avgpool3x3s2_forward": (_I, [_P, _P, ctypes.c_int64, _I, _I, _I, _P]),
    "cot_avgpool3x3s2_backward": (_I, [_P, _P, ctypes.c_int64, _I, _I, _I, _P]),
    "cot_maxpool3x3s2_forward": (_I, [_P, _P, ctypes.c_int64, _I, _I, _I, _P]),
    "cot_maxpool3x3s2_backward": (_I, [_P, _P, _P, ctypes.c_int64, _I, _I, _I, _P]),
    "cot_blurpool3x3s2_forward": (_I, [_P, _P, ctypes.c_int64, _I, _I, _I, _P]),
    "cot_blurpool3x3s2_backward": (_I, [_P, _P, ctypes.c_int64, _I, _I, _I, _P]),
    "cot_se_gap": (_I, [_P, _P, ctypes.c_int64, _I, _I, _P]),
    "cot_se_gate": (_I, [_P, _P, _P, ctypes.c_int64, _I, _I, _P]),
    "cot_se_gate_backward": (_I, [_P, _P, _P, _P, _P, ctypes.c_int64, _I, _I, _P]),
    "cot_maxpool3x3s2_forward_taps": (_I, [_P, _P, _P, ctypes.c_int64, _I, _I, _I, _P]),
    "cot_maxpool3x3s2_backward_taps": (_I, [_P, _P, _P, ctypes.c_int64, _I, _I, _I, _P]),
    "cot_stem7x7s2_workspace": (ctypes.c_int64, [_I, _I, _I]),
    "cot_stem7x7s2_forward": (_I, [_P, _P, _P, _I, _I, _I, _I, _P]),
    "cot_stem7x7s2_backward_weight": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "cot_stem3x3s2_workspace": (ctypes.c_int64, [_I, _I, _I, _I]),
    "cot_stem3x3s2_forward": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "cot_stem3x3s2_backward_weight": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "cot_sgd_step": (_I, [_P, _P, _P, _P, ctypes.c_int64, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                          _I, _I, _I, _P]),
    "cot_sgd_step_lr": (_I, [_P, _P, _P, _P, ctypes.c_int64, _P, ctypes.c_float, ctypes.c_float, ctypes.c_float, _I, _I, _I, _P]),
    "cot_grad_norm_parts": (_I, []),
    "cot_grad_sumsq": (_I, [_P, ctypes.c_int64, _I, _P, _P]),
    "cot_grad_clip_finish": (_I, [_P, ctypes.c_int64, ctypes.c_float, _P, _P]),
    "cot_sgd_step_clip": (_I, [_P, _P, _P, _P, ctypes.c_int64, ctypes.c_float, _P, _P, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                               _I, _I, _I, _P]),
    "cot_agc_max_groups": (_I, []),
    "cot_agc_clip": (_I, [_P, _P, _P, ctypes.c_int64, ctypes.c_int64, ctypes.c_float, ctypes.c_float, _P, _I, _P]),
    "cot_adam_tick": (_I, [_P, _P, ctypes.c_double, ctypes.c_double, _P]),
    "cot_adamw_step": (_I, [_P] * 5 + [ctypes.c_int64, ctypes.c_float, _P, _P, _P, ctypes.c_double, ctypes.c_double] + [ctypes.c_float] * 3 + [_I, _I, _I, _P]),
    "cot_lookahead_tick": (_I, [_P, _P, _I, _I, _P]),
    "cot_lookahead_step": (_I, [_P, _P, _P, ctypes.c_int64, ctypes.c_double, _P, _I, _P]),
    "cot_conv1x1_workspace": (ctypes.c_int64, [_I, _I, _I, _I, _I]),
    "cot_conv1x1_forward": (_I, [_P, _P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "cot_conv1x1_backward_data": (_I, [_P, _P, _P, _P, _I, _I, _P, _I, _I, _I, _I, _I, _P]),
    "cot_conv1x1_backward_weight": (_I, [_P, _P, _P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "cot_conv1x1_backward_data_relu_res_covers": (_I, [_I] * 5),
    "cot_conv1x1_backward_data_relu_res": (_I, [_P] * 5 + [_I] * 5 + [_P]),
    "cot_conv3x3g_masks_bytes": (ctypes.c_int64, [_I, _I]),
    "cot_conv3x3g_masks": (_I, [_P, _I, _I, _P]),
    "cot_conv3x3g_workspace": (ctypes.c_int64, [_I] * 6),
    "cot_conv3x3g_forward": (_I, [_P] * 5 + [_I] * 7 + [_P]),
    "cot_conv3x3g_backward_data": (_I, [_P] * 3 + [_I] + [_P] * 2 + [_I] * 7 + [_P]),
    "cot_conv3x3g_backward_weight": (_I, [_P] * 5 + [_I] * 7 + [_P]),
    "cot_conv3x3g_backward_weight_guarded": (_I, [_P] * 5 + [_I] * 8 + [_P]),
    "cot_conv3x3g_packed_bytes": (ctypes.c_int64, [_I] * 3),
    "cot_conv3x3g_pack": (_I, [_P, _P] + [_I] * 8 + [_P]),
    "cot_conv3x3g_forward_packed": (_I, [_P] * 3 + [_I] * 7 + [_P]),
    "cot_conv3x3g_backward_data_packed": (_I, [_P] * 3 + [_I] * 8 + [_P]),
    "cot_convg_workspace": (ctypes.c_int64, [_I] * 7),
    "cot_conv1x1g_forward": (_I, [_P] * 4 + [_I] * 6 + [_P]),
    "cot_conv1x1g_backward_data": (_I, [_P] * 3 + [_I] * 7 + [_P]),
    "cot_conv1x1g_backward_weight": (_I, [_P] * 5 + [_I] * 6 + [_P]),
    "cot_ema_step": (_I, [_P, _P, ctypes.c_int64, ctypes.c_float, _I, _P]),
    "cot_conv1x1_lds_covers": (_I, [_I, _I, _I, _I]),
    "cot_input_normalize": (_I, [_P, _P, _P, _P, ctypes.c_int64, _I, _I, _I, _P]),
    "cot_mix_normalize": (_I, [_P] * 5 + [_I] * 5 + [_P]),
    "cot_soft_target_ce_forward": (_I, [_P, _P, _P, ctypes.c_double, _P, _P, _P, _I, _I, _I, _P]),
    "cot_soft_target_ce_backward": (_I, [_P, _P, _P, ctypes.c_double, _P, _P, _P, _I, _I, _I, _P]),
    "cot_eval_score": (_I, [_P] * 5 + [_I, _I, _I, _P]),
    "cot_bn_act_workspace": (_I, [_I, _I]),
    "cot_bn_act_forward": (_I, [_P] * 11 + [_I, _I, _I, ctypes.c_float, ctypes.c_float, _I, _I, _P]),
    "cot_bn_act_backward": (_I, [_P] * 12 + [_I, _I, _I, _I, _I, _P]),
    "cot_bn_act_forward_ps": (_I, [_P] * 12 + [_I, _I, _I, ctypes.c_float, ctypes.c_float, _I, _I, _P]),
    "cot_bn_act_backward_ps": (_I, [_P] * 13 + [_I, _I, _I, _I, _I, _P]),
    "cot_bn_relu_mask_bytes": (ctypes.c_int64, [_I, _I, _I, _I]),
    "cot_bn_act_forward_mask": (_I, [_P] * 13 + [_I, _I, _I, ctypes.c_float, ctypes.c_float, _I, _I, _P]),
    "cot_bn_act_backward_mask": (_I, [_P] * 13 + [_I, _I, _I, _I, _I, _P]),
    "cot_conv1x1_stats_covers": (_I, [_I] * 4),
    "cot_conv1x1_forward_stats": (_I, [_P, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "cot_bn_tile_stats_finalize": (_I, [_P] * 6 + [_I, _I, _I, ctypes.c_float, ctypes.c_float, _P]),
    "cot_bn_act_apply_forward": (_I, [_P] * 8 + [_I, _I, _I, _I, _I, _P]),
    "cot_bn_act_lay_covers": (_I, [_I, _I, _I, _I]),
    "cot_bn_act_forward_lay": (_I, [_P] * 12 + [_I, _I, _I, ctypes.c_float, ctypes.c_float, _I, _I, _I, _P]),
    "cot_bn_act_backward_lay": (_I, [_P] * 13 + [_I, _I, _I, _I, _I, _I, _P]),
    "cot_radix_gap_t_lay": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _P]),
    "cot_radix_mix_logits_lay": (_I, [_P] * 5 + [_I, _I, _I, _I, _I, _P]),
    "cot_radix_mix_backward_reduce_lay": (_I, [_P] * 5 + [_I, _I, _I, _I, _I, _P]),
    "cot_radix_mix_backward_apply_lay": (_I, [_P] * 5 + [_I, _I, _I, _I, _I, _P]),
    "cot_agg_rowstats_floats": (ctypes.c_int64, [_I, _I, _I]),
    "cot_agg_forward_rowstats": (_I, [_P] * 8 + [_I, _G, _I, _P]),
    "cot_bn_rowstats_finalize": (_I, [_P] * 6 + [_I, _I, _I, _I, ctypes.c_float, ctypes.c_float, _P]),
    "cot_bn_batch_stats": (_I, [_P] * 7 + [_I, _I, _I, ctypes.c_float, ctypes.c_float, _I, _P]),
    "cot_bn_stats_sums": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "cot_radix_gap_t_bn": (_I, [_P] * 11 + [_I, _I, _I, ctypes.c_float, ctypes.c_float, _I, _I, _P]),
    "cot_radix_mix_logits_bn": (_I, [_P] * 9 + [_I, _I, _I, _I, _I, _P]),
    "cot_radix_mix_backward_reduce_bn": (_I, [_P] * 10 + [_I, _I, _I, _I, _I, _P]),
    "cot_radix_mix_backward_apply_bn": (_I, [_P] * 13 + [_I, _I, _I, _I, _I, _P]),
    "cot_group_norm9_forward_lay": (_I, [_P] * 6 + [_I, _I, _I, ctypes.c_float, _I, _I, _P]),
    "cot_group_norm9_backward_lay": (_I, [_P] * 9 + [_I, _I, _I, _I, _I, _P]),
    "cot_group_norm9_backward_params": (_I, [_P] * 3 + [_I, _I, _I, _P]),
    "cot_bn_act_inference": (_I, [_P] * 7 + [_I, _I, _I, ctypes.c_float, _I, _I, _P]),
    "cot_profile_begin": (_I, []),
    "cot_profile_end": (_I, [ctypes.POINTER(ProfileRec), _I]),
}
# the `int` returns that are a value, not a cot_status (a size, a count, a mode, a yes/no): api() passes them through unchecked
NOT_STATUS = frozenset((
    "cot_abi_version", "cot_agg_out_size", "cot_xchg_mode", "cot_launch_log", "cot_bn_act_workspace", "cot_profile_end",
    "cot_gn9_fused_covers", "cot_conv1x1_backward_data_relu_res_covers", "cot_conv1x1_lds_covers", "cot_bn_act_lay_covers",
    "cot_conv1x1_stats_covers", "cot_grad_norm_parts", "cot_agc_max_groups"))


def build(verbose=False):
    """Compile the HIP sources for gfx950 (used by __graft_entry__.build and by developers)."""
    import subprocess
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "-j8"]
    subprocess.check_call(cmd, stdout=None if verbose else subprocess.DEVNULL)
    return LIB_PATH


# How a wrapper calls the library.  `L = api()` is the library with every status checked: `L.cot_x(ptr(a), ..., stream())` raises
# CotError (the entry point's name, the status, cot_last_error()) unless it returns COT_OK; sizes, counts and the *_covers predicates
# (NOT_STATUS, the int64 / string returns) come back as they are.  lib() is the raw handle for callers that branch on a status.
# Every wrapper's eligible() and stream() read the one DEVICE_ONLY flag below, here, at call time.
#
# Module fallbacks.  Every wrapper (conv1x1, conv3x3g, fused_bn, group_norm9, pool3x3, stem7x7, head_fused) serves a tensor that is off its
# kernels' grid with the torch module it wraps.  While the library's kernels were asked for (the wrapper's switch is on) and the tensor is
# on a GPU, each such call is counted here per site (bench.py prints the counters as `module_fallbacks`), and COT_STRICT_DISPATCH=1
# turns it into an error -- for deployments that must never leave the hand-written path silently.
STRICT_DISPATCH = os.environ.get("COT_STRICT_DISPATCH", "0") == "1"
FALLBACKS = {}


def fallback(site, x=None, detail=""):
    if x is not None and not getattr(x, "is_cuda", False):
        return
    FALLBACKS[site] = FALLBACKS.get(site, 0) + 1
    if STRICT_DISPATCH:
        shape = tuple(x.shape) if x is not None else ()
        raise RuntimeError(f"{site}: {shape} {getattr(x, 'dtype', '')} {detail} is off the library's kernels and COT_STRICT_DISPATCH=1 "
                           "(the torch module would have run)")


def bind(cdll, lenient=False):
    """restype / argtypes of every SYMBOLS entry on a loaded library (lenient: entry points it lacks are simply not bound)"""
    for name, (res, args) in SYMBOLS.items():
        if lenient and not hasattr(cdll, name):
            continue
        fn = getattr(cdll, name)  # AttributeError here = header/library mismatch
        fn.restype, fn.argtypes = res, args
    return cdll


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). cotnet_amd has no CPU or eager fallback.")
        # (lenient under COT_LIB_PATH: a developer A/B against an OLDER build of the library)
        L = bind(ctypes.CDLL(LIB_PATH), lenient=bool(os.environ.get("COT_LIB_PATH")))
        if L.cot_abi_version() != 1:
            raise RuntimeError(f"libcotnet_hip.so ABI version {L.cot_abi_version()} != 1")
        def clearing(raw):  # every caller (tests, bench.py --tune, COT_TUNING) changes a key through these wrappers
            def fn(*args):
                for d in _SHAPE_CACHES:
                    d.clear()
                return raw(*args)
            return fn
        L.cot_set_tuning = clearing(L.cot_set_tuning)
        if hasattr(L, "cot_reset_tuning"):
            L.cot_reset_tuning = clearing(L.cot_reset_tuning)
        # developer knobs: COT_TUNING="12=1,bn_chan=0" -> cot_set_tuning(12, 1), cot_set_tuning(21, 0)  (include/cotnet_amd.h)
        for k, v in parse_tuning(os.environ.get("COT_TUNING", ""), L):
            if L.cot_set_tuning(k, v) != 0:
                raise RuntimeError(f"COT_TUNING: {L.cot_last_error().decode()}")
        _lib = L
    return _lib


# The tuning keys by name (enum cot_tuning_key in include/cotnet_amd.h).  Every helper takes the handle it steers: lib(), or a host
# build of the kernels bound with bind(ctypes.CDLL(...)) (the tests' emulator).
def tuning_keys(L):
    """{"BN_FOLD": 12, ...}: what cot_tuning_name tells of the handle's library"""
    names = ((k, L.cot_tuning_name(k)) for k in range(64))
    return {n.decode().upper(): k for k, n in names if n}


class Tune:
    """Tune(L).BN_FOLD == 12: the keys of a handle as attributes, asked for on first use (no handle: lib())"""

    def __init__(self, L=None):
        self._L = L

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        self.__dict__.update(tuning_keys(self._L or lib()))
        try:
            return self.__dict__[name]
        except KeyError:
            raise AttributeError(f"no tuning key {name}") from None


TUNE = Tune()


def _clear_caches():
    for d in _SHAPE_CACHES:
        d.clear()


def _set_tuning(L, key, value):
    _clear_caches()  # (lib()'s own cot_set_tuning does it too; an emulator handle's does not)
    if L.cot_set_tuning(key, value) != 0:
        raise RuntimeError(L.cot_last_error().decode())


def get_tuning(L, key):
    v = ctypes.c_int()
    if L.cot_get_tuning(key, ctypes.byref(v)) != 0:
        raise RuntimeError(L.cot_last_error().decode())
    return v.value


def reset_tuning(L):
    """every key back to the value the library starts with"""
    _clear_caches()
    L.cot_reset_tuning()


@contextlib.contextmanager
def tuned(L, **knobs):
    """with tuned(L, BN_FOLD=0, BN_CHAN=0): ... -- the keys set in the order given, the values they had put back in reverse order on
    the way out, whatever way that is.  Nests."""
    keys = tuning_keys(L)
    unknown = [n for n in knobs if n not in keys]
    if unknown:
        raise KeyError(f"no tuning key {unknown} (include/cotnet_amd.h: enum cot_tuning_key)")
    old = []
    try:
        for name, value in knobs.items():
            old.append((keys[name], get_tuning(L, keys[name])))
            _set_tuning(L, keys[name], value)
        yield
    finally:
        for key, value in reversed(old):
            _set_tuning(L, key, value)


def parse_tuning(text, L=None):
    """"12=1,bn_chan=0" -> [(12, 1), (21, 0)]: a key is its number or its name in either case (L: the handle the names are asked of,
    lib() by default and only when a name occurs)"""
    out = []
    for item in filter(None, (t.strip() for t in text.split(","))):
        k, v = item.split("=")
        out.append((int(k) if k.strip().lstrip("-").isdigit() else tuning_keys(L or lib())[k.strip().upper()], int(v)))
    return out


class CotError(RuntimeError):  # an entry point returned a cot_status other than COT_OK: .entry is its name, .status the code
    def __init__(self, status, entry, message):
        super().__init__(message)
        self.status, self.entry = status, entry


def check(status, what):
    if status != 0:
        L = lib()
        raise CotError(status, what, f"{what} failed: {L.cot_status_string(status).decode()} -- "
                                     f"{L.cot_last_error().decode()}")


class _Checked:
    """view of one library handle: a status entry point's wrapper is built on first use and found in the instance's dict from then
    on; it looks the entry point up on the handle per call, as `L.cot_x(...)` always did (tests rebind entry points there)"""

    def __init__(self, raw):
        self._raw = raw

    def __getattr__(self, name):
        raw = self._raw
        if name in NOT_STATUS or SYMBOLS.get(name, (None,))[0] is not _I:
            return getattr(raw, name)
        getattr(raw, name)  # (AttributeError here, not at the first launch)

        def fn(*args):
            rc = getattr(raw, name)(*args)
            if rc:
                check(rc, name)
        setattr(self, name, fn)
        return fn


_api = None


def api():
    """lib() with every status checked ("How a wrapper calls the library" above); follows whatever lib() returns now"""
    global _api
    L = lib()
    if _api is None or _api._raw is not L:
        _api = _Checked(L)
    return _api


def ptr(t):
    # a plain int is accepted for a c_void_p parameter and skips building a ctypes object per argument (~1000 per step)
    return t.data_ptr() if t is not None else None


DEVICE_ONLY = True  # False: CPU tensors reach the kernels too (tests, with a host-compiled build of them behind lib())
_TLS = threading.local()  # .st: the compute stream's handle for the node invocation running on this thread


def _current_stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def stream():
    if not DEVICE_ONLY:
        return None
    st = getattr(_TLS, "st", None)
    return st if st is not None else _current_stream()


def capturing():
    """True while the current stream records into a HIP graph: the launches issued now do not run until the graph is replayed, so
    nothing they are meant to fill may be put into a cache that eager calls read (cot_layer_fused, conv3x3g)"""
    if not DEVICE_ONLY:
        return False
    import torch
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def one_stream_query(fn):
    """torch.cuda.current_stream() costs ~9 us and a node makes ~100 launches: ask once per forward / backward of a node (the
    current stream cannot change inside one; forward and backward run on different threads, hence thread-local).  Measured:
    1.3 ms of a step's ~12 ms of host time (gpurun_out/r3_cpu_profile.log)"""
    @functools.wraps(fn)
    def wrapped(*a, **k):
        if not DEVICE_ONLY or getattr(_TLS, "st", None) is not None:
            return fn(*a, **k)
        _TLS.st = _current_stream()
        try:
            return fn(*a, **k)
        finally:
            _TLS.st = None
    return wrapped


def last_kernel():
    return lib().cot_last_kernel().decode()


_DTYPES = None


def dtype_code(torch_dtype):
    global _DTYPES
    if _DTYPES is None:
        import torch
        _DTYPES = {torch.float32: COT_F32, torch.float64: COT_F64, torch.bfloat16: COT_BF16, torch.float16: COT_F16}
    try:
        return _DTYPES[torch_dtype]
    except KeyError:
        raise TypeError(f"cotnet_amd: unsupported dtype {torch_dtype} (float32/float64/bfloat16/float16)")
