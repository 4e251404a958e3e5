"""The C-ABI library loads and exports every symbol include/cotnet_amd.h declares (no compute without a GPU);
argument validation happens before any device work and reports through cot_last_error()."""
import ctypes
import os
import re

import pytest

from cotnet_amd import _lib
from tests.conftest import ROOT


def header_functions():
    src = open(os.path.join(ROOT, "include", "cotnet_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(cot_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    assert os.path.exists(_lib.LIB_PATH), "libcotnet_hip.so missing: run __graft_entry__.build()"
    L = ctypes.CDLL(_lib.LIB_PATH)
    names = header_functions()
    assert len(names) >= 12
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/cotnet_amd.h but not exported"
    assert sorted(_lib.SYMBOLS) == names, "cotnet_amd/_lib.py SYMBOLS out of sync with the header"


def test_abi_version_and_status_strings():
    L = _lib.lib()
    assert L.cot_abi_version() == 1
    assert L.cot_status_string(0) == b"ok"
    assert L.cot_status_string(-1) == b"invalid argument"


def test_out_size_matches_reference_formula():
    L = _lib.lib()
    for H in (7, 14, 28, 56, 9, 11):
        for k, s, p, d in ((3, 1, 1, 1), (5, 1, 2, 1), (3, 2, 1, 1), (3, 1, 2, 2), (1, 1, 0, 1)):
            assert L.cot_agg_out_size(H, k, s, p, d) == int((H + 2 * p - (d * (k - 1) + 1)) / s + 1)


def test_validation_errors_without_touching_the_gpu():
    L = _lib.lib()
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: validation fails first
    g = _lib.AggGeom(2, 10, 8, 8, 1, 4, 3, 3, 1, 1, 1, 1, 1, 1)  # C % wC != 0
    rc = L.cot_agg_forward(fake, fake, fake, ctypes.byref(g), _lib.COT_F32, _lib.COT_NCHW, None)
    assert rc == -1 and b"not divisible" in L.cot_last_error()
    g = _lib.AggGeom(2, 8, 8, 8, 1, 4, 3, 3, 1, 1, 1, 1, 1, 1)
    assert L.cot_agg_forward(None, fake, fake, ctypes.byref(g), _lib.COT_F32, _lib.COT_NCHW, None) == -1
    assert L.cot_agg_forward(fake, fake, fake, ctypes.byref(g), 99, _lib.COT_NCHW, None) == -2
    assert L.cot_agg_forward(fake, fake, fake, ctypes.byref(g), _lib.COT_F32, 7, None) == -2
    assert L.cot_agg_forward(ctypes.c_void_p(0x1004), fake, fake, ctypes.byref(g), _lib.COT_F32, 0, None) == -1
    assert b"16-byte" in L.cot_last_error()
    assert L.cot_agg_backward(fake, fake, fake, None, None, ctypes.byref(g), 0, 0, None) == -1
    g5 = _lib.AggGeom(2, 8, 8, 8, 1, 4, 5, 5, 1, 1, 2, 2, 1, 1)
    assert L.cot_aggmix_forward(fake, fake, fake, fake, ctypes.byref(g5), 2, 2, 0, None) == -1
    with pytest.raises(RuntimeError, match="invalid argument"):
        _lib.check(-1, "probe")


def test_not_status_set_matches_the_header():
    """_lib.NOT_STATUS names exactly the `int` returns that are values; every other `int` entry point is one the header declares,
    i.e. one under its convention "return value: COT_OK (0) or a negative cot_status" """
    ints = {n for n, (res, _) in _lib.SYMBOLS.items() if res is ctypes.c_int}
    assert _lib.NOT_STATUS <= ints, sorted(_lib.NOT_STATUS - ints)
    assert {n for n in ints if n.endswith("_covers")} <= _lib.NOT_STATUS
    declared = set(header_functions())
    for n in ints - _lib.NOT_STATUS:
        assert n in declared, n


def test_checked_view_raises_with_entry_and_status():
    """_lib.api(): a status other than COT_OK raises CotError naming the entry point; values pass through unchecked"""
    A = _lib.api()
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: validation fails first
    g = _lib.AggGeom(2, 10, 8, 8, 1, 4, 3, 3, 1, 1, 1, 1, 1, 1)  # C % wC != 0
    with pytest.raises(_lib.CotError, match="cot_agg_forward failed: invalid argument -- .*not divisible") as e:
        A.cot_agg_forward(fake, fake, fake, ctypes.byref(g), _lib.COT_F32, _lib.COT_NCHW, None)
    assert isinstance(e.value, RuntimeError) and e.value.status == -1 and e.value.entry == "cot_agg_forward"
    g = _lib.AggGeom(2, 8, 8, 8, 1, 4, 3, 3, 1, 1, 1, 1, 1, 1)
    with pytest.raises(_lib.CotError) as e:
        A.cot_agg_forward(fake, fake, fake, ctypes.byref(g), 99, _lib.COT_NCHW, None)
    assert e.value.status == _lib.COT_ERR_UNSUPPORTED and e.value.entry == "cot_agg_forward"
    with pytest.raises(_lib.CotError) as e:
        _lib.check(-1, "probe")
    assert (e.value.status, e.value.entry) == (-1, "probe")
    assert A.cot_conv1x1_lds_covers(256, 256, 0, 3136) == 1 and A.cot_conv1x1_lds_covers(7, 7, 0, 3136) == 0  # predicates: no raise
    assert A.cot_abi_version() == 1 and A.cot_agg_out_size(8, 3, 1, 1, 1) == 8
    assert A.cot_status_string(-1) == b"invalid argument"
    assert _lib.api() is A and A._raw is _lib.lib()  # one view per handle


def test_checked_view_follows_lib(monkeypatch):
    """the view is resolved from _lib.lib() at use: a test that swaps the library swaps what the wrappers launch"""
    class Other:
        def cot_agg_forward(self, *a):
            return 0

        def cot_abi_version(self):
            return 7
    other = Other()
    real = _lib.api()
    monkeypatch.setattr(_lib, "lib", lambda: other)
    assert _lib.api()._raw is other and _lib.api().cot_abi_version() == 7 and _lib.api().cot_agg_forward(1, 2) is None
    monkeypatch.undo()
    assert _lib.api()._raw is real._raw


_TUNING_KEYS_CHILD = r"""
import ctypes, sys
from cotnet_amd import _lib
L = ctypes.CDLL(_lib.LIB_PATH)
L.cot_last_error.restype = ctypes.c_char_p
assert L.cot_set_tuning(26, 1) == 0  # dry run: no launch, no HIP call
bad = []
for key in list(range(0, 35)) + list(range(36, 55)):
    for value in (0, 1):
        if L.cot_set_tuning(key, value) != 0:
            bad.append((key, value, L.cot_last_error()))
for key in (-1, 35, 55):
    rc = L.cot_set_tuning(key, 1)
    if rc != -1 or b"unknown tuning key" not in L.cot_last_error():
        bad.append((key, rc, L.cot_last_error()))
print("BAD", bad)
sys.exit(1 if bad else 0)
"""


def _child(script):
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-c", script], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr


def test_tuning_keys():
    """cot_set_tuning takes every key in {0-34, 36-54} with the values 0 and 1 and refuses -1, 35 and 55 as unknown -- in a child
    process, so that the knobs it turns reach no other test"""
    _child(_TUNING_KEYS_CHILD)


def header_tuning_enum():
    src = open(os.path.join(ROOT, "include", "cotnet_amd.h")).read()
    body = re.search(r"enum cot_tuning_key \{(.*?)\};", re.sub(r"/\*.*?\*/", "", src, flags=re.S), flags=re.S).group(1)
    return [(n, int(v)) for n, v in re.findall(r"\bCOT_TUNE_([A-Z0-9_]+)\s*=\s*(\d+)", body)]


def test_tuning_names_match_the_header():
    """every enumerator of enum cot_tuning_key is cot_tuning_name(value) in upper case behind the prefix; names and values are unique;
    35 and 55 are no keys (nothing is set here: no child process needed)"""
    L = _lib.lib()
    enum = header_tuning_enum()
    assert sorted(v for _, v in enum) == list(range(0, 35)) + list(range(36, 55))
    assert len({n for n, _ in enum}) == len(enum)
    for name, value in enum:
        assert L.cot_tuning_name(value) == name.lower().encode(), (name, value)
    assert L.cot_tuning_name(35) is None and L.cot_tuning_name(55) is None and L.cot_tuning_name(-1) is None
    assert _lib.tuning_keys(L) == dict(enum)
    assert _lib.TUNE.BN_FOLD == 12 and _lib.Tune(L).CONV_BIG_XSWZ == 48
    assert _lib.parse_tuning("12=1,bn_chan=0, MIX_LANES=128") == [(12, 1), (21, 0), (52, 128)]


_TUNING_RESET_CHILD = r"""
import sys
from cotnet_amd import _lib
L = _lib.lib()
KEYS = list(range(0, 35)) + list(range(36, 55))
fresh = {k: _lib.get_tuning(L, k) for k in KEYS}
bad = []
for k, want in ((12, 1), (13, 4096), (18, 256), (21, 1), (48, 7), (52, 256)):  # the globals' initialisers, by name in the assertion
    if fresh[k] != want:
        bad.append(("default", L.cot_tuning_name(k), fresh[k], want))


def idempotent(what):  # cot_set_tuning(k, cot_get_tuning(k)) changes nothing: what tuned()'s restore relies on
    for k in KEYS:
        v = _lib.get_tuning(L, k)
        assert L.cot_set_tuning(k, v) == 0
        if _lib.get_tuning(L, k) != v:
            bad.append(("set(get)", what, L.cot_tuning_name(k), v, _lib.get_tuning(L, k)))


idempotent("defaults")
for value in (0, 1, 5, 300, -2):
    for k in KEYS:
        assert L.cot_set_tuning(k, value) == 0
    idempotent(value)
for value in (0, 1, 7):
    for k in KEYS:
        assert L.cot_set_tuning(k, value) == 0
assert L.cot_reset_tuning() == 0
for k in KEYS:
    if _lib.get_tuning(L, k) != fresh[k]:
        bad.append(("reset", L.cot_tuning_name(k), _lib.get_tuning(L, k), fresh[k]))
print("BAD", bad)
sys.exit(1 if bad else 0)
"""


def test_tuning_reset_and_idempotence():
    """in a fresh process: keys 12, 13, 18, 21, 48, 52 read 1, 4096, 256, 1, 7, 256; cot_set_tuning(k, cot_get_tuning(k)) leaves every
    key as it is, for the defaults and after every key was set to 0, 1, 5, 300, -2; after every key was set to 0, 1 and 7,
    cot_reset_tuning puts each back to what the fresh process read"""
    _child(_TUNING_RESET_CHILD)


_TUNED_CHILD = r"""
from cotnet_amd import _lib
L = _lib.lib()
T = _lib.TUNE
get = lambda k: _lib.get_tuning(L, k)
cache = _lib.register_cache({})
assert (get(T.BN_FOLD), get(T.BN_CHAN), get(T.C1_WGRAD_WAVES)) == (1, 1, 2048)
cache["shape"] = 1
with _lib.tuned(L, BN_FOLD=0, C1_WGRAD_WAVES=-3):
    assert not cache, "emptied on entry"
    assert (get(T.BN_FOLD), get(T.C1_WGRAD_WAVES)) == (0, -3)
    with _lib.tuned(L, BN_FOLD=1, BN_CHAN=512):  # nests
        assert (get(T.BN_FOLD), get(T.BN_CHAN), get(T.C1_WGRAD_WAVES)) == (1, 512, -3)
    assert (get(T.BN_FOLD), get(T.BN_CHAN), get(T.C1_WGRAD_WAVES)) == (0, 1, -3)
    cache["shape"] = 2
assert not cache, "emptied on exit"
assert (get(T.BN_FOLD), get(T.C1_WGRAD_WAVES)) == (1, 2048)
try:
    with _lib.tuned(L, BN_SMALL_M=0, MIX_LANES=128):
        cache["shape"] = 3
        raise ZeroDivisionError
except ZeroDivisionError:
    pass
assert not cache and (get(T.BN_SMALL_M), get(T.MIX_LANES)) == (256, 256), "restored on an exception"
try:
    with _lib.tuned(L, BN_FOLD=0, NO_SUCH_KEY=1):
        raise SystemExit("entered with an unknown key")
except KeyError:
    pass
assert get(T.BN_FOLD) == 1
L.cot_set_tuning(T.BN_FOLD, 0)
cache["shape"] = 4
_lib.reset_tuning(L)
assert not cache and get(T.BN_FOLD) == 1
cache["shape"] = 5
L.cot_reset_tuning()  # (lib()'s handle: wrapped as cot_set_tuning is)
assert not cache
"""


def test_tuned_context_manager():
    """_lib.tuned nests, restores on an exception, and empties a register_cache dictionary on entry and on exit; so does reset_tuning"""
    _child(_TUNED_CHILD)


def test_product_has_no_cpu_fallback():
    """CPU tensors take the reference's route (copy to the GPU); without a GPU that must raise, not compute."""
    import torch
    from cotnet_amd.aggregation_zeropad import aggregation_zeropad
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises((RuntimeError, AssertionError)):
        aggregation_zeropad(torch.randn(1, 8, 4, 4), torch.randn(1, 1, 4, 9, 4, 4), 3, 1, 1, 1)


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "cotnet_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in text.replace("# oracle", ""), f"{f} mentions the oracle"
