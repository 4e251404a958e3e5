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


def test_tuning_keys():
    """cot_set_tuning takes every key in {0-34, 36-54} with the values 0 and 1 and refuses -1, 35 and 55 as unknown -- in a child
    process, so that the knobs it turns reach no other test"""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-c", _TUNING_KEYS_CHILD], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr


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
