"""Pre-GPU check of csrc/local_relation7.hip (LR-Net's 7x7 window): the SAME kernels compiled for the host (tests/emul), driven through the
C ABI with CPU pointers, against the fp64 checker of tests/lr_k7_cases.py.  tests/test_lrnet_k7_gpu.py runs the same functions on the MI355X."""
import ctypes
import random

import pytest
import torch

from cotnet_amd import _lib
from tests import lr_k7_cases as L7
from tests.emul import build_emul

try:
    E = _lib.bind(ctypes.CDLL(build_emul.build()))
except FileNotFoundError:  # no host compiler: the GPU tests still gate parity
    E = None

pytestmark = pytest.mark.skipif(E is None, reason="host emulation build unavailable")
DEV = "cpu"


@pytest.mark.parametrize("dtype", L7.DTYPES)
@pytest.mark.parametrize("case", L7.DIRECTED, ids=L7.case_id)
def test_directed_shapes_match_the_fp64_statement(case, dtype):
    """fails without the feature: all three entry points answer -2 at 7x7"""
    L7.directed(E, DEV, *case, dtype, seed=sum(case))


@pytest.mark.parametrize("dtype", L7.DTYPES)
def test_lds_boundary(dtype):
    L7.lds_boundary(E, DEV, dtype)


@pytest.mark.parametrize("dtype", L7.DTYPES)
@pytest.mark.parametrize("H,W", [(9, 30), (7, 7), (2, 150)])
def test_saturated_softmax(H, W, dtype):
    L7.saturated(E, DEV, H, W, dtype)


def test_other_windows_dtypes_and_paddings_are_refused():
    L7.refusals(E)


def test_misaligned_pointers_are_refused():
    L7.misaligned(E, DEV)


def test_three_by_three_is_untouched():
    """same kernels by name, same workspace size: [gL: N G 9 HW elements, 256-aligned][partials: G N tiles 72 floats]"""
    g = L7.geom(2, 16, 14, 14, k=3)
    assert E.cot_local_relation_workspace_bytes(ctypes.byref(g), _lib.COT_BF16) == ((2 * 2 * 9 * 196 * 2 + 255) & ~255) + 2 * 2 * 1 * 72 * 4
    q, k, v, gout, pos = L7.inputs(2, 16, 14, 14, torch.float32, 3, ks=3)
    out, probs = torch.empty_like(v), torch.empty(2, 1, 2, 9, 14, 14)
    P = L7.P
    assert E.cot_local_relation_forward(P(q), P(k), P(v), P(pos), P(out), P(probs), ctypes.byref(g), _lib.COT_F32, None) == 0
    assert E.cot_last_kernel().decode() == "lr_fwd"
    want = L7.reference64(q, k, v, pos, gout, ks=3)
    assert ((out.double() - want[0]).abs() <= 2e-5 * (1 + want[0].abs())).all()


def test_results_are_bit_identical_under_another_lane_schedule():
    q, k, v, gout, pos = L7.inputs(2, 24, 9, 30, torch.bfloat16, 5)
    a, pa = L7.run(E, q, k, v, gout, pos)
    E.emul_set_order(2)  # a different lane schedule: the fixed-order reductions and the barriers must not notice
    try:
        b, pb = L7.run(E, q, k, v, gout, pos)
    finally:
        E.emul_set_order(0)
    for x, y in zip(a + (pa,), b + (pb,)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("seed", [81, 82])
def test_random_shapes(seed):
    rng = random.Random(seed)
    failures, descs = [], []
    for _ in range(40):
        ok, desc = L7.fuzz_case(E, DEV, rng)
        descs.append(desc)
        if not ok:
            failures.append(desc)
    assert not failures, failures
    refused = [d for d in descs if d[0] == "refused"]
    assert len(refused) <= 0.15 * len(descs), (len(refused), len(descs))
    assert len(L7.FUZZ_WIDTHS) * 0.15 >= sum(1 for w in L7.FUZZ_WIDTHS if not L7.fits(1, w))  # the rule alone meets the cap
