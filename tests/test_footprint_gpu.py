"""tests/footprint_cases.py through libcotnet_hip.so on the MI355X: every kernel entry point on device operands inside filled margins, at
operand bases = 0 and = 16 (mod 256 bytes), against the same call on fresh allocations -- what the real buffer loads, LDS copies and
vector stores touch, and whether a result depends on where its operands lie (the product hands the kernels views into larger buffers:
fused_bn.new_guarded, the gradient buckets, the channel-major blocks' shared buffers).  An overrun lands in a margin the test owns and
is reported; nothing here is meant to fault."""
import pytest
import torch

from tests import footprint_cases as fc

pytestmark = pytest.mark.gpu
_CALLED = set()
_RAN = set()


class _DeviceLib:
    _test_device = "cuda"

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, name)


@pytest.fixture
def device_lib():
    from cotnet_amd import _lib
    L = _DeviceLib(_lib.lib())  # (raises when the HIP library is missing: no fallback)
    yield L
    torch.cuda.synchronize()


@pytest.mark.parametrize("base", [0, 16])
@pytest.mark.parametrize("family", sorted(fc.CASES))
def test_footprint_and_placement(family, base, device_lib):
    for case, args in fc.CASES[family]:
        try:
            fc.run_case(device_lib, case, args, base, _CALLED)  # (synchronises before the check)
        except AssertionError as e:
            raise AssertionError(f"{case.__name__}{args} base {base}: {e}") from e
    _RAN.add((family, base))


def test_every_entry_point_has_a_case_or_a_reason(device_lib):
    """(the cases above have run by now: pytest keeps the file's order; a family that has not -- a selection by -k -- runs here)"""
    for family in sorted(fc.CASES):
        if not any(f == family for f, _ in _RAN):
            for case, args in fc.CASES[family]:
                fc.run_case(device_lib, case, args, 0, _CALLED)
    assert all(reason for reason in fc.EXEMPT.values())
    assert fc.uncovered(_CALLED) == []
