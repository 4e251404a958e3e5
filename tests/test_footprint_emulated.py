"""tests/footprint_cases.py through the host-emulated library: every kernel entry point on operands inside filled margins, at two
alignments, against the same call on plain operands (what is written, what is read and used, what the result depends on) -- plus the
self-test of the checker on stand-in "kernels" written in torch, each wrong in one way."""
import pytest
import torch

from tests import footprint_cases as fc
from tests import test_kernels_emulated as tke

_emulated = pytest.mark.skipif(tke._EMUL is None, reason="host emulation build unavailable")
_CALLED = set()
_RAN = set()


@pytest.fixture
def _library_defaults():
    """the cases run on the library's defaults and set what they vary with _lib.tuned"""
    yield
    fc._lib.reset_tuning(tke._EMUL)


@_emulated
@pytest.mark.parametrize("base", [0, 16])
@pytest.mark.parametrize("family", sorted(fc.CASES))
def test_footprint_and_placement(family, base, _library_defaults):
    for case, args in fc.CASES[family]:
        try:
            fc.run_case(tke._EMUL, case, args, base, _CALLED)
        except AssertionError as e:
            raise AssertionError(f"{case.__name__}{args} base {base}: {e}") from e
    _RAN.add((family, base))


@_emulated
def test_every_entry_point_has_a_case_or_a_reason():
    """(the cases above have run by now: pytest keeps the file's order; a family that has not -- a selection by -k -- runs here)"""
    for family in sorted(fc.CASES):
        if not any(f == family for f, _ in _RAN):
            for case, args in fc.CASES[family]:
                fc.run_case(tke._EMUL, case, args, 0, _CALLED)
    assert all(reason for reason in fc.EXEMPT.values())
    assert not set(fc.EXEMPT) - set(fc._lib.SYMBOLS), "EXEMPT names something the header does not declare"
    assert fc.uncovered(_CALLED, exported=tke._EMUL) == []


# ---- the checker itself, on CPU tensors and torch "kernels": no library code runs here

def _past(body, k):
    """the flat view of `body` shifted by k elements (reaches k elements outside it); where the allocation has no room for that -- the
    plain operands -- a copy, so that the stand-in misbehaves on margined operands only"""
    off = body.storage_offset() + k
    if off < 0 or (off + body.numel()) * body.element_size() > body.untyped_storage().nbytes():
        return body.reshape(-1).clone()
    return torch.as_strided(body, (body.numel(),), (1,), off)


def _double(x, y, ws):
    ws.view(torch.float32)[:] = 1.0
    y.copy_(2 * x.float())


def _writes_past_the_end(x, y, ws):
    _double(x, y, ws)
    _past(y, 1)[-1] = 7.0


def _writes_before_the_start(x, y, ws):
    _double(x, y, ws)
    _past(y, -1)[0] = 7.0


def _leaves_one_unwritten(x, y, ws):
    ws.view(torch.float32)[:] = 1.0
    y.view(-1)[:-1] = 2 * x.view(-1)[:-1].float()


def _uses_a_margin_value(x, y, ws):
    _double(x, y, ws)
    y.view(-1)[-1] += _past(x, 1)[-1].float()  # (the element behind x enters a sum)


def _modifies_its_input(x, y, ws):
    _double(x, y, ws)
    x.view(-1)[3] = 0.0


def _overruns_its_workspace(x, y, ws):
    _double(x, y, ws)
    w = ws.view(torch.float32)
    _past(w, 1)[-1] = 1.0


def _stand_in_case(kernel):
    def case(L, A):
        x = A.i(torch.arange(1, 31, dtype=torch.float32).view(2, 3, 5).bfloat16())
        y, ws = A.o((2, 3, 5), torch.float32), A.w(64)
        kernel(x, y, ws)
    return case


@pytest.mark.parametrize("base", [0, 16])
def test_checker_accepts_a_correct_kernel(base):
    fc.run_case(None, _stand_in_case(_double), (), base)


@pytest.mark.parametrize("base", [0, 16])
@pytest.mark.parametrize("kernel,message", [
    (_writes_past_the_end, "margin behind the operand was written"), (_writes_before_the_start, "margin before the operand was written"),
    (_leaves_one_unwritten, "is NaN"), (_uses_a_margin_value, "is NaN"), (_modifies_its_input, "an input was modified"),
    (_overruns_its_workspace, "margin behind the operand was written")])
def test_checker_catches(kernel, message, base):
    with pytest.raises(AssertionError, match=message):
        fc.run_case(None, _stand_in_case(kernel), (), base)


def test_checker_catches_a_result_that_depends_on_the_placement():
    def case(L, A):
        x, y = A.i(torch.ones(8)), A.o(8, torch.float32)
        y.copy_(x + (x.data_ptr() % 32) / 16)
    fc.run_case(None, case, (), 0)
    with pytest.raises(AssertionError, match="differs from the same call on plain operands"):
        fc.run_case(None, case, (), 16)


def test_checker_catches_an_unwritten_byte_of_a_mask():
    """one-byte outputs may hold the fill's value legitimately: the plain run's other fill shows a byte neither run wrote"""
    def case(L, A):
        m = A.o(16, torch.uint8)
        m[:15] = 0xA5
    with pytest.raises(AssertionError, match="differs from the same call on plain operands"):
        fc.run_case(None, case, (), 0)


def test_margins_and_alignment():
    A = fc.Arena("cpu", 16)
    t = A.i(torch.zeros(2, 4, 7, 7).bfloat16())
    blk = A.i(torch.zeros(8, dtype=torch.int32), align=4)
    acc = A.io(torch.zeros(4, dtype=torch.int64), align=8)
    assert t.data_ptr() % 256 == 16 and blk.data_ptr() % 16 == 4 and acc.data_ptr() % 16 == 8
    op = A.ops[0]
    need = (fc.MARGIN_PLANES * 49 + 7 + 1) * 2
    assert op.off >= need and op.raw.numel() - op.off - op.nbytes >= need
    assert A.ops[1].off >= fc.MIN_MARGIN * 4
    assert fc.Arena("cpu", 0).i(torch.zeros(5)).data_ptr() % 256 == 0
