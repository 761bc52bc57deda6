"""The GEMM kernels' last step, the fp32 -> fp16 / bf16 conversion, pinned
bit for bit on every dispatch path.

tests/test_gpu_kat.py's operands in {-1, 0, 1} give representable results,
so the conversion is an identity there, and the tolerance tests allow more
than a truncation costs. Here the operands of tests/rounding_ref.py keep the
fp32 accumulation exact in any order while most results are NOT
representable, so exactly one output is right: round_once(float64 product),
nearest with ties to even, rounded once. A kernel that truncates, rounds
ties away, rounds a partial sum to the operand type on its way through a
hand-off (pair, split, K-split: README's "fp32 hand-off"), or rounds the
product before adding C (accumulate.h's "rounded once") differs in at least
5 % of the outputs of every case; tests/test_rounding_host.py proves that
for each case below, on the host.

Every case runs under select_dsd_kernel 0 (8-wave template, the compiler's
conversion), 5 (4-wave kernel, its hand-placed conversion) and 1 (default
dispatch); each must equal the expectation, hence each other, with
sp.pair_errors() == 0. Where the expected value is 0 (empty block-rows,
all-zero blocks, operands holding -0) the output's sign bit is clear. All
value buffers lie inside guard bands (tests/rounding_gpu.py).
"""

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected here, skipped: no device
    pytest.skip("no GPU", allow_module_level=True)

import sputnik_amd as sp  # noqa: E402
from tests import rounding_gpu as G  # noqa: E402
from tests import rounding_ref as R  # noqa: E402

sp.lib()  # fail loudly if the native library is missing


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _plan_check(p):
    """The path the case is named after, asserted under the default
    dispatch as the KAT of that path asserts it."""
    c = p.case
    a, b = p.X.m, p.Y.m
    if c.name == "tallpipe":
        assert sp.dsd_plan(a, c.ta, b, c.tb, p.C) == 4
    elif c.name == "grouped":
        assert _cus() == R.CUS, "case sized for another device"
        assert sp.sdd_plan(a, c.ta, b, c.tb, p.C) == 1, "grouped SDD tiles"
    elif c.name == "tailsplit":
        assert _cus() == R.CUS, "case sized for another device"
        assert sp.sdd_kernel(a, c.ta, b, c.tb, p.C) == 3
    elif c.name == "bt":
        assert sp.sdd_kernel(a, c.ta, b, c.tb, p.C) == 4
    elif c.name.startswith("ksplit"):
        assert sp.sdd_plan(a, c.ta, b, c.tb, p.C) == 2, "K-split SDD"


def _check_modes(p, got, want, what):
    for mode in G.MODES:
        G.assert_exact(got[mode], want, f"{what} mode {mode}")
    for mode in G.MODES[1:]:
        assert torch.equal(got[mode].view(torch.int16),
                           got[G.MODES[0]].view(torch.int16)), \
            f"{what}: mode {mode} and mode {G.MODES[0]} differ in bits"
    assert sp.pair_errors() == 0


@pytest.mark.parametrize("case", R.ROUNDING_CASES, ids=lambda c: c.id)
def test_rounded_once(case):
    h = R.host(case)
    p = G.Problem(h)
    want = G.expect(h.expected(), case.dtype)
    ex = case.name == "tall"            # MatmulEx, precomputed metadata
    if ex:
        sp.Transpose(p.X.m)
    if case.name == "pairs":
        for pairs in (1, 0):
            with G.knobs({"pairs": pairs}):
                got = p.run_modes(_plan_check, ex)
            _check_modes(p, got, want, f"{case.id} pairs={pairs}")
        return
    got = p.run_modes(_plan_check, ex)
    _check_modes(p, got, want, case.id)


@pytest.mark.parametrize("case", R.ACCUMULATE_CASES,
                         ids=lambda c: c.id + "-" + c.acc)
def test_accumulate_rounded_once(case):
    """C += op(A) op(B) with C_in a representable value of the product's
    magnitude: round_once(P + C_in), not round(round(P) + C_in); into an
    fp32 C the same values are exact (which guards the builder). Where the
    sparse operand stores nothing C keeps C_in."""
    h = R.host(case)
    p = G.Problem(h)
    for s in (p.X, p.Y):
        if hasattr(s, "offsets"):
            sp.Transpose(s.m)
    p.out.t.copy_(torch.from_numpy(h.c_in).to(p.out.t.dtype))
    sp.MatmulAccumulateEx(p.X.m, case.ta, p.Y.m, case.tb, p.C)
    torch.cuda.synchronize()
    want = torch.from_numpy(np.ascontiguousarray(h.expected())).to(
        p.out.t.dtype).cuda()
    G.K._equal(p.out.t, want, f"{case.id} C {case.acc}")
    assert p.out.intact(), "wrote outside C"
    assert sp.pair_errors() == 0
