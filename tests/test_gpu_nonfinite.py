"""What the GEMM kernels do with values that are not small finite numbers:
NaN and +-Inf operands, sums that overflow fp16, fp16 subnormal results and
operands.

The kernels' masking is software (lanes redirected past the operand, a k
mask on SDD's K tail, absent blocks of a grouped SDD tile, NaN written on a
hand-off time-out). Masking by multiplying with 0 in place of selecting
looks right until the masked value is NaN or Inf, so:

  * locality: NaN, +Inf and -Inf planted in one operand reach exactly the
    outputs IEEE arithmetic says (rounding_ref.expected_with_specials: only
    stored blocks contribute), with the NaN mask and the signs of the
    infinities exact and every other element bit-identical to the finite
    expectation; a NaN that is data is not a time-out, so
    sp.pair_errors() == 0. NaN payloads and signs are not compared. A NaN
    in rows of the dense operand that no stored block touches, or in rows
    of A / columns of B whose SDD output block is not stored, reaches
    nothing. The operands' NaN guard bands (tests/rounding_gpu.py) extend
    this to loads from outside an operand.
  * overflow: outputs that are exactly 65519, 65520, -65520 and 3 * 65536 in
    fp32 become 65504, +inf, -inf, +inf in fp16; the bf16 ties 257, 259, 385
    become 256, 260, 384; a finite product plus a finite C that overflows
    accumulates to inf.
  * fp16 subnormals: results n * 2^-24 below 2^-14 (exact), n / 8 * 2^-24
    (rounded at the fixed quantum) and above (rounded); operands that are
    themselves subnormal. The expectation is IEEE throughout.

bf16 subnormals lie in fp32's subnormal range, where the fp32 accumulation
itself is at stake; they are out of scope here.

Every case runs under select_dsd_kernel 0, 5 and 1 and inside guard bands,
as in tests/test_gpu_rounding.py.
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

B = R.B
SPOTS = ((3, 5), (40, 77), (100, 9))     # in-block (row, column)
NAN_ONLY = (np.nan,)


def _op(x, t):
    return x.T if t else x


def _op_level(operand, values, t):
    """(float64 op(operand), stored mask of op(operand) or None)."""
    if isinstance(operand, R.Sparse):
        return (_op(operand.dense(values), t).astype(np.float64),
                _op(operand.stored(), t))
    return _op(values, t).astype(np.float64), None


def _values(operand):
    return operand.values if isinstance(operand, R.Sparse) else operand


def _plant_sparse(s):
    """NaN / +Inf / -Inf in the first, middle and last stored block of every
    7th block-row (so the blocks a pair or split launch hands off and the
    ones it keeps are both hit)."""
    vals = s.values.copy()
    where = []
    for r in range(0, len(s.offsets) - 1, 7):
        a, b = int(s.offsets[r]), int(s.offsets[r + 1])
        if a == b:
            continue
        for e, (i, j) in zip((a, (a + b) // 2, b - 1), SPOTS):
            where.append((e * B + i) * B + j)
    assert len(where) >= 3
    R.plant(vals, where)
    return vals


def _plant_dense(d, t, spots, what=(np.nan, np.inf, -np.inf)):
    """`spots`: (row, column) of op(d)."""
    vals = d.copy()
    cols = vals.shape[1]
    R.plant(vals, [(c * cols + r) if t else (r * cols + c) for r, c in spots],
            what)
    return vals


def _variants(h):
    """(name, x values, y values, expects_nan) per planted variant."""
    c = h.case
    # (multiples of 8: the k a K-split case's thinned operand keeps)
    ks = (8, (c.k // 2 + 8) // 8 * 8, (c.k - 3) // 8 * 8)
    rows, cols = (7, 300, c.m - 1), (17, 200, c.n - 1)
    if h.C is not None:                   # rows / columns of stored blocks
        r_of = np.repeat(np.arange(len(h.C.offsets) - 1), np.diff(h.C.offsets))
        es = (0, h.C.nb // 2, h.C.nb - 1)
        rows = [int(r_of[e]) * B + i for e, (i, _) in zip(es, SPOTS)]
        cols = [int(h.C.indices[e]) * B + j for e, (_, j) in zip(es, SPOTS)]
    x_spots = list(zip(rows, ks))
    y_spots = list(zip(ks, cols))
    out = []
    if isinstance(h.X, R.Sparse):
        out.append(("x", _plant_sparse(h.X), None, True))
    else:
        out.append(("x", _plant_dense(h.X, c.ta, x_spots), None, True))
    if isinstance(h.Y, R.Sparse):
        out.append(("y", None, _plant_sparse(h.Y), True))
    else:
        out.append(("y", None, _plant_dense(h.Y, c.tb, y_spots), True))
    if not c.gap:
        return out
    gap = (2 * B + 5, 3 * B - 1)          # block index 2
    if c.op == "sdd":                     # C stores no block-row / -column 2
        out.append(("unstored", _plant_dense(h.X, c.ta, [(gap[0], 5),
                                                        (gap[1], c.k - 1)],
                                             NAN_ONLY),
                    _plant_dense(h.Y, c.tb, [(7, gap[0]), (c.k - 2, gap[1])],
                                 NAN_ONLY), False))
    elif isinstance(h.X, R.Sparse) and not isinstance(h.Y, R.Sparse):
        out.append(("untouched", None,
                    _plant_dense(h.Y, c.tb, [(gap[0], 17), (gap[1], c.n - 1)],
                                 NAN_ONLY), False))
    elif isinstance(h.Y, R.Sparse) and not isinstance(h.X, R.Sparse):
        out.append(("untouched", _plant_dense(h.X, c.ta, [(7, gap[0]),
                                                         (c.m - 1, gap[1])],
                                              NAN_ONLY), None, False))
    return out


def _same(got, want, what):
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), (
        f"{what}: NaN mask differs in {int((gn != wn).sum())} elements "
        f"(got {int(gn.sum())} NaN, expected {int(wn.sum())})")
    ok = ~wn
    g, w = got[ok], want[ok]
    if not torch.equal(g, w):
        bad = g != w
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} non-NaN elements "
                             f"differ, first got {g[i].item()} want "
                             f"{w[i].item()}")


def _plan_check(p):
    """The grouped and K-split cases take the path they are named after."""
    c = p.case
    if c.name == "nfgrouped":
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert cus == R.CUS, "case sized for another device"
        assert sp.sdd_plan(p.X.m, c.ta, p.Y.m, c.tb, p.C) == 1
    elif c.name == "nfksplit":
        assert sp.sdd_plan(p.X.m, c.ta, p.Y.m, c.tb, p.C) == 2


@pytest.mark.parametrize("case", R.NONFINITE_CASES, ids=lambda c: c.id)
def test_nonfinite_stays_local(case):
    h = R.host(case)
    dt = case.dtype
    for name, x, y, expects_nan in _variants(h):
        ox, mx = _op_level(h.X, _values(h.X) if x is None else x, case.ta)
        oy, my = _op_level(h.Y, _values(h.Y) if y is None else y, case.tb)
        want64 = R.expected_with_specials(ox, mx, oy, my, finite=h.P)
        want = G.expect(h.layout(R.round_once(want64, dt)), dt)
        what = f"{case.id} planted {name}"
        if expects_nan:
            assert bool(torch.isnan(want).any()) and bool(torch.isinf(want).any())
            assert not bool(torch.isnan(want).all())
        else:
            assert not bool(torch.isnan(want).any()), "the test's own plan"
        p = G.Problem(h, x=x, y=y)
        got = p.run_modes(_plan_check)
        for mode in G.MODES:
            _same(got[mode], want, f"{what} mode {mode}")
        assert sp.pair_errors() == 0, what


# ------------------------------------------------------------------ overflow --

# (first factors in X, [(second factors in Y, exact sum, rounded)])
CRAFTED = {
    "f16": ((255.0, 1.0), [((256.0, 239.0), 65519.0, 65504.0),
                           ((256.0, 240.0), 65520.0, np.inf),
                           ((-256.0, -240.0), -65520.0, -np.inf),
                           ((768.0, 768.0), 196608.0, np.inf)]),
    "bf16": ((1.0, 1.0), [((256.0, 1.0), 257.0, 256.0),
                          ((256.0, 3.0), 259.0, 260.0),
                          ((384.0, 1.0), 385.0, 384.0)]),
}


def _craft(h):
    """Copies of a NN case's operand values with one output row whose first
    len(targets) chosen columns are exactly the sums of CRAFTED: row i0 of
    op(X) is zero but for two k, where Y holds the second factors. Returns
    (x values, y values, [(output row, column, exact, rounded)])."""
    c = h.case
    assert not c.ta and not c.tb
    (xa, xb), targets = CRAFTED[c.dtype]
    x, y = _values(h.X).copy(), _values(h.Y).copy()
    if c.op == "dsd":                     # a stored block of block-row 0
        e = int(h.X.offsets[0])
        assert h.X.offsets[1] > e
        i0, k0, j0 = 7, int(h.X.indices[e]) * B + 11, 3
        x[h.X.offsets[0]:h.X.offsets[1], 7, :] = 0
        x[e, 7, 11], x[e, 7, 12] = xa, xb
        for t, ((ya, yb), _, _) in enumerate(targets):
            y[k0, j0 + t], y[k0 + 1, j0 + t] = ya, yb
    elif c.op == "dds":                   # the first stored block of Y
        rows = np.repeat(np.arange(len(h.Y.offsets) - 1), np.diff(h.Y.offsets))
        i0, k0, j0 = 9, int(rows[0]) * B + 11, int(h.Y.indices[0]) * B + 3
        x[i0, :] = 0
        x[i0, k0], x[i0, k0 + 1] = xa, xb
        for t, ((ya, yb), _, _) in enumerate(targets):
            y[0, 11, 3 + t], y[0, 12, 3 + t] = ya, yb
    else:                                 # sdd: the first stored block of C
        rows = np.repeat(np.arange(len(h.C.offsets) - 1), np.diff(h.C.offsets))
        i0, k0 = int(rows[0]) * B + 7, 11
        j0 = int(h.C.indices[0]) * B + 3
        x[i0, :] = 0
        x[i0, k0], x[i0, k0 + 1] = xa, xb
        for t, ((ya, yb), _, _) in enumerate(targets):
            y[k0, j0 + t], y[k0 + 1, j0 + t] = ya, yb
    return x, y, [(i0, j0 + t, s, r) for t, (_, s, r) in enumerate(targets)]


NN_SMALL = [c for c in R.NONFINITE_CASES
            if c.name == "nf" and not c.ta and not c.tb
            and c.op in ("dsd", "dds", "sdd")]


@pytest.mark.parametrize("case", NN_SMALL, ids=lambda c: c.id)
def test_overflow_and_ties_at_chosen_outputs(case):
    """fp16: 65519 -> 65504, 65520 -> inf, -65520 -> -inf, 3 * 65536 -> inf;
    bf16: the ties 257 -> 256, 259 -> 260, 385 -> 384. Whole output exact."""
    h = R.host(case)
    x, y, targets = _craft(h)
    ox, _ = _op_level(h.X, x, False)
    oy, _ = _op_level(h.Y, y, False)
    full = ox @ oy
    assert float((np.abs(ox) @ np.abs(oy)).max()) < 2.0 ** 24   # fp32 exact
    rounded = R.round_once(full, case.dtype)
    for i, j, exact, want in targets:
        assert full[i, j] == exact and rounded[i, j] == want, (i, j, full[i, j])
    want = G.expect(h.layout(rounded), case.dtype)
    p = G.Problem(h, x=x, y=y)
    got = p.run_modes()
    for mode in G.MODES:
        G.assert_exact(got[mode], want, f"{case.id} crafted mode {mode}")
    assert sp.pair_errors() == 0


def test_accumulate_overflows_to_inf():
    """A finite product plus a finite C whose sum passes 65520 is +-inf."""
    case = R.ACCUMULATE_CASES[0]
    assert case.dtype == "f16" and case.acc == "operand"
    h = R.host(case)
    c_in = h.c_in.astype(np.float64).copy()
    up = np.argwhere(h.P >= 16)[:40:2]
    down = np.argwhere(h.P <= -16)[:40:2]
    assert len(up) and len(down)
    c_in[tuple(up.T)] = R.F16_MAX
    c_in[tuple(down.T)] = -R.F16_MAX
    rounded = R.round_once(h.P + c_in, "f16")
    assert (rounded[tuple(up.T)] == np.inf).all()
    assert (rounded[tuple(down.T)] == -np.inf).all()
    p = G.Problem(h)
    for s in (p.X, p.Y):
        if hasattr(s, "offsets"):
            sp.Transpose(s.m)
    p.out.t.copy_(torch.from_numpy(c_in).to(torch.float16))
    sp.MatmulAccumulateEx(p.X.m, case.ta, p.Y.m, case.tb, p.C)
    torch.cuda.synchronize()
    G.K._equal(p.out.t, G.expect(rounded, "f16"), "accumulate overflow")
    assert p.out.intact()


# ---------------------------------------------------------------- subnormals --

F16_NN = [c for c in NN_SMALL if c.dtype == "f16"]


def _bands(h):
    """Integer operand values of a NN case with the second operand thinned
    in the output columns j % 128 < 32 (k % 128 >= 16 zeroed: sums an eighth
    as large), and the mask of the first operand's rows i % 128 < 64."""
    x, y = _values(h.X).copy(), _values(h.Y).copy()
    kk = (np.arange(y.shape[-2]) % B >= 16)[:, None]
    jj = (np.arange(y.shape[-1]) % B < 32)[None, :]
    y[..., kk & jj] = 0
    band = (np.arange(x.shape[-2]) % B < 64)[:, None] & np.ones(
        (1, x.shape[-1]), bool)
    return x, y, band


def _run_scaled(h, x, y):
    ox, _ = _op_level(h.X, x, False)
    oy, _ = _op_level(h.Y, y, False)
    full = ox @ oy                         # exact: integers * 2^-s
    rounded = R.round_once(full, "f16")
    want = G.expect(h.layout(rounded), "f16")
    p = G.Problem(h, x=x, y=y)
    got = p.run_modes()
    return p, got, want, h.layout(full)


@pytest.mark.parametrize("case", F16_NN, ids=lambda c: c.id)
def test_f16_subnormal_results(case):
    """Operands int * 2^-10 (rows i % 128 < 64: 2^-13) and int * 2^-14, all
    normal fp16 values; results n * 2^-24 and n / 8 * 2^-24: exact fp16
    subnormals (n < 1024), subnormals rounded at the fixed quantum 2^-24,
    and rounded normals (n >= 2048) all occur, and all are IEEE."""
    h = R.host(case)
    x, y, band = _bands(h)
    xs = np.where(band, R.scaled(x, -13), R.scaled(x, -10))
    ys = R.scaled(y, -14)
    for v in (xs, ys):                     # operands: zero or normal
        assert (np.abs(v[v != 0]) >= 2.0 ** -14).all()
    p, got, want, full = _run_scaled(h, xs, ys)
    n = np.abs(full) * 2.0 ** 24
    sub = (n > 0) & (n < 1024)
    assert (sub & (n == np.floor(n))).sum() > 1000          # exact subnormals
    assert (sub & (n != np.floor(n))).sum() > 1000          # rounded ones
    assert ((n >= 2048) & (n % 2 == 1)).sum() > 1000        # rounded normals
    for mode in G.MODES:
        G.assert_exact(got[mode], want, f"{case.id} subnormal results mode {mode}")


@pytest.mark.parametrize("case", F16_NN, ids=lambda c: c.id)
def test_f16_subnormal_inputs(case):
    """First operand int * 2^-24 (fp16 subnormals), second int * 2^4: the
    matrix unit must take subnormal operands at their value. On a mismatch
    torch.matmul on the same densified operands is the witness named in the
    message: equal values in both kernels and the witness would be the
    matrix unit's behaviour, any other difference is a kernel bug."""
    h = R.host(case)
    x, y = _values(h.X), _values(h.Y)
    xs, ys = R.scaled(x, -24), R.scaled(y, 4)
    assert (np.abs(xs[xs != 0]) < 2.0 ** -14).all()
    p, got, want, _ = _run_scaled(h, xs, ys)
    for mode in G.MODES:
        try:
            G.assert_exact(got[mode], want, f"{case.id} subnormal inputs mode {mode}")
        except AssertionError as err:
            ox, _ = _op_level(h.X, xs, False)
            oy, _ = _op_level(h.Y, ys, False)
            w = torch.matmul(torch.from_numpy(ox).half().cuda(),
                             torch.from_numpy(oy).half().cuda())
            w = G.expect(h.layout(w.float().cpu().numpy()), "f16")
            raise AssertionError(
                f"{err}; modes agree: "
                f"{all(torch.equal(got[m], got[0]) for m in G.MODES)}; "
                f"torch.matmul equals this mode: {torch.equal(w, got[mode])}, "
                f"equals IEEE: {torch.equal(w, want)}") from None
