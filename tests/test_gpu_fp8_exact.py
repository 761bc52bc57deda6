"""GPU: the fp8 products (sputnik/block/fp8.h) bit for bit, through the C ABI,
against the correctly rounded emulation of tests/fp8_ref.py. Every comparison
here is on bits; there is no tolerance.

  arithmetic  fp8_ref.exact_case: bytes whose products and partial sums are
              exact in fp32 in any order (so the matrix cores' summation
              order cannot show), steps that cancel in pairs so that the
              roundings of s = sa * sb and of acc = fma(s, P, acc) reach the
              leading bits of C. SDD with 1, 3 and 5 steps (3: the first
              refill of a ring stage; 5: odd, stage 0 refilled twice), DSD
              with 4 x 5 x 2 blocks and rows of 5, 0, 1 and 3 stored blocks
              in storage order, and fp8_ref.tie_case, where every output is a
              tie of round_T. tests/test_fp8_host.py shows on the CPU that a
              separate multiply and add, (sa P) sb, an unrounded scale
              product, ascending order, an accumulator rounded to T and
              ties-away each change most of these outputs.
  decode      every finite e4m3 byte, from every byte position of both
              16-byte reads of a lane, times 1.0 and two powers of two.
  non-finite  a NaN byte in either operand, an Inf and a NaN scale, 0 * Inf,
              and accumulators on both sides of fp16's tie to Inf: the NaN
              mask is the emulation's, everything else is bit-equal.
  skipped     a stored block whose index is out of range: DSD as if the block
              were not stored, SDD with that tile left unwritten.
"""

import functools

import numpy as np
import pytest
import torch

import sputnik_amd as sp
from tests import fp8_ref as R
from tests import helpers as H
from tests import rounding_ref as RR

pytestmark = pytest.mark.gpu

DTYPES = ["f16", "bf16"]
PATTERN = 0x5555           # the 16-bit fill of an output before the call
PAD_BYTE = 0x3A            # e4m3 1.25; four of them are the fp32 7.1e-4
# Bytes around every buffer of a padded call: a block row of the largest A
# (128 x 640), which is also more than a block row of scales (128 x 5 fp32)
# and than a k-block of every W row; a multiple of 4096, so the buffers keep
# the alignment of a fresh allocation.
PAD = 128 * 640
assert PAD % 4096 == 0


def host(t) -> np.ndarray:
    return t.float().cpu().numpy()


def place(a: np.ndarray, dtype, pad: bool):
    """`a` on the device as `dtype`; with `pad`, in the middle of a larger
    allocation of PAD_BYTE bytes (finite and non-zero as e4m3 and as fp32)."""
    a = np.ascontiguousarray(a)
    raw = a.view(np.uint8).reshape(-1)
    if pad:
        whole = np.full(PAD + raw.size + PAD, PAD_BYTE, np.uint8)
        whole[PAD:PAD + raw.size] = raw
        t = torch.from_numpy(whole).cuda()[PAD:PAD + raw.size]
    else:
        t = torch.from_numpy(raw.copy()).cuda()
    return t.view(dtype).view(*a.shape)


def fresh(shape, dtype):
    """A moated output filled with PATTERN: (view, whole, pad)."""
    fill = torch.tensor([PATTERN], dtype=torch.int16).view(
        H.torch_dtype(dtype)).item()
    return RR.moated(shape, H.torch_dtype(dtype), fill, row=shape[-1])


def out_shape(ops):
    if ops.kind == "sdd":
        return (len(ops.topology[1]), 128, 128)
    return (ops.m, ops.n)


def call(ops, dtype, out, pad=False, indices=None, row_indices=None):
    """The product of `ops` into `out`; `indices` / `row_indices` replace
    the topology's (the out-of-range tests)."""
    offsets, idx = ops.topology
    idx = idx if indices is None else indices
    nb = len(idx)
    d_off = place(offsets, torch.int32, pad)
    d_idx = place(np.asarray(idx, np.int16), torch.int16, pad)
    wq = place(ops.wq, torch.float8_e4m3fn, pad)
    sw = place(ops.sw, torch.float32, pad)
    if ops.kind == "sdd":
        rows = R.row_indices(offsets) if row_indices is None else row_indices
        c = sp.BlockMatrix(ops.m, ops.n, 128, nb * 128 * 128, out, d_off,
                           d_idx)
        c.row_indices = place(np.asarray(rows, np.int16), torch.int16, pad)
        sp.SddFp8(place(ops.aq, torch.float8_e4m3fn, pad),
                  place(ops.sa, torch.float32, pad), wq, sw, c)
    else:
        sq, ss = ops.sparse()
        s = sp.BlockMatrix(ops.m, ops.k, 128, nb * 128 * 128,
                           place(sq, torch.float8_e4m3fn, pad), d_off, d_idx)
        sp.DsdFp8(s, place(ss, torch.float32, pad), wq, sw,
                  sp.Matrix(ops.m, ops.n, out))
    torch.cuda.synchronize()


def run_twice(ops, dtype, **kw) -> np.ndarray:
    """The output's bits, uint16 in C's layout, after two runs into fresh
    moated outputs that must agree bit for bit and leave the moats intact."""
    runs = []
    for _ in range(2):
        out, whole, pad = fresh(out_shape(ops), dtype)
        call(ops, dtype, out, **kw)
        assert RR.moat_intact(whole, pad, PATTERN)
        runs.append(out.view(torch.int16).cpu().numpy().view(np.uint16))
    assert np.array_equal(runs[0], runs[1]), "two runs differ"
    return runs[0]


def as_values(bits: np.ndarray, dtype) -> np.ndarray:
    t = torch.from_numpy(bits.view(np.int16).copy()).view(H.torch_dtype(dtype))
    return t.float().numpy()


def explain(ops, dtype, got_bits, want, order=None) -> str:
    """The first differing element with its steps: P, the scales, the
    emulated accumulator after each, and the two results."""
    want_bits = RR.bits(want, dtype)
    with np.errstate(invalid="ignore"):
        diff = (got_bits != want_bits) & ~(np.isnan(want)
                                           & np.isnan(as_values(got_bits, dtype)))
    if not diff.any():
        return "no difference"
    at = tuple(int(v) for v in np.argwhere(diff)[0])
    if ops.kind == "sdd":
        offsets, indices = ops.topology
        rb, nb = int(R.row_indices(offsets)[at[0]]), int(indices[at[0]])
        row, col = rb * 128 + at[1], nb * 128 + at[2]
    else:
        row, col = at
    order = order or ops.order
    steps = (order[row // 128] if order else range(ops.k // 128))
    lines = [f"{int(diff.sum())} of {diff.size} differ; first at {at} = C["
             f"{row}, {col}]: gpu {as_values(got_bits, dtype)[at]!r} "
             f"(0x{int(got_bits[at]):04x}), expected {want[at]!r} "
             f"(0x{int(want_bits[at]):04x})"]
    acc = np.zeros((1, 1), np.float32)
    for kb in steps:
        ks = slice(kb * 128, (kb + 1) * 128)
        p, _ = R.interval_sum(ops.aq[row:row + 1, ks], ops.wq[col:col + 1, ks])
        sa, sw = ops.sa[row, kb], ops.sw[kb, col // 128]
        with np.errstate(invalid="ignore", over="ignore"):
            acc = R.fma32(sa * sw, p, acc)
        lines.append(f"  kb {kb}: P {float(p[0, 0])!r} sa {float(sa)!r} sb "
                     f"{float(sw)!r} s {float(sa * sw)!r} -> acc "
                     f"{float(acc[0, 0])!r}")
    return "\n".join(lines)


def assert_bits(ops, dtype, got_bits, want, order=None):
    """Bit equality wherever the expected value is not a NaN, and the same
    NaN mask."""
    got = as_values(got_bits, dtype)
    nan = np.isnan(want)
    same = np.array_equal(np.isnan(got), nan) and np.array_equal(
        got_bits[~nan], RR.bits(want, dtype)[~nan])
    assert same, explain(ops, dtype, got_bits, want, order)


# ---- A: the arithmetic ----------------------------------------------------------

EXACT = ([("sdd", k) for k in R.SDD_DEEP_K] + [("dsd", R.DSD_DEEP_K)])


@functools.lru_cache(maxsize=None)
def exact(kind, k):
    return R.exact_case(kind, k)


@pytest.mark.parametrize("kind,k", EXACT,
                         ids=[f"{kind}-k{k}" for kind, k in EXACT])
@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_arithmetic(dtype, kind, k):
    ops = exact(kind, k)
    want = ops.expected(dtype)
    assert np.isfinite(want).all()
    got = run_twice(ops, dtype)
    assert_bits(ops, dtype, got, want)
    if kind == "dsd":
        assert not got[128:256].any()       # the empty block row: +0


@pytest.mark.parametrize("dtype", DTYPES)
def test_ties_of_the_final_rounding_go_to_even(dtype):
    ops = R.tie_case(dtype)
    want = ops.expected(dtype)
    away = ops.expected(dtype, model="round_half_up")
    assert (RR.bits(want, dtype) != RR.bits(away, dtype)).all()
    assert_bits(ops, dtype, run_twice(ops, dtype), want)


# ---- B: every byte through the decode -------------------------------------------

@pytest.mark.parametrize("patterned", ["a", "w"])
@pytest.mark.parametrize("kind", ["sdd", "dsd"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_byte_through_the_decode(dtype, kind, patterned):
    ops = R.byte_case(kind, patterned)
    want = RR.round_once(R.byte_case_expected(ops), dtype)
    if kind == "sdd":
        want = R.blocks_from_dense(want, *ops.topology)
    zero = want == 0
    assert zero.any() and not np.signbit(want[zero]).any()
    got = run_twice(ops, dtype)
    assert_bits(ops, dtype, got, want)
    assert not got[zero].any()              # -0 bytes give +0 sums


# ---- C: non-finite values and overflow ------------------------------------------

SPECIALS = ["nan_a", "nan_w", "inf_sa", "nan_sw", "overflow"]


@pytest.mark.parametrize("what", SPECIALS)
@pytest.mark.parametrize("kind", ["sdd", "dsd"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_nonfinite_and_overflow(dtype, kind, what):
    """The expected values are the emulation's, whose interval sums are
    computed with the NaN bytes taken out and their rows and columns set
    afterwards (fp8_ref.interval_sum), never by a NaN through BLAS; a DSD's
    planted weight byte reaches only the block rows that store its k-block
    (tests/test_fp8_host.py asserts where each planted item reaches)."""
    ops, (row, kb) = R.special_case(kind, what)
    dense = R.round_t(ops.acc(), dtype)
    want = (R.blocks_from_dense(dense, *ops.topology) if kind == "sdd"
            else dense)
    got_bits = run_twice(ops, dtype)
    assert_bits(ops, dtype, got_bits, want)
    got = as_values(got_bits, dtype)
    if kind == "sdd":
        got = R.dense_from_blocks(ops.m, ops.n, *ops.topology, got)
    if what in ("nan_a", "nan_sw", "nan_w"):
        assert np.isnan(got).any() and not np.isinf(got).any()
    if what == "inf_sa":
        assert np.isnan(got[row, 3::4]).all()
        assert (got[row] == np.inf).any() and (got[row] == -np.inf).any()
        assert np.isfinite(np.delete(got, row, axis=0)).all()
    if what == "overflow":
        pos, neg = got[row:row + 3, 10], got[row:row + 3, 11]
        if dtype == "f16":      # past the tie, the tie itself, just below
            assert list(pos) == [np.inf, np.inf, 65504.0]
            assert list(neg) == [-np.inf, -np.inf, -65504.0]
        else:
            assert np.isfinite(got[row:row + 3]).all()
            assert list(pos) == [65536.0] * 3 and list(neg) == [-65536.0] * 3


# ---- D: stored blocks that are out of range -------------------------------------

@pytest.mark.parametrize("bad", ["past-the-end", "minus-one"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_dsd_skips_a_stored_block_whose_column_is_out_of_range(dtype, bad):
    """One stored index of the deep DSD is k_blocks, or -1: the result is the
    emulation's with that block removed. Every operand, scale and index
    buffer lies inside a larger allocation of finite, non-zero bytes (PAD on
    both sides: a block row of the operand, of its scales and a k-block of
    each weight row), so a kernel without the range check would read defined
    memory and give a wrong value, never a stray access."""
    ops = exact("dsd", R.DSD_DEEP_K)
    offsets, indices = ops.topology
    at = 1                                  # block row 0, the second of a pair
    planted = indices.copy()
    planted[at] = ops.k // 128 if bad == "past-the-end" else -1
    order = [list(o) for o in ops.order]
    assert order[0].pop(at) == int(indices[at])
    want = ops.expected(dtype, order=order)
    assert not np.array_equal(want[:128], ops.expected(dtype)[:128])
    got = run_twice(ops, dtype, pad=True, indices=planted)
    assert_bits(ops, dtype, got, want, order)


@pytest.mark.parametrize("bad", ["row-past-the-end", "column-minus-one"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_sdd_leaves_a_tile_whose_index_is_out_of_range_unwritten(dtype, bad):
    """One row_indices entry is m_blocks, or one column index is -1: that
    tile keeps the fill pattern and every other tile is exact. The buffers
    are padded as in the DSD test, for the same reason: a missing check
    would read a block row of A and of its scales past the end, or a block
    row of W in front of it, all inside the allocation."""
    ops = exact("sdd", R.SDD_DEEP_K[-1])
    offsets, indices = ops.topology
    tile = 3
    rows, cols = R.row_indices(offsets).copy(), indices.copy()
    if bad == "row-past-the-end":
        rows[tile] = ops.m // 128
    else:
        cols[tile] = -1
    want = ops.expected(dtype)
    got = run_twice(ops, dtype, pad=True, indices=cols, row_indices=rows)
    assert (got[tile] == PATTERN).all()
    keep = np.arange(len(indices)) != tile
    assert np.array_equal(got[keep], RR.bits(want, dtype)[keep]), explain(
        ops, dtype, np.where(keep[:, None, None], got, RR.bits(want, dtype)),
        want)
