"""Numpy reference of the fp8 gradient pieces (sputnik/block/fp8.h,
"Gradients"), built on tests/fp8_ref.py and shared by
tests/test_fp8_grad_host.py and tests/test_gpu_fp8_grad*.py. Nothing here
calls the library.

    quantize_cols            the column outputs of QuantizeTiles: bytes
                             [cols, rows] and scales [rows / 128, cols], one
                             per 128 x 1 tile, from the definition
    transposed_order         offsets_t / indices_t / block_offsets of a BCSR
                             topology, by counting (stable within a column)
    quantize_blocks_t        the column outputs of QuantizeBlocks
    interval_sums            P [k / 128, m, n] of fp8_ref.interval_sum
    chain                    acc = fma32(float32(sa[row] * sb[kb, col]), P,
                             acc) per stored interval, in storage order, and
                             the wrong models of it (MODELS)
    finish                   round_out(acc), or round_out(acc + C_old)
    bound                    the header's acceptance bound
    Case / exact_case / random_case / tie_case
                             the inputs of tests/test_gpu_fp8_grad_wgrad.py

Bound: |C - exact| <= 2^-p |exact| + (K + 2 K / 128 + 1) 2^-23 sum |terms|,
the form of fp8_ref.bound plus the fp32 add of C_old; without the first
summand for fp32 output. With `add`, C_old is one of the terms.
"""

from __future__ import annotations

import numpy as np

from tests import fp8_ref as R
from tests.moe_ref import P_BITS

B = R.B

# The sparse source of the tests: 6 x 4 blocks. Column 0 holds five blocks,
# column 1 none, and block row 0 is stored out of order, so block_offsets is
# not the identity.
SRC_ROWS, SRC_COLS = 6 * B, 4 * B
SRC_TOPOLOGY = (np.array([0, 2, 4, 5, 6, 7, 8], np.int32),
                np.array([3, 0, 0, 2, 0, 0, 2, 0], np.int16))
WGRAD_N = 256


# ---- quantisers -----------------------------------------------------------------

def quantize_cols(x, pow2: bool = False):
    """x [rows, cols] -> (qt uint8 [cols, rows], scales_t float32 [rows /
    128, cols]): the tile of scales_t[rb, c] is x[128 rb : 128 rb + 128, c]."""
    x = np.asarray(x, dtype=np.float32)
    rows, cols = x.shape
    t = x.reshape(rows // B, B, cols)
    s = R.scale(R.amax_finite(t, axis=1), pow2)
    q = R.quantize(t, s[:, None, :]).reshape(rows, cols)
    return np.ascontiguousarray(q.T), s


def transposed_order(offsets, indices, col_blocks: int):
    """(offsets_t int32 [col_blocks + 1], indices_t int16 [nb], block_offsets
    int32 [nb]) as the device Transpose leaves them: the stored blocks by
    column, within a column in storage order."""
    offsets, indices = np.asarray(offsets), np.asarray(indices)
    rows = R.row_indices(offsets)
    offsets_t = np.zeros(col_blocks + 1, np.int32)
    for c in indices:
        offsets_t[int(c) + 1] += 1
    offsets_t = np.cumsum(offsets_t).astype(np.int32)
    fill = offsets_t[:-1].copy()
    indices_t = np.zeros(len(indices), np.int16)
    block_offsets = np.zeros(len(indices), np.int32)
    for b, c in enumerate(indices):
        at = fill[int(c)]
        indices_t[at], block_offsets[at] = rows[b], b
        fill[int(c)] += 1
    return offsets_t, indices_t, block_offsets


def quantize_blocks_t(values, block_offsets, pow2: bool = False):
    """Block values [nb, 128, 128] -> (qt uint8 [nb, 128, 128], scales_t
    float32 [nb * 128]): output block j is source block block_offsets[j]
    stored [column][row], scales_t[128 j + c] for source column c."""
    values = np.asarray(values, dtype=np.float32)
    t = np.ascontiguousarray(values[np.asarray(block_offsets)].transpose(0, 2, 1))
    return R.quantize_sparse(t, pow2)


# ---- the product ------------------------------------------------------------------

MODELS = ("block_scale", "mul_then_add")


def interval_sums(aq, bq) -> np.ndarray:
    """P [k / 128, m, n], float32, of aq [m, k] and bq [n, k] bytes."""
    k = np.shape(aq)[1]
    return np.stack([R.interval_sum(aq[:, kb * B:(kb + 1) * B],
                                    bq[:, kb * B:(kb + 1) * B])[0]
                     for kb in range(k // B)])


def chain(p, sa, sb, order, model=None) -> np.ndarray:
    """acc [m, n], float32: per block row the k-blocks `order` lists, s =
    float32(sa[row, kb] * sb[kb, col]), acc = fma32(s, p[kb], acc). sa [m,
    k / 128], sb [k / 128, n]. `model` names a wrong variant: block_scale
    uses one scale of B per 128 columns (the first column's), mul_then_add
    rounds s * P before the add."""
    p = np.asarray(p, np.float32)
    _, m, n = p.shape
    sa, sb = np.asarray(sa, np.float32), np.asarray(sb, np.float32)
    if model == "block_scale":
        sb = np.repeat(sb[:, ::B], B, axis=1)
    acc = np.zeros((m, n), np.float32)
    for rb in range(m // B):
        rows = slice(rb * B, (rb + 1) * B)
        for kb in order[rb]:
            with np.errstate(invalid="ignore", over="ignore"):
                s = sa[rows, kb:kb + 1] * sb[kb][None, :]
                if model == "mul_then_add":
                    acc[rows] = (s * p[kb, rows]) + acc[rows]
                else:
                    acc[rows] = R.fma32(s, p[kb, rows], acc[rows])
    return acc


def finish(acc, out: str, c_old=None, order=None) -> np.ndarray:
    """C as float32 values: round_out(acc), or with `c_old` round_out(acc +
    float(c_old)), one fp32 add and one rounding; `out` is "f16", "bf16" or
    "f32". Block rows with no step in `order` keep c_old."""
    acc = np.asarray(acc, np.float32)
    if c_old is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            acc = acc + np.asarray(c_old, np.float32)
    c = acc if out == "f32" else R.round_t(acc, out)
    if c_old is not None and order is not None:
        c = c.copy()
        for rb, steps in enumerate(order):
            if not steps:
                c[rb * B:(rb + 1) * B] = c_old[rb * B:(rb + 1) * B]
    return c


def bound(ref64, absum, k: int, out: str, fast: bool = False) -> np.ndarray:
    """... and in kFast EPS_FAST + (2 K / 128 + 2) 2^-23 in place of the
    last factor, as fp8_fast_ref.bound_fast."""
    from tests.fp8_fast_ref import EPS_FAST

    lead = 0.0 if out == "f32" else 2.0 ** -P_BITS[out] * np.abs(ref64)
    ops = (EPS_FAST + (2 * k // B + 2) * 2.0 ** -23 if fast
           else (k + 2 * k // B + 1) * 2.0 ** -23)
    return lead + ops * absum


def dequantize_cols(bq, sb) -> np.ndarray:
    """float64 B [k, n] of bytes [n, k] and scales [k / 128, n]."""
    return R.decode(np.asarray(bq)).T * np.repeat(np.asarray(sb, np.float64),
                                                  B, axis=0)


# ---- the cases of the product tests -------------------------------------------------

class Case:
    """One DsdFp8Wgrad on the host: the sparse operand as a dense matrix aq
    [m, k] bytes with sa [m, k / 128] (only its stored blocks exist), bq
    [n, k] bytes with sb [k / 128, n], and the sparse operand's topology."""

    def __init__(self, aq, sa, bq, sb, topology):
        self.aq, self.sa, self.bq, self.sb = aq, sa, bq, sb
        self.topology = topology
        self.m, self.k = aq.shape
        self.n = bq.shape[0]
        self.order = R.storage_order(*topology)

    def sparse(self):
        """(sq [nb, 128, 128], ss [nb * 128]) as the kernel takes them."""
        return R.Operands("dsd", self.aq, self.sa, self.bq, None,
                          self.topology).sparse()

    def acc(self, model=None, p=None):
        p = interval_sums(self.aq, self.bq) if p is None else p
        return chain(p, self.sa, self.sb, self.order, model)

    def copy(self):
        return Case(self.aq.copy(), self.sa.copy(), self.bq.copy(),
                    self.sb.copy(), self.topology)


def wgrad_topology():
    """The transposed SRC_TOPOLOGY: 4 x 6 blocks, block rows of 5, 0, 2 and
    1 stored blocks."""
    offsets_t, indices_t, _ = transposed_order(*SRC_TOPOLOGY, SRC_COLS // B)
    return offsets_t, indices_t


def _stored_mask(m, k, topology):
    stored = np.zeros((m // B, k // B), bool)
    stored[R.row_indices(topology[0]), topology[1]] = True
    return stored


def random_exact(seed) -> Case:
    """EXACT_BYTES at random with ordinary scales, per row of the sparse
    operand's blocks and per (k-block, column) of B; unstored blocks hold
    zero bytes and zero scales."""
    topo = wgrad_topology()
    m, k, n = SRC_COLS, SRC_ROWS, WGRAD_N
    rng = np.random.default_rng(seed)
    aq = R.EXACT_BYTES[rng.integers(0, len(R.EXACT_BYTES), (m, k))]
    bq = R.EXACT_BYTES[rng.integers(0, len(R.EXACT_BYTES), (n, k))]
    sa = R.ordinary_scales(rng, (m, k // B))
    sb = R.ordinary_scales(rng, (k // B, n))
    stored = _stored_mask(m, k, topo)
    sa = np.where(np.repeat(stored, B, axis=0), sa, np.float32(0))
    aq = np.where(np.repeat(np.repeat(stored, B, axis=0), B, axis=1), aq,
                  np.uint8(0))
    return Case(aq, sa, bq, sb, topo)


def exact_case(seed: int = 0) -> Case:
    """The rounding-visible inputs, after fp8_ref.exact_case: per block row
    the steps in storage order taken two by two as cancelling pairs (the
    second step has the first's B bytes and column scales, its A bytes with
    the sign flipped and its sa moved by -2 .. +2 ulps per row), so that what
    a pair leaves in the accumulator is the rounding residue of the fp32
    steps; a step left over after a pair is a one-hot block with sa scaled by
    2^-20, a block row of one step keeps its random block with sa scaled by
    2^-6."""
    case = random_exact([51, seed])
    rng = np.random.default_rng([52, seed])
    kbs = case.k // B
    rep = list(range(kbs))
    for steps in case.order:
        for a, b in zip(steps[0::2], steps[1::2]):
            ra, rb_ = rep[a], rep[b]
            rep = [min(ra, rb_) if r in (ra, rb_) else r for r in rep]
    for kb, r in enumerate(rep):
        case.bq[:, kb * B:(kb + 1) * B] = case.bq[:, r * B:(r + 1) * B]
        case.sb[kb] = case.sb[r]
    for rb, steps in enumerate(case.order):
        rows = slice(rb * B, (rb + 1) * B)
        for a, b in zip(steps[0::2], steps[1::2]):
            case.aq[rows, b * B:(b + 1) * B] = (
                case.aq[rows, a * B:(a + 1) * B] ^ np.uint8(0x80))
            ulps = rng.integers(-2, 3, B).astype(np.int32)
            case.sa[rows, b] = (case.sa[rows, a].view(np.int32)
                                + ulps).view(np.float32)
        if len(steps) % 2 and len(steps) > 1:
            last = steps[-1]
            i = np.arange(B)
            hot = np.zeros((B, B), np.uint8)
            vals = (np.where(i % 2, -1.0, 1.0) * (8 + i % 8) / 8.0
                    * np.exp2(i % 4))
            hot[i, (37 * (rb * B + i) + 11) % B] = [R.byte_of(v) for v in vals]
            case.aq[rows, last * B:(last + 1) * B] = hot
            case.sa[rows, last] *= np.float32(2.0 ** -20)
        if len(steps) == 1:   # |P| reaches 2^12: keep fp16 finite
            case.sa[rows, steps[0]] *= np.float32(2.0 ** -6)
    assert np.isin(case.aq, R.EXACT_BYTES).all()
    assert np.isin(case.bq, R.EXACT_BYTES).all()
    return case


def random_case(dtype: str, seed=0):
    """Random values of T quantised as the backward pass quantises them:
    (case, source block values, b [k, n])."""
    from tests.moe_ref import values

    nb = len(SRC_TOPOLOGY[1])
    src = values((nb, B, B), dtype, [53, seed, 1])
    b = values((SRC_ROWS, WGRAD_N), dtype, [53, seed, 2])
    return case_from_values(src, b), src, b


def case_from_values(src, b, pow2: bool = False) -> Case:
    """The Case of source block values [nb, 128, 128] on SRC_TOPOLOGY and a
    dense b [SRC_ROWS, n]: the source's transpose times b."""
    offsets_t, indices_t, block_offsets = transposed_order(*SRC_TOPOLOGY,
                                                           SRC_COLS // B)
    topo = (offsets_t, indices_t)
    qt, st = quantize_blocks_t(src, block_offsets, pow2)
    aq = R.dense_from_blocks(SRC_COLS, SRC_ROWS, *topo, qt)
    sa = R.expand_block_scales(SRC_COLS, SRC_ROWS, *topo, st)
    bq, sb = quantize_cols(b, pow2)
    return Case(aq, sa, bq, sb, topo)


def tie_case(out: str) -> Case:
    """Every stored output has acc = 2^-p exactly (p = 11 for fp16, 8 for
    bf16): one-hot rows of 1.0 against all-ones B, sa = 2^-p at the first
    step of a block row and 0 at the others, sb = 1. Added to C_old = 1 or 1 +
    2^-(p - 1) the sum is a tie of round_T."""
    case = random_exact([54])
    i = np.arange(case.m)
    case.bq[:] = R.ONE
    case.sb[:] = 1.0
    case.sa[:] = 0.0
    for rb, steps in enumerate(case.order):
        rows = slice(rb * B, (rb + 1) * B)
        for n_step, kb in enumerate(steps):
            hot = np.zeros((B, B), np.uint8)
            hot[np.arange(B), (37 * i[rows] + 11) % B] = R.ONE
            case.aq[rows, kb * B:(kb + 1) * B] = hot
            if n_step == 0:
                case.sa[rows, kb] = 2.0 ** -P_BITS[out]
    return case
