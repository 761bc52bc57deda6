"""Numpy reference of the fp8 products (sputnik/block/fp8.h), shared by
tests/test_fp8_host.py and tests/test_gpu_fp8*.py. Nothing here calls the
library.

    decode / encode          OCP e4m3fn bytes <-> values (encode: round to
                             nearest even; test_fp8_host.py holds it against
                             torch's float8_e4m3fn cast)
    scale                    the two scale rules, in float32
    quantize_rows / _sparse / _weight
                             bytes and scales as the quantisers must give
                             them, bit for bit
    hidden                   the H a fused quantiser sees: the epilogue ops of
                             tests/activation_ref.py and tests/gated_ref.py
                             rounded to T (exact for relu; gelu / silu go
                             through the device's exp and reciprocal, so the
                             GPU tests take that H from the 16-bit kernels)
    dequantize_*             float64 operands from bytes and scales
    matmul64                 float64 products with their sum |terms|
                             (dense_from_blocks / blocks_from_dense move a
                             sparse operand or result in and out of it)
    product32                the fp32 arithmetic of the kernel, emulated
    bound                    the acceptance bound of the random-data tests
    fma32 / accumulate       the same arithmetic correctly rounded (no float64
                             double rounding), NaN / Inf aware, and the wrong
                             models of it (MODELS) that test_fp8_host.py shows
                             visible on the exact cases
    exact_case / byte_case / special_case / tie_case
                             the inputs of tests/test_gpu_fp8_exact.py

Bound: |gpu - ref64| <= 2^-P_BITS[T] |ref64| + (K + 2 K / 128) 2^-23
sum |terms|, the form and constants of moe_ref.scatter_bound: one rounding
to T of the exact sum, plus 2^-23 per fp32 operation (which covers an
accumulator that truncates), K products and two scale multiplies per scale
interval.
"""

from __future__ import annotations

import numpy as np

from oracle import oracle as O
from tests.activation_ref import act32
from tests.gated_ref import gate32
from tests.moe_ref import P_BITS

B = 128
FP8_MAX = np.float32(448.0)
SCALE_FLOOR = np.float32(2.0 ** -126)
NAN_BYTE = 0x7F


# ---- e4m3fn -------------------------------------------------------------------

def _decode_table() -> np.ndarray:
    t = np.empty(256, dtype=np.float64)
    for b in range(256):
        e, m = (b >> 3) & 15, b & 7
        if (b & 0x7F) == 0x7F:
            v = np.nan
        elif e == 0:
            v = m * 2.0 ** -9
        else:
            v = (8 + m) * 2.0 ** (e - 10)
        t[b] = -v if b & 0x80 else v
    return t


DECODE = _decode_table()


def decode(q: np.ndarray) -> np.ndarray:
    """float64 values of e4m3fn bytes (0x7F / 0xFF: NaN; the zeros keep
    their sign)."""
    return DECODE[np.asarray(q, dtype=np.uint8)]


def encode(v) -> np.ndarray:
    """rne_e4m3 of finite float32 values with |v| < 464, as bytes."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    u = v.view(np.uint32)
    a = u & np.uint32(0x7FFFFFFF)
    normal = ((a + np.uint32(0x7FFFF) + ((a >> np.uint32(20)) & np.uint32(1)))
              >> np.uint32(20)).astype(np.int64) - (120 << 3)
    normal = np.minimum(normal, 0x7E)
    is_normal = a >= np.uint32(0x3C800000)  # |v| >= 2^-6
    sub = np.rint(np.where(is_normal, 0, a.view(np.float32)).astype(np.float64)
                  * 512.0).astype(np.int64)
    mag = np.where(is_normal, normal, sub)
    return (((u >> np.uint32(24)) & np.uint32(0x80)).astype(np.int64)
            | mag).astype(np.uint8)


# ---- scales -------------------------------------------------------------------

def amax_finite(x: np.ndarray, axis) -> np.ndarray:
    """Largest |x| over the finite elements along `axis` (0 without any)."""
    x = np.asarray(x, dtype=np.float32)
    return np.max(np.where(np.isfinite(x), np.abs(x), np.float32(0)),
                  axis=axis).astype(np.float32)


def scale(amax, pow2: bool = False) -> np.ndarray:
    amax = np.asarray(amax, dtype=np.float32)
    if not pow2:
        with np.errstate(under="ignore"):
            return np.maximum(amax / FP8_MAX, SCALE_FLOOR).astype(np.float32)
    m, e = np.frexp(amax)  # amax = m 2^e, m in [0.5, 1)
    e = e - np.where(m <= np.float32(0.875), 9, 8)
    s = np.ldexp(np.float32(1), np.maximum(e, -126)).astype(np.float32)
    return np.where(amax == 0, SCALE_FLOOR, s).astype(np.float32)


def scaled_value(x, s) -> np.ndarray:
    """float32(x) / s in float32: what the encoder sees (finite x)."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return (np.asarray(x, np.float32) / np.asarray(s, np.float32)).astype(
            np.float32)


def quantize(x, s) -> np.ndarray:
    """Bytes of x under the (broadcast) scales s; NaN and +-Inf give the
    e4m3 NaN with the element's sign."""
    x = np.asarray(x, dtype=np.float32)
    finite = np.isfinite(x)
    q = encode(np.where(finite, scaled_value(np.where(finite, x, 0), s), 0))
    special = (NAN_BYTE | (np.signbit(x).astype(np.uint8) << 7)).astype(np.uint8)
    return np.where(finite, q, special).astype(np.uint8)


# ---- the three quantisers ------------------------------------------------------

def quantize_rows(x, pow2: bool = False):
    """x [rows, cols] (values of T as float32) -> (q uint8 [rows, cols],
    scales float32 [rows, cols / 128])."""
    x = np.asarray(x, dtype=np.float32)
    rows, cols = x.shape
    t = x.reshape(rows, cols // B, B)
    s = scale(amax_finite(t, axis=2), pow2)
    return quantize(t, s[:, :, None]).reshape(rows, cols), s


def quantize_sparse(values, pow2: bool = False):
    """Block values [nb, 128, 128] -> (q uint8 [nb, 128, 128], scales float32
    [nb * 128]): row tiles of the matrix [nb * 128, 128]."""
    values = np.asarray(values, dtype=np.float32)
    q, s = quantize_rows(values.reshape(-1, B), pow2)
    return q.reshape(values.shape), s.reshape(-1)


def quantize_weight(w, pow2: bool = False):
    """w [k, n] -> (q uint8 [n, k], scales float32 [k / 128, n / 128])."""
    w = np.asarray(w, dtype=np.float32)
    k, n = w.shape
    t = w.reshape(k // B, B, n // B, B)
    s = scale(amax_finite(t, axis=(1, 3)), pow2)
    q = quantize(t, s[:, None, :, None]).reshape(k, n)
    return np.ascontiguousarray(q.T), s


def hidden(act: str, x, gate=None, dtype: str = "f16") -> np.ndarray:
    """round_T(act(x)), or round_T(x * act(gate)), float32 values of T: the
    float32 stand-ins of activation_ref / gated_ref (bit-exact with the
    device for relu only)."""
    if gate is None:
        h = act32(act, x) + np.float32(0)
    else:
        h = gate32(act, x, gate)
    return O.round_to(np.asarray(h, dtype=np.float32), dtype)


# ---- products -----------------------------------------------------------------

def dequantize_rows(q, s) -> np.ndarray:
    """float64 [rows, cols] of bytes [rows, cols] and scales [rows, cols/128]."""
    q = np.asarray(q)
    return decode(q) * np.repeat(np.asarray(s, np.float64), B, axis=1)


def dequantize_weight(q, s) -> np.ndarray:
    """float64 w [k, n] of bytes [n, k] and scales [k / 128, n / 128]."""
    s = np.asarray(s, np.float64)
    return decode(np.asarray(q)).T * np.repeat(np.repeat(s, B, axis=0), B, axis=1)


def dense_from_blocks(rows, cols, offsets, indices, blocks) -> np.ndarray:
    out = np.zeros((rows, cols), dtype=np.asarray(blocks).dtype)
    for r in range(rows // B):
        for j in range(int(offsets[r]), int(offsets[r + 1])):
            c = int(indices[j])
            out[r * B:(r + 1) * B, c * B:(c + 1) * B] = blocks[j]
    return out


def blocks_from_dense(dense, offsets, indices) -> np.ndarray:
    rows = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    return np.stack([dense[r * B:(r + 1) * B, int(c) * B:(int(c) + 1) * B]
                     for r, c in zip(rows, indices)]) if len(indices) else (
        np.zeros((0, B, B), dtype=dense.dtype))


def matmul64(a64, w64):
    """(a w, |a| |w|) in float64."""
    return a64 @ w64, np.abs(a64) @ np.abs(w64)


def product32(aq, sa, wq, sw, order=None) -> np.ndarray:
    """The kernel's arithmetic emulated: per k-block (ascending, or in
    `order`, a list of k-blocks per block row of A) P = the float32-rounded
    sum of the 128 products and acc = fma(sa * sw, P, acc) in float32.
    aq [m, k] bytes with sa [m, k / 128]; wq [n, k] bytes with sw [k / 128,
    n / 128]. Returns acc, float32 [m, n]."""
    a, w = decode(aq), decode(wq)
    m, k = a.shape
    n = w.shape[0]
    acc = np.zeros((m, n), dtype=np.float32)
    sa = np.asarray(sa, np.float32)
    sw = np.asarray(sw, np.float32)
    for rb in range(m // B):
        rows = slice(rb * B, (rb + 1) * B)
        for kb in (range(k // B) if order is None else order[rb]):
            ks = slice(kb * B, (kb + 1) * B)
            p = (a[rows, ks] @ w[:, ks].T).astype(np.float32)
            s = (sa[rows, kb:kb + 1] * np.repeat(sw[kb], B)[None, :]).astype(
                np.float32)
            acc[rows] = (s.astype(np.float64) * p.astype(np.float64)
                         + acc[rows].astype(np.float64)).astype(np.float32)
    return acc


def bound(ref64, absum, k: int, dtype: str) -> np.ndarray:
    return (2.0 ** -P_BITS[dtype] * np.abs(ref64)
            + (k + 2 * k // B) * 2.0 ** -23 * absum)


# ---- the cases of the GEMM tests ----------------------------------------------
#
# SDD: C [256, 384] = A [256, 256] . W [256, 384], C with 5 of its 6 blocks,
# column indices out of order. DSD: C [384, 384] = S [384, 256] . W, S with an
# empty block row and column indices out of order.
SDD_M, SDD_K, SDD_N = 256, 256, 384
SDD_TOPOLOGY = (np.array([0, 3, 5], np.int32),
                np.array([2, 0, 1, 1, 0], np.int16))
DSD_M, DSD_K, DSD_N = 384, 256, 384
DSD_TOPOLOGY = (np.array([0, 2, 2, 4], np.int32),
                np.array([1, 0, 1, 0], np.int16))


def row_indices(offsets) -> np.ndarray:
    return np.repeat(np.arange(len(offsets) - 1), np.diff(offsets)).astype(
        np.int16)


def kat_rows(m: int, k: int) -> np.ndarray:
    """One-hot rows: row i holds x_i = +-(8 + i % 8) / 8 * 2^(i % 7 - 3) at
    column (37 i + 11) % k, a different k per row that covers every k of a
    block. 4 significant bits: exact in e4m3 under a pow2 scale, and the
    scale differs per row and per k-block (the other k-blocks are all zero)."""
    i = np.arange(m)
    x = np.zeros((m, k), dtype=np.float32)
    x[i, (37 * i + 11) % k] = (np.where(i % 2, -1.0, 1.0) * (8 + i % 8) / 8.0
                               * np.exp2(i % 7 - 3))
    return x


def kat_weight(k: int, n: int) -> np.ndarray:
    """Distinct small integers in an asymmetric pattern, (7 k + 11 n) % 15 - 7,
    times a power of two per 128 x 128 block."""
    kk, nn = np.meshgrid(np.arange(k), np.arange(n), indexing="ij")
    return (((7 * kk + 11 * nn) % 15 - 7)
            * np.exp2((kk // B + 2 * (nn // B)) % 3)).astype(np.float32)


def expand_block_scales(m, k, offsets, indices, s_blocks) -> np.ndarray:
    """Dense [m, k / 128] row scales from the per-block-row scales of a
    sparse operand ([nb * 128]); 0 where no block is stored."""
    out = np.zeros((m, k // B), dtype=np.float32)
    s_blocks = np.asarray(s_blocks, np.float32).reshape(-1, B)
    for r in range(m // B):
        for j in range(int(offsets[r]), int(offsets[r + 1])):
            out[r * B:(r + 1) * B, int(indices[j])] = s_blocks[j]
    return out


def storage_order(offsets, indices):
    """The k-blocks of every block row in storage order (product32's order)."""
    return [[int(c) for c in indices[int(offsets[r]):int(offsets[r + 1])]]
            for r in range(len(offsets) - 1)]


# ---- the arithmetic, correctly rounded, and wrong models of it -----------------
#
# product32 above adds in float64 and casts, which can round twice. fma32 is
# the fused step without that: s * p is exact in float64 (24 + 24 bits), the
# float64 add is rounded to odd with the TwoSum residual, and a
# round-to-nearest cast of a round-to-odd value with two spare bits is the
# correctly rounded result.

def fma32(s, p, acc) -> np.ndarray:
    """float32(s * p + acc), rounded once, of float32 arrays (IEEE for NaN,
    Inf and 0 * Inf)."""
    s64 = np.asarray(s, np.float32).astype(np.float64)
    p64 = np.asarray(p, np.float32).astype(np.float64)
    a64 = np.asarray(acc, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        prod = s64 * p64
        t = prod + a64
        bb = t - prod
        err = (prod - (t - bb)) + (a64 - bb)
        fix = np.isfinite(t) & (err != 0) & (
            (np.ascontiguousarray(t).view(np.uint64) & np.uint64(1)) == 0)
        odd = np.nextafter(t, np.where(err > 0, np.inf, -np.inf))
        return np.where(fix, odd, t).astype(np.float32)


def interval_sum(a_bytes, w_bytes) -> np.ndarray:
    """P of one scale interval: a_bytes [128, 128] . w_bytes [n, 128]^T from
    +0, float32. A NaN byte makes its whole row (of A) or column (of W) NaN,
    without sending a NaN through BLAS; sums of zeros are +0. Returns (P,
    sum |products|)."""
    a, w = decode(a_bytes), decode(w_bytes)
    bad_a, bad_w = np.isnan(a), np.isnan(w)
    a, w = np.where(bad_a, 0.0, a), np.where(bad_w, 0.0, w)
    p = (a @ w.T + 0.0).astype(np.float32)
    p[bad_a.any(axis=1), :] = np.nan
    p[:, bad_w.any(axis=1)] = np.nan
    return p, np.abs(a) @ np.abs(w).T


MODELS = ("mul_then_add", "scale_after_p", "exact_scale", "ascending_order",
          "partial_in_T", "round_half_up")


def accumulate(aq, sa, wq, sw, order=None, model=None, dtype=None,
               exact_p=False) -> np.ndarray:
    """acc [m, n], float32, of sputnik/block/fp8.h: per block row the
    k-blocks ascending or as `order` lists them, s = float32(sa * sw), acc =
    fma32(s, P, acc). `model` names a wrong variant (MODELS; partial_in_T
    needs `dtype`, round_half_up is in `rounded`): mul_then_add rounds s * P
    before the add, scale_after_p is fma32(float32(sa * P), sw, acc),
    exact_scale leaves sa * sw unrounded (to float64 precision),
    ascending_order ignores `order`, partial_in_T rounds acc to T after every
    step. With `exact_p` asserts that every interval's sum |products| is
    below 2^24 units of 2^-6, so that P is exact in any summation order."""
    m, k = np.shape(aq)
    n = np.shape(wq)[0]
    sa = np.asarray(sa, np.float32)
    sw = np.asarray(sw, np.float32)
    acc = np.zeros((m, n), dtype=np.float32)
    f64 = np.float64
    for rb in range(m // B):
        rows = slice(rb * B, (rb + 1) * B)
        steps = range(k // B) if order is None else order[rb]
        if model == "ascending_order":
            steps = sorted(steps)
        for kb in steps:
            ks = slice(kb * B, (kb + 1) * B)
            p, absum = interval_sum(aq[rows, ks], wq[:, ks])
            if exact_p:
                assert absum.max() * 64 < 2.0 ** 24
            a_s = sa[rows, kb:kb + 1]
            w_s = np.repeat(sw[kb], B)[None, :]
            with np.errstate(invalid="ignore", over="ignore"):
                s = a_s * w_s                      # float32, rounded
                if model == "mul_then_add":
                    acc[rows] = (s * p) + acc[rows]
                elif model == "scale_after_p":
                    acc[rows] = fma32(a_s * p, np.broadcast_to(w_s, p.shape),
                                      acc[rows])
                elif model == "exact_scale":
                    acc[rows] = (a_s.astype(f64) * w_s.astype(f64)
                                 * p.astype(f64) + acc[rows].astype(f64)
                                 ).astype(np.float32)
                else:
                    acc[rows] = fma32(s, p, acc[rows])
            if model == "partial_in_T":
                acc[rows] = round_t(acc[rows], dtype)
    return acc


def round_t(acc32, dtype: str, model=None) -> np.ndarray:
    """round_T(acc), once, nearest even, as float32 (overflow: +-Inf); with
    model == "round_half_up" ties go away from zero."""
    from tests import rounding_ref as RR

    conv = RR.round_half_up if model == "round_half_up" else RR.round_once
    return conv(np.asarray(acc32, np.float32).astype(np.float64), dtype)


def rounded(aq, sa, wq, sw, dtype, order=None, model=None) -> np.ndarray:
    """round_T of `accumulate` under `model`: the C the contract fixes (model
    None), float32 [m, n]."""
    return round_t(accumulate(aq, sa, wq, sw, order, model, dtype), dtype,
                   model)


# ---- the deep cases and their exact inputs --------------------------------------
#
# SDD deep: C [256, 384] with SDD_TOPOLOGY and K = 128 (1 step), 384 (3: the
# smallest with a refill of a ring stage) or 640 (5: odd, two refills of stage
# 0). DSD deep: m, k, n blocks 4, 5, 2, all different; block rows of 5, 0, 1
# and 3 stored blocks, each out of order.
SDD_DEEP_M, SDD_DEEP_N = 256, 384
SDD_DEEP_K = (128, 384, 640)
DSD_DEEP_M, DSD_DEEP_K, DSD_DEEP_N = 512, 640, 256
DSD_DEEP_TOPOLOGY = (np.array([0, 5, 5, 6, 9], np.int32),
                     np.array([3, 0, 4, 1, 2, 4, 1, 4, 0], np.int16))

# The e4m3 bytes whose value is a multiple of 1/8 with |v| <= 15 (80 of them,
# the two zeros included): a product is a multiple of 2^-6 of at most 225, so
# every partial sum of 128 products is below 2^21 units and exact in fp32.
EXACT_BYTES = np.array([b for b in range(256)
                        if np.isfinite(DECODE[b]) and abs(DECODE[b]) <= 15
                        and DECODE[b] * 8 == np.rint(DECODE[b] * 8)], np.uint8)
ONE = 0x38


def byte_of(v: float) -> int:
    """The e4m3 byte of a value e4m3 holds exactly."""
    (b,) = np.flatnonzero((DECODE == v) & (np.signbit(DECODE)
                                           == np.signbit(v)))
    return int(b)


class Operands:
    """One product on the host. aq [m, k] bytes and sa [m, k / 128] are the
    left operand as a dense matrix; for DSD (`topology` is the sparse
    operand's, for SDD it is C's) only its stored blocks exist, `order` is
    their storage order and `sparse()` gives the operand as the kernel takes
    it."""

    def __init__(self, kind, aq, sa, wq, sw, topology):
        self.kind, self.topology = kind, topology
        self.aq, self.sa, self.wq, self.sw = aq, sa, wq, sw
        self.m, self.k = aq.shape
        self.n = wq.shape[0]
        self.order = storage_order(*topology) if kind == "dsd" else None

    def sparse(self):
        """(sq [nb, 128, 128], ss [nb * 128]) of a DSD's left operand."""
        offsets, indices = self.topology
        sq = blocks_from_dense(self.aq, offsets, indices)
        rows = row_indices(offsets)
        ss = np.concatenate([self.sa[r * B:(r + 1) * B, int(c)]
                             for r, c in zip(rows, indices)])
        return np.ascontiguousarray(sq), ss.astype(np.float32)

    def acc(self, model=None, dtype=None, order=None, exact_p=False):
        return accumulate(self.aq, self.sa, self.wq, self.sw,
                          self.order if order is None else order, model,
                          dtype, exact_p)

    def expected(self, dtype, model=None, order=None):
        """round_T(acc) in C's layout: [m, n], or C's stored blocks (SDD)."""
        c = round_t(self.acc(model, dtype, order), dtype, model)
        if self.kind == "sdd":
            return blocks_from_dense(c, *self.topology)
        return c

    def copy(self):
        return Operands(self.kind, self.aq.copy(), self.sa.copy(),
                        self.wq.copy(), self.sw.copy(), self.topology)


def ordinary_scales(rng, shape) -> np.ndarray:
    """uniform[1, 2) * 2^[-3, 3], float32: not powers of two."""
    return (rng.uniform(1.0, 2.0, shape)
            * np.exp2(rng.integers(-3, 4, shape))).astype(np.float32)


def _deep_shape(kind, k):
    if kind == "sdd":
        return SDD_DEEP_M, k, SDD_DEEP_N, SDD_TOPOLOGY
    return DSD_DEEP_M, DSD_DEEP_K, DSD_DEEP_N, DSD_DEEP_TOPOLOGY


def random_exact(kind: str, k: int, seed) -> Operands:
    """EXACT_BYTES at random with ordinary scales (a DSD's unstored blocks
    hold zero bytes and zero scales)."""
    m, k, n, topo = _deep_shape(kind, k)
    rng = np.random.default_rng(seed)
    aq = EXACT_BYTES[rng.integers(0, len(EXACT_BYTES), (m, k))]
    wq = EXACT_BYTES[rng.integers(0, len(EXACT_BYTES), (n, k))]
    sa = ordinary_scales(rng, (m, k // B))
    sw = ordinary_scales(rng, (k // B, n // B))
    if kind == "dsd":
        stored = np.zeros((m // B, k // B), bool)
        stored[row_indices(topo[0]), topo[1]] = True
        sa = np.where(np.repeat(stored, B, axis=0), sa, np.float32(0))
        aq = np.where(np.repeat(np.repeat(stored, B, axis=0), B, axis=1), aq,
                      np.uint8(0))
    return Operands(kind, aq, sa, wq, sw, topo)


def _shape(kind: str, deep: bool):
    if deep:
        return _deep_shape(kind, SDD_DEEP_K[-1])
    if kind == "sdd":
        return SDD_M, SDD_K, SDD_N, SDD_TOPOLOGY
    return DSD_M, DSD_K, DSD_N, DSD_TOPOLOGY


def _from_values(kind, x, w, topo, pow2) -> Operands:
    """Operands quantised from values: x [m, k] (a DSD's through its stored
    blocks, as quantize_sparse takes them) and w [k, n]."""
    wq, sw = quantize_weight(w, pow2)
    if kind == "sdd":
        aq, sa = quantize_rows(x, pow2)
    else:
        m, k = x.shape
        sq, ss = quantize_sparse(blocks_from_dense(x, *topo), pow2)
        aq = dense_from_blocks(m, k, *topo, sq)
        sa = expand_block_scales(m, k, *topo, ss)
    return Operands(kind, aq, sa, wq, sw, topo)


def random_case(kind: str, deep: bool, dtype: str) -> Operands:
    """The random-data case of test_random_*_within_bound (the seeds of the
    shallow cases are those tests' own)."""
    from tests.moe_ref import values

    m, k, n, topo = _shape(kind, deep)
    seed = [11 if kind == "sdd" else 12] + ([k] if deep else [])
    w = values((k, n), dtype, seed + [2])
    if kind == "sdd":
        x = values((m, k), dtype, seed + [1])
    else:
        x = dense_from_blocks(m, k, *topo, values((len(topo[1]), B, B), dtype,
                                                  seed + [1]))
    return _from_values(kind, x, w, topo, False)


def kat_case(kind: str, deep: bool):
    """The lane-map known-answer case: (operands, x, w) with x = kat_rows
    (zero outside a DSD's stored blocks) and w = kat_weight, pow2 scales."""
    m, k, n, topo = _shape(kind, deep)
    x, w = kat_rows(m, k), kat_weight(k, n)
    if kind == "dsd":
        stored = np.zeros((m // B, k // B), bool)
        stored[row_indices(topo[0]), topo[1]] = True
        x = np.where(np.repeat(np.repeat(stored, B, axis=0), B, axis=1), x,
                     np.float32(0))
    return _from_values(kind, x, w, topo, True), x, w


def exact_case(kind: str, k: int = DSD_DEEP_K, seed: int = 0) -> Operands:
    """The rounding-visible inputs: EXACT_BYTES, ordinary scales, and per
    block row the steps (in k order, or the row's storage order) taken two by
    two as cancelling pairs: the second step of a pair has the first's W
    bytes and sw row, its A bytes with the sign bit flipped and its sa moved
    by -2 .. +2 ulps per row, so that what a pair leaves in the accumulator
    is the rounding residue of the fp32 steps. A step left over after at
    least one pair is a one-hot row (kat_rows' columns) with sa scaled by
    2^-20, which is of the residues' size; a block row of one step keeps its
    random block, with sa scaled by 2^-6."""
    m, k, n, topo = _deep_shape(kind, k)
    ops = random_exact(kind, k, [41, seed, k])
    rng = np.random.default_rng([42, seed, k])
    order = ops.order or [list(range(k // B))] * (m // B)
    # k-blocks that must share W bytes and sw (a DSD's rows pair different
    # k-blocks, and the pairs have to agree)
    rep = list(range(k // B))
    for steps in order:
        for a, b in zip(steps[0::2], steps[1::2]):
            ra, rb_ = rep[a], rep[b]
            rep = [min(ra, rb_) if r in (ra, rb_) else r for r in rep]
    for kb, r in enumerate(rep):
        ops.wq[:, kb * B:(kb + 1) * B] = ops.wq[:, r * B:(r + 1) * B]
        ops.sw[kb] = ops.sw[r]
    for rb, steps in enumerate(order):
        rows = slice(rb * B, (rb + 1) * B)
        for a, b in zip(steps[0::2], steps[1::2]):
            ops.aq[rows, b * B:(b + 1) * B] = (
                ops.aq[rows, a * B:(a + 1) * B] ^ np.uint8(0x80))
            ulps = rng.integers(-2, 3, B).astype(np.int32)
            ops.sa[rows, b] = (ops.sa[rows, a].view(np.int32)
                               + ulps).view(np.float32)
        if len(steps) % 2 and len(steps) > 1:
            last = steps[-1]
            i = np.arange(B)
            hot = np.zeros((B, B), np.uint8)
            # +-(8 + i % 8) / 8 * 2^(i % 4): 1 .. 15, multiples of 1/8
            vals = (np.where(i % 2, -1.0, 1.0) * (8 + i % 8) / 8.0
                    * np.exp2(i % 4))
            hot[i, (37 * (rb * B + i) + 11) % B] = [byte_of(v) for v in vals]
            ops.aq[rows, last * B:(last + 1) * B] = hot
            ops.sa[rows, last] *= np.float32(2.0 ** -20)
        if len(steps) == 1:   # |P| reaches 2^12: keep fp16 finite
            ops.sa[rows, steps[0]] *= np.float32(2.0 ** -6)
    assert np.isin(ops.aq, EXACT_BYTES).all()
    assert np.isin(ops.wq, EXACT_BYTES).all()
    return ops


def tie_case(dtype: str) -> Operands:
    """SDD, K = 128, every output a tie of round_T: one-hot rows and weights
    that hold +-2^j only, sa = 1 + 2^-p (p = 11 for fp16, 8 for bf16: half a
    unit of T above 1) and sw a power of two, so acc = +-2^e (1 + 2^-p)
    exactly and round-to-nearest-even gives +-2^e where ties-away gives the
    next value up."""
    m, k, n, topo = _deep_shape("sdd", B)
    i, j = np.arange(m), np.arange(n)
    aq = np.zeros((m, k), np.uint8)
    aq[i, (37 * i + 11) % k] = [byte_of(v) for v in
                                np.where(i % 2, -1.0, 1.0) * np.exp2(i % 4)]
    wq = np.empty((n, k), np.uint8)
    kk = np.arange(k)
    wq[:] = np.array([byte_of(v) for v in np.exp2(np.arange(-3.0, 4.0))]
                     )[(j[:, None] + 3 * kk[None, :]) % 7]
    wq[(j[:, None] + kk[None, :]) % 3 == 0] ^= np.uint8(0x80)
    sa = np.full((m, 1), 1.0 + 2.0 ** -P_BITS[dtype], np.float32)
    sw = np.exp2(np.arange(n // B, dtype=np.float32) - 1).reshape(1, -1)
    return Operands("sdd", aq, sa, wq, sw, topo)


# ---- every byte through the decode ----------------------------------------------

BYTE_K = 384


def byte_case(kind: str, patterned: str) -> Operands:
    """K = 384, pow2 scales from {1, 2, 4} per row and per block. One operand
    one-hot with 1.0 at column (37 i + 11) % K of row i, the other
    (`patterned`: "a" or "w") holds (row + 3 col) & 0xFF with the two NaN
    bytes replaced by their neighbours 0x7E / 0xFE. Every output is one
    decoded byte times two powers of two."""
    if kind == "sdd":
        m, k, n, topo = SDD_DEEP_M, BYTE_K, SDD_DEEP_N, SDD_TOPOLOGY
    else:  # every block stored, in a rotated order per block row
        m, k, n = 384, BYTE_K, 256
        topo = (np.array([0, 3, 6, 9], np.int32),
                np.array([2, 0, 1, 0, 1, 2, 1, 2, 0], np.int16))

    def one_hot(rows):
        q = np.zeros((rows, k), np.uint8)
        i = np.arange(rows)
        q[i, (37 * i + 11) % k] = ONE
        return q

    def pattern(rows):
        q = ((np.arange(rows)[:, None] + 3 * np.arange(k)[None, :]) & 0xFF
             ).astype(np.uint8)
        return np.where((q & 0x7F) == 0x7F, q - np.uint8(1), q)

    aq = pattern(m) if patterned == "a" else one_hot(m)
    wq = one_hot(n) if patterned == "a" else pattern(n)
    sa = np.exp2((np.arange(m)[:, None] + np.arange(k // B)[None, :]) % 3
                 ).astype(np.float32)
    sw = np.exp2((np.arange(k // B)[:, None] + 2 * np.arange(n // B)[None, :])
                 % 3).astype(np.float32)
    return Operands(kind, aq, sa, wq, sw, topo)


def byte_case_expected(ops: Operands) -> np.ndarray:
    """decode(byte) * sa * sw per output, float64 [m, n], straight from the
    definition (not through `accumulate`); a -0 byte gives +0."""
    a = decode(ops.aq) * np.repeat(ops.sa.astype(np.float64), B, axis=1)
    w = decode(ops.wq) * np.repeat(np.repeat(ops.sw.astype(np.float64), B,
                                             axis=0), B, axis=1).T
    out = np.zeros((ops.m, ops.n))
    if (ops.aq != 0).sum() == ops.m:      # A one-hot: C[i, j] = a_i w[j, c_i]
        c = np.argmax(ops.aq != 0, axis=1)
        out = a[np.arange(ops.m), c][:, None] * w[:, c].T
    else:
        c = np.argmax(ops.wq != 0, axis=1)
        out = a[:, c] * w[np.arange(ops.n), c][None, :]
    return out + 0.0


def byte_case_coverage(ops: Operands) -> np.ndarray:
    """bool [256, 16, 2]: byte b was multiplied by the one-hot 1.0 into a
    stored output from byte position col % 16 of a lane's first (chunks 0-3
    of the 128-byte row) or second (chunks 4-7) 16-byte read."""
    seen = np.zeros((256, 16, 2), bool)
    offsets, indices = ops.topology
    a_hot = (ops.aq != 0).sum() == ops.m
    hot = ops.aq if a_hot else ops.wq
    col = np.argmax(hot != 0, axis=1)
    pat = ops.wq if a_hot else ops.aq
    if ops.kind == "sdd":
        tiles = list(zip(row_indices(offsets), indices))
    else:
        tiles = [(r, c) for r in range(ops.m // B) for c in range(ops.n // B)]
    for r, c in tiles:
        rows, cols = np.arange(r * B, (r + 1) * B), np.arange(c * B, (c + 1) * B)
        hot_ids, pat_ids = (rows, cols) if a_hot else (cols, rows)
        cc = col[hot_ids]
        b = pat[np.ix_(pat_ids, cc)]
        pos = np.broadcast_to(cc[None, :], b.shape)
        seen[b, pos % 16, (pos % B) // 64] = True
    return seen


# ---- non-finite values and overflow ---------------------------------------------

def special_case(kind: str, what: str, seed: int = 0):
    """random_exact (SDD: K = 384; DSD deep) with one item planted; returns
    (operands, note). `what`: "nan_a" a 0x7F in A, "nan_w" a 0xFF in W,
    "inf_sa" sa = +Inf on one row of one interval, that row one-hot there
    and a quarter of W's bytes at its column zero, so that P = 0 and 0 * Inf
    = NaN at those outputs, "nan_sw" sb = NaN on one (kb, nb), "overflow" three one-hot rows
    whose accumulator reaches 65520 (1 + 2^-10), 65520 exactly (fp16's tie to
    Inf) and the float32 below 65520, at the columns where W holds +-15."""
    ops = random_exact(kind, 384, [43, seed, kind == "dsd"])
    ops.sa *= np.float32(2.0 ** -8)         # |C| of order 10^2: fp16 finite
    order = ops.order or [list(range(ops.k // B))] * (ops.m // B)
    rb = 0 if kind == "sdd" else 3          # a block row with several steps
    # its second step; DSD: its third, k-block 0, which block row 2 lacks
    kb = order[rb][2 if kind == "dsd" else 1]
    row = rb * B + 77
    if what == "nan_a":
        ops.aq[row, kb * B + 21] = 0x7F
    elif what == "nan_w":
        ops.wq[200, kb * B + 90] = 0xFF
    elif what == "inf_sa":
        ops.sa[row, kb] = np.inf
        # P = 0 at some outputs of that row: 0 * Inf is NaN there
        ops.aq[row, kb * B:(kb + 1) * B] = 0
        ops.aq[row, kb * B + 5] = ONE
        ops.wq[3::4, kb * B + 5] = 0
    elif what == "nan_sw":
        ops.sw[kb, 1] = np.nan
    elif what == "overflow":
        c = kb * B + 9
        ops.wq[10, c], ops.wq[11, c] = byte_of(15.0), byte_of(-15.0)
        ops.sw[kb, 0] = 1.0
        base = np.float32(65520.0 / 15.0)   # 4368
        for r, s in ((row, base * np.float32(1 + 2.0 ** -10)),
                     (row + 1, base),
                     (row + 2, np.nextafter(base, np.float32(0)))):
            ops.aq[r] = 0
            ops.aq[r, c] = ONE
            ops.sa[r, kb] = s
    else:
        raise ValueError(what)
    return ops, (row, kb)
