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
