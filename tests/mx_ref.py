"""Host reference of the MX formats of sputnik/block/mx.h (numpy only): the
e8m0 scale rule per element type, the e4m3 (tests/fp8_ref.py's codec) and
e2m1 quantisers, their decoders, and the float64 product over decoded
operands with sum |terms|. Nothing here calls the library.
"""

import numpy as np

from tests import fp8_ref as F

MXB = 32
E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
EPS_FAST = 2.0 ** -7


def scale_bytes(amax, e2m1: bool) -> np.ndarray:
    """The e8m0 byte of a 32-block from its finite amax (float32)."""
    amax = np.asarray(amax, dtype=np.float32)
    m, e = np.frexp(amax)  # amax = m 2^e, m in [0.5, 1)
    if e2m1:
        e = e - np.where(m <= np.float32(0.75), 3, 2)
    else:
        e = e - np.where(m <= np.float32(0.875), 9, 8)
    e = np.where(amax == 0, -126, np.maximum(e, -126))
    return (e + 127).astype(np.uint8)


def e8m0(b) -> np.ndarray:
    """float64 value of e8m0 bytes (0xFF: NaN)."""
    b = np.asarray(b, dtype=np.uint8)
    return np.where(b == 0xFF, np.nan, np.exp2(b.astype(np.float64) - 127.0))


def encode_e2m1(v) -> np.ndarray:
    """rne_e2m1 codes of finite values with |v| <= 6: the nearest of the
    eight magnitudes, a tie to the even code (mantissa bit 0)."""
    v = np.asarray(v, dtype=np.float64)
    dist = np.abs(np.abs(v)[..., None] - E2M1)
    best = dist.min(axis=-1, keepdims=True)
    # (a tie is between neighbouring codes, one of them even)
    mag = np.where(dist == best, np.arange(8) + 8 * (np.arange(8) % 2),
                   99).min(axis=-1) % 8
    return mag.astype(np.uint8) | (np.signbit(v).astype(np.uint8) << 3)


def quantize(x, e2m1: bool = False):
    """x [rows, k] (values of T as float32) -> (codes uint8 [rows, k]: e4m3
    bytes or e2m1 codes, one per element; scales uint8 [rows, k / 32])."""
    x = np.asarray(x, dtype=np.float32)
    rows, k = x.shape
    blocks = x.reshape(rows, k // MXB, MXB)
    finite = np.isfinite(blocks)
    sb = scale_bytes(F.amax_finite(blocks, axis=2), e2m1)
    # x / s is exact: s is a power of two (float64 keeps every quotient)
    v = np.where(finite, blocks, 0).astype(np.float64) / e8m0(sb)[..., None]
    if e2m1:
        bad = ~finite.all(axis=2)
        q = np.where(bad[..., None], 0, encode_e2m1(v))
        sb = np.where(bad, 0xFF, sb)
    else:
        nan = (F.NAN_BYTE | (np.signbit(blocks).astype(np.uint8) << 7))
        with np.errstate(under="ignore"):
            q = np.where(finite, F.encode(v.astype(np.float32)), nan)
    return q.astype(np.uint8).reshape(rows, k), sb.astype(np.uint8)


def pack(codes) -> np.ndarray:
    """e2m1 codes [rows, k] -> bytes [rows, k / 2], element 2 i in bits 3:0."""
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).astype(np.uint8)


def decode(codes, scales, e2m1: bool = False) -> np.ndarray:
    """float64 values of codes [rows, k] under scales [rows, k / 32]."""
    codes = np.asarray(codes, dtype=np.uint8)
    if e2m1:
        v = np.where(codes & 8, -E2M1[codes & 7], E2M1[codes & 7])
    else:
        v = F.decode(codes)
    return v * np.repeat(e8m0(scales), MXB, axis=1)


def matmul64(a64, w64):
    """(a . w^T, sum |terms|) for a [m, k] and w [n, k], float64."""
    return a64 @ w64.T, np.abs(a64) @ np.abs(w64).T


def bound(ref64, absum, k: int, dtype: str) -> np.ndarray:
    """mx.h: 2^-p |exact| + (eps_fast + (K / 128 + 1) 2^-23) sum |terms|."""
    p = 11 if dtype == "f16" else 8
    return (2.0 ** -p * np.abs(ref64)
            + (EPS_FAST + (k // 128 + 1) * 2.0 ** -23) * absum)


def expand_block_scales(m, k, offsets, indices, s_blocks) -> np.ndarray:
    """Scales [nnz_blocks * 128, 4] of stored blocks -> [m, k / 32] (2^0 where
    nothing is stored)."""
    out = np.full((m, k // MXB), 127, np.uint8)
    rows = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    for b, (r, c) in enumerate(zip(rows, indices)):
        out[r * 128:(r + 1) * 128, 4 * c:4 * c + 4] = \
            s_blocks[b * 128:(b + 1) * 128]
    return out
