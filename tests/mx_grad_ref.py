"""Host reference of the MX gradient pieces of sputnik/block/mx.h (numpy only),
on tests/mx_ref.py: the column quantisation is the row quantisation of the
transpose, and the bound is mx_ref.bound extended by the `add` term."""

import numpy as np

from tests import mx_ref as R
from tests.moe_ref import P_BITS


def quantize_cols(x):
    """x [rows, cols] -> (qt uint8 [cols, rows], scales_t uint8 [cols, rows /
    32]): one e8m0 byte per column and 32 consecutive rows."""
    return R.quantize(np.ascontiguousarray(np.asarray(x, np.float32).T))


def quantize_blocks_t(values, block_offsets):
    """Block values [nb, 128, 128] -> (qt uint8 [nb, 128, 128], scales_t uint8
    [nb * 128, 4]): output block j is source block block_offsets[j] stored
    [column][row], scales_t[128 j + c] the four bytes of source column c."""
    t = np.asarray(values, np.float32)[np.asarray(block_offsets)]
    q, s = R.quantize(t.transpose(0, 2, 1).reshape(-1, 128))
    return q.reshape(-1, 128, 128), s


def bound(ref64, absum, k, out: str, add: bool = False) -> np.ndarray:
    """mx.h, DsdMxWgrad: 2^-p |exact| (absent for fp32 output) + (eps_fast +
    (K / 128 + 1 + add) 2^-23) sum |terms|."""
    lead = 0.0 if out == "f32" else 2.0 ** -P_BITS[out] * np.abs(ref64)
    return lead + (R.EPS_FAST + (k // 128 + 1 + int(add)) * 2.0 ** -23) * absum
