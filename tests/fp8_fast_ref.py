"""Host side of the tests of the fp8 products' fast accumulation
(sputnik/block/fp8.h, Fp8Accumulate::kFast), shared by
tests/test_fp8_fast_host.py, tests/test_gpu_fp8_fast*.py and
scripts/probe_fp8_accum.py. Nothing here calls the library.

In kFast the interval sum P is defined by the hardware
(v_mfma_scale_f32_16x16x128_f8f6f4), and there is no CPU model of it. The
tests therefore take P from Fp8IntervalSums, the contract's definition of P as
a callable, and hold the product kernels to

    from_interval_sums   acc = fma32(float32(sa * sw), P[kb], acc) per
                         interval in the contract's order, then round_T: the
                         arithmetic around P, from fp8_ref.fma32 / round_t

bit for bit; Fp8IntervalSums itself is held to the float64 dot products of
the decoded bytes within EPS_FAST of sum |products|:

    EPS_FAST             the measured eps_fast of fp8.h: the smallest power
                         of two at or above twice the worst |P - exact| /
                         sum |products| seen over `families` (the worst was
                         2^-8.24; profiles/fp8/accum_probe.jsonl)
    bound_fast           |C - exact| <= 2^-p |exact| + (EPS_FAST + (2 K / 128
                         + 1) 2^-23) sum |terms|: one rounding to T, EPS_FAST
                         of every interval's sum |products|, and per interval
                         one rounding of the scale product and one of the
                         fma, plus one to spare
    families             the seeded operand families of the measurement
"""

from __future__ import annotations

import numpy as np

from tests import fp8_ref as R
from tests.moe_ref import P_BITS

B = R.B
EPS_FAST = 2.0 ** -7


def bound_fast(ref64, absum, k: int, dtype: str) -> np.ndarray:
    return (2.0 ** -P_BITS[dtype] * np.abs(ref64)
            + (EPS_FAST + (2 * k // B + 1) * 2.0 ** -23) * absum)


def from_interval_sums(p, sa, sw, order=None, dtype=None) -> np.ndarray:
    """round_T of the chain over the interval sums p [k / 128, m, n]
    (float32): per block row the k-blocks ascending or as `order` lists
    them, s = float32(sa * sw), acc = fma32(s, p[kb], acc); sa [m, k / 128],
    sw [k / 128, n / 128]. float32 [m, n]; with dtype None the accumulator
    itself."""
    p = np.asarray(p, np.float32)
    steps_all, m, n = p.shape
    sa = np.asarray(sa, np.float32)
    sw = np.asarray(sw, np.float32)
    acc = np.zeros((m, n), np.float32)
    for rb in range(m // B):
        rows = slice(rb * B, (rb + 1) * B)
        for kb in (range(steps_all) if order is None else order[rb]):
            with np.errstate(invalid="ignore", over="ignore"):
                s = sa[rows, kb:kb + 1] * np.repeat(sw[kb], B)[None, :]
                acc[rows] = R.fma32(s, p[kb, rows], acc[rows])
    return acc if dtype is None else R.round_t(acc, dtype)


# ---- the operand families of the eps_fast measurement ---------------------------
#
# Each is (aq [m, k] bytes, bq [n, k] bytes), finite, every dimension a
# multiple of 128.

FINITE_BYTES = np.array([b for b in range(256) if (b & 0x7F) != 0x7F],
                        np.uint8)
LARGE = 256.0                       # the large entry of A in (c) and (d)
SMALL_EXPONENTS = range(-7, 10)     # a: the other entries of A are 2^-a
COLUMN_EXPONENTS = range(-9, 9)     # e: B's column j holds +-2^e


def lane_group(t):
    """The lane group (l / 16) whose 32 operand bytes hold position t of an
    interval: k = 16 g .. 16 g + 15 and 64 + 16 g .. 64 + 16 g + 15."""
    return (np.asarray(t) % 64) // 16


def _constant_columns(n: int = B) -> np.ndarray:
    """bq [n, 128]: row j is the constant +-2^e, (e, sign) cycling."""
    combos = [(e, s) for e in COLUMN_EXPONENTS for s in (1.0, -1.0)]
    col = np.array([R.byte_of(s * 2.0 ** e)
                    for e, s in (combos[j % len(combos)] for j in range(n))],
                   np.uint8)
    assert n >= len(combos)
    return np.repeat(col[:, None], B, axis=1)


def _large_among_small(second=None) -> np.ndarray:
    """aq [17 * 128, 128]: row (a, t) holds LARGE at position t and 2^-a
    elsewhere; with `second` ("same": the same lane group, the other 16-byte
    read; "other": the next lane group) a -LARGE at a second position."""
    rows = []
    for a in SMALL_EXPONENTS:
        block = np.full((B, B), R.byte_of(2.0 ** -a), np.uint8)
        t = np.arange(B)
        block[t, t] = R.byte_of(LARGE)
        if second is not None:
            t2 = (t + (64 if second == "same" else 16)) % B
            assert ((lane_group(t2) == lane_group(t)).all() if second == "same"
                    else (lane_group(t2) != lane_group(t)).all())
            block[t, t2] = R.byte_of(-LARGE)
        rows.append(block)
    return np.concatenate(rows)


def families():
    """name -> (aq, bq) of the four families of fp8.h's measurement."""
    from tests.moe_ref import values

    rng = np.random.default_rng([61, 1])
    m, n, k = 256, 384, 5 * B
    random_bytes = (FINITE_BYTES[rng.integers(0, len(FINITE_BYTES), (m, k))],
                    FINITE_BYTES[rng.integers(0, len(FINITE_BYTES), (n, k))])
    aq, _ = R.quantize_rows(values((m, k), "bf16", [61, 2]))
    bq, _ = R.quantize_weight(values((k, n), "bf16", [61, 3]))
    columns = _constant_columns()
    return {
        "random_bytes": random_bytes,
        "quantised_normal": (aq, bq),
        "large_among_small": (_large_among_small(), columns),
        "cancelling_large": (np.concatenate([_large_among_small("same"),
                                             _large_among_small("other")]),
                             columns),
    }


def exact_sums(aq, bq):
    """(exact, sum |products|) per interval, float64 [k / 128, m, n], of
    finite bytes: every product is a multiple of 2^-18 below 2^18 and a
    128-term sum of them is exact in float64."""
    a, b = R.decode(aq), R.decode(bq)
    steps = a.shape[1] // B
    exact = np.stack([a[:, i * B:(i + 1) * B] @ b[:, i * B:(i + 1) * B].T
                      for i in range(steps)])
    absum = np.stack([np.abs(a[:, i * B:(i + 1) * B])
                      @ np.abs(b[:, i * B:(i + 1) * B]).T
                      for i in range(steps)])
    return exact, absum


def worst_ratio(p, aq, bq) -> float:
    """max |p - exact| / sum |products| over every output of every interval
    (an all-zero dot product must be +-0)."""
    exact, absum = exact_sums(aq, bq)
    err = np.abs(np.asarray(p, np.float64) - exact)
    assert np.isfinite(err).all()
    assert (err[absum == 0] == 0).all()
    return float((err / np.where(absum == 0, 1.0, absum)).max())
