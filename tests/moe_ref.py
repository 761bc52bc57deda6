"""Numpy references of the MoE token permutation (sputnik/block/moe.h), shared
by tests/test_moe_host.py and tests/test_gpu_moe*.py. Nothing here calls the
library.

    route        MegaBlocks' indices_and_padded_bins order from top_experts:
                 np.argsort(kind="stable") plus cumsums, and row_of
    gather       the padded matrix (float32 values of type T), +0 elsewhere
    scatter32    the scatter as the kernel computes it: a float32 multiply,
                 float32 adds from 0 in ascending k, one rounding to T
    scatter64    the exact float64 scatter and sum_k |w y|
    wgrad64      the exact float64 weight gradient and sum_h |dout y|

Values of type T ("f16" / "bf16", oracle.round_to's names) travel as float32
arrays that hold only representable values.

The test shapes live here too, so that the CPU self-checks run on the very
cases and seeds the GPU tests use: CASES are (tokens, top_k, E, routing) at
the smallest sizes where the kernels can still go wrong, HIDDEN the row
lengths (8: one 16-byte piece; 264: no multiple of a wave's 512-element
step; 100: the element path; 4096: several steps per row).
"""

from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

from oracle import oracle as O

Route = namedtuple("Route", "indices bin_ids bins padded_bins "
                            "tokens_per_expert row_of top_k tokens")

# _ROUND_U of tests/helpers.py as exponents, plus fp32 for fp32 weights.
P_BITS = {"bf16": 8, "f16": 11, "f32": 24}

# routing: "random"; "empty" (one expert gets nothing); "exact" (expert 0
# gets exactly 128 assignments, expert 1 exactly 129); "one" (everything on
# the last expert).
CASES = [
    (1, 1, 1, "one"),
    (1, 4, 4, "random"),
    (129, 1, 1, "one"),
    (129, 2, 4, "empty"),
    (129, 4, 8, "random"),
    (300, 1, 8, "exact"),
    (300, 2, 4, "exact"),
    (300, 4, 8, "one"),
]
HIDDEN = [8, 264, 100, 4096]
DTYPES = ["f16", "bf16"]
# (case, hidden) with top_k past the 4 picks the scatter kernel looks up in
# front of its piece loop: 37 tokens leave one live row in the last 4-row
# task, and 264 is a partial last step on the 16-byte path.
DEEP_CASE = ((37, 6, 8, "random"), 264)


def scatter_cases():
    """(case, hidden) pairs of the scatter and weight-gradient tests."""
    return [(c, h) for c in CASES for h in HIDDEN] + [DEEP_CASE]


def scatter_hiddens(case):
    """The row lengths at which scatter_cases() runs `case`."""
    return [h for c, h in scatter_cases() if c == case]


def rows_bound(n: int, num_experts: int) -> int:
    return -(-(n + 127 * num_experts) // 128) * 128


def routing(tokens: int, top_k: int, num_experts: int, kind: str,
            seed: int = 0) -> np.ndarray:
    """top_experts [tokens, top_k] (int64) of one of the routing kinds."""
    rng = np.random.default_rng([seed, tokens, top_k, num_experts])
    n, e = tokens * top_k, num_experts
    if kind == "random":
        flat = rng.integers(0, e, n)
    elif kind == "empty":
        skip = int(rng.integers(0, e))
        flat = rng.integers(0, e - 1, n)
        flat[flat >= skip] += 1
    elif kind == "exact":
        assert n >= 257 and e >= 3
        flat = np.concatenate([np.zeros(128, np.int64), np.ones(129, np.int64),
                               rng.integers(2, e, n - 257)])
        rng.shuffle(flat)
    elif kind == "one":
        flat = np.full(n, e - 1)
    else:
        raise ValueError(kind)
    return flat.astype(np.int64).reshape(tokens, top_k)


def route(top_experts: np.ndarray, num_experts: int) -> Route:
    top_experts = np.asarray(top_experts)
    tokens = top_experts.shape[0]
    top_k = top_experts.shape[1] if top_experts.ndim == 2 else 1
    flat = top_experts.reshape(-1)
    indices = np.argsort(flat, kind="stable")
    bin_ids = flat[indices]
    tpe = np.bincount(flat, minlength=num_experts)
    bins = np.cumsum(tpe)
    padded = np.cumsum((tpe + 127) // 128 * 128)
    bin0 = np.concatenate([[0], bins[:-1]])
    pad0 = np.concatenate([[0], padded[:-1]])
    row = pad0[bin_ids] + (np.arange(flat.size) - bin0[bin_ids])
    row_of = np.empty(flat.size, dtype=np.int64)
    row_of[indices] = row
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
    return Route(i32(indices), i32(bin_ids), i32(bins), i32(padded), i32(tpe),
                 i32(row_of), top_k, tokens)


def exact_rows(r: Route) -> int:
    return int(r.padded_bins[-1]) if r.padded_bins.size else 0


def gather(x: np.ndarray, r: Route, rows: int, weights=None,
           dtype: str = "f16") -> np.ndarray:
    """x [tokens, hidden] (values of T) -> [rows, hidden]; with weights
    round_T(float32(w[a]) * x[a / top_k]) (exact in float32 for w of T)."""
    x = np.asarray(x, dtype=np.float32)
    out = np.zeros((rows, x.shape[1]), dtype=np.float32)
    src = x[np.arange(r.row_of.size) // r.top_k]
    if weights is not None:
        w = np.asarray(weights, dtype=np.float32).reshape(-1, 1)
        src = O.round_to(w * src, dtype)
    out[r.row_of] = src
    return out


def scatter32(y: np.ndarray, r: Route, weights=None,
              dtype: str = "f16") -> np.ndarray:
    y = np.asarray(y, dtype=np.float32)
    rows = r.row_of.reshape(r.tokens, r.top_k)
    acc = np.zeros((r.tokens, y.shape[1]), dtype=np.float32)
    w = (None if weights is None else
         np.asarray(weights, dtype=np.float32).reshape(r.tokens, r.top_k))
    for k in range(r.top_k):
        p = y[rows[:, k]]
        if w is not None:
            p = (w[:, k:k + 1] * p).astype(np.float32)
        acc = (acc + p).astype(np.float32)
    return O.round_to(acc, dtype)


def scatter64(y: np.ndarray, r: Route, weights=None):
    """(exact sum, sum_k |w y|), both float64 [tokens, hidden]."""
    y = np.asarray(y, dtype=np.float64)
    rows = r.row_of.reshape(r.tokens, r.top_k)
    w = (np.ones((r.tokens, r.top_k)) if weights is None else
         np.asarray(weights, dtype=np.float64).reshape(r.tokens, r.top_k))
    p = w[:, :, None] * y[rows]
    return p.sum(axis=1), np.abs(p).sum(axis=1)


def wgrad64(dout: np.ndarray, y: np.ndarray, r: Route):
    """(exact dw, sum_h |dout y|), both float64 [n]."""
    d = np.asarray(dout, dtype=np.float64)[np.arange(r.row_of.size) // r.top_k]
    p = d * np.asarray(y, dtype=np.float64)[r.row_of]
    return p.sum(axis=1), np.abs(p).sum(axis=1)


def wgrad32(dout: np.ndarray, y: np.ndarray, r: Route) -> np.ndarray:
    """The weight gradient accumulated in float32 (one of the orders the
    kernel is free to take), not yet rounded to the output type."""
    d = np.asarray(dout, dtype=np.float32)[np.arange(r.row_of.size) // r.top_k]
    return (d * np.asarray(y, dtype=np.float32)[r.row_of]).sum(
        axis=1, dtype=np.float32)


def scatter_bound(ref64, absum, top_k: int, dtype: str) -> np.ndarray:
    """One rounding to T of the exact sum plus the fp32 accumulation."""
    return (2.0 ** -P_BITS[dtype] * np.abs(ref64)
            + top_k * 2.0 ** -23 * absum)


def wgrad_bound(ref64, absum, hidden: int, out_type: str) -> np.ndarray:
    return (2.0 ** -P_BITS[out_type] * np.abs(ref64)
            + hidden * 2.0 ** -24 * absum)


# ---- inputs -----------------------------------------------------------------

def values(shape, dtype: str, seed) -> np.ndarray:
    """Values of T with magnitudes in [2^-10, 4] and random signs."""
    rng = np.random.default_rng(seed)
    mag = np.exp2(rng.uniform(-10.0, 2.0, shape))
    sign = np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    # (both ends are representable and rounding is monotone: it keeps them)
    return O.round_to((mag * sign).astype(np.float32), dtype)


def unit_weights(n: int, dtype: str, seed) -> np.ndarray:
    """Weights of T in (0, 1]; for "f32", float32 weights in [1/8, 1]."""
    u = np.random.default_rng(seed).random(n)
    if dtype == "f32":
        return (1.0 - 0.875 * u).astype(np.float32)
    return O.round_to((1.0 - u).astype(np.float32), dtype)


@functools.lru_cache(maxsize=None)
def case_route(case) -> Route:
    tokens, top_k, e, kind = case
    return route(routing(tokens, top_k, e, kind), e)


Inputs = namedtuple("Inputs", "route x y dout w w32 y_cols y_rows dout_abs")


@functools.lru_cache(maxsize=None)
def case_inputs(case, hidden: int, dtype: str) -> Inputs:
    """The operands of one test case, computed once and never modified:
    x, dout [tokens, hidden] and y [bound rows, hidden] of T with random
    signs, w [n] of T, w32 [n] of float32. y's rows past the exact row count
    are there for the runs that size the padded matrix by rows_bound.

    y_cols, y_rows and dout_abs are for the two tests with a bound relative
    to the exact result (scatter_bound, wgrad_bound). Those bounds have no
    term for T's subnormal range, where a correctly rounded fp16 result is
    off by up to 2^-25 whatever its size, so their operands are signed so
    that no sum cancels: y_cols is |y| with one sign per column (a token's
    top_k rows add up: |sum| >= 2^-3 * 2^-10, a normal fp16 number), y_rows
    is |y| with one sign per row against dout_abs = |dout| (a dot product's
    terms add up; both signs of dw occur). test_moe_host.py checks that the
    float32 emulation meets both bounds on exactly these operands."""
    tokens, top_k, e, _ = case
    r = case_route(case)
    n = tokens * top_k
    seed = [tokens, top_k, e, hidden, DTYPES.index(dtype)]
    x = values((tokens, hidden), dtype, seed + [1])
    y = values((rows_bound(n, e), hidden), dtype, seed + [2])
    dout = values((tokens, hidden), dtype, seed + [3])
    rng = np.random.default_rng(seed + [6])
    col = np.where(rng.random(hidden) < 0.5, -1, 1).astype(np.float32)
    row = np.where(rng.random((y.shape[0], 1)) < 0.5, -1, 1).astype(np.float32)
    out = Inputs(r, x, y, dout, unit_weights(n, dtype, seed + [4]),
                 unit_weights(n, "f32", seed + [5]), np.abs(y) * col,
                 np.abs(y) * row, np.abs(dout))
    for a in out[1:]:
        a.setflags(write=False)
    return out
