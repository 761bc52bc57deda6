"""Numpy references of the expert biases (sputnik/block/bias.h and the
PaddedScatterBias calls of moe.h), shared by tests/test_bias_host.py and
tests/test_gpu_bias*.py. Nothing here calls the library.

    bias_stage     xb = round_T((float32(x) + float32(b[col])) + 0) over
                   block data [nb, 128, 128] with its column indices
    column_sum64   the exact float64 column sums of a block matrix and
                   sum |.|, with the number of rows summed per column
    scatter32      the scatter with bias as the kernel computes it: a float32
                   add, a float32 multiply (omitted without weights), a
                   float32 accumulate per k from 0, one rounding to T
    scatter64      the exact float64 scatter and sum_k |w| (|y| + |b|)
    wgrad64        the exact weight gradient and sum_h |dout| (|y| + |b|)
    bgrad64        the exact bias gradient, sum |w dout| and the counts n_e

Values of type T ("f16" / "bf16", oracle.round_to's names) travel as float32
arrays that hold only representable values. The routing cases, shapes and
operands are moe_ref's (CASES, HIDDEN, case_inputs); the bias of a case is
made here, so the CPU self-checks run on the very inputs the GPU tests use.
"""

from __future__ import annotations

import functools

import numpy as np

from oracle import oracle as O
from tests import moe_ref as M

B = 128
P_BITS = M.P_BITS

# moe_ref.CASES x these, plus one long row and one large top_k: what the
# scatter tests run.
HIDDEN = [8, 264, 100]
LONG_CASE = ((129, 2, 4, "empty"), 4096)
DEEP_CASE = M.DEEP_CASE


# ---- the bias stage ---------------------------------------------------------

def column_bias(cols: int, dtype: str = "f16") -> np.ndarray:
    """A distinct value of T per logical column: (c - cols / 2) / 8. Exact in
    fp16 for |c - cols/2| <= 2^11 and in bf16 for |c - cols/2| <= 2^8; past
    that, rounded (still monotone, distinct per block position)."""
    c = np.arange(cols, dtype=np.float32)
    return O.round_to((c - cols // 2) / 8.0, dtype)


def bias_stage(x_blocks: np.ndarray, indices, bias: np.ndarray,
               dtype: str) -> np.ndarray:
    """x_blocks [nb, 128, 128] (values of T), block b at block column
    indices[b]; returns round_T((x + bias[col]) + 0) in float32."""
    x = np.asarray(x_blocks, dtype=np.float32)
    idx = np.asarray(indices, dtype=np.int64)
    cols = idx[:, None] * B + np.arange(B)[None, :]            # [nb, 128]
    b = np.asarray(bias, dtype=np.float32)[cols][:, None, :]   # [nb, 1, 128]
    s = (x + b).astype(np.float32)
    s = (s + np.float32(0.0)).astype(np.float32)
    return O.round_to(s, dtype)


# ---- column sums ------------------------------------------------------------

def column_sum64(blocks: np.ndarray, indices, cols: int):
    """(sum, sum |.|, rows summed), float64 / float64 / int64 [cols]."""
    x = np.asarray(blocks, dtype=np.float64)
    s = np.zeros(cols)
    a = np.zeros(cols)
    n = np.zeros(cols, dtype=np.int64)
    for b, c in enumerate(np.asarray(indices, dtype=np.int64)):
        s[c * B:(c + 1) * B] += x[b].sum(axis=0)
        a[c * B:(c + 1) * B] += np.abs(x[b]).sum(axis=0)
        n[c * B:(c + 1) * B] += B
    return s, a, n


def column_sum32(blocks: np.ndarray, indices, cols: int) -> np.ndarray:
    """Column sums accumulated in float32 (one of the orders a kernel is free
    to take: row after row, block after block)."""
    x = np.asarray(blocks, dtype=np.float32)
    s = np.zeros(cols, dtype=np.float32)
    for b, c in enumerate(np.asarray(indices, dtype=np.int64)):
        for r in range(B):
            s[c * B:(c + 1) * B] += x[b, r]
    return s


def column_sum_bound(ref64, absum, n) -> np.ndarray:
    """One rounding of the exact sum to fp32 plus an fp32 accumulation of n
    terms in any order."""
    return 2.0 ** -24 * np.abs(ref64) + n * 2.0 ** -24 * absum


# ---- the scatter with an output bias ----------------------------------------

def row_expert(r: M.Route, rows: int) -> np.ndarray:
    """Per assignment: the expert read off its row (#{e : padded_bins[e] <=
    row}), or -1 where the row is outside [0, rows) or owned by no expert."""
    row = r.row_of.astype(np.int64)
    e = np.searchsorted(r.padded_bins, row, side="right")
    ok = (row >= 0) & (row < rows) & (e < r.padded_bins.size)
    return np.where(ok, e, -1)


def _terms(y, b2, r: M.Route, dt):
    """(y[row_k], b2[e_k], ok) as [tokens, top_k, hidden] / [tokens, top_k]."""
    y = np.asarray(y, dtype=dt)
    e = row_expert(r, y.shape[0]).reshape(r.tokens, r.top_k)
    ok = e >= 0
    rows = np.where(ok, r.row_of.reshape(r.tokens, r.top_k), 0)
    yk = np.where(ok[:, :, None], y[rows], 0)
    bk = np.where(ok[:, :, None], np.asarray(b2, dtype=dt)[np.where(ok, e, 0)],
                  0)
    return yk.astype(dt), bk.astype(dt), ok


def scatter32(y, b2, r: M.Route, weights=None, dtype: str = "f16"):
    yk, bk, ok = _terms(y, b2, r, np.float32)
    w = (None if weights is None else
         np.asarray(weights, dtype=np.float32).reshape(r.tokens, r.top_k))
    acc = np.zeros((r.tokens, yk.shape[2]), dtype=np.float32)
    for k in range(r.top_k):
        p = (yk[:, k] + bk[:, k]).astype(np.float32)
        if w is not None:
            wk = np.where(ok[:, k], w[:, k], np.float32(1.0))
            p = (wk[:, None].astype(np.float32) * p).astype(np.float32)
        acc = (acc + p).astype(np.float32)
    return O.round_to(acc, dtype)


def scatter64(y, b2, r: M.Route, weights=None):
    """(exact sum, sum_k |w| (|y| + |b|)), float64 [tokens, hidden]."""
    yk, bk, ok = _terms(y, b2, r, np.float64)
    w = (np.ones((r.tokens, r.top_k)) if weights is None else
         np.asarray(weights, dtype=np.float64).reshape(r.tokens, r.top_k))
    w = np.where(ok, w, 0.0)[:, :, None]
    return ((w * (yk + bk)).sum(axis=1),
            (np.abs(w) * (np.abs(yk) + np.abs(bk))).sum(axis=1))


# Half of T's subnormal spacing: what a round-to-nearest result is off by at
# most where the exact value lies below T's smallest normal number (fp16:
# 2^-14), whatever its size. Weights of T in (0, 1] can be small enough to
# take a product of normal numbers there, so the relative term alone is not
# a bound that a correctly rounded result meets.
SUBNORMAL_HALF_STEP = {"f16": 2.0 ** -25, "bf16": 2.0 ** -134}


def scatter_bound(ref64, absum, top_k: int, dtype: str) -> np.ndarray:
    """One rounding to T of the exact sum (relative 2^-P, or half a
    subnormal step where that is larger); per k one add, one multiply and
    one accumulate in fp32 (top_k + 2 covers the partial sums' growth)."""
    return (np.maximum(2.0 ** -P_BITS[dtype] * np.abs(ref64),
                       SUBNORMAL_HALF_STEP[dtype])
            + (top_k + 2) * 2.0 ** -23 * absum)


def wgrad64(dout, y, b2, r: M.Route):
    """(exact dw, sum_h |dout| (|y| + |b|)), float64 [n]."""
    yk, bk, _ = _terms(y, b2, r, np.float64)
    d = np.asarray(dout, dtype=np.float64)[:, None, :]
    return ((d * (yk + bk)).sum(axis=2).reshape(-1),
            (np.abs(d) * (np.abs(yk) + np.abs(bk))).sum(axis=2).reshape(-1))


def wgrad32(dout, y, b2, r: M.Route) -> np.ndarray:
    yk, bk, _ = _terms(y, b2, r, np.float32)
    d = np.asarray(dout, dtype=np.float32)[:, None, :]
    return (d * (yk + bk).astype(np.float32)).sum(
        axis=2, dtype=np.float32).reshape(-1)


def bgrad64(dout, r: M.Route, num_experts: int, weights=None):
    """(exact db2, sum |w dout|, n_e): float64 [E, hidden] twice, int64 [E]."""
    d = np.asarray(dout, dtype=np.float64)
    n = r.indices.size
    w = (np.ones(n) if weights is None else
         np.asarray(weights, dtype=np.float64).reshape(-1))
    db = np.zeros((num_experts, d.shape[1]))
    ab = np.zeros_like(db)
    cnt = np.zeros(num_experts, dtype=np.int64)
    b0 = 0
    for e in range(num_experts):
        b1 = int(r.bins[e])
        a = r.indices[b0:b1].astype(np.int64)
        p = w[a][:, None] * d[a // r.top_k]
        db[e] = p.sum(axis=0)
        ab[e] = np.abs(p).sum(axis=0)
        cnt[e] = b1 - b0
        b0 = b1
    return db, ab, cnt


def bgrad32(dout, r: M.Route, num_experts: int, weights=None) -> np.ndarray:
    """db2 accumulated in float32 in sorted order (one order a kernel may
    take)."""
    d = np.asarray(dout, dtype=np.float32)
    n = r.indices.size
    w = (np.ones(n, dtype=np.float32) if weights is None else
         np.asarray(weights, dtype=np.float32).reshape(-1))
    db = np.zeros((num_experts, d.shape[1]), dtype=np.float32)
    b0 = 0
    for e in range(num_experts):
        b1 = int(r.bins[e])
        for i in range(b0, b1):
            a = int(r.indices[i])
            db[e] += (w[a] * d[a // r.top_k]).astype(np.float32)
        b0 = b1
    return db


def bgrad_bound(ref64, absum, counts) -> np.ndarray:
    """One rounding of the exact sum to fp32; n_e products, each rounded
    once, accumulated in fp32 in any order."""
    n = np.asarray(counts, dtype=np.float64)[:, None]
    return 2.0 ** -24 * np.abs(ref64) + (n + 1) * 2.0 ** -24 * absum


# ---- inputs -----------------------------------------------------------------

def scatter_cases():
    """(case, hidden) pairs of the scatter tests."""
    return ([(c, h) for c in M.CASES for h in HIDDEN]
            + [LONG_CASE, DEEP_CASE])


@functools.lru_cache(maxsize=None)
def case_bias(case, hidden: int, dtype: str) -> np.ndarray:
    """b2 [E, hidden] of T for one case, computed once and never modified.
    |b2| with one sign per column, the signs moe_ref gives y_cols, so that
    with y_cols no sum cancels (scatter_bound has no term for T's subnormal
    range; moe_ref.case_inputs)."""
    tokens, top_k, e, _ = case
    seed = [tokens, top_k, e, hidden, M.DTYPES.index(dtype)]
    b = np.abs(M.values((e, hidden), dtype, seed + [7]))
    inp = M.case_inputs(case, hidden, dtype)
    sign = np.sign(inp.y_cols[0]).astype(np.float32)
    sign[sign == 0] = 1.0
    out = (b * sign).astype(np.float32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case_bias_abs(case, hidden: int, dtype: str) -> np.ndarray:
    """|b2|, for the weight-gradient test against moe_ref's y_rows and
    dout_abs: with a positive bias the terms of a row with positive sign add
    up; rows of negative sign may cancel against the bias, which wgrad_bound
    covers through its absolute sum (the result is fp32 or rounded to T from
    a value that is not subnormal for these magnitudes)."""
    out = np.abs(case_bias(case, hidden, dtype))
    out.setflags(write=False)
    return out
