"""Numpy references of the MoE router and the device sort
(sputnik/block/router.h), shared by tests/test_router_host.py and
tests/test_gpu_router*.py. Nothing here calls the library.

    expected_ids   the k picks: np.argsort(-l, kind="stable")[:, :k] (the
                   largest first, ties to the lower index, NaN last)
    forward64      float64 weights and scores for given picks
    forward32      the same in float32 arithmetic, rounded once to the
                   output type: the emulation the bounds were derived for
    grad64         float64 dlogits and the absolute-value image
                   p_j (a_j + sum_i a_i p_i) its bound is relative to
    grad32         the gradient in float32 arithmetic, rounded once
    sort_ref       the routing tensors MoeSort must produce, ids outside
                   [0, E) included (moe_ref.route covers the valid ids)

Values of a type ("f16" / "bf16" / "f32") travel as float32 arrays that hold
only representable values. The test cases live here too, so that the CPU
self-checks run on the very inputs the GPU tests use; every input is computed
once, cached and read-only.
"""

from __future__ import annotations

import functools

import numpy as np

from oracle import oracle as O
from tests import moe_ref

P_BITS = moe_ref.P_BITS            # {"bf16": 8, "f16": 11, "f32": 24}
LTYPES = ["f16", "bf16", "f32"]
CHUNK = 1024                       # sputnik::block::kMoeSortChunk

# (tokens, E, top_k): one lane in use; k = E; E = one wave; E one past a
# wave; small E with many tokens; every template width (1, 2, 4, 16 waves of
# experts; 8 below); k at its limit.
ROUTER_CASES = [
    (1, 1, 1), (1, 4, 4), (5, 64, 2), (129, 65, 8), (67, 8, 2), (33, 256, 8),
    (9, 1024, 32), (300, 8, 2),
    (3, 500, 7),     # (added: the 8-register width, 256 < E <= 512)
]
KINDS = ["random", "ties", "equal", "special"]


def rnd(x, t: str) -> np.ndarray:
    x = np.asarray(x, dtype=np.float32)
    return x if t == "f32" else O.round_to(x, t)


@functools.lru_cache(maxsize=None)
def logits(case, kind: str, ltype: str) -> np.ndarray:
    """[tokens, E] float32 holding values of `ltype`."""
    tokens, e, k = case
    rng = np.random.default_rng([tokens, e, k, KINDS.index(kind),
                                 LTYPES.index(ltype)])
    if kind == "equal":
        l = np.full((tokens, e), 0.75, dtype=np.float32)
    elif kind == "ties":
        # a < k entries at 3, then enough at 0.25 to hold the k-th and the
        # (k+1)-th largest, the rest at -2, in random places
        l = np.empty((tokens, e), dtype=np.float32)
        for r in range(tokens):
            a = int(rng.integers(0, k))
            b = int(rng.integers(min(k + 1, e) - a, e - a + 1))
            l[r] = rng.permutation(np.array(
                [3.0] * a + [0.25] * b + [-2.0] * (e - a - b), np.float32))
    else:
        l = rnd(rng.uniform(-8.0, 8.0, (tokens, e)).astype(np.float32), ltype)
    if kind == "special":
        l = l.copy()
        for r in range(tokens):
            u = rng.random(e)
            which = (r + e) % 4
            if which == 0:                      # some NaN
                l[r, u < 0.3] = np.nan
                l[r, rng.integers(e)] = np.nan
            elif which == 1:                    # +inf and -inf
                l[r, u < 0.25] = np.inf
                l[r, u > 0.75] = -np.inf
            elif which == 2:                    # only -inf
                l[r, :] = -np.inf
            else:                               # everything at once
                l[r, u < 0.2] = np.nan
                l[r, (u >= 0.2) & (u < 0.4)] = -np.inf
                l[r, (u >= 0.4) & (u < 0.6)] = 0.0
                l[r, (u >= 0.6) & (u < 0.8)] = -0.0
    l = np.ascontiguousarray(l, dtype=np.float32)
    l.setflags(write=False)
    return l


def expected_ids(l: np.ndarray, k: int) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return np.argsort(-l, axis=1, kind="stable")[:, :k].astype(np.int32)


def softmax64(l: np.ndarray) -> np.ndarray:
    l = np.asarray(l, dtype=np.float64)
    ex = np.exp(l - l.max(axis=1, keepdims=True))
    return ex / ex.sum(axis=1, keepdims=True)


def forward64(l, ids, normalize: bool):
    """(weights [tokens, k], scores [tokens, E]) in float64."""
    p = softmax64(l)
    w = np.take_along_axis(p, ids.astype(np.int64), axis=1)
    if normalize:
        w = w / w.sum(axis=1, keepdims=True)
    return w, p


def _softmax32(l):
    l = np.asarray(l, dtype=np.float32)
    ex = np.exp((l - l.max(axis=1, keepdims=True)).astype(np.float32))
    ex = ex.astype(np.float32)
    return (ex / ex.sum(axis=1, keepdims=True, dtype=np.float32)).astype(
        np.float32)


def forward32(l, ids, normalize: bool, out_type: str):
    p = _softmax32(l)
    w = np.take_along_axis(p, ids.astype(np.int64), axis=1)
    if normalize:
        w = (w / w.sum(axis=1, keepdims=True, dtype=np.float32)).astype(
            np.float32)
    return rnd(w, out_type), rnd(p, out_type)


def _sub(out_type: str) -> float:
    return 2.0 ** -25 if out_type == "f16" else 0.0


def weights_bound(ref, e: int, k: int, out_type: str) -> np.ndarray:
    return ((2.0 ** -P_BITS[out_type] + (e + k + 64) * 2.0 ** -24)
            * np.abs(ref) + _sub(out_type))


def scores_bound(ref, e: int, out_type: str) -> np.ndarray:
    return ((2.0 ** -P_BITS[out_type] + (e + 64) * 2.0 ** -24) * np.abs(ref)
            + _sub(out_type))


# ---- gradient ---------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def grad_ids(case, ltype: str) -> np.ndarray:
    """The picks of the "random" logits, except: row 0 slot 0 is E (out of
    range), row 1's last slot is -7 (out of range), and row 2's slot 1
    repeats its slot 0 (top_k >= 2)."""
    tokens, e, k = case
    ids = expected_ids(logits(case, "random", ltype), k).copy()
    ids[0, 0] = e
    if tokens >= 2:
        ids[1, k - 1] = -7
    if tokens >= 3 and k >= 2:
        ids[2, 1] = ids[2, 0]
    ids.setflags(write=False)
    return ids


@functools.lru_cache(maxsize=None)
def grad_inputs(case, ltype: str, wtype: str):
    """(dweights [tokens, k], dscores [tokens, E]) of `wtype` ("f32", or the
    logits' type), magnitudes in [2^-10, 4], random signs."""
    tokens, e, k = case
    seed = [tokens, e, k, LTYPES.index(ltype), wtype == "f32"]
    make = moe_ref.values if wtype != "f32" else (
        lambda shape, _t, s: moe_ref.values(shape, "f16", s))
    dw = make((tokens, k), wtype, seed + [1])
    ds = make((tokens, e), wtype, seed + [2])
    for a in (dw, ds):
        a.setflags(write=False)
    return dw, ds


def _dp(p, ids, dw, dscores, normalize, absolute, ft):
    """dp [tokens, E] in arithmetic of type `ft`; with `absolute` every term
    enters by its absolute value (the image the bound is relative to)."""
    tokens, e = p.shape
    k = ids.shape[1]
    dw = np.asarray(dw, dtype=ft)
    if absolute:
        dw = np.abs(dw)
    dp = (np.zeros((tokens, e), ft) if dscores is None
          else np.asarray(dscores, dtype=ft).copy())
    if absolute:
        dp = np.abs(dp)
    valid = (ids >= 0) & (ids < e)
    safe = np.where(valid, ids, 0).astype(np.int64)
    psel = np.where(valid, np.take_along_axis(p, safe, axis=1), 0).astype(ft)
    if normalize:
        with np.errstate(invalid="ignore", divide="ignore"):
            total = psel.sum(axis=1, keepdims=True, dtype=ft)
            c = ((dw * psel).sum(axis=1, keepdims=True, dtype=ft)
                 / total).astype(ft)
            g = ((dw + c) / total if absolute else (dw - c) / total).astype(ft)
    else:
        g = dw
    rows = np.arange(tokens)
    for j in range(k):          # one slot at a time: a repeated id adds twice
        v = valid[:, j]
        dp[rows[v], safe[v, j]] += g[v, j]
    return dp


def grad64(l, ids, dw, dscores, normalize: bool):
    """(dlogits, image), float64: image_j = p_j (a_j + sum_i a_i p_i)."""
    p = softmax64(l)
    dp = _dp(p, ids, dw, dscores, normalize, False, np.float64)
    a = _dp(p, ids, dw, dscores, normalize, True, np.float64)
    ref = p * (dp - (dp * p).sum(axis=1, keepdims=True))
    return ref, p * (a + (a * p).sum(axis=1, keepdims=True))


def grad32(l, ids, dw, dscores, normalize: bool, ltype: str) -> np.ndarray:
    p = _softmax32(l)
    dp = _dp(p, ids, dw, dscores, normalize, False, np.float32)
    dot = (dp * p).astype(np.float32).sum(axis=1, keepdims=True,
                                          dtype=np.float32)
    return rnd((p * (dp - dot).astype(np.float32)).astype(np.float32), ltype)


def grad_bound(ref, image, e: int, k: int, ltype: str) -> np.ndarray:
    return (2.0 ** -P_BITS[ltype] * np.abs(ref)
            + (2 * e + 2 * k + 128) * 2.0 ** -24 * image + _sub(ltype))


# ---- sort -------------------------------------------------------------------

SORT_N = [1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5]
SORT_E = [1, 8, 65, 1024]
SORT_CASES = [(n, e) for n in SORT_N for e in SORT_E]
OUT_OF_RANGE_CASE = (CHUNK + 70, 8)


@functools.lru_cache(maxsize=None)
def sort_ids(n: int, e: int) -> np.ndarray:
    ids = np.random.default_rng([n, e]).integers(0, e, n).astype(np.int32)
    ids.setflags(write=False)
    return ids


@functools.lru_cache(maxsize=None)
def out_of_range_ids() -> np.ndarray:
    n, e = OUT_OF_RANGE_CASE
    rng = np.random.default_rng(5)
    ids = rng.integers(0, e, n).astype(np.int32)
    bad = rng.choice(n, 40, replace=False)
    ids[bad] = rng.choice(np.array([-1, e, e + 5, -2 ** 31, 2 ** 31 - 1],
                                   np.int64), 40).astype(np.int32)
    ids[[0, CHUNK - 1, CHUNK, n - 1]] = [-1, e, 2 ** 31 - 1, -2 ** 31]
    ids.setflags(write=False)
    return ids


def sort_ref(flat: np.ndarray, e: int, rows: int) -> moe_ref.Route:
    """The routing tensors of router.h for any int32 ids: the ids in [0, E)
    in a stable sort, the others behind them in assignment order with bin id
    E, in no bin and with row_of = -1; a row at or past `rows` is -1."""
    flat = np.asarray(flat, dtype=np.int64).reshape(-1)
    valid = (flat >= 0) & (flat < e)
    col = np.where(valid, flat, e)
    indices = np.argsort(col, kind="stable")
    bin_ids = col[indices]
    tpe = np.bincount(col, minlength=e + 1)[:e]
    bins = np.cumsum(tpe)
    padded = np.cumsum((tpe + 127) // 128 * 128)
    bin0 = np.concatenate([[0], bins])
    pad0 = np.concatenate([[0], padded])
    pos = np.arange(flat.size)
    row = pad0[bin_ids] + (pos - bin0[bin_ids])
    row[(bin_ids >= e) | (row >= rows)] = -1
    row_of = np.empty(flat.size, dtype=np.int64)
    row_of[indices] = row
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
    return moe_ref.Route(i32(indices), i32(bin_ids), i32(bins), i32(padded),
                         i32(tpe), i32(row_of), 1, flat.size)
