"""Numpy references of the sigmoid-score router (RouterScoreTopK and
RouterScoreTopKGrad, sputnik/block/router.h), shared by
tests/test_router_score_host.py and tests/test_gpu_router_score*.py. Nothing
here calls the library.

    select      the picks of given selection values c = s + bias: groups,
                eligibility, order (larger first, ties to the lower index,
                -0 = +0, NaN last), in the arithmetic of c's dtype
    picks64/32  the picks in float64 / in the float32 emulation
    gaps_ok     the condition under which the float64 picks are the only right
                answer (below)
    forward64   float64 weights and scores for given picks
    forward32   the same in float32 arithmetic, rounded once
    grad64      float64 dlogits with the absolute image its bound is relative
                to; grad32 the float32 emulation

Selection is on computed fp32 values, so exact picks need a condition on the
inputs: in float64, every two consecutive values among the k + 1 largest
eligible c, and every two consecutive group scores, are either equal by
construction (bit-equal logits under bit-equal bias: then the float32 values
are equal too, which is how it is tested) or at least GAP = 2^-14 apart. The
fp32 sigmoid, add and group sum err by under 2^-19.5 on these ranges. The
generator redraws a row's logits until that holds.

Values of a type ("f16" / "bf16" / "f32") travel as float32 arrays holding
only representable values; every input is computed once, cached, read-only.
"""

from __future__ import annotations

import functools

import numpy as np

from tests import moe_ref
from tests import router_ref as R0

P_BITS = R0.P_BITS
LTYPES = R0.LTYPES
KINDS = R0.KINDS
rnd = R0.rnd
_sub = R0._sub
GAP = 2.0 ** -14
U = 2.0 ** -24                      # half an fp32 ulp, relative

# (tokens, E, top_k, num_groups, topk_groups)
CASES = [
    (1, 1, 1, 1, 1),        # one token, one expert
    (5, 64, 2, 1, 1),       # one wave, no groups
    (129, 65, 8, 5, 3),     # groups of 13 straddling the lane and j split
    (67, 8, 2, 4, 2),       # groups of 2
    (33, 256, 8, 8, 4),     # the V3 shape
    (9, 1024, 32, 64, 2),   # k = the eligible experts; G at its limit
    (3, 500, 7, 4, 1),      # kPer 8
    (4, 16, 4, 16, 4),      # gs = 1
    (300, 8, 2, 1, 1),      # many tokens, no groups
    (17, 384, 8, 3, 2),     # non-power-of-two G; kPer rounded up past E
]
IDS = ["%dx%d-k%d-g%d-%d" % c for c in CASES]
VALUE_KINDS = ["random", "ties", "equal"]       # ("special": only ids pinned)


# ---- selection --------------------------------------------------------------

def sigmoid64(l):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(l, dtype=np.float64)))


def sigmoid32(l):
    l = np.asarray(l, dtype=np.float32)
    one = np.float32(1.0)
    with np.errstate(over="ignore"):
        return (one / (one + np.exp(-l).astype(np.float32))).astype(np.float32)


def _desc(v, axis):
    """Stable descending argsort, NaN last (-0 equals +0)."""
    with np.errstate(invalid="ignore"):
        return np.argsort(-v, axis=axis, kind="stable")


def group_scores(c, g: int):
    """[tokens, G]: the sum of each group's first two values in the order (the
    first alone for groups of one), in c's dtype. None without groups."""
    if g == 1:
        return None
    tokens, e = c.shape
    gs = e // g
    cg = c.reshape(tokens, g, gs)
    srt = np.take_along_axis(cg, _desc(cg, 2), axis=2)
    return srt[:, :, 0] + srt[:, :, 1] if gs > 1 else srt[:, :, 0]


def select(c, k: int, g: int, gk: int):
    """(ids int32 [tokens, k], order [tokens, eligible]: every eligible
    expert in the order, group order [tokens, G] or None)."""
    tokens, e = c.shape
    gs = e // g
    scores = group_scores(c, g)
    eligible = np.ones((tokens, e), dtype=bool)
    gorder = None
    if scores is not None:
        gorder = _desc(scores, 1)
        on = np.zeros((tokens, g), dtype=bool)
        np.put_along_axis(on, gorder[:, :gk], True, axis=1)
        eligible = np.repeat(on, gs, axis=1)
    rank = _desc(c, 1)
    keep = np.take_along_axis(eligible, rank, axis=1)
    front = np.argsort(~keep, axis=1, kind="stable")[:, :gk * gs]
    order = np.take_along_axis(rank, front, axis=1)
    return order[:, :k].astype(np.int32), order, gorder


def c64(l, bias):
    return sigmoid64(l) + np.asarray(bias, dtype=np.float64)


def c32(l, bias):
    return (sigmoid32(l) + np.asarray(bias, dtype=np.float32)).astype(
        np.float32)


def picks64(l, bias, case) -> np.ndarray:
    return select(c64(l, bias), *case[2:])[0]


def picks32(l, bias, case) -> np.ndarray:
    return select(c32(l, bias), *case[2:])[0]


def _clear(a64, a32):
    """Per row: every two neighbours of a64 (in its order; a32 the float32
    values in the same positions) are equal in both or GAP apart in float64;
    pairs with a NaN are left out (NaN's place does not depend on
    rounding)."""
    if a64.shape[1] < 2:
        return np.ones(a64.shape[0], dtype=bool)
    x, y = a64[:, :-1], a64[:, 1:]
    with np.errstate(invalid="ignore"):
        same = (x == y) & (a32[:, :-1] == a32[:, 1:])
        apart = x - y >= GAP
    return (same | apart | np.isnan(x) | np.isnan(y)).all(axis=1)


def gaps_ok(l, bias, case) -> np.ndarray:
    """bool [tokens]: the condition of the module docstring, row by row."""
    tokens, e, k, g, gk = case
    a, b = c64(l, bias), c32(l, bias)
    _, order, gorder = select(a, k, g, gk)
    first = order[:, :k + 1]
    ok = _clear(np.take_along_axis(a, first, axis=1),
                np.take_along_axis(b, first, axis=1))
    if gorder is not None:
        ok &= _clear(np.take_along_axis(group_scores(a, g), gorder, axis=1),
                     np.take_along_axis(group_scores(b, g), gorder, axis=1))
    return ok


# ---- inputs -----------------------------------------------------------------

def _seed(case, kind, ltype):
    return list(case) + [KINDS.index(kind), LTYPES.index(ltype)]


@functools.lru_cache(maxsize=None)
def bias(case, kind: str) -> np.ndarray:
    """fp32 [E]. "random" and "special": uniform in [-0.5, 0.5] ("special":
    drawn again until a row of zero scores, what only -inf logits give, meets
    the gap condition, which no redraw of the logits could mend); "ties" and
    "equal": one value everywhere."""
    tokens, e, k, g, gk = case
    if kind in ("ties", "equal"):
        b = np.full(e, 0.25, dtype=np.float32)
    else:
        rng = np.random.default_rng(list(case) + [KINDS.index(kind), 77])
        lowest = np.full((1, e), -np.inf, dtype=np.float32)
        for _ in range(100000):
            b = rng.uniform(-0.5, 0.5, e).astype(np.float32)
            if kind == "random" or gaps_ok(lowest, b, case)[0]:
                break
        else:
            raise AssertionError("no bias found for %r" % (case,))
    b.setflags(write=False)
    return b


def _tie_row(rng, case):
    """Logits from three levels under one bias, so that all but `a` < Gk
    groups score the same (the topk_groups boundary is a tie whenever there
    is one) and, after redraws, the k-th and the (k+1)-th pick are equal."""
    tokens, e, k, g, gk = case
    gs = e // g
    hi, mid, lo = 3.0, 0.25, -2.0
    if g == 1:
        a = int(rng.integers(0, k))
        b = int(rng.integers(min(k + 1, e) - a, e - a + 1))
        return rng.permutation(np.array(
            [hi] * a + [mid] * b + [lo] * (e - a - b), np.float32))
    strong = rng.choice(g, int(rng.integers(0, gk)), replace=False)
    b = int(rng.integers(1, gs + 1))
    row = np.empty(e, dtype=np.float32)
    for grp in range(g):
        if grp in strong:
            vals = [hi] * min(2, gs) + [mid] * max(gs - 2, 0)
        else:
            vals = [mid] * b + [lo] * (gs - b)
        row[grp * gs:(grp + 1) * gs] = rng.permutation(
            np.array(vals, np.float32))
    return row


def ties_reach(l, bias_, case) -> np.ndarray:
    """bool [tokens]: the k-th and (k+1)-th pick are equal (where a (k+1)-th
    exists) and so are the group scores at the topk_groups boundary (where
    there is one)."""
    tokens, e, k, g, gk = case
    a = c64(l, bias_)
    _, order, gorder = select(a, k, g, gk)
    ok = np.ones(tokens, dtype=bool)
    if k < order.shape[1]:
        v = np.take_along_axis(a, order[:, k - 1:k + 1], axis=1)
        ok &= v[:, 0] == v[:, 1]
    if gorder is not None and gk < g:
        s = np.take_along_axis(group_scores(a, g), gorder[:, gk - 1:gk + 1],
                               axis=1)
        ok &= s[:, 0] == s[:, 1]
    return ok


def _special(rng, row, r: int, e: int):
    u = rng.random(e)
    which = (r + e) % 4
    if which == 0:                      # some NaN
        row[u < 0.3] = np.nan
        row[rng.integers(e)] = np.nan
    elif which == 1:                    # +inf and -inf
        row[u < 0.25] = np.inf
        row[u > 0.75] = -np.inf
        row[rng.integers(e)] = np.inf
    elif which == 2:                    # only -inf
        row[:] = -np.inf
    else:                               # everything at once
        row[u < 0.2] = np.nan
        row[(u >= 0.2) & (u < 0.4)] = -np.inf
        row[(u >= 0.4) & (u < 0.6)] = 0.0
        row[(u >= 0.6) & (u < 0.8)] = -0.0
    return row


@functools.lru_cache(maxsize=None)
def _logits(case, kind: str, ltype: str):
    tokens, e, k, g, gk = case
    rng = np.random.default_rng(_seed(case, kind, ltype))
    b = bias(case, kind)
    l = np.empty((tokens, e), dtype=np.float32)
    most = 0
    for r in range(tokens):
        for tries in range(100000):
            if kind == "equal":
                row = np.full(e, 0.75, dtype=np.float32)
            elif kind == "ties":
                row = _tie_row(rng, case)
            else:
                row = rnd(rng.uniform(-6.0, 6.0, e).astype(np.float32), ltype)
                if kind == "special":
                    row = _special(rng, row.copy(), r, e)
            one = row.reshape(1, e)
            if gaps_ok(one, b, case)[0] and (
                    kind != "ties" or ties_reach(one, b, case)[0]):
                break
        else:
            raise AssertionError("no row found for %r %s" % (case, kind))
        most = max(most, tries)
        l[r] = row
    l.setflags(write=False)
    return l, most


def logits(case, kind: str, ltype: str) -> np.ndarray:
    """[tokens, E] float32 holding values of `ltype`; every row meets
    gaps_ok."""
    return _logits(case, kind, ltype)[0]


def redraws(case, kind: str, ltype: str) -> int:
    """The most redraws any row of logits(...) needed."""
    return _logits(case, kind, ltype)[1]


# ---- forward ----------------------------------------------------------------

def forward64(l, ids, normalize: bool, scale: float):
    """(weights [tokens, k], scores [tokens, E]) in float64."""
    s = sigmoid64(l)
    w = np.take_along_axis(s, ids.astype(np.int64), axis=1)
    if normalize:
        w = w / w.sum(axis=1, keepdims=True)
    return w * float(np.float32(scale)), s


def forward32(l, ids, normalize: bool, scale: float, out_type: str):
    s = sigmoid32(l)
    w = np.take_along_axis(s, ids.astype(np.int64), axis=1)
    if normalize:
        w = (w / w.sum(axis=1, keepdims=True, dtype=np.float32)).astype(
            np.float32)
    w = (w * np.float32(scale)).astype(np.float32)
    return rnd(w, out_type), rnd(s, out_type)


# In units of U = 2^-24 relative (one correctly rounded fp32 operation):
# expf within 2 ulp (4), 1 + x (1), the division (1).
SIGMOID_OPS = 6


def scores_bound(ref, out_type: str) -> np.ndarray:
    """One rounding to the output type of a sigmoid SIGMOID_OPS off."""
    return ((2.0 ** -P_BITS[out_type] + SIGMOID_OPS * U) * np.abs(ref)
            + _sub(out_type))


def weights_bound(ref, k: int, out_type: str) -> np.ndarray:
    """The picked sigmoid (6); with normalize the sum of k positive terms,
    each 6 off, in any order (k - 1 additions; the wave's butterfly has 6
    levels: k + 6 covers both) and the division (1); the scale (1): 6 + 6 +
    (k + 6) + 1 + 1 = 20 + k, then one rounding to the output type."""
    return ((2.0 ** -P_BITS[out_type] + (20 + k) * U) * np.abs(ref)
            + _sub(out_type))


# ---- gradient ---------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def grad_ids(case, ltype: str) -> np.ndarray:
    """The picks of the "random" logits, except (as router_ref.grad_ids): row
    0 slot 0 is E (out of range), row 1's last slot is -7, and row 2's slot 1
    repeats its slot 0 (top_k >= 2)."""
    tokens, e, k = case[:3]
    ids = picks64(logits(case, "random", ltype), bias(case, "random"),
                  case).copy()
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
    tokens, e, k = case[:3]
    seed = list(case) + [LTYPES.index(ltype), wtype == "f32"]
    make = moe_ref.values if wtype != "f32" else (
        lambda shape, _t, s: moe_ref.values(shape, "f16", s))
    dw = make((tokens, k), wtype, seed + [1])
    ds = make((tokens, e), wtype, seed + [2])
    for a in (dw, ds):
        a.setflags(write=False)
    return dw, ds


def _ds(s, ids, dw, dscores, normalize, scale, absolute, ft):
    """ds [tokens, E] in arithmetic of type `ft`; with `absolute` every term
    enters by its absolute value (the image the bound is relative to)."""
    tokens, e = s.shape
    k = ids.shape[1]
    dw = np.asarray(dw, dtype=ft)
    scale = ft(np.float32(scale))
    if absolute:
        dw, scale = np.abs(dw), abs(scale)
    ds = (np.zeros((tokens, e), ft) if dscores is None
          else np.asarray(dscores, dtype=ft).copy())
    if absolute:
        ds = np.abs(ds)
    valid = (ids >= 0) & (ids < e)
    safe = np.where(valid, ids, 0).astype(np.int64)
    ssel = np.where(valid, np.take_along_axis(s, safe, axis=1), 0).astype(ft)
    dw = np.where(valid, dw, 0).astype(ft)
    if normalize:
        # (a row without a valid pick divides 0 by 0 and adds nothing)
        with np.errstate(invalid="ignore", divide="ignore"):
            total = ssel.sum(axis=1, keepdims=True, dtype=ft)
            c = ((dw * ssel).astype(ft).sum(axis=1, keepdims=True, dtype=ft)
                 / total).astype(ft)
            g = ((scale * (dw + c if absolute else dw - c)).astype(ft)
                 / total).astype(ft)
    else:
        g = (scale * dw).astype(ft)
    rows = np.arange(tokens)
    for j in range(k):          # one slot at a time: a repeated id adds twice
        v = valid[:, j]
        ds[rows[v], safe[v, j]] += g[v, j]
    return ds


def grad64(l, ids, dw, dscores, normalize: bool, scale: float):
    """(dlogits, image, s), float64: image = the absolute image of ds."""
    s = sigmoid64(l)
    ds = _ds(s, ids, dw, dscores, normalize, scale, False, np.float64)
    image = _ds(s, ids, dw, dscores, normalize, scale, True, np.float64)
    return ds * s * (1.0 - s), image, s


def grad32(l, ids, dw, dscores, normalize: bool, scale: float,
           ltype: str) -> np.ndarray:
    s = sigmoid32(l)
    ds = _ds(s, ids, dw, dscores, normalize, scale, False, np.float32)
    one = np.float32(1.0)
    return rnd(((ds * s).astype(np.float32) * (one - s)).astype(np.float32),
               ltype)


def grad_bound(ref, image, s, k: int, ltype: str) -> np.ndarray:
    """dlogits = ds s (1 - s). Relative to its absolute image, ds is off by
    4 k + 41 units: with normalize, c = sum_j dw_j s_j / S carries 6 + 1 per
    term, k + 6 for the sum, 12 + k for S and 1 for the division (2 k + 26);
    g = scale (dw - c) / S adds the subtraction, the scale, S and the
    division (k + 15) on |dw| + |c|; the k additions into ds add k. The
    product: s is 6 off, each multiplication 1, and 1 - s is off by 6 s (the
    error of s, not relative to 1 - s) plus its own rounding. In all
    ((4 k + 41) + 6 + 1 + 1 + 1) s (1 - s) + 6 s^2, times the image, then one
    rounding to the logits' type."""
    return (2.0 ** -P_BITS[ltype] * np.abs(ref)
            + U * ((4 * k + 50) * s * (1.0 - s) + 6 * s * s) * image
            + _sub(ltype))
