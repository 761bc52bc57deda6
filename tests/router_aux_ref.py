"""Numpy references and bounds of the router's auxiliary-loss statistics
(RouterTopKAux / RouterTopKAuxGrad, sputnik/block/router.h), shared by
tests/test_router_aux_host.py and tests/test_gpu_router_aux*.py. They build
on tests/router_ref.py; nothing here calls the library.

    stats64     float64 score_sums [E], z_sum and the per-token m / lse
    stats32     the same in float32 arithmetic and in the kernel's order: 16
                tokens per wave in sequence, the 4 waves of a group in wave
                order, the groups in ascending order
    grad64      float64 dlogits and the absolute-value image its bound is
                relative to, with dscore_sums and dz_sum
    grad32      the gradient in float32 arithmetic, rounded once

Bounds (u = 2^-24):

    score_sums  |err| <= (E + 64 + tokens) u ref. Each p_te carries the
                project's per-score error (E + 64) u p without the output
                rounding (router_ref.scores_bound), and each of the at most
                tokens - 1 additions one rounding; every term is >= 0, so the
                sum of the terms' bounds is the bound times the sum, in any
                order of summation.
    z_sum       |err| <= sum_t 2 |lse_t| d_t + (tokens + 2) u ref with
                d_t = (E + 64) u + 2 u (|m_t| + |lse_t - m_t|): d_t bounds the
                error of lse_t = m_t + log s_t (the relative error (E + 64) u
                of s_t is the absolute error of its logarithm; logf and the
                addition round once each, relative to |lse_t - m_t| and to
                |m_t| + |lse_t - m_t|), 2 |lse_t| d_t its square's, and the
                square, the additions and the two reduction stages round
                (tokens + 2) times relative to the non-negative sum.
    dlogits     router_ref.grad_bound unchanged, with dscore_sums broadcast
                into dscores for the reference and the image, 2 dz lse_t p_tj
                added to the reference and 2 |dz| (|lse_t| + 1) p_tj to the
                image.
"""

from __future__ import annotations

import functools

import numpy as np

from tests import moe_ref
from tests import router_ref as R

T = 64                             # sputnik::block::kRouterAuxTokens
WAVES = 4
U = 2.0 ** -24

# (tokens, E, top_k): a partial wave, a full group, a group plus one token, a
# ragged last group, and every register width (E <= 64, 128, 256, 512, 1024).
AUX_CASES = [
    (1, 1, 1), (1, 4, 4), (T - 1, 8, 2), (T, 64, 2), (T + 1, 65, 8),
    (3 * T + 5, 8, 2), (33, 256, 8), (9, 1024, 32), (3, 500, 7), (300, 8, 2),
]
IDS = ["%dx%d-k%d" % c for c in AUX_CASES]


def kinds(case):
    """The value kinds a case runs with: all three where router_ref has the
    case, the uniform(-8, 8) recipe alone elsewhere."""
    return (["random", "ties", "equal"] if case in R.ROUTER_CASES
            else ["random"])


logits = R.logits                  # (the same recipe for any case)


@functools.lru_cache(maxsize=None)
def aux_grads(case, ltype: str):
    """(dscore_sums float32 [E], dz_sum float32 [1]): magnitudes in
    [2^-10, 4], random signs."""
    tokens, e, k = case
    seed = [tokens, e, k, R.LTYPES.index(ltype)]
    dss = moe_ref.values((e,), "f16", seed + [3]).astype(np.float32)
    dz = moe_ref.values((1,), "f16", seed + [4]).astype(np.float32)
    for a in (dss, dz):
        a.setflags(write=False)
    return dss, dz


# ---- forward ------------------------------------------------------------------

def stats64(l):
    """(score_sums [E], z_sum, m [tokens], lse [tokens]) in float64."""
    l = np.asarray(l, dtype=np.float64)
    m = l.max(axis=1)
    ex = np.exp(l - m[:, None])
    s = ex.sum(axis=1)
    lse = m + np.log(s)
    return (ex / s[:, None]).sum(axis=0), float((lse * lse).sum()), m, lse


def _kernel_order_sum(x):
    """float32 sum over axis 0 of x [tokens, ...] in the kernel's order."""
    x = np.asarray(x, dtype=np.float32)
    tokens = x.shape[0]
    groups = -(-tokens // T)
    pad = np.zeros((groups * T,) + x.shape[1:], np.float32)
    pad[:tokens] = x
    pad = pad.reshape((groups, WAVES, T // WAVES) + x.shape[1:])
    wave = np.zeros((groups, WAVES) + x.shape[1:], np.float32)
    for i in range(T // WAVES):
        wave = (wave + pad[:, :, i]).astype(np.float32)
    group = wave[:, 0]
    for w in range(1, WAVES):
        group = (group + wave[:, w]).astype(np.float32)
    total = np.zeros(x.shape[1:], np.float32)
    for g in range(groups):
        total = (total + group[g]).astype(np.float32)
    return total


def _lse32(l):
    l = np.asarray(l, dtype=np.float32)
    m = l.max(axis=1)
    ex = np.exp((l - m[:, None]).astype(np.float32)).astype(np.float32)
    s = ex.sum(axis=1, dtype=np.float32)
    return (m + np.log(s).astype(np.float32)).astype(np.float32)


def stats32(l):
    """(score_sums float32 [E], z_sum float32) as the kernels form them."""
    p = R._softmax32(l)
    lse = _lse32(l)
    return (_kernel_order_sum(p),
            _kernel_order_sum((lse * lse).astype(np.float32)))


def score_sums_bound(ref, tokens: int, e: int) -> np.ndarray:
    return (e + 64 + tokens) * U * np.abs(ref)


def z_sum_bound(ref: float, m, lse, e: int) -> float:
    tokens = len(m)
    d = (e + 64) * U + 2 * U * (np.abs(m) + np.abs(lse - m))
    return float((2 * np.abs(lse) * d).sum() + (tokens + 2) * U * abs(ref))


# ---- gradient -----------------------------------------------------------------

def _broadcast(l, dscores, dss, ft):
    if dss is None:
        return dscores
    base = (np.zeros(np.shape(l), ft) if dscores is None
            else np.asarray(dscores, dtype=ft))
    return (base + np.asarray(dss, dtype=ft)[None, :]).astype(ft)


def grad64(l, ids, dw, dscores, dss, dz, normalize: bool):
    """(dlogits, image) in float64; dss / dz None: absent."""
    ref, image = R.grad64(l, ids, dw, _broadcast(l, dscores, dss, np.float64),
                          normalize)
    if dz is not None:
        dz = float(np.asarray(dz).reshape(-1)[0])
        _, _, _, lse = stats64(l)
        p = R.softmax64(l)
        ref = ref + 2 * dz * lse[:, None] * p
        image = image + 2 * abs(dz) * (np.abs(lse)[:, None] + 1) * p
    return ref, image


def grad32(l, ids, dw, dscores, dss, dz, normalize: bool, ltype: str):
    p = R._softmax32(l)
    dp = R._dp(p, ids, dw, _broadcast(l, dscores, dss, np.float32), normalize,
               False, np.float32)
    dot = (dp * p).astype(np.float32).sum(axis=1, keepdims=True,
                                          dtype=np.float32)
    out = (p * (dp - dot).astype(np.float32)).astype(np.float32)
    if dz is not None:
        zc = (np.float32(2) * np.float32(np.asarray(dz).reshape(-1)[0])
              * _lse32(l)).astype(np.float32)
        out = (out + (zc[:, None] * p).astype(np.float32)).astype(np.float32)
    return R.rnd(out, ltype)


def grad_bound(ref, image, e: int, k: int, ltype: str) -> np.ndarray:
    return R.grad_bound(ref, image, e, k, ltype)
