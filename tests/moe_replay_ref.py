"""The routings of tests/test_gpu_moe_replay.py (numpy, host only) and what
the tests rely on about them, asserted before anything runs on a device.

Five [tokens, top_k] int32 arrays over 4 experts, top_k = 2:

    random   the router-like choice of test_gpu_moe_ops._mlp_data (distinct
             experts per token)
    last     both picks of every token on the last expert (duplicate experts
             per token; 600 -> 640 rows)
    first    everything on expert 0: the rows behind padded_bins[-1] then
             belong to the last expert, which has no token
    empty    expert 1 gets nothing
    exact    expert 0 gets exactly 128 assignments, expert 1 exactly 129
             (moe_ref's "exact" kind)

Between them the padded layouts differ in every expert's row count, in
padded_bins[-1] and in the number of slack block rows between padded_bins[-1]
and moe_rows_bound, which is what a graph replayed under another routing has
to follow on the device.
"""

from __future__ import annotations

import itertools

import numpy as np

from tests import moe_ref as R

NAMES = ("random", "last", "first", "empty", "exact")


def routings(random_top: np.ndarray, num_experts: int) -> dict:
    """name -> top_experts [tokens, top_k] int32 (read-only), checked."""
    random_top = np.asarray(random_top)
    tokens, top_k = random_top.shape
    e = num_experts
    rng = np.random.default_rng([29, tokens, top_k, e])
    others = [i for i in range(e) if i != 1]
    out = {
        "random": random_top,
        "last": np.full((tokens, top_k), e - 1),
        "first": np.zeros((tokens, top_k)),
        "empty": np.stack([rng.permutation(others)[:top_k]
                           for _ in range(tokens)]),
        "exact": R.routing(tokens, top_k, e, "exact"),
    }
    out = {k: np.ascontiguousarray(v, dtype=np.int32) for k, v in out.items()}
    for v in out.values():
        v.setflags(write=False)
    check(out, e)
    return out


def counts(top: np.ndarray, num_experts: int) -> np.ndarray:
    return np.bincount(top.reshape(-1), minlength=num_experts)


def padded_rows(top: np.ndarray, num_experts: int) -> int:
    """padded_bins[-1]: every count rounded up to a multiple of 128."""
    return int(((counts(top, num_experts) + 127) // 128 * 128).sum())


def check(tops: dict, num_experts: int) -> None:
    """What the replay tests assume about the routings (host arithmetic)."""
    e = num_experts
    assert tuple(tops) == NAMES
    shape = tops["random"].shape
    n = shape[0] * shape[1]
    rows = R.rows_bound(n, e)
    tpe = {k: counts(v, e) for k, v in tops.items()}
    for k, v in tops.items():
        assert v.shape == shape and v.dtype == np.int32, k
        assert v.min() >= 0 and v.max() < e and tpe[k].sum() == n, k
    for a, b in itertools.combinations(NAMES, 2):
        assert not np.array_equal(tpe[a], tpe[b]), (a, b)
    assert tpe["last"][e - 1] == n and tpe["first"][0] == n
    assert tpe["empty"][1] == 0 and (np.delete(tpe["empty"], 1) > 0).all()
    assert tpe["exact"][0] == 128 and tpe["exact"][1] == 129
    assert (tpe["random"] > 128).all()       # (two block rows per expert)
    # duplicate experts per token only where the routing asks for them
    assert (tops["random"][:, 0] != tops["random"][:, 1]).all()
    assert (tops["empty"][:, 0] != tops["empty"][:, 1]).all()
    padded = {k: padded_rows(v, e) for k, v in tops.items()}
    assert all(p % 128 == 0 and p <= rows for p in padded.values())
    assert len(set(padded.values())) >= 3, padded
    assert sum(p < rows for p in padded.values()) >= 3, padded
    # the slack of `last` / `first`: n rounded up once, against n + 127 e
    assert padded["last"] == padded["first"] == -(-n // 128) * 128
