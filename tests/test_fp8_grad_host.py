"""CPU: the reference of the fp8 gradient pieces (tests/fp8_grad_ref.py) is
what it says it is, and the inputs of tests/test_gpu_fp8_grad_wgrad.py show
the arithmetic they are meant to pin.

  columns     quantize_cols is fp8_ref.quantize_rows of the transpose.
  order       transposed_order agrees with a stable argsort of the indices.
  blocks      quantize_blocks_t is quantize_cols of each source block, in the
              transposed order.
  models      on the exact case, one scale of B per block instead of per
              column, and a multiply rounded before the add, each change most
              outputs (fp32 output, and after rounding to T).
  tie         tie_case's sums are ties of round_T, and ties-away differs.
"""

import numpy as np
import pytest

from tests import fp8_grad_ref as G
from tests import fp8_ref as R
from tests import rounding_ref as RR
from tests.moe_ref import P_BITS, values


@pytest.mark.parametrize("pow2", [False, True])
def test_quantize_cols_is_quantize_rows_of_the_transpose(pow2):
    x = values((256, 384), "bf16", [71])
    x[5, 7], x[130, 300] = np.nan, -np.inf
    x[:128, 9] = 0.0
    qt, st = G.quantize_cols(x, pow2)
    q, s = R.quantize_rows(np.ascontiguousarray(x.T), pow2)
    assert qt.shape == (384, 256) and st.shape == (2, 384)
    assert np.array_equal(qt, q)
    assert np.array_equal(st.view(np.uint32), s.T.copy().view(np.uint32))
    assert st[0, 9] == R.SCALE_FLOOR and qt[7, 5] == 0x7F and qt[300, 130] == 0xFF


def test_transposed_order_is_a_stable_sort_by_column():
    offsets, indices = G.SRC_TOPOLOGY
    offsets_t, indices_t, block_offsets = G.transposed_order(offsets, indices, 4)
    order = np.argsort(indices, kind="stable")
    assert np.array_equal(block_offsets, order)
    assert np.array_equal(indices_t, R.row_indices(offsets)[order])
    assert np.array_equal(offsets_t, [0, 5, 5, 7, 8])
    assert not np.array_equal(block_offsets, np.arange(len(indices)))
    # a random topology as well
    rng = np.random.default_rng(72)
    mask = rng.random((7, 5)) < 0.5
    offs = np.concatenate([[0], np.cumsum(mask.sum(1))]).astype(np.int32)
    idx = np.concatenate([rng.permutation(np.flatnonzero(r)) for r in mask]
                         ).astype(np.int16)
    o_t, i_t, b_o = G.transposed_order(offs, idx, 5)
    order = np.argsort(idx, kind="stable")
    assert np.array_equal(b_o, order)
    assert np.array_equal(i_t, R.row_indices(offs)[order])
    assert np.array_equal(np.diff(o_t), mask.sum(0))


def test_quantize_blocks_t_is_the_column_quantisation_of_each_block():
    nb = len(G.SRC_TOPOLOGY[1])
    src = values((nb, 128, 128), "f16", [73])
    _, _, block_offsets = G.transposed_order(*G.SRC_TOPOLOGY, 4)
    qt, st = G.quantize_blocks_t(src, block_offsets)
    for j, b in enumerate(block_offsets):
        q, s = G.quantize_cols(src[b])
        assert np.array_equal(qt[j], q)
        assert np.array_equal(st[j * 128:(j + 1) * 128], s[0])


def changed(a, b, rows) -> float:
    a, b = a[rows], b[rows]
    return float((a.view(np.uint32) != b.view(np.uint32)).mean())


def test_wrong_models_change_most_outputs_of_the_exact_case():
    case = G.exact_case()
    assert [len(s) for s in case.order] == [5, 0, 2, 1]
    p = G.interval_sums(case.aq, case.bq)
    for kb in range(case.k // 128):     # P is exact in any order
        ks = slice(kb * 128, (kb + 1) * 128)
        assert R.interval_sum(case.aq[:, ks], case.bq[:, ks])[1].max() * 64 < 2 ** 24
    right = case.acc(p=p)
    several = np.r_[0:128, 256:384]      # block rows with more than one step
    stored = np.r_[0:128, 256:512]
    off_first = np.ones(case.n, bool)
    off_first[::128] = False             # block_scale is right at column 0
    for out in ("f32", "f16", "bf16"):
        want = G.finish(right, out)
        block = G.finish(case.acc("block_scale", p), out)
        sep = G.finish(case.acc("mul_then_add", p), out)
        f_block = changed(want[:, off_first], block[:, off_first], stored)
        f_sep = changed(want, sep, several)
        print(f"{out}: block_scale changes {f_block:.3f}, mul_then_add "
              f"{f_sep:.3f} of the outputs")
        assert f_block > 0.5 and f_sep > 0.5, out
    # a block row of one step is fma(s, P, 0): a rounded product either way
    assert changed(right, case.acc("mul_then_add", p), np.r_[384:512]) == 0


@pytest.mark.parametrize("out", ["f16", "bf16"])
def test_tie_case_sums_are_ties(out):
    case = G.tie_case(out)
    acc = case.acc()
    p = P_BITS[out]
    stored = np.r_[0:128, 256:512]
    assert (acc[stored] == np.float32(2.0 ** -p)).all()
    c_old = np.where(np.arange(case.n) % 2, 1.0 + 2.0 ** -(p - 1), 1.0
                     ).astype(np.float32)[None, :].repeat(case.m, 0)
    got = G.finish(acc, out, c_old, case.order)
    assert (got[stored][:, 0::2] == 1.0).all()
    assert (got[stored][:, 1::2] == np.float32(1.0 + 2.0 ** -(p - 2))).all()
    away = RR.round_half_up((acc + c_old).astype(np.float64), out)
    assert (away[stored][:, 0::2] != 1.0).all()
    assert np.array_equal(got[128:256], c_old[128:256])
