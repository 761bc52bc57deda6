"""GPU: DsdFp8Wgrad (sputnik/block/fp8.h, "Gradients"), the DSD whose dense
operand carries one scale per interval and column, through the C ABI.

The sparse operand has the transposed topology of fp8_grad_ref (4 x 6 blocks;
block rows of 5, 0, 2 and 1 stored blocks, so the two-stage ring turns over
more than twice in block row 0 and block row 1 runs no step) and n = 256:
8 workgroups.

  exact      fp8_grad_ref.exact_case (P exact in any order, ordinary scales,
             cancelling pairs): bit for bit the fma32 chain with per-column
             scales, T in {f16, bf16} and fp32 output, both modes; in kFast P
             comes from Fp8IntervalSums, as tests/test_gpu_fp8_fast.py has it.
             tests/test_fp8_grad_host.py shows that a per-block scale and a
             separate multiply each change most of these outputs.
  add        bit for bit round(acc + C_old) over a non-trivial C_old; block
             row 1 untouched under add and +0 without; a tie goes to even.
  bound      random data within the header's bound of the float64 product.
  per column the same operands with column scales that differ inside a block
             differ from the per-block product in exactly the expected
             columns.
  rejections every rejection leaves C's fill intact; an out-of-range stored
             block contributes zero.
  forms      through QuantizeBlocks / QuantizeTiles the product equals the
             dense computation on the dequantised operands within the bound,
             and DsdFp8 on the same operand with block-constant column scales
             equals DsdFp8Wgrad bit for bit.
"""

import ctypes
import functools

import numpy as np
import pytest
import torch

import sputnik_amd as sp
from tests import fp8_grad_ref as G
from tests import fp8_ref as R
from tests import rounding_ref as RR
from tests import test_gpu_fp8_exact as E
from tests import test_gpu_fp8_fast as F
from tests.moe_ref import P_BITS

pytestmark = pytest.mark.gpu

OUTS = ["f16", "bf16", "f32"]
MODES = ["fp32", "fast"]
INVALID = 1
PATTERN32 = 0x55555555


def fresh(shape, out):
    """A moated output filled with the pattern: (view, whole, pad, pattern)."""
    if out == "f32":
        fill = torch.tensor([PATTERN32], dtype=torch.int32).view(
            torch.float32).item()
        return RR.moated(shape, torch.float32, fill, row=shape[-1]) + (
            PATTERN32,)
    return E.fresh(shape, out) + (E.PATTERN,)


def out_bits(t) -> np.ndarray:
    if t.dtype == torch.float32:
        return t.cpu().numpy().view(np.uint32)
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def want_bits(c, out) -> np.ndarray:
    if out == "f32":
        return np.ascontiguousarray(c, np.float32).view(np.uint32)
    return RR.bits(c, out)


def put(c_old, out, view):
    """C_old's values (float32 holding values of the output type) into
    `view`."""
    if out == "f32":
        view.copy_(torch.from_numpy(np.ascontiguousarray(c_old, np.float32)))
    else:
        view.view(torch.int16).copy_(torch.from_numpy(
            RR.bits(c_old, out).view(np.int16)))


def call(case, out_t, mode, add=False, indices=None):
    offsets, idx = case.topology
    idx = idx if indices is None else indices
    sq, ss = case.sparse()
    s = sp.BlockMatrix(case.m, case.k, 128, len(idx) * 128 * 128,
                       E.place(sq, torch.float8_e4m3fn, False),
                       E.place(offsets, torch.int32, False),
                       E.place(np.asarray(idx, np.int16), torch.int16, False))
    sp.DsdFp8Wgrad(s, E.place(ss, torch.float32, False),
                   E.place(case.bq, torch.float8_e4m3fn, False),
                   E.place(case.sb, torch.float32, False),
                   sp.Matrix(case.m, case.n, out_t), add=add, accumulate=mode)
    torch.cuda.synchronize()


def run_twice(case, out, mode, c_old=None, **kw) -> np.ndarray:
    """The output's bits after two runs into fresh moated outputs that must
    agree bit for bit and leave the moats intact."""
    runs = []
    for _ in range(2):
        view, whole, pad, pattern = fresh((case.m, case.n), out)
        if c_old is not None:
            put(c_old, out, view)
        call(case, view, mode, add=c_old is not None, **kw)
        assert RR.moat_intact(whole, pad, pattern)
        runs.append(out_bits(view))
    assert np.array_equal(runs[0], runs[1]), "two runs differ"
    return runs[0]


@functools.lru_cache(maxsize=None)
def exact():
    return G.exact_case()


@functools.lru_cache(maxsize=None)
def sums(mode):
    """P of the exact case: the reference's in kFp32 (held against
    Fp8IntervalSums by tests/test_gpu_fp8_fast.py), Fp8IntervalSums' in
    kFast."""
    case = exact()
    if mode == "fp32":
        return G.interval_sums(case.aq, case.bq)
    return F.interval_sums(case.aq, case.bq, "fast")


def old_values(case, out, seed):
    """A non-trivial C_old of the output type, of the accumulator's size."""
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal((case.m, case.n)) * 2.0 ** -4).astype(np.float32)
    return v if out == "f32" else R.round_t(v, out)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("out", OUTS)
def test_exact_case_bit_for_bit(out, mode):
    case = exact()
    acc = case.acc(p=sums(mode))
    got = run_twice(case, out, mode)
    assert np.array_equal(got, want_bits(G.finish(acc, out), out))
    assert not got[128:256].any()               # the empty block row: +0
    if mode == "fp32":                          # the wrong models are visible
        for model in G.MODELS:
            wrong = want_bits(G.finish(case.acc(model, sums(mode)), out), out)
            assert (got != wrong).mean() > 0.25, model


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("out", OUTS)
def test_add_rounds_once_and_leaves_empty_block_rows_alone(out, mode):
    case = exact()
    acc = case.acc(p=sums(mode))
    c_old = old_values(case, out, [91, OUTS.index(out)])
    got = run_twice(case, out, mode, c_old)
    want = G.finish(acc, out, c_old, case.order)
    assert np.array_equal(got, want_bits(want, out))
    assert np.array_equal(got[128:256], want_bits(c_old, out)[128:256])
    if out != "f32":    # not two roundings
        twice = R.round_t(R.round_t(acc, out) + c_old, out)
        assert (got != want_bits(twice, out)).any()


@pytest.mark.parametrize("out", ["f16", "bf16"])
def test_add_rounds_a_tie_to_even(out):
    case = G.tie_case(out)
    p = P_BITS[out]
    c_old = np.where(np.arange(case.n) % 2, 1.0 + 2.0 ** -(p - 1), 1.0
                     ).astype(np.float32)[None, :].repeat(case.m, 0)
    got = run_twice(case, out, "fp32", c_old)
    want = G.finish(case.acc(), out, c_old, case.order)
    assert np.array_equal(got, want_bits(want, out))
    stored = np.r_[0:128, 256:512]
    away = RR.round_half_up((case.acc() + c_old).astype(np.float64), out)
    assert (got[stored] != want_bits(away, out)[stored]).any()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_random_within_bound_and_the_forms_agree(dtype, mode):
    """Values of T through the device quantisers (QuantizeBlocks' column
    pair, QuantizeTiles' column pair) into DsdFp8Wgrad, against the float64
    product of the dequantised operands, into T and into fp32."""
    case, src, b = G.random_case(dtype)
    from tests import test_gpu_fp8 as T
    from tests import test_gpu_fp8_grad_quantize as Q

    s, block_offsets = Q.source(T.dev(src, dtype))
    nb = s.num_blocks
    qt = torch.empty(nb, 128, 128, dtype=torch.float8_e4m3fn, device="cuda")
    st = torch.empty(nb * 128, device="cuda")
    sp.QuantizeBlocks(s, qt=qt, scales_t=st)
    bqt = torch.empty(case.n, case.k, dtype=torch.float8_e4m3fn, device="cuda")
    bst = torch.empty(case.k // 128, case.n, device="cuda")
    sp.QuantizeTiles(T.dev(b, dtype), qt=bqt, scales_t=bst)
    # the device's operands are the reference's
    sq, ss = case.sparse()
    assert np.array_equal(qt.view(torch.uint8).cpu().numpy(), sq)
    assert np.array_equal(st.cpu().numpy(), ss)
    assert np.array_equal(bqt.view(torch.uint8).cpu().numpy(), case.bq)
    assert np.array_equal(bst.cpu().numpy(), case.sb)
    a64 = R.dequantize_rows(case.aq, case.sa)
    ref, absum = R.matmul64(a64, G.dequantize_cols(case.bq, case.sb))
    st_t = sp.BlockMatrix(case.m, case.k, 128, nb * 128 * 128, qt,
                          s.offsets_t, s.indices_t)
    for out in (dtype, "f32"):
        view, whole, pad, pattern = fresh((case.m, case.n), out)
        sp.DsdFp8Wgrad(st_t, st, bqt, bst, sp.Matrix(case.m, case.n, view),
                       accumulate=mode)
        torch.cuda.synchronize()
        assert RR.moat_intact(whole, pad, pattern)
        got = view.float().cpu().numpy().astype(np.float64)
        lim = G.bound(ref, absum, case.k, out, fast=mode == "fast")
        err = np.abs(got - ref)
        print(f"{dtype} -> {out} {mode}: worst error / bound = "
              f"{float((err / np.maximum(lim, 1e-300)).max()):.3f}")
        assert (err <= lim).all()
        assert not got[128:256].any()


@pytest.mark.parametrize("mode", MODES)
def test_block_constant_column_scales_equal_dsd_fp8(mode):
    case = exact().copy()
    sw = R.ordinary_scales(np.random.default_rng(92),
                           (case.k // 128, case.n // 128))
    case.sb = np.ascontiguousarray(np.repeat(sw, 128, axis=1))
    got = run_twice(case, "bf16", mode)
    ops = R.Operands("dsd", case.aq, case.sa, case.bq, sw, case.topology)
    assert np.array_equal(got, F.run_twice(ops, "bf16", mode))


def test_column_scales_that_differ_inside_a_block_show_in_their_columns():
    """The test that pins the new arithmetic: from block-constant column
    scales, doubling the scales of columns 5 and 200 at every k-block doubles
    exactly those outputs (a power of two: exact), and leaves every other
    column's bits alone."""
    case = exact().copy()
    sw = R.ordinary_scales(np.random.default_rng(93),
                           (case.k // 128, case.n // 128))
    case.sb = np.ascontiguousarray(np.repeat(sw, 128, axis=1))
    base = run_twice(case, "f32", "fp32").view(np.float32)
    case.sb[:, [5, 200]] *= np.float32(2.0)
    got = run_twice(case, "f32", "fp32").view(np.float32)
    changed = np.zeros(case.n, bool)
    changed[[5, 200]] = True
    assert np.array_equal(got[:, ~changed].view(np.uint32),
                          base[:, ~changed].view(np.uint32))
    assert np.array_equal(got[:, changed], 2.0 * base[:, changed])
    stored = np.r_[0:128, 256:512]
    assert (base[stored][:, changed] != 0).mean() > 0.9
    # ... and it is the chain with per-column scales
    assert np.array_equal(got.view(np.uint32),
                          want_bits(G.finish(case.acc(), "f32"), "f32"))


def test_an_out_of_range_stored_block_contributes_zero():
    case = exact()
    idx = case.topology[1].copy()
    idx[1], idx[6] = case.k // 128, -1      # block row 0's second, row 2's last
    got = run_twice(case, "bf16", "fp32", indices=idx)
    order = [[kb for kb in steps] for steps in case.order]
    order[0] = [kb for n, kb in enumerate(order[0]) if n != 1]
    order[2] = order[2][:-1]
    acc = G.chain(sums("fp32"), case.sa, case.sb, order)
    assert np.array_equal(got, want_bits(G.finish(acc, "bf16"), "bf16"))


def test_rejections_leave_c_untouched():
    case = exact()
    offsets, idx = case.topology
    nb = len(idx)
    sq, ss = case.sparse()
    d_sq = E.place(sq, torch.float8_e4m3fn, False)
    d_ss = E.place(ss, torch.float32, False)
    d_bq = E.place(case.bq, torch.float8_e4m3fn, False)
    d_sb = E.place(case.sb, torch.float32, False)
    d_off = E.place(offsets, torch.int32, False)
    d_idx = E.place(idx, torch.int16, False)
    view, whole, pad, pattern = fresh((case.m, case.n), "f32")
    f = sp.lib().sputnik_dsd_fp8_wgrad

    def go(data=d_sq, ss_=d_ss, bq=d_bq, sb=d_sb, c_ptr=None, rows=case.m,
           cols=case.n, k=case.k, dtype=1, out=1, add=0, mode=0, size=128,
           nonzeros=nb * 128 * 128, off=d_off):
        s = sp.BlockMatrix(case.m, k, size, nonzeros, data, off, d_idx)
        cs = s._c()
        cm = sp._CMatrix(rows, cols, view.data_ptr() if c_ptr is None
                         else c_ptr)
        ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        return f(ctypes.byref(cs), ptr(ss_), ptr(bq), ptr(sb),
                 ctypes.byref(cm), dtype, out, add, mode, None)

    for add in (0, 1):
        assert go(add=add, mode=2) == INVALID
        assert go(add=add, out=2) == INVALID
        assert go(add=add, dtype=2) == INVALID
        assert go(add=add, k=case.k - 64) == INVALID
        assert go(add=add, cols=192) == INVALID
        assert go(add=add, rows=case.m + 128) == INVALID
        assert go(add=add, size=64) == INVALID
        assert go(add=add, nonzeros=nb * 128 * 128 + 128) == INVALID
        assert go(add=add, ss_=None) == INVALID
        assert go(add=add, sb=None) == INVALID
        assert go(add=add, bq=None) == INVALID
        assert go(add=add, off=None) == INVALID
        assert go(add=add, c_ptr=view.data_ptr() + 8) == INVALID
        assert go(add=add, c_ptr=d_bq.data_ptr()) == INVALID    # C is an input
        assert go(add=add, c_ptr=d_sb.data_ptr()) == INVALID
        assert go(add=add, c_ptr=d_sq.data_ptr()) == INVALID
    torch.cuda.synchronize()
    assert bool((whole.view(torch.int32) == PATTERN32).all())
    assert go(rows=0, cols=case.n, k=case.k) == INVALID     # c.rows != s.rows
    # ... and the same call with nothing wrong runs
    assert go() == 0
    torch.cuda.synchronize()
    assert RR.moat_intact(whole, pad, pattern)
    assert not bool((view.view(torch.int32) == PATTERN32).all())
