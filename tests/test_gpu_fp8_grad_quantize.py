"""GPU: the quantisers of the fp8 backward pass (sputnik/block/fp8.h,
"Gradients") through the C ABI, bit for bit.

  tiles      QuantizeTiles on [256, 384] (2 x 3 tiles, non-square): the row
             pair equals QuantizeRows' bits, the column pair the reference's
             (tests/fp8_grad_ref.quantize_cols), with the special rows of
             tests/test_gpu_fp8.py turned into columns (subnormal amax, an
             all-zero tile, NaN, +Inf, +-0), both scale rules, both dtypes.
             A null row pair or a null column pair leaves the other pair's
             bits unchanged. One workgroup per tile: there is no second trip.
  blocks     QuantizeBlocks on the 6 x 4 topology of fp8_grad_ref (column 0
             with five blocks, column 1 empty, block row 0 out of order), the
             three stages: row outputs equal the existing row quantisers on
             the same values, column outputs the reference in the order of
             the device Transpose's block_offsets.
  weight     TransposeWeightFp8 of QuantizeWeight(w) equals QuantizeWeight of
             the transposed buffer, bit for bit.
  bounds     every output sits in a guard pattern that stays intact.
  rejections hipErrorInvalidValue with nothing written; a block_offsets entry
             out of range leaves its output block unwritten.
"""

import ctypes

import numpy as np
import pytest
import torch

import sputnik_amd as sp
from tests import fp8_grad_ref as G
from tests import fp8_ref as R
from tests import moe_ref as M
from tests import test_gpu_fp8 as T

pytestmark = pytest.mark.gpu

DTYPES = ["f16", "bf16"]
SHAPE = (256, 384)
INVALID = 1


def bits32(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint32)


def bytes_of(t) -> np.ndarray:
    return t.view(torch.uint8).cpu().numpy()


def column_values(dtype, seed):
    """[256, 384] whose columns carry test_gpu_fp8's special rows."""
    return np.ascontiguousarray(T.row_values(SHAPE[::-1], dtype, seed).T)


def tiles_call(dx, pow2, rows=True, cols=True):
    m, n = dx.shape
    out, checks = {}, []
    if rows:
        out["q"], ok = T.guarded((m, n), torch.float8_e4m3fn)
        checks.append(ok)
        out["scales"], ok = T.guarded((m, n // 128), torch.float32)
        checks.append(ok)
    if cols:
        out["qt"], ok = T.guarded((n, m), torch.float8_e4m3fn)
        checks.append(ok)
        out["scales_t"], ok = T.guarded((m // 128, n), torch.float32)
        checks.append(ok)
    sp.QuantizeTiles(dx, pow2=pow2, **out)
    torch.cuda.synchronize()
    assert all(ok() for ok in checks)
    return out


@pytest.mark.parametrize("pow2", [False, True], ids=["exact", "pow2"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_quantize_tiles_bit_for_bit(dtype, pow2):
    x = column_values(dtype, [81, pow2])
    dx = T.dev(x, dtype)
    both = tiles_call(dx, pow2)
    # rows: the existing call
    q = torch.empty(SHAPE, dtype=torch.float8_e4m3fn, device="cuda")
    s = torch.empty(SHAPE[0], SHAPE[1] // 128, device="cuda")
    sp.QuantizeRows(dx, q, s, pow2)
    assert np.array_equal(bytes_of(both["q"]), bytes_of(q))
    assert np.array_equal(bits32(both["scales"]), bits32(s))
    # columns: the reference
    qt_ref, st_ref = G.quantize_cols(x, pow2)
    got_qt, got_st = bytes_of(both["qt"]), both["scales_t"].cpu().numpy()
    assert np.array_equal(got_st.view(np.uint32), st_ref.view(np.uint32))
    assert np.array_equal(got_qt, qt_ref)
    # the special columns are where they were planted: x[r, c] = rows[c, r]
    assert got_qt[0, 5] == 0x7F and got_qt[1, 7] == 0x7F
    assert got_qt[0, 10] == 0x00 and got_qt[0, 11] == 0x80
    assert got_st[0, 2] == R.SCALE_FLOOR and not got_qt[2, :128].any()
    if dtype == "bf16":
        assert got_st[1, 383] == R.SCALE_FLOOR
        assert got_qt[383, 255] == R.encode(np.float32(7 * 2.0 ** -7))
    # a null pair leaves the other pair's bits unchanged
    only_rows = tiles_call(dx, pow2, cols=False)
    only_cols = tiles_call(dx, pow2, rows=False)
    assert np.array_equal(bytes_of(only_rows["q"]), bytes_of(both["q"]))
    assert np.array_equal(bits32(only_rows["scales"]), bits32(both["scales"]))
    assert np.array_equal(bytes_of(only_cols["qt"]), got_qt)
    assert np.array_equal(bits32(only_cols["scales_t"]),
                          got_st.view(np.uint32))


@pytest.mark.parametrize("dtype", DTYPES)
def test_quantize_tiles_unaligned_buffers_give_the_same_bytes(dtype):
    x = column_values(dtype, [82])
    dx = T.dev(x, dtype)
    want = tiles_call(dx, False)
    m, n = SHAPE
    q, q_ok = T.guarded((m, n), torch.float8_e4m3fn, 1)
    s, s_ok = T.guarded((m, n // 128), torch.float32)
    qt, qt_ok = T.guarded((n, m), torch.float8_e4m3fn, 3)
    st, st_ok = T.guarded((m // 128, n), torch.float32)
    sp.QuantizeTiles(T.offset_by_one(dx), q, s, qt, st)
    torch.cuda.synchronize()
    assert q_ok() and s_ok() and qt_ok() and st_ok()
    assert np.array_equal(bytes_of(q), bytes_of(want["q"]))
    assert np.array_equal(bytes_of(qt), bytes_of(want["qt"]))
    assert np.array_equal(bits32(s), bits32(want["scales"]))
    assert np.array_equal(bits32(st), bits32(want["scales_t"]))


# ---- blocks -------------------------------------------------------------------------

def source(data):
    """The BlockMatrix of SRC_TOPOLOGY over `data` with the device
    Transpose's metadata, which must be the reference's."""
    offsets, indices = G.SRC_TOPOLOGY
    s = sp.BlockMatrix(G.SRC_ROWS, G.SRC_COLS, 128, len(indices) * 128 * 128,
                       data, torch.from_numpy(offsets).cuda(),
                       torch.from_numpy(indices).cuda())
    sp.AllocateTransposeBuffers(s)
    sp.Transpose(s)
    torch.cuda.synchronize()
    o_t, i_t, b_o = G.transposed_order(offsets, indices, G.SRC_COLS // 128)
    assert np.array_equal(s.offsets_t.cpu().numpy(), o_t)
    assert np.array_equal(s.indices_t.cpu().numpy(), i_t)
    assert np.array_equal(s.block_offsets.cpu().numpy(), b_o)
    return s, b_o


def block_values(dtype, seed):
    """[8, 128, 128] with the special cases planted in rows and columns."""
    nb = len(G.SRC_TOPOLOGY[1])
    v = T.row_values((nb * 128, 128), dtype, seed).reshape(nb, 128, 128)
    v[3] = v[3].T.copy()        # a block with the special rows as columns
    v[5, :, 9] = 0.0            # an all-zero column tile
    return v


def blocks_call(s, stage, act, z, pow2, rows=True, cols=True):
    nb = s.num_blocks
    out, checks = {}, []
    if rows:
        out["q"], ok = T.guarded((nb, 128, 128), torch.float8_e4m3fn)
        checks.append(ok)
        out["scales"], ok = T.guarded((nb * 128,), torch.float32)
        checks.append(ok)
    if cols:
        out["qt"], ok = T.guarded((nb, 128, 128), torch.float8_e4m3fn)
        checks.append(ok)
        out["scales_t"], ok = T.guarded((nb * 128,), torch.float32)
        checks.append(ok)
    sp.QuantizeBlocks(s, stage=stage, activation=act, z=z, pow2=pow2, **out)
    torch.cuda.synchronize()
    assert all(ok() for ok in checks)
    return out


STAGES = [(None, None), ("act", "relu"), ("act", "gelu"), ("act", "silu"),
          ("act_grad", "relu"), ("act_grad", "gelu"), ("act_grad", "silu")]


@pytest.mark.parametrize("stage,act", STAGES,
                         ids=[f"{s}-{a}" for s, a in STAGES])
@pytest.mark.parametrize("pow2", [False, True], ids=["exact", "pow2"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_quantize_blocks_bit_for_bit(dtype, pow2, stage, act):
    x = block_values(dtype, [83, 1])
    z = block_values(dtype, [83, 2])[::-1].copy()
    dx, dz = T.dev(x, dtype), T.dev(z, dtype)
    s, block_offsets = source(dx)
    nb = s.num_blocks
    # The values a stage quantises are those the 16-bit elementwise kernels
    # store; the existing row quantisers give the row outputs on them.
    q = torch.empty(nb * 128, 128, dtype=torch.float8_e4m3fn, device="cuda")
    sc = torch.empty(nb * 128, 1, device="cuda")
    if stage is None:
        h = dx
        sp.QuantizeRows(dx.view(-1, 128), q, sc, pow2)
    elif stage == "act":
        h = sp.BlockActivation(dx, act)
        sp.QuantizeRows(dx.view(-1, 128), q, sc, pow2, act)
    else:
        h = sp.BlockActivationGrad(dx, dz, act)
        sp.QuantizeRows(h.view(-1, 128), q, sc, pow2)
    got = blocks_call(s, stage, act, dz if stage == "act_grad" else None, pow2)
    assert np.array_equal(bytes_of(got["q"]).reshape(-1, 128), bytes_of(q))
    assert np.array_equal(bits32(got["scales"]), bits32(sc).reshape(-1))
    qt_ref, st_ref = G.quantize_blocks_t(T.host(h), block_offsets, pow2)
    assert np.array_equal(bits32(got["scales_t"]), st_ref.view(np.uint32))
    assert np.array_equal(bytes_of(got["qt"]), qt_ref)
    # a null pair leaves the other pair's bits unchanged
    z_arg = dz if stage == "act_grad" else None
    only_rows = blocks_call(s, stage, act, z_arg, pow2, cols=False)
    only_cols = blocks_call(s, stage, act, z_arg, pow2, rows=False)
    assert np.array_equal(bytes_of(only_rows["q"]), bytes_of(got["q"]))
    assert np.array_equal(bits32(only_rows["scales"]), bits32(got["scales"]))
    assert np.array_equal(bytes_of(only_cols["qt"]), qt_ref)
    assert np.array_equal(bits32(only_cols["scales_t"]),
                          st_ref.view(np.uint32))


def test_quantize_blocks_rejections_and_a_bad_block_offset():
    x = T.dev(block_values("f16", [84]), "f16")
    s, block_offsets = source(x)
    nb = s.num_blocks
    q = torch.full((nb, 128, 128), T.FILL, dtype=torch.uint8, device="cuda")
    sc = torch.full((nb * 128,), 7.0, device="cuda")
    qt = torch.full((nb, 128, 128), T.FILL, dtype=torch.uint8, device="cuda")
    st = torch.full((nb * 128,), 7.0, device="cuda")
    f = sp.lib().sputnik_quantize_blocks

    def call(sm, stage=0, act=0, z=None, q_=q, sc_=sc, qt_=qt, st_=st,
             dtype=0):
        cs = sm._c()
        ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        return f(ctypes.byref(cs), stage, act, ptr(z), ptr(q_), ptr(sc_),
                 ptr(qt_), ptr(st_), 0, dtype, None)

    offsets, indices = s.offsets, s.indices
    plain = sp.BlockMatrix(G.SRC_ROWS, G.SRC_COLS, 128, nb * 128 * 128, x,
                           offsets, indices)
    assert call(plain) == INVALID                       # no block_offsets
    assert call(s, q_=None, sc_=None, qt_=None, st_=None) == INVALID
    assert call(s, sc_=None) == INVALID                 # half a pair
    assert call(s, st_=None) == INVALID
    assert call(s, stage=3) == INVALID
    assert call(s, stage=1, act=9) == INVALID
    assert call(s, stage=2, act=0, z=None) == INVALID   # act_grad needs z
    assert call(s, dtype=2) == INVALID
    assert call(s, q_=x) == INVALID                     # an output is the input
    assert call(s, qt_=q) == INVALID                    # two outputs alias
    odd = sp.BlockMatrix(G.SRC_ROWS, G.SRC_COLS, 64, nb * 128 * 128, x,
                         offsets, indices)
    odd.block_offsets = s.block_offsets
    assert call(odd) == INVALID
    torch.cuda.synchronize()
    assert bool((q == T.FILL).all()) and bool((qt == T.FILL).all())
    assert bool((sc == 7.0).all()) and bool((st == 7.0).all())
    # zero blocks succeed, whatever the pointers
    empty = sp.BlockMatrix(G.SRC_ROWS, G.SRC_COLS, 128, 0, None, offsets, None)
    assert call(empty) == 0
    # the column pair alone, with entries 2 and 6 of block_offsets out of
    # range: those output blocks stay unwritten, the others are right
    bad = block_offsets.copy()
    bad[2], bad[6] = -1, nb
    broken = sp.BlockMatrix(G.SRC_ROWS, G.SRC_COLS, 128, nb * 128 * 128, x,
                            offsets, indices)
    broken.block_offsets = torch.from_numpy(bad).cuda()
    assert call(broken, q_=None, sc_=None) == 0
    torch.cuda.synchronize()
    qt_ref, st_ref = G.quantize_blocks_t(T.host(x), block_offsets)
    got_qt, got_st = qt.cpu().numpy(), st.cpu().numpy().reshape(nb, 128)
    for j in range(nb):
        if j in (2, 6):
            assert (got_qt[j] == T.FILL).all() and (got_st[j] == 7.0).all()
        else:
            assert np.array_equal(got_qt[j], qt_ref[j])
            assert np.array_equal(got_st[j], st_ref.reshape(nb, 128)[j])
    assert bool((q == T.FILL).all()) and bool((sc == 7.0).all())


def test_quantize_tiles_rejections_write_nothing():
    x = torch.ones(SHAPE, dtype=torch.float16, device="cuda")
    m, n = SHAPE
    q = torch.full((m, n), T.FILL, dtype=torch.uint8, device="cuda")
    s = torch.full((m, n // 128), 7.0, device="cuda")
    qt = torch.full((n, m), T.FILL, dtype=torch.uint8, device="cuda")
    st = torch.full((m // 128, n), 7.0, device="cuda")
    f = sp.lib().sputnik_quantize_tiles
    a = (q.data_ptr(), s.data_ptr(), qt.data_ptr(), st.data_ptr())
    assert f(x.data_ptr(), 192, n, *a, 0, 0, None) == INVALID
    assert f(x.data_ptr(), m, 192, *a, 0, 0, None) == INVALID
    assert f(x.data_ptr(), -128, n, *a, 0, 0, None) == INVALID
    assert f(None, m, n, *a, 0, 0, None) == INVALID
    assert f(x.data_ptr(), m, n, None, None, None, None, 0, 0, None) == INVALID
    assert f(x.data_ptr(), m, n, a[0], None, a[2], a[3], 0, 0, None) == INVALID
    assert f(x.data_ptr(), m, n, a[0], a[1], a[2], None, 0, 0, None) == INVALID
    assert f(x.data_ptr(), m, n, x.data_ptr(), a[1], a[2], a[3], 0, 0,
             None) == INVALID
    assert f(x.data_ptr(), m, n, *a, 0, 2, None) == INVALID
    assert f(None, 0, n, None, None, None, None, 0, 0, None) == INVALID
    assert f(None, 0, n, *a, 0, 0, None) == 0           # zero-sized work
    torch.cuda.synchronize()
    assert bool((q == T.FILL).all()) and bool((qt == T.FILL).all())
    assert bool((s == 7.0).all()) and bool((st == 7.0).all())


# ---- the weight transpose -------------------------------------------------------------

@pytest.mark.parametrize("pow2", [False, True], ids=["exact", "pow2"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_transpose_weight_equals_quantize_weight_of_the_transpose(dtype, pow2):
    k, n = 256, 384
    w = M.values((k, n), dtype, [85, k, n])
    w *= np.exp2(3 * (np.arange(k)[:, None] // 128)
                 - np.arange(n)[None, :] // 128).astype(np.float32)
    w[:128, 128:256] = 0.0
    w[200, 300], w[130, 5] = np.nan, -np.inf
    dw = T.dev(w, dtype)
    q = torch.empty(n, k, dtype=torch.float8_e4m3fn, device="cuda")
    s = torch.empty(k // 128, n // 128, device="cuda")
    sp.QuantizeWeight(dw, q, s, False, pow2)
    # the weight w^T [n, k], from the same buffer read as its transpose
    want_q = torch.empty(k, n, dtype=torch.float8_e4m3fn, device="cuda")
    want_s = torch.empty(n // 128, k // 128, device="cuda")
    sp.QuantizeWeight(dw, want_q, want_s, True, pow2)
    for offset in (0, 1):
        qt, qt_ok = T.guarded((k, n), torch.float8_e4m3fn, offset)
        st, st_ok = T.guarded((n // 128, k // 128), torch.float32)
        sp.TransposeWeightFp8(q, s, qt, st)
        torch.cuda.synchronize()
        assert qt_ok() and st_ok()
        assert np.array_equal(bytes_of(qt), bytes_of(want_q)), offset
        assert np.array_equal(bits32(st), bits32(want_s)), offset
    ref_q, ref_s = R.quantize_weight(np.ascontiguousarray(w.T), pow2)
    assert np.array_equal(bytes_of(want_q), ref_q)
    assert np.array_equal(bits32(want_s), ref_s.view(np.uint32))
    f = sp.lib().sputnik_fp8_transpose_weight
    fill = torch.full((k, n), T.FILL, dtype=torch.uint8, device="cuda")
    a = (q.data_ptr(), s.data_ptr())
    assert f(*a, 192, n, fill.data_ptr(), want_s.data_ptr(), None) == INVALID
    assert f(*a, k, n, None, want_s.data_ptr(), None) == INVALID
    assert f(*a, k, n, q.data_ptr(), want_s.data_ptr(), None) == INVALID
    assert f(*a, k, n, fill.data_ptr(), s.data_ptr(), None) == INVALID
    assert f(None, None, 0, n, None, None, None) == 0
    torch.cuda.synchronize()
    assert bool((fill == T.FILL).all())
