"""GPU: QuantizeBlocksMxGatedGrad and QuantizeBlocksMxGated (sputnik/block/
mx.h, "Gradients of a gated expert") bit for bit against the numpy MX
quantisation of what BlockGateGrad / BlockGate store, on the 6 x 4 topology
and the planted block values of tests/test_gpu_fp8_grad_quantize.py, and their
rejections."""

import ctypes

import numpy as np
import pytest
import torch

import sputnik_amd as sp
from tests import fp8_grad_ref as G
from tests import mx_grad_ref as MG
from tests import mx_ref as R
from tests import test_gpu_fp8 as T
from tests import test_gpu_fp8_grad_quantize as Q

pytestmark = pytest.mark.gpu

INVALID = 1
NB = len(G.SRC_TOPOLOGY[1])
SHAPES = ((NB, 128, 128), (NB * 128, 4))
GRID = [pytest.mark.parametrize("act", ["relu", "gelu", "silu"]),
        pytest.mark.parametrize("dtype", Q.DTYPES)]


def grid(f):
    for mark in GRID:
        f = mark(f)
    return f


def raw(t):
    return t.view(torch.uint8).cpu().numpy()


def inputs(dtype):
    """D, G and U: three different tensors of planted block values."""
    d = Q.block_values(dtype, [93, 1])
    g = Q.block_values(dtype, [93, 2])[::-1].copy()
    u = np.roll(Q.block_values(dtype, [93, 3]), 3, axis=0)
    return [T.dev(v, dtype) for v in (d, g, u)]


def images(rows=True, cols=True):
    """((q, scales, qt, scales_t) with None for a pair left out, the guards'
    checks)."""
    out, checks = [], []
    for want in (rows, cols):
        for shape, dt in zip(SHAPES, (torch.float8_e4m3fn, torch.uint8)):
            t, ok = T.guarded(shape, dt) if want else (None, lambda: True)
            out.append(t)
            checks.append(ok)
    return tuple(out), checks


def reference(values, block_offsets):
    q, s = R.quantize(np.asarray(values, np.float32).reshape(-1, 128))
    return (q.reshape(SHAPES[0]), s) + MG.quantize_blocks_t(values,
                                                            block_offsets)


def assert_images(got, values, block_offsets):
    for i, (t, ref) in enumerate(zip(got, reference(values, block_offsets))):
        assert t is None or np.array_equal(raw(t), ref), i


@grid
def test_gated_grad_images_bit_for_bit(dtype, act):
    d, g, u = inputs(dtype)
    s, block_offsets = Q.source(d)
    values = [T.host(v) for v in sp.BlockGateGrad(d, g, u, act)]
    wants = [(True,) * 4]
    if (dtype, act) == ("bf16", "silu"):     # each pair alone
        wants += [tuple(i == j for j in range(4)) for i in range(4)]
    for want in wants:
        (dg, ok_g), (du, ok_u) = images(*want[:2]), images(*want[2:])
        sp.QuantizeBlocksMxGatedGrad(s, g, u, act, dg, du)
        torch.cuda.synchronize()
        assert all(ok() for ok in ok_g + ok_u)
        assert_images(dg, values[0], block_offsets)
        assert_images(du, values[1], block_offsets)


@grid
def test_quantize_blocks_gated_bit_for_bit(dtype, act):
    _, g, u = inputs(dtype)
    s, block_offsets = Q.source(u)
    out, checks = images()
    sp.QuantizeBlocksMxGated(s, g, act, *out)
    q = torch.empty(NB * 128, 128, dtype=torch.float8_e4m3fn, device="cuda")
    sc = torch.empty(NB * 128, 4, dtype=torch.uint8, device="cuda")
    sp.QuantizeRowsMx(u.view(-1, 128), q, sc, act, g.view(-1, 128))
    torch.cuda.synchronize()
    assert all(ok() for ok in checks)
    assert np.array_equal(raw(out[0]).reshape(-1, 128), raw(q))
    assert np.array_equal(raw(out[1]), raw(sc))
    h = T.host(sp.BlockGate(u, g, act))
    assert_images((None, None) + out[2:], h, block_offsets)


def test_rejections_and_bad_block_offsets():
    d, g, u = inputs("f16")
    s, block_offsets = Q.source(d)
    outs = [torch.full(SHAPES[i % 2], T.FILL, dtype=torch.uint8, device="cuda")
            for i in range(8)]
    ptr = lambda t: None if t is None else t.data_ptr()        # noqa: E731
    f = sp.lib().sputnik_quantize_blocks_mx_gated_grad

    def call(sm=s, gate=g, up=u, act=2, o=outs, dtype=0):
        cs = sm._c()
        return f(ctypes.byref(cs), ptr(gate), ptr(up), act,
                 *[ptr(t) for t in o], dtype, None)

    def but(i, t):
        return outs[:i] + [t] + outs[i + 1:]

    def matrix(block=128, nnz=NB * 128 * 128, data=d, offs=s.block_offsets):
        m = sp.BlockMatrix(G.SRC_ROWS, G.SRC_COLS, block, nnz, data,
                           s.offsets, s.indices if nnz else None)
        m.block_offsets = offs
        return m

    assert call(gate=None) == INVALID and call(up=None) == INVALID
    assert call(matrix(data=None)) == INVALID
    assert call(o=but(1, None)) == INVALID                # half a pair
    assert call(o=but(6, None)) == INVALID
    assert call(o=[None] * 8) == INVALID
    assert call(act=-1) == INVALID and call(act=3) == INVALID
    assert call(matrix(offs=None)) == INVALID             # columns need them
    assert call(o=but(0, g)) == INVALID                   # an output is G
    assert call(o=but(6, outs[2])) == INVALID             # two outputs alias
    assert call(matrix(block=64)) == INVALID
    assert call(dtype=2) == INVALID
    cs, o4 = s._c(), [ptr(t) for t in outs[:4]]
    for a in ((None, 2, *o4), (ptr(g), 9, *o4), (ptr(g), 2, *[None] * 4),
              (ptr(g), 2, o4[0], None, *o4[2:]), (ptr(g), 2, ptr(d), *o4[1:])):
        assert sp.lib().sputnik_quantize_blocks_mx_gated(
            ctypes.byref(cs), *a, 0, None) == INVALID, a
    torch.cuda.synchronize()
    assert all(bool((t == T.FILL).all()) for t in outs)
    assert call(matrix(nnz=0, data=None)) == 0            # zero blocks
    # the column pairs alone, entries 2 and 6 of block_offsets out of range
    bad = block_offsets.copy()
    bad[2], bad[6] = -1, NB
    o = [None, None, outs[2], outs[3], None, None, outs[6], outs[7]]
    assert call(matrix(offs=torch.from_numpy(bad).cuda()), o=o) == 0
    torch.cuda.synchronize()
    for v, qt, st in zip(sp.BlockGateGrad(d, g, u, "silu"), o[2::4], o[3::4]):
        qt_ref, st_ref = MG.quantize_blocks_t(T.host(v), block_offsets)
        got_qt, got_st = raw(qt), raw(st).reshape(NB, 128, 4)
        for j in range(NB):
            if j in (2, 6):
                assert (got_qt[j] == T.FILL).all() and (got_st[j] == T.FILL).all()
            else:
                assert np.array_equal(got_qt[j], qt_ref[j])
                assert np.array_equal(got_st[j], st_ref.reshape(NB, 128, 4)[j])
    assert all(bool((outs[i] == T.FILL).all()) for i in (0, 1, 4, 5))
