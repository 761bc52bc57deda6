"""CPU: the MX gradient entry points are exported and reject bad arguments
with hipErrorInvalidValue before any device call: the pointers here are
made-up addresses that nothing may touch."""

import ctypes

import pytest

import sputnik_amd as sp

BAD = sp.hipErrorInvalidValue
X, Q, S, QT, ST, Z, OFF, IDX, BO, C = (0x10000 * (i + 1) for i in range(10))


def test_symbols_are_exported():
    for name in ("QuantizeTilesMx", "QuantizeBlocksMx", "DsdMxWgrad"):
        assert callable(getattr(sp, name)) and name in sp.__all__
    for name in ("sputnik_quantize_tiles_mx", "sputnik_quantize_blocks_mx",
                 "sputnik_dsd_mx_wgrad"):
        assert hasattr(sp.lib(), name)


@pytest.mark.parametrize("args", [
    dict(q=None, s=None, qt=None, st=None), dict(s=None), dict(qt=None),
    dict(rows=192), dict(cols=32), dict(rows=-128), dict(dtype=2),
    dict(x=None), dict(q=X), dict(qt=Q)], ids=str)
def test_quantize_tiles_mx_rejections(args):
    a = dict(x=X, rows=256, cols=384, q=Q, s=S, qt=QT, st=ST, dtype=0)
    f = sp.lib().sputnik_quantize_tiles_mx
    assert f(*{**a, **args}.values(), None) == BAD


def block_matrix(data=X, nonzeros=8 * 128 * 128, block=128, block_offsets=BO):
    s = sp._CBlockMatrix()
    s.rows, s.cols, s.block_size, s.nonzeros = 768, 512, block, nonzeros
    s.data, s.offsets, s.indices, s.block_offsets = data, OFF, IDX, block_offsets
    return s


@pytest.mark.parametrize("m,args", [
    ({}, dict(q=None, s=None, qt=None, st=None)), ({}, dict(s=None)),
    ({}, dict(stage=3, act=1)), ({}, dict(stage=-1)), ({}, dict(stage=1, act=3)),
    ({}, dict(stage=2, act=-1, z=Z)), ({}, dict(stage=2, act=2)),
    ({}, dict(q=X)), ({}, dict(qt=BO)), ({}, dict(stage=2, act=2, z=Z, st=Z)),
    ({}, dict(dtype=5)), (dict(block_offsets=None), {}),
    (dict(nonzeros=100), {}), (dict(block=64), {}), (dict(data=None), {})],
    ids=str)
def test_quantize_blocks_mx_rejections(m, args):
    a = dict(stage=0, act=0, z=None, q=Q, s=S, qt=QT, st=ST, dtype=0)
    s = block_matrix(**m)
    assert sp.lib().sputnik_quantize_blocks_mx(
        ctypes.byref(s), *{**a, **args}.values(), None) == BAD


@pytest.mark.parametrize("args", [
    dict(s_s=None), dict(b=None), dict(b_s=None), dict(c=None),
    dict(cols=192), dict(rows=640), dict(out=2), dict(out=-1), dict(dtype=2),
    dict(c=X), dict(c=QT), dict(c=ST), dict(c=OFF),      # C is an input
    dict(c=C + 8), dict(b=QT + 4),                       # 16-byte operands
    dict(s_s=S + 2), dict(b_s=ST + 1), dict(block=64)], ids=str)
def test_dsd_mx_wgrad_rejections(args):
    a = dict(s_s=S, b=QT, b_s=ST, c=C, cols=256, rows=768, out=0, dtype=0,
             block=128)
    a.update(args)
    s = block_matrix(block=a["block"])
    c = sp._CMatrix(a["rows"], a["cols"], a["c"])
    assert sp.lib().sputnik_dsd_mx_wgrad(
        ctypes.byref(s), a["s_s"], a["b"], a["b_s"], ctypes.byref(c),
        a["out"], 0, a["dtype"], None) == BAD
