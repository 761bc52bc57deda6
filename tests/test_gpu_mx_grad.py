"""GPU: the MX gradient pieces (sputnik/block/mx.h, "Gradients") against
tests/mx_grad_ref.py: QuantizeTilesMx and QuantizeBlocksMx bit for bit, and
DsdMxWgrad on a known answer (one-hot rows per 32-token group, scales that
differ per (row, group) and (column, group)) and on random data within the
header's bound, for both output types with and without `add`."""

import numpy as np
import pytest
import torch

import sputnik_amd as sp
from tests import fp8_grad_ref as G
from tests import fp8_ref as F
from tests import mx_grad_ref as MG
from tests import mx_ref as R
from tests import rounding_ref as RR
from tests.test_gpu_fp8 import dev, guarded, host
from tests.test_gpu_fp8_grad_quantize import block_values, source
from tests.test_gpu_mx import (ULP, cuda, dsd_call, exact, kat,
                               random_operands, stored)

pytestmark = pytest.mark.gpu

DTYPES = ["f16", "bf16"]
E4M3 = torch.float8_e4m3fn
PAIRS = [(True, True), (True, False), (False, True)]
TOPOLOGY = G.wgrad_topology()     # 4 x 6 blocks: rows of 5, 0, 2 and 1 steps
M_, K_, N_ = G.SRC_COLS, G.SRC_ROWS, G.WGRAD_N


def raw(t):
    return t.view(torch.uint8).cpu().numpy()


def check_pairs(call, shapes, want, rows, cols):
    """call(**outputs) into guarded buffers of the pairs asked for."""
    out, checks = {}, []
    for name, shape, on in zip(("q", "scales", "qt", "scales_t"), shapes,
                               (rows, rows, cols, cols)):
        if on:
            out[name], ok = guarded(shape, torch.uint8 if "scales" in name
                                    else E4M3)
            checks.append(ok)
    call(**out)
    torch.cuda.synchronize()
    assert all(ok() for ok in checks)
    for name, got in out.items():
        assert np.array_equal(raw(got), want[name]), (name, rows, cols)


@pytest.mark.parametrize("dtype", DTYPES)
def test_quantize_tiles_bit_for_bit(dtype):
    rng = np.random.default_rng(11)    # every 32-group spans many binades
    x = rng.standard_normal((256, 384)) * np.exp2(
        rng.integers(-10, 6, (256, 384)))
    x = np.asarray(RR.round_once(x, dtype), np.float32)
    x[32:64, 5] = 0.0                       # an all-zero 32 x 1 group
    x[3, 7], x[100, 200] = np.nan, -np.inf
    x[128:160, 9:11] = 0.25                 # amax on / above the m = 0.875 edge
    x[130, 9], x[130, 10] = 0.875 * 4, (0.875 + ULP[dtype]) * 4
    rows, cols = x.shape
    want = dict(zip(("q", "scales", "qt", "scales_t"),
                    R.quantize(x) + MG.quantize_cols(x)))
    qt, st = want["qt"], want["scales_t"]
    assert st[5, 1] == 1 and not qt[5, 32:64].any()
    assert qt[7, 3] == 0x7F and qt[200, 100] == 0xFF
    assert st[10, 4] == st[9, 4] + 1 and qt[9, 130] == 0x7E
    shapes = ((rows, cols), (rows, cols // 32), (cols, rows), (cols, rows // 32))
    dx = dev(x, dtype)
    for which in PAIRS:
        check_pairs(lambda **o: sp.QuantizeTilesMx(dx, **o), shapes, want,
                    *which)
    # both pairs null: rejected (nothing to write to)
    assert sp.lib().sputnik_quantize_tiles_mx(
        dx.data_ptr(), rows, cols, None, None, None, None, 0,
        None) == sp.hipErrorInvalidValue


@pytest.mark.parametrize("stage,act", [(None, None), ("act", "gelu"),
                                       ("act_grad", "gelu")],
                         ids=["none", "gelu", "gelu-grad"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_quantize_blocks_bit_for_bit(dtype, stage, act):
    dx = dev(block_values(dtype, [84, 1]), dtype)
    dz = dev(block_values(dtype, [84, 2])[::-1].copy(), dtype)
    s, block_offsets = source(dx)
    nb = s.num_blocks
    # the staged values as the 16-bit elementwise kernels store them, and
    # QuantizeRowsMx's bits on them
    q = torch.empty(nb * 128, 128, dtype=E4M3, device="cuda")
    sc = torch.empty(nb * 128, 4, dtype=torch.uint8, device="cuda")
    if stage == "act_grad":
        h = sp.BlockActivationGrad(dx, dz, act)
        sp.QuantizeRowsMx(h.view(-1, 128), q, sc)
    else:
        h = dx if stage is None else sp.BlockActivation(dx, act)
        sp.QuantizeRowsMx(dx.view(-1, 128), q, sc, act)
    want = dict(zip(("q", "scales", "qt", "scales_t"),
                    (raw(q).reshape(nb, 128, 128), raw(sc))
                    + MG.quantize_blocks_t(host(h), block_offsets)))
    shapes = ((nb, 128, 128), (nb * 128, 4)) * 2
    z = dz if stage == "act_grad" else None

    def call(sm=s, **o):
        sp.QuantizeBlocksMx(sm, stage=stage, activation=act, z=z, **o)
    for which in PAIRS:
        check_pairs(call, shapes, want, *which)
    plain = sp.BlockMatrix(s.rows, s.cols, 128, s.nonzeros, dx, s.offsets,
                           s.indices)
    with pytest.raises(sp.SputnikError):    # columns need block_offsets
        call(plain, qt=q.view(nb, 128, 128), scales_t=sc)


def wgrad_call(aq, sa, wq, sw, c_old, out, dtype, add):
    """DsdMxWgrad over TOPOLOGY's blocks of the dense aq [m, k] / sa [m, k /
    32] into a sink of `out` holding c_old; the sink as float64 values."""
    offsets, indices = TOPOLOGY
    nb = len(indices)
    sq = F.blocks_from_dense(aq, offsets, indices)
    ss = F.blocks_from_dense(np.repeat(sa, 32, axis=1), offsets,
                             indices)[:, :, ::32].reshape(nb * 128, 4)
    s = sp.BlockMatrix(M_, K_, 128, nb * 128 * 128, cuda(sq, E4M3),
                       cuda(offsets), cuda(indices))
    c = (torch.from_numpy(c_old.astype(np.float32)).cuda() if out == "f32"
         else dev(c_old, dtype))
    sp.DsdMxWgrad(s, cuda(ss), cuda(wq, E4M3), cuda(sw), sp.Matrix(M_, N_, c),
                  add)
    torch.cuda.synchronize()
    return c.double().cpu().numpy()


def rounded(value64, out, dtype):
    r = value64.astype(np.float32) if out == "f32" else RR.round_once(
        value64, dtype)
    return np.asarray(r, np.float64)


CASES = [(d, o, a) for d in DTYPES for o in (d, "f32") for a in (False, True)]


@pytest.mark.parametrize("dtype,out,add", CASES)
def test_wgrad_known_answer(dtype, out, add):
    o = kat(M_, K_, N_, "e4m3", 9)
    # multiples of 2^-4 below 2^14; with c_old a small integer the sum is
    # exact in fp32 and is rounded once
    ref = exact(*o, "e4m3", stored(M_, K_, TOPOLOGY))[0]
    c_old = np.random.default_rng(12).integers(-8, 9, ref.shape).astype(
        np.float64)
    got = wgrad_call(*o, c_old, out, dtype, add)
    want = rounded(ref + c_old if add else ref, out, dtype)
    if add:
        want[128:256] = c_old[128:256]      # the empty block row: untouched
    assert np.array_equal(got, want)
    assert not np.signbit(got[128:256]).any() or add    # +0 rows


@pytest.mark.parametrize("dtype,out,add", CASES)
def test_wgrad_random_within_bound(dtype, out, add):
    o = random_operands(M_, K_, N_, "e4m3", dtype, [13, 1])
    ref, absum = exact(*o, "e4m3", stored(M_, K_, TOPOLOGY))
    c_old = np.asarray(RR.round_once(np.random.default_rng(14).standard_normal(
        ref.shape), dtype), np.float64)
    got, again = (wgrad_call(*o, c_old, out, dtype, add) for _ in range(2))
    assert np.array_equal(got, again)
    k_row = np.repeat(np.diff(TOPOLOGY[0]) * 128, 128)[:, None]
    if add:     # C_old is one of the terms; an empty row is left alone
        ref, absum = ref + c_old, absum + np.abs(c_old)
        assert np.array_equal(got[128:256], c_old[128:256])
    err, lim = np.abs(got - ref), MG.bound(ref, absum, k_row, out, add)
    print(f"{dtype} {out} add={add}: worst error / bound = "
          f"{float((err / np.maximum(lim, 1e-300)).max()):.3f}")
    assert (err <= lim).all()
    if out == dtype and not add:    # DsdMx's bits
        assert np.array_equal(got, host(dsd_call(*o, "e4m3", dtype, TOPOLOGY)))
