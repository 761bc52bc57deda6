"""GPU: DsdMxPair (sputnik/block/mx.h) bit for bit against DsdMx over the
host-built concatenation [S1 | S2] . [B1; B2], and within the header's bound
of the float64 product of the decoded operands. The topology has block rows
of 5, 0, 2 and 1 stored blocks: the second pair starts in the other ring stage
(odd) and in the same one (even), and one row is empty."""

import ctypes

import numpy as np
import pytest
import torch

import sputnik_amd as sp
from tests import fp8_grad_ref as G
from tests import fp8_ref as F
from tests import helpers as H
from tests.test_gpu_fp8 import host
from tests.test_gpu_mx import (check_random, cuda, dsd_call, exact,
                               random_operands, stored)

pytestmark = pytest.mark.gpu

E4M3 = torch.float8_e4m3fn
OFFSETS, INDICES = G.wgrad_topology()
M_, K_, N_ = G.SRC_COLS, G.SRC_ROWS, G.WGRAD_N      # 4 x 6 blocks, n = 256
KB = K_ // 128


def operands(dtype):
    """Two operand sets whose bytes and scales differ, and their concatenation
    along k with its topology: each row's blocks, pair 1's then pair 2's."""
    o1 = random_operands(M_, K_, N_, "e4m3", dtype, [21, 1])
    o2 = random_operands(M_, K_, N_, "e4m3", dtype, [21, 2])
    assert all((a != b).any() for a, b in zip(o1, o2))
    rows = np.split(INDICES, OFFSETS[1:-1])
    both = (2 * OFFSETS, np.concatenate([np.concatenate([r, r + KB])
                                         for r in rows]).astype(np.int16))
    return o1, o2, [np.concatenate(p, axis=1) for p in zip(o1, o2)], both


def blocks(aq, sa, drop=None):
    """(bytes [nb, 128, 128], scales [nb * 128, 4]) of the stored blocks."""
    sq = F.blocks_from_dense(aq, OFFSETS, INDICES)
    ss = F.blocks_from_dense(np.repeat(sa, 32, axis=1), OFFSETS,
                             INDICES)[:, :, ::32]
    if drop is not None:
        sq, ss = np.delete(sq, drop, axis=0), np.delete(ss, drop, axis=0)
    return cuda(sq, E4M3), cuda(ss.reshape(-1, 4))


def pair_call(o1, o2, dtype, out=None, topo=(OFFSETS, INDICES), drop=None):
    (s1, ss1), (s2, ss2) = (blocks(*o[:2], drop=drop) for o in (o1, o2))
    if out is None:
        out = torch.empty(M_, N_, dtype=H.torch_dtype(dtype), device="cuda")
    s = sp.BlockMatrix(M_, K_, 128, s1.numel(), s1, cuda(topo[0]),
                       cuda(topo[1]))
    sp.DsdMxPair(s, ss1, cuda(o1[2], E4M3), cuda(o1[3]), s2, ss2,
                 cuda(o2[2], E4M3), cuda(o2[3]), sp.Matrix(M_, N_, out))
    return out


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_pair_equals_dsd_over_the_concatenation(dtype):
    o1, o2, cat, both = operands(dtype)
    ref, absum = exact(*cat, "e4m3", stored(M_, 2 * K_, both))
    got = check_random(lambda out: pair_call(o1, o2, dtype, out), (M_, N_),
                       ref, absum, 2 * K_, dtype)
    want = dsd_call(*cat, "e4m3", dtype, both)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert not got[128:256].view(torch.int16).any()        # +0 rows
    # the pairs are told apart: S2 with B1 and S1 with B2 is another result
    swapped = pair_call(o2[:2] + o1[2:], o1[:2] + o2[2:], dtype)
    assert not torch.equal(swapped, got)
    # block 2 of row 0 under an index out of range: as if it were not stored,
    # in both pairs
    for bad in (KB, -1):
        indices = INDICES.copy()
        indices[2] = bad
        less = OFFSETS - np.array([0, 1, 1, 1, 1], np.int32)
        assert torch.equal(
            pair_call(o1, o2, dtype, topo=(OFFSETS, indices)).view(torch.int16),
            pair_call(o1, o2, dtype, topo=(less, np.delete(INDICES, 2)),
                      drop=2).view(torch.int16))


def test_pair_rejections():
    o1, o2, _, _ = operands("f16")
    with pytest.raises(ValueError):         # the weights differ in shape
        pair_call(o1, o2[:2] + (o2[2][:128], o2[3][:128]), "f16")
    (s1, ss1), (s2, ss2) = (blocks(*o[:2]) for o in (o1, o2))
    w = [cuda(o[2], E4M3) for o in (o1, o2)]
    sw = [cuda(o[3]) for o in (o1, o2)]
    y = torch.full((M_, N_), 7.0, dtype=torch.float16, device="cuda")
    s = sp.BlockMatrix(M_, K_, 128, s1.numel(), s1, cuda(OFFSETS),
                       cuda(INDICES))

    def call(s2_data=s2.data_ptr(), b2=w[1].data_ptr(), c=y.data_ptr()):
        cs, cm = s._c(), sp._CMatrix(M_, N_, c)
        return sp.lib().sputnik_dsd_mx_pair(
            ctypes.byref(cs), ss1.data_ptr(), w[0].data_ptr(),
            sw[0].data_ptr(), s2_data, ss2.data_ptr(), b2, sw[1].data_ptr(),
            ctypes.byref(cm), 0, None)

    bad = sp.hipErrorInvalidValue
    assert call(b2=w[1].data_ptr() + 8) == bad              # misaligned Bq
    assert call(c=s2.data_ptr()) == bad and call(c=w[0].data_ptr()) == bad
    assert call(s2_data=None) == bad
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    assert call() == sp.hipSuccess
    torch.cuda.synchronize()
    assert torch.equal(y, pair_call(o1, o2, "f16"))
