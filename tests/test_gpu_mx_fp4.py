"""GPU: MXFP4 activations (sputnik/block/mx.h) against tests/mx_ref.py: the
quantiser bit for bit, known-answer A4W4 products, the bound on random data,
NaN scales, bad indices, rejections and ops.moe_mlp_mx_fp4."""

import ctypes

import numpy as np
import pytest
import torch

import sputnik_amd as sp
from sputnik_amd import ops
from tests import fp8_ref as F
from tests import helpers as H
from tests import moe_ref as M
from tests import mx_ref as R
from tests import rounding_ref as RR
from tests.test_gpu_fp8 import dev, guarded, host
from tests.test_gpu_mx import (FULL, SDD_TOPOLOGY, STAGES, ULP, check_random,
                               cuda, kat_operand, stored)

pytestmark = pytest.mark.gpu

DTYPES = ["f16", "bf16"]
# 5 x 5 blocks: block rows of 0, 1, 2, 3 and 4 stored blocks, unordered
LADDER = (np.array([0, 0, 1, 3, 6, 10], np.int32),
          np.array([3, 4, 0, 2, 0, 1, 1, 4, 2, 0], np.int16))


def quantiser_values(shape, dtype, seed):
    """Values of T whose 32-blocks spread over 18 binades, specials planted."""
    rng = np.random.default_rng(seed)
    rows, cols = shape
    spread = np.exp2(rng.integers(-10, 8, (rows, cols // 32)))
    x = RR.round_once(rng.standard_normal(shape) * np.repeat(spread, 32, 1),
                      dtype).astype(np.float32)
    x[0, :32] = 0.0     # amax 6 = 0.75 * 2^3: s = 1, then the ties
    x[0, :8] = [6, 0.25, 0.75, 1.25, 2.5, 5, -0.25, -2.5]
    x[1, :64] = 0.125   # amax on and just above m = 0.75
    x[1, 0], x[1, 32] = 0.75 * 8, (0.75 + ULP[dtype]) * 8
    x[2, :32] = 0.0
    x[3, 10], x[3, 11] = 0.0, -0.0
    tiny = 2.0 ** -133 if dtype == "bf16" else 2.0 ** -24
    x[3, 32:64] = tiny * np.arange(-16, 16)
    x[4, 5], x[4, 40], x[5, 70] = np.nan, np.inf, -np.inf
    return x


@pytest.mark.parametrize("stage", STAGES, ids=lambda s: "-".join(s or ["plain"]))
@pytest.mark.parametrize("dtype", DTYPES)
def test_quantize_rows_fp4_bit_for_bit(dtype, stage):
    for n, shape in enumerate([(256, 384), (2 * 128, 128)]):  # rows; blocks
        x = quantiser_values(shape, dtype, [1, n])
        g = quantiser_values(shape, dtype, [2, n])[::-1].copy()
        dx, dg = dev(x, dtype), dev(g, dtype)
        kind, act = stage or (None, None)
        h = x if kind is None else host(
            sp.BlockActivation(dx, act) if kind == "act"
            else sp.BlockGate(dx, dg, act))
        c_ref, s_ref = R.quantize(h, e2m1=True)
        q, q_ok = guarded((shape[0], shape[1] // 2), torch.uint8)
        s, s_ok = guarded((shape[0], shape[1] // 32), torch.uint8)
        sp.QuantizeRowsMxFp4(dx, q, s, act, dg if kind == "gate" else None)
        torch.cuda.synchronize()
        assert np.array_equal(s.cpu().numpy(), s_ref), (shape, stage)
        assert np.array_equal(q.cpu().numpy(), R.pack(c_ref)), (shape, stage)
        assert q_ok() and s_ok()
        if kind is None:
            assert list(c_ref[0, :8]) == [7, 0, 2, 2, 4, 6, 8, 12]
            assert s_ref[1, 1] == s_ref[1, 0] + 1 and s_ref[2, 0] == 1
            # (bf16's subnormals lie under the scale floor: all +-0)
            assert (c_ref[3, 32:64] & 7).any() == (dtype == "f16")
            assert [s_ref[4, 0], s_ref[4, 1], s_ref[5, 2]] == [255] * 3
            assert s_ref[4, 2] != 255                 # the neighbour
            assert not c_ref[4, :64].any() and c_ref[4, 64:96].any()


def sdd4(ac, sa, wc, sw, dtype, topo, out=None):
    nb, td = len(topo[1]), H.torch_dtype(dtype)
    out = torch.empty(nb, 128, 128, dtype=td, device="cuda") if out is None \
        else out
    c = sp.BlockMatrix(ac.shape[0], wc.shape[0], 128, nb * 128 * 128, out,
                       cuda(topo[0]), cuda(topo[1]))
    c.row_indices = cuda(F.row_indices(topo[0]))
    sp.SddMxFp4(cuda(R.pack(ac)), cuda(sa), cuda(R.pack(wc)), cuda(sw), c)
    return out


def dsd4(ac, sa, wc, sw, dtype, topo, out=None, indices=None):
    # (the stored blocks are cut from the dense ac / sa; `indices` replaces
    # the topology's on the device)
    m, k, n, nb = ac.shape[0], ac.shape[1], wc.shape[0], len(topo[1])
    sq = R.pack(F.blocks_from_dense(ac, *topo).reshape(-1, 128))
    ss = F.blocks_from_dense(np.repeat(sa, 32, axis=1),
                             *topo)[:, :, ::32].reshape(nb * 128, 4)
    out = torch.empty(m, n, dtype=H.torch_dtype(dtype), device="cuda") \
        if out is None else out
    s = sp.BlockMatrix(m, k, 128, nb * 128 * 128, cuda(sq.reshape(nb, 128, 64)),
                       cuda(topo[0]),
                       cuda(topo[1] if indices is None else indices))
    sp.DsdMxFp4(s, cuda(ss), cuda(R.pack(wc)), cuda(sw), sp.Matrix(m, n, out))
    return out


def kat4(m, k, n, seed):
    """test_gpu_mx.kat with both sides e2m1: the dense rows keep {1, 2} x {1}
    under its scale ramps; the one-hot rows (every nibble position of both
    operands) run through the seven nonzero magnitudes."""
    ac, sa = kat_operand(m, k, [1.0, 2.0], lambda r, b: (r + 3 * b) % 5 - 2,
                         [seed, 1], True)
    wc, sw = kat_operand(n, k, [1.0], lambda c, b: (c % 5 + b) % 4 - 2,
                         [seed, 2], True)
    ramp = 1 + (np.arange(32)[:, None] + np.arange(k)[None, :] // 32) % 7
    for codes in (ac, wc):
        codes[:32] = np.where(codes[:32] & 7, (codes[:32] & 8) | ramp, 0)
    return ac, sa, wc, sw


def exact4(ac, sa, wc, sw, mask=True):
    return R.matmul64(np.where(mask, R.decode(ac, sa, True), 0.0),
                      R.decode(wc, sw, True))


# k: a half stage alone; one stage; a stage and a half; the ring wraps, + half
@pytest.mark.parametrize("k", [128, 256, 384, 640])
@pytest.mark.parametrize("dtype", DTYPES)
def test_known_answer_sdd(dtype, k):
    o = kat4(256, k, 256, k)
    want = RR.round_once(exact4(*o)[0], dtype)
    assert np.array_equal(
        RR.bits(host(sdd4(*o, dtype, SDD_TOPOLOGY)), dtype),
        RR.bits(F.blocks_from_dense(want, *SDD_TOPOLOGY), dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_known_answer_dsd(dtype):
    o = kat4(640, 640, 256, 7)
    want = RR.round_once(exact4(*o, stored(640, 640, LADDER))[0], dtype)
    bits = RR.bits(host(dsd4(*o, dtype, LADDER)), dtype)
    assert np.array_equal(bits, RR.bits(want, dtype))
    assert not bits[:128].any()  # +0 rows


def random4(m, k, n, dtype, seed):
    """test_gpu_mx.random_operands with both sides e2m1."""
    rng = np.random.default_rng(seed)
    spread = np.exp2(rng.integers(-13, 3, (m + n, k // 32)))
    x = rng.standard_normal((m + n, k)) * np.repeat(spread, 32, axis=1)
    c, s = R.quantize(RR.round_once(x, dtype), True)
    return c[:m], s[:m], c[m:], s[m:]


@pytest.mark.parametrize("dtype", DTYPES)
def test_random_within_bound(dtype):
    k = 640
    o = random4(256, k, 256, dtype, [5, k])
    ref, absum = exact4(*o)
    check_random(lambda out: sdd4(*o, dtype, SDD_TOPOLOGY, out),
                 (3, 128, 128), F.blocks_from_dense(ref, *SDD_TOPOLOGY),
                 F.blocks_from_dense(absum, *SDD_TOPOLOGY), k, dtype)
    # SDD on the full topology and DSD over the same bytes: the same bits
    every = (np.array([0, 5, 10], np.int32), np.arange(10, dtype=np.int16) % 5)
    assert np.array_equal(
        RR.bits(host(sdd4(*o, dtype, FULL)), dtype),
        RR.bits(F.blocks_from_dense(host(dsd4(*o, dtype, every)), *FULL),
                dtype))
    o = random4(640, k, 256, dtype, [6, k])
    ref, absum = exact4(*o, stored(640, k, LADDER))
    check_random(lambda out: dsd4(*o, dtype, LADDER, out), (640, 256), ref,
                 absum, k, dtype)


def test_nan_scale_reaches_its_row_or_column_only():
    ac, sa, wc, sw = kat4(256, 384, 256, 9)
    sa[5, 7] = 0xFF              # A: row 5, second half of stage 0
    sw[130, 9] = 0xFF            # B: column 130, the half stage
    want = np.zeros((256, 256), bool)
    want[5, :] = want[:, 130] = True
    got = host(sdd4(ac, sa, wc, sw, "bf16", FULL))
    assert np.array_equal(np.isnan(got), F.blocks_from_dense(want, *FULL))
    every = (np.array([0, 3, 6], np.int32), np.arange(6, dtype=np.int16) % 3)
    assert np.array_equal(np.isnan(host(dsd4(ac, sa, wc, sw, "bf16", every))),
                          want)


@pytest.mark.parametrize("bad", [(6, 9), (7, -1)],
                         ids=["first-half", "second-half"])
def test_out_of_range_index_contributes_zero(bad):
    at, index = bad              # block row 4 is stored blocks 6 .. 9
    o = kat4(640, 640, 256, 11)
    indices = LADDER[1].copy()
    mask = stored(640, 640, LADDER)
    mask[512:, 128 * indices[at]:128 * indices[at] + 128] = False
    indices[at] = index
    want = RR.round_once(exact4(*o, mask)[0], "f16")
    got = host(dsd4(*o, "f16", LADDER, indices=indices))
    assert np.array_equal(RR.bits(got, "f16"), RR.bits(want, "f16"))


def test_rejections_leave_the_output_untouched():
    L, bad = sp.lib(), sp.hipErrorInvalidValue
    stream = torch.cuda.current_stream().cuda_stream
    out = torch.full((4, 128, 128), 7.0, dtype=torch.float16, device="cuda")
    y = torch.full((256, 256), 7.0, dtype=torch.float16, device="cuda")
    aq = torch.zeros(256, 128, dtype=torch.uint8, device="cuda")
    wq = torch.zeros(256 * 128 + 16, dtype=torch.uint8, device="cuda")
    sa = torch.full((256, 8), 127, dtype=torch.uint8, device="cuda")
    offsets, indices = cuda(FULL[0]), cuda(FULL[1])
    row_indices = cuda(F.row_indices(FULL[0]))

    def sdd(a_s=sa.data_ptr(), k=256, b=wq.data_ptr(), data=out):
        c = sp.BlockMatrix(256, 256, 128, 4 * 128 * 128, data, offsets, indices)
        c.row_indices = row_indices
        cc = c._c()
        return L.sputnik_sdd_mx_fp4(aq.data_ptr(), a_s, k, b, sa.data_ptr(),
                                    ctypes.byref(cc), 0, stream)

    def dsd(cols=256, s_s=sa.data_ptr(), b=wq.data_ptr(), c_ptr=y.data_ptr()):
        s = sp.BlockMatrix(256, cols, 128, 4 * 128 * 128, aq, offsets, indices)
        cs, cm = s._c(), sp._CMatrix(256, 256, c_ptr)
        return L.sputnik_dsd_mx_fp4(ctypes.byref(cs), s_s, b, sa.data_ptr(),
                                    ctypes.byref(cm), 0, stream)

    # a null buffer, k off the tile, a misaligned operand, an aliased output
    assert sdd(a_s=None) == bad and sdd(k=192) == bad
    assert sdd(b=wq.data_ptr() + 8) == bad and sdd(data=aq) == bad
    assert dsd(s_s=None) == bad and dsd(cols=192) == bad
    assert dsd(b=wq.data_ptr() + 8) == bad and dsd(c_ptr=aq.data_ptr()) == bad
    assert L.sputnik_quantize_rows_mx_fp4(y.data_ptr(), None, 4, 192, 0, 0,
                                          out.data_ptr(), sa.data_ptr(), 0,
                                          stream) == bad
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((y == 7.0).all())
    assert sdd() == sp.hipSuccess and dsd() == sp.hipSuccess
    torch.cuda.synchronize()
    assert not out.any() and not y.any()  # zeros times ones


TOKENS, D_MODEL, FFN, EXPERTS, TOP_K = 300, 256, 256, 4, 2


def layer64(x, w1, w2, v1, top, ew, dtype, q=lambda a: a):
    """The expert layer in float64 on values of T (G, U and H rounded to T);
    `q` is what a product does to an operand [rows, k] first."""
    out = np.zeros((TOKENS, D_MODEL))
    for e in range(EXPERTS):
        cols = slice(e * FFN, (e + 1) * FFN)
        g, u = (w if w is None else RR.round_once(
            q(x) @ q(w[:, cols].T).T, dtype).astype(np.float64)
            for w in (w1, v1))
        h = (g / (1 + np.exp(-2 * np.sqrt(2 / np.pi) * (g + 0.044715 * g ** 3)))
             if u is None else u * g / (1 + np.exp(-g)))
        y = q(RR.round_once(h, dtype).astype(np.float64)) @ q(w2[cols].T).T
        out += sum(np.where(top[:, j] == e, ew[:, j], 0)
                   for j in range(TOP_K))[:, None] * y
    return out


def e2m1_round_trip(a):  # tests/mx_ref's MXFP4 of an operand [rows, k]
    return R.decode(*R.quantize(a.astype(np.float32), True), True)


@pytest.mark.parametrize("glu", [False, True], ids=["mlp", "glu"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_moe_mlp_mx_fp4_equals_its_chain_and_has_the_formats_error(dtype, glu):
    td, hidden = H.torch_dtype(dtype), EXPERTS * FFN
    xh = M.values((TOKENS, D_MODEL), dtype, [21])
    wh = [M.values(s, dtype, [22, i]) / np.float32(16)
          for i, s in enumerate([(D_MODEL, hidden), (hidden, D_MODEL),
                                 (D_MODEL, hidden)])]
    toph = M.routing(TOKENS, TOP_K, EXPERTS, "random", seed=5)
    ewh = M.unit_weights(TOKENS * TOP_K, dtype, [23]).reshape(TOKENS, TOP_K)
    x, top, ew = cuda(xh).to(td), cuda(toph), cuda(ewh).to(td)
    w1q, w2q, v1q = (ops.quantize_weight_mx(cuda(w).to(td), format="e2m1")
                     for w in wh)
    v1q = v1q if glu else None
    out = ops.moe_mlp_mx_fp4(x, top, ew, w1q, w2q, EXPERTS, v1q=v1q)
    route = ops.moe_route(top, EXPERTS)
    topo = ops.expert_topology(route.padded_bins, FFN // 128,
                               route.rows // 128, dtype=td)
    xq, xs = ops.quantize_rows_mx_fp4(ops.padded_gather(x, route))
    g = ops.sdd_mx_fp4(xq, xs, w1q, topo, td)
    hq = (ops.quantize_sparse_mx_fp4(ops.sdd_mx_fp4(xq, xs, v1q, topo, td),
                                     "silu", gate=g) if glu
          else ops.quantize_sparse_mx_fp4(g, "gelu"))
    chain = ops.padded_scatter(ops.dsd_mx_fp4(hq, w2q, td), route, ew)
    assert torch.equal(out.view(torch.int16), chain.view(torch.int16))

    args = [None if a is None else a.astype(np.float64) for a in (
        xh, wh[0], wh[1], wh[2] if glu else None)] + [toph, ewh, dtype]
    full, model = layer64(*args), layer64(*args, e2m1_round_trip)
    rel = float(np.linalg.norm(host(out) - full) / np.linalg.norm(full))
    fmt = float(np.linalg.norm(model - full) / np.linalg.norm(full))
    print(f"moe_mlp_mx_fp4 {dtype} {'glu' if glu else 'mlp'}: relative error "
          f"{rel:.5f}, the format's own {fmt:.5f}")
    assert rel <= 2 * fmt
