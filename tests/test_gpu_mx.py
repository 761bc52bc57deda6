"""GPU: the MX products (sputnik/block/mx.h) against tests/mx_ref.py: the
quantisers bit for bit, known-answer products (neighbouring 32-blocks under
different scales, one-hot rows per 32-block and nibble: the lane map), the
bound of mx.h on random data, NaN, rejections and ops.moe_mlp_mx."""

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
from tests.test_gpu_fp8 import dev, guarded, host, row_values

pytestmark = pytest.mark.gpu

DTYPES = ["f16", "bf16"]
FORMATS = ["e4m3", "e2m1"]
STAGES = [None, ("act", "gelu"), ("gate", "silu")]
ULP = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}   # of values in [0.5, 1)
DEEP = F.DSD_DEEP_TOPOLOGY        # 4 x 5 blocks: rows of 5, 0, 1, 3, unordered
SDD_TOPOLOGY = (np.array([0, 2, 3], np.int32), np.array([1, 0, 1], np.int16))
FULL = (np.array([0, 2, 4], np.int32), np.array([0, 1, 0, 1], np.int16))


def cuda(a, view=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if view is None else t.view(view)


@pytest.mark.parametrize("stage", STAGES, ids=lambda s: "-".join(s or ["plain"]))
@pytest.mark.parametrize("dtype", DTYPES)
def test_quantize_rows_bit_for_bit(dtype, stage):
    for n, shape in enumerate([(3, 128), (130, 384)]):
        x = row_values(shape, dtype, [1, n])   # NaN, +Inf, zero, +-0, subnormal
        x[0, 64:128] = 0.25
        x[0, 64], x[0, 96] = 0.875 * 4, -(0.875 + ULP[dtype]) * 4  # the edge
        g = row_values(shape, dtype, [2, n])[::-1].copy()
        dx, dg = dev(x, dtype), dev(g, dtype)
        kind, act = stage or (None, None)
        h = x if kind is None else host(
            sp.BlockActivation(dx, act) if kind == "act"
            else sp.BlockGate(dx, dg, act))
        q_ref, s_ref = R.quantize(h)
        q, q_ok = guarded(shape, torch.float8_e4m3fn)
        s, s_ok = guarded((shape[0], shape[1] // 32), torch.uint8)
        sp.QuantizeRowsMx(dx, q, s, act, dg if kind == "gate" else None)
        torch.cuda.synchronize()
        got_q, got_s = q.view(torch.uint8).cpu().numpy(), s.cpu().numpy()
        assert np.array_equal(got_s, s_ref), (shape, stage)
        assert np.array_equal(got_q, q_ref), (shape, stage)
        assert q_ok() and s_ok()
        if kind is None:
            assert got_q[0, 5] == 0x7F and got_q[1, 7] == 0x7F
            assert got_q[0, 10] == 0x00 and got_q[0, 11] == 0x80
            assert got_s[2, 0] == 1 and not got_q[2, :128].any()
            assert got_s[0, 3] == got_s[0, 2] + 1 and got_q[0, 64] == 0x7E


def weight_values(dtype):
    """w^T [n, k] = [384, 256] with the special blocks planted in row 0 .. 7."""
    wt = M.values((384, 256), dtype, [3]) * np.exp2(
        np.arange(256) // 32 - 4).astype(np.float32)
    tiny = 2.0 ** -133 if dtype == "bf16" else 2.0 ** -24
    wt[0, :32] = 0.0
    wt[0, 32:64] = tiny * np.arange(-16, 16)
    wt[1, 0], wt[1, 1], wt[1, 40], wt[1, 70] = 0.0, -0.0, np.nan, np.inf
    for row, edge in ((2, 0.875), (3, 0.75)):
        wt[row, :64] = 0.125
        wt[row, 0], wt[row, 32] = edge * 8, (edge + ULP[dtype]) * 8
    wt[4, :32] = 0.0   # amax 6 = 0.75 * 2^3: s = 1, then the e2m1 ties
    wt[4, :8] = [6, 0.25, 0.75, 1.25, 2.5, 5, -0.25, -2.5]
    return wt


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_quantize_weight_bit_for_bit(dtype, fmt):
    wt = weight_values(dtype)
    n, k = wt.shape
    e2m1 = fmt == "e2m1"
    c_ref, s_ref = R.quantize(wt, e2m1)
    q_ref = R.pack(c_ref) if e2m1 else c_ref
    if e2m1:
        assert list(c_ref[4, :8]) == [7, 0, 2, 2, 4, 6, 8, 12]
        assert s_ref[1, 1] == 0xFF and s_ref[1, 2] == 0xFF
        assert not c_ref[1, 32:96].any() and list(c_ref[1, :2]) == [0, 8]
    else:
        assert c_ref[1, 40] == 0x7F and c_ref[1, 70] == 0x7F
    # zero amax; an amax that is subnormal in T (bf16: the floor at work)
    assert s_ref[0, 0] == 1 and (s_ref[0, 1] == 1) == (dtype == "bf16")
    assert s_ref[2 + e2m1, 1] == s_ref[2 + e2m1, 0] + 1    # on / above the edge
    for transpose in (False, True):
        src = dev(wt if transpose else wt.T, dtype)
        q, q_ok = guarded(q_ref.shape, torch.uint8 if e2m1
                          else torch.float8_e4m3fn)
        s, s_ok = guarded((n, k // 32), torch.uint8)
        sp.QuantizeWeightMx(src, q, s, transpose, fmt)
        torch.cuda.synchronize()
        assert np.array_equal(s.cpu().numpy(), s_ref), transpose
        assert np.array_equal(q.view(torch.uint8).cpu().numpy(), q_ref)
        assert q_ok() and s_ok()


# ---- the products -----------------------------------------------------------

def weight_dev(codes, fmt):
    return (cuda(R.pack(codes)) if fmt == "e2m1"
            else cuda(codes, torch.float8_e4m3fn))


def sdd_call(aq, sa, wc, sw, fmt, dtype, topo, out=None):
    offsets, indices = topo
    nb = len(indices)
    if out is None:
        out = torch.empty(nb, 128, 128, dtype=H.torch_dtype(dtype),
                          device="cuda")
    c = sp.BlockMatrix(aq.shape[0], wc.shape[0], 128, nb * 128 * 128, out,
                       cuda(offsets), cuda(indices))
    c.row_indices = cuda(F.row_indices(offsets))
    sp.SddMx(cuda(aq, torch.float8_e4m3fn), cuda(sa), weight_dev(wc, fmt),
             cuda(sw), c, fmt)
    return out


def dsd_call(aq, sa, wc, sw, fmt, dtype, topo, out=None):
    """aq / sa dense [m, k] / [m, k / 32]: the stored blocks are cut out."""
    offsets, indices = topo
    m, k, n = aq.shape[0], aq.shape[1], wc.shape[0]
    nb = len(indices)
    sq = F.blocks_from_dense(aq, offsets, indices)
    ss = F.blocks_from_dense(np.repeat(sa, 32, axis=1), offsets,
                             indices)[:, :, ::32].reshape(nb * 128, 4)
    if out is None:
        out = torch.empty(m, n, dtype=H.torch_dtype(dtype), device="cuda")
    s = sp.BlockMatrix(m, k, 128, nb * 128 * 128,
                       cuda(sq, torch.float8_e4m3fn), cuda(offsets),
                       cuda(indices))
    sp.DsdMx(s, cuda(ss), weight_dev(wc, fmt), cuda(sw), sp.Matrix(m, n, out),
             fmt)
    return out


def stored(m, k, topo):  # boolean [m, k]: the element lies in a stored block
    return F.dense_from_blocks(m, k, *topo, np.ones(
        (len(topo[1]), 128, 128), bool))


def kat_operand(rows, k, values, expo, seed, e2m1=False):
    """Codes and scales [rows, k]: magnitudes from `values` with random signs;
    row r < 32 is one-hot per 32-block (position r, or 31 - r in odd blocks);
    the scale exponent of (row, block) is expo(row, block)."""
    rng = np.random.default_rng(seed)
    v = rng.choice(values, (rows, k)) * rng.choice([-1.0, 1.0], (rows, k))
    kk = np.arange(k)
    for r in range(32):
        pos = np.where((kk // 32) % 2, 31 - r, r)
        v[r] = np.where(kk % 32 == pos, v[r], 0.0)
    codes = R.encode_e2m1(v) if e2m1 else F.encode(v.astype(np.float32))
    e = expo(np.arange(rows)[:, None], np.arange(k // 32)[None, :])
    return codes, (e + 127).astype(np.uint8)


def kat(m, k, n, fmt, seed):
    # A scales 2^-2 .. 2^2 with period 5 along the rows, B scales 2^-2 .. 2^1
    # with period 20 along the columns; the four blocks of a step differ in
    # both. Products: multiples of 2^-4 of at most 16, within a ratio of 2 *
    # 2^4 * 2^3 = 2^8: every sum of up to 640 of them is exact in fp32.
    aq, sa = kat_operand(m, k, [1.0, 2.0], lambda r, b: (r + 3 * b) % 5 - 2,
                         [seed, 1])
    wc, sw = kat_operand(n, k, [1.0], lambda c, b: (c % 5 + b) % 4 - 2,
                         [seed, 2], fmt == "e2m1")
    return aq, sa, wc, sw


def exact(aq, sa, wc, sw, fmt, mask=None):
    a64 = R.decode(aq, sa)
    if mask is not None:
        a64 = np.where(mask, a64, 0.0)
    return R.matmul64(a64, R.decode(wc, sw, fmt == "e2m1"))


@pytest.mark.parametrize("k", [128, 384, 640])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_known_answer_sdd(dtype, fmt, k):
    ops_ = kat(256, k, 256, fmt, k)
    got = sdd_call(*ops_, fmt, dtype, SDD_TOPOLOGY)
    want = RR.round_once(exact(*ops_, fmt)[0], dtype)
    assert np.array_equal(RR.bits(host(got), dtype), RR.bits(
        F.blocks_from_dense(want, *SDD_TOPOLOGY), dtype))


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_known_answer_dsd(dtype, fmt):
    ops_ = kat(512, 640, 256, fmt, 7)
    got = dsd_call(*ops_, fmt, dtype, DEEP)
    want = RR.round_once(exact(*ops_, fmt, stored(512, 640, DEEP))[0], dtype)
    bits = RR.bits(host(got), dtype)
    assert np.array_equal(bits, RR.bits(want, dtype))
    assert not bits[128:256].any()  # +0 rows


def random_operands(m, k, n, fmt, dtype, seed):
    """Bytes quantised from normal data whose 32-blocks spread over 16
    binades (2^-13 .. 2^2: the sums stay inside fp16)."""
    rng = np.random.default_rng(seed)

    def values(rows):
        spread = np.exp2(rng.integers(-13, 3, (rows, k // 32)))
        x = rng.standard_normal((rows, k)) * np.repeat(spread, 32, axis=1)
        return RR.round_once(x, dtype)
    return R.quantize(values(m)) + R.quantize(values(n), fmt == "e2m1")


def check_random(call, shape, ref, absum, k, dtype):
    pattern = 0x5555
    fill = torch.tensor([pattern], dtype=torch.int16).view(
        H.torch_dtype(dtype)).item()
    runs = []
    for _ in range(2):
        out, whole, pad = RR.moated(shape, H.torch_dtype(dtype), fill,
                                    row=shape[-1])
        call(out)
        torch.cuda.synchronize()
        assert RR.moat_intact(whole, pad, pattern)
        runs.append(out.clone())
    assert torch.equal(runs[0].view(torch.int16), runs[1].view(torch.int16))
    err = np.abs(host(runs[0]).astype(np.float64) - ref)
    assert (err <= R.bound(ref, absum, k, dtype)).all()
    # the accumulation alone: what is left beyond the rounding to T
    p = 11 if dtype == "f16" else 8
    ratio = float((np.maximum(err - 2.0 ** -p * np.abs(ref), 0)
                   / np.maximum(absum, 1e-300)).max())
    print(f"{dtype}: worst |C - exact| / sum |terms| = 2^{np.log2(ratio):.2f}")
    assert ratio <= R.EPS_FAST / 2
    return runs[0]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_random_within_bound(dtype, fmt):
    k = 640
    o = random_operands(256, k, 256, fmt, dtype, [5, k])
    ref, absum = exact(*o, fmt)
    check_random(lambda out: sdd_call(*o, fmt, dtype, SDD_TOPOLOGY, out),
                 (3, 128, 128), F.blocks_from_dense(ref, *SDD_TOPOLOGY),
                 F.blocks_from_dense(absum, *SDD_TOPOLOGY), k, dtype)
    # SDD on the full topology and DSD over the same bytes: the same bits
    full = host(sdd_call(*o, fmt, dtype, FULL))
    every = (np.array([0, 5, 10], np.int32), np.arange(10, dtype=np.int16) % 5)
    dense = host(dsd_call(*o, fmt, dtype, every))
    assert np.array_equal(RR.bits(full, dtype), RR.bits(
        F.blocks_from_dense(dense, *FULL), dtype))
    o = random_operands(512, k, 256, fmt, dtype, [6, k])
    ref, absum = exact(*o, fmt, stored(512, k, DEEP))
    check_random(lambda out: dsd_call(*o, fmt, dtype, DEEP, out), (512, 256),
                 ref, absum, k, dtype)


@pytest.mark.parametrize("fmt", FORMATS)
def test_nan_reaches_its_row_or_column_only(fmt):
    aq, sa, wc, sw = kat(256, 384, 256, fmt, 9)
    aq[5, 200] = 0x7F            # a NaN byte of A: row 5 of block row 0
    sw[130, 7] = 0xFF            # a NaN scale of B: column 130
    want = np.zeros((256, 256), bool)
    want[5, :] = want[:, 130] = True
    got = host(sdd_call(aq, sa, wc, sw, fmt, "bf16", FULL))
    assert np.array_equal(np.isnan(got), F.blocks_from_dense(want, *FULL))
    got = host(dsd_call(aq, sa, wc, sw, fmt, "bf16", FULL))
    assert np.array_equal(np.isnan(got), want)


def test_rejections_leave_the_output_untouched():
    L, bad = sp.lib(), sp.hipErrorInvalidValue
    stream = torch.cuda.current_stream().cuda_stream
    out = torch.full((4, 128, 128), 7.0, dtype=torch.float16, device="cuda")
    aq = torch.zeros(256, 256, dtype=torch.uint8, device="cuda")
    wq = torch.zeros(256 * 256 + 16, dtype=torch.uint8, device="cuda")
    sa = torch.full((256, 8), 127, dtype=torch.uint8, device="cuda")
    sw = sa.clone()
    c = sp.BlockMatrix(256, 256, 128, 4 * 128 * 128, out, cuda(FULL[0]),
                       cuda(FULL[1]))
    c.row_indices = cuda(F.row_indices(FULL[0]))
    alias = sp.BlockMatrix(256, 256, 128, 4 * 128 * 128, aq, c.offsets,
                           c.indices)
    alias.row_indices = c.row_indices

    def sdd(a=aq.data_ptr(), a_s=sa.data_ptr(), k=256, b=wq.data_ptr(),
            fmt=0, cm=c):
        cc = cm._c()
        return L.sputnik_sdd_mx(a, a_s, k, b, sw.data_ptr(), fmt,
                                ctypes.byref(cc), 0, stream)

    assert sdd(a_s=None) == bad and sdd(k=192) == bad
    assert sdd(b=wq.data_ptr() + 8) == bad and sdd(cm=alias) == bad
    assert sdd(fmt=2) == bad and sdd(fmt=-1) == bad
    y = torch.full((256, 256), 7.0, dtype=torch.float16, device="cuda")

    def dsd(cols=256, s_s=sa.data_ptr(), b=wq.data_ptr(), fmt=1,
            c_ptr=y.data_ptr()):
        s = sp.BlockMatrix(256, cols, 128, 4 * 128 * 128, aq, c.offsets,
                           c.indices)
        cs, cm = s._c(), sp._CMatrix(256, 256, c_ptr)
        return L.sputnik_dsd_mx(ctypes.byref(cs), s_s, b, sw.data_ptr(), fmt,
                                ctypes.byref(cm), 0, stream)

    assert dsd(s_s=None) == bad and dsd(cols=192) == bad
    assert dsd(b=wq.data_ptr() + 8) == bad and dsd(c_ptr=aq.data_ptr()) == bad
    assert dsd(fmt=2) == bad
    q = torch.full((4, 256), 0x55, dtype=torch.uint8, device="cuda")
    x = torch.ones(4, 256, dtype=torch.float16, device="cuda")
    assert L.sputnik_quantize_rows_mx(x.data_ptr(), None, 4, 192, 0, 0,
                                      q.data_ptr(), sa.data_ptr(), 0,
                                      stream) == bad
    assert L.sputnik_quantize_weight_mx(x.data_ptr(), 256, 256, 0, 2,
                                        q.data_ptr(), sa.data_ptr(), 0,
                                        stream) == bad
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((y == 7.0).all())
    assert bool((q == 0x55).all())
    assert sdd() == sp.hipSuccess and dsd(fmt=0) == sp.hipSuccess
    torch.cuda.synchronize()
    assert not out.any() and not y.any()  # zeros times ones


# ---- ops.moe_mlp_mx ---------------------------------------------------------

TOKENS, D_MODEL, FFN, EXPERTS, TOP_K = 300, 256, 256, 4, 2
# Relative Frobenius error against ops.moe_mlp on the dequantised weights
# (only the activations' quantisation differs): twice the measured value
# (DESIGN 10 has the figures).
MOE_CAP = {("f16", False, "e4m3"): 2 * 0.03711, ("f16", False, "e2m1"): 2 * 0.03701,
           ("f16", True, "e4m3"): 2 * 0.04479, ("f16", True, "e2m1"): 2 * 0.04537,
           ("bf16", False, "e4m3"): 2 * 0.03753, ("bf16", False, "e2m1"): 2 * 0.03768,
           ("bf16", True, "e4m3"): 2 * 0.04537, ("bf16", True, "e2m1"): 2 * 0.04578}


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("glu", [False, True], ids=["mlp", "glu"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_moe_mlp_mx_equals_its_chain_and_is_close_to_the_16_bit_layer(
        dtype, glu, fmt):
    td, hidden = H.torch_dtype(dtype), EXPERTS * FFN
    x = cuda(M.values((TOKENS, D_MODEL), dtype, [21])).to(td)
    ws = [cuda(M.values(s, dtype, [22, i]) / np.float32(16)).to(td)
          for i, s in enumerate([(D_MODEL, hidden), (hidden, D_MODEL),
                                 (D_MODEL, hidden)])]
    top = cuda(M.routing(TOKENS, TOP_K, EXPERTS, "random", seed=5))
    ew = cuda(M.unit_weights(TOKENS * TOP_K, dtype, [23]).reshape(
        TOKENS, TOP_K)).to(td)
    w1q, w2q, v1q = (ops.quantize_weight_mx(w, format=fmt) for w in ws)
    # (checkpoint bytes, as torch's own views where this build has them)
    w1q = ops.MxWeight.from_tensors(
        w1q.q.clone().view(getattr(torch, "float4_e2m1fn_x2", torch.uint8)
                           if fmt == "e2m1" else torch.uint8),
        w1q.scales.clone().view(getattr(torch, "float8_e8m0fnu", torch.uint8)),
        fmt)
    v1q = v1q if glu else None
    out = ops.moe_mlp_mx(x, top, ew, w1q, w2q, EXPERTS, v1q=v1q)
    assert out.dtype == td and not out.requires_grad

    route = ops.moe_route(top, EXPERTS)
    topo = ops.expert_topology(route.padded_bins, FFN // 128,
                               route.rows // 128, dtype=td)
    xq, xs = ops.quantize_rows_mx(ops.padded_gather(x, route))
    g = ops.sdd_mx(xq, xs, w1q, topo, td)
    hq = (ops.quantize_sparse_mx(ops.sdd_mx(xq, xs, v1q, topo, td), "silu",
                                 gate=g) if glu
          else ops.quantize_sparse_mx(g, "gelu"))
    chain = ops.padded_scatter(ops.dsd_mx(hq, w2q, td), route, ew)
    assert torch.equal(out.view(torch.int16), chain.view(torch.int16))

    def dequantised(w):
        codes = w.q.view(torch.uint8).cpu().numpy()
        if fmt == "e2m1":
            codes = np.stack([codes & 15, codes >> 4], -1).reshape(w.n, w.k)
        full = R.decode(codes, w.scales.cpu().numpy(), fmt == "e2m1").T
        assert np.array_equal(RR.round_once(full, dtype), full)  # exact in T
        return cuda(full.astype(np.float32)).to(td)
    full = host(ops.moe_mlp(x, top, ew, dequantised(w1q), dequantised(w2q),
                            EXPERTS, v1=dequantised(v1q) if glu else None))
    rel = float(np.linalg.norm(host(out) - full) / np.linalg.norm(full))
    print(f"moe_mlp_mx {dtype} {'glu' if glu else 'mlp'} {fmt}: relative "
          f"error {rel:.5f}")
    assert rel <= MOE_CAP[dtype, glu, fmt]
