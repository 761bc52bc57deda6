"""GPU: the fp8 products through the C ABI (sputnik/block/fp8.h) against
tests/fp8_ref.py.

  quantisers  bytes and scales bit for bit, both scale rules, fp16 and bf16,
              plain and fused with kOutAct / kOutGate, with a NaN, a +Inf, an
              all-zero tile, a +-0 pair and a tile of subnormal amax planted.
              relu is exact in the reference; for gelu / silu the H comes from
              the 16-bit elementwise kernels, which is the contract: the fused
              quantiser gives the quantisation of the H those store.
              Also with x / gate one element and q one byte off their
              alignment (the element-access path), and on 131072 + 16 + 3
              tiles (the second trip of the grid-stride loop).
  lane-map    known-answer data (one-hot rows, asymmetric integers, pow2
              scales that differ per row and per k-block): every output is an
              exact small integer times a power of two, compared bit for bit.
  random      |gpu - ref64| <= fp8_ref.bound on every element, two runs with
              identical bits, moats around the output intact.
              Both at the 2-step shapes and at fp8_ref's deep ones (5
              steps; tests/test_gpu_fp8_exact.py holds those bit for bit).
  rejections  hipErrorInvalidValue with the output untouched.
"""

import ctypes

import numpy as np
import pytest
import torch

import sputnik_amd as sp
from oracle import oracle as O
from tests import fp8_ref as R
from tests import helpers as H
from tests import moe_ref as M
from tests import rounding_ref as RR

pytestmark = pytest.mark.gpu

DTYPES = ["f16", "bf16"]
ROW_SHAPES = [(3, 128), (130, 384), (5 * 128, 128)]  # the last: 5 blocks
MODES = [None, ("act", "relu"), ("act", "gelu"), ("gate", "relu"),
         ("gate", "silu")]
FILL = 0x55


def dev(a, dtype):
    """Values of T on the device, moved as bit patterns (a cast on the way
    may change the sign of a NaN)."""
    bits = np.ascontiguousarray(RR.bits(a, dtype)).view(np.int16)
    return torch.from_numpy(bits).cuda().view(H.torch_dtype(dtype))


def host(t) -> np.ndarray:
    return t.float().cpu().numpy()


def dev_bytes(q: np.ndarray):
    return torch.from_numpy(np.ascontiguousarray(q)).cuda().view(
        torch.float8_e4m3fn)


def guarded(shape, dtype, offset=0):
    """An output of `dtype` inside a larger allocation of FILL bytes, `offset`
    bytes past an aligned address: (view, check) with check() true while
    every byte around it is intact."""
    numel = int(np.prod(shape))
    size = torch.empty((), dtype=dtype).element_size()
    pad = 4096
    whole = torch.full(((numel + 2 * pad) * size + offset,), FILL,
                       dtype=torch.uint8, device="cuda")
    lo, hi = pad * size + offset, (pad + numel) * size + offset
    view = whole[lo:hi].view(dtype).view(*shape)

    def intact():
        return bool((whole[:lo] == FILL).all()) and bool(
            (whole[hi:] == FILL).all())
    return view, intact


def offset_by_one(t):
    """t's bits one element past an aligned address."""
    whole = torch.empty(t.numel() + 8, dtype=t.dtype, device="cuda")
    view = whole[1:1 + t.numel()].view(t.shape)
    view.view(torch.int16).copy_(t.contiguous().view(torch.int16))
    assert view.data_ptr() % 16 == 2
    return view


def plain_row_values(shape, dtype, seed, rng=None):
    """Values of T whose row scale runs over 17 binades."""
    rng = np.random.default_rng(seed) if rng is None else rng
    rows, cols = shape
    mag = np.exp2(rng.uniform(-12.0, 0.0, shape)
                  + rng.integers(-8, 9, (rows, 1)))
    sign = np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    return O.round_to((mag * sign).astype(np.float32), dtype)


def row_values(shape, dtype, seed):
    """plain_row_values with the special cases planted."""
    rng = np.random.default_rng(seed)
    rows, cols = shape
    x = plain_row_values(shape, dtype, None, rng)
    x[0, 5] = np.nan
    x[1, 7] = np.inf
    x[2, :128] = 0.0            # an all-zero tile
    x[0, 10], x[0, 11] = 0.0, -0.0
    # a tile of subnormal values (bf16: amax / 448 is subnormal in fp32 too)
    tiny = 2.0 ** -133 if dtype == "bf16" else 2.0 ** -24
    r = subnormal_row(rows)
    x[r, cols - 128:] = (tiny * rng.integers(-7, 8, 128)).astype(np.float32)
    x[r, cols - 1] = np.float32(7 * tiny)
    if r == 1:
        x[1, 7] = np.inf
    return x


def subnormal_row(rows: int) -> int:
    """The row whose last tile holds subnormal values: the last one, or with
    3 rows the row of the +Inf (row 2 is the all-zero tile)."""
    return rows - 1 if rows > 3 else 1


@pytest.mark.parametrize("mode", MODES, ids=lambda m: "plain" if m is None
                         else "-".join(m))
@pytest.mark.parametrize("pow2", [False, True], ids=["exact", "pow2"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_quantize_rows_bit_for_bit(dtype, pow2, mode):
    for n, shape in enumerate(ROW_SHAPES):
        x = row_values(shape, dtype, [1, n])
        g = row_values(shape, dtype, [2, n])[::-1].copy()
        dx, dg = dev(x, dtype), dev(g, dtype)
        kind, act = mode if mode else (None, None)
        # The H of a fused mode is the one the 16-bit elementwise kernel
        # stores (the sign of a NaN it produces included); relu is also
        # held against the reference wherever that is not a NaN.
        if kind is None:
            h = x
        elif kind == "act":
            h = host(sp.BlockActivation(dx, act))
        else:
            h = host(sp.BlockGate(dx, dg, act))
        if act == "relu":
            want = R.hidden(act, x, g if kind == "gate" else None, dtype)
            keep = ~np.isnan(want)
            assert np.array_equal(RR.bits(h, dtype)[keep],
                                  RR.bits(want, dtype)[keep])
        q_ref, s_ref = R.quantize_rows(h, pow2)
        q, q_ok = guarded(shape, torch.float8_e4m3fn)
        s, s_ok = guarded((shape[0], shape[1] // 128), torch.float32)
        sp.QuantizeRows(dx, q, s, pow2, act,
                        dg if kind == "gate" else None)
        torch.cuda.synchronize()
        got_q = q.view(torch.uint8).cpu().numpy()
        got_s = s.cpu().numpy()
        what = f"{dtype} pow2={pow2} {mode} {shape}"
        assert np.array_equal(got_s.view(np.uint32), s_ref.view(np.uint32)), what
        assert np.array_equal(got_q, q_ref), what
        assert q_ok() and s_ok(), what
        if kind is None:
            assert got_q[0, 5] == 0x7F and got_q[1, 7] == 0x7F
            assert got_q[0, 10] == 0x00 and got_q[0, 11] == 0x80
            assert got_s[2, 0] == R.SCALE_FLOOR and not got_q[2, :128].any()
            if dtype == "bf16":  # the floor at work: 7 * 2^-133 / 2^-126
                r = subnormal_row(shape[0])
                assert got_s[r, -1] == R.SCALE_FLOOR
                assert got_q[r, -1] == R.encode(np.float32(7 * 2.0 ** -7))


@pytest.mark.parametrize("pow2", [False, True], ids=["exact", "pow2"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_quantize_weight_both_orientations(dtype, pow2):
    k, n = 256, 384
    w = M.values((k, n), dtype, [3, k, n])
    # (a different magnitude, so a different scale, per block)
    w *= np.exp2(3 * (np.arange(k)[:, None] // 128)
                 - np.arange(n)[None, :] // 128).astype(np.float32)
    w[:128, 128:256] = 0.0       # an all-zero block
    w[200, 300] = np.nan
    w[130, 5] = -np.inf
    q_ref, s_ref = R.quantize_weight(w, pow2)
    for transpose in (False, True):
        src = dev(w.T if transpose else w, dtype)
        q, q_ok = guarded((n, k), torch.float8_e4m3fn)
        s, s_ok = guarded((k // 128, n // 128), torch.float32)
        sp.QuantizeWeight(src, q, s, transpose, pow2)
        torch.cuda.synchronize()
        assert np.array_equal(s.cpu().numpy().view(np.uint32),
                              s_ref.view(np.uint32)), transpose
        assert np.array_equal(q.view(torch.uint8).cpu().numpy(), q_ref), transpose
        assert q_ok() and s_ok()
    assert s_ref[0, 1] == R.SCALE_FLOOR
    assert q_ref[300, 200] == 0x7F and q_ref[5, 130] == 0xFF


UNALIGNED_MODES = [None, ("act", "relu"), ("gate", "silu")]


@pytest.mark.parametrize("mode", UNALIGNED_MODES,
                         ids=lambda m: "plain" if m is None else "-".join(m))
@pytest.mark.parametrize("dtype", DTYPES)
def test_quantize_rows_unaligned_buffers_give_the_same_bytes(dtype, mode):
    """The element-access path (x or gate not 16-byte, q not 8-byte aligned):
    x (and gate) one element off, q one byte off, each alone and both. Bytes
    and scales equal the aligned call's and the reference's; every byte
    around q stays intact."""
    shape = (130, 384)
    x = row_values(shape, dtype, [1, 1])
    g = row_values(shape, dtype, [2, 1])[::-1].copy()
    dx, dg = dev(x, dtype), dev(g, dtype)
    kind, act = mode if mode else (None, None)
    if kind is None:
        h = x
    elif kind == "act":
        h = host(sp.BlockActivation(dx, act))
    else:
        h = host(sp.BlockGate(dx, dg, act))
    q_ref, s_ref = R.quantize_rows(h)

    def run(x_off, q_off):
        q, q_ok = guarded(shape, torch.float8_e4m3fn, q_off)
        s, s_ok = guarded((shape[0], shape[1] // 128), torch.float32)
        xx, gg = (offset_by_one(dx), offset_by_one(dg)) if x_off else (dx, dg)
        assert q.data_ptr() % 8 == q_off
        sp.QuantizeRows(xx, q, s, False, act, gg if kind == "gate" else None)
        torch.cuda.synchronize()
        assert q_ok() and s_ok(), (x_off, q_off)
        return q.view(torch.uint8).cpu().numpy(), s.cpu().numpy()

    q0, s0 = run(0, 0)
    assert np.array_equal(q0, q_ref)
    assert np.array_equal(s0.view(np.uint32), s_ref.view(np.uint32))
    for x_off, q_off in ((1, 0), (0, 1), (1, 1)):
        q1, s1 = run(x_off, q_off)
        assert np.array_equal(q1, q0), (x_off, q_off)
        assert np.array_equal(s1.view(np.uint32), s0.view(np.uint32))


@pytest.mark.parametrize("dtype", DTYPES)
def test_quantize_weight_unaligned_buffers_give_the_same_bytes(dtype):
    k, n = 256, 384
    w = M.values((k, n), dtype, [3, k, n])
    w *= np.exp2(3 * (np.arange(k)[:, None] // 128)
                 - np.arange(n)[None, :] // 128).astype(np.float32)
    q_ref, s_ref = R.quantize_weight(w)
    for transpose in (False, True):
        src = offset_by_one(dev(w.T if transpose else w, dtype))
        q, q_ok = guarded((n, k), torch.float8_e4m3fn, 1)
        s, s_ok = guarded((k // 128, n // 128), torch.float32)
        sp.QuantizeWeight(src, q, s, transpose, False)
        torch.cuda.synchronize()
        assert np.array_equal(s.cpu().numpy().view(np.uint32),
                              s_ref.view(np.uint32)), transpose
        assert np.array_equal(q.view(torch.uint8).cpu().numpy(), q_ref), transpose
        assert q_ok() and s_ok()


# 131072 + 16 + 3 tiles: the grid is capped at 8192 workgroups of 16 tiles, so
# the grid-stride loop takes a second trip with one full workgroup and one of
# 3 tiles. 34 MB of input; the reference takes under 2 s on the host.
SECOND_TRIP_SHAPE = (43697, 384)
assert SECOND_TRIP_SHAPE[0] * 3 == 8192 * 16 + 16 + 3


@pytest.mark.parametrize("dtype,pow2", [("bf16", False), ("f16", True)],
                         ids=["bf16-exact", "f16-pow2"])
def test_quantize_rows_second_trip_of_the_grid_stride_loop(dtype, pow2):
    x = plain_row_values(SECOND_TRIP_SHAPE, dtype, [4, pow2])
    q_ref, s_ref = R.quantize_rows(x, pow2)
    q, q_ok = guarded(SECOND_TRIP_SHAPE, torch.float8_e4m3fn)
    s, s_ok = guarded((SECOND_TRIP_SHAPE[0], 3), torch.float32)
    sp.QuantizeRows(dev(x, dtype), q, s, pow2)
    torch.cuda.synchronize()
    got_q, got_s = q.view(torch.uint8).cpu().numpy(), s.cpu().numpy()
    assert np.array_equal(got_s.view(np.uint32), s_ref.view(np.uint32))
    assert np.array_equal(got_q, q_ref)
    trip_two = np.s_[8192 * 16:]
    assert np.array_equal(got_q.reshape(-1, 128)[trip_two],
                          q_ref.reshape(-1, 128)[trip_two])
    assert q_ok() and s_ok()


# ---- the products ---------------------------------------------------------------

def sdd_call(aq, sa, wq, sw, dtype, out=None):
    """C's block values [5, 128, 128] of T for the SDD cases (m and n from
    the operands; both cases have SDD_TOPOLOGY); `out` a preallocated tensor
    or None."""
    offsets, indices = R.SDD_TOPOLOGY
    nb = len(indices)
    if out is None:
        out = torch.empty(nb, 128, 128, dtype=H.torch_dtype(dtype),
                          device="cuda")
    c = sp.BlockMatrix(aq.shape[0], wq.shape[0], 128, nb * 128 * 128, out,
                       torch.from_numpy(offsets).cuda(),
                       torch.from_numpy(indices).cuda())
    c.row_indices = torch.from_numpy(R.row_indices(offsets)).cuda()
    sp.SddFp8(dev_bytes(aq), torch.from_numpy(sa).cuda(), dev_bytes(wq),
              torch.from_numpy(sw).cuda(), c)
    return out


def dsd_call(sq, ss, wq, sw, dtype, out=None, deep=False):
    offsets, indices = R.DSD_DEEP_TOPOLOGY if deep else R.DSD_TOPOLOGY
    nb = len(indices)
    m, (n, k) = 128 * (len(offsets) - 1), wq.shape
    if out is None:
        out = torch.empty(m, n, dtype=H.torch_dtype(dtype), device="cuda")
    s = sp.BlockMatrix(m, k, 128, nb * 128 * 128, dev_bytes(sq),
                       torch.from_numpy(offsets).cuda(),
                       torch.from_numpy(indices).cuda())
    sp.DsdFp8(s, torch.from_numpy(ss).cuda(), dev_bytes(wq),
              torch.from_numpy(sw).cuda(), sp.Matrix(m, n, out))
    return out


# The shallow cases (at most 2 steps per output tile) and the deep ones of
# fp8_ref (5 steps, which refill both stages of the ring; the DSD with 4 x 5
# x 2 blocks and block rows of 5, 0, 1 and 3 stored blocks).


def _lane_map_kat_sdd(dtype, deep):
    k = R.SDD_DEEP_K[-1] if deep else R.SDD_K
    x, w = R.kat_rows(R.SDD_M, k), R.kat_weight(k, R.SDD_N)
    (aq, sa), (wq, sw) = R.quantize_rows(x, True), R.quantize_weight(w, True)
    got = sdd_call(aq, sa, wq, sw, dtype)
    torch.cuda.synchronize()
    want = (x.astype(np.float64) @ w.astype(np.float64) + 0.0).astype(
        np.float32)
    want = R.blocks_from_dense(want, *R.SDD_TOPOLOGY)
    assert np.array_equal(RR.bits(host(got), dtype), RR.bits(want, dtype))


def _lane_map_kat_dsd(dtype, deep):
    # (x is zero outside the stored blocks: the empty block row 128-255)
    ops, x, w = R.kat_case("dsd", deep)
    assert not x[128:256].any() and (ops.m, ops.k, ops.n) == (
        (R.DSD_DEEP_M, R.DSD_DEEP_K, R.DSD_DEEP_N) if deep
        else (R.DSD_M, R.DSD_K, R.DSD_N))
    (sq, ss), wq, sw = ops.sparse(), ops.wq, ops.sw
    got = dsd_call(sq, ss, wq, sw, dtype, deep=deep)
    torch.cuda.synchronize()
    want = (x.astype(np.float64) @ w.astype(np.float64) + 0.0).astype(
        np.float32)
    got_bits = RR.bits(host(got), dtype)
    assert np.array_equal(got_bits, RR.bits(want, dtype))
    assert not got_bits[128:256].any()  # +0 rows


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
    got = host(runs[0]).astype(np.float64)
    err, lim = np.abs(got - ref), R.bound(ref, absum, k, dtype)
    worst = float((err / np.maximum(lim, 1e-300)).max())
    print(f"{dtype}: worst error / bound = {worst:.3f}")
    assert (err <= lim).all(), worst


def _random_sdd_within_bound(dtype, deep):
    if deep:
        ops = R.random_case("sdd", True, dtype)
        aq, sa, wq, sw = ops.aq, ops.sa, ops.wq, ops.sw
    else:
        (aq, sa) = R.quantize_rows(M.values((R.SDD_M, R.SDD_K), dtype,
                                            [11, 1]))
        (wq, sw) = R.quantize_weight(M.values((R.SDD_K, R.SDD_N), dtype,
                                              [11, 2]))
    ref, absum = R.matmul64(R.dequantize_rows(aq, sa),
                            R.dequantize_weight(wq, sw))
    topo = R.SDD_TOPOLOGY
    check_random(lambda out: sdd_call(aq, sa, wq, sw, dtype, out),
                 (len(topo[1]), 128, 128), R.blocks_from_dense(ref, *topo),
                 R.blocks_from_dense(absum, *topo), aq.shape[1], dtype)


def _random_dsd_within_bound(dtype, deep):
    if deep:
        ops = R.random_case("dsd", True, dtype)
        offsets, indices = ops.topology
        (sq, ss), wq, sw = ops.sparse(), ops.wq, ops.sw
        m, k, n = ops.m, ops.k, ops.n
    else:
        offsets, indices = R.DSD_TOPOLOGY
        m, k, n = R.DSD_M, R.DSD_K, R.DSD_N
        sq, ss = R.quantize_sparse(M.values((len(indices), 128, 128), dtype,
                                            [12, 1]))
        wq, sw = R.quantize_weight(M.values((k, n), dtype, [12, 2]))
    a64 = R.dequantize_rows(
        R.dense_from_blocks(m, k, offsets, indices, sq),
        R.expand_block_scales(m, k, offsets, indices, ss))
    ref, absum = R.matmul64(a64, R.dequantize_weight(wq, sw))
    check_random(lambda out: dsd_call(sq, ss, wq, sw, dtype, out, deep),
                 (m, n), ref, absum, k, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_lane_map_kat_sdd(dtype):
    _lane_map_kat_sdd(dtype, False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_lane_map_kat_sdd_deep(dtype):
    _lane_map_kat_sdd(dtype, True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_lane_map_kat_dsd(dtype):
    _lane_map_kat_dsd(dtype, False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_lane_map_kat_dsd_deep(dtype):
    _lane_map_kat_dsd(dtype, True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_random_sdd_within_bound(dtype):
    _random_sdd_within_bound(dtype, False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_random_sdd_within_bound_deep(dtype):
    _random_sdd_within_bound(dtype, True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_random_dsd_within_bound(dtype):
    _random_dsd_within_bound(dtype, False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_random_dsd_within_bound_deep(dtype):
    _random_dsd_within_bound(dtype, True)


# ---- rejections -----------------------------------------------------------------

def test_rejections_leave_the_output_untouched():
    L = sp.lib()
    offsets, indices = R.SDD_TOPOLOGY
    nb = len(indices)
    k = R.SDD_K
    out = torch.full((nb, 128, 128), 7.0, dtype=torch.float16, device="cuda")
    aq = torch.zeros(R.SDD_M, k, dtype=torch.uint8, device="cuda")
    wq = torch.zeros(R.SDD_N, k, dtype=torch.uint8, device="cuda")
    sa = torch.ones(R.SDD_M, k // 128, device="cuda")
    sw = torch.ones(k // 128, R.SDD_N // 128, device="cuda")
    c = sp.BlockMatrix(R.SDD_M, R.SDD_N, 128, nb * 128 * 128, out,
                       torch.from_numpy(offsets).cuda(),
                       torch.from_numpy(indices).cuda())
    c.row_indices = torch.from_numpy(R.row_indices(offsets)).cuda()
    stream = torch.cuda.current_stream().cuda_stream

    def sdd(a, a_s, kk, b, b_s, cm):
        cc = cm._c()
        return L.sputnik_sdd_fp8(a, a_s, kk, b, b_s, ctypes.byref(cc), 0,
                                 stream)

    ok = (aq.data_ptr(), sa.data_ptr(), k, wq.data_ptr(), sw.data_ptr(), c)
    assert sdd(*ok) == sp.hipSuccess
    torch.cuda.synchronize()
    assert not out.any()  # zeros times ones
    out.fill_(7.0)
    assert sdd(aq.data_ptr(), sa.data_ptr(), 192, wq.data_ptr(),
               sw.data_ptr(), c) == sp.hipErrorInvalidValue
    assert sdd(aq.data_ptr(), None, k, wq.data_ptr(), sw.data_ptr(),
               c) == sp.hipErrorInvalidValue
    assert sdd(aq.data_ptr(), sa.data_ptr(), -128, wq.data_ptr(),
               sw.data_ptr(), c) == sp.hipErrorInvalidValue
    alias = sp.BlockMatrix(R.SDD_M, R.SDD_N, 128, nb * 128 * 128, aq,
                           c.offsets, c.indices)
    alias.row_indices = c.row_indices
    assert sdd(aq.data_ptr(), sa.data_ptr(), k, wq.data_ptr(), sw.data_ptr(),
               alias) == sp.hipErrorInvalidValue
    no_rows = sp.BlockMatrix(R.SDD_M, R.SDD_N, 128, nb * 128 * 128, out,
                             c.offsets, c.indices)
    assert sdd(aq.data_ptr(), sa.data_ptr(), k, wq.data_ptr(), sw.data_ptr(),
               no_rows) == sp.hipErrorInvalidValue

    # DSD: K = 192 columns in the sparse operand, a null scale pointer, C = Bq
    y = torch.full((R.SDD_M, 128), 7.0, dtype=torch.float16, device="cuda")
    w2 = torch.zeros(128, R.SDD_N, dtype=torch.uint8, device="cuda")
    s2 = torch.ones(R.SDD_N // 128, 1, device="cuda")
    hs = torch.ones(nb * 128, device="cuda")
    hq = torch.zeros(nb, 128, 128, dtype=torch.uint8, device="cuda")

    def dsd(cols, hs_ptr, c_ptr):
        s = sp.BlockMatrix(R.SDD_M, cols, 128, nb * 128 * 128, hq,
                           c.offsets, c.indices)
        cs, cm = s._c(), sp._CMatrix(R.SDD_M, 128, c_ptr)
        return L.sputnik_dsd_fp8(ctypes.byref(cs), hs_ptr, w2.data_ptr(),
                                 s2.data_ptr(), ctypes.byref(cm), 0, stream)

    assert dsd(192, hs.data_ptr(), y.data_ptr()) == sp.hipErrorInvalidValue
    assert dsd(R.SDD_N, None, y.data_ptr()) == sp.hipErrorInvalidValue
    assert dsd(R.SDD_N, hs.data_ptr(), w2.data_ptr()) == sp.hipErrorInvalidValue

    # Aq, Bq and C 8 bytes off a 16-byte boundary (each buffer has the room,
    # so nothing here would leave its allocation if the check were missing)
    def shifted(t):
        """A copy of t's bytes 8 bytes into a fresh allocation: (view of t's
        dtype and shape, the whole allocation as bytes)."""
        raw = t.contiguous().view(torch.uint8).reshape(-1)
        whole = torch.empty(raw.numel() + 16, dtype=torch.uint8, device="cuda")
        assert whole.data_ptr() % 16 == 0
        whole[8:8 + raw.numel()] = raw
        return whole[8:8 + raw.numel()].view(t.dtype).view(t.shape), whole

    aq8, wq8, (out8, out8_whole) = shifted(aq)[0], shifted(wq)[0], shifted(out)
    c8 = sp.BlockMatrix(R.SDD_M, R.SDD_N, 128, nb * 128 * 128, out8,
                        c.offsets, c.indices)
    c8.row_indices = c.row_indices
    assert aq8.data_ptr() % 16 == 8 and out8.data_ptr() % 16 == 8
    for a, b, cm in ((aq8, wq, c), (aq, wq8, c), (aq, wq, c8)):
        assert sdd(a.data_ptr(), sa.data_ptr(), k, b.data_ptr(),
                   sw.data_ptr(), cm) == sp.hipErrorInvalidValue
    # a block size other than 128, nonzeros that are no whole number of
    # blocks, and an element type that does not exist
    for size, nonzeros in ((64, nb * 128 * 128), (128, nb * 128 * 128 + 128)):
        odd = sp.BlockMatrix(R.SDD_M, R.SDD_N, size, nonzeros, out, c.offsets,
                             c.indices)
        odd.row_indices = c.row_indices
        assert sdd(*ok[:5], odd) == sp.hipErrorInvalidValue
    cc = c._c()
    assert L.sputnik_sdd_fp8(*ok[:5], ctypes.byref(cc), 2,
                             stream) == sp.hipErrorInvalidValue

    def dsd_with(data=hq, bq=w2, c_ptr=None, c_rows=R.SDD_M, dtype=0,
                 size=128, nonzeros=nb * 128 * 128):
        s = sp.BlockMatrix(R.SDD_M, R.SDD_N, size, nonzeros, data, c.offsets,
                           c.indices)
        cs = s._c()
        cm = sp._CMatrix(c_rows, 128, y.data_ptr() if c_ptr is None else c_ptr)
        return L.sputnik_dsd_fp8(ctypes.byref(cs), hs.data_ptr(),
                                 bq.data_ptr(), s2.data_ptr(),
                                 ctypes.byref(cm), dtype, stream)

    (y8, y8_whole) = shifted(y)
    bad = sp.hipErrorInvalidValue
    assert dsd_with(data=shifted(hq)[0]) == bad
    assert dsd_with(bq=shifted(w2)[0]) == bad
    assert dsd_with(c_ptr=y8.data_ptr()) == bad
    assert dsd_with(size=64) == bad
    assert dsd_with(nonzeros=nb * 128 * 128 + 128) == bad
    assert dsd_with(c_rows=R.SDD_M + 128) == bad    # c.rows != s.rows
    assert dsd_with(dtype=2) == bad
    torch.cuda.synchronize()
    assert bool((out8_whole[8:-8].view(torch.float16) == 7.0).all())
    assert bool((y8_whole[8:-8].view(torch.float16) == 7.0).all())

    # the quantisers
    x = torch.ones(4, 256, dtype=torch.float16, device="cuda")
    q = torch.full((4, 256), FILL, dtype=torch.uint8, device="cuda")
    s = torch.full((4, 2), 7.0, device="cuda")
    rows = L.sputnik_quantize_rows
    assert rows(x.data_ptr(), 4, 192, q.data_ptr(), s.data_ptr(), 0, 0,
                stream) == sp.hipErrorInvalidValue
    assert rows(x.data_ptr(), 4, 256, q.data_ptr(), None, 0, 0,
                stream) == sp.hipErrorInvalidValue
    assert rows(x.data_ptr(), -4, 256, q.data_ptr(), s.data_ptr(), 0, 0,
                stream) == sp.hipErrorInvalidValue
    assert rows(x.data_ptr(), 4, 256, x.data_ptr(), s.data_ptr(), 0, 0,
                stream) == sp.hipErrorInvalidValue
    assert L.sputnik_quantize_rows_act(x.data_ptr(), 4, 256, 9, q.data_ptr(),
                                       s.data_ptr(), 0, 0,
                                       stream) == sp.hipErrorInvalidValue
    assert L.sputnik_quantize_rows_gated(x.data_ptr(), None, 4, 256, 0,
                                         q.data_ptr(), s.data_ptr(), 0, 0,
                                         stream) == sp.hipErrorInvalidValue
    assert L.sputnik_quantize_weight(x.data_ptr(), 256, 192, 0, q.data_ptr(),
                                     s.data_ptr(), 0, 0,
                                     stream) == sp.hipErrorInvalidValue
    # zero-sized work succeeds, whatever the pointers
    assert rows(None, 0, 256, None, None, 0, 0, stream) == sp.hipSuccess
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((q == FILL).all())
    assert bool((s == 7.0).all()) and bool((y == 7.0).all())
    # ... and the same DSD call with nothing wrong runs: zeros times ones
    assert dsd(R.SDD_N, hs.data_ptr(), y.data_ptr()) == sp.hipSuccess
    torch.cuda.synchronize()
    assert not y.any()
