"""CPU: the fp8 format of sputnik/block/fp8.h as tests/fp8_ref.py states it
(the GPU tests hold the kernels against that reference bit for bit), and the
argument checks of the Python layer that are raised before the library is
called. No GPU work."""

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import fp8_ref as R
from tests import moe_ref as M
from tests import rounding_ref as RR


def torch_bytes(v32: np.ndarray) -> np.ndarray:
    t = torch.from_numpy(np.ascontiguousarray(v32, dtype=np.float32))
    return t.to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def all_bf16() -> np.ndarray:
    bits = np.arange(65536, dtype=np.uint32) << 16
    with np.errstate(invalid="ignore"):
        return bits.view(np.float32).copy()


def tiles(dtype: str, seed: int) -> np.ndarray:
    """[rows, 128] tiles of T whose amax runs over the exponents -149 .. 126
    (bf16; fp16 over its own range), with elements down to zero."""
    rng = np.random.default_rng(seed)
    lo, hi = (-149, 126) if dtype == "bf16" else (-24, 15)
    exps = np.arange(lo, hi + 1).repeat(4)
    mag = np.exp2(exps[:, None] + rng.uniform(-12.0, 0.0, (exps.size, R.B)))
    mag[:, 0] = np.exp2(exps) * rng.uniform(1.0, 1.99, exps.size)
    sign = np.where(rng.random(mag.shape) < 0.5, -1.0, 1.0)
    with np.errstate(over="ignore", under="ignore"):
        x = O.round_to((mag * sign).astype(np.float32), dtype)
    return np.where(np.isfinite(x), x, np.float32(0))


def test_decode_table():
    d = R.DECODE
    assert d[0x7E] == 448.0 and d[0xFE] == -448.0
    assert np.isnan(d[0x7F]) and np.isnan(d[0xFF])
    assert d[0x08] == 2.0 ** -6 and d[0x01] == 2.0 ** -9
    assert d[0x00] == 0.0 and np.signbit(d[0x80])
    assert np.isfinite(d).sum() == 254
    ref = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).double()
    assert np.array_equal(d, ref.numpy(), equal_nan=True)


def test_encoder_equals_torch_cast_on_every_bf16_pattern():
    v = all_bf16()
    finite = np.isfinite(v)
    # Every finite value moved into the encoder's range by a power of two:
    # m 2^e with m in [0.5, 1) becomes m 2^min(e, 9), or 2^8 where that would
    # pass 448.
    m, e = np.frexp(np.where(finite, v, 0))
    top = np.where(np.abs(m) <= 0.875, 9, 8)
    w = np.ldexp(m, np.minimum(e, top)).astype(np.float32)
    assert np.abs(w).max() == 448.0
    got = R.encode(w)
    assert np.array_equal(got[finite], torch_bytes(w)[finite])
    # ... and decoding gives the nearest e4m3 value back.
    assert np.array_equal(R.decode(got)[finite],
                          torch.from_numpy(w).to(torch.float8_e4m3fn)
                          .double().numpy()[finite])
    # NaN and +-Inf: the e4m3 NaN with the element's sign.
    q = R.quantize(v, np.float32(1))
    assert np.array_equal(q[~finite],
                          0x7F | (np.signbit(v[~finite]).astype(np.uint8) << 7))


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("pow2", [False, True])
def test_tiles_equal_torch_cast_and_stay_below_the_overflow_edge(dtype, pow2):
    x = tiles(dtype, 1)
    q, s = R.quantize_rows(x, pow2)
    y = R.scaled_value(x, s)  # [rows, 128] / [rows, 1]
    worst = float(np.abs(y).max())
    print(f"{dtype} pow2={pow2}: max |x / scale| = {worst!r}")
    # 448 and one fp32 rounding (448 has an ulp of 2^-15 ~ 0.00003), far
    # below 464 where e4m3 rounds to the NaN code.
    assert worst <= float(np.nextafter(np.float32(448), np.float32(512)))
    assert np.array_equal(q, torch_bytes(y))
    # above the floor the row's largest element uses the top of the range
    top = np.abs(R.decode(q)).max(axis=1)
    assert (top[s[:, 0] > R.SCALE_FLOOR] >= (224.0 if pow2 else 448.0)).all()


def test_the_floor_keeps_subnormal_amax_tiles_in_range():
    # amax / 448 is subnormal for amax < 448 * 2^-126: its quotient loses
    # bits, and without the floor x / scale leaves the range.
    amax = np.exp2(np.arange(-149.0, -117.0)).astype(np.float32)
    x = np.zeros((amax.size, R.B), dtype=np.float32)
    x[:, 3] = amax
    x[:, 7] = -amax * np.float32(0.75)
    s = R.scale(amax)
    assert (s >= R.SCALE_FLOOR).all() and (s[:8] == R.SCALE_FLOOR).all()
    assert np.abs(R.scaled_value(x, s[:, None])).max() <= 448.0
    with np.errstate(divide="ignore", under="ignore", over="ignore"):
        bare = amax / R.FP8_MAX
        without = np.abs(x[:, 3] / bare)
    assert (without > 464.0).any(), "the floor is what this test is about"
    q, _ = R.quantize_rows(x)
    assert np.isfinite(R.decode(q)).all()


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_pow2_scales_are_the_smallest_that_fit_and_dequantise_exactly(dtype):
    x = tiles(dtype, 2)
    q, s = R.quantize_rows(x, pow2=True)
    amax = np.abs(x).max(axis=1).astype(np.float64)
    s64 = s[:, 0].astype(np.float64)
    m, _ = np.frexp(s64)
    assert (m == 0.5).all() and (s64 >= 2.0 ** -126).all()
    assert (amax / s64 <= 448.0).all()
    smaller_fits = amax / (s64 / 2) <= 448.0
    assert (~smaller_fits | (s64 == 2.0 ** -126)).all()
    d = R.decode(q).astype(np.float32)
    with np.errstate(under="ignore"):
        back = (d * s).astype(np.float32) / s
    assert np.array_equal(back, d)
    # values of at most 4 significant bits survive unchanged
    k = R.kat_rows(256, 256)
    qk, sk = R.quantize_rows(k, pow2=True)
    assert np.array_equal(R.dequantize_rows(qk, sk), k.astype(np.float64))
    w = R.kat_weight(256, 384)
    qw, sw = R.quantize_weight(w, pow2=True)
    assert np.array_equal(R.dequantize_weight(qw, sw), w.astype(np.float64))


def test_weight_blocks_and_sparse_rows():
    rng = np.random.default_rng(3)
    w = O.round_to(rng.standard_normal((256, 384)).astype(np.float32), "bf16")
    w[:128, :128] = 0
    q, s = R.quantize_weight(w)
    assert q.shape == (384, 256) and s.shape == (2, 3)
    assert s[0, 0] == R.SCALE_FLOOR and not q[:128, :128].any()
    blk = w[128:, 256:]
    assert s[1, 2] == np.float32(np.abs(blk).max()) / np.float32(448)
    assert np.array_equal(q[256:, 128:].T, R.quantize(blk, s[1, 2]))
    v = O.round_to(rng.standard_normal((5, 128, 128)).astype(np.float32), "f16")
    qs, ss = R.quantize_sparse(v)
    assert qs.shape == v.shape and ss.shape == (5 * 128,)
    assert np.array_equal(qs[3, 17], R.quantize(v[3, 17], ss[3 * 128 + 17]))


def test_relu_hidden_is_exact_and_zero_is_positive():
    x = np.array([-2.0, -0.0, 0.0, 3.0], dtype=np.float32)
    g = np.array([1.0, 2.0, -1.0, 4.0], dtype=np.float32)
    assert np.array_equal(R.hidden("relu", x), [0, 0, 0, 3])
    assert not np.signbit(R.hidden("relu", x)).any()
    h = R.hidden("relu", x, gate=g)  # x * relu(g)
    assert np.array_equal(h, [-2.0, 0.0, 0.0, 12.0])
    assert not np.signbit(h[1:3]).any()


def _random_operands(dtype, m, k, n, seed):
    a = M.values((m, k), dtype, [seed, 1])
    w = M.values((k, n), dtype, [seed, 2])
    return R.quantize_rows(a), R.quantize_weight(w)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_fp32_emulation_meets_the_gpu_bound(dtype):
    """The bound tests/test_gpu_fp8.py holds the kernel to, met by an fp32
    evaluation of the kernel's arithmetic on that test's own cases (same
    generators, same seeds)."""
    # SDD
    (aq, sa), (wq, sw) = _random_operands(dtype, R.SDD_M, R.SDD_K, R.SDD_N, 11)
    ref, absum = R.matmul64(R.dequantize_rows(aq, sa),
                            R.dequantize_weight(wq, sw))
    got = O.round_to(R.product32(aq, sa, wq, sw), dtype).astype(np.float64)
    assert (np.abs(got - ref) <= R.bound(ref, absum, R.SDD_K, dtype)).all()
    # DSD, in the storage order of its unordered rows
    offsets, indices = R.DSD_TOPOLOGY
    vals = M.values((len(indices), R.B, R.B), dtype, [12, 1])
    sq, ss = R.quantize_sparse(vals)
    wq, sw = R.quantize_weight(M.values((R.DSD_K, R.DSD_N), dtype, [12, 2]))
    dense_q = R.dense_from_blocks(R.DSD_M, R.DSD_K, offsets, indices, sq)
    dense_s = R.expand_block_scales(R.DSD_M, R.DSD_K, offsets, indices, ss)
    ref, absum = R.matmul64(R.dequantize_rows(dense_q, dense_s),
                            R.dequantize_weight(wq, sw))
    got = O.round_to(R.product32(dense_q, dense_s, wq, sw,
                                 R.storage_order(offsets, indices)),
                     dtype).astype(np.float64)
    assert (np.abs(got - ref) <= R.bound(ref, absum, R.DSD_K, dtype)).all()
    assert not got[128:256].any()  # the empty block row


@pytest.mark.parametrize("kind", ["sdd", "dsd"])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_fp32_emulation_meets_the_gpu_bound_at_the_deep_shapes(dtype, kind):
    """The same for the deep cases (5 steps; DSD with 4 x 5 x 2 blocks and
    rows of 5, 0, 1 and 3 stored blocks), with the correctly rounded
    emulation."""
    ops = R.random_case(kind, True, dtype)
    assert (ops.m, ops.k, ops.n) == ((256, 640, 384) if kind == "sdd"
                                     else (512, 640, 256))
    ref, absum = R.matmul64(R.dequantize_rows(ops.aq, ops.sa),
                            R.dequantize_weight(ops.wq, ops.sw))
    got = R.round_t(ops.acc(), dtype).astype(np.float64)
    assert (np.abs(got - ref) <= R.bound(ref, absum, ops.k, dtype)).all()
    if kind == "dsd":
        assert not got[128:256].any() and got[256:384].any()


def test_deep_cases_reach_the_ring_steady_state_and_are_not_square():
    assert [k // R.B for k in R.SDD_DEEP_K] == [1, 3, 5]
    offsets, indices = R.DSD_DEEP_TOPOLOGY
    blocks = (R.DSD_DEEP_M // R.B, R.DSD_DEEP_K // R.B, R.DSD_DEEP_N // R.B)
    assert blocks == (4, 5, 2) and len(offsets) == blocks[0] + 1
    assert list(np.diff(offsets)) == [5, 0, 1, 3]
    for row in R.storage_order(offsets, indices):
        assert len(set(row)) == len(row) and max(row, default=0) < blocks[1]
        assert len(row) < 2 or row != sorted(row)


def test_fma32_is_correctly_rounded():
    """Against exact rational arithmetic, on sums that cancel to their last
    bits (where a float64 sum cast to float32 rounds twice), and IEEE on the
    special values."""
    from fractions import Fraction

    rng = np.random.default_rng(5)
    n = 4000
    s = R.ordinary_scales(rng, n)
    p = (rng.integers(-2 ** 20, 2 ** 20, n) / 64.0).astype(np.float32)
    acc = (-s.astype(np.float64) * p
           * (1 + rng.integers(-3, 4, n) * 2.0 ** -23)).astype(np.float32)
    acc[::7] = rng.standard_normal(len(acc[::7])).astype(np.float32)
    got = R.fma32(s, p, acc)
    for i in range(n):
        exact = (Fraction(float(s[i])) * Fraction(float(p[i]))
                 + Fraction(float(acc[i])))
        g = np.float32(got[i])
        miss = abs(Fraction(float(g)) - exact)
        for side in (-np.inf, np.inf):
            other = Fraction(float(np.nextafter(g, np.float32(side))))
            assert miss <= abs(other - exact), i
            if miss == abs(other - exact):      # a tie: the even one
                assert int(g.view(np.uint32)) % 2 == 0, i
    # a float64 sum that is inexact and lands on a float32 tie: rounded once
    # (down, the exact value is below the tie), where the cast rounds twice
    one, tiny = np.float32(1), np.float32(2.0 ** -60)
    tie = np.float32(1 + 2.0 ** -24)
    assert R.fma32(tie, one, -tiny) == one
    assert R.fma32(np.float32(1 + 2.0 ** -23), np.float32(1 + 2.0 ** -23),
                   np.float32(2.0 ** -24)) == np.float32(1 + 3 * 2.0 ** -23)
    f = np.float32
    assert np.isnan(R.fma32(f(np.inf), f(0), f(1)))
    assert R.fma32(f(np.inf), f(-2), f(1)) == -np.inf
    assert np.isnan(R.fma32(f(np.inf), f(2), f(-np.inf)))
    assert np.isnan(R.fma32(f(np.nan), f(2), f(1)))
    z = R.fma32(f(3), f(-0.0), f(0.0))
    assert z == 0 and not np.signbit(z)


EXACT_CASES = [("sdd", k) for k in R.SDD_DEEP_K] + [("dsd", R.DSD_DEEP_K)]


def _paired_rows(ops) -> np.ndarray:
    """The rows of the output whose block row takes at least two steps."""
    steps = (np.array([len(o) for o in ops.order]) if ops.order
             else np.full(ops.m // R.B, ops.k // R.B))
    return np.repeat(steps >= 2, R.B)


@pytest.mark.parametrize("kind,k", EXACT_CASES)
def test_exact_cases_have_an_exact_p_and_finite_outputs(kind, k):
    """The condition that makes the bit-exact GPU tests independent of the
    matrix cores' summation order: only EXACT_BYTES (multiples of 1/8 up to
    15), so every product is a multiple of 2^-6 and every interval's sum
    |products| stays below 2^24 such units."""
    assert len(R.EXACT_BYTES) == 80
    v = R.decode(R.EXACT_BYTES)
    assert np.array_equal(v * 8, np.rint(v * 8)) and np.abs(v).max() == 15
    ops = R.exact_case(kind, k)
    assert np.isin(ops.aq, R.EXACT_BYTES).all()
    assert np.isin(ops.wq, R.EXACT_BYTES).all()
    acc = ops.acc(exact_p=True)        # asserts the sum |products| bound
    for kb in range(ops.k // R.B):     # ... and P itself, on the product
        ks = slice(kb * R.B, (kb + 1) * R.B)
        p64 = R.decode(ops.aq[:, ks]) @ R.decode(ops.wq[:, ks]).T
        assert np.array_equal(p64.astype(np.float32).astype(np.float64), p64)
        assert np.array_equal(p64 * 64, np.rint(p64 * 64))
    stored = np.repeat([len(o) > 0 for o in ops.order] if ops.order
                       else [True] * (ops.m // R.B), R.B)
    for dtype in ("f16", "bf16"):
        c = R.round_t(acc, dtype)
        assert np.isfinite(c).all()
        assert not RR.bits(c[~stored], dtype).any()     # +0 rows
        share = float(np.mean(c[stored] != 0))
        print(f"{kind} K={k} {dtype}: non-zero {share:.4f}, max |C| "
              f"{float(np.abs(c).max()):.4g}")
        assert share > 0.99


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_wrong_models_are_visible_on_the_exact_cases(dtype):
    """Each wrong model of the arithmetic changes at least 25 % of the
    outputs, after rounding to T, of every exact case it can show on: a
    condition on the inputs of tests/test_gpu_fp8_exact.py. Counted over the
    rows of block rows with at least two steps; K = 128 has one step, after
    which every model but the rounding of T is the contract's own
    (fma(s, P, 0) = round(s P)), so it is left out, and the order of the
    steps can differ only for DSD. Measured, fp16 / bf16:

        model            SDD K=384      SDD K=640      DSD deep
        mul_then_add     0.959 / 0.896  0.993 / 0.965  0.979 / 0.931
        scale_after_p    0.971 / 0.920  0.995 / 0.973  0.984 / 0.945
        exact_scale      0.963 / 0.905  0.993 / 0.967  0.978 / 0.932
        ascending_order                                0.931 / 0.839
        partial_in_T     1.000 / 1.000  1.000 / 1.000  1.000 / 1.000

    round_half_up differs from round-to-nearest-even on ties only, and an
    fp32 accumulator of random residues is a tie of T once in 2^13 (fp16) or
    2^16 (bf16) outputs: 0.001 and below on the cases above. It is held to
    the same 25 % on fp8_ref.tie_case, where every output is a tie (measured
    1.000 / 1.000)."""
    for kind, k in EXACT_CASES[1:]:
        ops = R.exact_case(kind, k)
        rows = _paired_rows(ops)
        assert rows.sum() >= 2 * R.B
        want = RR.bits(R.round_t(ops.acc(), dtype), dtype)[rows]
        for model in R.MODELS[:-1]:
            if model == "ascending_order" and kind != "dsd":
                continue
            got = RR.bits(R.round_t(ops.acc(model, dtype), dtype), dtype)[rows]
            share = float(np.mean(got != want))
            print(f"{kind} K={k} {dtype} {model}: {share:.3f}")
            assert share >= 0.25, (kind, k, model, share)
    ops = R.tie_case(dtype)
    acc = ops.acc(exact_p=True)
    assert np.array_equal(acc.astype(np.float64),
                          R.dequantize_rows(ops.aq, ops.sa)
                          @ R.dequantize_weight(ops.wq, ops.sw))  # exact
    even = RR.bits(R.round_t(acc, dtype), dtype)
    away = RR.bits(R.round_t(acc, dtype, "round_half_up"), dtype)
    share = float(np.mean(even != away))
    print(f"ties {dtype} round_half_up: {share:.3f}")
    assert share >= 0.25


@pytest.mark.parametrize("kind", ["sdd", "dsd"])
@pytest.mark.parametrize("patterned", ["a", "w"])
def test_byte_case_covers_every_byte_at_every_position(kind, patterned):
    """Each of the 254 finite bytes is multiplied into a stored output from
    each of the 16 byte positions of both 16-byte reads of a lane, in the
    patterned operand; and the expected values straight from the definition
    are what the emulation gives."""
    ops = R.byte_case(kind, patterned)
    assert not ((ops.aq & 0x7F) == 0x7F).any()
    assert not ((ops.wq & 0x7F) == 0x7F).any()
    seen = R.byte_case_coverage(ops)
    finite = np.isfinite(R.DECODE)
    assert finite.sum() == 254 and seen[finite].all()
    assert not seen[~finite].any()
    for s in (ops.sa, ops.sw):
        assert set(np.unique(s)) == {1.0, 2.0, 4.0}
    want = R.byte_case_expected(ops)
    assert not np.signbit(want[want == 0]).any()
    assert np.array_equal(ops.acc(exact_p=False).astype(np.float64), want)
    for dtype in ("f16", "bf16"):   # 4 significant bits: exact in T
        assert np.array_equal(R.round_t(want.astype(np.float32), dtype), want)


@pytest.mark.parametrize("kind", ["sdd", "dsd"])
def test_special_cases_plant_what_they_say(kind):
    """The planted NaN / Inf reach the outputs they should and no others,
    and the overflow rows sit on both sides of fp16's tie to Inf."""
    ops, (row, kb) = R.special_case(kind, "nan_a")
    bad = np.isnan(ops.acc())
    assert bad[row].all() and bad.sum() == ops.n

    ops, (row, kb) = R.special_case(kind, "nan_w")
    bad = np.isnan(ops.acc())
    reach = np.array([kb in (o if ops.order else range(ops.k // R.B))
                      for o in (ops.order or [None] * (ops.m // R.B))])
    assert reach.any() and (kind == "sdd" or not reach.all())
    want = np.zeros_like(bad)
    want[np.repeat(reach, R.B), 200] = True
    assert np.array_equal(bad, want)

    ops, (row, kb) = R.special_case(kind, "inf_sa")
    acc = ops.acc()
    changed = ~np.isfinite(acc)
    assert changed[row].all() and changed.sum() == ops.n
    assert np.isnan(acc[row, 3::4]).all()               # 0 * Inf
    rest = np.delete(acc[row], np.s_[3::4])
    assert np.isinf(rest).sum() > ops.n // 2            # Inf * P, either sign
    assert (rest == np.inf).any() and (rest == -np.inf).any()

    ops, (row, kb) = R.special_case(kind, "nan_sw")
    bad = np.isnan(ops.acc())
    assert bad[:, :128].sum() == 0 and bad[:, 256:].sum() == 0
    assert bad[:, 128:256].all(axis=1).sum() == bad.sum() // 128 > 0

    ops, (row, kb) = R.special_case(kind, "overflow")
    acc = ops.acc()
    assert acc[row, 10] > 65520 and acc[row + 1, 10] == 65520
    assert 65504 < acc[row + 2, 10] < 65520
    assert np.array_equal(acc[row:row + 3, 11], -acc[row:row + 3, 10])
    f16 = R.round_t(acc, "f16")[row:row + 3]
    assert list(f16[:, 10]) == [np.inf, np.inf, 65504.0]
    assert list(f16[:, 11]) == [-np.inf, -np.inf, -65504.0]
    assert np.isfinite(R.round_t(acc, "bf16")[row:row + 3]).all()


def test_kat_is_exact_in_fp32():
    x, w = R.kat_rows(R.SDD_M, R.SDD_K), R.kat_weight(R.SDD_K, R.SDD_N)
    (aq, sa), (wq, sw) = R.quantize_rows(x, True), R.quantize_weight(w, True)
    want = x.astype(np.float64) @ w.astype(np.float64)
    assert np.array_equal(R.product32(aq, sa, wq, sw).astype(np.float64), want)
    for dtype in ("f16", "bf16"):
        assert np.array_equal(O.round_to(want.astype(np.float32), dtype), want)
    # every k of a block is hit by some row, and rows differ in scale
    assert np.array_equal(np.sort(np.nonzero(x)[1]), np.arange(R.SDD_K))
    assert len(np.unique(sa)) > 8 and len(np.unique(sw)) == 3


# ---- the Python layer's checks, before any library call ------------------------

def test_argument_checks_raise_before_the_library_is_called():
    import sputnik_amd as sp
    from sputnik_amd import ops

    x = torch.zeros(4, 256, dtype=torch.bfloat16)
    with pytest.raises(TypeError):
        ops.quantize_rows(x.float())
    with pytest.raises(ValueError):
        ops.quantize_rows(torch.zeros(4, 192, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        ops.quantize_weight(torch.zeros(192, 128, dtype=torch.float16))
    with pytest.raises(ValueError, match="forward only"):
        ops.quantize_rows(x.clone().requires_grad_())
    q = torch.zeros(4, 256, dtype=torch.float8_e4m3fn)
    s = torch.zeros(4, 2, dtype=torch.float32)
    with pytest.raises(TypeError):
        sp.QuantizeRows(x, q.view(torch.uint8), s)
    with pytest.raises(ValueError):
        sp.QuantizeRows(x, q, torch.zeros(4, 1, dtype=torch.float32))
    with pytest.raises(ValueError):
        sp.QuantizeRows(x, q, s, activation="tanh")
    with pytest.raises(ValueError):
        sp.QuantizeRows(x, q, s, gate=x.clone())  # a gate without activation
    wq = torch.zeros(384, 256, dtype=torch.float8_e4m3fn)
    with pytest.raises(ValueError):
        ops.Fp8Weight.from_tensors(wq, torch.zeros(3, 2))  # [n/128, k/128]
    with pytest.raises(TypeError):
        ops.Fp8Weight.from_tensors(wq.view(torch.uint8).to(torch.int16),
                                   torch.zeros(2, 3))
    w = ops.Fp8Weight.from_tensors(wq.view(torch.uint8), torch.ones(2, 3))
    assert w.shape == (256, 384) and w.q.dtype == torch.float8_e4m3fn
    with pytest.raises(TypeError):
        ops.sdd_fp8(q, s, wq, None)
    with pytest.raises(TypeError):
        ops.dsd_fp8(None, w)


def test_moe_mlp_fp8_checks():
    from sputnik_amd import ops

    x = torch.zeros(8, 256, dtype=torch.bfloat16)
    top = torch.zeros(8, 2, dtype=torch.int64)
    ew = torch.ones(8, 2, dtype=torch.bfloat16)

    def weight(k, n):
        return ops.Fp8Weight.from_tensors(
            torch.zeros(n, k, dtype=torch.float8_e4m3fn),
            torch.ones(k // 128, n // 128))

    w1, w2 = weight(256, 512), weight(512, 256)
    with pytest.raises(ValueError, match="forward only"):
        ops.moe_mlp_fp8(x.clone().requires_grad_(), top, ew, w1, w2, 4)
    with pytest.raises(ValueError, match="forward only"):
        ops.moe_mlp_fp8(x, top, ew.clone().requires_grad_(), w1, w2, 4)
    with pytest.raises(TypeError, match="Fp8Weight"):
        ops.moe_mlp_fp8(x, top, ew, torch.zeros(256, 512, dtype=x.dtype), w2, 4)
    with pytest.raises(ValueError):
        ops.moe_mlp_fp8(x, top, ew, w1, weight(512, 128), 4)
    with pytest.raises(ValueError):
        ops.moe_mlp_fp8(x, top, ew, w1, w2, 3)  # 512 columns, 3 experts
    with pytest.raises(ValueError):
        ops.moe_mlp_fp8(x, top, ew, w1, w2, 4, v1q=weight(256, 256))
    with pytest.raises(ValueError):
        ops.moe_mlp_fp8(x, top, ew, w1, w2, 4, activation="tanh")
