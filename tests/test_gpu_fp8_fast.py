"""GPU: the fp8 products' fast accumulation (sputnik/block/fp8.h,
Fp8Accumulate::kFast) and Fp8IntervalSums, through the C ABI.

In kFast an interval's P is what the scaled e4m3 MFMA returns, which the CPU
cannot emulate. The method: Fp8IntervalSums is the definition of P as a cold,
plain kernel; the product kernels are held bit for bit to the chain
fp8_fast_ref.from_interval_sums over it (the correctly rounded fma and
round_T of tests/fp8_ref.py), and Fp8IntervalSums itself to known answers
(lane map) and to float64 dot products within EPS_FAST.

  lane map    Fp8IntervalSums in both modes on the one-hot byte cases and the
              known-answer case: every (row, k, column) and every byte; in
              kFp32 also bit-equal to fp8_ref.interval_sum on exact bytes.
  method      the shipped kFp32 kernel equals the chain over
              Fp8IntervalSums(kFp32) on random data: the harness is sound.
  fast        the kFast kernel equals the chain over Fp8IntervalSums(kFast)
              on random, known-answer, exact and special cases, every
              element, DSD in storage order, two runs, moats intact.
  switch      on a large product among small ones the two modes' P differ
              (the dropped addends) and the fast product follows kFast's.
  bound       random data within bound_fast of the float64 product.
  eps         the worst |P - exact| / sum |products| over the four families
              is at most EPS_FAST / 2.
  NaN         a NaN byte reaches exactly its row or column of the interval's
              tiles.
  rejections  a wrong mode, k = 192, a null or aliased P: hipErrorInvalidValue
              and nothing written.
"""

import ctypes
import functools

import numpy as np
import pytest
import torch

import sputnik_amd as sp
from tests import fp8_fast_ref as F
from tests import fp8_ref as R
from tests import helpers as H
from tests import rounding_ref as RR
from tests import test_gpu_fp8_exact as E

pytestmark = pytest.mark.gpu

DTYPES = ["f16", "bf16"]
MODES = ["fp32", "fast"]
INVALID = 1          # hipErrorInvalidValue
P_PATTERN = 0x55555555


def interval_sums(aq: np.ndarray, wq: np.ndarray, mode: str) -> np.ndarray:
    """P [k / 128, m, n] of Fp8IntervalSums, into a moated output that must
    stay intact around it."""
    m, k = aq.shape
    n = wq.shape[0]
    fill = torch.tensor([P_PATTERN], dtype=torch.int32).view(torch.float32)
    p, whole, pad = RR.moated((k // 128, m, n), torch.float32, fill.item(),
                              row=n)
    sp.Fp8IntervalSums(E.place(aq, torch.float8_e4m3fn, False),
                       E.place(wq, torch.float8_e4m3fn, False), p,
                       accumulate=mode)
    torch.cuda.synchronize()
    assert RR.moat_intact(whole, pad, P_PATTERN)
    return p.cpu().numpy()


def bits32(x) -> np.ndarray:
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def call(ops, dtype, out, mode):
    """The product of `ops` into `out` under `mode`."""
    offsets, idx = ops.topology
    nb = len(idx)
    d_off = E.place(offsets, torch.int32, False)
    d_idx = E.place(np.asarray(idx, np.int16), torch.int16, False)
    wq = E.place(ops.wq, torch.float8_e4m3fn, False)
    sw = E.place(ops.sw, torch.float32, False)
    if ops.kind == "sdd":
        c = sp.BlockMatrix(ops.m, ops.n, 128, nb * 128 * 128, out, d_off,
                           d_idx)
        c.row_indices = E.place(R.row_indices(offsets), torch.int16, False)
        sp.SddFp8(E.place(ops.aq, torch.float8_e4m3fn, False),
                  E.place(ops.sa, torch.float32, False), wq, sw, c,
                  accumulate=mode)
    else:
        sq, ss = ops.sparse()
        s = sp.BlockMatrix(ops.m, ops.k, 128, nb * 128 * 128,
                           E.place(sq, torch.float8_e4m3fn, False), d_off,
                           d_idx)
        sp.DsdFp8(s, E.place(ss, torch.float32, False), wq, sw,
                  sp.Matrix(ops.m, ops.n, out), accumulate=mode)
    torch.cuda.synchronize()


def run_twice(ops, dtype, mode) -> np.ndarray:
    """The output's bits (uint16, C's layout) after two runs into fresh
    moated outputs that must agree bit for bit and leave the moats intact."""
    runs = []
    for _ in range(2):
        out, whole, pad = E.fresh(E.out_shape(ops), dtype)
        call(ops, dtype, out, mode)
        assert RR.moat_intact(whole, pad, E.PATTERN)
        runs.append(out.view(torch.int16).cpu().numpy().view(np.uint16))
    assert np.array_equal(runs[0], runs[1]), "two runs differ"
    return runs[0]


def layout(ops, dense):
    """A dense [m, n] result in C's layout."""
    if ops.kind == "sdd":
        return R.blocks_from_dense(dense, *ops.topology)
    return dense


def chain(ops, dtype, mode) -> np.ndarray:
    """round_T of the contract's chain over Fp8IntervalSums(mode), in C's
    layout."""
    p = interval_sums(ops.aq, ops.wq, mode)
    return layout(ops, F.from_interval_sums(p, ops.sa, ops.sw, ops.order,
                                            dtype))


def assert_same_bits(got_bits, want, dtype, what=""):
    """Bit equality wherever the expected value is not a NaN, and the same
    NaN mask; every element."""
    got = E.as_values(got_bits, dtype)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN masks differ"
    diff = got_bits[~nan] != RR.bits(want, dtype)[~nan]
    assert not diff.any(), (f"{what}: {int(diff.sum())} of {diff.size} "
                            f"elements differ")


@functools.lru_cache(maxsize=None)
def random_case(kind, deep, dtype):
    return R.random_case(kind, deep, dtype)


@functools.lru_cache(maxsize=None)
def float64_product(kind, deep, dtype):
    """(ref, sum |terms|) of random_case in C's layout."""
    ops = random_case(kind, deep, dtype)
    ref, absum = R.matmul64(R.dequantize_rows(ops.aq, ops.sa),
                            R.dequantize_weight(ops.wq, ops.sw))
    return layout(ops, ref), layout(ops, absum)


# ---- the lane map of Fp8IntervalSums --------------------------------------------

@pytest.mark.parametrize("patterned", ["a", "w"])
@pytest.mark.parametrize("mode", MODES)
def test_interval_sums_of_every_byte(mode, patterned):
    """One operand one-hot with 1.0: P is the decoded byte in the interval
    that holds the hot position and +0 in the others, bit for bit."""
    ops = R.byte_case("sdd", patterned)
    a, w = R.decode(ops.aq), R.decode(ops.wq)
    want = np.stack([a[:, ks] @ w[:, ks].T + 0.0 for ks in
                     (slice(i * 128, (i + 1) * 128)
                      for i in range(ops.k // 128))]).astype(np.float32)
    hot = np.argmax((ops.aq if patterned == "w" else ops.wq) != 0, axis=1)
    cold = np.arange(ops.k // 128)[:, None] != (hot // 128)[None, :]
    cold = cold[:, :, None] if patterned == "w" else cold[:, None, :]
    assert not want[np.broadcast_to(cold, want.shape)].any()
    assert len(np.unique(want)) >= 253          # every finite byte value
    got = interval_sums(ops.aq, ops.wq, mode)
    assert np.array_equal(bits32(got), bits32(want))


@pytest.mark.parametrize("mode", MODES)
def test_interval_sums_of_the_known_answer_case(mode):
    ops, x, w = R.kat_case("sdd", False)
    a, b = R.decode(ops.aq), R.decode(ops.wq)
    want = np.stack([a[:, i * 128:(i + 1) * 128] @ b[:, i * 128:(i + 1) * 128].T
                     + 0.0 for i in range(ops.k // 128)]).astype(np.float32)
    got = interval_sums(ops.aq, ops.wq, mode)
    assert np.array_equal(bits32(got), bits32(want))
    # ... which is x w with the scales put back
    back = F.from_interval_sums(got, ops.sa, ops.sw)
    assert np.array_equal(back, (x.astype(np.float64) @ w).astype(np.float32))


def test_fp32_interval_sums_equal_the_reference_on_exact_bytes():
    ops = R.exact_case("sdd", R.SDD_DEEP_K[-1])
    got = interval_sums(ops.aq, ops.wq, "fp32")
    for kb in range(ops.k // 128):
        ks = slice(kb * 128, (kb + 1) * 128)
        want, _ = R.interval_sum(ops.aq[:, ks], ops.wq[:, ks])
        assert np.array_equal(bits32(got[kb]), bits32(want)), kb


# ---- the method, on the shipped kernel ------------------------------------------

RANDOM = [(kind, deep) for kind in ("sdd", "dsd") for deep in (False, True)]
RANDOM_IDS = [f"{kind}-{'deep' if deep else 'shallow'}" for kind, deep in RANDOM]


@pytest.mark.parametrize("kind,deep", RANDOM, ids=RANDOM_IDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_fp32_kernel_equals_the_chain_over_its_interval_sums(dtype, kind,
                                                             deep):
    ops = random_case(kind, deep, dtype)
    assert_same_bits(run_twice(ops, dtype, "fp32"), chain(ops, dtype, "fp32"),
                     dtype, "kFp32")


# ---- the fast kernel, to the bit --------------------------------------------------

@pytest.mark.parametrize("kind,deep", RANDOM, ids=RANDOM_IDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_fast_kernel_equals_the_chain_and_is_within_its_bound(dtype, kind,
                                                              deep):
    ops = random_case(kind, deep, dtype)
    got = run_twice(ops, dtype, "fast")
    assert_same_bits(got, chain(ops, dtype, "fast"), dtype, "kFast")
    ref, absum = float64_product(kind, deep, dtype)
    err = np.abs(E.as_values(got, dtype).astype(np.float64) - ref)
    lim = F.bound_fast(ref, absum, ops.k, dtype)
    print(f"kFast {kind} {dtype} deep={deep}: worst error / bound = "
          f"{float((err / np.maximum(lim, 1e-300)).max()):.3f}; worst error / "
          f"sum |terms| = 2^"
          f"{float(np.log2((err / np.maximum(absum, 1e-300)).max())):.2f}")
    assert err.shape == ref.shape and (err <= lim).all()


@pytest.mark.parametrize("kind", ["sdd", "dsd"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_fast_kernel_on_the_known_answer_case(dtype, kind):
    ops, x, w = R.kat_case(kind, False)
    got = run_twice(ops, dtype, "fast")
    assert_same_bits(got, chain(ops, dtype, "fast"), dtype, "kFast")
    answer = RR.round_once(x.astype(np.float64) @ w.astype(np.float64), dtype)
    assert np.array_equal(got, RR.bits(layout(ops, answer), dtype))


@pytest.mark.parametrize("kind,k", E.EXACT,
                         ids=[f"{kind}-k{k}" for kind, k in E.EXACT])
@pytest.mark.parametrize("dtype", DTYPES)
def test_fast_kernel_on_the_exact_case(dtype, kind, k):
    ops = E.exact(kind, k)
    got = run_twice(ops, dtype, "fast")
    assert_same_bits(got, chain(ops, dtype, "fast"), dtype, "kFast")
    if kind == "dsd":
        assert not got[128:256].any()       # the empty block row: +0


@pytest.mark.parametrize("what", E.SPECIALS)
@pytest.mark.parametrize("kind", ["sdd", "dsd"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_fast_kernel_on_the_special_cases(dtype, kind, what):
    ops, (row, kb) = R.special_case(kind, what)
    got_bits = run_twice(ops, dtype, "fast")
    assert_same_bits(got_bits, chain(ops, dtype, "fast"), dtype, what)
    if what not in ("nan_a", "nan_w"):
        return
    # A NaN byte: exactly its row (A) or its column (W) of the tiles of the
    # block rows that take its interval, and nothing else.
    got = E.as_values(got_bits, dtype)
    stored = np.ones((ops.m, ops.n), bool)
    if kind == "sdd":
        stored = R.dense_from_blocks(ops.m, ops.n, *ops.topology,
                                     np.ones_like(got, dtype=bool))
        got = R.dense_from_blocks(ops.m, ops.n, *ops.topology, got)
    order = ops.order or [list(range(ops.k // 128))] * (ops.m // 128)
    want = np.zeros((ops.m, ops.n), bool)
    if what == "nan_a":
        want[row, :] = True
    else:
        for rb, steps in enumerate(order):
            if kb in steps:
                want[rb * 128:(rb + 1) * 128, 200] = True
    want &= stored
    assert want.any()
    assert np.array_equal(np.isnan(got), want)
    assert np.isfinite(got[~want]).all()


def test_sdd_and_dsd_give_the_same_bits_for_the_same_intervals():
    """SDD on a full topology, and DSD over the same bytes stored in
    ascending order."""
    base = random_case("sdd", True, "bf16")
    m, k, n = base.m, base.k, base.n
    full = lambda rows, cols: (                             # noqa: E731
        np.arange(rows + 1, dtype=np.int32) * cols,
        np.tile(np.arange(cols, dtype=np.int16), rows))
    sdd = R.Operands("sdd", base.aq, base.sa, base.wq, base.sw,
                     full(m // 128, n // 128))
    dsd = R.Operands("dsd", base.aq, base.sa, base.wq, base.sw,
                     full(m // 128, k // 128))
    a = run_twice(sdd, "bf16", "fast")
    b = run_twice(dsd, "bf16", "fast")
    assert np.array_equal(R.dense_from_blocks(m, n, *sdd.topology, a), b)


# ---- the switch reaches the kernel -------------------------------------------------

@functools.lru_cache(maxsize=None)
def family_sums(name, mode):
    aq, bq = F.families()[name]
    return interval_sums(aq, bq, mode)


def test_the_modes_differ_on_a_large_product_among_small_ones():
    aq, bq = F.families()["large_among_small"]
    fast, fp32 = (family_sums("large_among_small", mode)
                  for mode in ("fast", "fp32"))
    exact, _ = F.exact_sums(aq, bq)          # (every one fits fp32)
    differ = bits32(fast) != bits32(fp32)
    print(f"large among small: {int(differ.sum())} of {differ.size} interval "
          f"sums differ between kFast and kFp32; "
          f"{int((fast != exact).sum())} and {int((fp32 != exact).sum())} "
          f"differ from the exact sums")
    assert differ.any()
    # ... and the fast product is the chain over kFast's sums. sa = 2^-12
    # keeps fp16 finite; every block of C is stored.
    m, n = aq.shape[0], bq.shape[0]
    topo = (np.arange(m // 128 + 1, dtype=np.int32),
            np.zeros(m // 128, np.int16))
    ops = R.Operands("sdd", aq, np.full((m, 1), 2.0 ** -12, np.float32), bq,
                     np.ones((1, 1), np.float32), topo)
    got = run_twice(ops, "f16", "fast")
    want = layout(ops, F.from_interval_sums(fast, ops.sa, ops.sw, None, "f16"))
    assert np.isfinite(want).all()
    assert_same_bits(got, want, "f16", "kFast")
    other = layout(ops, F.from_interval_sums(fp32, ops.sa, ops.sw, None,
                                             "f16"))
    print(f"... {int((got != RR.bits(other, 'f16')).sum())} of {got.size} "
          f"fp16 outputs differ from the chain over kFp32's sums")


# ---- eps_fast --------------------------------------------------------------------

def test_eps_fast_holds_with_its_margin_on_the_four_families():
    worst = {}
    for name, (aq, bq) in F.families().items():
        worst[name] = F.worst_ratio(family_sums(name, "fast"), aq, bq)
        print(f"{name}: worst |P - exact| / sum |products| = 2^"
              f"{np.log2(max(worst[name], 1e-300)):.2f}")
    assert max(worst.values()) <= F.EPS_FAST / 2, worst


# ---- rejections --------------------------------------------------------------------

def test_a_wrong_mode_is_rejected_with_nothing_written():
    ops = random_case("sdd", False, "bf16")
    offsets, idx = ops.topology
    out, whole, pad = E.fresh(E.out_shape(ops), "bf16")
    c = sp.BlockMatrix(ops.m, ops.n, 128, len(idx) * 128 * 128, out,
                       E.place(offsets, torch.int32, False),
                       E.place(idx, torch.int16, False))
    c.row_indices = E.place(R.row_indices(offsets), torch.int16, False)
    aq = E.place(ops.aq, torch.float8_e4m3fn, False)
    sa = E.place(ops.sa, torch.float32, False)
    wq = E.place(ops.wq, torch.float8_e4m3fn, False)
    sw = E.place(ops.sw, torch.float32, False)
    cc = c._c()
    L = sp.lib()
    for mode in (2, -1):
        assert L.sputnik_sdd_fp8_acc(
            sp._ptr(aq), sp._ptr(sa), ops.k, sp._ptr(wq), sp._ptr(sw),
            ctypes.byref(cc), 1, mode, None) == INVALID
    dsd = random_case("dsd", False, "bf16")
    sq, ss = dsd.sparse()
    d_off, d_idx = dsd.topology
    s = sp.BlockMatrix(dsd.m, dsd.k, 128, len(d_idx) * 128 * 128,
                       E.place(sq, torch.float8_e4m3fn, False),
                       E.place(d_off, torch.int32, False),
                       E.place(d_idx, torch.int16, False))
    y, y_whole, y_pad = E.fresh((dsd.m, dsd.n), "bf16")
    cs, cy = s._c(), sp.Matrix(dsd.m, dsd.n, y)._c()
    dss = E.place(ss, torch.float32, False)
    dwq = E.place(dsd.wq, torch.float8_e4m3fn, False)
    dsw = E.place(dsd.sw, torch.float32, False)
    assert L.sputnik_dsd_fp8_acc(
        ctypes.byref(cs), sp._ptr(dss), sp._ptr(dwq), sp._ptr(dsw),
        ctypes.byref(cy), 1, 2, None) == INVALID
    torch.cuda.synchronize()
    for t in (whole, y_whole):
        assert bool((t.view(torch.int16) == E.PATTERN).all())
    # ... and the accepted modes of the same calls succeed
    assert L.sputnik_sdd_fp8_acc(
        sp._ptr(aq), sp._ptr(sa), ops.k, sp._ptr(wq), sp._ptr(sw),
        ctypes.byref(cc), 1, 1, None) == 0
    torch.cuda.synchronize()
    assert RR.moat_intact(whole, pad, E.PATTERN)
    assert not bool((out.view(torch.int16) == E.PATTERN).all())


def test_interval_sums_rejections_write_nothing():
    m, n, k = 128, 128, 256
    aq = torch.zeros(m, k, dtype=torch.uint8, device="cuda")
    bq = torch.zeros(n, k, dtype=torch.uint8, device="cuda")
    p = torch.full((k // 128, m, n), P_PATTERN, dtype=torch.int32,
                   device="cuda")
    f = sp.lib().sputnik_fp8_interval_sums
    a, b, o = aq.data_ptr(), bq.data_ptr(), p.data_ptr()
    for mode in (0, 1):
        assert f(a, b, m, n, 192, mode, o, None) == INVALID      # k = 192
        assert f(a, b, m, 192, k, mode, o, None) == INVALID
        assert f(a, b, m, n, k, mode, None, None) == INVALID     # a null P
        assert f(None, b, m, n, k, mode, o, None) == INVALID
        assert f(a, b, m, n, k, mode, a, None) == INVALID        # P is A
        assert f(a, b, m, n, k, mode, b, None) == INVALID        # P is B
        assert f(a + 8, b, m, n, k, mode, o, None) == INVALID    # alignment
        assert f(a, b, m, n, k, mode, o + 4, None) == INVALID
        assert f(a, b, m, n, -128, mode, o, None) == INVALID
    assert f(a, b, m, n, k, 2, o, None) == INVALID               # the mode
    assert f(a, b, 0, n, k, 1, o, None) == 0                     # zero-sized
    torch.cuda.synchronize()
    assert bool((p == P_PATTERN).all())
    assert not aq.any() and not bq.any()
    with pytest.raises(ValueError):
        sp.Fp8IntervalSums(aq.view(torch.float8_e4m3fn)[:, :192],
                           bq.view(torch.float8_e4m3fn)[:, :192], p)
