"""GPU: expert biases (sputnik/block/bias.h, moe.h PaddedScatterBias*): the
column bias in the SDD epilogue on both routes, BlockColumnSum, and the
scatter with an output bias with its two gradients.

Expected values come from numpy (tests/bias_ref.py), never from the library.
The SDD checks apply the numpy bias stage to the device's own plain SDD output
(the contract of bias.h: the plain product followed by an elementwise pass,
bit for bit); that product itself is checked against the oracle by
tests/test_gpu_activation.py on these very problems. Bit-for-bit comparisons
between routes are route checks, not correctness oracles."""

import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import sputnik_amd as sp  # noqa: E402
from tests import bias_ref as R  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests import moe_ref as M  # noqa: E402
from tests.test_gpu_activation import (  # noqa: E402,F401
    SMALL_INDICES, SMALL_OFFSETS, Problem, _grouped_problem_data,
    _small_operands, route)

pytestmark = pytest.mark.gpu

B = 128
DTYPES = ("f16", "bf16")
TRANSPOSES = [(False, False), (False, True), (True, False), (True, True)]
HIP_ERROR_INVALID_VALUE = 1


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _f32(t: torch.Tensor) -> np.ndarray:
    return t.detach().float().cpu().numpy()


def _t_bits(a: np.ndarray, dtype: str) -> np.ndarray:
    """The bit patterns of float32 values representable in T."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return t.to(H.torch_dtype(dtype)).view(torch.int16).numpy().view(np.uint16)


def _dev(a, dtype):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(
        H.torch_dtype(dtype)).cuda()


def _bias_dev(values: np.ndarray, dtype: str, unaligned: bool = False):
    """The bias on the device; `unaligned`: one element into an allocation,
    so that it is 2-byte but not 16-byte aligned."""
    n = values.size
    if not unaligned:
        return _dev(values, dtype)
    buf = torch.zeros(n + 8, dtype=H.torch_dtype(dtype), device="cuda")
    t = buf[1:1 + n]
    t.copy_(_dev(values, dtype))
    assert t.data_ptr() % 16 != 0 and t.is_contiguous()
    return t


def _same(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


# ---- the column bias of the SDD epilogue ------------------------------------

def _bias_products(p, bias, act, gate):
    """(C, H, Z, H without Z, Hg, U, Hg without U) of the three products."""
    c, cd = p.c()
    sp.MatmulBias(p.A, p.ta, p.Bm, p.tb, c, bias)
    c, h = p.c()
    z = torch.full_like(h, float("nan"))
    sp.MatmulBiasActivation(p.A, p.ta, p.Bm, p.tb, c, bias, act, z)
    c, h0 = p.c()
    sp.MatmulBiasActivation(p.A, p.ta, p.Bm, p.tb, c, bias, act)
    c, hg = p.c()
    u = torch.full_like(hg, float("nan"))
    sp.MatmulBiasGated(p.A, p.ta, p.Bm, p.tb, c, bias, act, gate, u)
    c, hg0 = p.c()
    sp.MatmulBiasGated(p.A, p.ta, p.Bm, p.tb, c, bias, act, gate)
    torch.cuda.synchronize()
    return cd, h, z, h0, hg, u, hg0


def _check_bias_products(p, dtype, act, routes, route, unaligned=False):
    plain = p.plain()
    torch.cuda.synchronize()
    bias_np = R.column_bias(p.n, dtype)
    bias = _bias_dev(bias_np, dtype, unaligned)
    want = _t_bits(R.bias_stage(_f32(plain), p.indices, bias_np, dtype), dtype)
    gate = plain                                    # any G of T will do
    first = None
    for r in routes:
        route(r)
        cd, h, z, h0, hg, u, hg0 = _bias_products(p, bias, act, gate)
        what = f"route {r}"
        assert np.array_equal(_bits(cd), want), f"{what}: MatmulBias"
        assert np.array_equal(_bits(z), want), f"{what}: kept Z"
        assert np.array_equal(_bits(u), want), f"{what}: kept U"
        assert _same(h, sp.BlockActivation(z, act)), f"{what}: H == act(Z)"
        assert _same(h, h0), f"{what}: H with / without Z"
        assert _same(hg, sp.BlockGate(u, gate, act)), f"{what}: H == gate(U, G)"
        assert _same(hg, hg0), f"{what}: gated H with / without U"
        got = tuple(_bits(t) for t in (h, hg))
        if first is None:
            first = got
        else:
            for name, x, y in zip(("H", "gated H"), first, got):
                assert np.array_equal(x, y), \
                    f"{name} differs between routes {routes[0]} and {r}"
    # a zero bias: the bias-free products under == (only -0 may become +0)
    route(routes[0])
    zero = torch.zeros(p.n, dtype=p.td, device="cuda")
    cd, h, z, _, hg, u, _ = _bias_products(p, zero, act, gate)
    h_free, z_free = p.forward(act, keep_z=True)
    c, hg_free = p.c()
    sp.MatmulGated(p.A, p.ta, p.Bm, p.tb, c, act, gate)
    torch.cuda.synchronize()
    for name, x, y in (("C", cd, plain), ("Z", z, z_free), ("H", h, h_free),
                       ("U", u, plain), ("gated H", hg, hg_free)):
        assert torch.equal(x.float(), y.float()), f"zero bias: {name}"


@pytest.mark.parametrize("ta,tb", TRANSPOSES)
@pytest.mark.parametrize("k", [64, 192])
@pytest.mark.parametrize("dtype", DTYPES)
def test_small_ksplit_tile(dtype, k, ta, tb, route):
    """The one-block k-split tile: three block rows with one empty, unsorted
    columns, both k-halves. The bias differs per logical column, so a bias
    taken from the block's position instead of its column index shows. One
    case per dtype takes a bias that is not 16-byte aligned."""
    a, b, _ = _small_operands(dtype, k)
    p = Problem(a, b, ta, tb, SMALL_OFFSETS, SMALL_INDICES, dtype)
    route(0)
    assert sp.sdd_act_route(p.A, ta, p.Bm, tb, p.c()[0]) == 1  # auto: fused
    act = ("relu", "gelu", "silu")[(k // 64 + ta + 2 * tb) % 3]
    _check_bias_products(p, dtype, act, (1, 2, 0), route,
                         unaligned=(k == 64 and not ta and tb))


@pytest.mark.parametrize("dtype,act,ta,tb", [
    ("f16", "relu", False, False), ("f16", "gelu", False, True),
    ("bf16", "silu", True, False), ("bf16", "relu", True, True)])
def test_grouped_tiles(dtype, act, ta, tb, route):
    """The fused epilogue on the grouped 128 x 512 tiles, groups of 1 to 4
    blocks at the row ends: the column of every block of a group."""
    a, b, _, offsets, indices = _grouped_problem_data(dtype)
    p = Problem(a, b, ta, tb, offsets, indices, dtype)
    assert sp.sdd_kernel(p.A, ta, p.Bm, tb, p.c()[0]) == 1
    _check_bias_products(p, dtype, act, (1, 2, 0), route,
                         unaligned=(ta and tb))


@pytest.mark.parametrize("dtype,act,ta,tb", [
    ("f16", "gelu", False, False), ("bf16", "silu", False, True)])
def test_grouped_route2_on_the_4wave_kernel(dtype, act, ta, tb, route):
    """What auto runs at MoE shapes: the plain SDD on the 4-wave grouped
    kernel, the elementwise kernel with the bias behind it."""
    a, b, _, offsets, indices = _grouped_problem_data(dtype, k=128)
    p = Problem(a, b, ta, tb, offsets, indices, dtype)
    c = p.c()[0]
    prev = sp.select_dsd_kernel(5)
    try:
        assert sp.sdd_kernel(p.A, ta, p.Bm, tb, c) == 3
        route(0)
        assert sp.sdd_act_route(p.A, ta, p.Bm, tb, c) == 2
        _check_bias_products(p, dtype, act, (1, 2, 0), route)
    finally:
        sp.select_dsd_kernel(prev)


@pytest.mark.parametrize("r", [1, 2])
def test_graph_capture(r, route):
    """Captured once per route, replayed twice: bit-identical to eager."""
    dtype, act = "bf16", "gelu"
    a, b, _ = _small_operands(dtype, 192)
    p = Problem(a, b, False, True, SMALL_OFFSETS, SMALL_INDICES, dtype)
    bias = _bias_dev(R.column_bias(p.n, dtype), dtype)
    route(r)
    gate = p.plain()
    eager = _bias_products(p, bias, act, gate)
    c0, cd = p.c()
    c1, h = p.c()
    c2, hg = p.c()
    z, u = torch.full_like(h, float("nan")), torch.full_like(h, float("nan"))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sp.MatmulBias(p.A, p.ta, p.Bm, p.tb, c0, bias)
        sp.MatmulBiasActivation(p.A, p.ta, p.Bm, p.tb, c1, bias, act, z)
        sp.MatmulBiasGated(p.A, p.ta, p.Bm, p.tb, c2, bias, act, gate, u)
    for _ in range(2):
        for t in (cd, h, z, hg, u):
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for x, i in ((cd, 0), (h, 1), (z, 2), (hg, 4), (u, 5)):
            assert _same(x, eager[i]), i
    del graph


def test_rejections_launch_nothing():
    a, b, _ = _small_operands("f16", 64)
    p = Problem(a, b, False, False, SMALL_OFFSETS, SMALL_INDICES, "f16")
    c, h = p.c()
    z = torch.full_like(h, float("nan"))
    ca, cb, cc = p.A._c(), p.Bm._c(), c._c()
    code = sp.lib().sputnik_sdd_bias(              # a null bias
        ctypes.byref(ca), 0, ctypes.byref(cb), 0, ctypes.byref(cc), None, 0,
        None, 0, sp._stream(None))
    assert code == HIP_ERROR_INVALID_VALUE
    with pytest.raises(sp.SputnikError):           # bias == C
        sp.MatmulBias(p.A, False, p.Bm, False, c, h.view(-1)[:p.n])
    with pytest.raises(sp.SputnikError):           # bias == Z
        sp.MatmulBiasActivation(p.A, False, p.Bm, False, c, z.view(-1)[:p.n],
                                "relu", z)
    with pytest.raises(sp.SputnikError):           # bias == A
        sp.MatmulBias(p.A, False, p.Bm, False, c, p.a_dev.view(-1)[:p.n])
    torch.cuda.synchronize()
    assert torch.isnan(h.float()).all() and torch.isnan(z.float()).all()


# ---- BlockColumnSum ---------------------------------------------------------

# 256 x 512: column blocks 1 and 3 hold nothing.
GAPPY_OFFSETS = [0, 2, 3]
GAPPY_INDICES = [2, 0, 2]
TOPOLOGIES = {"small": (384, 640, SMALL_OFFSETS, SMALL_INDICES),
              "gappy": (256, 512, GAPPY_OFFSETS, GAPPY_INDICES)}


def _sparse(name, values, dtype, transposed=True):
    rows, cols, offsets, indices = TOPOLOGIES[name]
    data = _dev(values, dtype)
    m = sp.BlockMatrix(rows, cols, B, len(indices) * B * B, data,
                       torch.tensor(offsets, dtype=torch.int32).cuda(),
                       torch.tensor(indices, dtype=torch.int16).cuda())
    if transposed:
        sp.AllocateTransposeBuffers(m)
        sp.Transpose(m)
    return m


def _column_sum(m):
    out = torch.full((m.cols,), float("nan"), dtype=torch.float32,
                     device="cuda")
    sp.BlockColumnSum(m, out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(TOPOLOGIES))
def test_column_sum(name, dtype):
    rows, cols, offsets, indices = TOPOLOGIES[name]
    nb = len(indices)
    rng = np.random.default_rng([nb, cols, dtype == "bf16"])
    # integers, |v| <= 8: every order of summation is exact
    ints = rng.integers(-8, 9, (nb, B, B)).astype(np.float32)
    ref, _, _ = R.column_sum64(ints, indices, cols)
    got = _column_sum(_sparse(name, ints, dtype))
    assert np.array_equal(got.view(np.uint32),
                          ref.astype(np.float32).view(np.uint32)), \
        "integer blocks: exact, +0 where a column block is empty"
    # random values of T
    vals = M.values((nb, B, B), dtype, [nb, cols, 5])
    m = _sparse(name, vals, dtype)
    got = _column_sum(m)
    ref, absum, n = R.column_sum64(vals, indices, cols)
    err = np.abs(got.astype(np.float64) - ref)
    bound = R.column_sum_bound(ref, absum, n)
    print(f"column_sum {name} {dtype}: max err / bound "
          f"{(err / np.maximum(bound, 1e-300)).max():.3g}")
    assert (err <= bound).all()
    assert np.array_equal(got.view(np.uint32), _column_sum(m).view(np.uint32)), \
        "two runs, the same bits"


def test_column_sum_needs_transposed_metadata():
    _, cols, _, indices = TOPOLOGIES["small"]
    m = _sparse("small", np.ones((len(indices), B, B)), "f16",
                transposed=False)
    out = torch.full((cols,), 7.0, dtype=torch.float32, device="cuda")
    with pytest.raises(sp.SputnikError):
        sp.BlockColumnSum(m, out)
    torch.cuda.synchronize()
    assert (out == 7.0).all()


# ---- the scatter with an output bias ----------------------------------------

def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def _weights(c, kind, dtype):
    """(numpy weights, device weights, their type name) of one kind."""
    if kind is None:
        return None, None, dtype
    if kind == "T":
        return c.w, _dev(c.w, dtype), dtype
    return c.w32, torch.from_numpy(np.array(c.w32)).cuda(), "f32"


def _scatter(y, b2, r, w, dtype, tokens):
    out = torch.full((tokens, y.shape[1]), float("nan"),
                     dtype=H.torch_dtype(dtype), device="cuda")
    sp.PaddedScatterBias(y, _i32(r.row_of), _i32(r.padded_bins), b2, out,
                         r.top_k, w)
    torch.cuda.synchronize()
    return out


_IDS = ["%dx%d-E%d-%s-h%d" % (*c, h) for c, h in R.scatter_cases()]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case,hidden", R.scatter_cases(), ids=_IDS)
def test_scatter_bias(case, hidden, dtype):
    tokens, top_k, e, kind = case
    c = M.case_inputs(case, hidden, dtype)
    r = c.route
    rows = M.exact_rows(r)
    b2_np = R.case_bias(case, hidden, dtype)
    y_np = np.array(c.y_cols[:rows])
    pad = np.ones(rows, dtype=bool)
    pad[r.row_of] = False
    y_np[pad] = np.nan            # padding rows must not be read
    y, b2 = _dev(y_np, dtype), _dev(b2_np, dtype)
    dout = _dev(c.dout, dtype)
    for wkind in (None, "T", "f32"):
        w_np, w, _ = _weights(c, wkind, dtype)
        what = f"{case} h={hidden} {dtype} weights={wkind}"
        got = _f32(_scatter(y, b2, r, w, dtype, tokens))
        assert np.isfinite(got).all(), f"{what}: a padding row was read"
        ref32 = R.scatter32(y_np, b2_np, r, w_np, dtype)
        assert np.array_equal(got.view(np.uint32), ref32.view(np.uint32)), \
            f"{what}: out != the fp32 reference"
        ref64, absum = R.scatter64(y_np, b2_np, r, w_np)
        err = np.abs(got.astype(np.float64) - ref64)
        assert (err <= R.scatter_bound(ref64, absum, top_k, dtype)).all(), what
        # db2, from the unrounded products, no atomics
        db = torch.full((e, hidden), float("nan"), dtype=torch.float32,
                        device="cuda")
        sp.PaddedScatterBiasGrad(dout, _i32(r.indices), _i32(r.bins), db,
                                 top_k, w)
        db_again = torch.full_like(db, float("nan"))
        sp.PaddedScatterBiasGrad(dout, _i32(r.indices), _i32(r.bins),
                                 db_again, top_k, w)
        torch.cuda.synchronize()
        g = db.cpu().numpy()
        ref, ab, cnt = R.bgrad64(c.dout, r, e, w_np)
        assert (np.abs(g.astype(np.float64) - ref)
                <= R.bgrad_bound(ref, ab, cnt)).all(), f"{what}: db2"
        assert (g[cnt == 0].view(np.uint32) == 0).all(), \
            f"{what}: an expert without tokens gives +0"
        assert np.array_equal(g.view(np.uint32),
                              db_again.cpu().numpy().view(np.uint32)), \
            f"{what}: db2, two runs"
    if kind == "empty":
        assert (r.tokens_per_expert == 0).any()
    # dw, in T and in fp32: operands signed so that no sum cancels
    y_rows, b_abs = _dev(c.y_rows[:rows], dtype), \
        _dev(R.case_bias_abs(case, hidden, dtype), dtype)
    d_abs = _dev(c.dout_abs, dtype)
    ref, ab = R.wgrad64(c.dout_abs, c.y_rows[:rows],
                        R.case_bias_abs(case, hidden, dtype), r)
    for out_type, td in ((dtype, H.torch_dtype(dtype)),
                         ("f32", torch.float32)):
        dw = torch.full((tokens * top_k,), float("nan"), dtype=td,
                        device="cuda")
        sp.PaddedScatterBiasWeightGrad(d_abs, y_rows, _i32(r.row_of),
                                       _i32(r.padded_bins), b_abs, dw, top_k)
        torch.cuda.synchronize()
        err = np.abs(_f32(dw).astype(np.float64) - ref)
        assert (err <= M.wgrad_bound(ref, ab, hidden + 1, out_type)).all(), \
            f"{case} h={hidden} {dtype}: dw in {out_type}"


@pytest.mark.parametrize("dtype", DTYPES)
def test_scatter_bias_row_out_of_range(dtype):
    """A row_of entry of -1 contributes zero, its bias included."""
    case, hidden = (129, 2, 4, "empty"), 264
    c = M.case_inputs(case, hidden, dtype)
    row_of = np.array(c.route.row_of)
    row_of[[0, 5, 6, 7]] = -1            # one and both picks of a token
    r = c.route._replace(row_of=row_of)
    rows = M.exact_rows(r)
    b2_np = R.case_bias(case, hidden, dtype)
    y, b2 = _dev(c.y_cols[:rows], dtype), _dev(b2_np, dtype)
    for wkind in (None, "f32"):
        w_np, w, _ = _weights(c, wkind, dtype)
        got = _f32(_scatter(y, b2, r, w, dtype, case[0]))
        ref = R.scatter32(c.y_cols[:rows], b2_np, r, w_np, dtype)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert (got[3] == 0).all(), "token 3 lost both picks"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case,hidden", [R.DEEP_CASE,
                                         ((129, 2, 4, "empty"), 264)],
                         ids=["deep", "empty"])
def test_wgrad_with_a_zero_bias_is_the_plain_wgrad(case, hidden, dtype):
    """PaddedScatterBiasWeightGrad with an all +0 bias equals
    PaddedScatterWeightGrad bit for bit, dw of T and of fp32, on the 16-byte
    path and (buffers offset by 4 elements) the element path: the two are
    one kernel body, the sum order is the same, and y + 0 changes no term
    in a way that can change the sum."""
    c = M.case_inputs(case, hidden, dtype)
    r, td = c.route, H.torch_dtype(dtype)
    rows, n = M.exact_rows(r), r.tokens * r.top_k
    row_of, padded_bins = _i32(r.row_of), _i32(r.padded_bins)

    def put(values, offset):
        flat = torch.zeros(values.size + offset, dtype=td, device="cuda")
        assert flat.data_ptr() % 16 == 0
        t = flat[offset:].view(*values.shape)
        t.copy_(_dev(values, dtype))
        return t
    for offset in (0, 4):
        dout, y = put(c.dout, offset), put(c.y[:rows], offset)
        zero = put(np.zeros((case[2], hidden), dtype=np.float32), offset)
        for wd in (td, torch.float32):
            plain = torch.full((n,), float("nan"), dtype=wd, device="cuda")
            biased = torch.full_like(plain, float("nan"))
            sp.PaddedScatterWeightGrad(dout, y, row_of, plain, r.top_k)
            sp.PaddedScatterBiasWeightGrad(dout, y, row_of, padded_bins, zero,
                                           biased, r.top_k)
            torch.cuda.synchronize()
            assert not torch.isnan(plain.float()).any()
            assert torch.equal(plain.view(torch.uint8),
                               biased.view(torch.uint8)), \
                f"offset {offset}, dw {wd}"


@pytest.mark.parametrize("dtype", DTYPES)
def test_scatter_bias_integers_are_exact(dtype):
    """Integer y, b2 and dout with unit weights: every order is exact."""
    hidden = 264
    r = M.case_route((300, 2, 4, "exact"))
    tokens, top_k, e = r.tokens, r.top_k, 4
    rows = M.exact_rows(r)
    rng = np.random.default_rng(11)
    y_np = rng.integers(-8, 9, (rows, hidden)).astype(np.float32)
    b_np = rng.integers(-8, 9, (e, hidden)).astype(np.float32)
    d_np = rng.integers(-8, 9, (tokens, hidden)).astype(np.float32)
    ones = np.ones(tokens * top_k, dtype=np.float32)
    y, b2, dout, w = (_dev(a, dtype) for a in (y_np, b_np, d_np, ones))
    got = _f32(_scatter(y, b2, r, w, dtype, tokens))
    ref, _ = R.scatter64(y_np, b_np, r, ones)
    assert np.array_equal(got.astype(np.float64), ref)
    db = torch.empty((e, hidden), dtype=torch.float32, device="cuda")
    sp.PaddedScatterBiasGrad(dout, _i32(r.indices), _i32(r.bins), db, top_k, w)
    dw = torch.empty(tokens * top_k, dtype=torch.float32, device="cuda")
    sp.PaddedScatterBiasWeightGrad(dout, y, _i32(r.row_of),
                                   _i32(r.padded_bins), b2, dw, top_k)
    torch.cuda.synchronize()
    assert np.array_equal(db.cpu().numpy().astype(np.float64),
                          R.bgrad64(d_np, r, e, ones)[0])
    assert np.array_equal(dw.cpu().numpy().astype(np.float64),
                          R.wgrad64(d_np, y_np, b_np, r)[0])
