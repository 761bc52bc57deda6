"""CPU: the host side of the MoE token permutation (sputnik/block/moe.h).
The numpy reference checks itself (tests/moe_ref.py), and its float32
emulations meet the bounds the GPU tests hold the kernels to, on the very
cases and seeds those tests use. The Python entry points exist, type and
shape errors are raised before the library is called, the C and C++ symbols
are exported, and every C entry point rejects what include/sputnik_amd.h
lists, without a device and without aborting. No compute call is made."""

import ctypes
import inspect
import subprocess

import numpy as np
import pytest

import sputnik_amd as sp
from oracle import oracle as O
from tests import moe_ref as R
from tests.test_cpp_moe import SYMBOLS

torch = pytest.importorskip("torch")


# ---- the reference checks itself --------------------------------------------

@pytest.mark.parametrize("case", [c for c in R.CASES if c[1] == 1])
def test_gather_then_unweighted_scatter_returns_x_at_top_k_1(case):
    c = R.case_inputs(case, 100, "bf16")
    r, x = c.route, c.x
    xp = R.gather(x, r, R.exact_rows(r))
    back = R.scatter32(xp, r, None, "bf16")
    assert np.array_equal(back.view(np.uint32), x.view(np.uint32))


@pytest.mark.parametrize("case", R.CASES)
def test_row_of_is_a_bijection_onto_the_non_padding_rows(case):
    r = R.case_route(case)
    n = case[0] * case[1]
    bin0 = np.concatenate([[0], r.padded_bins[:-1]])
    live = np.concatenate([np.arange(b, b + c) for b, c in
                           zip(bin0, r.tokens_per_expert)])
    assert r.row_of.size == n == live.size
    assert np.array_equal(np.sort(r.row_of), live)
    # and every assignment sits in its own expert's bin
    flat = R.routing(*case).reshape(-1)
    assert np.array_equal(np.searchsorted(r.padded_bins, r.row_of, "right"),
                          flat)
    assert np.array_equal(r.bin_ids, flat[r.indices])


def test_rows_bound_covers_every_routing():
    from sputnik_amd import ops
    rng = np.random.default_rng(11)
    tight = 0
    for trial in range(300):
        e = int(rng.integers(1, 17))
        tokens, top_k = int(rng.integers(1, 400)), int(rng.integers(1, 5))
        n = tokens * top_k
        kind = trial % 4
        if kind == 0:      # uniform, some experts empty when n < e
            flat = rng.integers(0, e, n)
        elif kind == 1:    # as many experts as fit at exactly 128, rest on one
            flat = np.repeat(np.arange(e), 128)[:n]
            flat = np.concatenate([flat, np.full(n - flat.size, e - 1)])
        elif kind == 2:    # everything on one expert
            flat = np.full(n, int(rng.integers(0, e)))
        else:              # the worst case: 1 past a multiple of 128 each
            flat = np.repeat(np.arange(e), 129)[:n]
            flat = np.concatenate([flat, np.full(n - flat.size, 0)])
        r = R.route(flat.reshape(tokens, top_k), e)
        bound = ops.moe_rows_bound(n, e)
        assert bound == R.rows_bound(n, e) and bound % 128 == 0
        assert bound >= n + 127 * e > bound - 128
        assert bound >= R.exact_rows(r)
        tight += R.exact_rows(r) > bound - 128 - 127
    assert tight > 0  # (the bound is reached, up to its own rounding)


# ---- the emulation meets the GPU tests' bounds ------------------------------

@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("case", R.CASES + [R.DEEP_CASE[0]])
def test_emulation_meets_the_fp32_weight_scatter_bound(case, dtype):
    for hidden in R.scatter_hiddens(case):
        c = R.case_inputs(case, hidden, dtype)
        r = c.route
        got = R.scatter32(c.y_cols, r, c.w32, dtype).astype(np.float64)
        ref, absum = R.scatter64(c.y_cols, r, c.w32)
        assert (np.abs(got - ref)
                <= R.scatter_bound(ref, absum, r.top_k, dtype)).all()


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("case", R.CASES + [R.DEEP_CASE[0]])
def test_emulation_meets_the_wgrad_bound(case, dtype):
    for hidden in R.scatter_hiddens(case):
        c = R.case_inputs(case, hidden, dtype)
        acc = R.wgrad32(c.dout_abs, c.y_rows, c.route)
        ref, absum = R.wgrad64(c.dout_abs, c.y_rows, c.route)
        assert ref.size < 100 or ((ref > 0).any() and (ref < 0).any())
        for out_type, got in (("f32", acc), (dtype, O.round_to(acc, dtype))):
            assert (np.abs(got.astype(np.float64) - ref)
                    <= R.wgrad_bound(ref, absum, hidden, out_type)).all()


def test_t_weight_products_are_exact_in_fp32():
    """What makes the T-weight scatter and gather bit-exact checks
    independent of fma contraction."""
    for dtype in R.DTYPES:
        c = R.case_inputs(R.CASES[6], 264, dtype)
        r, y, w = c.route, c.y, c.w
        p64 = w.astype(np.float64)[:, None] * y.astype(np.float64)[r.row_of]
        assert np.array_equal(p64.astype(np.float32).astype(np.float64), p64)
        assert (np.abs(y) >= 2.0 ** -10).all() and (np.abs(y) <= 4).all()
        assert (w > 0).all() and (w <= 1).all()


# ---- entry points -----------------------------------------------------------

def test_python_entry_points_exist():
    from sputnik_amd import ops
    sig = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert sig(sp.MoeBins) == ["bin_ids", "num_experts", "bins",
                               "tokens_per_expert", "padded_bins", "stream"]
    assert sig(sp.MoeRowMap) == ["indices", "bin_ids", "bins", "padded_bins",
                                 "rows", "row_of", "stream"]
    assert sig(sp.PaddedGather) == ["x", "indices", "bins", "padded_bins",
                                    "out", "top_k", "weights", "stream"]
    assert sig(sp.PaddedScatter) == ["y", "row_of", "out", "top_k", "weights",
                                     "stream"]
    assert sig(sp.PaddedScatterWeightGrad) == ["dout", "y", "row_of", "dw",
                                               "top_k", "stream"]
    for name in ("MoeBins", "MoeRowMap", "PaddedGather", "PaddedScatter",
                 "PaddedScatterWeightGrad", "SPUTNIK_WEIGHTS_OPERAND",
                 "SPUTNIK_WEIGHTS_F32"):
        assert name in sp.__all__, name
    assert sp.SPUTNIK_WEIGHTS_OPERAND == 0 and sp.SPUTNIK_WEIGHTS_F32 == 1
    assert sig(ops.moe_rows_bound) == ["n", "num_experts"]
    assert sig(ops.moe_route) == ["top_experts", "num_experts", "rows"]
    assert sig(ops.MoeRoute.from_megablocks) == [
        "indices", "bin_ids", "bins", "padded_bins", "top_k", "rows"]
    assert sig(ops.padded_gather) == ["x", "route"]
    assert sig(ops.padded_scatter) == ["y", "route", "weights"]
    assert sig(ops.moe_mlp) == ["x", "top_experts", "expert_weights", "w1",
                                "w2", "num_experts", "activation", "v1",
                                "rows"]
    for name in ("MoeRoute", "moe_rows_bound", "moe_route", "padded_gather",
                 "padded_scatter", "moe_mlp"):
        assert name in ops.__all__, name
    assert [f.name for f in ops.MoeRoute.__dataclass_fields__.values()] == [
        "indices", "bin_ids", "bins", "padded_bins", "tokens_per_expert",
        "row_of", "top_k", "tokens", "rows"]
    assert ops.moe_rows_bound(0, 0) == 0
    assert ops.moe_rows_bound(1, 1) == 128
    assert ops.moe_rows_bound(2, 1) == 256


def _exported():
    return subprocess.run(["nm", "-D", "--defined-only", sp.LIB_PATH],
                          capture_output=True, text=True, check=True).stdout


C_ENTRIES = ("sputnik_moe_bins", "sputnik_moe_row_map",
             "sputnik_padded_gather", "sputnik_padded_scatter",
             "sputnik_padded_scatter_wgrad")


def test_c_and_cpp_symbols_exported():
    out = _exported().split()
    for s in C_ENTRIES + SYMBOLS:
        assert s in out, s
    for s in C_ENTRIES:
        assert hasattr(sp.lib(), s)


# ---- errors raised before the library is called -----------------------------

@pytest.fixture
def no_library(monkeypatch):
    """Any use of the library fails the test."""
    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(sp, "lib", boom)


def _i32(n):
    return torch.zeros(n, dtype=torch.int32)


def _mat(rows, cols, dtype=torch.bfloat16):
    return torch.zeros(rows, cols, dtype=dtype)


def test_binding_errors_raise_before_the_library(no_library):
    x, out = _mat(4, 16), _mat(128, 16)
    idx, bins = _i32(8), _i32(2)
    ok = dict(x=x, indices=idx, bins=bins, padded_bins=bins, out=out, top_k=2)

    def gather(**kw):
        sp.PaddedGather(**{**ok, **kw})

    for bad in (dict(x=_mat(4, 16, torch.float32)),          # not fp16 / bf16
                dict(out=_mat(128, 16, torch.float16)),      # another dtype
                dict(indices=_i32(8).long()),                # not int32
                dict(weights=torch.zeros(8, dtype=torch.float16))):
        with pytest.raises(TypeError):
            gather(**bad)
    for bad in (dict(out=_mat(128, 24)),                     # another hidden
                dict(out=_mat(100, 16)),                     # rows % 128
                dict(indices=_i32(7)),                       # != tokens * top_k
                dict(top_k=0),
                dict(x=torch.zeros(16, dtype=torch.bfloat16)),   # 1-D
                dict(x=_mat(4, 32)[:, ::2]),                 # not contiguous
                dict(padded_bins=_i32(3)),
                dict(weights=torch.zeros(7))):
        with pytest.raises(ValueError):
            gather(**bad)

    y, tok = _mat(128, 16), _mat(4, 16)
    with pytest.raises(TypeError):
        sp.PaddedScatter(y, _i32(8), _mat(4, 16, torch.float16), 2)
    with pytest.raises(TypeError):
        sp.PaddedScatter(y, _i32(8).long(), tok, 2)
    with pytest.raises(TypeError):
        sp.PaddedScatter(y, _i32(8), tok, 2,
                         weights=torch.zeros(8, dtype=torch.float64))
    with pytest.raises(ValueError):
        sp.PaddedScatter(y, _i32(9), tok, 2)
    with pytest.raises(ValueError):
        sp.PaddedScatter(_mat(100, 16), _i32(8), tok, 2)
    with pytest.raises(TypeError):
        sp.PaddedScatterWeightGrad(tok, y, _i32(8),
                                   torch.zeros(8, dtype=torch.float16), 2)
    with pytest.raises(ValueError):
        sp.PaddedScatterWeightGrad(tok, _mat(128, 24), _i32(8),
                                   torch.zeros(8), 2)
    with pytest.raises(TypeError):
        sp.MoeBins(_i32(8).long(), 2, bins, _i32(2), _i32(2))
    with pytest.raises(ValueError):
        sp.MoeBins(_i32(8), 3, bins, _i32(2), _i32(2))
    with pytest.raises(ValueError):
        sp.MoeRowMap(idx, _i32(8), bins, bins, 100, _i32(8))
    with pytest.raises(ValueError):
        sp.MoeRowMap(idx, _i32(7), bins, bins, 128, _i32(8))


def test_ops_errors_raise_before_the_library(no_library):
    from sputnik_amd import ops
    top = torch.zeros(4, 2, dtype=torch.int64)
    with pytest.raises(TypeError):
        ops.moe_route(top.float(), 2)
    with pytest.raises(ValueError):
        ops.moe_route(top, 0)
    with pytest.raises(ValueError):
        ops.moe_route(top.reshape(2, 2, 2), 2)
    for rows in (ops.moe_rows_bound(8, 2) - 128, ops.moe_rows_bound(8, 2) + 1):
        with pytest.raises(ValueError):
            ops.moe_route(top, 2, rows=rows)
    with pytest.raises(ValueError):
        ops.MoeRoute.from_megablocks(_i32(8), _i32(8), _i32(2), _i32(2), 2,
                                     rows=128)
    with pytest.raises(ValueError):
        ops.MoeRoute.from_megablocks(_i32(8), _i32(7), _i32(2), _i32(2), 2)
    with pytest.raises(ValueError):
        ops.MoeRoute.from_megablocks(_i32(9), _i32(9), _i32(2), _i32(2), 2)
    with pytest.raises(TypeError):
        ops.MoeRoute.from_megablocks(_i32(8).float(), _i32(8), _i32(2),
                                     _i32(2), 2)

    route = ops.MoeRoute(_i32(8), _i32(8), _i32(2), _i32(2), _i32(2), _i32(8),
                         top_k=2, tokens=4, rows=384)
    with pytest.raises(TypeError):
        ops.padded_gather(_mat(4, 16), "route")
    with pytest.raises(TypeError):
        ops.padded_gather(_mat(4, 16, torch.float32), route)
    with pytest.raises(ValueError):
        ops.padded_gather(_mat(5, 16), route)
    with pytest.raises(ValueError):
        ops.padded_scatter(_mat(256, 16), route)
    with pytest.raises(TypeError):
        ops.padded_scatter(_mat(384, 16), route,
                           torch.zeros(4, 2, dtype=torch.float16))
    with pytest.raises(ValueError):
        ops.padded_scatter(_mat(384, 16), route, torch.zeros(2, 4))

    x = _mat(4, 256)
    w1, w2, ew = _mat(256, 512), _mat(512, 256), torch.zeros(4, 2)
    with pytest.raises(TypeError):
        ops.moe_mlp(x, top, ew, w1.half(), w2, 2)
    with pytest.raises(TypeError):
        ops.moe_mlp(x, top, ew.double(), w1, w2, 2)
    with pytest.raises(ValueError):
        ops.moe_mlp(x, top, ew, w1, w2, 3)           # 512 columns, 3 experts
    with pytest.raises(ValueError):
        ops.moe_mlp(x, top, ew, w1, w2.t(), 2)
    with pytest.raises(ValueError):
        ops.moe_mlp(x, top, ew, w1, w2, 2, v1=_mat(256, 256))
    with pytest.raises(ValueError):
        ops.moe_mlp(x, top, torch.zeros(4, 3), w1, w2, 2)
    with pytest.raises(ValueError):
        ops.moe_mlp(_mat(5, 256), top, ew, w1, w2, 2)
    with pytest.raises(ValueError):
        ops.moe_mlp(x, top, ew, w1, w2, 2, activation="tanh")
    with pytest.raises(ValueError):
        ops.moe_mlp(x, top, ew, w1, w2, 2, rows=128)


# ---- the C entry points reject, never abort (no device is touched) ----------

A, B, C, D, E_, F = (ctypes.c_void_p(0x1000 * i) for i in range(1, 7))
NULL = None


def test_moe_bins_rejections():
    f = sp.lib().sputnik_moe_bins
    bad = sp.hipErrorInvalidValue
    assert f(A, -1, 4, B, C, D, NULL) == bad
    assert f(A, 8, -1, B, C, D, NULL) == bad
    assert f(A, 2 ** 31 - 1, 1, B, C, D, NULL) == bad      # n + 127 E
    for args in ((NULL, 8, 4, B, C, D), (A, 8, 4, NULL, C, D),
                 (A, 8, 4, B, NULL, D), (A, 8, 4, B, C, NULL)):
        assert f(*args, NULL) == bad
    for args in ((A, 8, 4, A, C, D), (A, 8, 4, B, A, D), (A, 8, 4, B, C, A),
                 (A, 8, 4, B, B, D), (A, 8, 4, B, C, C)):
        assert f(*args, NULL) == bad
    assert f(NULL, 8, 0, NULL, NULL, NULL, NULL) == 0       # no expert


def test_moe_row_map_rejections():
    f = sp.lib().sputnik_moe_row_map
    bad = sp.hipErrorInvalidValue
    assert f(A, B, C, D, -1, 4, 128, E_, NULL) == bad
    assert f(A, B, C, D, 8, -1, 128, E_, NULL) == bad
    assert f(A, B, C, D, 8, 4, -128, E_, NULL) == bad
    assert f(A, B, C, D, 8, 4, 100, E_, NULL) == bad
    for i in range(5):
        args = [A, B, C, D, 8, 4, 128, E_]
        args[i if i < 4 else 7] = NULL
        assert f(*args, NULL) == bad
    for p in (A, B, C, D):
        assert f(A, B, C, D, 8, 4, 128, p, NULL) == bad
    assert f(NULL, NULL, NULL, NULL, 0, 4, 128, NULL, NULL) == 0


def test_padded_gather_rejections():
    f = sp.lib().sputnik_padded_gather
    bad = sp.hipErrorInvalidValue

    def call(x=A, indices=B, bins=C, padded=D, w=NULL, out=F, tokens=4,
             hidden=16, top_k=2, e=2, rows=128, dtype=1, wdtype=0):
        return f(x, indices, bins, padded, w, out, tokens, hidden, top_k, e,
                 rows, dtype, wdtype, NULL)

    for kw in (dict(tokens=-1), dict(hidden=-1), dict(e=-1), dict(rows=-128),
               dict(top_k=0), dict(top_k=-2), dict(rows=100), dict(rows=129),
               dict(dtype=2), dict(dtype=-1), dict(w=E_, wdtype=2),
               dict(tokens=2 ** 30, top_k=2),
               dict(x=NULL), dict(indices=NULL), dict(bins=NULL),
               dict(padded=NULL), dict(out=NULL),
               dict(out=A), dict(out=B), dict(out=C), dict(out=D),
               dict(w=F)):
        assert call(**kw) == bad, kw
    assert call(rows=0, out=NULL) == 0
    assert call(hidden=0, out=NULL) == 0


def test_padded_scatter_rejections():
    f = sp.lib().sputnik_padded_scatter
    bad = sp.hipErrorInvalidValue

    def call(y=A, row_of=B, w=NULL, out=F, tokens=4, hidden=16, top_k=2,
             rows=128, dtype=0, wdtype=0):
        return f(y, row_of, w, out, tokens, hidden, top_k, rows, dtype,
                 wdtype, NULL)

    for kw in (dict(tokens=-1), dict(hidden=-1), dict(rows=-128),
               dict(top_k=0), dict(rows=100), dict(dtype=2),
               dict(w=E_, wdtype=-1), dict(tokens=2 ** 30, top_k=2),
               dict(y=NULL), dict(row_of=NULL), dict(out=NULL),
               dict(out=A), dict(out=B), dict(w=F)):
        assert call(**kw) == bad, kw
    assert call(tokens=0, out=NULL) == 0
    assert call(hidden=0, out=NULL) == 0


def test_padded_scatter_wgrad_rejections():
    f = sp.lib().sputnik_padded_scatter_wgrad
    bad = sp.hipErrorInvalidValue

    def call(dout=A, y=B, row_of=C, dw=F, tokens=4, hidden=16, top_k=2,
             rows=128, dtype=0, wdtype=1):
        return f(dout, y, row_of, dw, tokens, hidden, top_k, rows, dtype,
                 wdtype, NULL)

    for kw in (dict(tokens=-1), dict(hidden=-1), dict(rows=-128),
               dict(top_k=0), dict(rows=100), dict(dtype=2), dict(wdtype=2),
               dict(tokens=2 ** 30, top_k=2),
               dict(dout=NULL), dict(y=NULL), dict(row_of=NULL),
               dict(dw=NULL), dict(dw=A), dict(dw=B), dict(dw=C)):
        assert call(**kw) == bad, kw
    assert call(tokens=0, dw=NULL) == 0
