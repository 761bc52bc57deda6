"""CPU: the host side of the MoE router and the device sort
(sputnik/block/router.h). The float32 emulations of tests/router_ref.py meet
the bounds the GPU tests hold the kernels to, on the very inputs those tests
use; the reference picks and the sort reference check themselves; the Python
entry points exist, type and shape errors are raised before the library is
called, the C and C++ symbols are exported, and every C entry point rejects
what include/sputnik_amd.h lists, without a device and without aborting. No
compute call is made."""

import ctypes
import inspect
import subprocess

import numpy as np
import pytest

import sputnik_amd as sp
from tests import moe_ref
from tests import router_ref as R
from tests.test_cpp_router import SYMBOLS

torch = pytest.importorskip("torch")

_IDS = ["%dx%d-k%d" % c for c in R.ROUTER_CASES]
VALUE_KINDS = ["random", "ties", "equal"]     # ("special": only ids pinned)


def _wtypes(ltype):
    return [ltype] if ltype == "f32" else [ltype, "f32"]


# ---- the references check themselves ----------------------------------------

@pytest.mark.parametrize("case", R.ROUTER_CASES, ids=_IDS)
def test_reference_picks(case):
    tokens, e, k = case
    for ltype in R.LTYPES:
        for kind in R.KINDS:
            l = R.logits(case, kind, ltype)
            assert l.shape == (tokens, e)
            if ltype != "f32":      # representable in the type
                with np.errstate(invalid="ignore"):
                    assert np.array_equal(R.rnd(l, ltype), l, equal_nan=True)
            ids = R.expected_ids(l, k)
            assert ids.shape == (tokens, k)
            assert ((ids >= 0) & (ids < e)).all()
            assert all(len(set(row)) == k for row in ids.tolist())
            if kind == "equal":
                assert (ids == np.arange(k)).all()
            if kind == "random":
                assert (l.max(axis=1, keepdims=True) - l <= 16).all()
            # descending, NaN last, ties in ascending index
            v = np.take_along_axis(l, ids.astype(np.int64), axis=1)
            for row_v, row_i in zip(v.tolist(), ids.tolist()):
                for a, b, ia, ib in zip(row_v, row_v[1:], row_i, row_i[1:]):
                    if np.isnan(a):
                        assert np.isnan(b) and ia < ib
                    elif not np.isnan(b):
                        assert a > b or (a == b and ia < ib)
    special = R.logits(case, "special", "f32")
    assert not np.isfinite(special).all()


def test_ties_reach_the_boundary():
    """In the "ties" inputs the k-th and (k+1)-th largest are equal in every
    row, so the tie rule decides the picks."""
    for case in R.ROUTER_CASES:
        tokens, e, k = case
        if k == e:
            continue
        for ltype in R.LTYPES:
            s = -np.sort(-R.logits(case, "ties", ltype), axis=1)
            assert (s[:, k - 1] == s[:, k]).all()


def test_sort_reference_agrees_with_moe_ref_on_valid_ids():
    for n, e in R.SORT_CASES:
        ids = R.sort_ids(n, e)
        a = R.sort_ref(ids, e, moe_ref.rows_bound(n, e))
        b = moe_ref.route(ids.astype(np.int64).reshape(n, 1), e)
        for name in ("indices", "bin_ids", "bins", "padded_bins",
                     "tokens_per_expert", "row_of"):
            assert np.array_equal(getattr(a, name), getattr(b, name)), name
    n, e = R.OUT_OF_RANGE_CASE
    ids = R.out_of_range_ids()
    r = R.sort_ref(ids, e, moe_ref.rows_bound(n, e))
    bad = (ids < 0) | (ids >= e)
    assert bad.sum() >= 40 and r.bins[-1] == n - bad.sum()
    assert (r.row_of[bad] == -1).all() and (r.row_of[~bad] >= 0).all()
    assert (r.bin_ids[r.bins[-1]:] == e).all()
    assert np.array_equal(r.indices[r.bins[-1]:], np.flatnonzero(bad))
    assert sorted(r.indices.tolist()) == list(range(n))


# ---- the emulation meets the GPU tests' bounds ------------------------------

@pytest.mark.parametrize("ltype", R.LTYPES)
@pytest.mark.parametrize("case", R.ROUTER_CASES, ids=_IDS)
def test_emulation_meets_the_forward_bounds(case, ltype):
    tokens, e, k = case
    worst = 0.0
    for kind in VALUE_KINDS:
        l = R.logits(case, kind, ltype)
        ids = R.expected_ids(l, k)
        for normalize in (False, True):
            w_ref, p_ref = R.forward64(l, ids, normalize)
            for wtype in _wtypes(ltype):
                w, p = R.forward32(l, ids, normalize, wtype)
                wb = R.weights_bound(w_ref, e, k, wtype)
                pb = R.scores_bound(p_ref, e, wtype)
                assert (np.abs(w - w_ref) <= wb).all()
                assert (np.abs(p - p_ref) <= pb).all()
                if wtype == "f32":  # (the share of the fp32 terms alone)
                    worst = max(worst, float((np.abs(w - w_ref) / wb).max()),
                                float((np.abs(p - p_ref) / pb).max()))
    print("forward: largest share of the fp32 bound", worst)


@pytest.mark.parametrize("ltype", R.LTYPES)
@pytest.mark.parametrize("case", R.ROUTER_CASES, ids=_IDS)
def test_emulation_meets_the_gradient_bound(case, ltype):
    tokens, e, k = case
    l = R.logits(case, "random", ltype)
    ids = R.grad_ids(case, ltype)
    for wtype in _wtypes(ltype):
        dw, ds = R.grad_inputs(case, ltype, wtype)
        for normalize in (False, True):
            for dscores in (None, ds):
                ref, image = R.grad64(l, ids, dw, dscores, normalize)
                got = R.grad32(l, ids, dw, dscores, normalize, ltype)
                assert np.isfinite(ref).all()
                assert (np.abs(got - ref)
                        <= R.grad_bound(ref, image, e, k, ltype)).all()


def test_gradient_reference_against_autograd():
    """grad64 is the derivative of forward64 (float64 torch autograd), and
    its out-of-range and repeated picks behave as router.h says."""
    case, ltype = (67, 8, 2), "f32"
    l = R.logits(case, "random", ltype)
    ids = R.expected_ids(l, case[2])
    dw, ds = R.grad_inputs(case, ltype, "f32")
    for normalize in (False, True):
        lt = torch.from_numpy(np.array(l)).double().requires_grad_(True)
        p = torch.softmax(lt, dim=1)
        w = torch.gather(p, 1, torch.from_numpy(ids.astype(np.int64)))
        if normalize:
            w = w / w.sum(dim=1, keepdim=True)
        ((w * torch.from_numpy(np.array(dw)).double()).sum()
         + (p * torch.from_numpy(np.array(ds)).double()).sum()).backward()
        ref, _ = R.grad64(l, ids, dw, ds, normalize)
        assert np.allclose(ref, lt.grad.numpy(), rtol=1e-10, atol=1e-14)
    # an out-of-range pick contributes nothing; a repeated one adds twice
    one = ids[:, :1]
    base, _ = R.grad64(l, one, dw[:, :1], None, False)
    with_bad = np.concatenate([one, np.full_like(one, 8)], axis=1)
    got, _ = R.grad64(l, with_bad, dw, None, False)
    assert np.array_equal(got, base)
    twice, _ = R.grad64(l, np.concatenate([one, one], axis=1),
                        np.concatenate([dw[:, :1], dw[:, :1]], axis=1), None,
                        False)
    assert np.allclose(twice, 2 * base, rtol=1e-12, atol=0)


# ---- entry points -----------------------------------------------------------

def test_python_entry_points_exist():
    from sputnik_amd import ops
    sig = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert sig(sp.RouterTopK) == ["logits", "top_experts", "weights",
                                  "normalize", "scores", "stream"]
    assert sig(sp.RouterTopKGrad) == ["logits", "top_experts", "dweights",
                                      "dlogits", "normalize", "dscores",
                                      "stream"]
    assert sig(sp.MoeSort) == ["top_experts", "num_experts", "rows",
                               "indices", "bin_ids", "bins",
                               "tokens_per_expert", "padded_bins", "row_of",
                               "workspace", "stream"]
    assert sig(sp.moe_sort_workspace_bytes) == ["n", "num_experts"]
    for name in ("RouterTopK", "RouterTopKGrad", "MoeSort",
                 "moe_sort_workspace_bytes", "SPUTNIK_ROUTER_F16",
                 "SPUTNIK_ROUTER_BF16", "SPUTNIK_ROUTER_F32",
                 "MOE_SORT_CHUNK"):
        assert name in sp.__all__, name
    assert (sp.SPUTNIK_ROUTER_F16, sp.SPUTNIK_ROUTER_BF16,
            sp.SPUTNIK_ROUTER_F32) == (0, 1, 2)
    assert sp.MOE_SORT_CHUNK == R.CHUNK
    assert sig(ops.moe_router) == ["logits", "top_k", "normalize",
                                   "weights_dtype", "return_scores"]
    assert sig(ops.moe_layer) == ["x", "router_weight", "w1", "w2", "top_k",
                                  "activation", "v1", "rows", "normalize",
                                  "router_dtype", "device_sort",
                                  "return_scores"]
    assert sig(ops.moe_device_route) == sig(ops.moe_route) == [
        "top_experts", "num_experts", "rows"]
    assert inspect.signature(ops.moe_layer).parameters[
        "device_sort"].default is True
    for name in ("moe_router", "moe_layer", "moe_device_route"):
        assert name in ops.__all__, name


def test_header_names_the_chunk_constant():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "sputnik", "block",
                             "router.h")).read()
    assert "constexpr int kMoeSortChunk = %d;" % R.CHUNK in text
    assert "enum class RouterType { kF16 = 0, kBF16 = 1, kF32 = 2 }" in text
    umbrella = open(os.path.join(root, "include", "sputnik",
                                 "sputnik.h")).read()
    assert '#include "sputnik/block/router.h"' in umbrella


C_ENTRIES = ("sputnik_router_topk", "sputnik_router_topk_grad",
             "sputnik_moe_sort", "sputnik_moe_sort_workspace_bytes")


def test_c_and_cpp_symbols_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", sp.LIB_PATH],
                         capture_output=True, text=True,
                         check=True).stdout.split()
    for s in C_ENTRIES + SYMBOLS:
        assert s in out, s
    for s in C_ENTRIES:
        assert hasattr(sp.lib(), s)


def test_moe_sort_workspace_bytes():
    for n in (0, 1, R.CHUNK - 1, R.CHUNK, R.CHUNK + 1, 5 * R.CHUNK + 3,
              2 ** 31 - 1 - 127 * 8):
        for e in (1, 8, 1024):
            if n + 127 * e > 2 ** 31 - 1:
                continue
            want = -(-n // R.CHUNK) * (e + 1) * 4
            assert sp.moe_sort_workspace_bytes(n, e) == want, (n, e)
    f = sp.lib().sputnik_moe_sort_workspace_bytes
    assert f(-1, 8) == 0 and f(8, 0) == 0 and f(8, 1025) == 0
    assert f(2 ** 31 - 1, 1) == 0
    for bad in ((-1, 8), (8, 0), (8, 1025), (2 ** 31 - 1, 1)):
        with pytest.raises(ValueError):
            sp.moe_sort_workspace_bytes(*bad)


# ---- errors raised before the library is called -----------------------------

@pytest.fixture
def no_library(monkeypatch):
    """Any use of the library fails the test."""
    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(sp, "lib", boom)


def _i32(*shape):
    return torch.zeros(*shape, dtype=torch.int32)


def _mat(rows, cols, dtype=torch.bfloat16):
    return torch.zeros(rows, cols, dtype=dtype)


def test_binding_errors_raise_before_the_library(no_library):
    ok = dict(logits=_mat(4, 8), top_experts=_i32(4, 2), weights=_mat(4, 2))

    def topk(**kw):
        sp.RouterTopK(**{**ok, **kw})

    for bad in (dict(logits=_mat(4, 8, torch.float64)),
                dict(top_experts=_i32(4, 2).long()),
                dict(weights=_mat(4, 2, torch.float16)),
                dict(scores=_mat(4, 8, torch.float32)),   # weights are bf16
                dict(weights=_mat(4, 2, torch.float32), scores=_mat(4, 8))):
        with pytest.raises(TypeError):
            topk(**bad)
    for bad in (dict(logits=torch.zeros(8, dtype=torch.bfloat16)),   # 1-D
                dict(logits=_mat(4, 16)[:, ::2]),          # not contiguous
                dict(logits=_mat(4, 1025), top_experts=_i32(4, 2)),
                dict(logits=_mat(4, 0)),
                dict(top_experts=_i32(5, 2)),
                dict(top_experts=_i32(8)),
                dict(top_experts=_i32(4, 9), weights=_mat(4, 9)),    # k > E
                dict(logits=_mat(4, 64), top_experts=_i32(4, 33),
                     weights=_mat(4, 33)),                           # k > 32
                dict(top_experts=_i32(4, 0), weights=_mat(4, 0)),
                dict(weights=_mat(4, 3)),
                dict(scores=_mat(4, 7))):
        with pytest.raises(ValueError):
            topk(**bad)

    g = dict(logits=_mat(4, 8), top_experts=_i32(4, 2), dweights=_mat(4, 2),
             dlogits=_mat(4, 8))

    def grad(**kw):
        sp.RouterTopKGrad(**{**g, **kw})

    for bad in (dict(dlogits=_mat(4, 8, torch.float32)),   # the logits' type
                dict(dweights=_mat(4, 2, torch.float16)),
                dict(dscores=_mat(4, 8, torch.float32)),
                dict(logits=_mat(4, 8).int())):
        with pytest.raises(TypeError):
            grad(**bad)
    for bad in (dict(dlogits=_mat(4, 7)), dict(dweights=_mat(4, 3)),
                dict(dscores=_mat(3, 8)), dict(top_experts=_i32(4, 9))):
        with pytest.raises(ValueError):
            grad(**bad)

    s = dict(top_experts=_i32(8), num_experts=2, rows=384, indices=_i32(8),
             bin_ids=_i32(8), bins=_i32(2), tokens_per_expert=_i32(2),
             padded_bins=_i32(2), row_of=_i32(8),
             workspace=torch.zeros(12, dtype=torch.uint8))

    def sort(**kw):
        sp.MoeSort(**{**s, **kw})

    for bad in (dict(top_experts=_i32(8).long()), dict(bins=_i32(2).long()),
                dict(row_of=_i32(8).float())):
        with pytest.raises(TypeError):
            sort(**bad)
    for bad in (dict(indices=_i32(7)), dict(bin_ids=_i32(9)),
                dict(row_of=_i32(7)), dict(bins=_i32(3)),
                dict(padded_bins=_i32(1)), dict(num_experts=0),
                dict(num_experts=1025), dict(rows=100), dict(rows=-128),
                dict(workspace=torch.zeros(11, dtype=torch.uint8)),
                dict(workspace=None),
                dict(workspace=torch.zeros(4, 8, dtype=torch.uint8)[:, ::2])):
        with pytest.raises(ValueError):
            sort(**bad)


def test_ops_errors_raise_before_the_library(no_library):
    from sputnik_amd import ops
    logits = _mat(4, 8)
    with pytest.raises(TypeError):
        ops.moe_router(logits.double(), 2)
    with pytest.raises(TypeError):
        ops.moe_router(logits, 2, weights_dtype=torch.float16)
    for bad in (0, 9, True, 2.0):
        with pytest.raises(ValueError):
            ops.moe_router(logits, bad)
    with pytest.raises(ValueError):
        ops.moe_router(_mat(4, 64), 33)
    with pytest.raises(ValueError):
        ops.moe_router(_mat(4, 1025), 2)
    with pytest.raises(ValueError):
        ops.moe_router(torch.zeros(8, dtype=torch.bfloat16), 2)

    top = torch.zeros(4, 2, dtype=torch.int64)
    with pytest.raises(ValueError):
        ops.moe_device_route(top, 1025)
    with pytest.raises(ValueError):
        ops.moe_device_route(top, 2, rows=128)
    with pytest.raises(ValueError):
        ops.moe_device_route(top, 0)
    with pytest.raises(TypeError):
        ops.moe_device_route(top.float(), 2)
    # moe_mlp with a route built beforehand
    route = ops.MoeRoute(_i32(8), _i32(8), _i32(2), _i32(2), _i32(2), _i32(8),
                         top_k=2, tokens=4, rows=384)
    xm, ew = _mat(4, 256), torch.zeros(4, 2)
    m1, m2 = _mat(256, 512), _mat(512, 256)
    with pytest.raises(ValueError):
        ops.moe_mlp(xm, route, ew, _mat(256, 768), _mat(768, 256), 3)
    with pytest.raises(ValueError):
        ops.moe_mlp(xm, route, ew, m1, m2, 2, rows=512)
    with pytest.raises(ValueError):
        ops.moe_mlp(_mat(5, 256), route, ew, m1, m2, 2)
    with pytest.raises(ValueError):
        ops.moe_mlp(xm, route, torch.zeros(4, 3), m1, m2, 2)

    x, wr = _mat(4, 256), _mat(2, 256)
    w1, w2 = _mat(256, 512), _mat(512, 256)
    with pytest.raises(TypeError):
        ops.moe_layer(x.float(), wr, w1, w2, 2)
    with pytest.raises(TypeError):
        ops.moe_layer(x, wr.half(), w1, w2, 2)
    with pytest.raises(TypeError):
        ops.moe_layer(x, wr, w1, w2, 2, router_dtype=torch.float16)
    with pytest.raises(ValueError):
        ops.moe_layer(x, _mat(2, 128), w1, w2, 2)
    with pytest.raises(ValueError):
        ops.moe_layer(x, wr, w1, w2, 3)                  # top_k > E
    with pytest.raises(ValueError):
        ops.moe_layer(x, wr, w1, w2, 0)


# ---- the C entry points reject, never abort (no device is touched) ----------

A, B, C, D, E_, F, G, H_, I_ = (ctypes.c_void_p(0x1000 * i)
                                for i in range(1, 10))
NULL = None


def test_router_topk_rejections():
    f = sp.lib().sputnik_router_topk
    bad = sp.hipErrorInvalidValue

    def call(logits=A, top=B, w=C, scores=NULL, tokens=4, e=8, k=2, norm=0,
             ldtype=1, wdtype=0):
        return f(logits, top, w, scores, tokens, e, k, norm, ldtype, wdtype,
                 NULL)

    for kw in (dict(tokens=-1), dict(e=0), dict(e=-3), dict(e=1025),
               dict(k=0), dict(k=-1), dict(k=9), dict(e=64, k=33),
               dict(ldtype=3), dict(ldtype=-1), dict(wdtype=2),
               dict(wdtype=-1),
               dict(logits=NULL), dict(top=NULL), dict(w=NULL),
               dict(top=A), dict(w=A), dict(scores=A), dict(w=B),
               dict(scores=B), dict(scores=C)):
        assert call(**kw) == bad, kw
    assert call(tokens=0, logits=NULL, top=NULL, w=NULL) == 0


def test_router_topk_grad_rejections():
    f = sp.lib().sputnik_router_topk_grad
    bad = sp.hipErrorInvalidValue

    def call(logits=A, top=B, dw=C, ds=NULL, dl=E_, tokens=4, e=8, k=2,
             norm=1, ldtype=0, wdtype=1):
        return f(logits, top, dw, ds, dl, tokens, e, k, norm, ldtype, wdtype,
                 NULL)

    for kw in (dict(tokens=-1), dict(e=0), dict(e=1025), dict(k=0),
               dict(k=9), dict(e=64, k=33), dict(ldtype=3), dict(wdtype=2),
               dict(logits=NULL), dict(top=NULL), dict(dw=NULL),
               dict(dl=NULL), dict(dl=A), dict(dl=B), dict(dl=C),
               dict(ds=D, dl=D)):
        assert call(**kw) == bad, kw
    assert call(tokens=0, logits=NULL, top=NULL, dw=NULL, dl=NULL) == 0


def test_moe_sort_rejections():
    f = sp.lib().sputnik_moe_sort
    bad = sp.hipErrorInvalidValue
    names = ("top", "indices", "bin_ids", "bins", "tpe", "padded", "row_of",
             "ws")

    def call(top=A, n=8, e=4, rows=640, indices=B, bin_ids=C, bins=D, tpe=E_,
             padded=F, row_of=G, ws=H_, ws_bytes=20):
        return f(top, n, e, rows, indices, bin_ids, bins, tpe, padded, row_of,
                 ws, ws_bytes, NULL)

    for kw in (dict(n=-1), dict(e=0), dict(e=-1), dict(e=1025),
               dict(rows=-128), dict(rows=100),
               dict(n=2 ** 31 - 1, e=1, ws_bytes=2 ** 40),     # n + 127 E
               dict(ws_bytes=19), dict(ws_bytes=0),
               dict(n=R.CHUNK + 1, ws_bytes=39),
               dict(ws=ctypes.c_void_p(0x8002))):              # alignment
        assert call(**kw) == bad, kw
    for name in names:
        assert call(**{name: NULL}) == bad, name
    for i, a in enumerate(names):               # any two buffers the same
        for b in names[i + 1:]:
            assert call(**{a: I_, b: I_}) == bad, (a, b)
