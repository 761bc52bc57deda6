"""CPU: the host side of the sigmoid-score router (RouterScoreTopK /
RouterScoreTopKGrad, sputnik/block/router.h). The inputs of
tests/router_score_ref.py meet the gap condition that makes the float64 picks
the only right answer; the float32 emulation picks those ids and meets the
bounds the GPU tests hold the kernels to, on the very inputs those tests use;
the Python entry points exist and reject every limit before the library is
called; the C entry points reject what the header lists without a device;
router_bias_update on CPU tensors. No compute call is made."""

import ctypes
import inspect
import subprocess

import numpy as np
import pytest

import sputnik_amd as sp
from tests import router_score_ref as R
from tests.test_cpp_router_score import SYMBOLS

torch = pytest.importorskip("torch")


def _wtypes(ltype):
    return [ltype] if ltype == "f32" else [ltype, "f32"]


SCALES = {False: 1.0, True: 2.5}     # normalize -> the scale used with it


# ---- the inputs and the references check themselves -------------------------

@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_inputs_meet_the_gap_condition(case):
    tokens, e, k, g, gk = case
    for ltype in R.LTYPES:
        for kind in R.KINDS:
            l, b = R.logits(case, kind, ltype), R.bias(case, kind)
            assert l.shape == (tokens, e) and b.shape == (e,)
            assert b.dtype == np.float32 and np.isfinite(b).all()
            if ltype != "f32":      # representable in the type
                with np.errstate(invalid="ignore"):
                    assert np.array_equal(R.rnd(l, ltype), l, equal_nan=True)
            assert R.gaps_ok(l, b, case).all(), (ltype, kind)
            print(ltype, kind, "most redraws of a row:",
                  R.redraws(case, kind, ltype))
    assert not np.isfinite(R.logits(case, "special", "f32")).all()


@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_reference_picks(case):
    tokens, e, k, g, gk = case
    gs = e // g
    for ltype in R.LTYPES:
        for kind in R.KINDS:
            l, b = R.logits(case, kind, ltype), R.bias(case, kind)
            ids = R.picks64(l, b, case)
            assert ids.shape == (tokens, k) and ids.dtype == np.int32
            assert ((ids >= 0) & (ids < e)).all()
            assert all(len(set(row)) == k for row in ids.tolist())
            # at most topk_groups groups are used
            assert all(len(set(row)) <= gk for row in (ids // gs).tolist())
            # the float32 emulation picks the same
            assert np.array_equal(R.picks32(l, b, case), ids), (ltype, kind)
            if kind == "equal":     # the first eligible indices
                assert (ids == np.arange(k)).all()
            # descending in c, NaN last, ties in ascending index
            c = np.take_along_axis(R.c64(l, b), ids.astype(np.int64), axis=1)
            for row_v, row_i in zip(c.tolist(), ids.tolist()):
                for x, y, ix, iy in zip(row_v, row_v[1:], row_i, row_i[1:]):
                    if np.isnan(x):
                        assert np.isnan(y) and ix < iy
                    elif not np.isnan(y):
                        assert x > y or (x == y and ix < iy)


def test_reference_against_a_plain_loop():
    """select against the definition written out for one row at a time."""
    case = (129, 65, 8, 5, 3)
    tokens, e, k, g, gk = case
    gs = e // g
    for kind in ("random", "special"):
        l, b = R.logits(case, kind, "bf16"), R.bias(case, kind)
        c = R.c64(l, b)
        ids = R.picks64(l, b, case)

        def first(x, y):        # x = (value, index) before y in the order
            if np.isnan(x[0]) or np.isnan(y[0]):
                return (not np.isnan(x[0]) if np.isnan(x[0]) != np.isnan(y[0])
                        else x[1] < y[1])
            return x[0] > y[0] or (x[0] == y[0] and x[1] < y[1])

        def ordered(items):     # insertion sort by `first`
            out = []
            for it in items:
                at = len(out)
                while at > 0 and first(it, out[at - 1]):
                    at -= 1
                out.insert(at, it)
            return out

        for t in range(tokens):
            scores = []
            for grp in range(g):
                top = ordered([(c[t, i], i)
                               for i in range(grp * gs, (grp + 1) * gs)])
                scores.append((top[0][0] + top[1][0], grp))
            on = {grp for _, grp in ordered(scores)[:gk]}
            want = [i for _, i in ordered(
                [(c[t, i], i) for i in range(e) if i // gs in on])[:k]]
            assert ids[t].tolist() == want, (kind, t)


def test_ties_reach_both_boundaries():
    """In the "ties" inputs the k-th and (k+1)-th pick are equal and so are
    the group scores either side of the topk_groups boundary, in every row:
    the index rule alone decides."""
    for case in R.CASES:
        b = R.bias(case, "ties")
        assert (b == b[0]).all()
        for ltype in R.LTYPES:
            assert R.ties_reach(R.logits(case, "ties", ltype), b, case).all()


# ---- the emulation meets the GPU tests' bounds ------------------------------

@pytest.mark.parametrize("ltype", R.LTYPES)
@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_emulation_meets_the_forward_bounds(case, ltype):
    tokens, e, k, g, gk = case
    worst = 0.0
    for kind in R.VALUE_KINDS:
        l, b = R.logits(case, kind, ltype), R.bias(case, kind)
        ids = R.picks64(l, b, case)
        for normalize, scale in SCALES.items():
            w_ref, s_ref = R.forward64(l, ids, normalize, scale)
            for wtype in _wtypes(ltype):
                w, s = R.forward32(l, ids, normalize, scale, wtype)
                wb = R.weights_bound(w_ref, k, wtype)
                sb = R.scores_bound(s_ref, wtype)
                assert (np.abs(w - w_ref) <= wb).all()
                assert (np.abs(s - s_ref) <= sb).all()
                if wtype == "f32":
                    worst = max(worst, float((np.abs(w - w_ref) / wb).max()),
                                float((np.abs(s - s_ref) / sb).max()))
    print("forward: largest share of the fp32 bound", worst)


@pytest.mark.parametrize("ltype", R.LTYPES)
@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_emulation_meets_the_gradient_bound(case, ltype):
    tokens, e, k, g, gk = case
    l = R.logits(case, "random", ltype)
    ids = R.grad_ids(case, ltype)
    for wtype in _wtypes(ltype):
        dw, ds = R.grad_inputs(case, ltype, wtype)
        for normalize, scale in SCALES.items():
            for dscores in (None, ds):
                ref, image, s = R.grad64(l, ids, dw, dscores, normalize,
                                         scale)
                got = R.grad32(l, ids, dw, dscores, normalize, scale, ltype)
                assert np.isfinite(ref).all()
                assert (np.abs(got - ref)
                        <= R.grad_bound(ref, image, s, k, ltype)).all()


def test_gradient_reference_against_autograd():
    """grad64 is the derivative of forward64 (float64 torch autograd), and
    its out-of-range and repeated picks behave as router.h says."""
    case, ltype = (67, 8, 2, 4, 2), "f32"
    l = R.logits(case, "random", ltype)
    ids = R.picks64(l, R.bias(case, "random"), case)
    dw, ds = R.grad_inputs(case, ltype, "f32")
    for normalize, scale in SCALES.items():
        lt = torch.from_numpy(np.array(l)).double().requires_grad_(True)
        s = torch.sigmoid(lt)
        w = torch.gather(s, 1, torch.from_numpy(ids.astype(np.int64)))
        if normalize:
            w = w / w.sum(dim=1, keepdim=True)
        w = w * scale
        ((w * torch.from_numpy(np.array(dw)).double()).sum()
         + (s * torch.from_numpy(np.array(ds)).double()).sum()).backward()
        ref, _, _ = R.grad64(l, ids, dw, ds, normalize, scale)
        assert np.allclose(ref, lt.grad.numpy(), rtol=1e-10, atol=1e-14)
    one = ids[:, :1]
    base, _, _ = R.grad64(l, one, dw[:, :1], None, False, 1.0)
    with_bad = np.concatenate([one, np.full_like(one, 8)], axis=1)
    got, _, _ = R.grad64(l, with_bad, dw, None, False, 1.0)
    assert np.array_equal(got, base)
    twice, _, _ = R.grad64(l, np.concatenate([one, one], axis=1),
                           np.concatenate([dw[:, :1], dw[:, :1]], axis=1),
                           None, False, 1.0)
    assert np.allclose(twice, 2 * base, rtol=1e-12, atol=0)


# ---- entry points -----------------------------------------------------------

def test_python_entry_points_exist():
    from sputnik_amd import ops
    sig = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert sig(sp.RouterScoreTopK) == [
        "logits", "top_experts", "weights", "bias", "num_groups",
        "topk_groups", "normalize", "scale", "scores", "stream"]
    assert sig(sp.RouterScoreTopKGrad) == [
        "logits", "top_experts", "dweights", "dlogits", "normalize", "scale",
        "dscores", "stream"]
    for name in ("RouterScoreTopK", "RouterScoreTopKGrad",
                 "ROUTER_MAX_GROUPS"):
        assert name in sp.__all__, name
    assert sp.ROUTER_MAX_GROUPS == 64
    assert sig(ops.moe_score_router) == [
        "logits", "top_k", "bias", "num_groups", "topk_groups", "normalize",
        "scale", "weights_dtype", "return_scores"]
    assert sig(ops.moe_score_layer) == sig(ops.moe_layer) + [
        "router_bias", "num_groups", "topk_groups", "routed_scale"]
    assert sig(ops.router_bias_update) == ["bias", "tokens_per_expert",
                                           "rate"]
    for name in ("moe_score_router", "moe_score_layer",
                 "router_bias_update"):
        assert name in ops.__all__, name


def test_header_documents_the_score_router():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "sputnik", "block",
                             "router.h")).read()
    assert "constexpr int kRouterMaxGroups = 64;" in text
    for word in ("RouterScoreTopK", "RouterScoreTopKGrad", "are\n"
                 "//                   a tie"):
        assert word in text, word


C_ENTRIES = ("sputnik_router_score_topk", "sputnik_router_score_topk_grad")


def test_c_and_cpp_symbols_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", sp.LIB_PATH],
                         capture_output=True, text=True,
                         check=True).stdout.split()
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


def _i32(*shape):
    return torch.zeros(*shape, dtype=torch.int32)


def _mat(rows, cols, dtype=torch.bfloat16):
    return torch.zeros(rows, cols, dtype=dtype)


def test_binding_errors_raise_before_the_library(no_library):
    ok = dict(logits=_mat(4, 8), top_experts=_i32(4, 2), weights=_mat(4, 2),
              bias=torch.zeros(8), num_groups=4, topk_groups=2)

    def topk(**kw):
        sp.RouterScoreTopK(**{**ok, **kw})

    for bad in (dict(logits=_mat(4, 8, torch.float64)),
                dict(top_experts=_i32(4, 2).long()),
                dict(weights=_mat(4, 2, torch.float16)),
                dict(scores=_mat(4, 8, torch.float32)),   # weights are bf16
                dict(bias=torch.zeros(8, dtype=torch.bfloat16))):
        with pytest.raises(TypeError):
            topk(**bad)
    for bad in (dict(num_groups=3),                       # E % G != 0
                dict(top_experts=_i32(4, 5), weights=_mat(4, 5)),
                #                                 (top_k > topk_groups * gs)
                dict(top_experts=_i32(4, 3), weights=_mat(4, 3),
                     topk_groups=1),
                dict(logits=_mat(4, 128), bias=None, num_groups=128,
                     topk_groups=2),                      # G > 64
                dict(num_groups=2, topk_groups=4),        # Gk > G
                dict(topk_groups=0), dict(num_groups=0, topk_groups=0),
                dict(num_groups=4.0), dict(topk_groups=True),
                dict(scale=float("inf")), dict(scale=float("nan")),
                dict(scale=1e39),                         # inf in fp32
                dict(scale="1"),
                dict(bias=torch.zeros(7)), dict(bias=torch.zeros(1, 8)),
                dict(logits=_mat(4, 64), top_experts=_i32(4, 33),
                     weights=_mat(4, 33), bias=None, num_groups=1,
                     topk_groups=1),                      # k > 32
                dict(top_experts=_i32(4, 0), weights=_mat(4, 0)),
                dict(scores=_mat(4, 7))):
        with pytest.raises(ValueError):
            topk(**bad)
    # outputs that share an address with an input or with each other
    f32 = dict(logits=_mat(4, 2, torch.float32), bias=None, num_groups=1,
               topk_groups=1)
    buf = _mat(4, 2, torch.float32)
    for bad in (dict(weights=f32["logits"]),
                dict(weights=buf, scores=buf),
                dict(top_experts=buf.view(torch.int32), weights=buf)):
        with pytest.raises(ValueError, match="aliases"):
            topk(**{**f32, **bad})

    g = dict(logits=_mat(4, 8), top_experts=_i32(4, 2), dweights=_mat(4, 2),
             dlogits=_mat(4, 8))

    def grad(**kw):
        sp.RouterScoreTopKGrad(**{**g, **kw})

    for bad in (dict(dlogits=_mat(4, 8, torch.float32)),   # the logits' type
                dict(dweights=_mat(4, 2, torch.float16)),
                dict(dscores=_mat(4, 8, torch.float32)),
                dict(logits=_mat(4, 8).int())):
        with pytest.raises(TypeError):
            grad(**bad)
    for bad in (dict(dlogits=_mat(4, 7)), dict(dweights=_mat(4, 3)),
                dict(dscores=_mat(3, 8)), dict(top_experts=_i32(4, 9)),
                dict(scale=float("inf")), dict(scale=None),
                dict(dlogits=g["logits"])):
        with pytest.raises(ValueError):
            grad(**bad)
    both = _mat(4, 8)
    with pytest.raises(ValueError, match="aliases"):
        grad(dscores=both, dlogits=both)


def test_ops_errors_raise_before_the_library(no_library):
    from sputnik_amd import ops
    logits = _mat(4, 8)
    with pytest.raises(TypeError):
        ops.moe_score_router(logits.double(), 2)
    with pytest.raises(TypeError):
        ops.moe_score_router(logits, 2, weights_dtype=torch.float16)
    with pytest.raises(TypeError):
        ops.moe_score_router(logits, 2, bias=torch.zeros(8).double())
    for bad in (0, 9, True, 2.0):
        with pytest.raises(ValueError):
            ops.moe_score_router(logits, bad)
    for kw in (dict(num_groups=3), dict(num_groups=4, topk_groups=1),
               dict(num_groups=2, topk_groups=3), dict(topk_groups=0),
               dict(scale=float("nan")), dict(bias=torch.zeros(4)),
               dict(num_groups=True)):
        with pytest.raises(ValueError):
            ops.moe_score_router(logits, 3, **kw)
    with pytest.raises(ValueError):
        ops.moe_score_router(_mat(4, 128), 2, num_groups=128, topk_groups=2)

    x, wr = _mat(4, 256), _mat(8, 256)
    w1, w2 = _mat(256, 512), _mat(512, 256)
    with pytest.raises(TypeError):
        ops.moe_score_layer(x.float(), wr, w1, w2, 2)
    with pytest.raises(ValueError):
        ops.moe_score_layer(x, wr, w1, w2, 9)
    # (a CPU matmul makes the logits; the router's checks come next)
    with pytest.raises(ValueError):
        ops.moe_score_layer(x, wr, w1, w2, 3, num_groups=4, topk_groups=1)
    with pytest.raises(ValueError):
        ops.moe_score_layer(x, wr, w1, w2, 2, routed_scale=float("inf"))
    with pytest.raises(ValueError):
        ops.moe_score_layer(x, wr, w1, w2, 2, router_bias=torch.zeros(7))


def test_moe_layer_keeps_its_arguments():
    """The softmax layer is untouched: moe_score_layer is a new entry
    point."""
    from sputnik_amd import ops
    assert list(inspect.signature(ops.moe_layer).parameters)[-1] == \
        "return_scores"


# ---- router_bias_update -----------------------------------------------------

def test_router_bias_update_on_cpu_tensors():
    from sputnik_amd import ops
    bias = torch.tensor([0.5, 0.0, -0.25, 1.0])
    load = torch.tensor([9, 1, 3, 3], dtype=torch.int32)     # mean 4
    out = ops.router_bias_update(bias, load, 0.125)
    assert out is bias
    assert bias.tolist() == [0.375, 0.125, -0.125, 1.125]
    # a load at the mean stays; float loads are taken too
    ops.router_bias_update(bias, torch.tensor([4.0, 2.0, 6.0, 4.0]), 0.25)
    assert bias.tolist() == [0.375, 0.375, -0.375, 1.125]
    # no gradient is recorded
    b = torch.zeros(4, requires_grad=False)
    ops.router_bias_update(b, load, 1.0)
    assert not b.requires_grad
    with pytest.raises(TypeError):
        ops.router_bias_update(bias.double(), load, 0.1)
    with pytest.raises(TypeError):
        ops.router_bias_update(bias, [1, 2, 3, 4], 0.1)
    with pytest.raises(ValueError):
        ops.router_bias_update(bias, load[:3], 0.1)
    with pytest.raises(ValueError):
        ops.router_bias_update(bias.reshape(2, 2), load.reshape(2, 2), 0.1)


# ---- the C entry points reject, never abort (no device is touched) ----------

A, B, C, D, E_, F = (ctypes.c_void_p(0x1000 * i) for i in range(1, 7))
NULL = None


def test_router_score_topk_rejections():
    f = sp.lib().sputnik_router_score_topk
    bad = sp.hipErrorInvalidValue

    def call(logits=A, bias=F, top=B, w=C, scores=NULL, tokens=4, e=8, k=2,
             g=4, gk=2, norm=0, scale=1.0, ldtype=1, wdtype=0):
        return f(logits, bias, top, w, scores, tokens, e, k, g, gk, norm,
                 scale, ldtype, wdtype, NULL)

    for kw in (dict(tokens=-1), dict(e=0), dict(e=-3), dict(e=1025),
               dict(k=0), dict(k=-1), dict(k=5), dict(e=64, g=1, gk=1, k=33),
               dict(g=3), dict(g=0, gk=0), dict(gk=0), dict(gk=5),
               dict(g=-4, gk=-4), dict(e=128, g=128, gk=2),
               dict(gk=1, k=3), dict(scale=float("inf")),
               dict(scale=float("-inf")), dict(scale=float("nan")),
               dict(ldtype=3), dict(ldtype=-1), dict(wdtype=2),
               dict(wdtype=-1),
               dict(logits=NULL), dict(top=NULL), dict(w=NULL),
               dict(top=A), dict(w=A), dict(scores=A), dict(w=B),
               dict(scores=B), dict(scores=C), dict(w=F), dict(scores=F),
               dict(top=F)):
        assert call(**kw) == bad, kw
    assert call(tokens=0, logits=NULL, top=NULL, w=NULL, bias=NULL) == 0
    # (a limit broken is reported even when there are no tokens)
    assert call(tokens=0, g=3) == bad


def test_router_score_topk_grad_rejections():
    f = sp.lib().sputnik_router_score_topk_grad
    bad = sp.hipErrorInvalidValue

    def call(logits=A, top=B, dw=C, ds=NULL, dl=E_, tokens=4, e=8, k=2,
             norm=1, scale=2.5, ldtype=0, wdtype=1):
        return f(logits, top, dw, ds, dl, tokens, e, k, norm, scale, ldtype,
                 wdtype, NULL)

    for kw in (dict(tokens=-1), dict(e=0), dict(e=1025), dict(k=0),
               dict(k=9), dict(e=64, k=33), dict(ldtype=3), dict(wdtype=2),
               dict(scale=float("inf")), dict(scale=float("nan")),
               dict(logits=NULL), dict(top=NULL), dict(dw=NULL),
               dict(dl=NULL), dict(dl=A), dict(dl=B), dict(dl=C),
               dict(ds=D, dl=D)):
        assert call(**kw) == bad, kw
    assert call(tokens=0, logits=NULL, top=NULL, dw=NULL, dl=NULL) == 0
