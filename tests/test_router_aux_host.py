"""CPU: the host side of the router's auxiliary-loss statistics
(RouterTopKAux / RouterTopKAuxGrad, sputnik/block/router.h). The float32
emulation of tests/router_aux_ref.py, in the kernels' order of summation,
meets the bounds the GPU tests hold the kernels to, on the very inputs those
tests use; the gradient reference is the derivative torch autograd gives in
float64; the Python entry points and constants exist, type, shape and device
errors are raised before the library is called, the C and C++ symbols are
exported, and the C entry points reject what the header lists, without a
device and without aborting. No compute call is made."""

import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import sputnik_amd as sp
from tests import router_aux_ref as A
from tests import router_ref as R
from tests.test_cpp_router_aux import SYMBOLS

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _wtypes(ltype):
    return [ltype] if ltype == "f32" else [ltype, "f32"]


# ---- the emulation meets the GPU tests' bounds ------------------------------

def test_the_cases_cover_what_they_claim():
    assert A.T == sp.ROUTER_AUX_TOKENS and A.T % A.WAVES == 0
    tokens = {c[0] for c in A.AUX_CASES}
    assert {1, A.T - 1, A.T, A.T + 1, 3 * A.T + 5} <= tokens
    widths = {max(1, 1 << ((c[1] + 63) // 64 - 1).bit_length())
              for c in A.AUX_CASES}
    assert widths == {1, 2, 4, 8, 16}


@pytest.mark.parametrize("ltype", R.LTYPES)
@pytest.mark.parametrize("case", A.AUX_CASES, ids=A.IDS)
def test_emulation_meets_the_forward_bounds(case, ltype):
    tokens, e, k = case
    for kind in A.kinds(case):
        l = A.logits(case, kind, ltype)
        sums_ref, z_ref, m, lse = A.stats64(l)
        sums, z = A.stats32(l)
        assert sums.dtype == np.float32 and sums.shape == (e,)
        sb = A.score_sums_bound(sums_ref, tokens, e)
        zb = A.z_sum_bound(z_ref, m, lse, e)
        s_err = np.abs(sums.astype(np.float64) - sums_ref)
        z_err = abs(float(z) - z_ref)
        print(kind, "score_sums: share of the bound",
              float((s_err / sb).max()), "z_sum:", z_err / max(zb, 1e-300))
        assert (s_err <= sb).all(), kind
        assert z_err <= zb, kind
        assert abs(sums_ref.sum() - tokens) < 1e-9 * tokens


@pytest.mark.parametrize("ltype", R.LTYPES)
@pytest.mark.parametrize("case", A.AUX_CASES, ids=A.IDS)
def test_emulation_meets_the_gradient_bound(case, ltype):
    tokens, e, k = case
    l = A.logits(case, "random", ltype)
    ids = R.grad_ids(case, ltype)
    dss, dz = A.aux_grads(case, ltype)
    assert (np.abs(dss) >= 2.0 ** -10).all() and (np.abs(dss) <= 4).all()
    assert 2.0 ** -10 <= abs(float(dz[0])) <= 4
    for wtype in _wtypes(ltype):
        dw, ds = R.grad_inputs(case, ltype, wtype)
        for normalize in (False, True):
            for dscores in (None, ds):
                for s, z in ((None, None), (dss, None), (None, dz),
                             (dss, dz)):
                    ref, image = A.grad64(l, ids, dw, dscores, s, z,
                                          normalize)
                    got = A.grad32(l, ids, dw, dscores, s, z, normalize,
                                   ltype)
                    assert np.isfinite(ref).all()
                    assert (np.abs(got - ref)
                            <= A.grad_bound(ref, image, e, k, ltype)).all()
                    if s is None and z is None:     # router_ref's, exactly
                        assert np.array_equal(
                            got, R.grad32(l, ids, dw, dscores, normalize,
                                          ltype))


def test_gradient_reference_against_autograd():
    """grad64 is the derivative of sum(w dw) + sum(p ds) + sum_e dss_e
    score_sums_e + dz z_sum (float64 torch autograd on softmax /
    logsumexp)."""
    case, ltype = (3 * A.T + 5, 8, 2), "f32"
    l = A.logits(case, "random", ltype)
    ids = R.expected_ids(l, case[2])
    dw, ds = R.grad_inputs(case, ltype, "f32")
    dss, dz = A.aux_grads(case, ltype)
    td = lambda a: torch.from_numpy(np.array(a)).double()  # noqa: E731
    for normalize in (False, True):
        for s, z in ((dss, None), (None, dz), (dss, dz)):
            lt = td(l).requires_grad_(True)
            p = torch.softmax(lt, dim=1)
            w = torch.gather(p, 1, torch.from_numpy(ids.astype(np.int64)))
            if normalize:
                w = w / w.sum(dim=1, keepdim=True)
            loss = (w * td(dw)).sum() + (p * td(ds)).sum()
            if s is not None:
                loss = loss + (p.sum(0) * td(s)).sum()
            if z is not None:
                loss = loss + td(z)[0] * (torch.logsumexp(lt, 1) ** 2).sum()
            loss.backward()
            ref, _ = A.grad64(l, ids, dw, ds, s, z, normalize)
            assert np.allclose(ref, lt.grad.numpy(), rtol=1e-10, atol=1e-13)
    sums, z_sum, _, _ = A.stats64(l)
    lt = td(l)
    assert np.allclose(sums, torch.softmax(lt, 1).sum(0).numpy(), rtol=1e-12)
    assert np.isclose(z_sum, float((torch.logsumexp(lt, 1) ** 2).sum()),
                      rtol=1e-12)


# ---- entry points -----------------------------------------------------------

def test_python_entry_points_exist():
    from sputnik_amd import ops
    sig = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert sig(sp.RouterTopKAux) == ["logits", "top_experts", "weights",
                                     "score_sums", "workspace", "normalize",
                                     "scores", "z_sum", "stream"]
    assert sig(sp.RouterTopKAuxGrad) == ["logits", "top_experts", "dweights",
                                         "dlogits", "normalize", "dscores",
                                         "dscore_sums", "dz_sum", "stream"]
    assert sig(sp.router_aux_workspace_bytes) == ["tokens", "num_experts"]
    for name in ("RouterTopKAux", "RouterTopKAuxGrad",
                 "router_aux_workspace_bytes", "ROUTER_AUX_TOKENS"):
        assert name in sp.__all__, name
    assert sig(ops.moe_router_aux) == ["logits", "top_k", "normalize",
                                       "weights_dtype"]
    assert sig(ops.load_balancing_loss) == ["score_sums", "tokens_per_expert",
                                            "tokens", "top_k", "weight"]
    assert sig(ops.router_z_loss) == ["z_sum", "tokens", "weight"]
    # moe_layer_aux takes moe_layer's arguments, but for return_scores
    assert sig(ops.moe_layer_aux) == sig(ops.moe_layer)[:-1]
    assert sig(ops.moe_layer)[-1] == "return_scores"
    for name, p in inspect.signature(ops.moe_layer_aux).parameters.items():
        assert p.default == inspect.signature(ops.moe_layer).parameters[
            name].default, name
    assert [f for f in ops.MoeAux.__dataclass_fields__] == [
        "score_sums", "z_sum", "tokens_per_expert", "tokens", "top_k"]
    for name in ("moe_router_aux", "load_balancing_loss", "router_z_loss",
                 "moe_layer_aux", "MoeAux"):
        assert name in ops.__all__, name


def test_header_names_the_constant():
    text = open(os.path.join(ROOT, "include", "sputnik", "block",
                             "router.h")).read()
    assert ("constexpr int kRouterAuxTokens = %d;" % sp.ROUTER_AUX_TOKENS
            in text)
    assert sp.ROUTER_AUX_TOKENS == A.T == 64
    for name in ("RouterAuxWorkspaceBytes", "RouterTopKAux(",
                 "RouterTopKAuxGrad("):
        assert name in text, name


C_ENTRIES = ("sputnik_router_topk_aux", "sputnik_router_topk_aux_grad",
             "sputnik_router_aux_workspace_bytes")


def test_c_and_cpp_symbols_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", sp.LIB_PATH],
                         capture_output=True, text=True,
                         check=True).stdout.split()
    for s in C_ENTRIES + SYMBOLS:
        assert s in out, s
    for s in C_ENTRIES:
        assert hasattr(sp.lib(), s)
    header = open(os.path.join(ROOT, "include", "sputnik_amd.h")).read()
    for s in C_ENTRIES:
        assert s + "(" in header, s


def test_router_aux_workspace_bytes():
    for tokens in (0, 1, A.T - 1, A.T, A.T + 1, 5 * A.T + 3, 2 ** 31 - 1):
        for e in (1, 8, 1024):
            want = -(-tokens // A.T) * (e + 1) * 4
            assert sp.router_aux_workspace_bytes(tokens, e) == want
    f = sp.lib().sputnik_router_aux_workspace_bytes
    assert f(-1, 8) == 0 and f(8, 0) == 0 and f(8, 1025) == 0
    for bad in ((-1, 8), (8, 0), (8, 1025)):
        with pytest.raises(ValueError):
            sp.router_aux_workspace_bytes(*bad)


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


def _f32(n):
    return torch.zeros(n, dtype=torch.float32)


def _bytes(n):
    return torch.zeros(n, dtype=torch.uint8)


def test_binding_errors_raise_before_the_library(no_library):
    ok = dict(logits=_mat(4, 8), top_experts=_i32(4, 2), weights=_mat(4, 2),
              score_sums=_f32(8), workspace=_bytes(36))

    def aux(**kw):
        sp.RouterTopKAux(**{**ok, **kw})

    for bad in (dict(logits=_mat(4, 8, torch.float64)),
                dict(top_experts=_i32(4, 2).long()),
                dict(weights=_mat(4, 2, torch.float16)),
                dict(scores=_mat(4, 8, torch.float32)),   # weights are bf16
                dict(score_sums=_f32(8).bfloat16()),
                dict(score_sums=_f32(8).double()),
                dict(z_sum=_f32(1).bfloat16()),
                dict(z_sum=_i32(1))):
        with pytest.raises(TypeError):
            aux(**bad)
    for bad in (dict(logits=_mat(4, 16)[:, ::2]),          # not contiguous
                dict(logits=_mat(4, 1025)),
                dict(top_experts=_i32(4, 9), weights=_mat(4, 9)),    # k > E
                dict(weights=_mat(4, 3)),
                dict(scores=_mat(4, 7)),
                dict(score_sums=_f32(7)),
                dict(score_sums=_f32(9)),
                dict(score_sums=torch.zeros(1, 8)),                  # 2-D
                dict(score_sums=_f32(16)[::2]),
                dict(z_sum=_f32(2)),
                dict(z_sum=torch.zeros(())),
                dict(workspace=_bytes(35)),
                dict(workspace=None),
                dict(workspace=torch.zeros(4, 18, dtype=torch.uint8)[:, ::2]),
                dict(logits=_mat(65, 8), top_experts=_i32(65, 2),
                     weights=_mat(65, 2), workspace=_bytes(71)),     # 2 groups
                dict(score_sums=torch.zeros(8, device="meta")),
                dict(z_sum=torch.zeros(1, device="meta")),
                dict(workspace=torch.zeros(36, dtype=torch.uint8,
                                           device="meta"))):
        with pytest.raises(ValueError):
            aux(**bad)

    g = dict(logits=_mat(4, 8), top_experts=_i32(4, 2), dweights=_mat(4, 2),
             dlogits=_mat(4, 8))

    def grad(**kw):
        sp.RouterTopKAuxGrad(**{**g, **kw})

    for bad in (dict(dlogits=_mat(4, 8, torch.float32)),   # the logits' type
                dict(dweights=_mat(4, 2, torch.float16)),
                dict(dscores=_mat(4, 8, torch.float32)),
                dict(dscore_sums=_f32(8).bfloat16()),
                dict(dz_sum=_f32(1).double())):
        with pytest.raises(TypeError):
            grad(**bad)
    for bad in (dict(dlogits=_mat(4, 7)), dict(dweights=_mat(4, 3)),
                dict(dscores=_mat(3, 8)), dict(top_experts=_i32(4, 9)),
                dict(dscore_sums=_f32(7)), dict(dscore_sums=_f32(16)[::2]),
                dict(dz_sum=_f32(2)), dict(dz_sum=torch.zeros(())),
                dict(dscore_sums=torch.zeros(8, device="meta")),
                dict(dz_sum=torch.zeros(1, device="meta"))):
        with pytest.raises(ValueError):
            grad(**bad)


def test_ops_errors_raise_before_the_library(no_library):
    from sputnik_amd import ops
    logits = _mat(4, 8)
    with pytest.raises(TypeError):
        ops.moe_router_aux(logits.double(), 2)
    with pytest.raises(TypeError):
        ops.moe_router_aux(logits, 2, weights_dtype=torch.float16)
    for bad in (0, 9, True, 2.0):
        with pytest.raises(ValueError):
            ops.moe_router_aux(logits, bad)
    with pytest.raises(ValueError):
        ops.moe_router_aux(_mat(4, 64), 33)
    with pytest.raises(ValueError):
        ops.moe_router_aux(_mat(4, 1025), 2)
    with pytest.raises(ValueError):
        ops.moe_router_aux(torch.zeros(8, dtype=torch.bfloat16), 2)

    sums, tpe = _f32(8), _i32(8)
    with pytest.raises(TypeError):
        ops.load_balancing_loss(sums.bfloat16(), tpe, 4, 2)
    with pytest.raises(TypeError):
        ops.load_balancing_loss(sums, [1] * 8, 4, 2)
    for bad in (dict(tpe=_i32(7)), dict(sums=torch.zeros(1, 8),
                                        tpe=_i32(1, 8)),
                dict(tokens=0), dict(tokens=True), dict(tokens=4.0),
                dict(top_k=0), dict(top_k=2.0)):
        kw = dict(sums=sums, tpe=tpe, tokens=4, top_k=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.load_balancing_loss(kw["sums"], kw["tpe"], kw["tokens"],
                                    kw["top_k"])
    with pytest.raises(TypeError):
        ops.router_z_loss(_f32(1).double(), 4)
    for bad in ((_f32(2), 4), (_f32(1), 0), (_f32(1), 4.0)):
        with pytest.raises(ValueError):
            ops.router_z_loss(*bad)

    x, wr = _mat(4, 256), _mat(2, 256)
    w1, w2 = _mat(256, 512), _mat(512, 256)
    with pytest.raises(TypeError):      # the scores are what it replaces
        ops.moe_layer_aux(x, wr, w1, w2, 2, return_scores=True)
    with pytest.raises(TypeError):
        ops.moe_layer_aux(x.float(), wr, w1, w2, 2)
    with pytest.raises(TypeError):
        ops.moe_layer_aux(x, wr, w1, w2, 2, router_dtype=torch.float16)
    with pytest.raises(ValueError):
        ops.moe_layer_aux(x, _mat(2, 128), w1, w2, 2)
    with pytest.raises(ValueError):
        ops.moe_layer_aux(x, wr, w1, w2, 3)                      # top_k > E


def test_losses_on_the_host():
    """load_balancing_loss equals `weight` under perfect balance and is
    MegaBlocks' formula otherwise; tokens_per_expert carries no gradient."""
    from sputnik_amd import ops
    tokens, e, k = 96, 8, 2
    sums = torch.full((e,), tokens / e)              # p = 1 / E everywhere
    tpe = torch.full((e,), tokens * k // e, dtype=torch.int32)
    for weight in (1.0, 0.01):
        loss = ops.load_balancing_loss(sums, tpe, tokens, k, weight)
        assert loss.shape == () and loss.dtype == torch.float32
        assert abs(float(loss) - weight) <= 1e-6 * weight
    rng = np.random.default_rng(3)
    scores = torch.from_numpy(rng.random((tokens, e))).float()
    scores = scores / scores.sum(1, keepdim=True)
    counts = torch.from_numpy(rng.multinomial(tokens * k, [1 / e] * e))
    sums = scores.sum(0).requires_grad_(True)
    counts_f = counts.float().requires_grad_(True)
    loss = ops.load_balancing_loss(sums, counts_f, tokens, k, 0.5)
    want = 0.5 * e / (tokens * k) * float(
        (counts.double() * scores.double().mean(0)).sum())
    assert abs(float(loss.detach()) - want) <= 1e-6 * want
    loss.backward()
    assert counts_f.grad is None
    assert torch.allclose(sums.grad,
                          0.5 * e / (tokens ** 2 * k) * counts.float())
    z = torch.tensor([12.0], requires_grad=True)
    zl = ops.router_z_loss(z, tokens, 0.25)
    assert zl.shape == () and float(zl.detach()) == 0.25 * 12.0 / tokens
    zl.backward()
    assert z.grad.shape == (1,)
    assert float(z.grad) == float(np.float32(0.25 / tokens))


# ---- the C entry points reject, never abort (no device is touched) ----------

P = [ctypes.c_void_p(0x1000 * i) for i in range(1, 12)]
NULL = None


def test_router_topk_aux_rejections():
    f = sp.lib().sputnik_router_topk_aux
    bad = sp.hipErrorInvalidValue
    names = ("logits", "top", "w", "scores", "sums", "z", "ws")

    def call(logits=P[0], top=P[1], w=P[2], scores=NULL, sums=P[4], z=P[5],
             tokens=4, e=8, k=2, norm=0, ldtype=1, wdtype=0, ws=P[6],
             ws_bytes=36):
        return f(logits, top, w, scores, sums, z, tokens, e, k, norm, ldtype,
                 wdtype, ws, ws_bytes, NULL)

    for kw in (dict(tokens=-1), dict(e=0), dict(e=-3), dict(e=1025),
               dict(k=0), dict(k=-1), dict(k=9), dict(e=64, k=33),
               dict(ldtype=3), dict(ldtype=-1), dict(wdtype=2),
               dict(wdtype=-1),
               dict(logits=NULL), dict(top=NULL), dict(w=NULL),
               dict(sums=NULL), dict(ws=NULL),
               dict(tokens=0, sums=NULL),       # required even for no tokens
               dict(ws_bytes=35), dict(ws_bytes=0),
               dict(tokens=A.T + 1, ws_bytes=71),                # two groups
               dict(ws=ctypes.c_void_p(0x7002))):                # alignment
        assert call(**kw) == bad, kw
    for i, a in enumerate(names):               # any two buffers the same
        for b in names[i + 1:]:
            assert call(**{a: P[9], b: P[9]}) == bad, (a, b)


def test_router_topk_aux_grad_rejections():
    f = sp.lib().sputnik_router_topk_aux_grad
    bad = sp.hipErrorInvalidValue

    def call(logits=P[0], top=P[1], dw=P[2], ds=NULL, dss=NULL, dz=NULL,
             dl=P[6], tokens=4, e=8, k=2, norm=1, ldtype=0, wdtype=1):
        return f(logits, top, dw, ds, dss, dz, dl, tokens, e, k, norm, ldtype,
                 wdtype, NULL)

    for kw in (dict(tokens=-1), dict(e=0), dict(e=1025), dict(k=0),
               dict(k=9), dict(e=64, k=33), dict(ldtype=3), dict(wdtype=2),
               dict(logits=NULL), dict(top=NULL), dict(dw=NULL),
               dict(dl=NULL), dict(dl=P[0]), dict(dl=P[1]), dict(dl=P[2]),
               dict(ds=P[3], dl=P[3]), dict(dss=P[4], dl=P[4]),
               dict(dz=P[5], dl=P[5])):
        assert call(**kw) == bad, kw
    assert call(tokens=0, logits=NULL, top=NULL, dw=NULL, dl=NULL) == 0
