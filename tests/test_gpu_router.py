"""GPU: the MoE router and the device sort through the bindings (RouterTopK,
RouterTopKGrad, MoeSort; sputnik/block/router.h).

The picks are compared exactly with np.argsort(-l, kind="stable"); weights,
scores and the gradient with float64 numpy under the bounds of
tests/router_ref.py (which tests/test_router_host.py shows a float32
emulation to meet on these very inputs); MoeSort's tensors exactly with
tests/moe_ref.route, with ops.moe_route's torch.sort path, and for ids out of
range with router_ref.sort_ref.
"""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import sputnik_amd as sp  # noqa: E402
from sputnik_amd import ops  # noqa: E402
from tests import moe_ref  # noqa: E402
from tests import router_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

_IDS = ["%dx%d-k%d" % c for c in R.ROUTER_CASES]
_TORCH = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
_ROUTE = ("indices", "bin_ids", "bins", "padded_bins", "tokens_per_expert",
          "row_of")


def _dev(a, t):
    return torch.from_numpy(np.array(a)).to(_TORCH[t]).cuda()


def _np(t):
    return t.detach().float().cpu().numpy()


def _wtypes(ltype):
    return [ltype] if ltype == "f32" else [ltype, "f32"]


def _topk(l, k, ltype, wtype, normalize, with_scores):
    logits = _dev(l, ltype)
    tokens, e = l.shape
    # (outputs start as garbage: every element must be written)
    top = torch.full((tokens, k), -5, dtype=torch.int32, device="cuda")
    w = torch.full((tokens, k), float("nan"), dtype=_TORCH[wtype],
                   device="cuda")
    scores = (torch.full((tokens, e), float("nan"), dtype=_TORCH[wtype],
                         device="cuda") if with_scores else None)
    sp.RouterTopK(logits, top, w, normalize, scores)
    return (top.cpu().numpy(), _np(w).astype(np.float64),
            None if scores is None else _np(scores).astype(np.float64))


@pytest.mark.parametrize("ltype", R.LTYPES)
@pytest.mark.parametrize("case", R.ROUTER_CASES, ids=_IDS)
def test_picks_are_exact(case, ltype):
    tokens, e, k = case
    for kind in R.KINDS:
        l = R.logits(case, kind, ltype)
        want = R.expected_ids(l, k)
        for normalize in (False, True):
            top, _, _ = _topk(l, k, ltype, ltype, normalize, kind == "ties")
            assert top.dtype == np.int32
            assert np.array_equal(top, want), (kind, normalize)
        if kind == "equal":
            assert (want == np.arange(k)).all()


@pytest.mark.parametrize("ltype", R.LTYPES)
@pytest.mark.parametrize("case", R.ROUTER_CASES, ids=_IDS)
def test_weights_and_scores_within_bounds(case, ltype):
    tokens, e, k = case
    for kind in ("random", "ties", "equal"):
        l = R.logits(case, kind, ltype)
        ids = R.expected_ids(l, k)
        for normalize in (False, True):
            w_ref, p_ref = R.forward64(l, ids, normalize)
            for wtype in _wtypes(ltype):
                top, w, p = _topk(l, k, ltype, wtype, normalize, True)
                what = (kind, normalize, wtype)
                assert np.array_equal(top, ids), what
                w_err = np.abs(w - w_ref)
                p_err = np.abs(p - p_ref)
                wb = R.weights_bound(w_ref, e, k, wtype)
                pb = R.scores_bound(p_ref, e, wtype)
                print(what, "weights: share of the bound",
                      float((w_err / wb).max()), "scores:",
                      float((p_err / pb).max()))
                assert (w_err <= wb).all(), what
                assert (p_err <= pb).all(), what


@pytest.mark.parametrize("ltype", R.LTYPES)
@pytest.mark.parametrize("case", R.ROUTER_CASES, ids=_IDS)
def test_gradient_within_bound(case, ltype):
    """On picks that hold an id past E, a negative id and a repeated id."""
    tokens, e, k = case
    l = R.logits(case, "random", ltype)
    ids = R.grad_ids(case, ltype)
    logits = _dev(l, ltype)
    top = torch.from_numpy(np.array(ids)).cuda()
    for wtype in _wtypes(ltype):
        dw, ds = R.grad_inputs(case, ltype, wtype)
        dw_d, ds_d = _dev(dw, wtype), _dev(ds, wtype)
        for normalize in (False, True):
            for dscores, dscores_d in ((None, None), (ds, ds_d)):
                dlogits = torch.full((tokens, e), float("nan"),
                                     dtype=_TORCH[ltype], device="cuda")
                sp.RouterTopKGrad(logits, top, dw_d, dlogits, normalize,
                                  dscores_d)
                got = _np(dlogits).astype(np.float64)
                ref, image = R.grad64(l, ids, dw, dscores, normalize)
                bound = R.grad_bound(ref, image, e, k, ltype)
                err = np.abs(got - ref)
                what = (wtype, normalize, dscores is not None)
                print(what, "gradient: share of the bound",
                      float((err / np.maximum(bound, 1e-300)).max()))
                assert np.isfinite(got).all(), what
                assert (err <= bound).all(), what


# ---- sort -------------------------------------------------------------------

def _sort(ids, e, rows, fill=0):
    n = ids.size
    flat = torch.from_numpy(np.array(ids, dtype=np.int32)).cuda()
    out = {name: torch.full((n if name in ("indices", "bin_ids", "row_of")
                             else e,), -77, dtype=torch.int32, device="cuda")
           for name in _ROUTE}
    nbytes = sp.moe_sort_workspace_bytes(n, e)
    ws = torch.full((max(nbytes, 1),), fill, dtype=torch.uint8, device="cuda")
    sp.MoeSort(flat, e, rows, out["indices"], out["bin_ids"], out["bins"],
               out["tokens_per_expert"], out["padded_bins"], out["row_of"],
               ws)
    return {name: t.cpu().numpy() for name, t in out.items()}


def _assert_route(got, want, what):
    for name in _ROUTE:
        assert np.array_equal(got[name], getattr(want, name)), (what, name)


@pytest.mark.parametrize("e", R.SORT_E)
def test_moe_sort_matches_the_stable_sort(e):
    for n in R.SORT_N:
        ids = R.sort_ids(n, e)
        rows = moe_ref.rows_bound(n, e)
        want = moe_ref.route(ids.astype(np.int64).reshape(n, 1), e)
        got = _sort(ids, e, rows)
        _assert_route(got, want, (n, e))
        # a workspace of 0xff bytes gives the same
        again = _sort(ids, e, rows, fill=0xFF)
        for name in _ROUTE:
            assert np.array_equal(got[name], again[name]), (n, e, name)
        # and so does today's torch.sort route, tensor for tensor
        route = ops.moe_route(torch.from_numpy(np.array(ids)).cuda(), e, rows)
        for name in _ROUTE:
            assert np.array_equal(got[name], getattr(route, name).cpu()
                                  .numpy()), (n, e, name)


@pytest.mark.parametrize("case", moe_ref.CASES,
                         ids=["%dx%d-E%d-%s" % c for c in moe_ref.CASES])
def test_moe_sort_on_the_routing_kinds(case):
    tokens, top_k, e, kind = case
    want = moe_ref.case_route(case)
    ids = moe_ref.routing(*case).astype(np.int32).reshape(-1)
    exact = moe_ref.exact_rows(want)
    _assert_route(_sort(ids, e, exact), want, case)
    # fewer rows than the route needs: the rows past them map to -1
    if exact > 128:
        cut = _sort(ids, e, exact - 128)
        ref = np.where(want.row_of >= exact - 128, -1, want.row_of)
        assert np.array_equal(cut["row_of"], ref)
        assert (ref == -1).any()
        for name in _ROUTE[:-1]:
            assert np.array_equal(cut[name], getattr(want, name)), name
    for build in (ops.moe_route, ops.moe_device_route):
        route = build(torch.from_numpy(moe_ref.routing(*case)).cuda(), e)
        assert route.rows == exact
        assert (route.top_k, route.tokens) == (top_k, tokens)
        for name in _ROUTE:
            t = getattr(route, name)
            assert t.dtype == torch.int32
            assert np.array_equal(t.cpu().numpy(), getattr(want, name)), name


def test_moe_sort_with_ids_out_of_range():
    n, e = R.OUT_OF_RANGE_CASE
    ids = R.out_of_range_ids()
    rows = moe_ref.rows_bound(n, e)
    want = R.sort_ref(ids, e, rows)
    for fill in (0, 0xFF):
        got = _sort(ids, e, rows, fill)
        _assert_route(got, want, fill)
    bad = (ids < 0) | (ids >= e)
    assert (got["row_of"][bad] == -1).all()
    assert (got["bin_ids"][got["bins"][-1]:] == e).all()
    assert got["tokens_per_expert"].sum() == n - bad.sum()
    # nothing out of range reaches the gather: its rows are those of the
    # valid assignments alone
    x = torch.arange(1, n + 1, dtype=torch.float32).cuda() \
        .to(torch.bfloat16).reshape(n, 1).repeat(1, 8).contiguous()
    out = torch.empty(rows, 8, dtype=torch.bfloat16, device="cuda")
    dev = {k: torch.from_numpy(v).cuda() for k, v in got.items()}
    sp.PaddedGather(x, dev["indices"], dev["bins"], dev["padded_bins"], out,
                    1)
    ref = np.zeros((rows, 8), np.float32)
    ref[want.row_of[~bad]] = _np(x)[~bad]
    assert np.array_equal(_np(out), ref)


def test_moe_sort_of_nothing_writes_zero_counts():
    got = _sort(np.zeros(0, np.int32), 4, 0)
    for name in ("bins", "tokens_per_expert", "padded_bins"):
        assert (got[name] == 0).all(), name
