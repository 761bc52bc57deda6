"""GPU: the sigmoid-score router through the bindings (RouterScoreTopK,
RouterScoreTopKGrad; sputnik/block/router.h).

The picks are compared exactly with the float64 picks of
tests/router_score_ref.py, on inputs that meet its gap condition; weights,
scores and the gradient with float64 numpy under that file's bounds (which
tests/test_router_score_host.py shows a float32 emulation to meet on these
very inputs). Every output starts as garbage.
"""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import sputnik_amd as sp  # noqa: E402
from tests import router_score_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

_TORCH = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
SCALES = {False: 1.0, True: 2.5}     # normalize -> the scale used with it


def _dev(a, t):
    return torch.from_numpy(np.array(a)).to(_TORCH[t]).cuda()


def _np(t):
    return t.detach().float().cpu().numpy()


def _wtypes(ltype):
    return [ltype] if ltype == "f32" else [ltype, "f32"]


def _topk(l, b, case, ltype, wtype, normalize, scale, with_scores, raw=False):
    tokens, e, k, g, gk = case
    logits = _dev(l, ltype)
    bias = None if b is None else torch.from_numpy(np.array(b)).cuda()
    # (outputs start as garbage: every element must be written)
    top = torch.full((tokens, k), -5, dtype=torch.int32, device="cuda")
    w = torch.full((tokens, k), float("nan"), dtype=_TORCH[wtype],
                   device="cuda")
    scores = (torch.full((tokens, e), float("nan"), dtype=_TORCH[wtype],
                         device="cuda") if with_scores else None)
    sp.RouterScoreTopK(logits, top, w, bias, g, gk, normalize, scale, scores)
    if raw:
        return top, w, scores
    return (top.cpu().numpy(), _np(w).astype(np.float64),
            None if scores is None else _np(scores).astype(np.float64))


@pytest.mark.parametrize("ltype", R.LTYPES)
@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_picks_are_exact(case, ltype):
    tokens, e, k, g, gk = case
    for kind in R.KINDS:
        l, b = R.logits(case, kind, ltype), R.bias(case, kind)
        want = R.picks64(l, b, case)
        for normalize, scale in SCALES.items():
            top, _, _ = _topk(l, b, case, ltype, ltype, normalize, scale,
                              kind == "ties")
            assert top.dtype == np.int32
            if kind == "special":
                assert ((top >= 0) & (top < e)).all()
                assert all(len(set(row)) == k for row in top.tolist())
            assert np.array_equal(top, want), (kind, normalize)
        if kind == "equal":
            assert (want == np.arange(k)).all()


@pytest.mark.parametrize("ltype", R.LTYPES)
@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_weights_and_scores_within_bounds(case, ltype):
    tokens, e, k, g, gk = case
    for kind in R.VALUE_KINDS:
        l, b = R.logits(case, kind, ltype), R.bias(case, kind)
        ids = R.picks64(l, b, case)
        for normalize, scale in SCALES.items():
            w_ref, s_ref = R.forward64(l, ids, normalize, scale)
            for wtype in _wtypes(ltype):
                top, w, s = _topk(l, b, case, ltype, wtype, normalize, scale,
                                  True)
                what = (kind, normalize, wtype)
                assert np.array_equal(top, ids), what
                w_err = np.abs(w - w_ref)
                s_err = np.abs(s - s_ref)
                wb = R.weights_bound(w_ref, k, wtype)
                sb = R.scores_bound(s_ref, wtype)
                print(what, "weights: share of the bound",
                      float((w_err / wb).max()), "scores:",
                      float((s_err / sb).max()))
                assert (w_err <= wb).all(), what
                assert (s_err <= sb).all(), what


@pytest.mark.parametrize("case", [c for c in R.CASES if c[3] == 1],
                         ids=[i for c, i in zip(R.CASES, R.IDS) if c[3] == 1])
def test_null_bias_is_a_zero_bias(case):
    """Without groups, bias = None and a bias of zeros give the same bits."""
    tokens, e, k, g, gk = case
    zero = np.zeros(e, dtype=np.float32)
    for ltype in R.LTYPES:
        for kind in R.KINDS:
            l = R.logits(case, kind, ltype)
            a = _topk(l, None, case, ltype, ltype, True, 2.5, True, raw=True)
            b = _topk(l, zero, case, ltype, ltype, True, 2.5, True, raw=True)
            assert torch.equal(a[0], b[0]), (ltype, kind)
            for x, y in zip(a[1:], b[1:]):      # (NaN rows: compare bits)
                assert torch.equal(x.view(torch.int16 if ltype != "f32"
                                          else torch.int32),
                                   y.view(torch.int16 if ltype != "f32"
                                          else torch.int32)), (ltype, kind)
            if kind != "special":
                want = R.picks64(l, zero, case)
                assert np.array_equal(a[0].cpu().numpy(), want)


@pytest.mark.parametrize("ltype", ["f16", "bf16"])
def test_scale_is_applied_before_the_single_rounding(ltype):
    """The weights in the logits' type are the fp32 weights (scale applied)
    rounded once, bit for bit: not rounded weights times the scale."""
    case = (33, 256, 8, 8, 4)
    l, b = R.logits(case, "random", ltype), R.bias(case, "random")
    differs = False
    for normalize in (False, True):
        _, w32, s32 = _topk(l, b, case, ltype, "f32", normalize, 2.5, True,
                            raw=True)
        _, w, s = _topk(l, b, case, ltype, ltype, normalize, 2.5, True,
                        raw=True)
        assert torch.equal(w, w32.to(_TORCH[ltype]))
        assert torch.equal(s, s32.to(_TORCH[ltype]))
        _, w1, _ = _topk(l, b, case, ltype, ltype, normalize, 1.0, False,
                         raw=True)
        differs |= not torch.equal(w, (w1.float() * 2.5).to(_TORCH[ltype]))
    # (the test tells the two apart on these inputs)
    assert differs


@pytest.mark.parametrize("ltype", R.LTYPES)
@pytest.mark.parametrize("case", R.CASES, ids=R.IDS)
def test_gradient_within_bound(case, ltype):
    """On picks that hold an id past E, a negative id and a repeated id."""
    tokens, e, k, g, gk = case
    l = R.logits(case, "random", ltype)
    ids = R.grad_ids(case, ltype)
    logits = _dev(l, ltype)
    top = torch.from_numpy(np.array(ids)).cuda()
    for wtype in _wtypes(ltype):
        dw, ds = R.grad_inputs(case, ltype, wtype)
        dw_d, ds_d = _dev(dw, wtype), _dev(ds, wtype)
        for normalize, scale in SCALES.items():
            for dscores, dscores_d in ((None, None), (ds, ds_d)):
                dlogits = torch.full((tokens, e), float("nan"),
                                     dtype=_TORCH[ltype], device="cuda")
                sp.RouterScoreTopKGrad(logits, top, dw_d, dlogits, normalize,
                                       scale, dscores_d)
                got = _np(dlogits).astype(np.float64)
                ref, image, s = R.grad64(l, ids, dw, dscores, normalize,
                                         scale)
                bound = R.grad_bound(ref, image, s, k, ltype)
                err = np.abs(got - ref)
                what = (wtype, normalize, dscores is not None)
                print(what, "gradient: share of the bound",
                      float((err / np.maximum(bound, 1e-300)).max()))
                assert np.isfinite(got).all(), what
                assert (err <= bound).all(), what


def test_no_tokens():
    logits = torch.empty(0, 8, dtype=torch.bfloat16, device="cuda")
    top = torch.empty(0, 2, dtype=torch.int32, device="cuda")
    w = torch.empty(0, 2, dtype=torch.bfloat16, device="cuda")
    sp.RouterScoreTopK(logits, top, w, None, 4, 2)
    sp.RouterScoreTopKGrad(logits, top, w, torch.empty_like(logits))
    torch.cuda.synchronize()
