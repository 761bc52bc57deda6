"""GPU: the router with the auxiliary-loss statistics through the bindings
(RouterTopKAux, RouterTopKAuxGrad; sputnik/block/router.h).

top_experts, weights and scores are compared bit for bit with RouterTopK's
(rows of NaN and infinities included); score_sums, z_sum and the gradient
with float64 numpy under the bounds of tests/router_aux_ref.py (which
tests/test_router_aux_host.py shows a float32 emulation in the kernels' order
to meet on these very inputs). The sums must not depend on what the workspace
held nor change between two calls, and with neither statistic's gradient the
gradient is RouterTopKGrad's bit for bit.
"""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import sputnik_amd as sp  # noqa: E402
from tests import router_aux_ref as A  # noqa: E402
from tests import router_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

_TORCH = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


def _dev(a, t):
    return torch.from_numpy(np.array(a)).to(_TORCH[t]).cuda()


def _np(t):
    return t.detach().float().cpu().numpy()


def _wtypes(ltype):
    return [ltype] if ltype == "f32" else [ltype, "f32"]


def _same_bits(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    as_int = torch.int16 if a.element_size() == 2 else torch.int32
    return torch.equal(a.view(as_int), b.view(as_int))


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _aux(logits, k, wtype, normalize, fill, with_z=True):
    """One RouterTopKAux on outputs preset to garbage (every element must be
    written) and a workspace of `fill` bytes."""
    tokens, e = logits.shape
    top = torch.full((tokens, k), -5, dtype=torch.int32, device="cuda")
    w = _nan((tokens, k), _TORCH[wtype])
    scores = _nan((tokens, e), _TORCH[wtype])
    sums = _nan((e,), torch.float32)
    z = _nan((1,), torch.float32) if with_z else None
    nbytes = sp.router_aux_workspace_bytes(tokens, e)
    ws = torch.full((max(nbytes, 1),), fill, dtype=torch.uint8, device="cuda")
    sp.RouterTopKAux(logits, top, w, sums, ws, normalize, scores, z)
    return top, w, scores, sums, z


@pytest.mark.parametrize("ltype", R.LTYPES)
@pytest.mark.parametrize("case", A.AUX_CASES, ids=A.IDS)
def test_forward_matches_router_topk_and_the_bounds(case, ltype):
    tokens, e, k = case
    for kind in A.kinds(case) + ["special"]:
        l = A.logits(case, kind, ltype)
        logits = _dev(l, ltype)
        if kind != "special":
            sums_ref, z_ref, m, lse = A.stats64(l)
            sb = A.score_sums_bound(sums_ref, tokens, e)
            zb = A.z_sum_bound(z_ref, m, lse, e)
        for normalize in (False, True):
            for wtype in _wtypes(ltype):
                what = (kind, normalize, wtype)
                top, w, scores, sums, z = _aux(logits, k, wtype, normalize,
                                               0xFF)
                top0 = torch.full_like(top, -5)
                w0, scores0 = torch.full_like(w, 1.0), torch.full_like(scores,
                                                                       1.0)
                sp.RouterTopK(logits, top0, w0, normalize, scores0)
                assert torch.equal(top, top0), what
                assert _same_bits(w, w0), what
                assert _same_bits(scores, scores0), what
                # the same call again, and on a zeroed workspace
                for fill in (0xFF, 0):
                    _, _, _, sums2, z2 = _aux(logits, k, wtype, normalize,
                                              fill)
                    assert _same_bits(sums, sums2), (what, fill)
                    assert _same_bits(z, z2), (what, fill)
                # without z_sum the sums are the same
                _, _, _, sums3, _ = _aux(logits, k, wtype, normalize, 0xFF,
                                         with_z=False)
                assert _same_bits(sums, sums3), what
                if kind == "special":
                    continue
                s_err = np.abs(_np(sums).astype(np.float64) - sums_ref)
                z_err = abs(float(z.cpu()[0]) - z_ref)
                print(what, "score_sums: share of the bound",
                      float((s_err / sb).max()), "z_sum:",
                      z_err / max(zb, 1e-300))
                assert (s_err <= sb).all(), what
                assert z_err <= zb, what


@pytest.mark.parametrize("ltype", R.LTYPES)
@pytest.mark.parametrize("case", A.AUX_CASES, ids=A.IDS)
def test_gradient_within_bound(case, ltype):
    """On picks that hold an id past E, a negative id and a repeated id, for
    every combination of absent and given dscore_sums / dz_sum."""
    tokens, e, k = case
    l = A.logits(case, "random", ltype)
    ids = R.grad_ids(case, ltype)
    logits = _dev(l, ltype)
    top = torch.from_numpy(np.array(ids)).cuda()
    dss, dz = A.aux_grads(case, ltype)
    dss_d, dz_d = _dev(dss, "f32"), _dev(dz, "f32")
    for wtype in _wtypes(ltype):
        dw, ds = R.grad_inputs(case, ltype, wtype)
        dw_d, ds_d = _dev(dw, wtype), _dev(ds, wtype)
        for normalize in (False, True):
            for dscores, dscores_d in ((None, None), (ds, ds_d)):
                for s, z in ((None, None), (dss, None), (None, dz),
                             (dss, dz)):
                    dlogits = _nan((tokens, e), _TORCH[ltype])
                    sp.RouterTopKAuxGrad(
                        logits, top, dw_d, dlogits, normalize, dscores_d,
                        None if s is None else dss_d,
                        None if z is None else dz_d)
                    what = (wtype, normalize, dscores is not None,
                            s is not None, z is not None)
                    if s is None and z is None:
                        plain = _nan((tokens, e), _TORCH[ltype])
                        sp.RouterTopKGrad(logits, top, dw_d, plain, normalize,
                                          dscores_d)
                        assert _same_bits(dlogits, plain), what
                    got = _np(dlogits).astype(np.float64)
                    ref, image = A.grad64(l, ids, dw, dscores, s, z,
                                          normalize)
                    bound = A.grad_bound(ref, image, e, k, ltype)
                    err = np.abs(got - ref)
                    print(what, "gradient: share of the bound",
                          float((err / np.maximum(bound, 1e-300)).max()))
                    assert np.isfinite(got).all(), what
                    assert (err <= bound).all(), what


def test_no_tokens_writes_zeros():
    e = 8
    logits = torch.empty(0, e, dtype=torch.bfloat16, device="cuda")
    top = torch.empty(0, 2, dtype=torch.int32, device="cuda")
    w = torch.empty(0, 2, dtype=torch.bfloat16, device="cuda")
    sums, z = _nan((e,), torch.float32), _nan((1,), torch.float32)
    assert sp.router_aux_workspace_bytes(0, e) == 0
    sp.RouterTopKAux(logits, top, w, sums, None, False, None, z)
    assert _same_bits(sums, torch.zeros_like(sums))
    assert _same_bits(z, torch.zeros_like(z))
    sp.RouterTopKAuxGrad(logits, top, w, torch.empty_like(logits), False,
                         None, sums, z)
    torch.cuda.synchronize()
