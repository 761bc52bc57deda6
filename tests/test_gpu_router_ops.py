"""GPU: the router ops of sputnik_amd/ops.py: moe_router with autograd,
moe_mlp over a moe_device_route, and moe_layer.

moe_router is held to the float64 reference and bounds of
tests/router_ref.py. moe_mlp over a route from moe_device_route is compared
bit for bit with moe_mlp over its own torch.sort route (the route tensors are
identical, so everything behind them must be), and moe_layer bit for bit
with the same composition written out by hand (x @ wr.t() -> moe_router ->
moe_device_route -> moe_mlp): the numerics of each piece are
pinned by its own tests, and a dense fp32 reference of the whole chain would
leave correct bf16 arithmetic too little room (see _mlp_data in
tests/test_gpu_moe_ops.py, whose operands these tests use).
"""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from sputnik_amd import ops  # noqa: E402
from tests import router_ref as R  # noqa: E402
from tests.test_gpu_moe_ops import (D_MODEL, EXPERTS, FFN, TOKENS,  # noqa: E402
                                    TOP_K, _mlp_data)

pytestmark = pytest.mark.gpu

_TORCH = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
CASE = (67, 8, 2)


def _np(t):
    return t.detach().float().cpu().numpy()


def _bf16(a, grad=True):
    return torch.from_numpy(np.array(a)).bfloat16().cuda().requires_grad_(grad)


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("ltype,wtype", [("bf16", "bf16"), ("bf16", "f32"),
                                         ("f16", "f16"), ("f32", "f32")])
def test_moe_router_forward_backward(ltype, wtype, normalize):
    tokens, e, k = CASE
    l = R.logits(CASE, "random", ltype)
    ids = R.expected_ids(l, k)
    dw, ds = R.grad_inputs(CASE, ltype, wtype)
    logits = torch.from_numpy(np.array(l)).to(_TORCH[ltype]).cuda() \
        .requires_grad_(True)
    wd = None if wtype == ltype else torch.float32
    w, top, scores = ops.moe_router(logits, k, normalize, wd,
                                    return_scores=True)
    assert top.dtype == torch.int32 and not top.requires_grad
    assert w.dtype == scores.dtype == _TORCH[wtype]
    assert w.shape == (tokens, k) and scores.shape == (tokens, e)
    assert np.array_equal(top.cpu().numpy(), ids)
    w_ref, p_ref = R.forward64(l, ids, normalize)
    assert (np.abs(_np(w) - w_ref) <= R.weights_bound(w_ref, e, k, wtype)).all()
    assert (np.abs(_np(scores) - p_ref)
            <= R.scores_bound(p_ref, e, wtype)).all()
    dw_d = torch.from_numpy(np.array(dw)).to(_TORCH[wtype]).cuda()
    ds_d = torch.from_numpy(np.array(ds)).to(_TORCH[wtype]).cuda()
    # weights and scores together, then the weights alone
    torch.autograd.backward([w, scores], [dw_d, ds_d], retain_graph=True)
    ref, image = R.grad64(l, ids, dw, ds, normalize)
    assert logits.grad.dtype == logits.dtype
    assert (np.abs(_np(logits.grad) - ref)
            <= R.grad_bound(ref, image, e, k, ltype)).all()
    logits.grad = None
    w.backward(dw_d)
    ref, image = R.grad64(l, ids, dw, None, normalize)
    assert (np.abs(_np(logits.grad) - ref)
            <= R.grad_bound(ref, image, e, k, ltype)).all()
    # without scores the function has two outputs
    out = ops.moe_router(logits.detach(), k, normalize, wd)
    assert len(out) == 2 and torch.equal(out[1], top)
    assert torch.equal(out[0], w.detach())


def _run_mlp(d, glu, rows, device_sort):
    top = torch.from_numpy(np.array(d["top"])).cuda()
    x, w1, w2 = (_bf16(d[k]) for k in ("x", "w1", "w2"))
    v1 = _bf16(d["v1"]) if glu else None
    gates = torch.from_numpy(np.array(d["gates"])).cuda().requires_grad_(True)
    if device_sort:
        top = ops.moe_device_route(top, EXPERTS, rows)
    y = ops.moe_mlp(x, top, gates, w1, w2, EXPERTS, v1=v1, rows=rows)
    y.backward(_bf16(d["dy"], False))
    leaves = [x, gates, w1, w2] + ([v1] if glu else [])
    return [y.detach()] + [t.grad for t in leaves]


@pytest.mark.parametrize("glu", [False, True], ids=["mlp", "glu"])
@pytest.mark.parametrize("explicit_rows", [False, True])
def test_moe_mlp_device_sort_is_bit_identical(glu, explicit_rows):
    d = _mlp_data()
    rows = (ops.moe_rows_bound(TOKENS * TOP_K, EXPERTS) if explicit_rows
            else None)
    a = _run_mlp(d, glu, rows, False)
    b = _run_mlp(d, glu, rows, True)
    assert len(a) == len(b) == (6 if glu else 5)
    for i, (s, t) in enumerate(zip(a, b)):
        assert s is not None and s.dtype == t.dtype, i
        assert torch.equal(s, t), i
    assert a[0].abs().max() > 0


def _router_weight():
    """[E, d_model] in {-1, 0, 1} / 16: with x in {-1, 0, 1} the logits are
    multiples of 1/16 below 16, exact in bf16."""
    rng = np.random.default_rng(23)
    return (rng.integers(-1, 2, (EXPERTS, D_MODEL)) / 16).astype(np.float32)


def _layer_operands(d, glu, router_dtype):
    x, w1, w2 = (_bf16(d[k]) for k in ("x", "w1", "w2"))
    v1 = _bf16(d["v1"]) if glu else None
    wr = torch.from_numpy(_router_weight()).cuda()
    if router_dtype is None:
        wr = wr.bfloat16()
    wr.requires_grad_(True)
    return x, wr, w1, w2, v1


@pytest.mark.parametrize("glu", [False, True], ids=["mlp", "glu"])
@pytest.mark.parametrize("router_dtype", [None, torch.float32],
                         ids=["bf16", "fp32-router"])
def test_moe_layer_is_its_composition(glu, router_dtype):
    d = _mlp_data()
    dy = _bf16(d["dy"], False)
    rows = ops.moe_rows_bound(TOKENS * TOP_K, EXPERTS)
    results = []
    for whole in (True, False):
        x, wr, w1, w2, v1 = _layer_operands(d, glu, router_dtype)
        if whole:
            y = ops.moe_layer(x, wr, w1, w2, TOP_K, v1=v1, rows=rows,
                              normalize=True, router_dtype=router_dtype)
        else:
            rd = x.dtype if router_dtype is None else router_dtype
            logits = x.to(rd) @ wr.to(rd).t()
            gates, top = ops.moe_router(logits, TOP_K, True)
            assert gates.dtype == rd
            y = ops.moe_mlp(x, ops.moe_device_route(top, EXPERTS, rows),
                            gates, w1, w2, EXPERTS, v1=v1)
        assert y.shape == (TOKENS, D_MODEL) and y.dtype == torch.bfloat16
        y.backward(dy)
        leaves = [x, wr, w1, w2] + ([v1] if glu else [])
        for t in leaves:
            assert t.grad is not None and t.grad.shape == t.shape
            assert t.grad.dtype == t.dtype
        results.append([y.detach()] + [t.grad for t in leaves])
    for i, (s, t) in enumerate(zip(*results)):
        assert torch.equal(s, t), i
    y, dx, dwr = results[0][:3]
    assert y.abs().max() > 0 and dwr.abs().max() > 0 and dx.abs().max() > 0
    # rows=None gives the same output, and either sort the same gradients
    grads = []
    for device_sort in (True, False):
        x, wr, w1, w2, v1 = _layer_operands(d, glu, router_dtype)
        again = ops.moe_layer(x, wr, w1, w2, TOP_K, v1=v1, normalize=True,
                              router_dtype=router_dtype,
                              device_sort=device_sort)
        again.backward(dy)
        assert torch.equal(again.detach(), y), device_sort
        grads.append([x.grad, wr.grad, w1.grad, w2.grad])
    for s, t in zip(*grads):
        assert torch.equal(s, t)


def test_moe_layer_with_explicit_rows_makes_no_host_sync():
    d = _mlp_data()
    rows = ops.moe_rows_bound(TOKENS * TOP_K, EXPERTS)
    dy = _bf16(d["dy"], False)

    def run(x, wr, w1, w2, v1):
        y, scores, tpe = ops.moe_layer(x, wr, w1, w2, TOP_K, v1=v1, rows=rows,
                                       device_sort=True, return_scores=True)
        y.backward(dy)
        return y, scores, tpe, x.grad, wr.grad

    first = _layer_operands(d, True, None)
    second = _layer_operands(d, True, None)
    run(*first)                             # (first-use initialisation)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        y, scores, tpe, dx, dwr = run(*second)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert int(tpe.sum()) == TOKENS * TOP_K
    assert torch.isfinite(y.float()).all() and dwr.abs().max() > 0


@pytest.mark.parametrize("router_dtype", [None, torch.float32])
def test_moe_layer_return_scores(router_dtype):
    d = _mlp_data()
    x, wr, w1, w2, _ = _layer_operands(d, False, router_dtype)
    y, scores, tpe = ops.moe_layer(x, wr, w1, w2, TOP_K,
                                   router_dtype=router_dtype,
                                   return_scores=True)
    want = torch.bfloat16 if router_dtype is None else torch.float32
    assert y.shape == (TOKENS, D_MODEL) and y.dtype == torch.bfloat16
    assert scores.shape == (TOKENS, EXPERTS) and scores.dtype == want
    assert tpe.shape == (EXPERTS,) and tpe.dtype == torch.int32
    assert int(tpe.sum()) == TOKENS * TOP_K
    assert scores.requires_grad
    # a load-balancing loss formed in torch reaches the router weight
    loss = (scores.float().mean(0) * tpe.float()).sum()
    loss.backward()
    assert wr.grad is not None and wr.grad.abs().max() > 0
    assert torch.allclose(scores.float().sum(1),
                          torch.ones(TOKENS, device="cuda"), atol=2e-2)
