"""GPU: the sigmoid-score router ops of sputnik_amd/ops.py: moe_score_router
with autograd, moe_score_layer and router_bias_update.

moe_score_router is compared with the torch formulation of the DeepSeek-V3
gate (sigmoid, view into groups, topk(2).sum, topk over the groups, mask,
topk, gather, normalise, scale) on inputs that meet the gap condition of
tests/router_score_ref.py, so that the picks have one right answer: ids
exactly, weights and the gradient (torch autograd) within tests/helpers.RTOL.
moe_score_layer is compared bit for bit with its composition written out by
hand, as tests/test_gpu_router_ops.py does for moe_layer, whose operands
these tests use.
"""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from sputnik_amd import ops  # noqa: E402
from tests import router_score_ref as R  # noqa: E402
from tests.helpers import assert_close  # noqa: E402
from tests.test_gpu_moe_ops import (D_MODEL, EXPERTS, TOKENS,  # noqa: E402
                                    TOP_K, _mlp_data)
from tests.test_gpu_router_ops import (_bf16, _layer_operands,  # noqa: E402
                                       _np)

pytestmark = pytest.mark.gpu

_TORCH = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
V3 = (33, 256, 8, 8, 4)
GROUPS, TOP_GROUPS, SCALE = 2, 1, 2.5      # of the layer tests (4 experts)


def torch_gate(logits, bias, k, g, gk, normalize, scale):
    """The DeepSeek-V3 gate in torch, fp32: (weights, ids)."""
    tokens, e = logits.shape
    s = logits.float().sigmoid()
    c = s + bias
    if g > 1:
        group = c.view(tokens, g, e // g).topk(min(2, e // g), dim=-1)[0] \
            .sum(dim=-1)
        on = torch.zeros_like(group, dtype=torch.bool).scatter_(
            1, group.topk(gk, dim=-1)[1], True)
        mask = on.unsqueeze(-1).expand(tokens, g, e // g).reshape(tokens, e)
        c = c.masked_fill(~mask, float("-inf"))
    ids = c.topk(k, dim=-1)[1]
    w = s.gather(1, ids)
    if normalize:
        w = w / w.sum(dim=-1, keepdim=True)
    return w * scale, ids


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("ltype,wtype", [("bf16", "bf16"), ("bf16", "f32"),
                                         ("f16", "f16"), ("f32", "f32")])
@pytest.mark.parametrize("case", [V3, (300, 8, 2, 1, 1)],
                         ids=["v3", "no-groups"])
def test_moe_score_router_against_the_torch_gate(case, ltype, wtype,
                                                 normalize):
    tokens, e, k, g, gk = case
    l, b = R.logits(case, "random", ltype), R.bias(case, "random")
    dw, ds = R.grad_inputs(case, ltype, wtype)
    logits = torch.from_numpy(np.array(l)).to(_TORCH[ltype]).cuda() \
        .requires_grad_(True)
    bias = torch.from_numpy(np.array(b)).cuda()
    wd = None if wtype == ltype else torch.float32
    w, top, scores = ops.moe_score_router(
        logits, k, bias, g, gk, normalize, SCALE, wd, return_scores=True)
    assert top.dtype == torch.int32 and not top.requires_grad
    assert w.dtype == scores.dtype == _TORCH[wtype]
    assert w.shape == (tokens, k) and scores.shape == (tokens, e)

    ref_logits = logits.detach().float().requires_grad_(True)
    w_ref, ids_ref = torch_gate(ref_logits, bias, k, g, gk, normalize, SCALE)
    assert torch.equal(top.long(), ids_ref)
    assert np.array_equal(top.cpu().numpy(), R.picks64(l, b, case))
    tol = "bf16" if "bf16" in (ltype, wtype) and wtype != "f32" else "f16"
    assert_close(_np(w), _np(w_ref), tol, "weights")
    assert_close(_np(scores), _np(ref_logits.sigmoid()), tol, "scores")

    dw_d = torch.from_numpy(np.array(dw)).to(_TORCH[wtype]).cuda()
    ds_d = torch.from_numpy(np.array(ds)).to(_TORCH[wtype]).cuda()
    gtol = "bf16" if ltype == "bf16" else "f16"
    # weights and scores together, then the weights alone
    torch.autograd.backward([w, scores], [dw_d, ds_d], retain_graph=True)
    torch.autograd.backward([w_ref, ref_logits.sigmoid()],
                            [dw_d.float(), ds_d.float()], retain_graph=True)
    assert logits.grad.dtype == logits.dtype
    assert_close(_np(logits.grad), _np(ref_logits.grad), gtol, "dlogits")
    logits.grad = ref_logits.grad = None
    w.backward(dw_d)
    w_ref.backward(dw_d.float())
    assert_close(_np(logits.grad), _np(ref_logits.grad), gtol,
                 "dlogits from the weights")
    # the bias is not differentiable; without scores there are two outputs
    assert bias.grad is None
    out = ops.moe_score_router(logits.detach(), k, bias, g, gk, normalize,
                               SCALE, wd)
    assert len(out) == 2 and torch.equal(out[1], top)
    assert torch.equal(out[0], w.detach())


def _router_bias():
    return torch.tensor([0.125, -0.0625, 0.0, 0.03125], device="cuda")


@pytest.mark.parametrize("glu", [False, True], ids=["mlp", "glu"])
@pytest.mark.parametrize("router_dtype", [None, torch.float32],
                         ids=["bf16", "fp32-router"])
def test_moe_score_layer_is_its_composition(glu, router_dtype):
    d = _mlp_data()
    dy = _bf16(d["dy"], False)
    rows = ops.moe_rows_bound(TOKENS * TOP_K, EXPERTS)
    bias = _router_bias()
    results = []
    for whole in (True, False):
        x, wr, w1, w2, v1 = _layer_operands(d, glu, router_dtype)
        if whole:
            y = ops.moe_score_layer(
                x, wr, w1, w2, TOP_K, v1=v1, rows=rows, normalize=True,
                router_dtype=router_dtype, router_bias=bias,
                num_groups=GROUPS, topk_groups=TOP_GROUPS, routed_scale=SCALE)
        else:
            rd = x.dtype if router_dtype is None else router_dtype
            logits = x.to(rd) @ wr.to(rd).t()
            gates, top = ops.moe_score_router(logits, TOP_K, bias, GROUPS,
                                              TOP_GROUPS, True, SCALE)
            assert gates.dtype == rd
            # (one group of two is eligible: both its experts are picked)
            assert (top // 2 == top[:, :1] // 2).all()
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
    # the backward reaches the router weight
    assert y.abs().max() > 0 and dwr.abs().max() > 0 and dx.abs().max() > 0
    # it is another layer than the softmax one
    x, wr, w1, w2, v1 = _layer_operands(d, glu, router_dtype)
    soft = ops.moe_layer(x, wr, w1, w2, TOP_K, v1=v1, rows=rows,
                         normalize=True, router_dtype=router_dtype)
    assert not torch.equal(soft.detach(), y)


def test_moe_score_layer_with_explicit_rows_makes_no_host_sync():
    d = _mlp_data()
    rows = ops.moe_rows_bound(TOKENS * TOP_K, EXPERTS)
    dy = _bf16(d["dy"], False)
    bias = _router_bias()

    def run(x, wr, w1, w2, v1):
        y, scores, tpe = ops.moe_score_layer(
            x, wr, w1, w2, TOP_K, v1=v1, rows=rows, return_scores=True,
            router_bias=bias, num_groups=GROUPS, topk_groups=TOP_GROUPS,
            routed_scale=SCALE)
        y.backward(dy)
        ops.router_bias_update(bias, tpe, 0.001)
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
    assert scores.shape == (TOKENS, EXPERTS)
    assert ((scores.float() >= 0) & (scores.float() <= 1)).all()
    assert torch.isfinite(y.float()).all() and dwr.abs().max() > 0


def test_moe_layer_defaults_are_untouched():
    """moe_layer takes the softmax path it took, bit for bit: the composition
    of tests/test_gpu_router_ops.py still holds with the score router
    present, and the two layers differ."""
    d = _mlp_data()
    rows = ops.moe_rows_bound(TOKENS * TOP_K, EXPERTS)
    x, wr, w1, w2, _ = _layer_operands(d, False, None)
    y = ops.moe_layer(x, wr, w1, w2, TOP_K, rows=rows)
    logits = x @ wr.t()
    gates, top = ops.moe_router(logits, TOP_K)
    want = ops.moe_mlp(x, ops.moe_device_route(top, EXPERTS, rows), gates, w1,
                       w2, EXPERTS)
    assert torch.equal(y, want)


def test_router_bias_update_unloads_an_overloaded_expert():
    tokens, e, k = 512, 8, 2
    rng = np.random.default_rng(3)
    l = rng.uniform(-2.0, 2.0, (tokens, e)).astype(np.float32)
    l[:, 0] += 4.0                          # everyone wants expert 0
    logits = torch.from_numpy(l).cuda()
    bias = torch.zeros(e, device="cuda")
    loads = []
    for _ in range(40):
        _, top = ops.moe_score_router(logits, k, bias)
        tpe = ops.moe_device_route(top, e).tokens_per_expert
        loads.append(tpe)
        out = ops.router_bias_update(bias, tpe, 0.02)
        assert out is bias
    loads = torch.stack(loads).cpu().numpy()
    assert (loads.sum(axis=1) == tokens * k).all()
    assert loads[0, 0] == tokens
    assert bias[0].item() < -0.05 and bias[0] < bias[1:].min()
    assert loads[-1, 0] < loads[0, 0]
    assert loads[-1].max() - loads[-1].min() < loads[0].max() - loads[0].min()
