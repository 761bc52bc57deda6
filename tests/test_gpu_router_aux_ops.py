"""GPU: the auxiliary-loss ops of sputnik_amd/ops.py: moe_router_aux with
autograd, load_balancing_loss, router_z_loss and moe_layer_aux.

moe_router_aux's weights and ids are moe_router's bit for bit. The two
losses formed from its statistics are compared, value and gradient, with the
same losses formed in torch from logits.double().softmax(-1) / logsumexp,
under the bounds of tests/router_aux_ref.py. moe_layer_aux is compared bit
for bit with moe_layer where no loss is added (operands and
shapes of tests/test_gpu_router_ops.py), and runs without a host sync when
`rows` is given.
"""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from sputnik_amd import ops  # noqa: E402
from tests import router_aux_ref as A  # noqa: E402
from tests import router_ref as R  # noqa: E402
from tests.test_gpu_moe_ops import (D_MODEL, EXPERTS, TOKENS,  # noqa: E402
                                    TOP_K, _mlp_data)
from tests.test_gpu_router_ops import _bf16, _layer_operands  # noqa: E402

pytestmark = pytest.mark.gpu

_TORCH = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
LOSS_CASES = [(3 * A.T + 5, 8, 2), (33, 256, 8)]
LB_WEIGHT, Z_WEIGHT = 0.01, 0.001


def _np(t):
    return t.detach().float().cpu().numpy()


def _logits(case, ltype):
    l = A.logits(case, "random", ltype)
    return l, torch.from_numpy(np.array(l)).to(_TORCH[ltype]).cuda() \
        .requires_grad_(True)


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("ltype,wtype", [("bf16", "bf16"), ("bf16", "f32"),
                                         ("f16", "f16"), ("f32", "f32")])
def test_moe_router_aux_is_moe_router(ltype, wtype, normalize):
    case = LOSS_CASES[0]
    tokens, e, k = case
    l, logits = _logits(case, ltype)
    wd = None if wtype == ltype else torch.float32
    w, top, sums, z = ops.moe_router_aux(logits, k, normalize, wd)
    w0, top0 = ops.moe_router(logits, k, normalize, wd)
    assert top.dtype == torch.int32 and not top.requires_grad
    assert torch.equal(top, top0)
    assert w.dtype == _TORCH[wtype] and torch.equal(w, w0)
    assert w.requires_grad and sums.requires_grad and z.requires_grad
    assert sums.dtype == z.dtype == torch.float32
    assert sums.shape == (e,) and z.shape == (1,)
    sums_ref, z_ref, m, lse = A.stats64(l)
    assert (np.abs(_np(sums) - sums_ref)
            <= A.score_sums_bound(sums_ref, tokens, e)).all()
    assert abs(float(z.detach().cpu()[0]) - z_ref) <= A.z_sum_bound(
        z_ref, m, lse, e)
    # the gradient of the weights alone is moe_router's, bit for bit
    dw = torch.from_numpy(np.array(R.grad_inputs(case, ltype, wtype)[0])) \
        .to(_TORCH[wtype]).cuda()
    w.backward(dw)
    got, logits.grad = logits.grad, None
    w0.backward(dw)
    assert torch.equal(got, logits.grad)


@pytest.mark.parametrize("ltype", ["f32", "bf16"])
@pytest.mark.parametrize("case", LOSS_CASES,
                         ids=["%dx%d-k%d" % c for c in LOSS_CASES])
def test_losses_against_torch(case, ltype):
    tokens, e, k = case
    l, logits = _logits(case, ltype)
    _, top, sums, z = ops.moe_router_aux(logits, k)
    tpe = torch.bincount(top.reshape(-1).long(), minlength=e)
    assert int(tpe.sum()) == tokens * k
    lb = ops.load_balancing_loss(sums, tpe, tokens, k, LB_WEIGHT)
    zl = ops.router_z_loss(z, tokens, Z_WEIGHT)
    loss = lb + zl
    assert loss.shape == () and loss.dtype == torch.float32
    loss.backward()

    # the same losses in torch, float64
    ref_logits = logits.detach().double().requires_grad_(True)
    scale = LB_WEIGHT * e / (tokens * tokens * k)
    p = ref_logits.softmax(-1)
    lb_ref = scale * (tpe.double() * p.sum(0)).sum()
    z_ref = Z_WEIGHT * (torch.logsumexp(ref_logits, -1) ** 2).sum() / tokens
    (lb_ref + z_ref).backward()

    # value: the statistics' bounds through the two linear forms, plus the
    # fp32 roundings of the dot product over E terms, the two scalings and
    # the final addition ((E + 4) 2^-24 of the magnitudes; every term of
    # the dot product is >= 0)
    sums_ref, zs_ref, m, lse = A.stats64(l)
    counts = tpe.cpu().numpy().astype(np.float64)
    bound = (scale * float((counts * A.score_sums_bound(sums_ref, tokens,
                                                        e)).sum())
             + Z_WEIGHT / tokens * A.z_sum_bound(zs_ref, m, lse, e)
             + (e + 4) * A.U * (abs(lb_ref.item()) + abs(z_ref.item())))
    err = abs(loss.item() - (lb_ref + z_ref).item())
    print("loss", loss.item(), "share of the bound",
          err / bound)
    assert err <= bound
    # gradient: both against torch's and under router_aux_ref's bound
    ids = top.cpu().numpy()
    zero_dw = np.zeros((tokens, k), np.float32)
    ref, image = A.grad64(l, ids, zero_dw, None, scale * counts,
                          np.array([Z_WEIGHT / tokens]), False)
    assert np.allclose(ref, ref_logits.grad.cpu().numpy(), rtol=1e-9,
                       atol=1e-15)
    assert logits.grad.dtype == logits.dtype
    g_err = np.abs(_np(logits.grad).astype(np.float64) - ref)
    g_bound = A.grad_bound(ref, image, e, k, ltype)
    print("gradient: share of the bound",
          float((g_err / np.maximum(g_bound, 1e-300)).max()))
    assert (g_err <= g_bound).all()
    # one loss alone reaches the logits too (the other gradient is absent)
    for which in (0, 1):
        logits.grad = None
        _, _, sums, z = ops.moe_router_aux(logits, k)
        (ops.load_balancing_loss(sums, tpe, tokens, k, LB_WEIGHT) if which
         == 0 else ops.router_z_loss(z, tokens, Z_WEIGHT)).backward()
        ref, image = A.grad64(
            l, ids, zero_dw, None, scale * counts if which == 0 else None,
            None if which == 0 else np.array([Z_WEIGHT / tokens]), False)
        assert (np.abs(_np(logits.grad).astype(np.float64) - ref)
                <= A.grad_bound(ref, image, e, k, ltype)).all(), which


def _layer(d, glu, aux, add_loss, rows=None, operands=None, dy=None):
    x, wr, w1, w2, v1 = operands or _layer_operands(d, glu, None)
    dy = _bf16(d["dy"], False) if dy is None else dy
    layer = ops.moe_layer_aux if aux else ops.moe_layer
    out = layer(x, wr, w1, w2, TOP_K, v1=v1, rows=rows, normalize=True)
    y, info = out if aux else (out, None)
    if add_loss:
        loss = (ops.load_balancing_loss(info.score_sums,
                                        info.tokens_per_expert, info.tokens,
                                        info.top_k, 1.0)
                + ops.router_z_loss(info.z_sum, info.tokens, 0.1))
        torch.autograd.backward([y, loss], [dy, None])
    else:
        y.backward(dy)
    return y.detach(), info, x.grad, wr.grad, w1.grad, w2.grad


@pytest.mark.parametrize("glu", [False, True], ids=["mlp", "glu"])
def test_moe_layer_aux(glu):
    d = _mlp_data()
    plain = _layer(d, glu, False, False)
    aux = _layer(d, glu, True, False)
    info = aux[1]
    assert isinstance(info, ops.MoeAux)
    assert (info.tokens, info.top_k) == (TOKENS, TOP_K)
    assert info.score_sums.shape == (EXPERTS,) and info.z_sum.shape == (1,)
    assert info.score_sums.dtype == info.z_sum.dtype == torch.float32
    assert info.tokens_per_expert.dtype == torch.int32
    assert int(info.tokens_per_expert.sum()) == TOKENS * TOP_K
    assert abs(info.score_sums.sum().item() - TOKENS) < 1e-3 * TOKENS
    assert aux[0].shape == (TOKENS, D_MODEL)
    for i in (0, 2, 3, 4, 5):       # y and the gradients of x, wr, w1, w2
        assert torch.equal(plain[i], aux[i]), i
    with_loss = _layer(d, glu, True, True)
    assert torch.equal(with_loss[0], plain[0])
    for i in (4, 5):                # the experts do not see the losses
        assert torch.equal(with_loss[i], plain[i]), i
    assert not torch.equal(with_loss[3], plain[3])
    assert torch.isfinite(with_loss[3].float()).all()


def test_moe_layer_aux_makes_no_host_sync():
    d = _mlp_data()
    rows = ops.moe_rows_bound(TOKENS * TOP_K, EXPERTS)
    _layer(d, True, True, True, rows)       # (first-use initialisation)
    operands = _layer_operands(d, True, None)
    dy = _bf16(d["dy"], False)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        y, info, dx, dwr, _, _ = _layer(d, True, True, True, rows, operands,
                                        dy)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert int(info.tokens_per_expert.sum()) == TOKENS * TOP_K
    assert torch.isfinite(y.float()).all() and dwr.abs().max() > 0


def test_moe_layer_aux_does_not_return_scores():
    """The statistics replace the scores: asking for both raises."""
    d = _mlp_data()
    x, wr, w1, w2, _ = _layer_operands(d, False, None)
    with pytest.raises(TypeError):
        ops.moe_layer_aux(x, wr, w1, w2, TOP_K, return_scores=True)
