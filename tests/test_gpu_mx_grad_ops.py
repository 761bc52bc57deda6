"""GPU: ops.mlp_mx and ops.moe_mlp_mx_train on the shapes of
tests/test_gpu_fp8_grad_ops.py (96 tokens, top_k 2, 4 experts with one left
empty, d_model 256, 128 ffn columns per expert). The forward is held bit for
bit against the existing forward chain, each backward stage bit for bit
against the ctypes calls of mx.h's table, and each gradient against the
float64 product of its own dequantised operands within the header's bound.

The error against ops.mlp's gradients on the same 16-bit inputs measures the
format, not the code: it is printed, and only a regression cap of twice the
recorded value (FORMAT_ERROR) is asserted."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import sputnik_amd as sp  # noqa: E402
from sputnik_amd import ops  # noqa: E402
from tests import fp8_ref as F  # noqa: E402
from tests import moe_ref as M  # noqa: E402
from tests import mx_grad_ref as MG  # noqa: E402
from tests import mx_ref as R  # noqa: E402
from tests.test_gpu_fp8_grad_ops import (ACTS, D_MODEL, EXPERTS, HIDDEN,  # noqa: E402
                                         TOKENS, _bytes, _dev, _inputs, _np,
                                         _same)

pytestmark = pytest.mark.gpu

# Measured on an MI355X: relative 2-norm error of dx / dw1t / dw2, per
# activation the larger of the two dtypes. relu stands apart where act'
# enters, as tests/test_gpu_fp8_grad_ops.py explains.
FORMAT_ERROR = {"relu": (0.1680, 0.1672, 0.0496),
                "gelu": (0.0547, 0.0570, 0.0511),
                "silu": (0.0532, 0.0549, 0.0515)}


def _grads(xp, w1t, w2, dy, topo, act, need=(True, True, True),
           sinks=(None, None)):
    leaves = [t.detach().clone().requires_grad_(n)
              for t, n in zip((xp, w1t, w2), need)]
    y = ops.mlp_mx(*leaves, topo, act, *sinks)
    if y.requires_grad:
        y.backward(dy)
    return y.detach(), [t.grad for t in leaves]


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("dtype", M.DTYPES)
def test_mlp_mx_forward_and_every_backward_stage(dtype, act):
    xp, w1t, w2, dy, topo, route, *_ = _inputs(dtype)
    td, rows, nb = xp.dtype, route.rows, topo.nnz_blocks
    y, (dx, dw1t, dw2) = _grads(xp, w1t, w2, dy, topo, act)
    y2, again = _grads(xp, w1t, w2, dy, topo, act)      # the same bits twice
    assert _same(y, y2) and all(map(_same, (dx, dw1t, dw2), again))
    # Forward: the existing chain on the same weights.
    xq, xs = ops.quantize_rows_mx(xp)
    z = ops.sdd_mx(xq, xs, ops.quantize_weight_mx(w1t, transpose=True), topo,
                   td)
    assert _same(y, ops.dsd_mx(ops.quantize_sparse_mx(z, act),
                               ops.quantize_weight_mx(w2), td))
    # Backward, stage by stage through the bindings of the C ABI.
    topo._meta.ensure_transposed(z.data)
    topo._meta.ensure_row_indices(z.data)
    s = topo._meta.descriptor(z.data)

    def st(data):
        return sp.BlockMatrix(HIDDEN, rows, 128, nb * 128 * 128, data,
                              s.offsets_t, s.indices_t)

    def u8(*shape):
        return torch.empty(*shape, dtype=torch.uint8, device="cuda")

    def q8(*shape):
        return torch.empty(*shape, dtype=torch.float8_e4m3fn, device="cuda")

    def dense(m):
        return torch.empty(m, D_MODEL, dtype=td, device="cuda")
    w2q_t, w2s_t = q8(HIDDEN, D_MODEL), u8(HIDDEN, D_MODEL // 32)
    w1q, w1s = q8(D_MODEL, HIDDEN), u8(D_MODEL, HIDDEN // 32)
    sp.QuantizeWeightMx(w2, w2q_t, w2s_t, True)     # [n = F, k = h]
    sp.QuantizeWeightMx(w1t, w1q, w1s)              # [n = h, k = F]
    dyq, dys = q8(rows, D_MODEL), u8(rows, D_MODEL // 32)
    dyqt, dyst = q8(D_MODEL, rows), u8(D_MODEL, rows // 32)
    sp.QuantizeTilesMx(dy, dyq, dys, dyqt, dyst)
    xqt, xst = q8(D_MODEL, rows), u8(D_MODEL, rows // 32)
    sp.QuantizeTilesMx(xp, qt=xqt, scales_t=xst)
    hqt, hst = q8(nb, 128, 128), u8(nb * 128, 4)    # dW2 = H^T dY
    sp.QuantizeBlocksMx(s, qt=hqt, scales_t=hst, stage="act", activation=act)
    want_dw2 = dense(HIDDEN)
    sp.DsdMxWgrad(st(hqt), hst, dyqt, dyst,
                  sp.Matrix(HIDDEN, D_MODEL, want_dw2))
    dh = torch.empty(nb, 128, 128, dtype=td, device="cuda")  # dY W2^T
    sp.SddMx(dyq, dys, w2q_t, w2s_t, topo._meta.descriptor(dh))
    dzq, dzs, dzqt, dzst = (q8(nb, 128, 128), u8(nb * 128, 4),
                            q8(nb, 128, 128), u8(nb * 128, 4))
    sp.QuantizeBlocksMx(topo._meta.descriptor(dh), dzq, dzs, dzqt, dzst,
                        stage="act_grad", activation=act, z=z.data)
    want_dx, want_dw1 = dense(rows), dense(HIDDEN)  # dZ W1t, dZ^T X
    sp.DsdMx(topo._meta.descriptor(dzq), dzs, w1q, w1s,
             sp.Matrix(rows, D_MODEL, want_dx))
    sp.DsdMxWgrad(st(dzqt), dzst, xqt, xst,
                  sp.Matrix(HIDDEN, D_MODEL, want_dw1))
    assert _same(dw2, want_dw2) and _same(dx, want_dx)
    assert _same(dw1t, want_dw1)
    # Each gradient against float64 of its own dequantised operands.
    fwd = (topo.offsets.cpu().numpy(), topo.indices.cpu().numpy())
    bwd = (s.offsets_t.cpu().numpy(), s.indices_t.cpu().numpy())
    for name, got, blocks, scales, (m, k), meta, bq, bs, lim in (
            ("dx", dx, dzq, dzs, (rows, HIDDEN), fwd, w1q, w1s, R.bound),
            ("dw2", dw2, hqt, hst, (HIDDEN, rows), bwd, dyqt, dyst, MG.bound),
            ("dw1t", dw1t, dzqt, dzst, (HIDDEN, rows), bwd, xqt, xst,
             MG.bound)):
        a64 = R.decode(F.dense_from_blocks(m, k, *meta, _bytes(blocks)),
                       R.expand_block_scales(m, k, *meta, scales.cpu().numpy()))
        ref, absum = R.matmul64(a64, R.decode(_bytes(bq), bs.cpu().numpy()))
        err = np.abs(_np(got).astype(np.float64) - ref)
        assert (err <= lim(ref, absum, k, dtype)).all(), name


@pytest.mark.parametrize("dtype", M.DTYPES)
def test_needs_input_grad_subsets_and_sinks(dtype):
    xp, w1t, w2, dy, topo, *_ = _inputs(dtype)
    td = xp.dtype
    y, full = _grads(xp, w1t, w2, dy, topo, "gelu")
    for need in ((True, False, False), (False, True, False),
                 (False, False, True), (True, False, True),
                 (False, True, True), (False, False, False)):
        y1, got = _grads(xp, w1t, w2, dy, topo, "gelu", need)
        assert _same(y, y1)
        for n, g, f in zip(need, got, full):
            assert (g is None) if not n else _same(g, f), need
    # Sinks: sink = round(acc + sink_before), acc the fp32 accumulator, which
    # an fp32 sink of zeros receives exactly.
    acc = [torch.zeros(HIDDEN, D_MODEL, device="cuda") for _ in range(2)]
    _, got = _grads(xp, w1t, w2, dy, topo, "gelu", sinks=tuple(acc))
    assert got[1] is None and got[2] is None and _same(got[0], full[0])
    assert all(_same(a.to(td), f) for a, f in zip(acc, full[1:]))
    for sink_dtype in (torch.float32, td):
        before = [(torch.randn(HIDDEN, D_MODEL, device="cuda") / 8
                   ).to(sink_dtype) for _ in range(2)]
        sinks = [b.clone() for b in before]
        _grads(xp, w1t, w2, dy, topo, "gelu", sinks=tuple(sinks))
        for sink, b, a in zip(sinks, before, acc):
            assert _same(sink, (a + b.float()).to(sink_dtype))
    # a sink for a weight that does not itself require grad
    only = torch.zeros(HIDDEN, D_MODEL, device="cuda")
    _, got = _grads(xp, w1t, w2, dy, topo, "gelu", (True, False, False),
                    (None, only))
    assert got[1:] == [None, None] and _same(got[0], full[0])
    assert _same(only, acc[1])


@pytest.mark.parametrize("dtype", M.DTYPES)
def test_moe_mlp_mx_train_gradients_reach_every_input(dtype):
    xp, w1t, w2, dy, topo, route, x, top, ew = _inputs(dtype)
    leaves = [t.detach().clone().requires_grad_() for t in (x, ew, w1t, w2)]
    out = ops.moe_mlp_mx_train(leaves[0], top, *leaves[1:], EXPERTS)
    with torch.no_grad():       # forward: the inference layer, same weights
        want = ops.moe_mlp_mx(x, top, ew,
                              ops.quantize_weight_mx(w1t, transpose=True),
                              ops.quantize_weight_mx(w2), EXPERTS)
    assert _same(out.detach(), want)
    dout = _dev(M.values((TOKENS, D_MODEL), dtype, [35]), dtype)
    out.backward(dout)
    for name, t in zip(("x", "expert_weights", "w1t", "w2"), leaves):
        assert t.grad is not None and t.grad.shape == t.shape, name
        g = _np(t.grad)
        assert np.isfinite(g).all() and np.abs(g).max() > 0, name
    # a route built beforehand, and a sink
    sink = torch.zeros(HIDDEN, D_MODEL, device="cuda")
    again = [t.detach().clone().requires_grad_() for t in (x, ew)]
    ops.moe_mlp_mx_train(again[0], route, again[1], w1t, w2, EXPERTS,
                         dw2_out=sink).backward(dout)
    assert _same(again[0].grad, leaves[0].grad)
    assert _same(again[1].grad, leaves[1].grad)
    assert _same(sink.to(x.dtype), leaves[3].grad)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("dtype", M.DTYPES)
def test_format_error_of_the_gradients_against_the_16_bit_mlp(dtype, act):
    xp, w1t, w2, dy, topo, *_ = _inputs(dtype)
    ref = [t.detach().clone().requires_grad_() for t in (xp, w1t, w2)]
    ops.mlp(ref[0], ref[1].t(), ref[2], topo, act).backward(dy)
    _, got = _grads(xp, w1t, w2, dy, topo, act)
    rel = [float(np.linalg.norm(_np(g) - _np(r.grad))
                 / np.linalg.norm(_np(r.grad))) for g, r in zip(got, ref)]
    print(f"mlp_mx vs mlp {dtype} {act}: dx, dw1t, dw2 relative error", rel)
    assert all(v <= 2 * cap for v, cap in zip(rel, FORMAT_ERROR[act])), rel
