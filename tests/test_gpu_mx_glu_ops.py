"""GPU: ops.glu_mlp_mx and ops.moe_glu_mlp_mx_train on the shapes of
tests/test_gpu_fp8_glu_ops.py (96 tokens, top_k 2, 4 experts with one left
empty, d_model 256, 128 ffn columns per expert). The forward is held bit for
bit against the existing gated forward chain, each backward stage bit for bit
against the ctypes calls of mx.h's gated table, and each gradient against the
float64 product of its own dequantised operands within the header's bound.

The error against ops.glu_mlp's gradients on the same 16-bit inputs measures
the format, not the code: it is printed beside that of the fp8 path with
power-of-two scales in the fast mode, and asserted to be at most twice that
one. Both lose at most one binade to the power-of-two scale and MX groups are
finer (32 against 128); the factor 2 covers the sampling noise of 96 tokens.
Measured on an MI355X: both paths 0.059 - 0.064 on every gradient,
equal to the fourth decimal."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import sputnik_amd as sp  # noqa: E402
from sputnik_amd import ops  # noqa: E402
from tests import fp8_ref as F  # noqa: E402
from tests import moe_ref as M  # noqa: E402
from tests import mx_grad_ref as MG  # noqa: E402
from tests import mx_ref as R  # noqa: E402
from tests.test_gpu_fp8_glu_ops import _inputs  # noqa: E402
from tests.test_gpu_fp8_grad_ops import (ACTS, D_MODEL, EXPERTS, HIDDEN,  # noqa: E402
                                         _bytes, _dev, _np, _same)

pytestmark = pytest.mark.gpu

NAMES = ("dx", "dw1t", "dv1t", "dw2")


def _grads(xp, w1t, v1t, w2, dy, topo, act, need=(True,) * 4,
           sinks=(None,) * 3):
    leaves = [t.detach().clone().requires_grad_(n)
              for t, n in zip((xp, w1t, v1t, w2), need)]
    y = ops.glu_mlp_mx(*leaves, topo, act, *sinks)
    if y.requires_grad:
        y.backward(dy)
    return y.detach(), [t.grad for t in leaves]


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("dtype", M.DTYPES)
def test_glu_mlp_mx_forward_and_every_backward_stage(dtype, act):
    v1t, xp, w1t, w2, dy, topo, route, *_ = _inputs(dtype)
    td, rows, nb = xp.dtype, route.rows, topo.nnz_blocks
    y, grads = _grads(xp, w1t, v1t, w2, dy, topo, act)
    y2, again = _grads(xp, w1t, v1t, w2, dy, topo, act)  # the same bits twice
    assert _same(y, y2) and all(map(_same, grads, again))
    # Forward: the existing gated chain on the same weights.
    xq, xs = ops.quantize_rows_mx(xp)
    g, u = (ops.sdd_mx(xq, xs, ops.quantize_weight_mx(w, transpose=True),
                       topo, td) for w in (w1t, v1t))
    assert _same(y, ops.dsd_mx(ops.quantize_sparse_mx(u, act, gate=g),
                               ops.quantize_weight_mx(w2), td))
    # Backward, stage by stage through the bindings of the C ABI.
    meta = topo._meta
    meta.ensure_transposed(u.data)
    meta.ensure_row_indices(u.data)
    s = meta.descriptor(u.data)

    def st(data):
        return sp.BlockMatrix(HIDDEN, rows, 128, nb * 128 * 128, data,
                              s.offsets_t, s.indices_t)

    def u8(*shape):
        return torch.empty(*shape, dtype=torch.uint8, device="cuda")

    def q8(*shape):
        return torch.empty(*shape, dtype=torch.float8_e4m3fn, device="cuda")

    images = lambda: ops._lowp_images(      # noqa: E731
        ops._MX, nb, True, True, "cuda")
    w2q_t, w2s_t = q8(HIDDEN, D_MODEL), u8(HIDDEN, D_MODEL // 32)
    sp.QuantizeWeightMx(w2, w2q_t, w2s_t, True)     # [n = F, k = h]
    wq = [(q8(D_MODEL, HIDDEN), u8(D_MODEL, HIDDEN // 32)) for _ in range(2)]
    for w, (q, sc) in zip((w1t, v1t), wq):          # [n = h, k = F]
        sp.QuantizeWeightMx(w, q, sc)
    dyq, dys = q8(rows, D_MODEL), u8(rows, D_MODEL // 32)
    dyqt, dyst = q8(D_MODEL, rows), u8(D_MODEL, rows // 32)
    sp.QuantizeTilesMx(dy, dyq, dys, dyqt, dyst)
    xqt, xst = q8(D_MODEL, rows), u8(D_MODEL, rows // 32)
    sp.QuantizeTilesMx(xp, qt=xqt, scales_t=xst)
    h, dg, du = images(), images(), images()
    sp.QuantizeBlocksMxGated(s, g.data, act, qt=h[2], scales_t=h[3])
    d = torch.empty_like(u.data)                    # D = dY W2^T
    sp.SddMx(dyq, dys, w2q_t, w2s_t, meta.descriptor(d))
    sp.QuantizeBlocksMxGatedGrad(meta.descriptor(d), g.data, u.data, act, dg,
                                 du)
    want_dx = torch.empty(rows, D_MODEL, dtype=td, device="cuda")
    sp.DsdMxPair(meta.descriptor(dg[0]), dg[1], *wq[0], du[0], du[1], *wq[1],
                 sp.Matrix(rows, D_MODEL, want_dx))
    assert _same(grads[0], want_dx)
    # dx against float64 of its own dequantised operands, the 2 K bound
    fwd = (topo.offsets.cpu().numpy(), topo.indices.cpu().numpy())
    bwd = (s.offsets_t.cpu().numpy(), s.indices_t.cpu().numpy())

    def product64(blocks, scales, m, k, order, bq, bs):
        a64 = R.decode(F.dense_from_blocks(m, k, *order, _bytes(blocks)),
                       R.expand_block_scales(m, k, *order,
                                             scales.cpu().numpy()))
        return R.matmul64(a64, R.decode(_bytes(bq), bs.cpu().numpy()))

    parts = [product64(img[0], img[1], rows, HIDDEN, fwd, *w)
             for img, w in ((dg, wq[0]), (du, wq[1]))]
    ref, absum = parts[0][0] + parts[1][0], parts[0][1] + parts[1][1]
    err = np.abs(_np(grads[0]).astype(np.float64) - ref)
    assert (err <= R.bound(ref, absum, 2 * HIDDEN, dtype)).all()
    # The three weight gradients: bits, then mx_grad_ref.bound.
    for name, got, img, bqt, bst in (("dw1t", grads[1], dg, xqt, xst),
                                     ("dv1t", grads[2], du, xqt, xst),
                                     ("dw2", grads[3], h, dyqt, dyst)):
        want = torch.empty(HIDDEN, D_MODEL, dtype=td, device="cuda")
        sp.DsdMxWgrad(st(img[2]), img[3], bqt, bst,
                      sp.Matrix(HIDDEN, D_MODEL, want))
        assert _same(got, want), name
        ref, absum = product64(img[2], img[3], HIDDEN, rows, bwd, bqt, bst)
        err = np.abs(_np(got).astype(np.float64) - ref)
        assert (err <= MG.bound(ref, absum, rows, dtype)).all(), name


@pytest.mark.parametrize("dtype", M.DTYPES)
def test_needs_input_grad_subsets_and_sinks(dtype):
    v1t, xp, w1t, w2, dy, topo, *_ = _inputs(dtype)
    td, args = xp.dtype, (xp, w1t, v1t, w2, dy, topo, "silu")
    y, full = _grads(*args)
    for need in ((True, False, False, False), (False, True, False, False),
                 (False, False, True, False), (False, False, False, True),
                 (True, False, True, True), (False,) * 4):
        y1, got = _grads(*args, need)
        assert _same(y, y1)
        for n, g, f in zip(need, got, full):
            assert (g is None) if not n else _same(g, f), need
    # Sinks: sink = round(acc + sink_before), acc the fp32 accumulator, which
    # an fp32 sink of zeros receives exactly (dsd_mx_wgrad with add).
    acc = [torch.zeros(HIDDEN, D_MODEL, device="cuda") for _ in range(3)]
    _, got = _grads(*args, (True, False, True, False), tuple(acc))
    assert got[1:] == [None] * 3 and _same(got[0], full[0])
    assert all(_same(a.to(td), f) for a, f in zip(acc, full[1:]))
    for sink_dtype in (torch.float32, td):
        before = [(torch.randn(HIDDEN, D_MODEL, device="cuda") / 8
                   ).to(sink_dtype) for _ in range(3)]
        sinks = [b.clone() for b in before]
        _grads(*args, sinks=tuple(sinks))
        for sink, b, a in zip(sinks, before, acc):
            assert _same(sink, (a + b.float()).to(sink_dtype))


@pytest.mark.parametrize("dtype", M.DTYPES)
def test_moe_glu_mlp_mx_train_gradients_reach_every_input(dtype):
    v1t, xp, w1t, w2, dy, topo, route, x, top, ew = _inputs(dtype)
    leaves = [t.detach().clone().requires_grad_()
              for t in (x, ew, w1t, v1t, w2)]
    out = ops.moe_glu_mlp_mx_train(leaves[0], top, *leaves[1:], EXPERTS)
    with torch.no_grad():       # forward: the inference layer, same weights
        q = [ops.quantize_weight_mx(w, transpose=True) for w in (w1t, v1t)]
        want = ops.moe_mlp_mx(x, top, ew, q[0], ops.quantize_weight_mx(w2),
                              EXPERTS, v1q=q[1])
    assert _same(out.detach(), want)
    out.backward(_dev(M.values(tuple(out.shape), dtype, [35]), dtype))
    for name, t in zip(("x", "expert_weights", "w1t", "v1t", "w2"), leaves):
        assert t.grad is not None and t.grad.shape == t.shape, name
        g = _np(t.grad)
        assert np.isfinite(g).all() and np.abs(g).max() > 0, name


@pytest.mark.parametrize("dtype", M.DTYPES)
def test_format_error_of_the_gradients_against_the_16_bit_glu_mlp(dtype):
    v1t, xp, w1t, w2, dy, topo, *_ = _inputs(dtype)
    ref = [t.detach().clone().requires_grad_() for t in (xp, w1t, v1t, w2)]
    ops.glu_mlp(ref[0], ref[1].t(), ref[2].t(), ref[3], topo,
                "silu").backward(dy)
    fp8 = [t.detach().clone().requires_grad_() for t in (xp, w1t, v1t, w2)]
    ops.glu_mlp_fp8(*fp8, topo, "silu", "fast", True).backward(dy)
    _, mx = _grads(xp, w1t, v1t, w2, dy, topo, "silu")

    def rel(g, r):
        return float(np.linalg.norm(_np(g) - _np(r.grad))
                     / np.linalg.norm(_np(r.grad)))
    errors = [(name, rel(g, r), rel(f.grad, r))
              for name, g, f, r in zip(NAMES, mx, fp8, ref)]
    for name, e_mx, e_fp8 in errors:
        print(f"vs glu_mlp {dtype}: {name} relative error glu_mlp_mx "
              f"{e_mx:.4f}, glu_mlp_fp8 pow2 fast {e_fp8:.4f}")
    for name, e_mx, e_fp8 in errors:
        assert e_mx <= 2 * e_fp8, (name, dtype, e_mx, e_fp8)
