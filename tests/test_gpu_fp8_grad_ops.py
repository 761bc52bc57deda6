"""GPU: the fp8 gradient ops of sputnik_amd/ops.py: mlp_fp8 and
moe_mlp_fp8_train, with quantize_tiles, quantize_sparse_t, Fp8Weight.t() and
dsd_fp8_wgrad underneath.

96 tokens, top_k 2, 4 experts, d_model 256, 128 ffn columns per expert, as
tests/test_gpu_fp8_ops.py. mlp_fp8's forward is held bit for bit against the
existing forward chain with quantize_weight of the same weights; each
backward stage bit for bit against the ctypes calls of fp8.h's table, and each
gradient against the float64 product of its own dequantised operands within
the header's bound. Sinks, needs_input_grad subsets, the three activations,
both dtypes and both accumulation modes; two runs give identical bits.

The error of the gradients against ops.mlp's on the same 16-bit inputs
measures the format, not the code: it is printed, and only a regression cap of
twice the recorded value (FORMAT_ERROR below) is asserted.
"""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import sputnik_amd as sp  # noqa: E402
from sputnik_amd import ops  # noqa: E402
from tests import fp8_fast_ref as FR  # noqa: E402
from tests import fp8_grad_ref as G  # noqa: E402
from tests import fp8_ref as R  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests import moe_ref as M  # noqa: E402

pytestmark = pytest.mark.gpu

TOKENS, TOP_K, EXPERTS, D_MODEL, FFN = 96, 2, 4, 256, 128
HIDDEN = EXPERTS * FFN
ACTS = ["relu", "gelu", "silu"]
MODES = ["fp32", "fast"]

# Relative 2-norm error of mlp_fp8's gradients against ops.mlp's on the same
# 16-bit inputs, as measured on an MI355X: per activation the largest over
# both dtypes and both modes (which agree to the fourth decimal) of dx, dw1t
# and dw2. The assertion is twice these. relu stands apart in dx and dw1t,
# which pass through act'(Z): its derivative is a step, and the fp8 forward's
# Z has the other sign than the 16-bit Z in a few percent of the elements
# near zero, where the whole of dH is gained or lost. dw2 = H^T dY does not
# see act' and agrees across the activations.
FORMAT_ERROR = {
    "relu": {"dx": 0.1629, "dw1t": 0.1634, "dw2": 0.0489},
    "gelu": {"dx": 0.0553, "dw1t": 0.0553, "dw2": 0.0500},
    "silu": {"dx": 0.0537, "dw1t": 0.0534, "dw2": 0.0503},
}


def _dev(a, dtype):
    return torch.from_numpy(np.array(a)).to(H.torch_dtype(dtype)).cuda()


def _np(t):
    return t.float().cpu().numpy()


def _bytes(t):
    return t.view(torch.uint8).cpu().numpy()


def _same(a, b):
    if a.dtype == torch.float32:
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


def _inputs(dtype):
    """(xp [T, h] padded, w1t [F, h], w2 [F, h], dy [T, h], topo, route, x,
    top, ew) on the device."""
    x = M.values((TOKENS, D_MODEL), dtype, [31])
    w1t = M.values((HIDDEN, D_MODEL), dtype, [32, 1]) / np.float32(16)
    w2 = M.values((HIDDEN, D_MODEL), dtype, [32, 2]) / np.float32(16)
    top = torch.from_numpy(M.routing(TOKENS, TOP_K, EXPERTS, "empty",
                                     seed=5)).cuda()
    ew = _dev(M.unit_weights(TOKENS * TOP_K, dtype, [33]).reshape(
        TOKENS, TOP_K), dtype)
    x = _dev(x, dtype)
    route = ops.moe_route(top, EXPERTS)
    xp = ops.padded_gather(x, route)
    topo = ops.expert_topology(route.padded_bins, FFN // 128,
                               route.rows // 128, dtype=x.dtype)
    dy = _dev(M.values((route.rows, D_MODEL), dtype, [34]), dtype)
    return xp, _dev(w1t, dtype), _dev(w2, dtype), dy, topo, route, x, top, ew


def _grads(xp, w1t, w2, dy, topo, act, mode, need=(True, True, True),
           sinks=(None, None)):
    leaves = [t.detach().clone().requires_grad_(n)
              for t, n in zip((xp, w1t, w2), need)]
    y = ops.mlp_fp8(*leaves, topo, act, mode, False, *sinks)
    if y.requires_grad:
        y.backward(dy)
    return y.detach(), [t.grad for t in leaves]


def _within(got, ref, absum, k, out, fast, what, wgrad=True):
    """Within the header's bound: DsdFp8Wgrad's, or with `wgrad` false
    DsdFp8's (fp8_ref.bound, fp8_fast_ref.bound_fast)."""
    err = np.abs(got.astype(np.float64) - ref)
    if wgrad:
        lim = G.bound(ref, absum, k, out, fast)
    else:
        lim = (FR.bound_fast if fast else R.bound)(ref, absum, k, out)
    worst = float((err / np.maximum(lim, 1e-300)).max())
    print(f"{what}: worst error / bound = {worst:.3f}")
    assert (err <= lim).all(), (what, worst)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("dtype", M.DTYPES)
def test_mlp_fp8_forward_and_every_backward_stage(dtype, act, mode):
    xp, w1t, w2, dy, topo, route, *_ = _inputs(dtype)
    td, fast = xp.dtype, mode == "fast"
    rows = route.rows
    y, (dx, dw1t, dw2) = _grads(xp, w1t, w2, dy, topo, act, mode)

    # Forward: the existing chain with quantize_weight of the same weights.
    w1q = ops.quantize_weight(w1t, transpose=True)
    w2q = ops.quantize_weight(w2)
    assert w1q.shape == (D_MODEL, HIDDEN) and w2q.shape == (HIDDEN, D_MODEL)
    xq, xs = ops.quantize_rows(xp)
    z = ops.sdd_fp8(xq, xs, w1q, topo, td, mode)
    assert _same(y, ops.dsd_fp8(ops.quantize_sparse(z, act), w2q, td, mode))

    # Backward, stage by stage through the bindings of the C ABI.
    nb = topo.nnz_blocks
    e4m3, dev = torch.float8_e4m3fn, "cuda"
    topo._meta.ensure_transposed(z.data)
    topo._meta.ensure_row_indices(z.data)
    s = topo._meta.descriptor(z.data)
    st = lambda data: sp.BlockMatrix(                          # noqa: E731
        HIDDEN, rows, 128, nb * 128 * 128, data, s.offsets_t, s.indices_t)
    # the weights' backward layouts: exact transposes
    w2q_t, w1q_t = w2q.t(), w1q.t()
    for wt, again in ((w2q_t, ops.quantize_weight(w2, transpose=True)),
                      (w1q_t, ops.quantize_weight(w1t))):
        assert wt.shape == again.shape
        assert torch.equal(wt.q.view(torch.uint8), again.q.view(torch.uint8))
        assert torch.equal(wt.scales, again.scales)
    # dY along both axes, X along the columns
    dyq = torch.empty(rows, D_MODEL, dtype=e4m3, device=dev)
    dys = torch.empty(rows, D_MODEL // 128, device=dev)
    dyqt = torch.empty(D_MODEL, rows, dtype=e4m3, device=dev)
    dyst = torch.empty(rows // 128, D_MODEL, device=dev)
    sp.QuantizeTiles(dy, dyq, dys, dyqt, dyst)
    xqt = torch.empty(D_MODEL, rows, dtype=e4m3, device=dev)
    xst = torch.empty(rows // 128, D_MODEL, device=dev)
    sp.QuantizeTiles(xp, qt=xqt, scales_t=xst)
    # dW2 = H^T dY
    hqt = torch.empty(nb, 128, 128, dtype=e4m3, device=dev)
    hst = torch.empty(nb * 128, device=dev)
    sp.QuantizeBlocks(s, qt=hqt, scales_t=hst, stage="act", activation=act)
    want_dw2 = torch.empty(HIDDEN, D_MODEL, dtype=td, device=dev)
    sp.DsdFp8Wgrad(st(hqt), hst, dyqt, dyst,
                   sp.Matrix(HIDDEN, D_MODEL, want_dw2), accumulate=mode)
    assert _same(dw2, want_dw2)
    # dH = dY W2^T at the blocks, dZ = dH * act'(Z) along both axes
    dh = torch.empty(nb, 128, 128, dtype=td, device=dev)
    sp.SddFp8(dyq, dys, w2q_t.q, w2q_t.scales, topo._meta.descriptor(dh),
              accumulate=mode)
    dzq = torch.empty(nb, 128, 128, dtype=e4m3, device=dev)
    dzs = torch.empty(nb * 128, device=dev)
    dzqt = torch.empty(nb, 128, 128, dtype=e4m3, device=dev)
    dzst = torch.empty(nb * 128, device=dev)
    sp.QuantizeBlocks(topo._meta.descriptor(dh), dzq, dzs, dzqt, dzst,
                      stage="act_grad", activation=act, z=z.data)
    # dX = dZ W1t, dW1t = dZ^T X
    want_dx = torch.empty(rows, D_MODEL, dtype=td, device=dev)
    sp.DsdFp8(topo._meta.descriptor(dzq), dzs, w1q_t.q, w1q_t.scales,
              sp.Matrix(rows, D_MODEL, want_dx), accumulate=mode)
    assert _same(dx, want_dx)
    want_dw1 = torch.empty(HIDDEN, D_MODEL, dtype=td, device=dev)
    sp.DsdFp8Wgrad(st(dzqt), dzst, xqt, xst,
                   sp.Matrix(HIDDEN, D_MODEL, want_dw1), accumulate=mode)
    assert _same(dw1t, want_dw1)

    # Each gradient against the float64 product of its own dequantised
    # operands (fp8_ref.bound for the DSD, fp8_grad_ref.bound for the two
    # column-scaled products; in kFast with eps_fast).
    offsets, indices = topo.offsets.cpu().numpy(), topo.indices.cpu().numpy()
    o_t, i_t = s.offsets_t.cpu().numpy(), s.indices_t.cpu().numpy()

    def sparse64(blocks, scales, m, k, off, idx):
        return R.dequantize_rows(
            R.dense_from_blocks(m, k, off, idx, _bytes(blocks)),
            R.expand_block_scales(m, k, off, idx, scales.cpu().numpy()))

    ref, absum = R.matmul64(
        sparse64(dzq, dzs, rows, HIDDEN, offsets, indices),
        R.dequantize_weight(_bytes(w1q_t.q), w1q_t.scales.cpu().numpy()))
    _within(_np(dx), ref, absum, HIDDEN, dtype, fast, f"dx {dtype} {act}",
            wgrad=False)
    for name, got, blocks, scales, bqt, bst in (
            ("dw2", dw2, hqt, hst, dyqt, dyst),
            ("dw1t", dw1t, dzqt, dzst, xqt, xst)):
        ref, absum = R.matmul64(
            sparse64(blocks, scales, HIDDEN, rows, o_t, i_t),
            G.dequantize_cols(_bytes(bqt), bst.cpu().numpy()))
        _within(_np(got), ref, absum, rows, dtype, fast,
                f"{name} {dtype} {act}")

    # Two runs give identical bits.
    y2, (dx2, dw1t2, dw22) = _grads(xp, w1t, w2, dy, topo, act, mode)
    assert _same(y, y2) and _same(dx, dx2)
    assert _same(dw1t, dw1t2) and _same(dw2, dw22)


@pytest.mark.parametrize("dtype", M.DTYPES)
def test_needs_input_grad_subsets_and_sinks(dtype):
    xp, w1t, w2, dy, topo, *_ = _inputs(dtype)
    td = xp.dtype
    y, full = _grads(xp, w1t, w2, dy, topo, "gelu", "fp32")
    for need in ((True, False, False), (False, True, False),
                 (False, False, True), (True, False, True),
                 (False, True, True)):
        y1, got = _grads(xp, w1t, w2, dy, topo, "gelu", "fp32", need)
        assert _same(y, y1)
        for n, g, f in zip(need, got, full):
            assert (g is None) if not n else _same(g, f), need
    y0, none = _grads(xp, w1t, w2, dy, topo, "gelu", "fp32",
                      (False, False, False))
    assert _same(y, y0) and not y0.requires_grad and none == [None] * 3

    # Sinks: sink = round(acc + sink_before), acc the fp32 accumulator, which
    # an fp32 sink of zeros receives exactly.
    acc = [torch.zeros(HIDDEN, D_MODEL, device="cuda") for _ in range(2)]
    _, got = _grads(xp, w1t, w2, dy, topo, "gelu", "fp32", sinks=tuple(acc))
    assert got[1] is None and got[2] is None and _same(got[0], full[0])
    for a, f in zip(acc, full[1:]):
        assert _same(a.to(td), f)       # the gradient is round_T(acc)
    for sink_dtype in (torch.float32, td):
        before = [(torch.randn(HIDDEN, D_MODEL, device="cuda") / 8
                   ).to(sink_dtype) for _ in range(2)]
        sinks = [b.clone() for b in before]
        _grads(xp, w1t, w2, dy, topo, "gelu", "fp32", sinks=tuple(sinks))
        for sink, b, a in zip(sinks, before, acc):
            assert _same(sink, (a + b.float()).to(sink_dtype))
    # a sink for one weight only, that weight itself not requiring grad, and
    # no gradient asked of the other
    only = torch.zeros(HIDDEN, D_MODEL, device="cuda")
    _, got = _grads(xp, w1t, w2, dy, topo, "gelu", "fp32",
                    (True, False, False), (None, only))
    assert got[1] is None and got[2] is None and _same(got[0], full[0])
    assert _same(only, acc[1])


@pytest.mark.parametrize("dtype", M.DTYPES)
def test_low_level_ops(dtype):
    xp, w1t, w2, dy, topo, *_ = _inputs(dtype)
    q, s, qt, st = ops.quantize_tiles(xp)
    q0, s0 = ops.quantize_rows(xp)
    assert torch.equal(q.view(torch.uint8), q0.view(torch.uint8))
    assert torch.equal(s, s0)
    qt_ref, st_ref = G.quantize_cols(_np(xp))
    assert np.array_equal(_bytes(qt), qt_ref)
    assert np.array_equal(st.cpu().numpy(), st_ref)
    assert ops.quantize_tiles(xp, rows=False)[:2] == (None, None)
    z = ops.sdd_fp8(q, s, ops.quantize_weight(w1t, transpose=True), topo,
                    xp.dtype)
    ht = ops.quantize_sparse_t(z, "gelu")
    assert ht.shape == (HIDDEN, xp.shape[0])
    h = sp.BlockActivation(z.data, "gelu")
    _, _, b_o = G.transposed_order(topo.offsets.cpu().numpy(),
                                   topo.indices.cpu().numpy(), HIDDEN // 128)
    q_ref, s_ref = G.quantize_blocks_t(_np(h), b_o)
    assert np.array_equal(_bytes(ht.data), q_ref)
    assert np.array_equal(ht.scales.cpu().numpy(), s_ref)
    _, _, dyqt, dyst = ops.quantize_tiles(dy, rows=False)
    out = ops.dsd_fp8_wgrad(ht, dyqt, dyst, out_dtype=torch.float32)
    assert out.dtype == torch.float32
    again = torch.zeros_like(out)
    ops.dsd_fp8_wgrad(ht, dyqt, dyst, again, add=True)
    assert _same(out, again)
    with pytest.raises(ValueError):
        ops.dsd_fp8_wgrad(ht, dyqt, dyst, add=True)
    with pytest.raises(ValueError):
        ops.mlp_fp8(xp, w1t[:, :128], w2, topo)
    with pytest.raises(ValueError):
        ops.mlp_fp8(xp, w1t, w2, topo, accumulate="fp16")
    with pytest.raises(TypeError):
        ops.dsd_fp8_wgrad(z, dyqt, dyst)


@pytest.mark.parametrize("dtype", M.DTYPES)
def test_moe_mlp_fp8_train_gradients_reach_every_input(dtype):
    xp, w1t, w2, dy, topo, route, x, top, ew = _inputs(dtype)
    leaves = [t.detach().clone().requires_grad_() for t in (x, ew, w1t, w2)]
    out = ops.moe_mlp_fp8_train(leaves[0], top, leaves[1], leaves[2],
                                leaves[3], EXPERTS)
    assert out.dtype == x.dtype and tuple(out.shape) == (TOKENS, D_MODEL)
    # forward: the inference layer on the same weights
    with torch.no_grad():
        want = ops.moe_mlp_fp8(x, top, ew,
                               ops.quantize_weight(w1t, transpose=True),
                               ops.quantize_weight(w2), EXPERTS)
    assert _same(out.detach(), want)
    dout = _dev(M.values((TOKENS, D_MODEL), dtype, [35]), dtype)
    out.backward(dout)
    ref = [t.detach().clone().requires_grad_() for t in (x, ew, w1t, w2)]
    ops.moe_mlp(ref[0], top, ref[1], ref[2].t(), ref[3], EXPERTS,
                activation="gelu").backward(dout)
    for name, t, r in zip(("x", "expert_weights", "w1t", "w2"), leaves, ref):
        assert t.grad is not None and t.grad.shape == t.shape, name
        g, g16 = _np(t.grad), _np(r.grad)
        assert np.isfinite(g).all() and np.abs(g).max() > 0, name
        rel = float(np.linalg.norm(g - g16) / np.linalg.norm(g16))
        print(f"moe_mlp_fp8_train vs moe_mlp {dtype}: d{name} relative "
              f"error {rel:.4f}")
    # a route built beforehand, and sinks
    sink = torch.zeros(HIDDEN, D_MODEL, device="cuda")
    again = [t.detach().clone().requires_grad_() for t in (x, ew)]
    ops.moe_mlp_fp8_train(again[0], route, again[1], w1t, w2, EXPERTS,
                          w2_grad_out=sink).backward(dout)
    assert _same(again[0].grad, leaves[0].grad)
    assert _same(sink.to(x.dtype), leaves[3].grad)


@pytest.mark.parametrize("dtype", M.DTYPES)
def test_format_error_of_the_gradients_against_the_16_bit_mlp(dtype):
    xp, w1t, w2, dy, topo, *_ = _inputs(dtype)
    for act in ACTS:
        ref = [t.detach().clone().requires_grad_() for t in (xp, w1t, w2)]
        ops.mlp(ref[0], ref[1].t(), ref[2], topo, act).backward(dy)
        for mode in MODES:
            _, got = _grads(xp, w1t, w2, dy, topo, act, mode)
            for name, g, r in zip(("dx", "dw1t", "dw2"), got, ref):
                g16 = _np(r.grad)
                rel = float(np.linalg.norm(_np(g) - g16)
                            / np.linalg.norm(g16))
                print(f"mlp_fp8 vs mlp {dtype} {act} {mode}: {name} relative "
                      f"error {rel:.4f}")
                assert rel <= 2 * FORMAT_ERROR[act][name], (
                    name, dtype, act, mode, rel)
