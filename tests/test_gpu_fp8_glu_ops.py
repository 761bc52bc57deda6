"""GPU: DsdFp8Pair and the fp8 GLU ops (ops.glu_mlp_fp8,
ops.moe_glu_mlp_fp8_train) on the shapes and helpers of
tests/test_gpu_fp8_grad_ops.py: bit for bit against DsdFp8 on concatenated
operands, the existing forward chain and the ctypes calls of fp8.h's gated
table; within the header's bounds of the float64 products. The error against
ops.glu_mlp measures the format, not the code: printed, and capped at twice
the recorded value (FORMAT_ERROR)."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import sputnik_amd as sp  # noqa: E402
from sputnik_amd import ops  # noqa: E402
from tests import fp8_grad_ref as G  # noqa: E402
from tests import fp8_ref as R  # noqa: E402
from tests import moe_ref as M  # noqa: E402
from tests import test_gpu_fp8 as T  # noqa: E402
from tests import test_gpu_fp8_grad_ops as P  # noqa: E402

pytestmark = pytest.mark.gpu

EXPERTS, D_MODEL, HIDDEN = P.EXPERTS, P.D_MODEL, P.HIDDEN
NAMES = ("dx", "dw1t", "dv1t", "dw2")

# Relative 2-norm error of glu_mlp_fp8's gradients (silu) against
# ops.glu_mlp's on the same 16-bit inputs, as measured on an MI355X: the
# largest over both dtypes and both modes (which agree to the fourth decimal;
# fp16 gave 0.0636, 0.0632, 0.0584, 0.0599). The assertion is twice these.
FORMAT_ERROR = {"dx": 0.0638, "dw1t": 0.0632, "dv1t": 0.0603, "dw2": 0.0607}


def _pair_operands(dtype, seed):
    """(sq, ss, wq, sw) of one pair on DSD_DEEP_TOPOLOGY, quantised values."""
    nb = len(R.DSD_DEEP_TOPOLOGY[1])
    blocks = M.values((nb, 128, 128), dtype, [71, seed, 1])
    w = M.values((R.DSD_DEEP_K, R.DSD_DEEP_N), dtype, [71, seed, 2])
    return R.quantize_sparse(blocks) + R.quantize_weight(w)


def _dsd(offsets, indices, k, sq, ss, wq, sw, dtype, mode, second=None):
    """DsdFp8 or, with `second` = (sq, ss, wq, sw), DsdFp8Pair: C."""
    m, n = R.DSD_DEEP_M, R.DSD_DEEP_N
    out = torch.full((m, n), 3.0, dtype=P.H.torch_dtype(dtype), device="cuda")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    s = sp.BlockMatrix(m, k, 128, len(indices) * 128 * 128, T.dev_bytes(sq),
                       dev(offsets), dev(indices))
    args = [s, dev(ss), T.dev_bytes(wq), dev(sw)]
    if second is None:
        sp.DsdFp8(*args, sp.Matrix(m, n, out), accumulate=mode)
    else:
        sq2, ss2, wq2, sw2 = second
        sp.DsdFp8Pair(*args, T.dev_bytes(sq2), dev(ss2), T.dev_bytes(wq2),
                      dev(sw2), sp.Matrix(m, n, out), accumulate=mode)
    return out


def _product64(pairs, m, k, offsets, indices):
    """(sum of the pairs' float64 products, sum of |a| |w|): a pair is
    (blocks, block scales, weight bytes [n, k], weight scales) in numpy."""
    ref = absum = 0.0
    for sq, ss, wq, sw in pairs:
        a64 = R.dequantize_rows(R.dense_from_blocks(m, k, offsets, indices, sq),
                                R.expand_block_scales(m, k, offsets, indices, ss))
        r, a = R.matmul64(a64, R.dequantize_weight(wq, sw))
        ref, absum = ref + r, absum + a
    return ref, absum


@pytest.mark.parametrize("mode", P.MODES)
@pytest.mark.parametrize("dtype", M.DTYPES)
def test_dsd_fp8_pair(dtype, mode):
    offsets, indices = R.DSD_DEEP_TOPOLOGY
    m, k, kb = R.DSD_DEEP_M, R.DSD_DEEP_K, R.DSD_DEEP_K // 128
    one, two = _pair_operands(dtype, 1), _pair_operands(dtype, 2)
    got = _dsd(offsets, indices, k, *one, dtype, mode, two)
    # (a) DsdFp8 over [S1 | S2] . [B1; B2]: per block row its blocks twice,
    # the second time from pair 2 with the indices shifted by k / 128
    rows = R.row_indices(offsets)
    order = np.concatenate([np.tile(np.flatnonzero(rows == r), 2)
                            for r in range(m // 128)])
    second = np.concatenate([np.repeat([False, True], (rows == r).sum())
                             for r in range(m // 128)])

    def concatenated(idx):
        sq = np.where(second[:, None, None], two[0][order], one[0][order])
        ss = np.where(second[:, None], two[1].reshape(-1, 128)[order],
                      one[1].reshape(-1, 128)[order]).reshape(-1)
        cat = (idx[order] + kb * second).astype(np.int16)
        return _dsd(2 * offsets, cat, 2 * k, sq, ss,
                    np.concatenate([one[2], two[2]], axis=1),
                    np.concatenate([one[3], two[3]], axis=0), dtype, mode)

    assert P._same(got, concatenated(indices))
    # (b) the float64 product of the dequantised operands, 2 K bound
    ref, absum = _product64((one, two), m, k, offsets, indices)
    P._within(P._np(got), ref, absum, 2 * k, dtype, mode == "fast",
              f"pair {dtype} {mode}", wgrad=False)
    # (c) an index out of range contributes zero in both pairs (4 * kb is out
    # of range for the concatenated product too)
    broken = indices.copy()
    broken[7] = 4 * kb
    skipped = _dsd(offsets, broken, k, *one, dtype, mode, two)
    assert P._same(skipped, concatenated(broken))
    assert not P._same(skipped, got)
    # (d) the empty block row is +0, (e) a second run gives the same bits
    assert not got[128:256].view(torch.int16).any()
    assert P._same(got, _dsd(offsets, indices, k, *one, dtype, mode, two))


def _inputs(dtype):
    """test_gpu_fp8_grad_ops' inputs with v1t in front."""
    v1t = M.values((HIDDEN, D_MODEL), dtype, [32, 3]) / np.float32(16)
    return (P._dev(v1t, dtype),) + P._inputs(dtype)


def _grads(xp, w1t, v1t, w2, dy, topo, act, mode, need=(True,) * 4,
           sinks=(None,) * 3):
    leaves = [t.detach().clone().requires_grad_(n)
              for t, n in zip((xp, w1t, v1t, w2), need)]
    y = ops.glu_mlp_fp8(*leaves, topo, act, mode, False, *sinks)
    if y.requires_grad:
        y.backward(dy)
    return y.detach(), [t.grad for t in leaves]


@pytest.mark.parametrize("mode", P.MODES)
@pytest.mark.parametrize("act", P.ACTS)
@pytest.mark.parametrize("dtype", M.DTYPES)
def test_glu_mlp_fp8_forward_and_every_backward_stage(dtype, act, mode):
    v1t, xp, w1t, w2, dy, topo, route, *_ = _inputs(dtype)
    td, fast, rows, nb = xp.dtype, mode == "fast", route.rows, topo.nnz_blocks
    y, grads = _grads(xp, w1t, v1t, w2, dy, topo, act, mode)
    # Forward: the existing chain with quantize_weight of the same weights.
    w1q, v1q = (ops.quantize_weight(w, transpose=True) for w in (w1t, v1t))
    w2q = ops.quantize_weight(w2)
    xq, xs = ops.quantize_rows(xp)
    g = ops.sdd_fp8(xq, xs, w1q, topo, td, mode)
    u = ops.sdd_fp8(xq, xs, v1q, topo, td, mode)
    assert P._same(y, ops.dsd_fp8(ops.quantize_sparse(u, act, gate=g), w2q,
                                  td, mode))
    # Backward, stage by stage through the bindings of the C ABI.
    meta = topo._meta
    meta.ensure_transposed(u.data)
    meta.ensure_row_indices(u.data)
    s = meta.descriptor(u.data)
    images = lambda: ops._lowp_images(      # noqa: E731
        ops._FP8, nb, True, True, "cuda")
    dense = lambda: torch.empty(rows, D_MODEL, dtype=td, device="cuda")  # noqa: E731
    w2q_t, w1q_t, v1q_t = w2q.t(), w1q.t(), v1q.t()
    dyq, dys, dyqt, dyst = ops.quantize_tiles(dy)
    _, _, xqt, xst = ops.quantize_tiles(xp, rows=False)
    h, dg, du = images(), images(), images()
    sp.QuantizeBlocksGated(s, g.data, act, qt=h[2], scales_t=h[3])
    d = torch.empty_like(u.data)                 # D = dY W2^T at the blocks
    sp.SddFp8(dyq, dys, w2q_t.q, w2q_t.scales, meta.descriptor(d),
              accumulate=mode)
    sp.QuantizeBlocksGatedGrad(meta.descriptor(d), g.data, u.data, act, dg, du)
    want_dx = dense()                            # dG W1t + dU V1t
    sp.DsdFp8Pair(meta.descriptor(dg[0]), dg[1], w1q_t.q, w1q_t.scales, du[0],
                  du[1], v1q_t.q, v1q_t.scales,
                  sp.Matrix(rows, D_MODEL, want_dx), accumulate=mode)
    assert P._same(grads[0], want_dx)
    # dx against the float64 product of its own operands, the 2 K bound
    host = lambda *ts: [t.view(torch.uint8).cpu().numpy()      # noqa: E731
                        if t.dtype == torch.float8_e4m3fn
                        else t.cpu().numpy() for t in ts]
    ref, absum = _product64(
        (host(dg[0], dg[1], w1q_t.q, w1q_t.scales),
         host(du[0], du[1], v1q_t.q, v1q_t.scales)), rows, HIDDEN,
        topo.offsets.cpu().numpy(), topo.indices.cpu().numpy())
    P._within(P._np(grads[0]), ref, absum, 2 * HIDDEN, dtype, fast,
              f"dx {dtype} {act}", wgrad=False)
    # The three weight gradients: bits, then fp8_grad_ref.bound.
    o_t, i_t = s.offsets_t.cpu().numpy(), s.indices_t.cpu().numpy()
    for name, got, img, bqt, bst in (("dw1t", grads[1], dg, xqt, xst),
                                     ("dv1t", grads[2], du, xqt, xst),
                                     ("dw2", grads[3], h, dyqt, dyst)):
        want = torch.empty(HIDDEN, D_MODEL, dtype=td, device="cuda")
        sp.DsdFp8Wgrad(sp.BlockMatrix(HIDDEN, rows, 128, nb * 128 * 128,
                                      img[2], s.offsets_t, s.indices_t),
                       img[3], bqt, bst, sp.Matrix(HIDDEN, D_MODEL, want),
                       accumulate=mode)
        assert P._same(got, want), name
        sq, ss, bq, bs = host(img[2], img[3], bqt, bst)
        ref, absum = R.matmul64(
            R.dequantize_rows(
                R.dense_from_blocks(HIDDEN, rows, o_t, i_t, sq),
                R.expand_block_scales(HIDDEN, rows, o_t, i_t, ss)),
            G.dequantize_cols(bq, bs))
        P._within(P._np(got), ref, absum, rows, dtype, fast,
                  f"{name} {dtype} {act}")
    # Two runs give identical bits.
    y2, again = _grads(xp, w1t, v1t, w2, dy, topo, act, mode)
    assert P._same(y, y2)
    assert all(P._same(a, b) for a, b in zip(grads, again))


@pytest.mark.parametrize("dtype", M.DTYPES)
def test_needs_input_grad_subsets_and_sinks(dtype):
    v1t, xp, w1t, w2, dy, topo, *_ = _inputs(dtype)
    td, args = xp.dtype, (xp, w1t, v1t, w2, dy, topo, "silu", "fp32")
    y, full = _grads(*args)
    for need in ((True, False, False, False), (False, True, False, False),
                 (False, False, True, False), (False, False, False, True),
                 (True, False, True, True), (False,) * 4):
        y1, got = _grads(*args, need)
        assert P._same(y, y1)
        for n, g, f in zip(need, got, full):
            assert (g is None) if not n else P._same(g, f), need
    # Sinks: sink = round(acc + sink_before), acc the fp32 accumulator, which
    # an fp32 sink of zeros receives exactly (dsd_fp8_wgrad with add).
    acc = [torch.zeros(HIDDEN, D_MODEL, device="cuda") for _ in range(3)]
    _, got = _grads(*args, (True, False, True, False), tuple(acc))
    assert got[1:] == [None] * 3 and P._same(got[0], full[0])
    for a, f in zip(acc, full[1:]):
        assert P._same(a.to(td), f)
    for sink_dtype in (torch.float32, td):
        before = [(torch.randn(HIDDEN, D_MODEL, device="cuda") / 8
                   ).to(sink_dtype) for _ in range(3)]
        sinks = [b.clone() for b in before]
        _grads(*args, sinks=tuple(sinks))
        for sink, b, a in zip(sinks, before, acc):
            assert P._same(sink, (a + b.float()).to(sink_dtype))


@pytest.mark.parametrize("dtype", M.DTYPES)
def test_moe_glu_mlp_fp8_train_gradients_reach_every_input(dtype):
    v1t, xp, w1t, w2, dy, topo, route, x, top, ew = _inputs(dtype)
    leaves = [t.detach().clone().requires_grad_()
              for t in (x, ew, w1t, v1t, w2)]
    out = ops.moe_glu_mlp_fp8_train(leaves[0], top, *leaves[1:], EXPERTS)
    with torch.no_grad():
        q = [ops.quantize_weight(w, transpose=True) for w in (w1t, v1t)]
        want = ops.moe_mlp_fp8(x, top, ew, q[0], ops.quantize_weight(w2),
                               EXPERTS, v1q=q[1])
    assert P._same(out.detach(), want)
    out.backward(P._dev(M.values(tuple(out.shape), dtype, [35]), dtype))
    for name, t in zip(("x", "expert_weights", "w1t", "v1t", "w2"), leaves):
        assert t.grad is not None and t.grad.shape == t.shape, name
        g = P._np(t.grad)
        assert np.isfinite(g).all() and np.abs(g).max() > 0, name


@pytest.mark.parametrize("dtype", M.DTYPES)
def test_format_error_of_the_gradients_against_the_16_bit_glu_mlp(dtype):
    v1t, xp, w1t, w2, dy, topo, *_ = _inputs(dtype)
    ref = [t.detach().clone().requires_grad_() for t in (xp, w1t, v1t, w2)]
    ops.glu_mlp(ref[0], ref[1].t(), ref[2].t(), ref[3], topo,
                "silu").backward(dy)
    measured = []
    for mode in P.MODES:
        _, got = _grads(xp, w1t, v1t, w2, dy, topo, "silu", mode)
        for name, g, r in zip(NAMES, got, ref):
            g16 = P._np(r.grad)
            rel = float(np.linalg.norm(P._np(g) - g16) / np.linalg.norm(g16))
            print(f"glu_mlp_fp8 vs glu_mlp {dtype} {mode}: {name} relative "
                  f"error {rel:.4f}")
            measured.append((name, mode, rel))
    for name, mode, rel in measured:
        assert rel <= 2 * FORMAT_ERROR[name], (name, dtype, mode, rel)
