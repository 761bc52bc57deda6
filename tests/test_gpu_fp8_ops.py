"""GPU: the fp8 ops of sputnik_amd/ops.py: quantize_rows / quantize_sparse /
quantize_weight, sdd_fp8, dsd_fp8 and moe_mlp_fp8.

moe_mlp_fp8 is held, bit for bit, against the same chain called op by op, and
every stage of that chain against tests/fp8_ref.py from the GPU's own stage
inputs: the quantisers exactly, the products by fp8_ref.bound. The H a fused
quantiser sees is the one the 16-bit elementwise kernel stores from the same
block values (BlockActivation / BlockGate). The error of the whole layer
against ops.moe_mlp on the unquantised weights is printed, not asserted: it
measures the format, not the code (DESIGN has the figures).
"""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import sputnik_amd as sp  # noqa: E402
from sputnik_amd import ops  # noqa: E402
from tests import fp8_ref as R  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests import moe_ref as M  # noqa: E402
from tests import rounding_ref as RR  # noqa: E402

pytestmark = pytest.mark.gpu

TOKENS, TOP_K, EXPERTS, D_MODEL = 96, 2, 4, 256


def _dev(a, dtype):
    return torch.from_numpy(np.array(a)).to(H.torch_dtype(dtype)).cuda()


def _np(t):
    return t.float().cpu().numpy()


def _bytes(t):
    return t.view(torch.uint8).cpu().numpy()


def _same(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


def _inputs(dtype, ffn, glu):
    hidden = EXPERTS * ffn
    x = M.values((TOKENS, D_MODEL), dtype, [21, ffn])
    # (weights of about 1 / 16, so the layer's values stay of order one)
    ws = [M.values(shape, dtype, [22, i, ffn]) / np.float32(16)
          for i, shape in enumerate([(D_MODEL, hidden), (hidden, D_MODEL),
                                     (D_MODEL, hidden)])]
    top = M.routing(TOKENS, TOP_K, EXPERTS, "empty", seed=5)
    ew = M.unit_weights(TOKENS * TOP_K, dtype, [23]).reshape(TOKENS, TOP_K)
    w1, w2, v1 = (_dev(w, dtype) for w in ws)
    return (_dev(x, dtype), torch.from_numpy(top).cuda(), _dev(ew, dtype),
            w1, w2, v1 if glu else None)


def _within(got, ref, absum, k, dtype, what):
    err = np.abs(got.astype(np.float64) - ref)
    lim = R.bound(ref, absum, k, dtype)
    worst = float((err / np.maximum(lim, 1e-300)).max()) if err.size else 0.0
    print(f"{what}: worst error / bound = {worst:.3f}")
    assert (err <= lim).all(), (what, worst)


@pytest.mark.parametrize("explicit_rows", [False, True], ids=["exact", "bound"])
# (ffn 384: 3 DSD steps per expert row, past the ring's two stages)
@pytest.mark.parametrize("ffn", [128, 256, 384])
@pytest.mark.parametrize("glu", [False, True], ids=["gelu-mlp", "silu-glu"])
@pytest.mark.parametrize("dtype", M.DTYPES)
def test_moe_mlp_fp8_equals_its_chain_and_every_stage_its_reference(
        dtype, glu, ffn, explicit_rows):
    x, top, ew, w1, w2, v1 = _inputs(dtype, ffn, glu)
    hidden = EXPERTS * ffn
    td = x.dtype
    rows = (ops.moe_rows_bound(TOKENS * TOP_K, EXPERTS) if explicit_rows
            else None)
    w1q, w2q = ops.quantize_weight(w1), ops.quantize_weight(w2)
    v1q = ops.quantize_weight(v1) if glu else None
    for w, wq in ((w1, w1q), (w2, w2q)) + (((v1, v1q),) if glu else ()):
        q_ref, s_ref = R.quantize_weight(_np(w))
        assert np.array_equal(_bytes(wq.q), q_ref)
        assert np.array_equal(wq.scales.cpu().numpy(), s_ref)
        # ... and the transposed source gives the same Fp8Weight
        wt = ops.quantize_weight(w.t().contiguous(), transpose=True)
        assert torch.equal(wt.q.view(torch.uint8), wq.q.view(torch.uint8))
        assert torch.equal(wt.scales, wq.scales) and wt.shape == wq.shape

    out = ops.moe_mlp_fp8(x, top, ew, w1q, w2q, EXPERTS, v1q=v1q, rows=rows)
    assert out.dtype == td and tuple(out.shape) == (TOKENS, D_MODEL)
    assert not out.requires_grad

    # The chain, op by op.
    act = "silu" if glu else "gelu"
    route = ops.moe_route(top, EXPERTS, rows)
    xp = ops.padded_gather(x, route)
    topo = ops.expert_topology(route.padded_bins, ffn // 128,
                               route.rows // 128, dtype=td)
    xq, xs = ops.quantize_rows(xp)
    g = ops.sdd_fp8(xq, xs, w1q, topo, td)
    u = ops.sdd_fp8(xq, xs, v1q, topo, td) if glu else None
    hq = (ops.quantize_sparse(u, act, gate=g) if glu
          else ops.quantize_sparse(g, act))
    y = ops.dsd_fp8(hq, w2q, td)
    chain = ops.padded_scatter(y, route, ew)
    assert _same(out, chain)
    # ... and through a route built beforehand
    assert _same(out, ops.moe_mlp_fp8(x, route, ew, w1q, w2q, EXPERTS,
                                      v1q=v1q))

    # Stage by stage, from the GPU's own stage inputs.
    offsets, indices = topo.offsets.cpu().numpy(), topo.indices.cpu().numpy()
    q_ref, s_ref = R.quantize_rows(_np(xp))
    assert np.array_equal(_bytes(xq), q_ref)
    assert np.array_equal(xs.cpu().numpy(), s_ref)
    a64 = R.dequantize_rows(_bytes(xq), xs.cpu().numpy())
    for name, prod, wq in (("sdd w1", g, w1q),) + (
            (("sdd v1", u, v1q),) if glu else ()):
        ref, absum = R.matmul64(a64, R.dequantize_weight(
            _bytes(wq.q), wq.scales.cpu().numpy()))
        _within(_np(prod.data), R.blocks_from_dense(ref, offsets, indices),
                R.blocks_from_dense(absum, offsets, indices), D_MODEL, dtype,
                f"{name} {dtype}")
    h16 = (sp.BlockGate(u.data, g.data, act) if glu
           else sp.BlockActivation(g.data, act))
    q_ref, s_ref = R.quantize_sparse(_np(h16))
    assert np.array_equal(_bytes(hq.data), q_ref)
    assert np.array_equal(hq.scales.cpu().numpy(), s_ref)
    h64 = R.dequantize_rows(
        R.dense_from_blocks(route.rows, hidden, offsets, indices,
                            _bytes(hq.data)),
        R.expand_block_scales(route.rows, hidden, offsets, indices,
                              hq.scales.cpu().numpy()))
    ref, absum = R.matmul64(h64, R.dequantize_weight(
        _bytes(w2q.q), w2q.scales.cpu().numpy()))
    _within(_np(y), ref, absum, hidden, dtype, f"dsd w2 {dtype}")

    # Padding rows stay +0 through the chain.
    pad = np.ones(route.rows, dtype=bool)
    pad[route.row_of.cpu().numpy()] = False
    assert pad.any()
    assert not RR.bits(_np(xp), dtype)[pad].any()
    assert not _bytes(xq)[pad].any()
    block_rows = np.repeat(np.arange(route.rows // 128), np.diff(offsets))
    pad_blocks = pad.reshape(-1, 128)[block_rows]       # [nb, 128] rows
    assert not RR.bits(_np(g.data), dtype)[pad_blocks].any()
    assert not _bytes(hq.data)[pad_blocks].any()
    assert not RR.bits(_np(y), dtype)[pad].any()

    # Against the 16-bit layer on the unquantised weights: printed only.
    full = _np(ops.moe_mlp(x, top, ew, w1, w2, EXPERTS, v1=v1, rows=rows))
    diff = _np(out) - full
    rel = float(np.linalg.norm(diff) / np.linalg.norm(full))
    print(f"moe_mlp_fp8 vs moe_mlp {dtype} {'glu' if glu else 'mlp'} "
          f"ffn={ffn}: relative error {rel:.4f} (max |diff| "
          f"{float(np.abs(diff).max()):.4f}, rms of the output "
          f"{float(np.sqrt(np.mean(full * full))):.4f})")


def test_grad_requiring_inputs_raise():
    x, top, ew, w1, w2, _ = _inputs("bf16", 128, False)
    w1q, w2q = ops.quantize_weight(w1), ops.quantize_weight(w2)
    with pytest.raises(ValueError, match="forward only"):
        ops.moe_mlp_fp8(x.clone().requires_grad_(), top, ew, w1q, w2q, EXPERTS)
    with pytest.raises(ValueError, match="forward only"):
        ops.moe_mlp_fp8(x, top, ew.clone().requires_grad_(), w1q, w2q, EXPERTS)
    with pytest.raises(ValueError, match="forward only"):
        ops.quantize_weight(w1.clone().requires_grad_())
    with torch.no_grad():  # grad mode off: accepted, and no graph
        out = ops.moe_mlp_fp8(x.clone().requires_grad_(), top, ew, w1q, w2q,
                              EXPERTS)
    assert not out.requires_grad


def test_checkpoint_tensors_are_used_as_they_are():
    x, top, ew, w1, w2, _ = _inputs("bf16", 128, False)
    w1q, w2q = ops.quantize_weight(w1), ops.quantize_weight(w2)
    again = ops.Fp8Weight.from_tensors(w1q.q.view(torch.uint8).clone(),
                                       w1q.scales.clone())
    assert again.shape == w1q.shape
    assert _same(ops.moe_mlp_fp8(x, top, ew, again, w2q, EXPERTS),
                 ops.moe_mlp_fp8(x, top, ew, w1q, w2q, EXPERTS))
