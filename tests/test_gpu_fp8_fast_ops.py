"""GPU: `accumulate="fast"` through sputnik_amd/ops.py. moe_mlp_fp8 in the
fast mode is held, stage by stage and bit for bit, against the same chain
composed by hand from the ctypes entry points (sp.QuantizeRows, sp.SddFp8,
sp.DsdFp8 with accumulate="fast", which tests/test_gpu_fp8_fast.py holds to
Fp8IntervalSums), and the default call against the fp32-mode chain. The error
of the whole layer against ops.moe_mlp on the unquantised weights is printed
next to the fp32 mode's, not asserted: it measures the format (DESIGN has the
figures)."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import sputnik_amd as sp  # noqa: E402
from sputnik_amd import ops  # noqa: E402
from tests import test_gpu_fp8_ops as T  # noqa: E402

pytestmark = pytest.mark.gpu

EXPERTS, FFN = T.EXPERTS, 384   # 3 DSD steps per expert row: the ring refills


def by_hand(x, top, ew, w1q, w2q, v1q, act, mode):
    """The layer from the ctypes entry points; returns every stage."""
    td = x.dtype
    route = ops.moe_route(top, EXPERTS, None)
    xp = ops.padded_gather(x, route)
    topo = ops.expert_topology(route.padded_bins, FFN // 128,
                               route.rows // 128, dtype=td)
    rows = route.rows
    xq = torch.empty(rows, T.D_MODEL, dtype=torch.float8_e4m3fn, device="cuda")
    xs = torch.empty(rows, T.D_MODEL // 128, dtype=torch.float32,
                     device="cuda")
    sp.QuantizeRows(xp, xq, xs)

    def sdd(w):
        data = torch.empty(topo.nnz_blocks, 128, 128, dtype=td, device="cuda")
        topo._meta.ensure_row_indices(data)
        sp.SddFp8(xq, xs, w.q, w.scales, topo._meta.descriptor(data),
                  accumulate=mode)
        return data

    g = sdd(w1q)
    u = sdd(v1q) if v1q is not None else None
    hq = torch.empty(topo.nnz_blocks * 128, 128, dtype=torch.float8_e4m3fn,
                     device="cuda")
    hs = torch.empty(topo.nnz_blocks * 128, dtype=torch.float32, device="cuda")
    if u is None:
        sp.QuantizeRows(g.view(-1, 128), hq, hs.view(-1, 1), activation=act)
    else:
        sp.QuantizeRows(u.view(-1, 128), hq, hs.view(-1, 1), activation=act,
                        gate=g.view(-1, 128))
    y = torch.empty(rows, T.D_MODEL, dtype=td, device="cuda")
    sp.DsdFp8(topo._meta.descriptor(hq.view(-1, 128, 128)), hs, w2q.q,
              w2q.scales, sp.Matrix(rows, T.D_MODEL, y), accumulate=mode)
    out = ops.padded_scatter(y, route, ew)
    return dict(route=route, topo=topo, xq=xq, xs=xs, g=g, u=u, hq=hq, hs=hs,
                y=y, out=out)


@pytest.mark.parametrize("glu", [False, True], ids=["gelu-mlp", "silu-glu"])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_moe_mlp_fp8_fast_equals_the_entry_points_composed_by_hand(dtype,
                                                                   glu):
    x, top, ew, w1, w2, v1 = T._inputs(dtype, FFN, glu)
    td = x.dtype
    w1q, w2q = ops.quantize_weight(w1), ops.quantize_weight(w2)
    v1q = ops.quantize_weight(v1) if glu else None
    act = "silu" if glu else "gelu"
    outs = {}
    for mode in ("fp32", "fast"):
        hand = by_hand(x, top, ew, w1q, w2q, v1q, act, mode)
        # ops, stage by stage, from the same route
        route, topo = hand["route"], hand["topo"]
        xq, xs = ops.quantize_rows(ops.padded_gather(x, route))
        assert torch.equal(xq.view(torch.uint8), hand["xq"].view(torch.uint8))
        assert torch.equal(xs, hand["xs"])
        g = ops.sdd_fp8(xq, xs, w1q, topo, td, accumulate=mode)
        assert T._same(g.data, hand["g"])
        if glu:
            u = ops.sdd_fp8(xq, xs, v1q, topo, td, accumulate=mode)
            assert T._same(u.data, hand["u"])
            hq = ops.quantize_sparse(u, act, gate=g)
        else:
            hq = ops.quantize_sparse(g, act)
        assert torch.equal(hq.data.view(torch.uint8).reshape(-1),
                           hand["hq"].view(torch.uint8).reshape(-1))
        assert torch.equal(hq.scales.reshape(-1), hand["hs"])
        y = ops.dsd_fp8(hq, w2q, td, accumulate=mode)
        assert T._same(y, hand["y"])
        out = ops.moe_mlp_fp8(x, top, ew, w1q, w2q, EXPERTS, v1q=v1q,
                              accumulate=mode)
        assert out.dtype == td and not out.requires_grad
        assert T._same(out, hand["out"])
        outs[mode] = out
    # The default is the fp32 mode, bit for bit.
    assert T._same(ops.moe_mlp_fp8(x, top, ew, w1q, w2q, EXPERTS, v1q=v1q),
                   outs["fp32"])
    assert T._same(ops.sdd_fp8(xq, xs, w1q, topo, td).data,
                   ops.sdd_fp8(xq, xs, w1q, topo, td, accumulate="fp32").data)
    # ... and the fast mode is another kernel: on this data some outputs move
    assert not T._same(outs["fast"], outs["fp32"])

    full = T._np(ops.moe_mlp(x, top, ew, w1, w2, EXPERTS, v1=v1))
    for mode in ("fp32", "fast"):
        diff = T._np(outs[mode]) - full
        print(f"moe_mlp_fp8 accumulate={mode} vs moe_mlp {dtype} "
              f"{'glu' if glu else 'mlp'} ffn={FFN}: relative 2-norm error "
              f"{float(np.linalg.norm(diff) / np.linalg.norm(full)):.4f}")


def test_a_wrong_accumulate_raises():
    x, top, ew, w1, w2, _ = T._inputs("bf16", 128, False)
    w1q, w2q = ops.quantize_weight(w1), ops.quantize_weight(w2)
    with pytest.raises(ValueError, match="accumulate"):
        ops.moe_mlp_fp8(x, top, ew, w1q, w2q, EXPERTS, accumulate="fp16")
