"""GPU: the fused gated MX SDD (sputnik/block/mx.h, SddMxGated) against the
float64 product, the three-call chain it replaces (bit for bit), the CPU
models of its bias and clamped-SwiGLU stages, and ops.moe_glu_mx."""

import ctypes

import numpy as np
import pytest
import torch

import sputnik_amd as sp
from sputnik_amd import ops
from tests import activation_ref as A
from tests import bias_ref as B
from tests import fp8_ref as F
from tests import helpers as H
from tests import moe_ref as M
from tests import mx_ref as R
from tests import rounding_ref as RR
from tests.test_gpu_fp8 import FILL, dev, guarded, host
from tests.test_gpu_mx import (SDD_TOPOLOGY, check_random, cuda, exact,
                               random_operands, sdd_call, weight_dev)

pytestmark = pytest.mark.gpu

DTYPES, FORMATS, KS = ["f16", "bf16"], ["e4m3", "e2m1"], [128, 384]
M_ROWS = N_COLS = 256
NB, CLAMP = len(SDD_TOPOLOGY[1]), (1.702, 7.0)
cases = pytest.mark.parametrize("dtype,fmt,k", [
    (d, f, k) for d in DTYPES for f in FORMATS for k in KS])


def operands(fmt, dtype, k, seed=5):
    """(aq, sa, gate codes, gate scales, up codes, up scales), one draw halved.
    (With k = 128 a sum can land among fp16's subnormals, whose fixed quantum
    mx.h's bound leaves out: test_products asserts that this draw has none.)"""
    aq, sa, wc, sw = random_operands(M_ROWS, k, 2 * N_COLS, fmt, dtype,
                                     [seed, k])
    return aq, sa, wc[:N_COLS], sw[:N_COLS], wc[N_COLS:], sw[N_COLS:]


def fused(o, fmt, dtype, keep=(), topo=SDD_TOPOLOGY, interleaved=False,
          outs=None, **kw):
    """One SddMxGated call into guarded buffers (or `outs`); host arrays by
    name, 16-bit ones as bits."""
    aq, sa, gc, gs, uc, us = o
    offsets, indices = topo
    td = H.torch_dtype(dtype)
    c = sp.BlockMatrix(M_ROWS, N_COLS, 128, NB * 128 * 128,
                       torch.empty(0, dtype=td, device="cuda"), cuda(offsets),
                       cuda(indices))
    c.row_indices = cuda(F.row_indices(offsets))
    if interleaved:
        wq = weight_dev(np.stack([gc, uc], 1).reshape(2 * N_COLS, -1), fmt)
        ws = cuda(np.stack([gs, us], 1).reshape(2 * N_COLS, -1))
        w = (wq[0::2], ws[0::2], wq[1::2], ws[1::2])
    else:
        w = (weight_dev(gc, fmt), cuda(gs), weight_dev(uc, fmt), cuda(us))
    bufs = {"hq": guarded((NB, 128, 128), torch.float8_e4m3fn),
            "h_scales": guarded((NB * 128, 4), torch.uint8)}
    for name in keep:
        bufs[name + "_out"] = guarded((NB, 128, 128), td)
    for name, t in (outs or {}).items():
        bufs[name] = (t, lambda: True)
    sp.SddMxGated(cuda(aq, torch.float8_e4m3fn), cuda(sa), *w, c,
                  format=fmt, b_row_step=2 if interleaved else 1,
                  **{n: b[0] for n, b in bufs.items()}, **kw)
    torch.cuda.synchronize()
    assert all(ok() for _, ok in bufs.values())
    return {n.replace("_out", ""): (
        t.view(torch.uint8).cpu().numpy() if t.element_size() == 1
        else RR.bits(host(t), dtype)) for n, (t, _) in bufs.items()}


def blocks(dense):
    return F.blocks_from_dense(dense, *SDD_TOPOLOGY)


def same(got, want, names):
    assert all(np.array_equal(got[n], want[n]) for n in names)


@cases
def test_products_against_float64(dtype, fmt, k):
    o = operands(fmt, dtype, k)
    for name, w in (("g_out", o[2:4]), ("u_out", o[4:6])):
        ref, absum = exact(o[0], o[1], *w, fmt)
        # (the data admits the bound: the correctly rounded result meets it)
        assert (np.abs(RR.round_once(ref, dtype) - ref)
                <= R.bound(ref, absum, k, dtype)).all()
        check_random(lambda out: fused(o, fmt, dtype, outs={name: out}),
                     (NB, 128, 128), blocks(ref), blocks(absum), k, dtype)


@pytest.mark.parametrize("act", ["silu", "gelu"])
@cases
def test_bit_chain(dtype, fmt, k, act):
    o = operands(fmt, dtype, k)
    g = sdd_call(o[0], o[1], o[2], o[3], fmt, dtype, SDD_TOPOLOGY)
    u = sdd_call(o[0], o[1], o[4], o[5], fmt, dtype, SDD_TOPOLOGY)
    q = torch.empty(NB * 128, 128, dtype=torch.float8_e4m3fn, device="cuda")
    s = torch.empty(NB * 128, 4, dtype=torch.uint8, device="cuda")
    sp.QuantizeRowsMx(u.view(-1, 128), q, s, act, g.view(-1, 128))
    want = {"g": RR.bits(host(g), dtype), "u": RR.bits(host(u), dtype),
            "hq": q.view(torch.uint8).cpu().numpy().reshape(NB, 128, 128),
            "h_scales": s.cpu().numpy()}
    same(fused(o, fmt, dtype, keep="gu", activation=act), want, want)
    same(fused(o, fmt, dtype, activation=act), want, ["hq", "h_scales"])
    # one interleaved [2 n, k] weight, step 2: the same bits
    same(fused(o, fmt, dtype, keep="gu", activation=act, interleaved=True),
         want, want)


def clamped64(g, u, alpha=CLAMP[0], limit=CLAMP[1]):
    gc, uc = np.minimum(g, limit), np.clip(u, -limit, limit)
    return (uc + 1.0) * (gc * A._sigmoid(alpha * gc))


@cases
def test_bias_and_clamp(dtype, fmt, k):
    aq, sa, gc, gs, uc, us = operands(fmt, dtype, k, seed=4)
    rng = np.random.default_rng([8, k])
    refs = []
    for wc, ws in ((gc, gs), (uc, us)):
        # a power of two on the weight's scales brings the std to limit / 2
        ref = exact(aq, sa, wc, ws, fmt)[0]
        shift = int(np.rint(np.log2(CLAMP[1] / 2 / blocks(ref).std())))
        ws += np.uint8(shift % 256)
        bias = RR.round_once(rng.standard_normal(N_COLS) * 2.0, dtype)
        refs.append((blocks(ref * 2.0 ** shift + bias), bias))
    (g64, b1), (u64, bv1) = refs
    hit = [g64 > CLAMP[1], u64 > CLAMP[1], u64 < -CLAMP[1]]
    assert all(h.mean() >= 0.01 for h in hit), [h.mean() for h in hit]
    assert (~(hit[0] | hit[1] | hit[2])).mean() >= 0.5
    o = (aq, sa, gc, gs, uc, us)
    got = fused(o, fmt, dtype, keep="guh", clamp=CLAMP,
                gate_bias=dev(b1, dtype), up_bias=dev(bv1, dtype))
    vals = {}
    for name, w, bias in (("g", o[2:4], b1), ("u", o[4:6], bv1)):
        plain = host(sdd_call(aq, sa, *w, fmt, dtype, SDD_TOPOLOGY))
        vals[name] = B.bias_stage(plain, SDD_TOPOLOGY[1], bias, dtype)
        assert np.array_equal(got[name], RR.bits(vals[name], dtype)), name
    worst = A.check(got["h"], clamped64(vals["g"].astype(np.float64),
                                        vals["u"].astype(np.float64)),
                    dtype, "clamped SwiGLU")
    print(f"{dtype} {fmt} k={k}: worst {worst} steps")
    q, s = R.quantize(A.bits_to_f64(got["h"], dtype).reshape(-1, 128))
    same(got, {"hq": q.reshape(NB, 128, 128), "h_scales": s}, ["hq", "h_scales"])


@pytest.mark.parametrize("fmt", FORMATS)
def test_nan_row_and_out_of_range_block(fmt):
    o = operands(fmt, "bf16", 384)
    o[0][5, 200] = 0x7F          # a NaN byte of A: row 5 of block row 0
    got = fused(o, fmt, "bf16", keep="gu")
    want = np.zeros((NB, 128, 128), bool)
    want[:2, 5, :] = True        # blocks 0 and 1 are block row 0's
    assert all(np.array_equal(np.isnan(A.bits_to_f64(got[n], "bf16")), want)
               for n in "gu")
    assert np.array_equal((got["hq"] & 0x7F) == 0x7F, want)
    # block 1 at a column past the matrix: left as it was, in every output
    skipped = fused(o, fmt, "bf16", keep="guh",
                    topo=(SDD_TOPOLOGY[0], np.array([1, 2, 1], np.int16)))
    assert all((skipped[n][1].view(np.uint8) == FILL).all()
               for n in ("g", "u", "h", "hq"))
    assert (skipped["h_scales"][128:256] == FILL).all()
    assert np.array_equal(skipped["g"][[0, 2]], got["g"][[0, 2]])


def test_rejections_leave_the_outputs_untouched():
    L, bad = sp.lib(), sp.hipErrorInvalidValue
    stream = torch.cuda.current_stream().cuda_stream
    z = lambda *s: torch.zeros(*s, dtype=torch.uint8, device="cuda")  # noqa: E731
    aq, wq, sa, sw = z(256, 256), z(512 * 256 + 16), z(256, 8), z(512, 8)
    bias = torch.zeros(264, dtype=torch.float16, device="cuda")
    hq, hs = z(3, 128, 128) + 7, z(384, 4) + 7
    g = torch.full((3, 128, 128), 7.0, dtype=torch.float16, device="cuda")
    c = sp.BlockMatrix(256, 256, 128, 3 * 128 * 128, g,
                       cuda(SDD_TOPOLOGY[0]), cuda(SDD_TOPOLOGY[1]))
    c.row_indices = cuda(F.row_indices(SDD_TOPOLOGY[0]))
    cc = c._c()

    def call(a=aq.data_ptr(), k=256, gate=wq.data_ptr(),
             up=wq.data_ptr() + 256, us=sw.data_ptr() + 8, step=2, fmt=0,
             b1=bias.data_ptr(), kind=1, act=2, alpha=1.702, limit=7.0,
             q=hq.data_ptr(), s=hs.data_ptr(), keep_g=g.data_ptr(),
             keep_u=None):
        return L.sputnik_sdd_mx_gated(
            a, sa.data_ptr(), k, gate, sw.data_ptr(), up, us, step, fmt, b1,
            None, kind, act, alpha, limit, ctypes.byref(cc), q, s, keep_g,
            keep_u, None, 0, stream)

    nan, inf = float("nan"), float("inf")
    for kw in (dict(step=0), dict(step=3), dict(fmt=2), dict(kind=2),
               dict(act=3), dict(act=-1), dict(limit=0.0), dict(limit=nan),
               dict(alpha=inf), dict(k=192), dict(a=None), dict(q=None),
               dict(s=None), dict(up=wq.data_ptr() + 8),
               dict(us=sw.data_ptr() + 2), dict(b1=bias.data_ptr() + 1),
               dict(q=hq.data_ptr() + 4), dict(keep_g=aq.data_ptr()),
               dict(keep_u=g.data_ptr()), dict(q=wq.data_ptr())):
        assert call(**kw) == bad, kw
    torch.cuda.synchronize()
    assert bool((hq == 7).all() and (hs == 7).all() and (g == 7.0).all())
    assert call() == sp.hipSuccess
    torch.cuda.synchronize()
    assert not g.any() and not hq.any()      # zeros times 2^-127


TOKENS, D_MODEL, FFN, EXPERTS, TOP_K = 300, 256, 256, 4, 2
# Relative Frobenius error of the gpt-oss-shaped layer against float64 on the
# dequantised weights: twice the measured value (DESIGN 10 has the figures).
MOE_CAP = {("f16", "e4m3"): 2 * 0.04339, ("f16", "e2m1"): 2 * 0.04284,
           ("bf16", "e4m3"): 2 * 0.04382, ("bf16", "e2m1"): 2 * 0.04301}


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_moe_glu_mx_equals_its_chain_and_is_close_to_float64(dtype, fmt):
    td, hidden = H.torch_dtype(dtype), EXPERTS * FFN
    xv = M.values((TOKENS, D_MODEL), dtype, [31])
    wt = M.values((2 * hidden, D_MODEL), dtype, [32]) / np.float32(8)
    w2 = M.values((hidden, D_MODEL), dtype, [33]) / np.float32(16)
    b1, bv1 = (M.values((hidden,), dtype, [34, i]) / np.float32(4)
               for i in range(2))
    b2 = M.values((EXPERTS, D_MODEL), dtype, [35]) / np.float32(4)
    topv = M.routing(TOKENS, TOP_K, EXPERTS, "random", seed=5)
    ewv = M.unit_weights(TOKENS * TOP_K, dtype, [36]).reshape(TOKENS, TOP_K)
    x, top, ew = cuda(xv).to(td), cuda(topv), cuda(ewv).to(td)
    both = ops.quantize_weight_mx(cuda(wt).to(td), transpose=True, format=fmt)
    w1v1 = ops.MxGluWeight.from_interleaved(both.q, both.scales, fmt)
    w2q = ops.quantize_weight_mx(cuda(w2).to(td), format=fmt)
    kw = dict(clamp=CLAMP, b1=cuda(b1).to(td), bv1=cuda(bv1).to(td))
    out = ops.moe_glu_mx(x, top, ew, w1v1, w2q, EXPERTS, b2=cuda(b2).to(td),
                         **kw)
    assert out.dtype == td and not out.requires_grad

    route = ops.moe_route(top, EXPERTS)
    topo = ops.expert_topology(route.padded_bins, FFN // 128,
                               route.rows // 128, dtype=td)
    xq, xs = ops.quantize_rows_mx(ops.padded_gather(x, route))
    hq = ops.sdd_mx_gated(xq, xs, w1v1, topo, out_dtype=td, **kw)
    chain = ops.padded_scatter_bias(ops.dsd_mx(hq, w2q, td), route, ew,
                                    bias=cuda(b2).to(td))
    assert torch.equal(out.view(torch.int16), chain.view(torch.int16))

    def dequantised(w):     # [n, k] float64
        codes = w.q.view(torch.uint8).cpu().numpy()
        if fmt == "e2m1":
            codes = np.stack([codes & 15, codes >> 4], -1).reshape(w.n, w.k)
        return R.decode(codes, w.scales.cpu().numpy(), fmt == "e2m1")
    w1, w2d = dequantised(both), dequantised(w2q)
    y = np.zeros((EXPERTS, TOKENS, D_MODEL))
    for e in range(EXPERTS):
        cols = slice(e * FFN, (e + 1) * FFN)
        g = xv @ w1[0::2][cols].T + b1[cols]
        u = xv @ w1[1::2][cols].T + bv1[cols]
        y[e] = clamped64(g, u) @ w2d[:, cols].T + b2[e]
    ref = sum(ewv[:, j:j + 1].astype(np.float64)
              * y[topv[:, j], np.arange(TOKENS)] for j in range(TOP_K))
    rel = float(np.linalg.norm(host(out) - ref) / np.linalg.norm(ref))
    print(f"moe_glu_mx {dtype} {fmt}: relative error {rel:.5f}")
    assert rel <= MOE_CAP[dtype, fmt]
