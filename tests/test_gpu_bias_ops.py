"""GPU: the bias entry points of sputnik_amd/ops.py: sdd_bias, column_sum,
mlp_bias, glu_mlp_bias, moe_mlp_bias and moe_layer_bias, forward and backward.

Expected values: the same computation restated in float64 torch with autograd
on the same operands (a dense loop over experts for the MoE layer), under
helpers.assert_close, the criterion of tests/test_gpu_gated_ops.py. The
bit-for-bit comparison of moe_layer_bias without biases against moe_layer
compares the library with itself: it shows that the new entry point changes
nothing where no bias is given, it is not a correctness oracle."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import oracle as O  # noqa: E402
from sputnik_amd import ops  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests.test_gpu_activation_ops import (  # noqa: E402
    B, HIDDEN, K, TOKENS, _dev, _mask, _np, _topology)

pytestmark = pytest.mark.gpu

ACTS = ("relu", "gelu", "silu")
_DATA = {}


def _data(dtype, act=None):
    """Operands (rounded to T, float64 copies) once per (dtype, kind).

    Gaussian operands for fp16 with gelu and silu. Two cases take operands
    whose hidden pre-activations are exact in T instead: x in {-1, 0, 1}, w1
    and v1 in {-1, 0, 1} / 4 (every product a multiple of 1/4 below 16) and
    biases that are odd multiples of 1/8, so that Z = x w1 + b1 is exact and
    never closer to zero than 1/8.
    - relu: the contract rounds x w1 to T before the bias is added, so with
      Gaussian operands Z = round(x w1) + b1 is exactly zero now and then
      where the float64 restatement has a tiny nonzero value, and relu' of
      the two differs by a whole term of the gradient (measured: 154 of
      24576 elements of dx off by up to 1.0).
    - bf16: the bias adds one more rounding of Z to the chain that
      tests/test_gpu_moe_ops.py describes, which leaves helpers.assert_close
      no room with reals (measured with Gaussian operands: one of 49152
      elements of dv1 at about 1.3 times the tolerance, the rest inside)."""
    exact = act == "relu" or dtype == "bf16"
    key = (dtype, exact)
    if key not in _DATA and exact:
        rng = np.random.default_rng(43 + (dtype == "bf16"))
        d = dict(_data("f16"))                   # (dy, dh, w2: Gaussian)
        d = {k: O.round_to(v.astype(np.float32), dtype).astype(np.float64)
             for k, v in d.items()}

        def ints(*shape, scale=1.0):
            return rng.integers(-1, 2, shape).astype(np.float64) * scale

        def odd_eighths(n):
            return (2 * rng.integers(-4, 4, n) + 1).astype(np.float64) / 8
        d.update(x=ints(TOKENS, K), w1=ints(K, HIDDEN, scale=0.25),
                 v1=ints(K, HIDDEN, scale=0.25), b1=odd_eighths(HIDDEN),
                 bv1=odd_eighths(HIDDEN))
        for v in d.values():
            v.setflags(write=False)
        _DATA[key] = d
    if key not in _DATA:
        rng = np.random.default_rng(41 + (dtype == "bf16"))

        def make(*shape, scale=1.0):
            return O.round_to((scale * rng.standard_normal(shape)).astype(
                np.float32), dtype).astype(np.float64)
        _DATA[key] = dict(x=make(TOKENS, K), w1=make(K, HIDDEN, scale=0.25),
                          v1=make(K, HIDDEN, scale=0.25),
                          w2=make(HIDDEN, K, scale=0.1), dy=make(TOKENS, K),
                          dh=make(TOKENS, HIDDEN),
                          b1=make(HIDDEN, scale=0.5),
                          bv1=make(HIDDEN, scale=0.5))
        for v in _DATA[key].values():
            v.setflags(write=False)
    return _DATA[key]


def _f64(a, grad=True):
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).cuda() \
        .requires_grad_(grad)


def _act64(act, t):
    F = torch.nn.functional
    if act == "relu":
        return F.relu(t)
    if act == "gelu":
        return F.gelu(t, approximate="tanh")
    return F.silu(t)


def _block_mask():
    return torch.from_numpy(_mask()[::B, ::B] > 0)


def _sparse_of(dense64, dtype, topo):
    return topo.with_data(ops.from_dense_mask(_dev(dense64, dtype),
                                              _block_mask()).data)


def _close(leaves, refs, names, dtype, what):
    for name, t, r in zip(names, leaves, refs):
        assert t.grad is not None and t.grad.shape == t.shape, name
        assert t.grad.dtype == t.dtype, name
        H.assert_close(_np(t.grad), _np(r.grad), dtype, f"{what} {name}")


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_sdd_bias_and_column_sum(dtype):
    d = _data(dtype)
    mask = torch.from_numpy(_mask()).cuda()
    x, w1, b1 = (_dev(d[k], dtype, True) for k in ("x", "w1", "b1"))
    topo = _topology(dtype)
    c = ops.sdd_bias(x, w1, topo, b1)
    dh = _sparse_of(d["dh"], dtype, topo)
    c.data.backward(dh.data)
    torch.cuda.synchronize()
    refs = [_f64(d[k]) for k in ("x", "w1", "b1")]
    c64 = (refs[0] @ refs[1] + refs[2]) * mask
    c64.backward(_f64(d["dh"], False) * mask)
    H.assert_close(_np(c.to_dense()), _np(c64), dtype, "sdd_bias forward")
    _close((x, w1, b1), refs, ("da", "db", "dbias"), dtype, "sdd_bias")
    # column_sum of the incoming gradient is that bias gradient, unrounded
    s = ops.column_sum(dh)
    assert s.dtype == torch.float32 and s.shape == (HIDDEN,)
    H.assert_close(_np(s), (d["dh"] * _mask()).sum(axis=0), dtype,
                   "column_sum")
    assert torch.equal(s, ops.column_sum(dh)), "two calls, the same bits"


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_mlp_bias_forward_backward(dtype, act):
    d = _data(dtype, act)
    mask = torch.from_numpy(_mask()).cuda()
    names = ("x", "w1", "w2", "b1")
    leaves = [_dev(d[k], dtype, True) for k in names]
    x, w1, w2, b1 = leaves
    topo = _topology(dtype)
    y = ops.mlp_bias(x, w1, w2, topo, act, b1=b1)
    # x, w1, w2 and Z, as mlp keeps them: the bias is not saved
    assert len(y.grad_fn.saved_tensors) == 4
    y.backward(_dev(d["dy"], dtype))
    torch.cuda.synchronize()
    refs = [_f64(d[k]) for k in names]
    rx, rw1, rw2, rb1 = refs
    y64 = (_act64(act, rx @ rw1 + rb1) * mask) @ rw2
    y64.backward(_f64(d["dy"], False))
    H.assert_close(_np(y), _np(y64), dtype, f"mlp_bias {act} y")
    _close(leaves, refs, ("dx", "dw1", "dw2", "db1"), dtype,
           f"mlp_bias {act}")
    # sdd_act_bias is its first half
    h = ops.sdd_act_bias(x.detach(), w1.detach(), topo, act, bias=b1.detach())
    h64 = _act64(act, rx @ rw1 + rb1) * mask
    H.assert_close(_np(h.to_dense()), _np(h64), dtype, f"sdd_act_bias {act}")


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_glu_mlp_bias_forward_backward(dtype, act):
    d = _data(dtype, act)
    mask = torch.from_numpy(_mask()).cuda()
    names = ("x", "w1", "v1", "w2", "b1", "bv1")
    leaves = [_dev(d[k], dtype, True) for k in names]
    x, w1, v1, w2, b1, bv1 = leaves
    topo = _topology(dtype)
    y = ops.glu_mlp_bias(x, w1, v1, w2, topo, act, b1=b1, bv1=bv1)
    # x, w1, v1, w2, Z1 and Z2, as glu_mlp keeps them
    assert len(y.grad_fn.saved_tensors) == 6
    y.backward(_dev(d["dy"], dtype))
    torch.cuda.synchronize()
    refs = [_f64(d[k]) for k in names]
    rx, rw1, rv1, rw2, rb1, rbv1 = refs
    y64 = (_act64(act, rx @ rw1 + rb1) * (rx @ rv1 + rbv1) * mask) @ rw2
    y64.backward(_f64(d["dy"], False))
    H.assert_close(_np(y), _np(y64), dtype, f"glu_mlp_bias {act} y")
    _close(leaves, refs, ("dx", "dw1", "dv1", "dw2", "db1", "dbv1"), dtype,
           f"glu_mlp_bias {act}")


# ---- the MoE layer ----------------------------------------------------------

M_TOKENS, TOP_K, EXPERTS, D_MODEL, FFN = 129, 2, 4, 256, 128
_MOE = {}


def _moe_data():
    """Operands of the layer tests, once. As tests/test_gpu_moe_ops.py
    explains for moe_mlp, a chain of bf16 roundings leaves
    helpers.assert_close little room with random reals, so: x and dy in
    {-1, 0, 1}, the expert weights in {-1, 0, 1} / 16, the biases in
    {-1, 0, 1} / 4, the router weights of a token (1/4, 3/4), (1/2, 1/2) or
    (3/4, 1/4). Z1, Z2 and the weighted dy are then exact in bf16."""
    if not _MOE:
        rng = np.random.default_rng(23)

        def make(*shape, scale=1.0):
            return (rng.integers(-1, 2, shape) * scale).astype(np.float32)
        top = np.stack([rng.permutation(EXPERTS)[:TOP_K]
                        for _ in range(M_TOKENS)])
        first = rng.choice([0.25, 0.5, 0.75], M_TOKENS).astype(np.float32)
        _MOE.update(
            top=top, gates=np.stack([first, 1 - first], axis=1),
            x=make(M_TOKENS, D_MODEL),
            w1=make(D_MODEL, EXPERTS * FFN, scale=1 / 16),
            v1=make(D_MODEL, EXPERTS * FFN, scale=1 / 16),
            w2=make(EXPERTS * FFN, D_MODEL, scale=1 / 16),
            b1=make(EXPERTS * FFN, scale=1 / 4),
            bv1=make(EXPERTS * FFN, scale=1 / 4),
            b2=make(EXPERTS, D_MODEL, scale=1 / 4),
            wr=make(EXPERTS, D_MODEL, scale=1 / 16),
            dy=make(M_TOKENS, D_MODEL))
        for v in _MOE.values():
            v.setflags(write=False)
    return _MOE


def _dense_reference(d, glu):
    """y[t] = sum_k gate[t, k] * (MLP_e(x[t]) + b2[e]), e = top[t, k], in
    float64 torch: every expert applied to every token, then selected."""
    F = torch.nn.functional
    names = ["x", "gates", "w1", "w2", "b1", "b2"] + \
        (["v1", "bv1"] if glu else [])
    t = {k: _f64(d[k]) for k in names}
    top = torch.from_numpy(np.array(d["top"])).cuda()
    y = torch.zeros(M_TOKENS, D_MODEL, dtype=torch.float64, device="cuda")
    for e in range(EXPERTS):
        cols = slice(e * FFN, (e + 1) * FFN)
        z1 = t["x"] @ t["w1"][:, cols] + t["b1"][cols]
        if glu:
            h = F.silu(z1) * (t["x"] @ t["v1"][:, cols] + t["bv1"][cols])
        else:
            h = F.gelu(z1, approximate="tanh")
        share = (t["gates"] * (top == e)).sum(1, keepdim=True)
        y = y + share * (h @ t["w2"][cols] + t["b2"][e])
    y.backward(_f64(d["dy"], False))
    return y, names, [t[k] for k in names]


@pytest.mark.parametrize("glu", [False, True], ids=["mlp", "glu"])
@pytest.mark.parametrize("gate_dtype", ["f32", "bf16"])
def test_moe_mlp_bias_forward_backward_bf16(glu, gate_dtype):
    d = _moe_data()
    top = torch.from_numpy(np.array(d["top"])).cuda()
    ref_y, names, refs = _dense_reference(d, glu)
    leaves = []
    for k in names:
        if k == "gates":
            g = torch.from_numpy(np.array(d["gates"])).cuda()
            g = g.bfloat16() if gate_dtype == "bf16" else g
            leaves.append(g.requires_grad_(True))
        else:
            leaves.append(_dev(d[k], "bf16", True))
    t = dict(zip(names, leaves))
    y = ops.moe_mlp_bias(t["x"], top, t["gates"], t["w1"], t["w2"], EXPERTS,
                         v1=t.get("v1"),
                         rows=ops.moe_rows_bound(M_TOKENS * TOP_K, EXPERTS),
                         b1=t["b1"], bv1=t.get("bv1"), b2=t["b2"])
    assert y.shape == (M_TOKENS, D_MODEL) and y.dtype == torch.bfloat16
    y.backward(_dev(d["dy"], "bf16"))
    torch.cuda.synchronize()
    H.assert_close(_np(y), _np(ref_y), "bf16", "moe_mlp_bias y")
    _close(leaves, refs, ["d" + k for k in names], "bf16", "moe_mlp_bias")


def _layer_operands(d, glu, biases):
    keys = ["x", "wr", "w1", "w2"] + (["v1"] if glu else [])
    t = {k: _dev(d[k], "bf16", True) for k in keys}
    if biases:
        for k in ["b1", "b2"] + (["bv1"] if glu else []):
            t[k] = _dev(d[k], "bf16", True)
    return t


def test_moe_layer_bias_without_biases_is_moe_layer():
    d = _moe_data()
    dy = _dev(d["dy"], "bf16")
    outs = []
    for biased in (False, True):
        t = _layer_operands(d, True, False)
        if biased:
            y = ops.moe_layer_bias(t["x"], t["wr"], t["w1"], t["w2"], TOP_K,
                                   v1=t["v1"], b1=None, b2=None)
        else:
            y = ops.moe_layer(t["x"], t["wr"], t["w1"], t["w2"], TOP_K,
                              v1=t["v1"])
        y.backward(dy)
        outs.append([y.detach()] + [t[k].grad for k in ("x", "wr", "w1",
                                                        "v1", "w2")])
    for i, (a, b) in enumerate(zip(*outs)):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), i


def test_moe_layer_bias_with_explicit_rows_makes_no_host_sync():
    """Forward and backward with all three biases under torch's sync debug
    mode, then the forward captured into a graph and replayed: neither
    waits for the device."""
    d = _moe_data()
    rows = ops.moe_rows_bound(M_TOKENS * TOP_K, EXPERTS)
    dy = _dev(d["dy"], "bf16")

    def run(t):
        y = ops.moe_layer_bias(t["x"], t["wr"], t["w1"], t["w2"], TOP_K,
                               v1=t["v1"], rows=rows, b1=t["b1"],
                               bv1=t["bv1"], b2=t["b2"])
        y.backward(dy)
        return y

    first, second = (_layer_operands(d, True, True) for _ in range(2))
    run(first)                              # (first-use initialisation)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        y = run(second)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert torch.isfinite(y.float()).all()
    for k in ("b1", "bv1", "b2"):
        assert second[k].grad.abs().max() > 0, k
        assert torch.equal(second[k].grad, first[k].grad), k

    t = {k: v.detach() for k, v in second.items()}
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        out = ops.moe_layer_bias(t["x"], t["wr"], t["w1"], t["w2"], TOP_K,
                                 v1=t["v1"], rows=rows, b1=t["b1"],
                                 bv1=t["bv1"], b2=t["b2"])
    out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), y.detach().view(torch.int16))
    del graph
