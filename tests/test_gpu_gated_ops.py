"""GPU: ops.sdd_gated and ops.glu_mlp (sputnik_amd/ops.py), forward and
backward, with and without gradient sinks, on a 3-expert topology of a few
blocks (the shapes of tests/test_gpu_activation_ops.py). Expected values: the
same computation in fp32 torch with autograd on the same operands, under
helpers.assert_close. The bit-for-bit comparison of glu_mlp with the unfused
composition of this library's own calls (plain SDD, then the elementwise
kernels) is a route check, not a correctness oracle."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import sputnik_amd as sp  # noqa: E402
from sputnik_amd import ops  # noqa: E402
from tests import gated_ref as R  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests.test_gpu_activation_ops import (  # noqa: E402
    B, HIDDEN, K, TOKENS, _dev, _mask, _np, _topology)

pytestmark = pytest.mark.gpu

_DATA = {}


def _data(dtype):
    """Operands (rounded to T, float64 copies) once per dtype."""
    if dtype not in _DATA:
        from oracle import oracle as O
        rng = np.random.default_rng(31 + (dtype == "bf16"))

        def make(*shape, scale=1.0):
            return O.round_to((scale * rng.standard_normal(shape)).astype(
                np.float32), dtype).astype(np.float64)
        _DATA[dtype] = dict(x=make(TOKENS, K), w1=make(K, HIDDEN, scale=0.25),
                            v1=make(K, HIDDEN, scale=0.25),
                            w2=make(HIDDEN, K, scale=0.1), dy=make(TOKENS, K),
                            dh=make(TOKENS, HIDDEN), g=make(TOKENS, HIDDEN))
        for v in _DATA[dtype].values():
            v.setflags(write=False)
    return _DATA[dtype]


def _f32(a, grad=True):
    return torch.from_numpy(np.array(a, order="C")).float().cuda() \
        .requires_grad_(grad)


def _act32(act, t):
    F = torch.nn.functional
    if act == "relu":
        return F.relu(t)
    if act == "gelu":
        return F.gelu(t, approximate="tanh")
    return F.silu(t)


def _block_mask():
    return torch.from_numpy(_mask()[::B, ::B] > 0)


def _sparse_of(dense64, dtype, topo):
    """The blocks of a dense [TOKENS, HIDDEN] array, in topo's order."""
    return topo.with_data(ops.from_dense_mask(_dev(dense64, dtype),
                                              _block_mask()).data)


@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("sinks", [False, True])
def test_sdd_gated_forward_backward(dtype, act, sinks):
    d = _data(dtype)
    mask = torch.from_numpy(_mask()).float().cuda()
    x, v1 = _dev(d["x"], dtype, True), _dev(d["v1"], dtype, True)
    topo = _topology(dtype)
    gate = _sparse_of(d["g"], dtype, topo)
    gate.data.requires_grad_(True)
    kw = {}
    if sinks:
        sx = torch.full((TOKENS, K), 0.5, dtype=torch.float32, device="cuda")
        sv = torch.full((K, HIDDEN), 0.5, dtype=torch.float32, device="cuda")
        kw = dict(a_grad_out=sx, b_grad_out=sv)
    h = ops.sdd_gated(x, v1, topo, gate, act, **kw)
    dh = _sparse_of(d["dh"], dtype, topo)
    h.data.backward(dh.data)
    torch.cuda.synchronize()

    x32, v32, g32 = _f32(d["x"]), _f32(d["v1"]), _f32(d["g"])
    h32 = (x32 @ v32) * mask * _act32(act, g32)
    h32.backward(_f32(d["dh"], False) * mask)
    H.assert_close(_np(h.to_dense()), _np(h32), dtype,
                   f"sdd_gated {act} forward")
    H.assert_close(_np(topo.with_data(gate.data.grad).to_dense()),
                   _np(g32.grad) * _mask(), dtype, f"sdd_gated {act} dgate")
    if sinks:
        assert x.grad is None and v1.grad is None
        H.assert_close(_np(sx) - 0.5, _np(x32.grad), dtype,
                       f"sdd_gated {act} dx sink")
        H.assert_close(_np(sv) - 0.5, _np(v32.grad), dtype,
                       f"sdd_gated {act} dv1 sink")
    else:
        H.assert_close(_np(x.grad), _np(x32.grad), dtype,
                       f"sdd_gated {act} dx")
        H.assert_close(_np(v1.grad), _np(v32.grad), dtype,
                       f"sdd_gated {act} dv1")


def test_sdd_gated_rejects_a_foreign_gate():
    topo = _topology("f16")
    x, v1 = _dev(_data("f16")["x"], "f16"), _dev(_data("f16")["v1"], "f16")
    with pytest.raises(TypeError):
        ops.sdd_gated(x, v1, topo, topo.data, "silu")
    with pytest.raises(ValueError):
        ops.sdd_gated(x, v1, topo, topo.t(), "silu")


@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("sinks", [False, True])
def test_glu_mlp_forward_backward(dtype, act, sinks):
    d = _data(dtype)
    mask = torch.from_numpy(_mask()).float().cuda()
    x = _dev(d["x"], dtype, True)
    w1, v1 = _dev(d["w1"], dtype, True), _dev(d["v1"], dtype, True)
    w2 = _dev(d["w2"], dtype, True)
    dy = _dev(d["dy"], dtype)
    topo = _topology(dtype)
    kw = {}
    if sinks:
        s1 = torch.full((K, HIDDEN), 0.5, dtype=torch.float32, device="cuda")
        sv = torch.full((K, HIDDEN), 0.5, dtype=torch.float32, device="cuda")
        s2 = torch.full((HIDDEN, K), 0.5, dtype=torch.float32, device="cuda")
        kw = dict(w1_grad_out=s1, v1_grad_out=sv, w2_grad_out=s2)
    y = ops.glu_mlp(x, w1, v1, w2, topo, act, **kw)

    # Exactly two hidden-sized tensors are kept between the passes.
    hidden = topo.data.numel()
    kept = [t for t in y.grad_fn.saved_tensors if t.numel() == hidden]
    assert len(kept) == 2, [tuple(t.shape) for t in y.grad_fn.saved_tensors]
    assert len(y.grad_fn.saved_tensors) == 6          # x, w1, v1, w2, Z1, Z2

    y.backward(dy)
    torch.cuda.synchronize()

    x32, w1_32, v1_32, w2_32 = (_f32(d[n]) for n in ("x", "w1", "v1", "w2"))
    h32 = _act32(act, (x32 @ w1_32) * mask) * ((x32 @ v1_32) * mask)
    y32 = h32 @ w2_32
    y32.backward(_f32(d["dy"], False))
    H.assert_close(_np(y), _np(y32), dtype, f"glu_mlp {act} y")
    H.assert_close(_np(x.grad), _np(x32.grad), dtype, f"glu_mlp {act} dx")
    if sinks:
        assert w1.grad is None and v1.grad is None and w2.grad is None
        H.assert_close(_np(s1) - 0.5, _np(w1_32.grad), dtype,
                       f"glu_mlp {act} dw1 sink")
        H.assert_close(_np(sv) - 0.5, _np(v1_32.grad), dtype,
                       f"glu_mlp {act} dv1 sink")
        H.assert_close(_np(s2) - 0.5, _np(w2_32.grad), dtype,
                       f"glu_mlp {act} dw2 sink")
        return
    H.assert_close(_np(w1.grad), _np(w1_32.grad), dtype, f"glu_mlp {act} dw1")
    H.assert_close(_np(v1.grad), _np(v1_32.grad), dtype, f"glu_mlp {act} dv1")
    H.assert_close(_np(w2.grad), _np(w2_32.grad), dtype, f"glu_mlp {act} dw2")

    # Route check: the unfused composition of the library's own calls.
    xd, w1d, v1d, w2d = (t.detach() for t in (x, w1, v1, w2))
    same = lambda p, q: torch.equal(p.view(torch.int16), q.view(torch.int16))
    z1, z2 = ops._sdd(xd, w1d, topo), ops._sdd(xd, v1d, topo)
    hs = topo.with_data(sp.BlockGate(z2, z1, act))
    assert same(ops._dsd(hs, w2d), y.detach()), "y"
    dz1, dz2 = sp.BlockGateGrad(ops._sdd(dy, w2d.t(), topo), z1, z2, act)
    dz1s, dz2s = topo.with_data(dz1), topo.with_data(dz2)
    assert same(ops._dds(xd.t(), dz1s), w1.grad), "dw1"
    assert same(ops._dds(xd.t(), dz2s), v1.grad), "dv1"
    assert same(ops._dsd(hs.t(), dy), w2.grad), "dw2"
    dx = ops._dsd(dz1s, w1d.t())
    ops.dsd_acc(dz2s, v1d.t(), dx)
    assert same(dx, x.grad), "dx"


def test_glu_mlp_weight_views_and_default_activation():
    """Weights held transposed (.t() views of [HIDDEN, K] / [K, HIDDEN]
    tensors), sinks of the held shape, and the default activation (silu)."""
    dtype = "bf16"
    d = _data(dtype)
    x = _dev(d["x"], dtype, True)
    w1_t, v1_t = _dev(d["w1"].T, dtype, True), _dev(d["v1"].T, dtype, True)
    w2_t = _dev(d["w2"].T, dtype, True)
    dy = _dev(d["dy"], dtype)
    topo = _topology(dtype)
    sv = torch.zeros((HIDDEN, K), dtype=torch.float32, device="cuda")
    y = ops.glu_mlp(x, w1_t.t(), v1_t.t(), w2_t.t(), topo, v1_grad_out=sv)
    y.backward(dy)
    x2, w1, v1, w2 = (_dev(d[n], dtype, True) for n in ("x", "w1", "v1", "w2"))
    ref = ops.glu_mlp(x2, w1, v1, w2, topo, "silu")
    ref.backward(dy)
    torch.cuda.synchronize()
    H.assert_close(_np(y), _np(ref), dtype, "y over views")
    H.assert_close(_np(x.grad), _np(x2.grad), dtype, "dx over views")
    H.assert_close(_np(w1_t.grad), _np(w1.grad).T, dtype, "dw1 over views")
    H.assert_close(_np(w2_t.grad), _np(w2.grad).T, dtype, "dw2 over views")
    assert v1_t.grad is None
    H.assert_close(_np(sv), _np(v1.grad).T, dtype, "dv1 sink over a view")


def test_glu_mlp_second_backward_is_refused():
    """dZ2 is written over Z2, so a retained graph cannot run backward twice."""
    dtype = "f16"
    d = _data(dtype)
    x = _dev(d["x"], dtype, True)
    w1, v1, w2 = (_dev(d[n], dtype, True) for n in ("w1", "v1", "w2"))
    y = ops.glu_mlp(x, w1, v1, w2, _topology(dtype))
    dy = _dev(d["dy"], dtype)
    y.backward(dy, retain_graph=True)
    with pytest.raises(RuntimeError):
        y.backward(dy)
