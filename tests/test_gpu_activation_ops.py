"""GPU: ops.sdd_act and ops.mlp (sputnik_amd/ops.py), forward and backward,
with and without gradient sinks, on a 3-expert topology of a few blocks.
Expected values: a float64 dense reference under helpers.assert_close. The
bit-for-bit comparison of mlp with the unfused composition of this library's
own calls (plain SDD, then the elementwise kernels) is a route check, not a
correctness oracle."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import sputnik_amd as sp  # noqa: E402
from sputnik_amd import ops  # noqa: E402
from tests import activation_ref as R  # noqa: E402
from tests import helpers as H  # noqa: E402

pytestmark = pytest.mark.gpu

B = 128
EXPERTS, PER_EXPERT, K = 3, 2, 64
TOKENS, HIDDEN = EXPERTS * B, EXPERTS * PER_EXPERT * B


def _topology(dtype):
    """Block-diagonal: block-row e holds expert e's two block-columns."""
    offsets = torch.arange(0, EXPERTS * PER_EXPERT + 1, PER_EXPERT,
                           dtype=torch.int32, device="cuda")
    indices = torch.arange(EXPERTS * PER_EXPERT, dtype=torch.int16,
                           device="cuda")
    data = torch.empty(EXPERTS * PER_EXPERT, B, B, dtype=H.torch_dtype(dtype),
                       device="cuda")
    return ops.SparseMatrix((TOKENS, HIDDEN), data, offsets, indices)


def _mask():
    m = np.zeros((TOKENS, HIDDEN))
    for e in range(EXPERTS):
        m[e * B:(e + 1) * B, e * PER_EXPERT * B:(e + 1) * PER_EXPERT * B] = 1
    return m


_DATA = {}


def _data(dtype):
    """Operands (rounded to T, float64 copies) once per dtype."""
    if dtype not in _DATA:
        from oracle import oracle as O
        rng = np.random.default_rng(5 + (dtype == "bf16"))

        def make(*shape, scale=1.0):
            return O.round_to((scale * rng.standard_normal(shape)).astype(
                np.float32), dtype).astype(np.float64)
        _DATA[dtype] = dict(x=make(TOKENS, K), w1=make(K, HIDDEN, scale=0.25),
                            w2=make(HIDDEN, K, scale=0.1), dy=make(TOKENS, K),
                            dh=make(TOKENS, HIDDEN))
        for v in _DATA[dtype].values():
            v.setflags(write=False)
    return _DATA[dtype]


def _dev(a, dtype, grad=False):
    t = torch.from_numpy(np.array(a, order="C")).to(H.torch_dtype(dtype)).cuda()
    return t.requires_grad_(grad)


def _np(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("sinks", [False, True])
def test_sdd_act_forward_backward(dtype, act, sinks):
    d = _data(dtype)
    mask = _mask()
    x, w1 = _dev(d["x"], dtype, True), _dev(d["w1"], dtype, True)
    topo = _topology(dtype)
    kw = {}
    if sinks:
        sx = torch.full((TOKENS, K), 0.5, dtype=torch.float32, device="cuda")
        sw = torch.full((K, HIDDEN), 0.5, dtype=torch.float32, device="cuda")
        kw = dict(a_grad_out=sx, b_grad_out=sw)
    h = ops.sdd_act(x, w1, topo, act, **kw)
    z64 = (d["x"] @ d["w1"]) * mask
    H.assert_close(_np(h.to_dense()), R.act64(act, z64) * mask, dtype,
                   f"sdd_act {act} forward")
    dh = topo.with_data(ops.from_dense_mask(
        _dev(d["dh"], dtype), torch.from_numpy(_mask()[::B, ::B] > 0)).data)
    h.data.backward(dh.data)
    dz64 = d["dh"] * mask * R.dact64(act, z64)
    dx64, dw64 = dz64 @ d["w1"].T, d["x"].T @ dz64
    if sinks:
        assert x.grad is None and w1.grad is None
        H.assert_close(_np(sx) - 0.5, dx64, dtype, f"sdd_act {act} dx sink")
        H.assert_close(_np(sw) - 0.5, dw64, dtype, f"sdd_act {act} dw1 sink")
    else:
        H.assert_close(_np(x.grad), dx64, dtype, f"sdd_act {act} dx")
        H.assert_close(_np(w1.grad), dw64, dtype, f"sdd_act {act} dw1")


def test_sdd_act_transposed_topology_view():
    """A .t() view of the topology stores the product transposed, as _sdd."""
    dtype, act = "f16", "silu"
    d = _data(dtype)
    topo = _topology(dtype)
    a, b = _dev(d["w1"].T, dtype), _dev(d["x"].T, dtype)   # (x w1)^T = w1^T x^T
    h_t = ops.sdd_act(a, b, topo.t(), act)
    h = ops.sdd_act(_dev(d["x"], dtype), _dev(d["w1"], dtype), topo, act)
    assert h_t.shape == (HIDDEN, TOKENS)
    H.assert_close(_np(h_t.to_dense()), _np(h.to_dense()).T, dtype,
                   "sdd_act over a transposed view")


@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("sinks", [False, True])
def test_mlp_forward_backward(dtype, act, sinks):
    d = _data(dtype)
    mask = _mask()
    x = _dev(d["x"], dtype, True)
    w1, w2 = _dev(d["w1"], dtype, True), _dev(d["w2"], dtype, True)
    dy = _dev(d["dy"], dtype)
    topo = _topology(dtype)
    kw = {}
    if sinks:
        s1 = torch.full((K, HIDDEN), 0.5, dtype=torch.float32, device="cuda")
        s2 = torch.full((HIDDEN, K), 0.5, dtype=torch.float32, device="cuda")
        kw = dict(w1_grad_out=s1, w2_grad_out=s2)
    y = ops.mlp(x, w1, w2, topo, act, **kw)
    y.backward(dy)
    torch.cuda.synchronize()

    z64 = (d["x"] @ d["w1"]) * mask
    h64 = R.act64(act, z64) * mask
    dz64 = (d["dy"] @ d["w2"].T) * mask * R.dact64(act, z64)
    H.assert_close(_np(y), h64 @ d["w2"], dtype, f"mlp {act} y")
    H.assert_close(_np(x.grad), dz64 @ d["w1"].T, dtype, f"mlp {act} dx")
    dw1_64, dw2_64 = d["x"].T @ dz64, h64.T @ d["dy"]
    if sinks:
        assert w1.grad is None and w2.grad is None
        H.assert_close(_np(s1) - 0.5, dw1_64, dtype, f"mlp {act} dw1 sink")
        H.assert_close(_np(s2) - 0.5, dw2_64, dtype, f"mlp {act} dw2 sink")
        return
    H.assert_close(_np(w1.grad), dw1_64, dtype, f"mlp {act} dw1")
    H.assert_close(_np(w2.grad), dw2_64, dtype, f"mlp {act} dw2")

    # Route check: the unfused composition of the library's own calls.
    xd, w1d, w2d = x.detach(), w1.detach(), w2.detach()
    z = ops._sdd(xd, w1d, topo)
    hs = topo.with_data(sp.BlockActivation(z, act))
    same = lambda p, q: torch.equal(p.view(torch.int16), q.view(torch.int16))
    assert same(ops._dsd(hs, w2d), y.detach()), "y"
    dz_fused = ops._sdd_act(dy, w2d.t(), topo, sp._act_code(act), z=z,
                            grad=True)
    dz = sp.BlockActivationGrad(ops._sdd(dy, w2d.t(), topo), z, act)
    assert same(dz_fused, dz), "dZ: fused product vs plain SDD + gate"
    dzs = topo.with_data(dz)
    assert same(ops._dsd(dzs, w1d.t()), x.grad), "dx"
    assert same(ops._dds(xd.t(), dzs), w1.grad), "dw1"
    assert same(ops._dsd(hs.t(), dy), w2.grad), "dw2"
