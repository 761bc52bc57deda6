"""Gradient sinks of the differentiable ops (sputnik_amd/ops.py) and the raw
in-place forms dsd_acc / dds_acc.

Integer operands (-1, 0, 1) in fp16 over a masked topology, x [512 x 256]
and w [256 x 1024]: every gradient is a sum of at most 1024 products of such
values, so it is an exact integer in fp16 and in fp32, and a sink preset to
integers S0 in [-8, 8] must hold S0 + g exactly (|S0 + g| <= 1032 < 2048),
where g is the gradient the same op gives without a sink.
"""

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected here, skipped: no device
    pytest.skip("no GPU", allow_module_level=True)

import sputnik_amd as sp  # noqa: E402
from sputnik_amd import ops  # noqa: E402

sp.lib()

T = torch.float16
M, K, N = 512, 256, 1024
SINK_TYPES = [torch.float32, T]


def _ints(gen, *shape, lo=-1, hi=1):
    return torch.randint(lo, hi + 1, shape, generator=gen,
                         device="cuda").to(T)


@pytest.fixture(scope="module")
def data():
    gen = torch.Generator(device="cuda").manual_seed(3)
    mask = torch.rand(M // 128, N // 128, generator=gen, device="cuda") < 0.5
    mask[:, 0] = True
    mask[1, :] = False          # an empty block-row
    mask[1, 3] = True
    mask[:, 5] = False          # an empty block-column
    d = {
        "x": _ints(gen, M, K), "w": _ints(gen, K, N),
        "w2": _ints(gen, N, K), "xt": _ints(gen, K, M),
        "h": ops.from_dense_mask(_ints(gen, M, N), mask),
        "dh": _ints(gen, int(mask.sum()), 128, 128),
        "dy": _ints(gen, M, K), "dz": _ints(gen, K, N),
    }
    return d


def _leaf(t):
    return t.clone().requires_grad_()


def _s0(shape, dtype, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(-8, 9, shape, generator=gen,
                         device="cuda").to(dtype)


def _same(got, want, what):
    torch.cuda.synchronize()
    assert got.dtype == want.dtype and torch.equal(got, want), what


@pytest.mark.parametrize("sinks", ["a", "b", "ab"])
@pytest.mark.parametrize("sink_type", SINK_TYPES)
def test_sdd_sinks(data, sink_type, sinks):
    topo = data["h"]
    x0, w0 = _leaf(data["x"]), _leaf(data["w"])
    ops.sdd(x0, w0, topo).data.backward(data["dh"])
    x1, w1 = _leaf(data["x"]), _leaf(data["w"])
    sa = _s0((M, K), sink_type, 1) if "a" in sinks else None
    sb = _s0((K, N), sink_type, 2) if "b" in sinks else None
    sa0 = None if sa is None else sa.clone()
    sb0 = None if sb is None else sb.clone()
    ops.sdd(x1, w1, topo, a_grad_out=sa, b_grad_out=sb).data.backward(
        data["dh"])
    if sa is None:
        _same(x1.grad, x0.grad, "dx unchanged")
    else:
        assert x1.grad is None
        _same(sa, (sa0.double() + x0.grad.double()).to(sink_type), "x sink")
    if sb is None:
        _same(w1.grad, w0.grad, "dw unchanged")
    else:
        assert w1.grad is None
        _same(sb, (sb0.double() + w0.grad.double()).to(sink_type), "w sink")


@pytest.mark.parametrize("view", ["contiguous", "t_view"])
@pytest.mark.parametrize("sink_type", SINK_TYPES)
def test_dsd_sink(data, sink_type, view):
    """y = h @ b. As a .t() view of the weight the caller holds ([K x N]),
    the sink has the weight's shape and receives the weight's gradient."""
    h = data["h"]
    held = data["w"] if view == "t_view" else data["w2"]
    as_operand = (lambda t: t.t()) if view == "t_view" else (lambda t: t)
    hd0, b0 = _leaf(h.data), _leaf(held)
    ops.dsd(h.with_data(hd0), as_operand(b0)).backward(data["dy"])
    hd1, b1 = _leaf(h.data), _leaf(held)
    sink = _s0(tuple(held.shape), sink_type, 4)
    s0 = sink.clone()
    ops.dsd(h.with_data(hd1), as_operand(b1),
            b_grad_out=sink).backward(data["dy"])
    assert b1.grad is None
    _same(sink, (s0.double() + b0.grad.double()).to(sink_type),
          f"dsd b sink {view}")
    _same(hd1.grad, hd0.grad, "sparse gradient unchanged")


@pytest.mark.parametrize("view", ["contiguous", "t_view"])
@pytest.mark.parametrize("sink_type", SINK_TYPES)
def test_dds_sink(data, sink_type, view):
    """z = a @ h with a [K x M]; as a .t() view of x [M x K] the sink has
    x's shape."""
    h = data["h"]
    held = data["x"] if view == "t_view" else data["xt"]
    as_operand = (lambda t: t.t()) if view == "t_view" else (lambda t: t)
    a0, hd0 = _leaf(held), _leaf(h.data)
    ops.dds(as_operand(a0), h.with_data(hd0)).backward(data["dz"])
    a1, hd1 = _leaf(held), _leaf(h.data)
    sink = _s0(tuple(held.shape), sink_type, 5)
    s0 = sink.clone()
    ops.dds(as_operand(a1), h.with_data(hd1),
            a_grad_out=sink).backward(data["dz"])
    assert a1.grad is None
    _same(sink, (s0.double() + a0.grad.double()).to(sink_type),
          f"dds a sink {view}")
    _same(hd1.grad, hd0.grad, "sparse gradient unchanged")


def test_sink_is_checked(data):
    with pytest.raises(ValueError):
        ops.dsd(data["h"], data["w2"],
                b_grad_out=torch.zeros(K, N, device="cuda"))  # shape
    with pytest.raises(TypeError):
        ops.dsd(data["h"], data["w2"],
                b_grad_out=torch.zeros(N, K, dtype=torch.bfloat16,
                                       device="cuda"))
    with pytest.raises(ValueError):
        ops.dds(data["xt"], data["h"],
                a_grad_out=torch.zeros(M, K, device="cuda").t())


@pytest.mark.parametrize("sink_type", SINK_TYPES)
def test_raw_acc_forms(data, sink_type):
    """dsd_acc / dds_acc return `out`; exact, and the rows (columns) that meet
    no block keep their bits."""
    h = data["h"]
    hd = h.to_dense().double()
    out = _s0((M, K), sink_type, 6)
    o0 = out.clone()
    assert ops.dsd_acc(h, data["w2"], out) is out
    _same(out, (o0.double() + hd @ data["w2"].double()).to(sink_type),
          "dsd_acc")
    out = _s0((K, N), sink_type, 7)
    out[:, 5 * 128:6 * 128] = float("nan")
    o0 = out.clone()
    assert ops.dds_acc(data["xt"], h, out) is out
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[:, 5 * 128:6 * 128]).all())
    want = (o0.double() + data["xt"].double() @ hd).to(sink_type)
    keep = torch.ones_like(out, dtype=torch.bool)
    keep[:, 5 * 128:6 * 128] = False
    _same(torch.where(keep, out, torch.zeros_like(out)),
          torch.where(keep, want, torch.zeros_like(want)), "dds_acc")
    # the transposed view of the sparse operand: out += h^T @ dy
    out = _s0((N, K), sink_type, 8)
    o0 = out.clone()
    assert ops.dsd_acc(h.t(), data["dy"], out) is out
    want = (o0.double() + hd.t() @ data["dy"].double()).to(sink_type)
    _same(out, want, "dsd_acc transposed")
