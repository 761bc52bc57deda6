"""GPU: the gated SDD products (sputnik/block/gated.h), H = (A B) * act(G)
with U = A B kept on request, and the pair dU = (A B) * act(G), dG = (A B) *
U * act'(G), on both routes (the 8-wave kernel's fused epilogue and plain SDD
+ the elementwise kernel), and the elementwise kernel on its own.

Expected values come from float64 numpy (tests/gated_ref.py) and the CPU
oracle, never from the library; the criterion for the elementwise stage (two
representable steps, magnitude only below 2^-100) is activation_ref's.
Bit-for-bit comparisons between routes are route checks, not correctness
oracles. Shapes, operands and oracle products are those of
tests/test_gpu_activation.py (shared, computed once, never modified).

Worst step counts seen on MI355X: profiles/sdd_gated/README.md."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import sputnik_amd as sp  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import gated_ref as R  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests.test_gpu_activation import (  # noqa: E402
    B, DTYPES, SMALL_INDICES, SMALL_OFFSETS, TRANSPOSES, Problem, _bits,
    _from_bits, _grouped_problem_data, _small_operands)

pytestmark = pytest.mark.gpu

FORWARD_FACTORS = (1.0, -0.75, 0.375)
GRAD_FACTORS = ((1.0, 1.0), (-0.75, 0.5), (0.375, -1.0))     # (d, U)


@pytest.fixture
def route():
    """Sets the knob "sdd_act_route" for a test and restores it."""
    prev = sp.tuning("sdd_act_route")

    def set_route(r):
        sp.tuning("sdd_act_route", r)
    yield set_route
    sp.tuning("sdd_act_route", prev)


def _same(x: torch.Tensor, y: torch.Tensor) -> bool:
    return torch.equal(x.view(torch.int16), y.view(torch.int16))


def _nan_like(t):
    return torch.full_like(t, float("nan"))


def gated(p: Problem, act, gate, keep_u):
    c, h = p.c()
    u = _nan_like(h) if keep_u else None
    sp.MatmulGated(p.A, p.ta, p.Bm, p.tb, c, act, gate, u)
    return h, u


def gated_grad(p: Problem, act, gate, up, in_place=False):
    c, dg = p.c()
    du = up if in_place else _nan_like(dg)
    sp.MatmulGatedGrad(p.A, p.ta, p.Bm, p.tb, c, act, gate, up, du)
    return dg, du


def _relu_exact(act, worst):
    if act == "relu":
        assert worst == 0, "relu must be bit-exact"


# ---- exhaustive over G ------------------------------------------------------------

_REF = {}


def _exhaustive(dtype):
    """(bits [65536], g float64), computed once."""
    if dtype not in _REF:
        bits = R.all_finite_bits(dtype)
        _REF[dtype] = (bits, R.bits_to_f64(bits, dtype))
    return _REF[dtype]


def _as_blocks(x):
    """[65536] in the order of a [128, 512] matrix -> c's 4 blocks."""
    return np.ascontiguousarray(x.reshape(B, 4, B).transpose(1, 0, 2))


def _const_problem(dtype, f):
    """A = f I (128 x 128), B = ones [128, 512]: acc = f exactly at every
    element; c is 1 x 4 blocks."""
    return Problem(f * np.eye(B), np.ones((B, 4 * B)), False, False, [0, 4],
                   [0, 1, 2, 3], dtype)


@pytest.mark.parametrize("r", [1, 2])
@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_exhaustive_forward(dtype, act, r, route):
    route(r)
    bits, g64 = _exhaustive(dtype)
    gate = _from_bits(_as_blocks(bits), dtype)
    g_blocks = _as_blocks(g64)
    for f in FORWARD_FACTORS:
        p = _const_problem(dtype, f)
        assert sp.sdd_act_route(p.A, False, p.Bm, False, p.c()[0]) == r
        h, u = gated(p, act, gate, keep_u=True)
        h0, _ = gated(p, act, gate, keep_u=False)
        plain = p.plain()
        torch.cuda.synchronize()
        assert _same(u, plain), "the stored U equals the plain SDD"
        assert (u.double() == f).all().item(), "U = f exactly"
        worst = R.check(_bits(h), R.gate64(act, f, g_blocks), dtype,
                        f"H {act} {dtype} f={f} route {r}")
        print(f"worst steps forward {act} {dtype} f={f} route {r}: {worst}")
        _relu_exact(act, worst)
        assert _same(h, h0), "H with and without the U output"
        assert _same(h, sp.BlockGate(u, gate, act)), \
            "H == BlockGate(U, G) bit for bit"


@pytest.mark.parametrize("r", [1, 2])
@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_exhaustive_grad(dtype, act, r, route):
    route(r)
    bits, g64 = _exhaustive(dtype)
    gate = _from_bits(_as_blocks(bits), dtype)
    g_blocks = _as_blocks(g64)
    for d, uc in GRAD_FACTORS:
        p = _const_problem(dtype, d)
        up = torch.full((4, B, B), uc, dtype=p.td, device="cuda")
        dg, du = gated_grad(p, act, gate, up)
        h, _ = gated(p, act, gate, keep_u=False)
        plain = p.plain()
        torch.cuda.synchronize()
        wu = R.check(_bits(du), R.gate_du64(act, d, g_blocks), dtype,
                     f"dU {act} {dtype} d={d} route {r}")
        wg = R.check(_bits(dg), R.gate_dg64(act, d, uc, g_blocks), dtype,
                     f"dG {act} {dtype} d={d} U={uc} route {r}")
        print(f"worst steps grad {act} {dtype} d={d} U={uc} route {r}: "
              f"dU {wu} dG {wg}")
        _relu_exact(act, max(wu, wg))
        eg, eu = sp.BlockGateGrad(plain, gate, up, act)
        assert _same(dg, eg) and _same(du, eu), \
            "(dG, dU) == BlockGateGrad on the plain product"
        assert _same(du, h), "dU == MatmulGated's H for the same operands"


# ---- exhaustive over U (and D) with relu -------------------------------------------

@pytest.mark.parametrize("r", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_exhaustive_up_with_relu(dtype, r, route):
    """A = I, B = every finite pattern: U (or D) runs over every value, G is a
    constant. U relu(G) and D U relu'(G) are single fp32 products, so the
    result is round_T of the float64 product bit for bit; an operand that is
    swapped or read at the wrong offset shows here."""
    route(r)
    bits, x64 = _exhaustive(dtype)
    p = Problem(np.eye(B), x64.reshape(B, 4 * B), False, False, [0, 4],
                [0, 1, 2, 3], dtype)
    x_blocks = _as_blocks(x64)
    for gc in (1.0, 0.375, -2.0):
        gate = torch.full((4, B, B), gc, dtype=p.td, device="cuda")
        h, u = gated(p, "relu", gate, keep_u=True)
        torch.cuda.synchronize()
        on = 1.0 if gc > 0 else 0.0
        u_bits = _as_blocks(bits).copy()
        u_bits[u_bits == 0x8000] = 0       # (the product of -0 is +0)
        assert np.array_equal(_bits(u), u_bits), "U = B exactly"
        ref = R.round_bits_exact(x_blocks * (gc * on) + 0.0, dtype)
        assert np.array_equal(_bits(h), ref), f"H, G = {gc}"
        # dG with D exhaustive, U and G constant; dU = D relu(G)
        for uc in (0.5, -1.0):
            up = torch.full((4, B, B), uc, dtype=p.td, device="cuda")
            dg, du = gated_grad(p, "relu", gate, up)
            torch.cuda.synchronize()
            ref_g = R.round_bits_exact(x_blocks * (uc * on) + 0.0, dtype)
            assert np.array_equal(_bits(dg), ref_g), f"dG, G = {gc}, U = {uc}"
            assert np.array_equal(_bits(du), ref), f"dU, G = {gc}"


# ---- the elementwise kernel alone ---------------------------------------------------

@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_exhaustive_elementwise(dtype, act):
    """BlockGate / BlockGateGrad called directly over every finite G: out of
    place, in place (H over U, H over G; dG over D, dU over U), buffers that
    are not 16-byte aligned with an odd length (the scalar loop, bit for bit
    what the vector loop gave), aligned buffers with n % 8 != 0, and n = 0."""
    bits, g64 = _exhaustive(dtype)
    g = _from_bits(bits, dtype)
    n = g.numel() - 1                                    # odd length

    def unaligned(t, off):
        """A copy of t[:n] that starts `off` elements into an allocation."""
        x = torch.empty(n + 8, dtype=t.dtype, device="cuda")[off:off + n]
        x.copy_(t[:n])
        assert x.data_ptr() % 16 != 0
        return x

    for f in FORWARD_FACTORS:
        u = torch.full_like(g, f)
        h = sp.BlockGate(u, g, act)
        worst = R.check(_bits(h), R.gate64(act, f, g64), dtype,
                        f"gate {act} {dtype} f={f}")
        print(f"worst steps elementwise forward {act} {dtype} f={f}: {worst}")
        _relu_exact(act, worst)
        hs = sp.BlockGate(unaligned(u, 1), unaligned(g, 3), act,
                          out=unaligned(u, 5))           # scalar loop
        assert _same(hs, h[:n])
        ht = sp.BlockGate(u[:n].clone(), g[:n].clone(), act)  # vector + tail
        assert _same(ht, h[:n])
        uc = u.clone()
        sp.BlockGate(uc, g, act, out=uc)                 # in place over u
        assert _same(uc, h)
        if f == FORWARD_FACTORS[0]:
            gc = g.clone()
            sp.BlockGate(u, gc, act, out=gc)             # in place over g
            assert _same(gc, h)
    for d, uval in GRAD_FACTORS:
        dt, ut = torch.full_like(g, d), torch.full_like(g, uval)
        dg, du = sp.BlockGateGrad(dt, g, ut, act)
        wu = R.check(_bits(du), R.gate_du64(act, d, g64), dtype,
                     f"dU {act} {dtype} d={d}")
        wg = R.check(_bits(dg), R.gate_dg64(act, d, uval, g64), dtype,
                     f"dG {act} {dtype} d={d} u={uval}")
        print(f"worst steps elementwise grad {act} {dtype} d={d} u={uval}: "
              f"dU {wu} dG {wg}")
        _relu_exact(act, max(wu, wg))
        sg, su = sp.BlockGateGrad(unaligned(dt, 1), unaligned(g, 3),
                                  unaligned(ut, 5), act, dg=unaligned(dt, 7),
                                  du=unaligned(dt, 2))   # scalar loop
        assert _same(sg, dg[:n]) and _same(su, du[:n])
        tg, tu = sp.BlockGateGrad(dt[:n].clone(), g[:n].clone(),
                                  ut[:n].clone(), act)   # vector + tail
        assert _same(tg, dg[:n]) and _same(tu, du[:n])
        dc, uc = dt.clone(), ut.clone()
        sp.BlockGateGrad(dc, g, uc, act, dg=dc, du=uc)   # dG over D, dU over U
        assert _same(dc, dg) and _same(uc, du)
    assert sp.BlockGate(g[0:0], g[0:0], act).numel() == 0  # n = 0: no launch
    e = sp.BlockGateGrad(g[0:0], g[0:0], g[0:0], act)
    assert e[0].numel() == 0 and e[1].numel() == 0
    torch.cuda.synchronize()


# ---- small topologies and grouped tiles -----------------------------------------------

_SIDE = {}


def _side_buffers(dtype, nb):
    """Random G and U of T for nb blocks, as bits: once per (dtype, nb)."""
    if (dtype, nb) not in _SIDE:
        rng = np.random.default_rng(4242 + nb + (dtype == "bf16"))
        g = R.round_bits(2.0 * rng.standard_normal((nb, B, B)), dtype)
        u = R.round_bits(rng.standard_normal((nb, B, B)), dtype)
        for arr in (g, u):
            arr.setflags(write=False)
        _SIDE[dtype, nb] = (g, u)
    return _SIDE[dtype, nb]


def _check_products(p, ref_full, dtype, acts, what, routes, route):
    """U against the oracle; H, dU and dG against the float64 formulas of the
    device's own U = D = round(acc) from a plain SDD and the random G and U,
    under the criterion; every route in `routes` bit-identical to the first."""
    ref_blocks = p.blocks_of(ref_full)
    g_bits, u_bits = _side_buffers(dtype, p.nb)
    gate, up = _from_bits(g_bits, dtype), _from_bits(u_bits, dtype)
    g64 = R.bits_to_f64(g_bits, dtype).reshape(g_bits.shape)
    u64 = R.bits_to_f64(u_bits, dtype).reshape(u_bits.shape)
    plain = p.plain()
    torch.cuda.synchronize()
    d64 = R.bits_to_f64(_bits(plain), dtype).reshape(plain.shape)
    for b in range(p.nb):
        H.assert_close(d64[b], ref_blocks[b], dtype, f"{what} U block {b}")
    worst = {}
    for act in acts:
        first = None
        for r in routes:
            route(r)
            h, u = gated(p, act, gate, keep_u=True)
            h0, _ = gated(p, act, gate, keep_u=False)
            dg, du = gated_grad(p, act, gate, up)
            torch.cuda.synchronize()
            got = tuple(_bits(t) for t in (u, h, h0, dg, du))
            if first is None:
                first = got
                ub, hb, h0b, dgb, dub = got
                assert np.array_equal(ub, _bits(plain)), f"{what}: U == plain SDD"
                assert np.array_equal(hb, h0b), f"{what}: H with / without U"
                wh = R.check(hb, R.gate64(act, d64, g64), dtype,
                             f"{what} H {act}")
                wu = R.check(dub, R.gate_du64(act, d64, g64), dtype,
                             f"{what} dU {act}")
                wg = R.check(dgb, R.gate_dg64(act, d64, u64, g64), dtype,
                             f"{what} dG {act}")
                worst[act] = (wh, wu, wg)
                if act == "relu":
                    assert max(wh, wu, wg) == 0, "relu must be bit-exact"
            else:
                for name, x, y in zip(("U", "H", "H (no U)", "dG", "dU"),
                                      first, got):
                    assert np.array_equal(x, y), \
                        f"{what}: {name} differs between routes {routes[0]} and {r}"
    print(f"worst steps {what} (H, dU, dG): {worst}")
    return worst


@pytest.mark.parametrize("ta,tb", TRANSPOSES)
@pytest.mark.parametrize("k", [64, 192])
@pytest.mark.parametrize("dtype", DTYPES)
def test_small_ksplit_tile(dtype, k, ta, tb, route):
    """The one-block k-split tile (CfgSdd): K = 64 is one ring slot, 192 an
    odd number of slots; an empty block-row and unsorted columns. Routes 1, 2
    and auto agree bit for bit, and auto is the fused route."""
    a, b, ref = _small_operands(dtype, k)
    p = Problem(a, b, ta, tb, SMALL_OFFSETS, SMALL_INDICES, dtype)
    assert sp.sdd_kernel(p.A, ta, p.Bm, tb, p.c()[0]) == 0
    route(0)
    assert sp.sdd_act_route(p.A, ta, p.Bm, tb, p.c()[0]) == 1  # auto: fused
    _check_products(p, ref, dtype, R.ACTS, f"small {dtype} k={k} {ta}{tb}",
                    (1, 2, 0), route)


GROUPED_CASES = [
    ("f16", "relu", False, False), ("f16", "gelu", False, True),
    ("f16", "silu", True, False), ("bf16", "relu", True, True),
    ("bf16", "gelu", False, False), ("bf16", "silu", False, True)]


@pytest.mark.parametrize("dtype,act,ta,tb", GROUPED_CASES)
def test_grouped_tiles(dtype, act, ta, tb, route):
    """The fused epilogue on the grouped 128 x 512 tiles (CfgSddGrouped),
    groups of 1, 2, 3 and 4 blocks at the row ends, K = 64: the plain SDD runs
    the 8-wave grouped tile (sdd_kernel 1) and auto takes the fused route."""
    a, b, ref, offsets, indices = _grouped_problem_data(dtype)
    p = Problem(a, b, ta, tb, offsets, indices, dtype)
    c = p.c()[0]
    assert sp.sdd_plan(p.A, ta, p.Bm, tb, c) == 1, "grouped tiles not selected"
    assert sp.sdd_kernel(p.A, ta, p.Bm, tb, c) == 1
    route(0)
    assert sp.sdd_act_route(p.A, ta, p.Bm, tb, c) == 1
    _check_products(p, ref, dtype, (act,), f"grouped {dtype} {act} {ta}{tb}",
                    (1, 2, 0), route)


@pytest.mark.parametrize("dtype,act,ta,tb", GROUPED_CASES)
def test_grouped_route2_on_the_4wave_kernel(dtype, act, ta, tb, route):
    """What auto runs at MoE shapes: the plain SDD on the 4-wave grouped
    kernel (forced on with select_dsd_kernel; K = 128, a multiple of 128 as
    that kernel needs; sdd_kernel 3) writing U or D, the elementwise kernel
    behind it. Auto takes route 2 there, and routes 1 (the 8-wave grouped
    tile, fused), 2 and auto give the same bits."""
    a, b, ref, offsets, indices = _grouped_problem_data(dtype, k=128)
    p = Problem(a, b, ta, tb, offsets, indices, dtype)
    c = p.c()[0]
    prev = sp.select_dsd_kernel(5)
    try:
        assert sp.sdd_kernel(p.A, ta, p.Bm, tb, c) == 3, \
            "the 4-wave grouped kernel is not what the plain SDD runs"
        route(0)
        assert sp.sdd_act_route(p.A, ta, p.Bm, tb, c) == 2
        _check_products(p, ref, dtype, (act,),
                        f"grouped 4-wave {dtype} {act} {ta}{tb}", (1, 2, 0),
                        route)
    finally:
        sp.select_dsd_kernel(prev)


# ---- aliasing, graph capture, acceptance -----------------------------------------------

@pytest.mark.parametrize("r", [1, 2])
def test_up_grad_in_place(r, route):
    """up_grad is up: the bits of the out-of-place call."""
    dtype, act = "f16", "silu"
    a, b, _ = _small_operands(dtype, 192)
    p = Problem(a, b, False, False, SMALL_OFFSETS, SMALL_INDICES, dtype)
    g_bits, u_bits = _side_buffers(dtype, p.nb)
    gate, up = _from_bits(g_bits, dtype), _from_bits(u_bits, dtype)
    route(r)
    dg, du = gated_grad(p, act, gate, up)
    up2 = up.clone()
    dg2, du2 = gated_grad(p, act, gate, up2, in_place=True)
    torch.cuda.synchronize()
    assert du2 is up2
    assert _same(dg, dg2) and _same(du, du2)
    assert np.array_equal(_bits(up), u_bits), "the out-of-place call keeps U"


@pytest.mark.parametrize("r", [1, 2])
def test_graph_capture(r, route):
    """Captured once per route, replayed twice: bit-identical to eager."""
    dtype, act = "bf16", "gelu"
    a, b, _ = _small_operands(dtype, 192)
    p = Problem(a, b, False, True, SMALL_OFFSETS, SMALL_INDICES, dtype)
    g_bits, u_bits = _side_buffers(dtype, p.nb)
    gate, up = _from_bits(g_bits, dtype), _from_bits(u_bits, dtype)
    route(r)
    h_e, u_e = gated(p, act, gate, keep_u=True)
    dg_e, du_e = gated_grad(p, act, gate, up)
    torch.cuda.synchronize()
    c1, h = p.c()
    c2, dg = p.c()
    u, du = _nan_like(h), _nan_like(h)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sp.MatmulGated(p.A, p.ta, p.Bm, p.tb, c1, act, gate, u)
        sp.MatmulGatedGrad(p.A, p.ta, p.Bm, p.tb, c2, act, gate, up, du)
    for _ in range(2):
        for t in (h, u, dg, du):
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for x, y in ((h, h_e), (u, u_e), (dg, dg_e), (du, du_e)):
            assert _same(x, y)
    del graph


def test_rejections_launch_nothing():
    a, b, _ = _small_operands("f16", 64)
    p = Problem(a, b, False, False, SMALL_OFFSETS, SMALL_INDICES, "f16")
    c, h = p.c()
    gate, up, du = _nan_like(h), _nan_like(h), _nan_like(h)
    bad = [
        lambda: sp.MatmulGated(p.A, False, p.Bm, False, c, "relu", h),
        lambda: sp.MatmulGated(p.A, False, p.Bm, False, c, "relu", gate, h),
        lambda: sp.MatmulGated(p.A, False, p.Bm, False, c, "relu", gate, gate),
        lambda: sp.MatmulGatedGrad(p.A, False, p.Bm, False, c, "relu", gate,
                                   up, gate),
        lambda: sp.MatmulGatedGrad(p.A, False, p.Bm, False, c, "relu", gate,
                                   up, h),
        lambda: sp.MatmulGatedGrad(p.A, False, p.Bm, False, c, "relu", gate,
                                   h, du),
    ]
    for call in bad:
        with pytest.raises(sp.SputnikError):
            call()
    torch.cuda.synchronize()
    for t in (h, gate, up, du):
        assert torch.isnan(t.float()).all()
