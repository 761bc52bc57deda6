"""GPU: the SDD activation products (sputnik/block/activation.h),
H = act(A B) with the pre-activation Z kept on request, and
C = (A B) * act'(Z), on both routes (the 8-wave kernel's fused epilogue and
plain SDD + the elementwise kernel), and the elementwise kernel on its own.

Expected values come from float64 numpy (tests/activation_ref.py) and the CPU
oracle, never from the library; the criterion for the elementwise stage (two
representable steps, magnitude only below 2^-100) is stated there. Bit-for-bit
comparisons between routes are route checks, not correctness oracles.

Worst step counts seen on MI355X: profiles/sdd_activation/README.md."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import sputnik_amd as sp  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import activation_ref as R  # noqa: E402
from tests import helpers as H  # noqa: E402

pytestmark = pytest.mark.gpu

B = 128
DTYPES = ("f16", "bf16")
TRANSPOSES = [(False, False), (False, True), (True, False), (True, True)]


# ---- plumbing ---------------------------------------------------------------

def _bits(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _from_bits(bits: np.ndarray, dtype: str) -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).copy())
    return t.view(H.torch_dtype(dtype)).cuda()


@pytest.fixture
def route():
    """Sets the knob "sdd_act_route" for a test and restores it."""
    prev = sp.tuning("sdd_act_route")

    def set_route(r):
        sp.tuning("sdd_act_route", r)
    yield set_route
    sp.tuning("sdd_act_route", prev)


class Problem:
    """op(A) [M, K] times op(B) [K, N] at a given topology; A and B are
    stored transposed when their flag is set."""

    def __init__(self, a_math, b_math, ta, tb, offsets, indices, dtype):
        td = H.torch_dtype(dtype)
        self.dtype, self.ta, self.tb = dtype, ta, tb
        self.m, self.k = a_math.shape
        self.n = b_math.shape[1]
        a_st = np.array(a_math.T if ta else a_math, order="C")  # (copies)
        b_st = np.array(b_math.T if tb else b_math, order="C")
        self.a_dev = torch.from_numpy(a_st).to(td).cuda()
        self.b_dev = torch.from_numpy(b_st).to(td).cuda()
        self.A = sp.Matrix(a_st.shape[0], a_st.shape[1], self.a_dev)
        self.Bm = sp.Matrix(b_st.shape[0], b_st.shape[1], self.b_dev)
        self.offsets = np.asarray(offsets, dtype=np.int32)
        self.indices = np.asarray(indices, dtype=np.int16)
        self.nb = int(self.indices.size)
        self.off_dev = torch.from_numpy(self.offsets).cuda()
        self.idx_dev = torch.from_numpy(self.indices).cuda()
        self.row_indices = None
        self.td = td

    def c(self, data=None):
        if data is None:
            data = torch.full((self.nb, B, B), float("nan"), dtype=self.td,
                              device="cuda")
        m = sp.BlockMatrix(self.m, self.n, B, self.nb * B * B, data,
                           self.off_dev, self.idx_dev)
        if self.row_indices is None:
            sp.AllocateRowIndicesBuffer(m)
            sp.RowIndices(m, m.row_indices)
            self.row_indices = m.row_indices
        m.row_indices = self.row_indices
        return m, data

    def plain(self):
        c, data = self.c()
        sp.Matmul(self.A, self.ta, self.Bm, self.tb, c)
        return data

    def forward(self, act, keep_z):
        c, h = self.c()
        z = torch.full_like(h, float("nan")) if keep_z else None
        sp.MatmulActivation(self.A, self.ta, self.Bm, self.tb, c, act, z)
        return h, z

    def grad(self, act, z):
        c, out = self.c()
        sp.MatmulActivationGrad(self.A, self.ta, self.Bm, self.tb, c, act, z)
        return out

    def blocks_of(self, full):
        """A dense [M, N] array -> its stored blocks [nb, 128, 128]."""
        rows = np.repeat(np.arange(self.offsets.size - 1), np.diff(self.offsets))
        return np.stack([full[r * B:(r + 1) * B, c * B:(c + 1) * B]
                         for r, c in zip(rows, self.indices)]) \
            if self.nb else np.zeros((0, B, B))


# ---- exhaustive known-answer test ---------------------------------------------

_REF = {}


def _exhaustive(dtype):
    """(bits [65536], z float64, {act: (act64, dact64)}), computed once."""
    if dtype not in _REF:
        bits = R.all_finite_bits(dtype)
        z = R.bits_to_f64(bits, dtype)
        _REF[dtype] = (bits, z, {a: (R.act64(a, z), R.dact64(a, z))
                                 for a in R.ACTS})
    return _REF[dtype]


def _kat_problem(dtype, g):
    """A = g I (128 x 128), B [128, 512] = every pattern of T: A B = g B
    exactly; c is 1 x 4 blocks, block j = B[:, 128 j : 128 j + 128]."""
    bits, z, _ = _exhaustive(dtype)
    b_math = z.reshape(B, 4 * B)
    p = Problem(g * np.eye(B), b_math, False, False, [0, 4], [0, 1, 2, 3],
                dtype)
    z_blocks = bits.reshape(B, 4, B).transpose(1, 0, 2).copy()  # [4, 128, 128]
    # (the product of -0 is +0: an fp32 accumulator that starts at +0)
    z_blocks[z_blocks == 0x8000] = 0
    return p, z_blocks


def _relu_exact(act, worst):
    if act == "relu":
        assert worst == 0, "relu must be bit-exact"


@pytest.mark.parametrize("r", [1, 2])
@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_exhaustive_forward(dtype, act, r, route):
    route(r)
    _, _, refs = _exhaustive(dtype)
    p, z_bits = _kat_problem(dtype, 1.0)
    assert sp.sdd_act_route(p.A, False, p.Bm, False, p.c()[0]) == r
    h, z = p.forward(act, keep_z=True)
    h0, _ = p.forward(act, keep_z=False)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(z), z_bits), "Z = B exactly"
    ref = refs[act][0].reshape(B, 4, B).transpose(1, 0, 2)
    worst = R.check(_bits(h), ref, dtype, f"H {act} {dtype} route {r}")
    print(f"worst steps forward {act} {dtype} route {r}: {worst}")
    _relu_exact(act, worst)
    assert torch.equal(h.view(torch.int16), h0.view(torch.int16)), \
        "H with and without the Z output"
    he = sp.BlockActivation(z, act)
    assert torch.equal(h.view(torch.int16), he.view(torch.int16)), \
        "H == BlockActivation(Z) bit for bit"


@pytest.mark.parametrize("r", [1, 2])
@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_exhaustive_grad(dtype, act, r, route):
    route(r)
    bits, z64, refs = _exhaustive(dtype)
    d64 = refs[act][1].reshape(B, 4, B).transpose(1, 0, 2)
    for g in (1.0, -3.0, 0.375):
        # A B = g at every element: A = g I, B = ones; Z exhaustive
        p = Problem(g * np.eye(B), np.ones((B, 4 * B)), False, False, [0, 4],
                    [0, 1, 2, 3], dtype)
        z = _from_bits(np.ascontiguousarray(
            bits.reshape(B, 4, B).transpose(1, 0, 2)), dtype)
        out = p.grad(act, z)
        torch.cuda.synchronize()
        worst = R.check(_bits(out), g * d64, dtype,
                        f"C {act} {dtype} g={g} route {r}")
        print(f"worst steps grad {act} {dtype} g={g} route {r}: {worst}")
        _relu_exact(act, worst)
        gate = sp.BlockActivationGrad(torch.full_like(z, g), z, act)
        assert torch.equal(out.view(torch.int16), gate.view(torch.int16))


@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_exhaustive_elementwise(dtype, act):
    """The elementwise kernel called directly: out of place, in place, and,
    for both forms, over buffers that are not 16-byte aligned with an odd
    length (the scalar loop, which evaluates one element at a time where the
    vector loop evaluates packed pairs): every finite input again, bit for
    bit what the vector loop gave."""
    bits, z64, refs = _exhaustive(dtype)
    z = _from_bits(bits, dtype)
    h = sp.BlockActivation(z, act)
    worst = R.check(_bits(h), refs[act][0], dtype, f"act {act} {dtype}")
    print(f"worst steps elementwise forward {act} {dtype}: {worst}")
    _relu_exact(act, worst)
    n = z.numel() - 1                                    # odd length

    def unaligned(t, off):
        """A copy of t[:n] that starts `off` elements into an allocation."""
        u = torch.empty(n + 8, dtype=t.dtype, device="cuda")[off:off + n]
        u.copy_(t[:n])
        assert u.data_ptr() % 16 != 0
        return u

    for g in (1.0, -3.0, 0.375):
        gt = torch.full_like(z, g)
        d = sp.BlockActivationGrad(gt, z, act)
        worst = R.check(_bits(d), g * refs[act][1], dtype,
                        f"gate {act} {dtype} g={g}")
        print(f"worst steps elementwise gate {act} {dtype} g={g}: {worst}")
        _relu_exact(act, worst)
        ds = sp.BlockActivationGrad(unaligned(gt, 1), unaligned(z, 3), act,
                                    out=unaligned(gt, 5))   # scalar gate
        assert torch.equal(ds.view(torch.int16), d[:n].view(torch.int16))
        if g == 1.0:
            zc = z.clone()
            sp.BlockActivationGrad(gt, zc, act, out=zc)  # in place over z
            assert torch.equal(zc.view(torch.int16), d.view(torch.int16))
        sp.BlockActivationGrad(gt, z, act, out=gt)       # in place over g
        assert torch.equal(gt.view(torch.int16), d.view(torch.int16))
    zc = z.clone()
    sp.BlockActivation(zc, act, out=zc)                  # in place over z
    assert torch.equal(zc.view(torch.int16), h.view(torch.int16))
    assert sp.BlockActivation(z[0:0], act).numel() == 0  # n = 0: no launch
    hs = sp.BlockActivation(unaligned(z, 3), act, out=unaligned(z, 1))
    assert torch.equal(hs.view(torch.int16), h[:n].view(torch.int16))
    # aligned buffers, n % 8 != 0: the vector loop and the scalar tail
    ht = sp.BlockActivation(z[:n].clone(), act)
    assert torch.equal(ht.view(torch.int16), h[:n].view(torch.int16))


# ---- small topologies ----------------------------------------------------------

# 384 x 640: block-rows of 4, 0 and 3 blocks, columns unsorted.
SMALL_OFFSETS = [0, 4, 4, 7]
SMALL_INDICES = [3, 0, 4, 1, 2, 4, 0]

_SMALL = {}


def _small_operands(dtype, k):
    """A [384, k], B [k, 640] (rounded to T) and the oracle product, once per
    (dtype, k); shared by every transpose and never modified."""
    key = (dtype, k)
    if key not in _SMALL:
        rng = np.random.default_rng(1000 + k + (dtype == "bf16"))
        a = O.round_to(rng.standard_normal((384, k)).astype(np.float32), dtype)
        b = O.round_to(rng.standard_normal((k, 640)).astype(np.float32), dtype)
        ref = O.gemm(a, False, b, False)
        for arr in (a, b, ref):
            arr.setflags(write=False)
        _SMALL[key] = (a, b, ref)
    return _SMALL[key]


def _check_products(p, ref_full, dtype, acts, what, routes, route):
    """Z against the oracle; H and C against float64 act / act' of the device
    Z and g = round(acc) from a plain SDD, under the criterion; every route
    in `routes` bit-identical to the first."""
    ref_blocks = p.blocks_of(ref_full)
    g = p.plain()
    torch.cuda.synchronize()
    g64 = R.bits_to_f64(_bits(g), dtype).reshape(g.shape)
    worst = {}
    for act in acts:
        first = None
        for r in routes:
            route(r)
            h, z = p.forward(act, keep_z=True)
            h0, _ = p.forward(act, keep_z=False)
            c = p.grad(act, z)
            torch.cuda.synchronize()
            got = tuple(_bits(t) for t in (z, h, h0, c))
            if first is None:
                first = got
                zb, hb, h0b, cb = got
                assert np.array_equal(zb, _bits(g)), f"{what}: Z == plain SDD"
                z64 = R.bits_to_f64(zb, dtype).reshape(z.shape)
                for b in range(p.nb):
                    H.assert_close(z64[b], ref_blocks[b], dtype,
                                   f"{what} Z block {b}")
                assert np.array_equal(hb, h0b), f"{what}: H with / without Z"
                wf = R.check(hb, R.act64(act, z64), dtype, f"{what} H {act}")
                wg = R.check(cb, g64 * R.dact64(act, z64), dtype,
                             f"{what} C {act}")
                worst[act] = (wf, wg)
                if act == "relu":
                    assert wf == 0 and wg == 0, "relu must be bit-exact"
            else:
                for name, x, y in zip(("Z", "H", "H (no Z)", "C"), first, got):
                    assert np.array_equal(x, y), \
                        f"{what}: {name} differs between routes {routes[0]} and {r}"
    print(f"worst steps {what}: {worst}")
    return worst


@pytest.mark.parametrize("ta,tb", TRANSPOSES)
@pytest.mark.parametrize("k", [64, 192])
@pytest.mark.parametrize("dtype", DTYPES)
def test_small_ksplit_tile(dtype, k, ta, tb, route):
    """The one-block k-split tile (CfgSdd): K = 64 is one ring slot, 192 an
    odd number of slots, so both k-halves are covered; an empty block-row and
    unsorted columns. Routes 1, 2 and auto agree bit for bit."""
    a, b, ref = _small_operands(dtype, k)
    p = Problem(a, b, ta, tb, SMALL_OFFSETS, SMALL_INDICES, dtype)
    assert sp.sdd_kernel(p.A, ta, p.Bm, tb, p.c()[0]) == 0
    route(0)
    assert sp.sdd_act_route(p.A, ta, p.Bm, tb, p.c()[0]) == 1  # auto: fused
    _check_products(p, ref, dtype, R.ACTS, f"small {dtype} k={k} {ta}{tb}",
                    (1, 2, 0), route)


# ---- grouped tiles -------------------------------------------------------------

_GROUPED = {}


def _grouped_problem_data(dtype, k=64):
    """32 block-rows (the smallest shape that reaches UseGroupedSdd's
    threshold of 4 blocks per CU), per-row counts = 1, 2, 3, 0 mod 4.
    Operands and oracle product once per (dtype, K)."""
    if (dtype, k) not in _GROUPED:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        base = 4 * ((4 * cus + 31) // 32 // 4 + 1)      # multiple of 4
        counts = [base + (r % 4 + 1) % 4 for r in range(32)]  # 1, 2, 3, 0
        ncols = base + 3
        assert sum(counts) >= 4 * cus
        rng = np.random.default_rng(77 + k + (dtype == "bf16"))
        offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        indices = np.concatenate([
            rng.permutation(ncols)[:n] for n in counts]).astype(np.int16)
        m, n = 32 * B, ncols * B
        a = O.round_to(rng.standard_normal((m, k)).astype(np.float32), dtype)
        b = O.round_to(rng.standard_normal((k, n)).astype(np.float32), dtype)
        ref = O.gemm(a, False, b, False)
        for arr in (a, b, ref):
            arr.setflags(write=False)
        _GROUPED[dtype, k] = (a, b, ref, offsets, indices)
    return _GROUPED[dtype, k]


@pytest.mark.parametrize("dtype,act,ta,tb", [
    ("f16", "relu", False, False), ("f16", "gelu", False, True),
    ("f16", "silu", True, False), ("bf16", "relu", True, True),
    ("bf16", "gelu", False, False), ("bf16", "silu", False, True)])
def test_grouped_tiles(dtype, act, ta, tb, route):
    """The fused epilogue on the grouped 128 x 512 tiles (CfgSddGrouped),
    groups of 1, 2, 3 and 4 blocks at the row ends, K = 64. At this K the
    4-wave kernel does not apply (it needs K % 128 == 0), so the plain SDD
    runs the 8-wave grouped tile (sdd_kernel 1), auto takes the fused route,
    and route 2 is that tile plus the elementwise kernel; the 4-wave kernel
    under route 2 is test_grouped_route2_on_the_4wave_kernel."""
    a, b, ref, offsets, indices = _grouped_problem_data(dtype)
    p = Problem(a, b, ta, tb, offsets, indices, dtype)
    c = p.c()[0]
    assert sp.sdd_plan(p.A, ta, p.Bm, tb, c) == 1, "grouped tiles not selected"
    assert sp.sdd_kernel(p.A, ta, p.Bm, tb, c) == 1
    route(0)
    assert sp.sdd_act_route(p.A, ta, p.Bm, tb, c) == 1
    _check_products(p, ref, dtype, (act,), f"grouped {dtype} {act} {ta}{tb}",
                    (1, 2, 0), route)


@pytest.mark.parametrize("dtype,act,ta,tb", [
    ("f16", "gelu", False, False), ("bf16", "silu", False, True),
    ("bf16", "gelu", False, False), ("f16", "relu", False, True)])
def test_grouped_route2_on_the_4wave_kernel(dtype, act, ta, tb, route):
    """What auto runs at MoE shapes: the plain SDD on the 4-wave grouped
    kernel (forced on with select_dsd_kernel; K = 128, a multiple of 128 as
    that kernel needs; sdd_kernel 3) writing Z or C, the elementwise kernel
    behind it. Auto takes route 2 there, and routes 1 (the 8-wave grouped
    tile, fused), 2 and auto give bit-identical Z, H and C, all checked
    against the oracle and the float64 formulas."""
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


# ---- graph capture ---------------------------------------------------------------

@pytest.mark.parametrize("r", [1, 2])
def test_graph_capture(r, route):
    """Captured once per route, replayed twice: bit-identical to eager."""
    dtype, act = "bf16", "gelu"
    a, b, _ = _small_operands(dtype, 192)
    p = Problem(a, b, False, True, SMALL_OFFSETS, SMALL_INDICES, dtype)
    route(r)
    h_e, z_e = p.forward(act, keep_z=True)
    c_e = p.grad(act, z_e)
    torch.cuda.synchronize()
    c1, h = p.c()
    c2, c_out = p.c()
    z = torch.full_like(h, float("nan"))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sp.MatmulActivation(p.A, p.ta, p.Bm, p.tb, c1, act, z)
        sp.MatmulActivationGrad(p.A, p.ta, p.Bm, p.tb, c2, act, z)
    for _ in range(2):
        for t in (h, z, c_out):
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for x, y in ((h, h_e), (z, z_e), (c_out, c_e)):
            assert torch.equal(x.view(torch.int16), y.view(torch.int16))
    del graph


# ---- acceptance on the device ----------------------------------------------------

def test_rejections_launch_nothing():
    a, b, _ = _small_operands("f16", 64)
    p = Problem(a, b, False, False, SMALL_OFFSETS, SMALL_INDICES, "f16")
    c, h = p.c()
    with pytest.raises(sp.SputnikError):       # z must not be c.data
        sp.MatmulActivationGrad(p.A, False, p.Bm, False, c, "relu", h)
    torch.cuda.synchronize()
    assert torch.isnan(h.float()).all()
