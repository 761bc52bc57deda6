"""The accumulating DSD / DDS products, C += op(A) op(B) into a C of the
operand type or of fp32 (sputnik/block/accumulate.h), checked bit-exactly.

Conventions of tests/test_gpu_kat.py: operands are integers in {-1, 0, 1},
C_in integers in [-8, 8], so every partial sum of the fp32 accumulation, the
add of C_in and the final rounding are exact, and the expected output is
float64(op(A) @ op(B)) + C_in, compared with torch.equal on the whole
output. For a C of the operand type max|sum| + 8 stays inside the exact
integer range: fp16 (2048) with K <= 1024; bf16 (256) with K = 256 and the
dense operand zero on odd k, so |sum| <= 128. With an fp32 C every K used
here is exact. Each product (operands and the float64 reference) is built
once and shared by the tests that use it; no test changes it.
"""

import functools

import numpy as np
import pytest

from sputnik_amd import matrix_utils as mu

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected here, skipped: no device
    pytest.skip("no GPU", allow_module_level=True)

import sputnik_amd as sp  # noqa: E402
from tests import helpers as H  # noqa: E402

sp.lib()  # fail loudly if the native library is missing

B = mu.BLOCK
TD = {"f16": torch.float16, "bf16": torch.bfloat16}
TRANSPOSES = [(False, False), (False, True), (True, False), (True, True)]
C_TYPES = ["operand", "f32"]


def _ints(rng, shape):
    return rng.integers(-1, 2, size=shape).astype(np.float32)


def _to_device(host, dtype):
    return host.to(TD[dtype]).cuda()


class ISparse:
    """BCSR operand with integer values: host dense copy + device matrix
    (tests/test_gpu_kat.py), with the transposed metadata built."""

    def __init__(self, rows, cols, density, rng, dtype, topology=None,
                 values=_ints, place=_to_device):
        self.rows, self.cols = rows, cols
        if topology is not None:
            self.offsets, self.indices = topology
            nb = int(self.offsets[-1])
        else:
            nb = mu.nonzeros_for_density(rows, cols, density) // (B * B)
            self.offsets, self.indices = mu.random_topology(
                rows // B, cols // B, nb, rng, unordered=True)
        self.values = values(rng, (nb, B, B))
        self.dense = mu.to_dense(rows, cols, self.offsets, self.indices,
                                 self.values)
        self.dev = place(torch.from_numpy(self.values), dtype)
        self.m = sp.BlockMatrix(
            rows, cols, 128, nb * B * B, self.dev,
            torch.from_numpy(self.offsets.astype(np.int32)).cuda(),
            torch.from_numpy(self.indices.astype(np.int16)).cuda())
        sp.AllocateTransposeBuffers(self.m)
        sp.Transpose(self.m)


class IDense:
    def __init__(self, rows, cols, rng, dtype, zero_odd_axis=None,
                 values=_ints, place=_to_device):
        self.values = values(rng, (rows, cols))
        if zero_odd_axis == 0:
            self.values[1::2, :] = 0
        elif zero_odd_axis == 1:
            self.values[:, 1::2] = 0
        self.dev = place(torch.from_numpy(self.values), dtype)
        self.m = sp.Matrix(rows, cols, self.dev)


def _op(x, t):
    return x.T if t else x


def _equal(got, want, what):
    torch.cuda.synchronize()
    if not torch.equal(got, want):
        bad = (got != want)
        n = int(bad.sum())
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {n} of {got.numel()} elements differ, "
                             f"first at {idx}: got {got[tuple(idx)].item()} "
                             f"want {want[tuple(idx)].item()}")


class Problem:
    """C[m x n] += op(A)[m x k] op(B)[k x n]; A sparse for "dsd", B sparse
    for "dds". `topology`: the stored sparse operand's (offsets, indices).
    even_k: the dense operand is zero on odd k (bf16 bound, module doc)."""

    def __init__(self, op, m, k, n, ta, tb, dtype, density=0.5, seed=0,
                 topology=None, even_k=None):
        rng = np.random.default_rng(seed)
        self.op, self.m, self.k, self.n = op, m, k, n
        self.ta, self.tb, self.dtype = ta, tb, dtype
        if even_k is None:
            even_k = dtype == "bf16"
        a_shape = (k, m) if ta else (m, k)
        b_shape = (n, k) if tb else (k, n)
        if op == "dsd":
            self.S = ISparse(*a_shape, density, rng, dtype, topology=topology)
            k_axis = 1 if tb else 0
            self.D = IDense(*b_shape, rng, dtype,
                            zero_odd_axis=k_axis if even_k else None)
            a64, b64 = self.S.dense, self.D.values
        else:
            k_axis = 0 if ta else 1
            self.D = IDense(*a_shape, rng, dtype,
                            zero_odd_axis=k_axis if even_k else None)
            self.S = ISparse(*b_shape, density, rng, dtype, topology=topology)
            a64, b64 = self.D.values, self.S.dense
        self.P = _op(a64, ta).astype(np.float64) @ _op(b64, tb)
        self.S.dense = None  # (host copy no longer needed)
        self.rng = rng

    def c_in(self, c_type, seed=0):
        """(host float64, device tensor) of integers in [-8, 8]."""
        rng = np.random.default_rng(1000 + seed)
        host = rng.integers(-8, 9, size=(self.m, self.n)).astype(np.float64)
        return host, self.tensor(host, c_type)

    def tensor(self, host64, c_type):
        td = torch.float32 if c_type == "f32" else TD[self.dtype]
        return torch.from_numpy(np.ascontiguousarray(host64)).to(td).cuda()

    def operands(self):
        return ((self.S.m, self.D.m) if self.op == "dsd"
                else (self.D.m, self.S.m))

    def run(self, c_t, ex=True, stream=None):
        a, b = self.operands()
        fn = sp.MatmulAccumulateEx if ex else sp.MatmulAccumulate
        fn(a, self.ta, b, self.tb, sp.Matrix(self.m, self.n, c_t),
           stream=stream)

    def plain(self, c_t):
        a, b = self.operands()
        sp.MatmulEx(a, self.ta, b, self.tb, sp.Matrix(self.m, self.n, c_t))

    def check(self, c_type, what, ex=True, times=1, seed=0):
        host, c_t = self.c_in(c_type, seed)
        for _ in range(times):
            self.run(c_t, ex=ex)
        _equal(c_t, self.tensor(self.P * times + host, c_type), what)


@functools.lru_cache(maxsize=None)
def square(op, ta, tb, dtype):
    """Test 1's product: 1024 on the sparse side, 1032 on the dense one (a
    partial last tile), density 0.5."""
    k = 1024 if dtype == "f16" else 256
    m, n = (1024, 1032) if op == "dsd" else (1032, 1024)
    return Problem(op, m, k, n, ta, tb, dtype, 0.5, seed=17 + 2 * ta + tb)


# ------------------------------------------------------ 1. every product --

@pytest.mark.parametrize("c_type", C_TYPES)
@pytest.mark.parametrize("ta,tb", TRANSPOSES)
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("op,ex", [("dsd", False), ("dsd", True),
                                   ("dds", True)])
def test_every_product(op, ex, dtype, ta, tb, c_type):
    square(op, ta, tb, dtype).check(
        c_type, f"{op} acc {ta}{tb} {dtype} C {c_type} ex={ex}", ex=ex)


# ------------------------------------------------ 2. untouched empty rows --

def _mask_topology(mask):
    return mu.mask_to_bcsr(mask)


@functools.lru_cache(maxsize=None)
def holes(op, ta):
    """8 block-rows of op(A) (DSD) / block-columns of op(B) (DDS) with 1 and
    5 empty; K = 512, the dense extent 264."""
    rng = np.random.default_rng(5)
    mask = rng.random((8, 4)) < 0.6
    mask[:, 0] |= ~mask.any(axis=1)
    mask[[1, 5], :] = False
    if op == "dsd":
        stored = mask.T if ta else mask       # op(A) rows = stored cols if ta
        return Problem("dsd", 1024, 512, 264, ta, False, "f16",
                       topology=_mask_topology(stored), seed=6)
    return Problem("dds", 264, 512, 1024, False, False, "f16",
                   topology=_mask_topology(mask.T), seed=7)  # B is [K][N]


def _hole_slices(p):
    idx = np.r_[1 * B:2 * B, 5 * B:6 * B]
    return (idx, slice(None)) if p.op == "dsd" else (slice(None), idx)


@pytest.mark.parametrize("fill", ["values", "nan"])
@pytest.mark.parametrize("c_type", C_TYPES)
@pytest.mark.parametrize("op,ta", [("dsd", False), ("dsd", True),
                                   ("dds", False)])
def test_empty_rows_untouched(op, ta, c_type, fill):
    """Where the sparse operand has no blocks C is not touched: distinct
    non-integer values (or NaNs) preset there come back bit for bit; the
    rest of C is exact."""
    p = holes(op, ta)
    rng = np.random.default_rng(8)
    host = rng.integers(1, 9, size=(p.m, p.n)).astype(np.float64)
    host *= rng.choice([-1.0, 1.0], size=host.shape)
    c_t = p.tensor(host, c_type)
    hs = _hole_slices(p)
    rows, cols = (torch.as_tensor(s).cuda() if isinstance(s, np.ndarray) else s
                  for s in hs)
    shape = c_t[rows, cols].shape
    if fill == "nan":
        c_t[rows, cols] = float("nan")
    else:
        c_t[rows, cols] = (torch.randn(shape, device="cuda") * 3 + 0.37).to(
            c_t.dtype)
    before = c_t.clone()
    p.run(c_t)
    torch.cuda.synchronize()
    ints = {torch.float16: torch.int16, torch.bfloat16: torch.int16,
            torch.float32: torch.int32}[c_t.dtype]
    assert torch.equal(c_t[rows, cols].contiguous().view(ints),
                       before[rows, cols].contiguous().view(ints)), \
        f"{op} ta={ta} C {c_type}: empty rows changed"
    if fill == "nan":
        assert bool(torch.isnan(c_t[rows, cols]).all())
    want = p.tensor(p.P + host, c_type)
    want[rows, cols] = before[rows, cols]
    keep = torch.ones_like(c_t, dtype=torch.bool)
    keep[rows, cols] = False
    _equal(torch.where(keep, c_t, torch.zeros_like(c_t)),
           torch.where(keep, want, torch.zeros_like(want)),
           f"{op} ta={ta} C {c_type}: rows with blocks")


# ------------------------------------------------------ 3. pairs, small --

@functools.lru_cache(maxsize=None)
def few_rows(op, ta):
    """M = 512, K = 2048, N = 1024 with 13, 3, 9 and 5 of the 16 blocks in
    the 4 block-rows (DDS: block-columns of B): a plain call takes split
    mode here."""
    rng = np.random.default_rng(9)
    mask = np.zeros((4, 16), dtype=bool)
    for r, cnt in enumerate((13, 3, 9, 5)):
        mask[r, rng.choice(16, size=cnt, replace=False)] = True
    if op == "dsd":
        stored = mask.T if ta else mask
        return Problem("dsd", 512, 2048, 1024, ta, False, "f16",
                       topology=_mask_topology(stored), seed=10)
    return Problem("dds", 1024, 2048, 512, False, False, "f16",
                   topology=_mask_topology(mask.T), seed=11)


@pytest.mark.parametrize("op,ta", [("dsd", False), ("dsd", True),
                                   ("dds", False)])
def test_pairs_small_never_split(op, ta):
    p = few_rows(op, ta)
    a, b = p.operands()
    c = sp.Matrix(p.m, p.n, torch.empty(p.m, p.n, dtype=torch.float16,
                                        device="cuda"))
    plan = (sp.dsd_plan if op == "dsd" else sp.dds_plan)(a, ta, b, False, c)
    assert plan == 3, f"the plain call no longer takes split mode ({plan})"
    sp.pair_errors()
    p.check("f32", f"{op} ta={ta} pairs, small")
    assert sp.pair_errors() == 0


# ------------------------------------------------- 4. pairs, one per CU --

@functools.lru_cache(maxsize=None)
def one_per_cu(op):
    return Problem(op, 4096, 1024, 4096, False, False, "f16", 0.5, seed=12)


@pytest.mark.parametrize("op", ["dsd", "dds"])
def test_pairs_one_tile_per_cu(op):
    sp.pair_errors()
    one_per_cu(op).check("operand", f"{op} 4096^2 pairs")
    assert sp.pair_errors() == 0


# ----------------------------------------------------------------- 5. tall --

@functools.lru_cache(maxsize=None)
def tall(op, ta, density):
    """300 block-rows on the sparse side (the tall configuration), K = 384,
    dense extent 264. At density 0.02 most block-rows are empty."""
    if op == "dsd":
        return Problem("dsd", 300 * B, 384, 264, ta, False, "f16", density,
                       seed=13 + ta)
    return Problem("dds", 264, 384, 300 * B, ta, False, "f16", density,
                   seed=15 + ta)


@pytest.mark.parametrize("density", [0.3, 0.02])
@pytest.mark.parametrize("c_type", C_TYPES)
@pytest.mark.parametrize("ta", [False, True])
@pytest.mark.parametrize("op", ["dsd", "dds"])
def test_tall(op, ta, c_type, density):
    """Exact everywhere: the empty rows of the 2% operand keep C_in (their
    product is zero, so the expected value there is C_in itself)."""
    tall(op, ta, density).check(c_type,
                                f"{op} tall ta={ta} C {c_type} d={density}")


@functools.lru_cache(maxsize=None)
def tall_persistent():
    return Problem("dsd", 65536, 256, 1000, False, False, "f16", 0.3, seed=19)


def test_tall_persistent():
    tall_persistent().check("f32", "tall persistent 65536 x 256 x 1000")


# ---------------------------------------------------------------- 6. twice --

def test_twice_pairs():
    sp.pair_errors()
    one_per_cu("dsd").check("f32", "two calls, pairs", times=2, seed=1)
    assert sp.pair_errors() == 0


def test_twice_tall_persistent():
    tall_persistent().check("operand", "two calls, tall persistent", times=2,
                            seed=2)


# ----------------------------------- 7. the plain product's arithmetic --

@pytest.fixture
def eight_wave_no_split():
    """The plain call on the accumulating call's configuration: the 8-wave
    kernel, no split mode."""
    prev = sp.tuning("dsd4w", 0), sp.tuning("split", 0)
    yield
    sp.tuning("dsd4w", prev[0])
    sp.tuning("split", prev[1])


def _random_problem(op, m, k, n, ta, tb, dtype, seed, topology=None):
    rng = np.random.default_rng(seed)
    a_shape = (k, m) if ta else (m, k)
    b_shape = (n, k) if tb else (k, n)
    s_shape = a_shape if op == "dsd" else b_shape
    nnz = (int(topology[0][-1]) * B * B if topology is not None
           else mu.nonzeros_for_density(*s_shape, 0.5))
    S = H.HostSparse(*s_shape, nnz, rng, dtype, topology=topology)
    sp.AllocateTransposeBuffers(S.matrix)
    sp.Transpose(S.matrix)
    D = H.HostDense(*(b_shape if op == "dsd" else a_shape), rng, dtype)
    return (S.matrix, D.matrix) if op == "dsd" else (D.matrix, S.matrix)


def _same_as_plain(op, m, k, n, ta, tb, dtype, seed, topology=None):
    a, b = _random_problem(op, m, k, n, ta, tb, dtype, seed, topology)
    plain = torch.full((m, n), float("nan"), dtype=TD[dtype], device="cuda")
    sp.MatmulEx(a, ta, b, tb, sp.Matrix(m, n, plain))
    acc_t = torch.zeros(m, n, dtype=TD[dtype], device="cuda")
    sp.MatmulAccumulateEx(a, ta, b, tb, sp.Matrix(m, n, acc_t))
    acc_f = torch.zeros(m, n, dtype=torch.float32, device="cuda")
    sp.MatmulAccumulateEx(a, ta, b, tb, sp.Matrix(m, n, acc_f))
    torch.cuda.synchronize()
    assert not bool(torch.isnan(plain).any())
    _equal(acc_t, plain, f"{op} {ta}{tb} {dtype}: into T vs plain")
    _equal(acc_f.to(TD[dtype]), plain, f"{op} {ta}{tb} {dtype}: fp32 vs plain")


@pytest.mark.parametrize("ta,tb", TRANSPOSES)
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("op", ["dsd", "dds"])
def test_same_arithmetic_as_plain(op, dtype, ta, tb, eight_wave_no_split):
    """Random non-integer operands, C_in = 0: the accumulating call rounds
    the very accumulators the plain product rounds."""
    m, n = (1024, 1032) if op == "dsd" else (1032, 1024)
    _same_as_plain(op, m, 1024, n, ta, tb, dtype, 40 + 2 * ta + tb)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("op,ta", [("dsd", False), ("dsd", True),
                                   ("dds", False)])
def test_same_arithmetic_as_plain_pairs(op, ta, dtype, eight_wave_no_split):
    p = few_rows(op, ta)  # (its topology)
    topo = (p.S.offsets, p.S.indices)
    _same_as_plain(op, p.m, p.k, p.n, ta, False, dtype, 50, topology=topo)


# --------------------------------------------------------- 8. one rounding --

@pytest.mark.parametrize("c_type", C_TYPES)
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_one_rounding(dtype, c_type):
    """Row 0 of the product is 0.5 + eps with eps half an ulp of 0.5: rounded
    to T first it is 0.5, and C_in + 0.5 then ties back to C_in; added in
    fp32 and rounded once, C_in + 0.5 + eps rounds up to C_in + 1."""
    eps = 2.0 ** -12 if dtype == "f16" else 2.0 ** -9
    c0 = 1024.0 if dtype == "f16" else 128.0
    vals = torch.zeros(1, B, B, dtype=TD[dtype], device="cuda")
    vals[0, 0, 0] = 0.5
    vals[0, 0, 1] = eps
    a = sp.BlockMatrix(B, B, 128, B * B, vals,
                       torch.tensor([0, 1], dtype=torch.int32, device="cuda"),
                       torch.tensor([0], dtype=torch.int16, device="cuda"))
    b_t = torch.ones(B, B, dtype=TD[dtype], device="cuda")
    td = torch.float32 if c_type == "f32" else TD[dtype]
    c_t = torch.full((B, B), c0, dtype=td, device="cuda")
    sp.MatmulAccumulateEx(a, False, sp.Matrix(B, B, b_t), False,
                          sp.Matrix(B, B, c_t))
    want = torch.full((B, B), c0, dtype=td, device="cuda")
    want[0, :] = c0 + 0.5 + eps if c_type == "f32" else c0 + 1
    _equal(c_t, want, f"one rounding {dtype} C {c_type}")


# -------------------------------------------------------- 9. graph capture --

def test_graph_capture():
    """One accumulating DSD (pairs) captured and replayed three times:
    C_in + 3 P exactly (the pattern of test_graph_capture_with_pairs)."""
    p = one_per_cu("dsd")
    host, c_t = p.c_in("f32", seed=3)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    warm = torch.zeros_like(c_t)
    with torch.cuda.stream(s):
        p.run(warm)  # creates s's workspace
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    sp.pair_errors()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        p.run(c_t)
    c_t.copy_(p.tensor(host, "f32"))  # (capture does not run the launch)
    for _ in range(3):
        g.replay()
    _equal(c_t, p.tensor(3 * p.P + host, "f32"), "graph replays")
    assert sp.pair_errors() == 0


# ------------------------------- 10. no in-call events, no transposed B --

def test_dsd_nt_no_incall_events_no_bt():
    """DSD NT over a dense A: the plain call would transpose B into a
    workspace here; the accumulating call runs the NT kernel directly."""
    prev = sp.tuning("sdd_bt_min_mib", 1)
    try:
        p = Problem("dsd", 16384, 256, 2048, False, True, "f16", 1.0, seed=21)
        a, b = p.operands()
        probe = sp.Matrix(p.m, p.n, torch.empty(p.m, p.n, dtype=torch.float16,
                                                device="cuda"))
        assert sp.dsd_workspace_bytes(a, False, b, True, probe) > 0
        host, c_t = p.c_in("operand")
        torch.cuda.synchronize()
        events, launches = sp.incall_events(), sp.bt_launches()
        p.run(c_t)
        p.run(c_t, ex=False)
        assert sp.incall_events() == events
        assert sp.bt_launches() == launches
        _equal(c_t, p.tensor(2 * p.P + host, "operand"), "dsd nt acc")
    finally:
        sp.tuning("sdd_bt_min_mib", prev)
