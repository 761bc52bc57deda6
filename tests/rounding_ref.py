"""Inputs, models and expected values of the rounding-visible known-answer
tests (tests/test_rounding_host.py, tests/test_gpu_rounding.py,
tests/test_gpu_nonfinite.py). Host only: numpy, and torch for tensors on a
device the caller names. Nothing here calls the library.

The KATs of tests/test_gpu_kat.py use operands in {-1, 0, 1}; their results
are representable, so the kernels' last step, the fp32 -> fp16 / bf16
conversion, is an identity there. The operands built here keep what makes
those tests exact, and make the conversion do something:

  * one operand holds integers in [0, a_max], the other s_j * u with u an
    integer in [0, b_max] and one sign s_j per output column (per output row
    where the first operand carries it). Every product of one output element
    has the same sign, so every partial sum, in any order, is an integer no
    larger in magnitude than the total; with max|sum| < 2^24 the fp32
    accumulation is exact whatever the kernel's order. `Host` asserts that
    bound (and max|sum| < 65504 for fp16) on the product it built: a
    condition on the inputs, not a tolerance.
  * the totals are far above 2^11 (fp16) / 2^8 (bf16), so most of them are
    not representable and exactly one correct answer remains: the nearest
    representable value, ties to even (`round_once`).

The wrong models (`truncate`, `round_half_up`, `partial_in_T`,
`accumulate_twice`) exist only so that test_rounding_host.py can show that
each would be seen on these inputs. (a_max, b_max) is picked per case so
that the totals lie where a unit of the output type is 2, 4 or 8: there one
output in 2, 4 or 8 is a tie, which is what separates ties-to-even from
ties-away.

NaN / Inf planting (`plant`, `expected_with_specials`): the finite product
comes from `@` with the planted elements zeroed; the rows and columns a
planted element can reach are then recomputed by elementwise multiply and
sum in float64, never through BLAS (whose handling of 0 * NaN in blocked
kernels is its own business). Only STORED blocks of a sparse operand
contribute: the operand handed to these functions is the densified stored
matrix with a boolean `stored` mask, and a product term exists only where
both factors are stored. A NaN in row k of the dense operand therefore
reaches block-row r of the output only if r stores block-column k / 128; a
dense matmul of the zero-filled operands (the oracle's) would spread it
over the whole column strip and is the wrong reference here.
"""

from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from sputnik_amd import matrix_utils as mu

B = mu.BLOCK
# (explicit mantissa bits, minimum normal exponent, maximum exponent)
FORMATS = {"f16": (10, -14, 15), "bf16": (7, -126, 127)}
F16_MAX = 65504.0
CUS = 256  # compute units of the device the grouped / tail cases are sized for


# ---- the conversion, on bits -------------------------------------------------

def _convert(x64, dtype: str, mode: str) -> np.ndarray:
    """float64 -> T as float32 values (every T value is an fp32 value).
    mode: "even" nearest, ties to even; "half_up" nearest, ties away from
    zero (what adding half a unit to the bits and truncating gives);
    "truncate" toward zero (overflow then stays at T's largest finite)."""
    x = np.ascontiguousarray(x64, dtype=np.float64)
    p, emin, emax = FORMATS[dtype]
    u = x.view(np.uint64)
    neg = (u >> np.uint64(63)) != 0
    expo = ((u >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64)
    special = expo == 0x7FF
    tiny = expo == 0               # zero, or below every quantum of T
    e = expo - 1023
    sig = (u & np.uint64((1 << 52) - 1)) | np.uint64(1 << 52)  # |x| = sig 2^(e-52)
    # low bits of sig below T's quantum at this magnitude (more when the
    # result is subnormal in T); from 54 on the result is zero
    drop = np.clip((52 - p) + np.maximum(0, emin - e), 0, 54)
    sh = drop.astype(np.uint64)
    keep = sig >> sh
    rem = sig & ((np.uint64(1) << sh) - np.uint64(1))
    half = np.uint64(1) << (sh - np.uint64(1))
    if mode == "even":
        up = (rem > half) | ((rem == half) & ((keep & np.uint64(1)) == 1))
    elif mode == "half_up":
        up = rem >= half
    elif mode == "truncate":
        up = np.zeros(x.shape, bool)
    else:
        raise ValueError(mode)
    keep = keep + up.astype(np.uint64)
    with np.errstate(over="ignore"):   # (the inf / NaN inputs, replaced below)
        mag = np.ldexp(keep.astype(np.float64),
                       (e - 52 + drop).astype(np.int32))
    over = mag >= 2.0 ** (emax + 1)
    biggest = (2.0 - 2.0 ** -p) * 2.0 ** emax
    mag = np.where(over, biggest if mode == "truncate" else np.inf, mag)
    mag = np.where(tiny, 0.0, mag)
    out = np.where(neg, -mag, mag)
    out = np.where(special, x, out)
    with np.errstate(invalid="ignore"):
        return out.astype(np.float32)


def round_once(x64, dtype: str) -> np.ndarray:
    """The correctly rounded T value (nearest, ties to even) of exact
    float64 inputs, as float32: overflow gives +-inf, fp16 subnormals are
    rounded at their fixed quantum 2^-24, NaN and inf pass through."""
    return _convert(x64, dtype, "even")


def truncate(x64, dtype: str) -> np.ndarray:
    return _convert(x64, dtype, "truncate")


def round_half_up(x64, dtype: str) -> np.ndarray:
    return _convert(x64, dtype, "half_up")


def partial_in_T(parts, dtype: str) -> np.ndarray:
    """A hand-off that rounds to T: each listed partial sum is rounded to T,
    the rounded partials are added (exactly, as fp32 would here) and the
    total is rounded once more."""
    total = np.zeros(np.shape(parts[0]), np.float64)
    for part in parts:
        total += round_once(part, dtype).astype(np.float64)
    return round_once(total, dtype)


def accumulate_twice(P, C, dtype: str) -> np.ndarray:
    """round_T(round_T(P) + C) in place of round_T(P + C)."""
    return round_once(round_once(P, dtype).astype(np.float64) + C, dtype)


def bits(x32, dtype: str) -> np.ndarray:
    """uint16 bit patterns of float32 values that are T values."""
    x32 = np.ascontiguousarray(x32, dtype=np.float32)
    if dtype == "f16":
        return x32.astype(np.float16).view(np.uint16)
    return (x32.view(np.uint32) >> 16).astype(np.uint16)


# ---- values ------------------------------------------------------------------

def scaled(values, exp: int) -> np.ndarray:
    """values * 2^exp, float32: integer operands moved by a power of two, so
    products and sums are integers * 2^-s and the exactness argument of the
    module docstring holds unchanged."""
    return np.ldexp(np.asarray(values, np.float32), exp).astype(np.float32)


def sign_pattern(seed: int) -> np.ndarray:
    """128 signs, both present; output index j takes sign j % 128 (so a
    sparse operand's blocks need not know where they sit)."""
    s = np.where(np.random.default_rng(seed).random(B) < 0.5, -1.0, 1.0)
    s[0], s[1] = 1.0, -1.0
    return s.astype(np.float32)


def plain_values(a_max: int, neg_zero: bool = False):
    """values=(rng, shape) for the unsigned operand: integers in [0, a_max];
    with `neg_zero` every other zero is -0."""
    def gen(rng, shape):
        v = rng.integers(0, a_max + 1, size=shape).astype(np.float32)
        if neg_zero:
            z = np.flatnonzero(v == 0)[::2]
            v.reshape(-1)[z] = -0.0
        return v
    return gen


def signed_values(b_max: int, axis: int, seed: int):
    """values=(rng, shape) for the signed operand: s_j * u, u an integer in
    [0, b_max], j the index along `axis` (the output's)."""
    signs = sign_pattern(seed)

    def gen(rng, shape):
        u = rng.integers(0, b_max + 1, size=shape).astype(np.float32)
        s = signs[np.arange(shape[axis]) % B]
        view = [1] * len(shape)
        view[axis] = shape[axis]
        return u * s.reshape(view)   # (0 * -1 = -0: the operand holds -0)
    return gen


def pick_maxima(k_eff: float, dtype: str):
    """(a_max, b_max) from {1, 3, 7, 15} whose mean total, k_eff * a_max / 2
    * b_max / 2, is nearest (in ratio) the middle of the range where a unit
    of T is 2, 4 or 8: [2^11, 2^14) for fp16, [2^8, 2^11) for bf16."""
    target = 2.0 ** (12.5 if dtype == "f16" else 9.5)
    best = None
    for a in (1, 3, 7, 15):
        for b in (1, 3, 7, 15):
            if a > b:
                continue
            miss = abs(np.log(k_eff * a * b / 4.0 / target))
            if best is None or miss < best[0]:
                best = (miss, a, b)
    return best[1], best[2]


# ---- guard bands -------------------------------------------------------------

def moated(shape, dtype, fill, device="cuda", row=None):
    """A contiguous buffer of `shape` in the middle of a larger allocation.
    Returns (view, whole, pad): `whole` is the flat allocation, filled with
    `fill`, and `view` = whole[pad : pad + numel] reshaped. The moat on each
    side is at least 128 rows of the buffer's row length (`row`, default the
    last dimension) and a multiple of 4096 elements, so the view's alignment
    is that of a fresh allocation."""
    import torch

    numel = int(np.prod(shape))
    row = int(row if row is not None else shape[-1])
    pad = -(-max(128 * row, 1) // 4096) * 4096
    whole = torch.full((pad + numel + pad,), fill, dtype=dtype, device=device)
    return whole[pad:pad + numel].view(*shape), whole, pad


def moat_intact(whole, pad, pattern) -> bool:
    """Both moats of a `moated` output still hold `pattern`, bit for bit."""
    import torch

    ints = {2: torch.int16, 4: torch.int32}[whole.element_size()]
    raw = whole.view(ints)
    n = raw.numel()
    return bool((raw[:pad] == pattern).all()) and bool(
        (raw[n - pad:] == pattern).all())


# ---- the cases ---------------------------------------------------------------

SPARSE_X = ("dsd", "ssd", "dss")
SPARSE_Y = ("dds", "sds", "dss")
SPARSE_C = ("sdd", "ssd", "sds")
X_SIGNED = ("dds", "sds")


@dataclass(frozen=True)
class Case:
    """C[m x n] = op(X)[m x k] op(Y)[k x n]. `density` / `nb` size the sparse
    operands and a sparse output; `handoff`: None, "half" (pair and split
    hand-offs: the halves of each row's stored blocks) or an int S (K-split:
    S chunks of k-blocks); `holes`: an empty block-row and a block-row of
    all-zero blocks in the first sparse operand, zero rows in X for SDD;
    `tail`: the topology must leave a short last round of 4-block groups;
    `gap`: block index 2 of the K extent of every sparse operand stores
    nothing (an SDD's output: its block-row 2 and block-column 2)."""

    name: str
    op: str
    m: int
    k: int
    n: int
    ta: bool
    tb: bool
    dtype: str
    density: float = 0.5
    nb: int = None
    handoff: object = None
    holes: bool = False
    tail: bool = False
    gap: bool = False
    seed: int = 0
    acc: str = None        # None, "operand" or "f32": C_in's type

    @property
    def id(self):
        t = "NT"[self.ta] + "NT"[self.tb]
        return f"{self.name}-{self.op}-{t}-{self.dtype}"


class Sparse:
    """Stored BCSR operand on the host: topology, block values, dense copy."""

    def __init__(self, rows, cols, offsets, indices, values):
        self.rows, self.cols = rows, cols
        self.offsets, self.indices, self.values = offsets, indices, values
        self.nb = int(offsets[-1])

    @property
    def topology(self):
        return self.offsets, self.indices

    def dense(self, values=None):
        return mu.to_dense(self.rows, self.cols, self.offsets, self.indices,
                           self.values if values is None else values)

    def stored(self):
        """Boolean [rows, cols]: the element lies in a stored block."""
        m = mu.block_mask(self.offsets, self.indices, self.cols // B) != 0
        return np.repeat(np.repeat(m, B, axis=0), B, axis=1)

    def blocks_of(self, full):
        rows = np.repeat(np.arange(len(self.offsets) - 1), np.diff(self.offsets))
        if not len(rows):
            return np.zeros((0, B, B), full.dtype)
        return np.stack([full[r * B:(r + 1) * B, c * B:(c + 1) * B]
                         for r, c in zip(rows, self.indices)])


def _topology(rows_b, cols_b, nb, rng, drop_rows=(), drop_cols=(),
              tail=False):
    for _ in range(64):
        off, idx = mu.random_topology(rows_b, cols_b, nb, rng, unordered=True)
        rows = np.repeat(np.arange(rows_b), np.diff(off))
        keep = ~np.isin(rows, [r for r in drop_rows if r < rows_b - 1]) \
            & ~np.isin(idx, [c for c in drop_cols if c < cols_b - 1])
        if not keep.all():            # those block-rows / columns lose theirs
            counts = np.bincount(rows[keep], minlength=rows_b)
            off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
            idx = idx[keep]
        if tail:
            groups = int(((np.diff(off) + 3) // 4).sum())
            if not 0 < groups % CUS <= CUS // 4:
                continue
        return off.astype(np.int32), idx
    raise AssertionError("no topology with a short last round found")


def _first_half(sp: Sparse, transposed: bool):
    """Block values of `sp` with the second half of the stored blocks of
    every row of op(sp) zeroed: storage order for the stored rows, ascending
    for the rows of the transpose."""
    vals = sp.values.copy()
    if not transposed:
        for r in range(len(sp.offsets) - 1):
            a, b = int(sp.offsets[r]), int(sp.offsets[r + 1])
            vals[a + (b - a + 1) // 2:b] = 0
        return vals
    rows = np.repeat(np.arange(len(sp.offsets) - 1), np.diff(sp.offsets))
    for c in range(sp.cols // B):
        e = np.flatnonzero(sp.indices == c)
        e = e[np.argsort(rows[e], kind="stable")]
        vals[e[(len(e) + 1) // 2:]] = 0
    return vals


def _op(x, t):
    return x.T if t else x


class Host:
    """One case built on the host: operands, the exact float64 product P
    (of the stored blocks only), the hand-off partials, the expected output
    in the output's layout, and the input conditions asserted."""

    def __init__(self, case: Case):
        c = self.case = case
        rng = np.random.default_rng(c.seed + 7919)
        xs = (c.k, c.m) if c.ta else (c.m, c.k)
        ys = (c.n, c.k) if c.tb else (c.k, c.n)
        k_eff = c.k * (c.density if c.op in SPARSE_X and c.nb is None else 1) \
            * (c.density if c.op in SPARSE_Y and c.nb is None else 1)
        k_eff = max(k_eff, B)       # (a row that stores anything stores a block)
        ksplit = isinstance(c.handoff, int)
        if ksplit:                  # thinned past the first chunk, below
            k_eff *= 1.0 / c.handoff + (1 - 1.0 / c.handoff) / 8
        self.a_max, self.b_max = pick_maxima(k_eff, c.dtype)
        x_signed = c.op in X_SIGNED
        plain = plain_values(self.a_max, neg_zero=True)
        if x_signed:
            gx = signed_values(self.b_max, -1 if c.ta else -2, c.seed)
            gy = plain
        else:
            gx = plain
            gy = signed_values(self.b_max, -2 if c.tb else -1, c.seed)
        self.X = self._operand(c.op in SPARSE_X, xs, gx, rng, c.holes,
                               0 if c.ta else 1)
        self.Y = self._operand(c.op in SPARSE_Y, ys, gy, rng,
                               c.holes and c.op not in SPARSE_X,
                               1 if c.tb else 0)
        if c.holes and c.op == "sdd":           # zero output rows 128-255
            rows = (slice(None), slice(B, 2 * B)) if c.ta else slice(B, 2 * B)
            self.X[rows] = np.where(np.arange(B)[:, None] % 2 if not c.ta
                                    else np.arange(B)[None, :] % 2, -0.0, 0.0)
        if ksplit:
            # A K-split hands over S partials of about total / S each. Were
            # they equal, a partial that is not representable (so that
            # rounding it shows) would put the total S units higher, where
            # ties are too rare for round_half_up to show. So the first
            # chunk carries about half of every sum: past it X keeps one k
            # in 8. Every chunk still contributes to every output.
            kk = np.arange(c.k)
            thin = (kk >= (-(-c.k // B) // c.handoff) * B) & (kk % 8 != 0)
            self.X[(thin, slice(None)) if c.ta else (slice(None), thin)] = 0
        self.C = None
        if c.op in SPARSE_C:
            nb = c.nb if c.nb is not None else \
                mu.nonzeros_for_density(c.m, c.n, c.density) // (B * B)
            gap = (2,) if c.gap else ()
            off, idx = _topology(c.m // B, c.n // B, nb, rng, gap, gap, c.tail)
            self.C = Sparse(c.m, c.n, off, idx, None)
        x64 = _op(self.dense(self.X), c.ta).astype(np.float64)
        y64 = _op(self.dense(self.Y), c.tb).astype(np.float64)
        self.P = x64 @ y64
        self.parts = self._parts(x64, y64)
        self.c_in = None
        total = self.P
        if c.acc:
            mag = float(np.abs(self.P).mean())
            cin = rng.integers(-int(mag), int(mag) + 1, size=self.P.shape)
            self.c_in = round_once(cin.astype(np.float64), c.dtype)
            total = self.P + self.c_in.astype(np.float64)
        self.total = total
        peak = float(np.abs(total).max())
        peak = max(peak, float(np.abs(self.P).max()))
        assert peak < 2.0 ** 24, (c.id, peak)
        if c.dtype == "f16":
            assert peak < F16_MAX, (c.id, peak)
        self.peak = peak

    def _operand(self, sparse, shape, gen, rng, holes, k_axis):
        if not sparse:
            return gen(rng, shape)
        c = self.case
        nb = mu.nonzeros_for_density(shape[0], shape[1], c.density) // (B * B)
        drop = [(1,) if holes else (), ()]
        if c.gap:
            drop[k_axis] = drop[k_axis] + (2,)
        off, idx = _topology(shape[0] // B, shape[1] // B, nb, rng, *drop)
        vals = gen(rng, (len(idx), B, B))
        if holes and len(off) > 4:              # block-row 3: all-zero blocks
            blk = vals[off[3]:off[4]]
            blk[...] = np.where(np.arange(B)[:, None] % 2, -0.0, 0.0)
        return Sparse(shape[0], shape[1], off, idx, vals)

    @staticmethod
    def dense(operand, values=None):
        if isinstance(operand, Sparse):
            return operand.dense(values)
        return operand

    def _parts(self, x64, y64):
        c = self.case
        h = c.handoff
        if isinstance(h, int) and not isinstance(h, bool):
            kb = -(-c.k // B)
            cuts = [min(c.k, (i * kb // h) * B) for i in range(h)] + [c.k]
            return [x64[:, a:b] @ y64[a:b] for a, b in zip(cuts, cuts[1:])]
        if isinstance(self.X, Sparse):
            first = _op(self.X.dense(_first_half(self.X, c.ta)), c.ta)
            p1 = first.astype(np.float64) @ y64
        elif isinstance(self.Y, Sparse):
            first = _op(self.Y.dense(_first_half(self.Y, not c.tb)), c.tb)
            p1 = x64 @ first.astype(np.float64)
        else:
            cut = (-(-c.k // B) + 1) // 2 * B
            p1 = x64[:, :cut] @ y64[:cut]
        return [p1, self.P - p1]

    def layout(self, full):
        """`full` [m, n] in the output's layout: the stored blocks for a
        sparse output."""
        return self.C.blocks_of(full) if self.C is not None else full

    def expected(self):
        """round_once of the exact result, float32, in the output's layout
        (an fp32 C holds the exact result itself)."""
        if self.case.acc == "f32":
            return self.total.astype(np.float32)
        return self.layout(round_once(self.total, self.case.dtype))


@functools.lru_cache(maxsize=2)
def host(case: Case) -> Host:
    return Host(case)


TRANSPOSES = [(False, False), (False, True), (True, False), (True, True)]
DTYPES = ("f16", "bf16")


def _all_t(name, op, m, k, n, dtypes=DTYPES, **kw):
    return [Case(name, op, m, k, n, ta, tb, dt, seed=2 * ta + tb, **kw)
            for dt in dtypes for ta, tb in TRANSPOSES]


# One case per dispatch path, at the smallest shape at which
# tests/test_gpu_kat.py reaches it (the KAT named on each line).
ROUNDING_CASES = (
    _all_t("kat", "dsd", 1024, 1024, 1032, holes=True)       # test_kat_dsd
    + _all_t("kat", "dds", 1032, 1024, 1024, holes=True)     # test_kat_dds
    + [Case("tall", "dsd", 300 * 128, 384, 264, False, False, "f16",
            density=0.3, seed=1),                            # ..._dsd_ex_tall
       Case("tall", "dsd", 300 * 128, 256, 264, True, False, "bf16",
            density=0.3, seed=2),
       Case("tallpipe", "dsd", 280 * 128, 4096, 1024, False, False, "f16",
            density=1.0, seed=3),                            # TALL_PIPE_CASES[3]
       Case("split", "dsd", 512, 4096, 4096, False, False, "f16",
            handoff="half", seed=4),                         # ..._dsd_split
       Case("split", "dsd", 512, 4096, 4096, True, False, "bf16",
            handoff="half", seed=5),
       Case("split", "dds", 4096, 4096, 512, False, False, "f16",
            handoff="half", seed=6),                         # ..._dds_split
       Case("split", "dds", 4096, 4096, 512, False, True, "bf16",
            handoff="half", seed=7),
       Case("splitpartial", "dsd", 512, 1024, 1000, False, False, "f16",
            density=1.0, handoff="half", seed=8),
       Case("pairs", "dsd", 4096, 4096, 4096, False, False, "f16",
            handoff="half", seed=9),                         # ..._4096_pairs
       Case("pairs", "dds", 4096, 4096, 4096, False, False, "f16",
            handoff="half", seed=10)]
    + _all_t("k1032", "sdd", 1024, 1032, 1024, holes=True)   # test_kat_sdd
    + _all_t("k200", "sdd", 1024, 200, 1024)
    + [Case("grouped", "sdd", 6656, 200, 6656, False, False, "f16",
            nb=6 * CUS + 37, seed=11),                       # ..._sdd_grouped
       Case("grouped", "sdd", 6656, 256, 6656, True, True, "bf16",
            nb=6 * CUS + 37, seed=12),
       Case("tailsplit", "sdd", 8192, 256, 8192, False, False, "f16",
            tail=True, seed=13),                             # ..._tail_split
       Case("bt", "sdd", 8192, 512, 4096, False, True, "f16", density=0.6,
            seed=14),                                        # ..._bt_transpose
       Case("bt", "sdd", 8192, 256, 4096, True, True, "bf16", density=0.6,
            seed=15),
       Case("ksplit", "sdd", 1024, 2048, 4096, False, False, "f16", nb=60,
            handoff=8, seed=16),                             # KSPLIT_CASES[0]
       Case("ksplit4", "sdd", 4096, 1152, 4096, False, False, "f16", nb=150,
            handoff=4, seed=17),                             # KSPLIT_CASES[2]
       Case("ksplit", "sdd", 1024, 2048, 4096, False, False, "bf16", nb=60,
            handoff=8, seed=18)]                             # KSPLIT_CASES[1]
    + _all_t("kat", "ssd", 1024, 768, 1152, density=0.4)     # test_kat_ss
    + _all_t("kat", "sds", 1024, 768, 1152, density=0.4)
    + _all_t("kat", "dss", 896, 1024, 1024, holes=True)      # test_kat_dss
)

# Accumulating DSD / DDS: C += op(A) op(B), test_gpu_accumulate.py's shapes.
ACCUMULATE_CASES = [
    Case("acc", "dsd", 1024, 1024, 1032, False, False, "f16", acc="operand",
         seed=20),
    Case("acc", "dsd", 1024, 1024, 1032, True, True, "bf16", acc="operand",
         seed=21),
    Case("acc", "dds", 1032, 1024, 1024, False, True, "f16", acc="operand",
         seed=22),
    Case("acc", "dds", 1032, 1024, 1024, True, False, "bf16", acc="operand",
         seed=23),
    Case("acc", "dsd", 1024, 1024, 1032, False, False, "f16", acc="f32",
         seed=20),
]


# Overflow, NaN / Inf and subnormals (tests/test_gpu_nonfinite.py): small
# shapes, the reference recomputes strips without BLAS.
NONFINITE_CASES = [
    Case("nf", "dsd", 1024, 1024, 520, False, False, "f16", gap=True, seed=30),
    Case("nf", "dsd", 1024, 1024, 520, True, False, "bf16", gap=True, seed=31),
    Case("nf", "dds", 520, 1024, 1024, False, False, "bf16", gap=True, seed=32),
    Case("nf", "dds", 520, 1024, 1024, False, True, "f16", gap=True, seed=33),
    Case("nf", "sdd", 1024, 200, 1024, False, False, "f16", gap=True, seed=34),
    Case("nf", "sdd", 1024, 200, 1024, False, True, "bf16", gap=True, seed=35),
    Case("nf", "dsd", 1024, 1024, 520, False, False, "bf16", gap=True, seed=41),
    Case("nf", "dds", 520, 1024, 1024, False, False, "f16", gap=True, seed=42),
    Case("nf", "sdd", 1024, 200, 1024, False, False, "bf16", gap=True, seed=43),
    Case("nfsplit", "dsd", 512, 4096, 4096, False, False, "f16", gap=True,
         handoff="half", seed=36),
    Case("nfpairs", "dsd", 4096, 4096, 4096, False, False, "f16", gap=True,
         handoff="half", seed=37),
    Case("nfksplit", "sdd", 1024, 2048, 4096, False, False, "f16", nb=60,
         handoff=8, seed=38),
    Case("nfgrouped", "sdd", 6656, 200, 6656, False, False, "f16",
         nb=6 * CUS + 37, gap=True, seed=39),
    Case("nf", "dss", 896, 1024, 1024, False, False, "f16", gap=True, seed=40),
]


# ---- NaN / Inf ---------------------------------------------------------------

def plant(values, where, what=(np.nan, np.inf, -np.inf)):
    """Writes `what` cyclically at the flat positions `where` of `values`
    (in place). Returns the recorded [(flat position, value)]."""
    flat = values.reshape(-1)
    rec = []
    for i, pos in enumerate(where):
        v = np.float32(what[i % len(what)])
        flat[int(pos)] = v
        rec.append((int(pos), float(v)))
    return rec


def expected_with_specials(x, x_stored, y, y_stored, finite=None):
    """float64 x[m, k] @ y[k, n] with IEEE propagation of the non-finite
    elements, over the terms whose two factors are both stored (`*_stored`:
    boolean masks, None for a dense operand). Module docstring: the finite
    part by `@` on the operands with the non-finite elements zeroed
    (`finite`: that product if the caller has it; only its rows and columns
    away from the planted elements are used), then the rows of the output
    that a non-finite x can reach and the columns a non-finite y can reach
    recomputed by multiply-and-sum."""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    xs = np.ones(x.shape, bool) if x_stored is None else x_stored
    ys = np.ones(y.shape, bool) if y_stored is None else y_stored
    bad_x, bad_y = ~np.isfinite(x), ~np.isfinite(y)
    assert not (bad_x & ~xs).any() and not (bad_y & ~ys).any()
    if finite is not None:
        out = np.array(finite, np.float64)
    else:
        out = np.where(bad_x, 0.0, x) @ np.where(bad_y, 0.0, y)

    def strip(xr, xsr, yc, ysc):
        """sum_k xr[i, k] * yc[k, j] over the stored terms, k ascending."""
        acc = np.zeros((xr.shape[0], yc.shape[1]))
        with np.errstate(invalid="ignore"):
            for kk in range(xr.shape[1]):
                both = xsr[:, kk, None] & ysc[None, kk, :]
                if not both.any():
                    continue
                term = xr[:, kk, None] * yc[None, kk, :]
                acc += np.where(both, term, 0.0)
        return acc

    rows = np.flatnonzero(bad_x.any(axis=1))
    if len(rows):
        out[rows] = strip(x[rows], xs[rows], y, ys)
    cols = np.flatnonzero(bad_y.any(axis=0))
    if len(cols):
        out[:, cols] = strip(x, xs, y[:, cols], ys[:, cols])
    return out
