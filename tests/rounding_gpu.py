"""Device side of the rounding-visible KATs, shared by
tests/test_gpu_rounding.py and tests/test_gpu_nonfinite.py: a case of
tests/rounding_ref.py put on the device through the builders of
tests/test_gpu_kat.py, every value buffer inside guard bands, and run under
the three kernel selections.

Guard bands (rounding_ref.moated): sparse block data, dense operands,
outputs and the accumulate C are each a contiguous view in the middle of a
larger allocation. Operand bands are NaN, so a load from outside an operand
that reaches an accumulator shows in the exact comparison; output bands hold
SENTINEL and are compared bit for bit after every launch. Offset and index
lists keep their true sizes and are not poisoned: a poisoned index could
become a wild address.
"""

import contextlib

import numpy as np
import torch

import sputnik_amd as sp
from tests import rounding_ref as R
from tests import test_gpu_kat as K

TD = K.TD
SENTINEL = 0x7E5A          # int16 / low half of the int32 pattern
SENTINEL32 = 0x7E5A7E5A
MODES = (0, 5, 1)          # 8-wave, forced 4-wave, default dispatch

# Knobs that take a case's shape to the path it is named after (the
# fixtures of tests/test_gpu_kat.py: tall_pipe, bt_small, ksplit_any_k; the
# tail split's and the pair placement's knobs).
KNOBS = {
    "tallpipe": {"tall4w": 1},
    "bt": {"sdd_bt_min_mib": 1},
    "ksplit": {"sdd_ksplit": 8, "sdd_ksplit_min_k": 512},
    "ksplit4": {"sdd_ksplit": 8, "sdd_ksplit_min_k": 512},
    "nfksplit": {"sdd_ksplit": 8, "sdd_ksplit_min_k": 512},
    "tailsplit": {"sdd_tail_min_k": 256},
    "pairs": {"min_handoff": 1},
    "nfpairs": {"min_handoff": 1},
}


@contextlib.contextmanager
def knobs(settings):
    prev = [(name, sp.tuning(name, value)) for name, value in settings.items()]
    try:
        yield
    finally:
        for name, value in reversed(prev):
            sp.tuning(name, value)


@contextlib.contextmanager
def kernel_mode(mode):
    prev = sp.select_dsd_kernel(mode)
    try:
        yield
    finally:
        sp.select_dsd_kernel(prev)


def place_operand(host, dtype):
    """An operand's values in the middle of a NaN-filled allocation."""
    view, _, _ = R.moated(tuple(host.shape), TD[dtype], float("nan"))
    view.copy_(host.to(TD[dtype]))
    return view


class Output:
    """An output buffer of `shape` between sentinel bands; `.t` is the
    tensor of `td` the kernel writes."""

    def __init__(self, shape, td, row=None):
        wide = td == torch.float32
        self.pattern = SENTINEL32 if wide else SENTINEL
        raw, self.whole, self.pad = R.moated(
            shape, torch.int32 if wide else torch.int16, self.pattern, row=row)
        self.t = raw.view(td)

    def intact(self):
        return R.moat_intact(self.whole, self.pad, self.pattern)


class Problem:
    """Host case `h` on the device. `x` / `y` replace the host values of the
    operands (block values for a sparse one), for the planted variants."""

    def __init__(self, h, x=None, y=None):
        self.h, c = h, h.case
        self.case = c
        self.X = self._operand(h.X, x, (c.k, c.m) if c.ta else (c.m, c.k))
        self.Y = self._operand(h.Y, y, (c.n, c.k) if c.tb else (c.k, c.n))
        td = torch.float32 if c.acc == "f32" else TD[c.dtype]
        if h.C is not None:
            self.out = Output((h.C.nb, R.B, R.B), td)
            self.C = sp.BlockMatrix(
                c.m, c.n, 128, h.C.nb * R.B * R.B, self.out.t,
                torch.from_numpy(h.C.offsets.astype(np.int32)).cuda(),
                torch.from_numpy(h.C.indices.astype(np.int16)).cuda())
            sp.AllocateRowIndicesBuffer(self.C)
            sp.RowIndices(self.C, self.C.row_indices)
        else:
            self.out = Output((c.m, c.n), td)
            self.C = sp.Matrix(c.m, c.n, self.out.t)

    def _operand(self, host, values, shape):
        c = self.case
        if isinstance(host, R.Sparse):
            vals = host.values if values is None else values
            s = K.ISparse(shape[0], shape[1], None, None, c.dtype,
                          topology=host.topology,
                          values=lambda rng, shp: vals, place=place_operand)
            assert s.dev.shape == (host.nb, R.B, R.B)
            return s
        vals = host if values is None else values
        return K.IDense(shape[0], shape[1], None, c.dtype,
                        values=lambda rng, shp: vals, place=place_operand)

    def launch(self, ex=False):
        c = self.case
        (sp.MatmulEx if ex else sp.Matmul)(self.X.m, c.ta, self.Y.m, c.tb,
                                           self.C)

    def run(self, ex=False):
        """One launch into a NaN-filled output; the result, cloned."""
        self.out.t.fill_(float("nan"))
        self.launch(ex)
        torch.cuda.synchronize()
        return self.out.t.clone()

    def run_modes(self, at_default=None, ex=False):
        """{mode: output} under MODES; `at_default(problem)` runs under the
        default dispatch before its launch (plan assertions). Checks the
        output's bands after every launch."""
        got = {}
        with knobs(KNOBS.get(self.case.name, {})):
            for mode in MODES:
                with kernel_mode(mode):
                    if mode == 1 and at_default is not None:
                        at_default(self)
                    got[mode] = self.run(ex)
                    assert self.out.intact(), \
                        f"{self.case.id} mode {mode}: wrote outside the output"
        return got


def expect(x32, dtype):
    """float32 values that are T values -> device tensor of T (exact)."""
    return torch.from_numpy(np.ascontiguousarray(x32)).to(TD[dtype]).cuda()


def assert_exact(got, want, what):
    """torch.equal on the whole output, then the sign of every zero: where
    the expected value is 0 the sign bit is clear."""
    K._equal(got, want, what)
    zero = want == 0
    if bool(zero.any()):
        raw = got.view(torch.int16 if got.element_size() == 2 else torch.int32)
        assert bool((raw[zero] == 0).all()), f"{what}: a zero has its sign set"
