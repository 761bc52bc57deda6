"""GPU: the MoE token permutation kernels (sputnik/block/moe.h) through the
ctypes bindings of the C entry points, against tests/moe_ref.py (numpy; it
never calls the library).

Every case of moe_ref.CASES x HIDDEN x fp16 / bf16 (the scatter and the
weight gradient: DEEP_CASE too) runs in four layouts: the
buffers 256-byte aligned (the 16-byte path wherever hidden % 8 == 0) and
offset by 4 elements (8 bytes: the element path), each with the padded matrix
sized exactly (padded_bins[-1]) and by rows_bound (trailing zero rows).

  route     bins, padded_bins, tokens_per_expert and row_of equal the
            reference exactly
  gather    bit-identical, the +0 padding rows included, into an output
            prefilled with NaN; also with weights of type T (a product of two
            T values is exact in fp32, so it is rounded once)
  scatter   unweighted and with weights of T: bit-identical to the float32
            emulation (every product is exact in fp32, so an fma chain and
            multiply-then-add agree); with fp32 weights within
            2^-p |ref64| + top_k 2^-23 sum_k |w y|
  wgrad     within 2^-p |ref64| + hidden 2^-24 sum_h |dout y|, p that of the
            output type (24 for fp32 weights)

test_moe_host.py checks on the CPU that the emulation meets the two bounds
on these operands (moe_ref.case_inputs says how they avoid T's subnormals).
"""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import sputnik_amd as sp  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests import moe_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

OFFSETS = (0, 4)           # elements in front of every row buffer
CASE_IDS = ["%dx%d-E%d-%s" % c for c in R.CASES]
cases = pytest.mark.parametrize("case", R.CASES, ids=CASE_IDS)
hiddens = pytest.mark.parametrize("hidden", R.HIDDEN)
dtypes = pytest.mark.parametrize("dtype", R.DTYPES)
# moe_ref.scatter_cases(): cases x hiddens x dtypes under the ids of the three
# marks above, plus DEEP_CASE (the scatter's picks past the hoisted ones).
scatter_cases = pytest.mark.parametrize(
    "case,hidden,dtype",
    [(c, h, d) for c, h in R.scatter_cases() for d in R.DTYPES],
    ids=["%s-%d-%dx%d-E%d-%s" % (d, h, *c)
         for c, h in R.scatter_cases() for d in R.DTYPES])


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def _buffer(shape, td, offset, fill=float("nan")):
    """A contiguous device tensor of `shape` that starts `offset` elements
    into a fresh allocation (torch's are at least 256-byte aligned)."""
    numel = int(np.prod(shape))
    flat = torch.full((numel + offset,), fill, dtype=td, device="cuda")
    assert flat.data_ptr() % 256 == 0
    return flat[offset:].view(*shape)


def _put(values, td, offset):
    t = _buffer(values.shape, td, offset)
    t.copy_(torch.from_numpy(np.array(values)).to(td))
    return t


def _np32(t):
    return t.float().cpu().numpy()


def _same_bits(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = got.view(np.uint32) != ref.view(np.uint32)
    assert not bad.any(), (
        f"{what}: {int(bad.sum())}/{bad.size} elements differ, first at "
        f"{np.argwhere(bad)[0].tolist()}: {got[bad][0]!r} != {ref[bad][0]!r}")


def _row_counts(case, r):
    return (R.exact_rows(r), R.rows_bound(case[0] * case[1], case[2]))


class _DevRoute:
    def __init__(self, r):
        self.indices, self.bin_ids = _i32(r.indices), _i32(r.bin_ids)
        self.bins, self.padded_bins = _i32(r.bins), _i32(r.padded_bins)
        self.row_of = _i32(r.row_of)


@cases
def test_route(case):
    r = R.case_route(case)
    e, n = case[2], case[0] * case[1]
    bin_ids, indices = _i32(r.bin_ids), _i32(r.indices)
    bins, tpe, padded = (torch.full((e,), -7, dtype=torch.int32, device="cuda")
                         for _ in range(3))
    sp.MoeBins(bin_ids, e, bins, tpe, padded)
    assert np.array_equal(bins.cpu().numpy(), r.bins)
    assert np.array_equal(tpe.cpu().numpy(), r.tokens_per_expert)
    assert np.array_equal(padded.cpu().numpy(), r.padded_bins)
    for rows in _row_counts(case, r):
        row_of = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        sp.MoeRowMap(indices, bin_ids, bins, padded, rows, row_of)
        assert np.array_equal(row_of.cpu().numpy(), r.row_of)


@cases
@hiddens
@dtypes
def test_gather_bit_exact(case, hidden, dtype):
    c = R.case_inputs(case, hidden, dtype)
    r, td = c.route, H.torch_dtype(dtype)
    d = _DevRoute(r)
    for offset in OFFSETS:
        x, w = _put(c.x, td, offset), _put(c.w, td, 0)
        for rows in _row_counts(case, r):
            for weights, wref in ((None, None), (w, c.w)):
                out = _buffer((rows, hidden), td, offset)
                sp.PaddedGather(x, d.indices, d.bins, d.padded_bins, out,
                                r.top_k, weights=weights)
                _same_bits(_np32(out), R.gather(c.x, r, rows, wref, dtype),
                           f"gather offset {offset} rows {rows} "
                           f"weights {wref is not None}")


@scatter_cases
def test_scatter_bit_exact(case, hidden, dtype):
    c = R.case_inputs(case, hidden, dtype)
    r, td = c.route, H.torch_dtype(dtype)
    d = _DevRoute(r)
    refs = {False: R.scatter32(c.y, r, None, dtype),
            True: R.scatter32(c.y, r, c.w, dtype)}
    for offset in OFFSETS:
        w = _put(c.w, td, 0)
        for rows in _row_counts(case, r):
            y = _put(c.y[:rows], td, offset)
            for weighted in (False, True):
                out = _buffer((r.tokens, hidden), td, offset)
                sp.PaddedScatter(y, d.row_of, out, r.top_k,
                                 weights=w if weighted else None)
                _same_bits(_np32(out), refs[weighted],
                           f"scatter offset {offset} rows {rows} "
                           f"weights {weighted}")


@scatter_cases
def test_scatter_fp32_weights(case, hidden, dtype):
    c = R.case_inputs(case, hidden, dtype)
    r, td = c.route, H.torch_dtype(dtype)
    d = _DevRoute(r)
    ref, absum = R.scatter64(c.y_cols, r, c.w32)
    bound = R.scatter_bound(ref, absum, r.top_k, dtype)
    w = _put(c.w32, torch.float32, 0).view(r.tokens, r.top_k)
    for offset in OFFSETS:
        for rows in _row_counts(case, r):
            y = _put(c.y_cols[:rows], td, offset)
            out = _buffer((r.tokens, hidden), td, offset)
            sp.PaddedScatter(y, d.row_of, out, r.top_k, weights=w)
            err = np.abs(_np32(out).astype(np.float64) - ref)
            print(f"offset {offset} rows {rows}: max err / bound "
                  f"{np.nanmax(err / bound):.3f}")
            assert (err <= bound).all()


@scatter_cases
def test_wgrad(case, hidden, dtype):
    c = R.case_inputs(case, hidden, dtype)
    r, td = c.route, H.torch_dtype(dtype)
    d = _DevRoute(r)
    n = r.tokens * r.top_k
    ref, absum = R.wgrad64(c.dout_abs, c.y_rows, r)
    for offset in OFFSETS:
        dout = _put(c.dout_abs, td, offset)
        for rows in _row_counts(case, r):
            y = _put(c.y_rows[:rows], td, offset)
            for out_type, wd in (("f32", torch.float32), (dtype, td)):
                dw = _buffer((n,), wd, 0)
                sp.PaddedScatterWeightGrad(dout, y, d.row_of, dw, r.top_k)
                bound = R.wgrad_bound(ref, absum, hidden, out_type)
                err = np.abs(_np32(dw).astype(np.float64) - ref)
                print(f"offset {offset} rows {rows} {out_type}: max err / "
                      f"bound {np.nanmax(err / bound):.3f}")
                assert (err <= bound).all()


def test_metadata_out_of_range_reads_and_writes_nothing_outside():
    """Garbage routing tensors stand for rows of zeros: every output element
    is written (no NaN left), and nothing next to the outputs is touched."""
    case, hidden, dtype = R.CASES[4], 264, "bf16"
    c = R.case_inputs(case, hidden, dtype)
    r, td = c.route, H.torch_dtype(dtype)
    n, e = r.tokens * r.top_k, case[2]
    rows = R.exact_rows(r)
    big = 2 ** 31 - 1
    rng = np.random.default_rng(5)
    far = [-big, -1, max(n, rows), big]     # in range of no buffer

    def junk(k):
        return _i32(rng.choice(far, k))
    x, y = _put(c.x, td, 0), _put(c.y[:rows], td, 0)

    def guarded(shape, wd=td):
        flat = torch.full((int(np.prod(shape)) + 512,), float("nan"),
                          dtype=wd, device="cuda")
        return flat, flat[256:-256].view(*shape)

    flat, out = guarded((rows, hidden))
    for indices, bins, padded in ((junk(n), _i32(r.bins), _i32(r.padded_bins)),
                                  (_i32(r.indices), junk(e), junk(e)),
                                  (_i32(r.indices), _i32(r.bins), junk(e))):
        out.fill_(float("nan"))
        sp.PaddedGather(x, indices, bins, padded, out, r.top_k)
        assert not torch.isnan(out).any()
        assert torch.isnan(flat[:256]).all() and torch.isnan(flat[-256:]).all()

    flat, out = guarded((r.tokens, hidden))
    sp.PaddedScatter(y, junk(n), out, r.top_k)
    assert (out == 0).all()
    assert torch.isnan(flat[:256]).all() and torch.isnan(flat[-256:]).all()

    flat, dw = guarded((n,), torch.float32)
    sp.PaddedScatterWeightGrad(_put(c.dout, td, 0), y, junk(n), dw, r.top_k)
    assert (dw == 0).all()
    assert torch.isnan(flat[:256]).all() and torch.isnan(flat[-256:]).all()

    row_of = torch.full((n + 512,), -7, dtype=torch.int32, device="cuda")
    sp.MoeRowMap(junk(n), junk(n), junk(e), junk(e), rows, row_of[256:-256])
    got = row_of.cpu().numpy()
    assert (got[:256] == -7).all() and (got[-256:] == -7).all()
    assert ((got[256:-256] >= -7) & (got[256:-256] < rows)).all()
