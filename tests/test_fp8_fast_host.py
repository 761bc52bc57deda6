"""CPU: the host side of the fp8 products' fast accumulation
(sputnik/block/fp8.h, Fp8Accumulate::kFast). tests/fp8_fast_ref.py's chain
over interval sums is tied to the reference the shipped kernel already
matches, the Python layers reject a wrong `accumulate` before any library
call, and the new C entry points are declared and exported. No GPU work."""

import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import fp8_fast_ref as F
from tests import fp8_ref as R
from tests import rounding_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_SYMBOLS = ("sputnik_sdd_fp8_acc", "sputnik_dsd_fp8_acc",
             "sputnik_fp8_interval_sums")


def exact_sums_of(ops) -> np.ndarray:
    """P [k / 128, m, n] of fp8_ref.interval_sum, block row by block row."""
    p = np.empty((ops.k // R.B, ops.m, ops.n), np.float32)
    for kb in range(ops.k // R.B):
        ks = slice(kb * R.B, (kb + 1) * R.B)
        for rb in range(ops.m // R.B):
            rows = slice(rb * R.B, (rb + 1) * R.B)
            p[kb, rows], _ = R.interval_sum(ops.aq[rows, ks], ops.wq[:, ks])
    return p


CASES = ([("sdd", k) for k in R.SDD_DEEP_K] + [("dsd", R.DSD_DEEP_K)])


@pytest.mark.parametrize("kind,k", CASES,
                         ids=[f"{kind}-k{k}" for kind, k in CASES])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_chain_over_exact_interval_sums_is_the_reference(dtype, kind, k):
    ops = R.exact_case(kind, k)
    got = F.from_interval_sums(exact_sums_of(ops), ops.sa, ops.sw, ops.order,
                               dtype)
    want = R.rounded(ops.aq, ops.sa, ops.wq, ops.sw, dtype, ops.order)
    assert np.isfinite(want).all()
    assert np.array_equal(RR.bits(got, dtype), RR.bits(want, dtype))
    if kind == "dsd":   # ... and the order matters to it
        other = F.from_interval_sums(exact_sums_of(ops), ops.sa, ops.sw,
                                     [sorted(o) for o in ops.order], dtype)
        assert not np.array_equal(RR.bits(other, dtype), RR.bits(want, dtype))


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_chain_over_exact_interval_sums_keeps_the_ties(dtype):
    ops = R.tie_case(dtype)
    got = F.from_interval_sums(exact_sums_of(ops), ops.sa, ops.sw, None, dtype)
    want = R.rounded(ops.aq, ops.sa, ops.wq, ops.sw, dtype)
    assert np.array_equal(RR.bits(got, dtype), RR.bits(want, dtype))


def test_bound_fast_is_the_contracts():
    ref, absum = np.array([3.0]), np.array([10.0])
    assert F.EPS_FAST == 2.0 ** -7
    assert F.bound_fast(ref, absum, 256, "bf16")[0] == (
        2.0 ** -8 * 3.0 + (F.EPS_FAST + 5 * 2.0 ** -23) * 10.0)


def test_families_are_what_the_measurement_names():
    fam = F.families()
    for aq, bq in fam.values():
        assert aq.dtype == np.uint8 and bq.dtype == np.uint8
        assert aq.shape[1] == bq.shape[1]
        assert not any(d % 128 for d in aq.shape + bq.shape)
        assert np.isfinite(R.decode(aq)).all() and np.isfinite(R.decode(bq)).all()
    aq, bq = fam["random_bytes"]
    assert aq.shape == (256, 640) and bq.shape == (384, 640)
    assert len(np.unique(aq)) == 254
    a, b = (R.decode(v) for v in fam["large_among_small"])
    assert a.shape == (17 * 128, 128)
    # the large product at every position, with every ratio 2^-1 .. 2^-17
    assert sorted(set(np.argmax(a, axis=1))) == list(range(128))
    ratios = np.sort(np.unique(np.min(a, axis=1) / np.max(a, axis=1)))
    assert np.array_equal(ratios, 2.0 ** np.arange(-17.0, 0.0))
    assert (b == b[:, :1]).all()
    assert np.array_equal(np.unique(np.abs(b)), 2.0 ** np.arange(-9.0, 9.0))
    assert (b > 0).any() and (b < 0).any()
    a, _ = (R.decode(v) for v in fam["cancelling_large"])
    hi, lo = np.argmax(a, axis=1), np.argmin(a, axis=1)
    assert (a[np.arange(len(a)), lo] == -a[np.arange(len(a)), hi]).all()
    same = F.lane_group(hi) == F.lane_group(lo)
    assert same[:len(a) // 2].all() and not same[len(a) // 2:].any()


def _no_library(monkeypatch):
    import sputnik_amd as sp

    def lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(sp, "lib", lib)


@pytest.mark.parametrize("bad", ["fp16", "FAST", 1, None])
def test_bindings_reject_a_wrong_accumulate_before_the_library(monkeypatch,
                                                               bad):
    import sputnik_amd as sp

    _no_library(monkeypatch)
    for fn, args in ((sp.SddFp8, (None,) * 5), (sp.DsdFp8, (None,) * 5),
                     (sp.Fp8IntervalSums, (None,) * 3)):
        with pytest.raises(ValueError, match="accumulate"):
            fn(*args, accumulate=bad)


@pytest.mark.parametrize("bad", ["fp16", 1])
def test_ops_reject_a_wrong_accumulate_before_any_gpu_call(monkeypatch, bad):
    from sputnik_amd import ops

    _no_library(monkeypatch)
    x = torch.zeros(4, 128, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="accumulate"):
        ops.sdd_fp8(None, None, None, None, accumulate=bad)
    with pytest.raises(ValueError, match="accumulate"):
        ops.dsd_fp8(None, None, accumulate=bad)
    with pytest.raises(ValueError, match="accumulate"):
        ops.moe_mlp_fp8(x, None, None, None, None, 4, accumulate=bad)


def test_the_new_c_entry_points_are_declared_and_exported():
    import sputnik_amd as sp

    header = open(os.path.join(ROOT, "include", "sputnik_amd.h")).read()
    defined = subprocess.run(["nm", "-D", "--defined-only", sp.LIB_PATH],
                             capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in defined.splitlines() if line.strip()}
    for s in C_SYMBOLS:
        assert re.search(r"\bint %s\(" % s, header), s
        assert s in names, s
        assert s in sp._SIGNATURES, s
    # the entry points from before stay
    for s in ("sputnik_sdd_fp8", "sputnik_dsd_fp8"):
        assert s in names, s
