"""Host checks of tests/rounding_ref.py: the bit-level conversion model
against numpy and torch, and, for every case the GPU tests run
(tests/test_gpu_rounding.py, tests/test_gpu_nonfinite.py), that its inputs
can tell a wrong kernel from a right one.

Per case, printed and asserted:
  * the builder's bound (max |sum| < 2^24, < 65504 for fp16) held: Host
    asserts it while building;
  * at least 25 % of the outputs are not representable, so the conversion
    does something;
  * ties occur, and ties-to-even sends some up and some down;
  * every wrong model that applies to the case differs from round_once in
    at least 5 % of the outputs (truncate and round_half_up always;
    partial_in_T where the path has a hand-off; accumulate_twice for an
    accumulation into a C of the operand type).
The 5 % and 25 % are conditions on the inputs. A case that misses one gets
other values, not another floor.
"""

import numpy as np
import pytest

from tests import rounding_ref as R

torch = pytest.importorskip("torch")

MIN_UNREPRESENTABLE = 0.25
MIN_DIFFERENT = 0.05


# ---------------------------------------------------------------- round_once --

def _probe_values(rng):
    """float32 values (exact in float64) over T's whole range: normals,
    fp16 subnormals, the overflow threshold, zeros, and every midpoint
    between neighbouring fp16 / bf16 values in a few binades."""
    parts = [
        rng.standard_normal(20000).astype(np.float32),
        np.ldexp(rng.standard_normal(20000), rng.integers(-30, 18, 20000)
                 ).astype(np.float32),
        np.ldexp(rng.integers(-5000, 5000, 20000).astype(np.float32), -25),
        rng.uniform(65000, 66000, 4000).astype(np.float32),
        -rng.uniform(65000, 66000, 4000).astype(np.float32),
        np.arange(-8200, 8200, dtype=np.float32),
        np.arange(60000, 70000, dtype=np.float32),
        np.ldexp(np.arange(0, 4200, dtype=np.float32), -25),   # subnormal ties
        np.array([0.0, -0.0, np.inf, -np.inf, 65504, 65519.996, 65520,
                  2.0 ** -24, 2.0 ** -25, 2.0 ** -26, 3 * 2.0 ** -26],
                 np.float32),
    ]
    return np.concatenate(parts)


def test_round_once_matches_numpy_f16():
    x = _probe_values(np.random.default_rng(0))
    with np.errstate(over="ignore"):
        want = x.astype(np.float64).astype(np.float16)
    got = R.round_once(x.astype(np.float64), "f16")
    assert np.array_equal(R.bits(got, "f16"), want.view(np.uint16))
    nan = R.round_once(np.array([np.nan]), "f16")
    assert np.isnan(nan).all()


def test_round_once_matches_torch_bf16():
    x = _probe_values(np.random.default_rng(1))
    big = np.ldexp(np.random.default_rng(2).standard_normal(20000),
                   np.random.default_rng(3).integers(-100, 120, 20000)
                   ).astype(np.float32)
    x = np.concatenate([x, big, np.arange(0, 70000, dtype=np.float32)])
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy()
    got = R.round_once(x.astype(np.float64), "bf16")
    assert np.array_equal(R.bits(got, "bf16"), want.view(np.uint16))


def test_round_once_needs_no_double_rounding():
    """A float64 just above an fp16 tie rounds up although float32 would
    first round it onto the tie (and then to even, down)."""
    x = np.array([2049.0 + 2.0 ** -30, 2048.0 + 1.0 - 2.0 ** -30])
    assert R.round_once(x, "f16").tolist() == [2050.0, 2048.0]


@pytest.mark.parametrize("dtype,value,want", [
    ("f16", 2049, 2048), ("f16", 2051, 2052), ("f16", 65519, 65504),
    ("f16", 65520, np.inf), ("f16", -65520, -np.inf),
    ("f16", 3 * 65536, np.inf),
    ("bf16", 257, 256), ("bf16", 259, 260), ("bf16", 385, 384),
])
def test_round_once_boundary_integers(dtype, value, want):
    assert float(R.round_once(np.array([float(value)]), dtype)[0]) == want


def test_wrong_models_on_known_values():
    x = np.array([2049.0, 2051.0, 2050.5, -2049.0, 65519.0, 65520.0])
    assert R.truncate(x, "f16").tolist() == [2048, 2050, 2050, -2048, 65504,
                                             65504]
    assert R.round_half_up(x, "f16").tolist() == [2050, 2052, 2050, -2050,
                                                  65504, np.inf]
    # 2049 + 2051 = 4100 exactly; rounded first, 2048 + 2052 = 4100 too,
    # but 2049 + 1 = 2050 exactly and 2048 + 1 = 2049 -> 2048 rounded first
    assert R.partial_in_T([np.array([2049.0]), np.array([2051.0])],
                          "f16").tolist() == [4100.0]
    assert R.partial_in_T([np.array([2049.0]), np.array([1.0])],
                          "f16").tolist() == [2048.0]
    assert R.accumulate_twice(np.array([2049.0]), np.array([1.0]),
                              "f16").tolist() == [2048.0]
    assert R.round_once(np.array([2050.0]), "f16").tolist() == [2050.0]


def test_scaled_is_exact():
    v = np.arange(0, 1024, dtype=np.float32)
    for e in (-24, -10, 4):
        s = R.scaled(v, e)
        assert s.dtype == np.float32
        assert np.array_equal(s.astype(np.float64), v.astype(np.float64) * 2.0 ** e)


def test_moated_view_and_bands():
    view, whole, pad = R.moated((5, 1032), torch.float16, float("nan"),
                                device="cpu")
    assert pad % 4096 == 0 and pad >= 128 * 1032
    assert view.is_contiguous() and view.shape == (5, 1032)
    assert view.data_ptr() == whole.data_ptr() + 2 * pad
    assert whole.numel() == 2 * pad + 5 * 1032
    out, w2, p2 = R.moated((3, 8), torch.int16, 0x7E5A, device="cpu")
    assert R.moat_intact(w2, p2, 0x7E5A)
    w2[p2 - 1] = 0
    assert not R.moat_intact(w2, p2, 0x7E5A)
    w2[p2 - 1] = 0x7E5A
    w2[p2 + 24] = 0
    assert not R.moat_intact(w2, p2, 0x7E5A)


# ----------------------------------------------------- expected_with_specials --

def test_expected_with_specials_is_local_and_ieee():
    rng = np.random.default_rng(5)
    x = rng.integers(0, 4, (6, 8)).astype(np.float64)
    y = rng.integers(-3, 4, (8, 5)).astype(np.float64)
    x[2, 3] = np.nan
    x[4, 1] = np.inf
    y[1, :] = np.abs(y[1, :]) + 1       # inf * positive
    y[1, 2] = 0.0                       # inf * 0 = NaN
    y[6, 4] = -np.inf
    x[:, 6] = np.abs(x[:, 6]) + 1
    got = R.expected_with_specials(x, None, y, None)
    with np.errstate(invalid="ignore"):
        want = (x[:, :, None] * y[None, :, :]).sum(axis=1)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok], want[ok])
    assert np.isnan(got[2]).all() and np.isnan(got[4, 2])
    assert (got[[0, 1, 3, 5], 4] == -np.inf).all()
    assert np.isfinite(got[[0, 1, 3, 5], :4]).all()


def test_expected_with_specials_unstored_terms_do_not_exist():
    x = np.ones((4, 4))
    y = np.ones((4, 3))
    y[1, :] = np.nan                    # row 1 of the dense operand
    xs = np.ones((4, 4), bool)
    xs[:, 1] = False                    # no row stores column 1
    x[:, 1] = 0.0
    got = R.expected_with_specials(x, xs, y, None)
    assert np.array_equal(got, np.full((4, 3), 3.0))
    xs[2, 1] = True                     # row 2 stores it: only row 2 is hit
    got = R.expected_with_specials(x, xs, y, None)
    assert np.isnan(got[2]).all() and np.isfinite(got[[0, 1, 3]]).all()


# ------------------------------------------------------------------ the cases --

ALL_CASES = list(R.ROUNDING_CASES) + list(R.ACCUMULATE_CASES) \
    + list(R.NONFINITE_CASES)


def test_case_ids_are_unique():
    ids = [c.id + str(c.acc) for c in ALL_CASES]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.id + (c.acc or ""))
def test_case_discriminates(case):
    h = R.host(case)                    # asserts the builder's bound
    dt = case.dtype
    if case.acc == "f32":               # exact in fp32: nothing is rounded
        assert np.array_equal(h.expected().astype(np.float64), h.total)
        return
    total = h.layout(h.total)
    right = h.layout(R.round_once(h.total, dt))
    n = right.size
    unrep = float((right.astype(np.float64) != total).mean())
    down = h.layout(R.truncate(h.total, dt))
    up = h.layout(R.round_half_up(h.total, dt))
    tie = (up != down) & (np.abs(up.astype(np.float64) - total)
                          == np.abs(total - down.astype(np.float64)))
    ties_up = int((tie & (right == up)).sum())
    ties_down = int((tie & (right == down)).sum())
    share = {"truncate": float((down != right).mean()),
             "round_half_up": float((up != right).mean())}
    if case.handoff is not None:
        share["partial_in_T"] = float(
            (h.layout(R.partial_in_T(h.parts, dt)) != right).mean())
    if case.acc == "operand":
        twice = R.accumulate_twice(h.P, h.c_in.astype(np.float64), dt)
        share["accumulate_twice"] = float((h.layout(twice) != right).mean())
    print(f"{case.id}: a_max {h.a_max} b_max {h.b_max} max|sum| {h.peak:.0f} "
          f"outputs {n} unrepresentable {unrep:.3f} ties up/down "
          f"{ties_up}/{ties_down} " +
          " ".join(f"{k} {v:.3f}" for k, v in share.items()))
    assert np.array_equal(sum(h.parts), h.P)
    assert unrep >= MIN_UNREPRESENTABLE
    assert ties_up > 0 and ties_down > 0
    for model, s in share.items():
        assert s >= MIN_DIFFERENT, (model, s)
