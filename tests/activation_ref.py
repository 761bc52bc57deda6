"""Float64 reference and acceptance criterion of the SDD activation products
(sputnik/block/activation.h), shared by tests/test_activation_host.py and
tests/test_gpu_activation*.py. Nothing here calls the library.

Criterion for the elementwise stage, with ref = round_T(f64 formula):
  |ref| >= 2^-100: the result is within MAX_STEPS = 2 representable steps of
                   T from ref;
  |ref| <  2^-100: its magnitude is <= 2^-100 (where fp32 exp underflows).
A correctly rounded fp32 evaluation of the formulas stays within 1 step
(test_activation_host.py measures it over every finite input); the second
step is the margin for the device's exp and reciprocal, which are not
correctly rounded."""

from __future__ import annotations

import numpy as np

ACTS = ("relu", "gelu", "silu")
MAX_STEPS = 2
TINY = 2.0 ** -100
_C = np.sqrt(2.0 / np.pi)


# ---- 16-bit formats ---------------------------------------------------------

def all_finite_bits(dtype: str) -> np.ndarray:
    """Every 16-bit pattern of T as uint16 [65536], non-finite ones -> 0."""
    b = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    b[~np.isfinite(bits_to_f64(b, dtype))] = 0
    return b


def bits_to_f64(bits: np.ndarray, dtype: str) -> np.ndarray:
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    if dtype == "f16":
        return bits.view(np.float16).astype(np.float64)
    with np.errstate(invalid="ignore"):  # (signalling NaN patterns)
        return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def round_bits(x: np.ndarray, dtype: str) -> np.ndarray:
    """round_T of float64 values, as uint16 bit patterns (round to nearest
    even, straight from float64: no double rounding through fp32)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if dtype == "f16":
        with np.errstate(over="ignore"):
            return x.astype(np.float16).view(np.uint16)
    # bf16: keep 7 mantissa bits of the float64, then narrow (exact for
    # results in fp32's normal range; below it only the magnitude is checked).
    u = x.view(np.uint64)
    keep = np.uint64(45)
    bias = ((u >> keep) & np.uint64(1)) + np.uint64((1 << 44) - 1)
    r = ((u + bias) >> keep) << keep
    with np.errstate(over="ignore", under="ignore"):
        f = r.view(np.float64).astype(np.float32)
    return (f.view(np.uint32) >> 16).astype(np.uint16)


def _ordinal(bits: np.ndarray) -> np.ndarray:
    """Position on T's number line (+0 and -0 coincide)."""
    b = bits.astype(np.int32)
    mag = b & 0x7FFF
    return np.where(b & 0x8000, -mag, mag)


def steps_between(a_bits, b_bits) -> np.ndarray:
    return np.abs(_ordinal(np.asarray(a_bits)) - _ordinal(np.asarray(b_bits)))


# ---- float64 formulas -------------------------------------------------------

def _sigmoid(t):
    with np.errstate(over="ignore", under="ignore"):
        e = np.exp(-np.abs(t))
        return np.where(t >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def act64(act: str, x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    if act == "relu":
        return np.where(x > 0, x, 0.0)
    if act == "gelu":
        return x * _sigmoid(2.0 * _C * (x + 0.044715 * x ** 3))
    return x * _sigmoid(x)


def dact64(act: str, x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    if act == "relu":
        return np.where(x > 0, 1.0, 0.0)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        if act == "gelu":
            t = 2.0 * _C * (x + 0.044715 * x ** 3)
            s, oms = _sigmoid(t), _sigmoid(-t)
            tail = x * s * oms * (2.0 * _C) * (1.0 + 0.134145 * x * x)
            # (s (1 - s) underflows to 0 long before x^2 can overflow)
            return s + np.where(s * oms == 0.0, 0.0, tail)
        s, oms = _sigmoid(x), _sigmoid(-x)
        return s * (1.0 + np.where(oms == 0.0, 0.0, x * oms))


# ---- fp32 evaluation of the library's formulas (the CPU stand-in) ------------

def act32(act: str, x, coeff=0.044715, grad=False) -> np.ndarray:
    """The formulas of activation.h in float32 numpy, clamped as the device
    code clamps (gelu |x| <= 11, silu |x| <= 100). `coeff` lets the mutation
    test swap gelu's cubic coefficient."""
    f = np.float32
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore", under="ignore"):
        if act == "relu":
            return np.where(x > 0, f(1) if grad else x, f(0)).astype(np.float32)
        if act == "gelu":
            xc = np.clip(x, f(-11), f(11))
            c = f(_C)
            u = c * (xc + f(coeff) * (xc * xc * xc))
            s = f(1) / (f(1) + np.exp(-(f(2) * u)))
            if not grad:
                return x * s
            return s + xc * s * (f(1) - s) * (f(2) * c) * (
                f(1) + f(3 * coeff) * (xc * xc))
        xc = np.clip(x, f(-100), f(100))
        s = f(1) / (f(1) + np.exp(-xc))
        return x * s if not grad else s * (f(1) + xc * (f(1) - s))


# ---- the criterion ----------------------------------------------------------

def check(got_bits, ref64, dtype: str, what: str, max_steps: int = MAX_STEPS):
    """Asserts the criterion; returns the worst step count seen among the
    elements with |ref| >= 2^-100."""
    worst, bad, msg = measure(got_bits, ref64, dtype, max_steps)
    assert bad == 0, f"{what}: {msg}"
    return worst


def measure(got_bits, ref64, dtype: str, max_steps: int = MAX_STEPS):
    got_bits = np.asarray(got_bits, dtype=np.uint16).ravel()
    ref64 = np.asarray(ref64, dtype=np.float64).ravel()
    assert got_bits.shape == ref64.shape, (got_bits.shape, ref64.shape)
    ref_bits = round_bits(ref64, dtype)
    ref = bits_to_f64(ref_bits, dtype)
    got = bits_to_f64(got_bits, dtype)
    big = np.abs(ref) >= TINY
    steps = steps_between(got_bits, ref_bits)
    fail = np.where(big, steps > max_steps, ~(np.abs(got) <= TINY))
    fail |= ~np.isfinite(got)
    worst = int(steps[big].max()) if big.any() else 0
    msg = ""
    if fail.any():
        i = int(np.flatnonzero(fail)[0])
        msg = (f"{int(fail.sum())}/{fail.size} elements out of bounds; first "
               f"at {i}: got {got[i]!r} ref {ref[i]!r} ({int(steps[i])} steps); "
               f"worst {worst} steps")
    return worst, int(fail.sum()), msg
