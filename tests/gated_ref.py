"""Float64 references of the gated SDD products (sputnik/block/gated.h),
shared by tests/test_gated_host.py and tests/test_gpu_gated*.py. Nothing here
calls the library.

    gate64     u act(g)            H,  of MatmulGated / BlockGate
    gate_du64  d act(g)            dU, of MatmulGatedGrad / BlockGateGrad
    gate_dg64  d u act'(g)         dG

The formats, the float64 activations and the criterion are
tests/activation_ref.py's, unchanged: at most MAX_STEPS = 2 representable
steps from round_T(reference), and below 2^-100 the magnitude only. The
products add one exact fp32 multiply (d u: two significands of at most 11
bits) and one rounded one to what the activation products do, and a correctly
rounded fp32 evaluation still stays within 1 step
(test_gated_host.py measures it over every finite G)."""

from __future__ import annotations

import numpy as np

from tests.activation_ref import (ACTS, MAX_STEPS, TINY, act32, act64,  # noqa: F401
                                  all_finite_bits, bits_to_f64, check, dact64,
                                  measure, round_bits, steps_between)


def round_bits_exact(x, dtype: str) -> np.ndarray:
    """round_T of float64 values as uint16 bit patterns, correct over the
    whole range. activation_ref.round_bits is exact for bf16 only in fp32's
    normal range (the criterion checks nothing but the magnitude below that);
    the bit-for-bit relu tests here reach bf16's subnormals, which are whole
    multiples of 2^-133, rounded to nearest even."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    bits = round_bits(x, dtype)
    if dtype == "bf16":
        small = np.abs(x) < 2.0 ** -126
        q = np.rint(np.abs(x[small]) * 2.0 ** 133).astype(np.uint16)  # <= 128
        bits[small] = q | (np.signbit(x[small]).astype(np.uint16) << 15)
    return bits


def gate64(act: str, u, g) -> np.ndarray:
    return np.asarray(u, dtype=np.float64) * act64(act, g)


def gate_du64(act: str, d, g) -> np.ndarray:
    return np.asarray(d, dtype=np.float64) * act64(act, g)


def gate_dg64(act: str, d, u, g) -> np.ndarray:
    return (np.asarray(d, dtype=np.float64) * np.asarray(u, dtype=np.float64)
            * dact64(act, g))


# ---- fp32 evaluation of the library's formulas (the CPU stand-in) ------------

def gate32(act: str, u, g, grad_of_act: bool = False) -> np.ndarray:
    """float32(u) * act(float32(g)) in float32 numpy (act' when grad_of_act),
    + 0.0 as the device code adds it."""
    u = np.asarray(u, dtype=np.float32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return (u * act32(act, g, grad=grad_of_act) + np.float32(0)).astype(
            np.float32)


def gate_dg32(act: str, d, u, g) -> np.ndarray:
    """(d u) act'(g) in float32: the product d u first, as gated.h has it."""
    d = np.asarray(d, dtype=np.float32)
    u = np.asarray(u, dtype=np.float32)
    return gate32(act, d * u, g, grad_of_act=True)
