"""CPU: the host side of the gated SDD products (sputnik/block/gated.h): the
Python entry points and their exact signatures, the unchanged ops signatures,
the exported C and C++ symbols, type, size and None errors raised before the
library is called, and the C-ABI acceptance table without aborting. No
compute call is made (no GPU here).

Also the acceptance criterion (tests/gated_ref.py, activation_ref's
unchanged), with the GPU step stood in for by float32 numpy over every finite
fp16 / bf16 gate value and the constant factors the GPU tests use: the three
formulas pass within one step, and act' used where act belongs is rejected
at the two steps the GPU tests allow."""

import ctypes
import inspect
import subprocess

import numpy as np
import pytest

import sputnik_amd as sp
from tests import gated_ref as R

torch = pytest.importorskip("torch")

# The constant factors of the exhaustive GPU tests (tests/test_gpu_gated.py).
FORWARD_FACTORS = (1.0, -0.75, 0.375)
GRAD_FACTORS = ((1.0, 1.0), (-0.75, 0.5), (0.375, -1.0))


class _T:
    """Stand-in for a device tensor (tests/test_abi.py): only data_ptr() is
    read by the host checks; nothing is dereferenced."""

    def __init__(self, addr=0x1000):
        self.addr = addr

    def data_ptr(self):
        return self.addr


def _sparse(rows, cols, dtype, block=128, blocks=1):
    data = torch.zeros(1, 8, 8, dtype=dtype)  # (only its dtype is read)
    return sp.BlockMatrix(rows, cols, block, blocks * block * block, data,
                          _T(), _T(), row_indices=_T())


def _dense(rows, cols, dtype):
    return sp.Matrix(rows, cols, torch.zeros(1, dtype=dtype))


@pytest.fixture(autouse=True)
def gated_products_present():
    """Every test here is about the gated products: without them in the
    package (and the library) none of it holds."""
    assert hasattr(sp, "MatmulGated") and hasattr(sp, "BlockGateGrad")


@pytest.fixture
def no_library(monkeypatch):
    """Any use of the library fails the test."""
    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(sp, "lib", boom)


# ---- surface ------------------------------------------------------------------

def _params(fn):
    return list(inspect.signature(fn).parameters)


def test_python_entry_points_and_signatures():
    from sputnik_amd import ops
    assert _params(sp.MatmulGated) == [
        "a", "transpose_a", "b", "transpose_b", "c", "activation", "gate",
        "up", "stream", "workspace"]
    assert _params(sp.MatmulGatedGrad) == [
        "a", "transpose_a", "b", "transpose_b", "c", "activation", "gate",
        "up", "up_grad", "stream", "workspace"]
    sig = inspect.signature(sp.MatmulGated)
    assert sig.parameters["gate"].default is inspect.Parameter.empty
    assert sig.parameters["up"].default is None
    sig = inspect.signature(sp.MatmulGatedGrad)
    for name in ("gate", "up", "up_grad"):
        assert sig.parameters[name].default is inspect.Parameter.empty
    assert _params(sp.BlockGate) == ["u", "g", "activation", "out", "stream"]
    assert _params(sp.BlockGateGrad) == [
        "d", "g", "u", "activation", "dg", "du", "stream"]
    for name in ("MatmulGated", "MatmulGatedGrad", "BlockGate",
                 "BlockGateGrad"):
        assert name in sp.__all__, name
    assert _params(ops.sdd_gated) == [
        "a", "b", "topo", "gate", "activation", "a_grad_out", "b_grad_out"]
    assert _params(ops.glu_mlp) == [
        "x", "w1", "v1", "w2", "topo", "activation", "w1_grad_out",
        "v1_grad_out", "w2_grad_out"]
    assert (inspect.signature(ops.glu_mlp).parameters["activation"].default
            == "silu")
    for fn, names in ((ops.sdd_gated, ("a_grad_out", "b_grad_out")),
                      (ops.glu_mlp, ("w1_grad_out", "v1_grad_out",
                                     "w2_grad_out"))):
        for name in names:
            assert inspect.signature(fn).parameters[name].default is None
    assert "sdd_gated" in ops.__all__ and "glu_mlp" in ops.__all__


def test_existing_ops_signatures_unchanged():
    from sputnik_amd import ops
    assert hasattr(ops, "glu_mlp")                # (this change is present)
    assert _params(ops.sdd) == ["a", "b", "topo", "a_grad_out", "b_grad_out"]
    assert _params(ops.dsd) == ["a", "b", "b_grad_out"]
    assert _params(ops.dds) == ["a", "b", "a_grad_out"]
    assert _params(ops.sdd_act) == [
        "a", "b", "topo", "activation", "a_grad_out", "b_grad_out"]
    assert _params(ops.mlp) == [
        "x", "w1", "w2", "topo", "activation", "w1_grad_out", "w2_grad_out"]
    assert inspect.signature(ops.mlp).parameters["activation"].default == "gelu"
    assert _params(sp.MatmulActivation) == [
        "a", "transpose_a", "b", "transpose_b", "c", "activation",
        "pre_activation", "stream", "workspace"]


def _exported():
    return subprocess.run(["nm", "-D", "--defined-only", sp.LIB_PATH],
                          capture_output=True, text=True, check=True).stdout


def test_c_symbols_exported():
    out = _exported().split()
    for s in ("sputnik_sdd_gated", "sputnik_sdd_gated_grad",
              "sputnik_block_gate", "sputnik_block_gate_grad"):
        assert s in out, s
        assert hasattr(sp.lib(), s)


CPP_HEAD = "NS0_6MatrixEbS1_bNS0_11BlockMatrixENS0_10ActivationE"
CPP_TAIL = "NS0_8DataTypeEP12ihipStream_t"
CPP_SYMBOLS = (
    "_ZN7sputnik5block11MatmulGatedE" + CPP_HEAD + "PKvPv" + CPP_TAIL,
    "_ZN7sputnik5block15MatmulGatedGradE" + CPP_HEAD + "PKvS5_Pv" + CPP_TAIL,
)


def test_cpp_symbols_exported():
    """The two functions of sputnik/block/gated.h."""
    out = _exported()
    for sym in CPP_SYMBOLS:
        assert sym in out, sym


def test_one_knob_governs_both_families():
    """No second knob: sdd_act_route is the only route knob."""
    assert sp.tuning("sdd_act_route") == 0
    assert hasattr(sp, "MatmulGated")
    for name in ("sdd_gated_route", "sdd_gate_route", "gated_route"):
        with pytest.raises(KeyError):
            sp.tuning(name)


# ---- errors before the library ----------------------------------------------------

@pytest.mark.parametrize("grad", [False, True])
def test_type_and_size_errors_before_the_library(grad, no_library):
    h = torch.float16
    a, b = _dense(128, 64, h), _dense(64, 256, h)
    c = _sparse(128, 256, h, blocks=2)
    ok = torch.zeros(2 * 128 * 128, dtype=h)

    def f(a, ta, b, tb, c, act, gate, up=ok, up_grad=ok):
        if grad:
            return sp.MatmulGatedGrad(a, ta, b, tb, c, act, gate, up, up_grad)
        return sp.MatmulGated(a, ta, b, tb, c, act, gate, up)

    with pytest.raises(ValueError):                      # unknown activation
        f(a, False, b, False, c, "tanh", ok)
    with pytest.raises(ValueError):
        f(a, False, b, False, c, 3, ok)
    with pytest.raises(TypeError):                       # not an SDD
        f(c, False, b, False, c, "relu", ok)
    with pytest.raises(TypeError):
        f(a, False, b, False, _dense(128, 256, h), "relu", ok)
    with pytest.raises(TypeError):                       # mixed operand types
        f(a, False, _dense(64, 256, torch.bfloat16), False, c, "relu", ok)
    with pytest.raises(TypeError):
        f(_dense(128, 64, torch.float32), False, b, False, c, "relu", ok)
    with pytest.raises(TypeError):                       # the gate is required
        f(a, False, b, False, c, "relu", None)
    with pytest.raises(TypeError):                       # G of another type
        f(a, False, b, False, c, "relu", ok.to(torch.bfloat16))
    with pytest.raises(ValueError):                      # G of another size
        f(a, False, b, False, c, "relu", ok[:-8])
    with pytest.raises(ValueError):                      # strided G
        f(a, False, b, False, c, "relu",
          torch.zeros(4 * 128 * 128, dtype=h)[::2])
    with pytest.raises(TypeError):                       # U of another type
        f(a, False, b, False, c, "relu", ok, up=ok.to(torch.bfloat16))
    with pytest.raises(ValueError):                      # U of another size
        f(a, False, b, False, c, "relu", ok, up=ok[:-8])
    if grad:
        with pytest.raises(TypeError):                   # U, dU are required
            f(a, False, b, False, c, "relu", ok, up=None)
        with pytest.raises(TypeError):
            f(a, False, b, False, c, "relu", ok, up_grad=None)
        with pytest.raises(TypeError):
            f(a, False, b, False, c, "relu", ok,
              up_grad=ok.to(torch.bfloat16))
        with pytest.raises(ValueError):
            f(a, False, b, False, c, "relu", ok, up_grad=ok[:-8])


def test_block_gate_errors_before_the_library(no_library):
    z = torch.zeros(64, dtype=torch.float16)
    with pytest.raises(ValueError):
        sp.BlockGate(z, z, "elu")
    with pytest.raises(TypeError):
        sp.BlockGate(torch.zeros(64), torch.zeros(64), "relu")     # fp32
    with pytest.raises(TypeError):
        sp.BlockGate(z, z.to(torch.bfloat16), "relu")
    with pytest.raises(ValueError):
        sp.BlockGate(z, z[:32], "relu")
    with pytest.raises(TypeError):
        sp.BlockGate(z, z, "relu", out=torch.zeros(64, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        sp.BlockGate(z, z, "relu", out=torch.zeros(32, dtype=torch.float16))
    with pytest.raises(TypeError):
        sp.BlockGateGrad(z, z.to(torch.bfloat16), z, "relu")
    with pytest.raises(ValueError):
        sp.BlockGateGrad(z, z, z[:32], "relu")
    with pytest.raises(ValueError):
        sp.BlockGateGrad(z, z, z, 7)
    with pytest.raises(ValueError):
        sp.BlockGateGrad(z, z, z, "relu", dg=z[:32])
    with pytest.raises(TypeError):
        sp.BlockGateGrad(z, z, z, "relu", du=z.to(torch.bfloat16))
    out = torch.zeros(64, dtype=torch.float16)
    with pytest.raises(ValueError):                      # one tensor for both
        sp.BlockGateGrad(z, z, z, "relu", dg=out, du=out)


# ---- C-ABI acceptance ---------------------------------------------------------------

def _c_sparse(rows, cols, block):
    return sp.BlockMatrix(rows, cols, block, block * block, _T(), _T(), _T(),
                          row_indices=_T())._c()


def test_c_abi_acceptance_never_aborts():
    L = sp.lib()
    ref, P = ctypes.byref, ctypes.c_void_p
    a = sp.Matrix(256, 64, _T(0x3000))._c()
    b = sp.Matrix(64, 256, _T(0x4000))._c()
    c64, c128 = _c_sparse(256, 256, 64), _c_sparse(256, 256, 128)  # data 0x1000
    g, u, du = P(0x2000), P(0x5000), P(0x6000)
    inval, unsup = sp.hipErrorInvalidValue, sp.hipErrorNotSupported

    def fwd(a_, b_, c_, act=0, gate=g, up=u):
        return L.sputnik_sdd_gated(a_, 0, b_, 0, c_, act, gate, up, 0, None,
                                   0, None)

    def grad(a_, b_, c_, act=0, gate=g, up=u, up_grad=du):
        return L.sputnik_sdd_gated_grad(a_, 0, b_, 0, c_, act, gate, up,
                                        up_grad, 0, None, 0, None)

    for fn in (fwd, grad):
        for act in (3, -1, 100):                         # unknown activation
            assert fn(ref(a), ref(b), ref(c128), act=act) == inval
        for args in ((None, ref(b), ref(c128)), (ref(a), None, ref(c128)),
                     (ref(a), ref(b), None)):            # null operand
            assert fn(*args) == inval
        assert fn(ref(a), ref(b), ref(c64)) == unsup     # block size 64
        # a shape the plain SDD rejects: K mismatch
        bad_k = sp.Matrix(72, 256, _T(0x4000))._c()
        assert fn(ref(a), ref(bad_k), ref(c128)) == inval
        assert L.sputnik_sdd(ref(a), 0, ref(bad_k), 0, ref(c128), 0,
                             None) == inval
        assert fn(ref(a), ref(b), ref(c128), gate=None) == inval  # null gate
        # a side buffer that equals one it must not overlap
        assert fn(ref(a), ref(b), ref(c128), gate=P(0x1000)) == inval  # C
        assert fn(ref(a), ref(b), ref(c128), gate=P(0x3000)) == inval  # A
        assert fn(ref(a), ref(b), ref(c128), gate=P(0x4000)) == inval  # B
        assert fn(ref(a), ref(b), ref(c128), up=P(0x1000)) == inval  # up == C
        assert fn(ref(a), ref(b), ref(c128), up=P(0x3000)) == inval
        assert fn(ref(a), ref(b), ref(c128), up=P(0x4000)) == inval
        assert fn(ref(a), ref(b), ref(c128), up=g) == inval      # up == gate
    # null up / up_grad: required by the gradient only
    assert grad(ref(a), ref(b), ref(c128), up=None) == inval
    assert grad(ref(a), ref(b), ref(c128), up_grad=None) == inval
    assert grad(ref(a), ref(b), ref(c128), up_grad=g) == inval   # == gate
    assert grad(ref(a), ref(b), ref(c128), up_grad=P(0x1000)) == inval
    assert grad(ref(a), ref(b), ref(c128), up_grad=P(0x3000)) == inval
    assert grad(ref(a), ref(b), ref(c128), up_grad=P(0x4000)) == inval
    # missing row indices is reported, not aborted on
    no_rows = sp.BlockMatrix(256, 256, 128, 128 * 128, _T(), _T(), _T())._c()
    assert fwd(ref(a), ref(b), ref(no_rows), up=None) == inval
    assert grad(ref(a), ref(b), ref(no_rows)) == inval


def test_block_gate_c_abi():
    L = sp.lib()
    p, q = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000)
    inval = sp.hipErrorInvalidValue
    assert L.sputnik_block_gate(p, p, p, 64, 3, 0, None) == inval
    assert L.sputnik_block_gate(p, p, p, 64, 0, 2, None) == inval
    assert L.sputnik_block_gate(p, p, p, -1, 0, 0, None) == inval
    assert L.sputnik_block_gate(None, p, p, 64, 0, 0, None) == inval
    assert L.sputnik_block_gate(p, None, p, 64, 0, 0, None) == inval
    assert L.sputnik_block_gate(p, p, None, 64, 0, 0, None) == inval
    assert L.sputnik_block_gate(None, None, None, 0, 0, 0, None) == 0
    gg = L.sputnik_block_gate_grad
    assert gg(None, p, p, p, q, 64, 0, 0, None) == inval
    assert gg(p, None, p, p, q, 64, 0, 0, None) == inval
    assert gg(p, p, None, p, q, 64, 0, 0, None) == inval
    assert gg(p, p, p, None, q, 64, 0, 0, None) == inval
    assert gg(p, p, p, p, None, 64, 0, 0, None) == inval
    assert gg(p, p, p, p, p, 64, 0, 0, None) == inval    # dg == du
    assert gg(p, p, p, p, q, 64, 9, 0, None) == inval
    assert gg(p, p, p, p, q, 64, 0, 5, None) == inval
    assert gg(p, p, p, p, q, -2, 0, 0, None) == inval
    assert gg(p, p, p, p, q, 0, 1, 1, None) == 0


# ---- the criterion, with float32 numpy standing in for the GPU ------------------------

_INPUTS = {}


def _inputs(dtype):
    if dtype not in _INPUTS:
        bits = R.all_finite_bits(dtype)
        _INPUTS[dtype] = (bits, R.bits_to_f64(bits, dtype))
    return _INPUTS[dtype]


def _round(x32, dtype):
    return R.round_bits(x32.astype(np.float64), dtype)


@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_float32_formulas_meet_the_criterion(dtype, act):
    """Every finite G and the GPU tests' constant factors: a float32
    evaluation of H, dU and dG meets the criterion, finite, relu exact, and
    is within one step wherever the true result is at least 7e-37 (below
    that fp32 itself is subnormal)."""
    _, g = _inputs(dtype)
    cases = []
    for f in FORWARD_FACTORS:
        cases.append((f"H f={f}", R.gate32(act, f, g), R.gate64(act, f, g)))
    for d, u in GRAD_FACTORS:
        cases.append((f"dU d={d}", R.gate32(act, d, g), R.gate_du64(act, d, g)))
        cases.append((f"dG d={d} u={u}", R.gate_dg32(act, d, u, g),
                      R.gate_dg64(act, d, u, g)))
    for what, got32, ref in cases:
        assert np.isfinite(ref).all()
        got = _round(got32, dtype)
        worst = R.check(got, ref, dtype, f"{what} {act} {dtype}")
        if act == "relu":
            assert worst == 0, what
        big = np.abs(ref) >= 7e-37
        steps = R.steps_between(got, R.round_bits(ref, dtype))
        assert not (steps[big] > 1).any(), (what, int(steps[big].max()))


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_criterion_rejects_the_derivative_in_place_of_the_activation(dtype):
    """silu' used where silu belongs (and the reverse, in dG): rejected at the
    two steps allowed."""
    _, g = _inputs(dtype)
    wrong_h = _round(R.gate32("silu", 1.0, g, grad_of_act=True), dtype)
    _, bad, _ = R.measure(wrong_h, R.gate64("silu", 1.0, g), dtype)
    assert bad > 1000, bad
    wrong_dg = _round(R.gate32("silu", 1.0, g), dtype)
    _, bad, _ = R.measure(wrong_dg, R.gate_dg64("silu", 1.0, 1.0, g), dtype)
    assert bad > 1000, bad
    # ... and U left out of dG
    no_u = _round(R.gate32("gelu", -0.75, g, grad_of_act=True), dtype)
    _, bad, _ = R.measure(no_u, R.gate_dg64("gelu", -0.75, 0.5, g), dtype)
    assert bad > 1000, bad
