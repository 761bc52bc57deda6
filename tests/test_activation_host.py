"""CPU: the host side of the SDD activation products
(sputnik/block/activation.h): the Python entry points and their exact
signatures, the unchanged ops signatures, the exported C and C++ symbols,
type and size errors raised before the library is called, and the C-ABI
acceptance table without aborting. No compute call is made (no GPU here).

Also the acceptance criterion itself (tests/activation_ref.py), with the GPU
step stood in for by float32 numpy over every finite fp16 / bf16 input: the
formulas pass within one step, and a wrong gelu coefficient (0.0447 for
0.044715) is rejected at the two steps the GPU tests allow."""

import ctypes
import inspect
import subprocess

import numpy as np
import pytest

import sputnik_amd as sp
from tests import activation_ref as R

torch = pytest.importorskip("torch")


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
    assert _params(sp.MatmulActivation) == [
        "a", "transpose_a", "b", "transpose_b", "c", "activation",
        "pre_activation", "stream", "workspace"]
    assert _params(sp.MatmulActivationGrad) == [
        "a", "transpose_a", "b", "transpose_b", "c", "activation",
        "pre_activation", "stream", "workspace"]
    sig = inspect.signature(sp.MatmulActivation)
    assert sig.parameters["pre_activation"].default is None
    sig = inspect.signature(sp.MatmulActivationGrad)
    assert sig.parameters["pre_activation"].default is inspect.Parameter.empty
    assert _params(sp.BlockActivation) == ["z", "activation", "out", "stream"]
    assert _params(sp.BlockActivationGrad) == [
        "g", "z", "activation", "out", "stream"]
    for name in ("MatmulActivation", "MatmulActivationGrad", "BlockActivation",
                 "BlockActivationGrad", "SPUTNIK_ACT_RELU", "SPUTNIK_ACT_GELU",
                 "SPUTNIK_ACT_SILU"):
        assert name in sp.__all__, name
    assert (sp.SPUTNIK_ACT_RELU, sp.SPUTNIK_ACT_GELU,
            sp.SPUTNIK_ACT_SILU) == (0, 1, 2)
    assert _params(ops.sdd_act) == [
        "a", "b", "topo", "activation", "a_grad_out", "b_grad_out"]
    assert _params(ops.mlp) == [
        "x", "w1", "w2", "topo", "activation", "w1_grad_out", "w2_grad_out"]
    assert inspect.signature(ops.mlp).parameters["activation"].default == "gelu"
    for fn, names in ((ops.sdd_act, ("a_grad_out", "b_grad_out")),
                      (ops.mlp, ("w1_grad_out", "w2_grad_out"))):
        for name in names:
            assert inspect.signature(fn).parameters[name].default is None
    assert "sdd_act" in ops.__all__ and "mlp" in ops.__all__


def test_existing_ops_signatures_unchanged():
    from sputnik_amd import ops
    assert _params(ops.sdd) == ["a", "b", "topo", "a_grad_out", "b_grad_out"]
    assert _params(ops.dsd) == ["a", "b", "b_grad_out"]
    assert _params(ops.dds) == ["a", "b", "a_grad_out"]


def _exported():
    return subprocess.run(["nm", "-D", "--defined-only", sp.LIB_PATH],
                          capture_output=True, text=True, check=True).stdout


def test_c_symbols_exported():
    out = _exported().split()
    for s in ("sputnik_sdd_act", "sputnik_sdd_act_grad",
              "sputnik_block_activation", "sputnik_block_activation_grad"):
        assert s in out, s
        assert hasattr(sp.lib(), s)


def test_cpp_symbols_exported():
    """The two functions of sputnik/block/activation.h."""
    out = _exported()
    head = "NS0_6MatrixEbS1_bNS0_11BlockMatrixENS0_10ActivationE"
    tail = "NS0_8DataTypeEP12ihipStream_t"
    for sym in ("_ZN7sputnik5block16MatmulActivationE" + head + "Pv" + tail,
                "_ZN7sputnik5block20MatmulActivationGradE" + head + "PKv"
                + tail):
        assert sym in out, sym


def test_knob_is_listed():
    assert sp.tuning("sdd_act_route") == 0
    with pytest.raises(KeyError):
        sp.tuning("sdd_act_route", 3)
    assert sp.tuning("sdd_act_route") == 0


# ---- errors before the library ----------------------------------------------------

@pytest.mark.parametrize("fn", ["MatmulActivation", "MatmulActivationGrad"])
def test_type_and_size_errors_before_the_library(fn, no_library):
    f = getattr(sp, fn)
    h = torch.float16
    a, b = _dense(128, 64, h), _dense(64, 256, h)
    c = _sparse(128, 256, h, blocks=2)
    z_ok = torch.zeros(2 * 128 * 128, dtype=h)
    with pytest.raises(ValueError):                      # unknown activation
        f(a, False, b, False, c, "tanh", z_ok)
    with pytest.raises(ValueError):
        f(a, False, b, False, c, 3, z_ok)
    with pytest.raises(TypeError):                       # not an SDD
        f(c, False, b, False, c, "relu", z_ok)
    with pytest.raises(TypeError):
        f(a, False, b, False, _dense(128, 256, h), "relu", z_ok)
    with pytest.raises(TypeError):                       # mixed operand types
        f(a, False, _dense(64, 256, torch.bfloat16), False, c, "relu", z_ok)
    with pytest.raises(TypeError):
        f(_dense(128, 64, torch.float32), False, b, False, c, "relu", z_ok)
    with pytest.raises(TypeError):                       # Z of another type
        f(a, False, b, False, c, "relu", z_ok.to(torch.bfloat16))
    with pytest.raises(ValueError):                      # Z of another size
        f(a, False, b, False, c, "relu", z_ok[:-8])
    with pytest.raises(ValueError):                      # strided Z
        f(a, False, b, False, c, "relu",
          torch.zeros(4 * 128 * 128, dtype=h)[::2])


def test_grad_needs_the_pre_activation(no_library):
    h = torch.float16
    with pytest.raises(TypeError):
        sp.MatmulActivationGrad(_dense(128, 64, h), False, _dense(64, 256, h),
                                False, _sparse(128, 256, h, blocks=2), "relu",
                                None)


def test_block_activation_errors_before_the_library(no_library):
    z = torch.zeros(64, dtype=torch.float16)
    with pytest.raises(ValueError):
        sp.BlockActivation(z, "elu")
    with pytest.raises(TypeError):
        sp.BlockActivation(torch.zeros(64), "relu")      # fp32
    with pytest.raises(TypeError):
        sp.BlockActivation(z, "relu", out=torch.zeros(64, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        sp.BlockActivation(z, "relu", out=torch.zeros(32, dtype=torch.float16))
    with pytest.raises(TypeError):
        sp.BlockActivationGrad(z.to(torch.bfloat16), z, "relu")
    with pytest.raises(ValueError):
        sp.BlockActivationGrad(z[:32], z, "relu")
    with pytest.raises(ValueError):
        sp.BlockActivationGrad(z, z, 7)


# ---- C-ABI acceptance ---------------------------------------------------------------

def _c_sparse(rows, cols, block):
    return sp.BlockMatrix(rows, cols, block, block * block, _T(), _T(), _T(),
                          row_indices=_T())._c()


def test_c_abi_acceptance_never_aborts():
    L = sp.lib()
    fwd, grad = L.sputnik_sdd_act, L.sputnik_sdd_act_grad
    ref = ctypes.byref
    a, b = sp.Matrix(256, 64, _T())._c(), sp.Matrix(64, 256, _T())._c()
    c64, c128 = _c_sparse(256, 256, 64), _c_sparse(256, 256, 128)
    z = ctypes.c_void_p(0x2000)
    inval, unsup = sp.hipErrorInvalidValue, sp.hipErrorNotSupported
    for fn in (fwd, grad):
        for act in (3, -1, 100):                         # unknown activation
            assert fn(ref(a), 0, ref(b), 0, ref(c128), act, z, 0, None, 0,
                      None) == inval
        for args in ((None, ref(b), ref(c128)), (ref(a), None, ref(c128)),
                     (ref(a), ref(b), None)):            # null operand
            assert fn(args[0], 0, args[1], 0, args[2], 0, z, 0, None, 0,
                      None) == inval
        assert fn(ref(a), 0, ref(b), 0, ref(c64), 0, z, 0, None, 0,
                  None) == unsup                         # block size 64
        # shapes the plain SDD rejects: K mismatch, N not a multiple of 8
        bad_k = sp.Matrix(72, 256, _T())._c()
        assert fn(ref(a), 0, ref(bad_k), 0, ref(c128), 0, z, 0, None, 0,
                  None) == inval
        assert L.sputnik_sdd(ref(a), 0, ref(bad_k), 0, ref(c128), 0,
                             None) == inval
        # z == c.data
        assert fn(ref(a), 0, ref(b), 0, ref(c128), 0,
                  ctypes.c_void_p(0x1000), 0, None, 0, None) == inval
    # a null z: required by the gradient only
    assert grad(ref(a), 0, ref(b), 0, ref(c128), 0, None, 0, None, 0,
                None) == inval
    # missing row indices is reported, not aborted on
    no_rows = sp.BlockMatrix(256, 256, 128, 128 * 128, _T(), _T(), _T())._c()
    assert fwd(ref(a), 0, ref(b), 0, ref(no_rows), 0, None, 0, None, 0,
               None) == inval


def test_block_activation_c_abi():
    L = sp.lib()
    p = ctypes.c_void_p(0x1000)
    inval = sp.hipErrorInvalidValue
    assert L.sputnik_block_activation(p, p, 64, 3, 0, None) == inval
    assert L.sputnik_block_activation(p, p, 64, 0, 2, None) == inval
    assert L.sputnik_block_activation(p, p, -1, 0, 0, None) == inval
    assert L.sputnik_block_activation(None, p, 64, 0, 0, None) == inval
    assert L.sputnik_block_activation(p, None, 64, 0, 0, None) == inval
    assert L.sputnik_block_activation(None, None, 0, 0, 0, None) == 0
    assert L.sputnik_block_activation_grad(None, p, p, 64, 0, 0, None) == inval
    assert L.sputnik_block_activation_grad(p, None, p, 64, 0, 0, None) == inval
    assert L.sputnik_block_activation_grad(p, p, p, 64, 9, 0, None) == inval
    assert L.sputnik_block_activation_grad(p, p, p, 0, 1, 1, None) == 0


# ---- the criterion, with float32 numpy standing in for the GPU ------------------------

_INPUTS = {}


def _inputs(dtype):
    if dtype not in _INPUTS:
        bits = R.all_finite_bits(dtype)
        _INPUTS[dtype] = (bits, R.bits_to_f64(bits, dtype))
    return _INPUTS[dtype]


def _stub(act, z64, dtype, grad, coeff=0.044715):
    """round_T of the float32 evaluation, as bits."""
    return R.round_bits(R.act32(act, z64.astype(np.float32), coeff=coeff,
                                grad=grad).astype(np.float64), dtype)


@pytest.mark.parametrize("grad", [False, True])
@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_float32_formulas_meet_the_criterion(dtype, act, grad):
    """Every finite input: a float32 evaluation is within one step (a few
    bf16 inputs whose true result is below 7e-37 excepted, and those within
    two), finite, and relu exact."""
    _, z = _inputs(dtype)
    ref = R.dact64(act, z) if grad else R.act64(act, z)
    got = _stub(act, z, dtype, grad)
    worst = R.check(got, ref, dtype, f"{act} {dtype} grad={grad}")
    if act == "relu":
        assert worst == 0
    _, bad1, _ = R.measure(got, ref, dtype, max_steps=1)
    if bad1:
        tiny = np.abs(ref) < 7e-37
        steps = R.steps_between(got, R.round_bits(ref, dtype))
        assert dtype == "bf16" and not (steps[~tiny] > 1).any()


@pytest.mark.parametrize("dtype,at_one_step", [("f16", 272), ("bf16", 66)])
def test_criterion_rejects_a_wrong_gelu_coefficient(dtype, at_one_step):
    """0.0447 in place of 0.044715: out of bounds at one step for 272 fp16
    and 66 bf16 inputs, and still rejected at the two steps allowed."""
    _, z = _inputs(dtype)
    ref = R.act64("gelu", z)
    got = _stub("gelu", z, dtype, False, coeff=0.0447)
    _, bad1, _ = R.measure(got, ref, dtype, max_steps=1)
    _, bad2, _ = R.measure(got, ref, dtype, max_steps=R.MAX_STEPS)
    print(f"{dtype}: {bad1} out of bounds at 1 step, {bad2} at 2")
    assert bad1 >= at_one_step // 2, bad1
    assert bad2 > 0, "the mutation passes at two steps"
