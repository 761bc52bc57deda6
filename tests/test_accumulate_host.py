"""CPU: the host side of the accumulating DSD / DDS products
(sputnik/block/accumulate.h): the Python entry points and the ops keywords
exist, the C type is checked before the library is called, the C and C++
symbols are exported, and the C-ABI acceptance rules hold without aborting.
No compute call is made (no GPU here)."""

import ctypes
import inspect
import subprocess

import pytest

import sputnik_amd as sp

torch = pytest.importorskip("torch")


class _T:
    """Stand-in for a device tensor (tests/test_abi.py): only data_ptr() is
    read by the host checks; nothing is dereferenced."""

    def __init__(self, addr=0x1000):
        self.addr = addr

    def data_ptr(self):
        return self.addr


def _sparse(rows, cols, dtype, block=128):
    data = torch.zeros(1, 8, 8, dtype=dtype)  # (only its dtype is read)
    return sp.BlockMatrix(rows, cols, block, block * block, data, _T(), _T(),
                          offsets_t=_T(), indices_t=_T(), block_offsets=_T())


def _dense(rows, cols, dtype):
    return sp.Matrix(rows, cols, torch.zeros(1, dtype=dtype))


@pytest.fixture
def no_library(monkeypatch):
    """Any use of the library fails the test."""
    def boom():
        raise AssertionError("the library was called")
    monkeypatch.setattr(sp, "lib", boom)


def test_python_entry_points_exist():
    from sputnik_amd import ops
    for fn in (sp.MatmulAccumulate, sp.MatmulAccumulateEx):
        assert list(inspect.signature(fn).parameters) == [
            "a", "transpose_a", "b", "transpose_b", "c", "stream"]
    assert "MatmulAccumulate" in sp.__all__
    assert "MatmulAccumulateEx" in sp.__all__
    assert sp.SPUTNIK_OUT_OPERAND == 0 and sp.SPUTNIK_OUT_F32 == 1
    assert list(inspect.signature(ops.dsd_acc).parameters) == [
        "a", "b", "out"]
    assert list(inspect.signature(ops.dds_acc).parameters) == [
        "a", "b", "out"]
    assert list(inspect.signature(ops.sdd).parameters) == [
        "a", "b", "topo", "a_grad_out", "b_grad_out"]
    assert list(inspect.signature(ops.dsd).parameters) == [
        "a", "b", "b_grad_out"]
    assert list(inspect.signature(ops.dds).parameters) == [
        "a", "b", "a_grad_out"]
    for name in ("a_grad_out", "b_grad_out"):
        assert inspect.signature(ops.sdd).parameters[name].default is None


@pytest.mark.parametrize("fn", ["MatmulAccumulate", "MatmulAccumulateEx"])
@pytest.mark.parametrize("operand,c_dtype", [
    (torch.float16, torch.bfloat16), (torch.bfloat16, torch.float16),
    (torch.float16, torch.float64), (torch.bfloat16, torch.int32)])
def test_wrong_c_dtype_raises_before_the_library(fn, operand, c_dtype,
                                                 no_library):
    f = getattr(sp, fn)
    with pytest.raises(TypeError):   # DSD
        f(_sparse(256, 256, operand), False, _dense(256, 64, operand), False,
          _dense(256, 64, c_dtype))
    with pytest.raises(TypeError):   # DDS
        f(_dense(64, 256, operand), False, _sparse(256, 256, operand), False,
          _dense(64, 256, c_dtype))


def test_sparse_c_raises(no_library):
    s = _sparse(256, 256, torch.float16)
    d = _dense(256, 256, torch.float16)
    for a, b in ((d, d), (s, d), (d, s)):  # SDD, SSD, SDS shapes
        with pytest.raises(TypeError):
            sp.MatmulAccumulate(a, False, b, False, s)
        with pytest.raises(TypeError):
            sp.MatmulAccumulateEx(a, False, b, False, s)


def _exported():
    return subprocess.run(["nm", "-D", "--defined-only", sp.LIB_PATH],
                          capture_output=True, text=True, check=True).stdout


def test_c_symbols_exported():
    out = _exported().split()
    for s in ("sputnik_dsd_acc", "sputnik_dsd_ex_acc", "sputnik_dds_acc",
              "sputnik_dds_ex_acc"):
        assert s in out, s
        assert hasattr(sp.lib(), s)


def test_cpp_symbols_exported():
    """The four overloads of sputnik/block/accumulate.h."""
    out = _exported()
    tail = "NS0_8DataTypeENS0_10OutputTypeEP12ihipStream_t"
    for name in ("16MatmulAccumulate", "18MatmulAccumulateEx"):
        for args in ("NS0_11BlockMatrixEbNS0_6MatrixEbS2_",    # DSD
                     "NS0_6MatrixEbNS0_11BlockMatrixEbS1_"):   # DDS
            sym = "_ZN7sputnik5block" + name + "E" + args + tail
            assert sym in out, sym


def _c_sparse(rows, cols, block):
    return sp.BlockMatrix(rows, cols, block, block * block, _T(), _T(), _T(),
                          offsets_t=_T(), indices_t=_T(),
                          block_offsets=_T())._c()


@pytest.mark.parametrize("ex", [False, True])
def test_c_abi_acceptance_never_aborts(ex):
    L = sp.lib()
    dsd = L.sputnik_dsd_ex_acc if ex else L.sputnik_dsd_acc
    dds = L.sputnik_dds_ex_acc if ex else L.sputnik_dds_acc
    s64, s128 = _c_sparse(256, 256, 64), _c_sparse(256, 256, 128)
    d = sp.Matrix(256, 256, _T())._c()
    ref = ctypes.byref
    for c_type in (sp.SPUTNIK_OUT_OPERAND, sp.SPUTNIK_OUT_F32):
        assert dsd(ref(s64), 0, ref(d), 0, ref(d), 0, c_type,
                   None) == sp.hipErrorNotSupported
        assert dds(ref(d), 0, ref(s64), 0, ref(d), 0, c_type,
                   None) == sp.hipErrorNotSupported
    for c_type in (2, -1):
        assert dsd(ref(s128), 0, ref(d), 0, ref(d), 0, c_type,
                   None) == sp.hipErrorInvalidValue
        assert dds(ref(d), 0, ref(s128), 0, ref(d), 0, c_type,
                   None) == sp.hipErrorInvalidValue
    # a shape the plain call rejects is rejected the same way
    bad = sp.Matrix(256, 264, _T())._c()
    assert dsd(ref(s128), 0, ref(d), 0, ref(bad), 0, 0,
               None) == sp.hipErrorInvalidValue
    assert dsd(None, 0, ref(d), 0, ref(d), 0, 0,
               None) == sp.hipErrorInvalidValue
