"""CPU: the caller-owned workspace API is declared, exported and bound, and
the Python layer rejects a workspace that is not device memory before any
HIP call. (The GPU behaviour is in test_gpu_workspace.py.)"""

import ctypes
import os
import re

import pytest

import sputnik_amd as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_WS9 = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
        ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
        ctypes.c_void_p]
_Q5 = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
       ctypes.c_void_p]
# symbol -> (argtypes, restype), as include/sputnik_amd.h declares them
C_SYMBOLS = {
    "sputnik_sdd_ws": (_WS9, ctypes.c_int),
    "sputnik_dsd_ws": (_WS9, ctypes.c_int),
    "sputnik_dsd_ex_ws": (_WS9, ctypes.c_int),
    "sputnik_sdd_workspace_bytes": (_Q5, ctypes.c_size_t),
    "sputnik_dsd_workspace_bytes": (_Q5, ctypes.c_size_t),
    "sputnik_set_stream_workspace": ([ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_size_t], ctypes.c_int),
    "sputnik_retained_bytes": ([], ctypes.c_size_t),
    "sputnik_release_workspaces": ([], ctypes.c_size_t),
    "sputnik_incall_events": ([], ctypes.c_ulonglong),
    "sputnik_bt_launches": ([], ctypes.c_ulonglong),
}
PY_BINDINGS = ["set_stream_workspace", "sdd_workspace_bytes",
               "dsd_workspace_bytes", "retained_bytes", "release_workspaces",
               "incall_events", "bt_launches"]


def test_symbols_declared_exported_and_typed():
    header = open(os.path.join(ROOT, "include", "sputnik_amd.h")).read()
    L = sp.lib()
    for name, (args, res) in C_SYMBOLS.items():
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} not declared"
        fn = getattr(L, name)
        assert list(fn.argtypes) == args, name
        assert fn.restype is res, name


def test_python_bindings_exist():
    for name in PY_BINDINGS:
        assert callable(getattr(sp, name)), name
        assert name in sp.__all__, name


def test_counters_are_host_only_and_start_monotonic():
    a, b = sp.incall_events(), sp.bt_launches()
    assert a >= 0 and b >= 0
    assert sp.incall_events() >= a and sp.bt_launches() >= b


def test_cpu_workspace_raises_before_any_hip_call(monkeypatch):
    torch = pytest.importorskip("torch")
    # Any entry into the library from here on is a failure: the check has to
    # happen in Python, before the C-ABI (and so before any HIP call).
    def boom():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(sp, "lib", boom)
    A = sp.Matrix(128, 128, torch.zeros(128, 128, dtype=torch.float16))
    Bm = sp.Matrix(128, 128, torch.zeros(128, 128, dtype=torch.float16))
    C = sp.BlockMatrix(128, 128, 128, 128 * 128,
                       torch.zeros(1, 128, 128, dtype=torch.float16),
                       torch.tensor([0, 1], dtype=torch.int32),
                       torch.tensor([0], dtype=torch.int16))
    ws = torch.empty(1 << 16, dtype=torch.uint8)
    with pytest.raises(ValueError, match="device memory"):
        sp.Matmul(A, False, Bm, True, C, stream=0, workspace=ws)
    S = sp.BlockMatrix(128, 128, 128, 128 * 128, C.data, C.offsets, C.indices)
    D = sp.Matrix(128, 128, torch.zeros(128, 128, dtype=torch.float16))
    with pytest.raises(ValueError, match="device memory"):
        sp.MatmulEx(S, False, Bm, True, D, stream=0, workspace=ws)
    with pytest.raises(TypeError):
        sp.Matmul(A, False, Bm, True, C, stream=0, workspace=b"bytes")
