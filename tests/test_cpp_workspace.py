"""The C++ side of the caller-owned workspace API (include/sputnik/block/
workspace.h) used by a C++ caller: examples/cpp_workspace.cpp registers its
own transposed-B workspace for a stream and drives the reference's fixed
Matmul signature. Built by `make -C sputnik_amd` (build()); the CPU test
checks that it resolves the new C++ symbols from libsputnik.so, the GPU test
runs it."""

import os
import subprocess

import pytest

import sputnik_amd as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "bin", "cpp_workspace")

SYMBOLS = (
    "_ZN7sputnik5block18SetStreamWorkspaceEP12ihipStream_tPvm",
    "_ZN7sputnik5block17SddWorkspaceBytesENS0_6MatrixEbS1_bNS0_11BlockMatrixE",
    "_ZN7sputnik5block13RetainedBytesEv",
    "_ZN7sputnik5block17ReleaseWorkspacesEv",
)


def test_workspace_consumer_links_against_the_cpp_api():
    assert os.path.exists(BIN), "build it: make -C sputnik_amd"
    out = subprocess.run(["ldd", BIN], capture_output=True, text=True,
                         check=True).stdout
    line = [l for l in out.splitlines() if "libsputnik.so" in l]
    assert line and "not found" not in line[0], out
    syms = subprocess.run(["nm", "-D", "--undefined-only", BIN],
                          capture_output=True, text=True, check=True).stdout
    for s in SYMBOLS:
        assert s in syms, s


def test_workspace_cpp_symbols_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", sp.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    for s in SYMBOLS + (
            "_ZN7sputnik5block17DsdWorkspaceBytesENS0_11BlockMatrixEbNS0_6MatrixEbS2_",):
        assert s in out, s


@pytest.mark.gpu
def test_cpp_workspace_runs():
    assert os.path.exists(BIN), "build it: make -C sputnik_amd"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
