"""The C++ side of the gated SDD products (include/sputnik/block/gated.h) used
by a C++ caller: examples/cpp_gated.cpp runs a GLU expert MLP's calls,
H = (X V1) * relu(X W1) with U = X V1 kept, then dU (over U) and dG from
dY W2^T, and checks every element on the host. Built by `make -C
sputnik_amd` (build()); the CPU test checks that it resolves the new C++
symbols from libsputnik.so, the GPU test runs it."""

import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "bin", "cpp_gated")

_HEAD = "NS0_6MatrixEbS1_bNS0_11BlockMatrixENS0_10ActivationE"
_TAIL = "NS0_8DataTypeEP12ihipStream_t"
SYMBOLS = (
    "_ZN7sputnik5block11MatmulGatedE" + _HEAD + "PKvPv" + _TAIL,
    "_ZN7sputnik5block15MatmulGatedGradE" + _HEAD + "PKvS5_Pv" + _TAIL,
)


def test_gated_consumer_links_against_the_cpp_api():
    assert os.path.exists(BIN), "build it: make -C sputnik_amd"
    out = subprocess.run(["ldd", BIN], capture_output=True, text=True,
                         check=True).stdout
    line = [l for l in out.splitlines() if "libsputnik.so" in l]
    assert line and "not found" not in line[0], out
    syms = subprocess.run(["nm", "-D", "--undefined-only", BIN],
                          capture_output=True, text=True, check=True).stdout
    for s in SYMBOLS:
        assert s in syms, s


@pytest.mark.gpu
def test_cpp_gated_runs():
    assert os.path.exists(BIN), "build it: make -C sputnik_amd"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
