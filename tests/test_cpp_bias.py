"""The C++ side of the bias products (include/sputnik/block/bias.h and the
PaddedScatterBias call of moe.h) used by a C++ caller: examples/cpp_bias.cpp
runs C = X W1 + b, H = relu(X W1 + b) with Z kept, the column sums of Z and a
scatter with an output bias, and checks every element on the host. Built by
`make -C sputnik_amd` (build()); the CPU test checks that it resolves the new
C++ symbols from libsputnik.so, the GPU test runs it."""

import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "bin", "cpp_bias")

_HEAD = "NS0_6MatrixEbS1_bNS0_11BlockMatrixEPKv"
_TAIL = "NS0_8DataTypeEP12ihipStream_t"
SYMBOLS = (
    "_ZN7sputnik5block10MatmulBiasE" + _HEAD + _TAIL,
    "_ZN7sputnik5block20MatmulBiasActivationE" + _HEAD
    + "NS0_10ActivationEPv" + _TAIL,
    "_ZN7sputnik5block14BlockColumnSumENS0_11BlockMatrixENS0_8DataTypeEPf"
    "P12ihipStream_t",
    "_ZN7sputnik5block17PaddedScatterBiasEPKvPKiS4_S2_S2_PviiiiiNS0_8DataTypeE"
    "NS0_10WeightTypeEP12ihipStream_t",
)


def test_bias_consumer_links_against_the_cpp_api():
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
def test_cpp_bias_runs():
    assert os.path.exists(BIN), "build it: make -C sputnik_amd"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
