"""The C++ side of the accumulating products (include/sputnik/block/
accumulate.h) used by a C++ caller: examples/cpp_accumulate.cpp runs one DSD
and one DDS accumulation into an fp32 C and checks every element on the
host. Built by `make -C sputnik_amd` (build()); the CPU test checks that it
resolves the new C++ symbols from libsputnik.so, the GPU test runs it."""

import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "bin", "cpp_accumulate")

_TAIL = "NS0_8DataTypeENS0_10OutputTypeEP12ihipStream_t"
SYMBOLS = (
    "_ZN7sputnik5block16MatmulAccumulateENS0_11BlockMatrixEbNS0_6MatrixEbS2_"
    + _TAIL,
    "_ZN7sputnik5block16MatmulAccumulateENS0_6MatrixEbNS0_11BlockMatrixEbS1_"
    + _TAIL,
)


def test_accumulate_consumer_links_against_the_cpp_api():
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
def test_cpp_accumulate_runs():
    assert os.path.exists(BIN), "build it: make -C sputnik_amd"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
