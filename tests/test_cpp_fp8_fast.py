"""The C++ side of the fp8 products' fast accumulation
(include/sputnik/block/fp8.h, Fp8Accumulate) used by a C++ caller:
examples/cpp_fp8_fast.cpp runs Fp8IntervalSums in both modes and the SddFp8 /
DsdFp8 overloads that take the mode, in kFast, on known-answer data with
power-of-two scales and checks every element on the host. Built by `make -C
sputnik_amd` (build()); the CPU test checks that it resolves the new C++
symbols from libsputnik.so and that the overloads from before keep their
names, the GPU test runs it."""

import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "bin", "cpp_fp8_fast")

_MODE = "NS0_13Fp8AccumulateE"
_STREAM = "P12ihipStream_t"
_SDD = "_ZN7sputnik5block6SddFp8EPKvPKfiS2_S4_NS0_11BlockMatrixENS0_8DataTypeE"
_DSD = ("_ZN7sputnik5block6DsdFp8ENS0_11BlockMatrixEPKfPKvS3_NS0_6MatrixE"
        "NS0_8DataTypeE")
SYMBOLS = (
    "_ZN7sputnik5block15Fp8IntervalSumsEPKvS2_iii" + _MODE + "Pf" + _STREAM,
    _SDD + _MODE + _STREAM,
    _DSD + _MODE + _STREAM,
)
KEPT = (_SDD + _STREAM, _DSD + _STREAM)


def test_fp8_fast_consumer_links_against_the_cpp_api():
    assert os.path.exists(BIN), "build it: make -C sputnik_amd"
    out = subprocess.run(["ldd", BIN], capture_output=True, text=True,
                         check=True).stdout
    line = [l for l in out.splitlines() if "libsputnik.so" in l]
    assert line and "not found" not in line[0], out
    syms = subprocess.run(["nm", "-D", "--undefined-only", BIN],
                          capture_output=True, text=True, check=True).stdout
    for s in SYMBOLS:
        assert s in syms, s
    import sputnik_amd as sp
    defined = subprocess.run(["nm", "-D", "--defined-only", sp.LIB_PATH],
                             capture_output=True, text=True, check=True).stdout
    names = {l.split()[-1] for l in defined.splitlines() if l.strip()}
    for s in SYMBOLS + KEPT:
        assert s in names, s


@pytest.mark.gpu
def test_cpp_fp8_fast_runs():
    assert os.path.exists(BIN), "build it: make -C sputnik_amd"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
