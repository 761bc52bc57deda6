"""The C++ side of the fp8 products (include/sputnik/block/fp8.h) used by a
C++ caller: examples/cpp_fp8.cpp runs QuantizeRows / QuantizeWeight -> SddFp8
-> QuantizeRowsActivation (relu) -> DsdFp8 on known-answer data with
power-of-two scales and checks every byte, scale and output element on the
host. Built by `make -C sputnik_amd` (build()); the CPU test checks that it
resolves the new C++ symbols from libsputnik.so, the GPU test runs it."""

import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "bin", "cpp_fp8")

_TAIL = "NS0_8DataTypeEP12ihipStream_t"
SYMBOLS = (
    "_ZN7sputnik5block12QuantizeRowsEPKviiPvPfb" + _TAIL,
    "_ZN7sputnik5block22QuantizeRowsActivationEPKviiNS0_10ActivationEPvPfb"
    + _TAIL,
    "_ZN7sputnik5block14QuantizeWeightEPKviibPvPfb" + _TAIL,
    "_ZN7sputnik5block6SddFp8EPKvPKfiS2_S4_NS0_11BlockMatrixE" + _TAIL,
    "_ZN7sputnik5block6DsdFp8ENS0_11BlockMatrixEPKfPKvS3_NS0_6MatrixE" + _TAIL,
)


def test_fp8_consumer_links_against_the_cpp_api():
    assert os.path.exists(BIN), "build it: make -C sputnik_amd"
    out = subprocess.run(["ldd", BIN], capture_output=True, text=True,
                         check=True).stdout
    line = [l for l in out.splitlines() if "libsputnik.so" in l]
    assert line and "not found" not in line[0], out
    syms = subprocess.run(["nm", "-D", "--undefined-only", BIN],
                          capture_output=True, text=True, check=True).stdout
    for s in SYMBOLS:
        assert s in syms, s
    # ... and the library defines them, with the gated quantiser
    import sputnik_amd as sp
    defined = subprocess.run(["nm", "-D", "--defined-only", sp.LIB_PATH],
                             capture_output=True, text=True, check=True).stdout
    for s in SYMBOLS + ("_ZN7sputnik5block17QuantizeRowsGatedEPKvS2_iiNS0_"
                        "10ActivationEPvPfb" + _TAIL,):
        assert s in defined, s


@pytest.mark.gpu
def test_cpp_fp8_runs():
    assert os.path.exists(BIN), "build it: make -C sputnik_amd"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
