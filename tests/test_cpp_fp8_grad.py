"""The C++ side of the fp8 gradient pieces (include/sputnik/block/fp8.h,
"Gradients") used by a C++ caller: examples/cpp_fp8_grad.cpp runs Transpose ->
QuantizeBlocks / QuantizeTiles -> DsdFp8Wgrad (plain and with `add`) and
TransposeWeightFp8 on known-answer data with power-of-two scales and checks
every byte, scale and output element on the host. Built by `make -C
sputnik_amd` (build()); the CPU test checks that it resolves the new C++
symbols from libsputnik.so, the GPU test runs it."""

import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "bin", "cpp_fp8_grad")

SYMBOLS = ("QuantizeTiles", "QuantizeBlocks", "TransposeWeightFp8",
           "DsdFp8Wgrad")


def _mangled(listing: str, name: str) -> bool:
    return f"_ZN7sputnik5block{len(name)}{name}E" in listing


def test_fp8_grad_consumer_links_against_the_cpp_api():
    assert os.path.exists(BIN), "build it: make -C sputnik_amd"
    out = subprocess.run(["ldd", BIN], capture_output=True, text=True,
                         check=True).stdout
    line = [l for l in out.splitlines() if "libsputnik.so" in l]
    assert line and "not found" not in line[0], out
    syms = subprocess.run(["nm", "-D", "--undefined-only", BIN],
                          capture_output=True, text=True, check=True).stdout
    import sputnik_amd as sp
    defined = subprocess.run(["nm", "-D", "--defined-only", sp.LIB_PATH],
                             capture_output=True, text=True, check=True).stdout
    for s in SYMBOLS:
        assert _mangled(syms, s), s
        assert _mangled(defined, s), s


@pytest.mark.gpu
def test_cpp_fp8_grad_runs():
    assert os.path.exists(BIN), "build it: make -C sputnik_amd"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
