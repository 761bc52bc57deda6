"""The C++ side of the MoE token permutation (include/sputnik/block/moe.h)
used by a C++ caller: examples/cpp_moe.cpp routes 200 tokens to 2 of 4
experts (one of them empty), gathers them into the padded matrix, scatters
them back with fp32 weights and takes the weight gradient, and checks every
element on the host bit for bit. Built by `make -C sputnik_amd` (build());
the CPU test checks that it resolves the new C++ symbols from libsputnik.so,
the GPU test runs it."""

import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "bin", "cpp_moe")

_TAIL = "NS0_8DataTypeENS0_10WeightTypeEP12ihipStream_t"
SYMBOLS = (
    "_ZN7sputnik5block7MoeBinsEPKiiiPiS3_S3_P12ihipStream_t",
    "_ZN7sputnik5block9MoeRowMapEPKiS2_S2_S2_iiiPiP12ihipStream_t",
    "_ZN7sputnik5block12PaddedGatherEPKvPKiS4_S4_S2_Pviiiii" + _TAIL,
    "_ZN7sputnik5block13PaddedScatterEPKvPKiS2_Pviiii" + _TAIL,
    "_ZN7sputnik5block23PaddedScatterWeightGradEPKvS2_PKiPviiii" + _TAIL,
)


def test_moe_consumer_links_against_the_cpp_api():
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
def test_cpp_moe_runs():
    assert os.path.exists(BIN), "build it: make -C sputnik_amd"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
