"""The router's auxiliary-loss statistics (include/sputnik/block/router.h)
used by a C++ caller: examples/cpp_router_aux.cpp routes 200 tokens to 2 of 5
experts from fp32 logits with RouterTopKAux into a workspace of 0xff bytes,
takes the gradient with RouterTopKAuxGrad, and checks on the host, in double
arithmetic, the ids exactly (and the ids and weights equal to RouterTopK's),
score_sums, z_sum and dlogits within the header's bounds. Built by
`make -C sputnik_amd` (build()); the CPU test checks that it resolves the new
C++ symbols from libsputnik.so, the GPU test runs it."""

import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "bin", "cpp_router_aux")

_TYPES = "NS0_10RouterTypeENS0_10WeightTypeE"
SYMBOLS = (
    "_ZN7sputnik5block13RouterTopKAuxEPKvPiPvS4_PfS5_iiib" + _TYPES
    + "S4_mP12ihipStream_t",
    "_ZN7sputnik5block17RouterTopKAuxGradEPKvPKiS2_S2_PKfS6_Pviiib" + _TYPES
    + "P12ihipStream_t",
    "_ZN7sputnik5block23RouterAuxWorkspaceBytesEii",
)


def test_router_aux_consumer_links_against_the_cpp_api():
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
def test_cpp_router_aux_runs():
    assert os.path.exists(BIN), "build it: make -C sputnik_amd"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
