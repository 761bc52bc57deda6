"""The C++ side of the MoE router (include/sputnik/block/router.h) used by a
C++ caller: examples/cpp_router.cpp routes 200 tokens to 2 of 5 experts from
fp32 logits (some rows tied on purpose), sorts the picks with MoeSort, and
checks on the host the ids and every routing tensor exactly and the weights
and scores within the header's bound. Built by `make -C sputnik_amd`
(build()); the CPU test checks that it resolves the new C++ symbols from
libsputnik.so, the GPU test runs it."""

import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "bin", "cpp_router")

_TAIL = "iiibNS0_10RouterTypeENS0_10WeightTypeEP12ihipStream_t"
SYMBOLS = (
    "_ZN7sputnik5block10RouterTopKEPKvPiPvS4_" + _TAIL,
    "_ZN7sputnik5block14RouterTopKGradEPKvPKiS2_S2_Pv" + _TAIL,
    "_ZN7sputnik5block21MoeSortWorkspaceBytesEii",
    "_ZN7sputnik5block7MoeSortEPKiiiiPiS3_S3_S3_S3_S3_PvmP12ihipStream_t",
)
# what the example itself calls
USED = (SYMBOLS[0], SYMBOLS[2], SYMBOLS[3])


def test_router_consumer_links_against_the_cpp_api():
    assert os.path.exists(BIN), "build it: make -C sputnik_amd"
    out = subprocess.run(["ldd", BIN], capture_output=True, text=True,
                         check=True).stdout
    line = [l for l in out.splitlines() if "libsputnik.so" in l]
    assert line and "not found" not in line[0], out
    syms = subprocess.run(["nm", "-D", "--undefined-only", BIN],
                          capture_output=True, text=True, check=True).stdout
    for s in USED:
        assert s in syms, s


@pytest.mark.gpu
def test_cpp_router_runs():
    assert os.path.exists(BIN), "build it: make -C sputnik_amd"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
