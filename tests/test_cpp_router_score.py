"""The sigmoid-score router (include/sputnik/block/router.h) used by a C++
caller: examples/cpp_router_score.cpp routes 300 tokens to 3 of 16 experts in
the 2 best of 4 groups from fp32 logits and a selection bias (some rows tied
on purpose), and checks on the host, in double arithmetic, the ids exactly
and the weights and scores within the bound it states. Built by
`make -C sputnik_amd` (build()); the CPU test checks that it resolves the new
C++ symbol from libsputnik.so, the GPU test runs it."""

import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "bin", "cpp_router_score")

_TAIL = "NS0_10RouterTypeENS0_10WeightTypeEP12ihipStream_t"
SYMBOLS = (
    "_ZN7sputnik5block15RouterScoreTopKEPKvPKfPiPvS6_iiiiibf" + _TAIL,
    "_ZN7sputnik5block19RouterScoreTopKGradEPKvPKiS2_S2_Pviiibf" + _TAIL,
)
# what the example itself calls
USED = (SYMBOLS[0],)


def test_router_score_consumer_links_against_the_cpp_api():
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
def test_cpp_router_score_runs():
    assert os.path.exists(BIN), "build it: make -C sputnik_amd"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL OK" in r.stdout
