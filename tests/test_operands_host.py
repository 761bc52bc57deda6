"""The operand binding pinned on the host: tests/operands_host.cpp (built by
`make -C sputnik_amd` as build/bin/operands_host, host code only) runs
sputnik_amd/csrc/operands.cpp over a fixed case list and prints, per case,
the Status, the metadata flags and every non-zero GemmParams field. The
output must equal tests/golden/operands.txt line by line. That file was
recorded from the six hand-written Prepare* functions the binding replaced,
so it is their behaviour: a difference is a behaviour change, never a reason
to regenerate it."""

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "bin", "operands_host")
GOLDEN = os.path.join(ROOT, "tests", "golden", "operands.txt")


def _case(line):
    return line.split(":", 1)[0]


def test_operand_binding_matches_the_recorded_cases():
    assert os.path.exists(BIN), "build it: make -C sputnik_amd"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = r.stdout.splitlines()
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    for g, w in zip(got, want):
        assert g == w, "case %r:\n  got  %s\n  want %s" % (_case(w), g, w)
    longer = got if len(got) > len(want) else want
    assert len(got) == len(want), "%d cases printed, %d recorded; first unmatched: %r" % (
        len(got), len(want), _case(longer[min(len(got), len(want))]))
    names = [_case(l) for l in want]
    assert len(set(names)) == len(names), "case names are unique"
