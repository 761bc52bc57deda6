"""The dispatcher's routes against the recorded table, and launches against
the queries.

tests/route_table.json is what tests/route_table.py printed on an MI355X
before the per-product route functions (dispatch.cpp RouteDsd / RouteDds /
RouteSdd) replaced the hand-copied selection chains: every plan, kernel,
epilogue-route and workspace-size query for a fixed list of problems and
knob settings. The library must reproduce every row, the queries must leave
every workspace and counter alone, and the table must still name every code
of every query. Where the library lets a test see what a launch did
(sputnik_bt_launches), the launch must agree with the query.
"""

import json
import os

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected here, skipped: no device
    pytest.skip("no GPU", allow_module_level=True)

import sputnik_amd as sp  # noqa: E402
from tests import route_table  # noqa: E402
from tests.test_gpu_kat import _equal, kat_dsd  # noqa: E402
from tests.test_gpu_workspace import SddProblem, _ws, shared_problem  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "route_table.json")) as _f:
    RECORDED = json.load(_f)


@pytest.fixture
def bt_small():
    """The transposed-B path from a 1-MiB B on (default: 256 MiB)."""
    prev = sp.tuning("sdd_bt_min_mib", 1)
    yield
    sp.tuning("sdd_bt_min_mib", prev)


def test_route_table_reproduced_and_read_only():
    cus = route_table.cus()
    assert cus == RECORDED["cus"], (
        f"tests/route_table.json was recorded on {RECORDED['cus']} CUs, this "
        f"device has {cus}: record it again there (tests/route_table.py)")
    assert RECORDED["counters_unchanged"]
    before = route_table.counters()
    rows = route_table.rows()
    after = route_table.counters()
    want = RECORDED["rows"]
    assert [r["id"] for r in rows] == [r["id"] for r in want], "the row list moved"
    bad = [(g["id"], g["result"], w["result"]) for g, w in zip(rows, want)
           if g["result"] != w["result"]]
    assert not bad, (f"{len(bad)} of {len(want)} rows differ (id, got, recorded); "
                     f"first: {bad[:5]}")
    assert after == before, "a query allocated, launched or tied something"


def test_route_table_names_every_code():
    seen = {}
    for r in RECORDED["rows"]:
        for k, v in r["result"].items():
            seen.setdefault((r["family"], k), set()).add(v)
    assert seen["dsd", "plan"] == {-1, 0, 1, 2, 3, 4}
    assert seen["dds", "plan"] == {-1, 0, 1, 2, 3}
    assert seen["sdd", "plan"] == {-1, 0, 1, 2}
    assert seen["sdd", "kernel"] == {-1, 0, 1, 2, 3, 4}
    assert seen["sdd", "act_route"] == {-1, 1, 2}
    assert 0 in seen["dsd", "workspace_bytes"] and len(seen["dsd", "workspace_bytes"]) > 1
    assert 0 in seen["sdd", "workspace_bytes"] and len(seen["sdd", "workspace_bytes"]) > 1


# ------------------------------------------ launches against the queries --

def _sdd_problem(ta):
    return shared_problem(4096) if not ta else SddProblem(8192, 256, 4096, True, "f16", 47)


@pytest.mark.parametrize("ta", [False, True])
@pytest.mark.parametrize("min_mib", [1, 0])
def test_sdd_launch_transposes_iff_kernel_is_4(ta, min_mib):
    """Eager default stream, library route: one Matmul enqueues exactly one
    transpose of B iff sdd_kernel says 4."""
    p = _sdd_problem(ta)
    prev = sp.tuning("sdd_bt_min_mib", min_mib)
    try:
        kernel = sp.sdd_kernel(p.A.m, ta, p.Bd.m, True, p.Cs.m)
        assert kernel == (4 if min_mib else 3)
        assert (p.workspace_bytes() != 0) == (kernel == 4)
        p.clear()
        launches = sp.bt_launches()
        p.run()
        assert sp.bt_launches() - launches == (1 if kernel == 4 else 0)
        p.check(f"sdd {'T' if ta else 'N'}T kernel {kernel}")
    finally:
        sp.tuning("sdd_bt_min_mib", prev)


@pytest.mark.parametrize("ta", [False, True])
def test_sdd_launch_with_workspace(ta, bt_small):
    """A fitting workspace=: one transpose, and the library allocates,
    synchronises and keeps nothing."""
    p = _sdd_problem(ta)
    ws = _ws(p.workspace_bytes())
    p.clear()
    torch.cuda.synchronize()
    launches, events, held = sp.bt_launches(), sp.incall_events(), sp.retained_bytes()
    p.run(workspace=ws)
    assert sp.bt_launches() == launches + 1
    assert sp.incall_events() == events
    assert sp.retained_bytes() == held
    p.check(f"sdd {'T' if ta else 'N'}T workspace")


_dsd = {}


def _dsd_problem():
    """test_kat_dsd_nt_bt_transpose's problem, built (and run) once with the
    path off."""
    if not _dsd:
        prev = sp.tuning("sdd_bt_min_mib", 0)
        try:
            got, want, (A, Bd, C) = kat_dsd(16384, 256, 2048, 1.0, False, True, "f16",
                                            seed=53)
        finally:
            sp.tuning("sdd_bt_min_mib", prev)
        _equal(got, want, "dsd nt, path off")
        _dsd.update(got=got, want=want, A=A, Bd=Bd, C=C)
    return _dsd


@pytest.mark.parametrize("min_mib", [1, 0])
def test_dsd_launch_transposes_iff_workspace_bytes(min_mib):
    """Eager default stream (the library route is open): one Matmul enqueues
    exactly one transpose of B iff dsd_workspace_bytes is non-zero."""
    d = _dsd_problem()
    prev = sp.tuning("sdd_bt_min_mib", min_mib)
    try:
        nbytes = sp.dsd_workspace_bytes(d["A"].m, False, d["Bd"].m, True, d["C"])
        assert nbytes == (2048 * 256 * 2 if min_mib else 0)
        assert sp.dsd_plan(d["A"].m, False, d["Bd"].m, True, d["C"]) == 1
        d["got"].fill_(float("nan"))
        launches = sp.bt_launches()
        sp.Matmul(d["A"].m, False, d["Bd"].m, True, d["C"])
        assert sp.bt_launches() - launches == (1 if nbytes else 0)
        _equal(d["got"], d["want"], f"dsd nt, sdd_bt_min_mib {min_mib}")
    finally:
        sp.tuning("sdd_bt_min_mib", prev)


def test_dsd_launch_with_workspace(bt_small):
    d = _dsd_problem()
    ws = _ws(sp.dsd_workspace_bytes(d["A"].m, False, d["Bd"].m, True, d["C"]))
    d["got"].fill_(float("nan"))
    torch.cuda.synchronize()
    launches, events, held = sp.bt_launches(), sp.incall_events(), sp.retained_bytes()
    sp.Matmul(d["A"].m, False, d["Bd"].m, True, d["C"], workspace=ws)
    assert sp.bt_launches() == launches + 1
    assert sp.incall_events() == events
    assert sp.retained_bytes() == held
    _equal(d["got"], d["want"], "dsd nt workspace")
