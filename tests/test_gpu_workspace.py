"""Caller-owned workspaces for the transposed-B path (include/sputnik_amd.h,
"Caller-owned workspaces"): with memory supplied per call or per stream, SDD
NT / TT and DSD NT run the transpose + N-major product without the library
allocating, freeing or synchronising anything (its own counter,
sputnik_incall_events, does not move), also under graph capture and from two
threads; memory that does not fit keeps the NT kernel; what the library
still holds can be seen and returned.

All data is the integer-valued KAT data of test_gpu_kat (values -1 / 0 / 1,
K <= 512 for fp16 and 256 for bf16), so every comparison is exact. Shapes
are the existing bt KATs': the smallest at which the path's gates and the
grouped 4-wave plan hold with sdd_bt_min_mib at 1.
"""

import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected here, skipped: no device
    pytest.skip("no GPU", allow_module_level=True)

import sputnik_amd as sp  # noqa: E402
from sputnik_amd import ops  # noqa: E402
from tests.test_gpu_kat import (IDense, ISparse, _equal, _expect,  # noqa: E402
                                _op, kat_dsd, kat_sdd)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def bt_small():
    """The transposed-B path from a 1-MiB B on (default: 256 MiB)."""
    prev = sp.tuning("sdd_bt_min_mib", 1)
    yield
    sp.tuning("sdd_bt_min_mib", prev)


class SddProblem:
    """SDD with B^T stored [N][K], its exact answer, a NaN-filled output."""

    def __init__(self, m, k, n, ta, dtype, seed):
        rng = np.random.default_rng(seed)
        self.ta, self.dtype, self.k, self.n = ta, dtype, k, n
        self.A = IDense(*((k, m) if ta else (m, k)), rng, dtype)
        self.Bd = IDense(n, k, rng, dtype)
        self.Cs = ISparse(m, n, 0.6, rng, dtype)
        sp.AllocateRowIndicesBuffer(self.Cs.m)
        sp.RowIndices(self.Cs.m, self.Cs.m.row_indices)
        full = _op(self.A.values, ta).astype(np.float64) @ self.Bd.values.T
        self.want = _expect(self.Cs.blocks_of(full), dtype)
        self.Cs.dense = None  # (host copy no longer needed)
        self.bt_bytes = n * k * 2

    def workspace_bytes(self):
        return sp.sdd_workspace_bytes(self.A.m, self.ta, self.Bd.m, True, self.Cs.m)

    def run(self, **kw):
        sp.Matmul(self.A.m, self.ta, self.Bd.m, True, self.Cs.m, **kw)

    def clear(self):
        self.Cs.dev.fill_(float("nan"))

    def check(self, what):
        _equal(self.Cs.dev, self.want, what)


_shared = {}


def shared_problem(n):
    """The NT fp16 K = 256 problems of test_sdd_bt_two_threads_one_stream,
    built once and shared (each test NaN-fills the output before it runs)."""
    if n not in _shared:
        _shared[n] = SddProblem(8192, 256, n, False, "f16", {4096: 31, 6144: 32}[n])
    return _shared[n]


def _ws(nbytes):
    return torch.empty(nbytes, dtype=torch.uint8, device="cuda")


# ---------------------------------------------------- 1. per-call route --

@pytest.mark.parametrize("ta", [False, True])
@pytest.mark.parametrize("dtype,k", [("f16", 512), ("bf16", 256)])
def test_sdd_per_call_workspace_exact_no_incall_events(ta, dtype, k, bt_small):
    """SDD NT / TT with a workspace of exactly sdd_workspace_bytes: exact,
    one transpose launch per call, and nothing allocated, freed or
    synchronised across N = 4096, 4096, 6144 (the third call is the growth
    case that synchronises on the library route)."""
    probs = {n: SddProblem(8192, k, n, ta, dtype, n + 10 * ta) for n in (4096, 6144)}
    torch.cuda.synchronize()
    events = sp.incall_events()
    for i, n in enumerate((4096, 4096, 6144)):
        p = probs[n]
        nbytes = p.workspace_bytes()
        assert nbytes == p.bt_bytes and nbytes % 256 == 0
        ws = _ws(nbytes)  # a fresh one per call, larger for the third
        p.clear()
        launches = sp.bt_launches()
        p.run(workspace=ws)
        assert sp.bt_launches() == launches + 1
        p.check(f"sdd ws {'T' if ta else 'N'}T {dtype} call {i} n={n}")
    assert sp.incall_events() == events


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("ex", [False, True])
def test_dsd_nt_per_call_workspace_exact_no_incall_events(dtype, ex, bt_small):
    """DSD NT over a dense A through Matmul and MatmulEx with a workspace of
    exactly dsd_workspace_bytes (the problem is kat_dsd's, which also runs it
    once on the library route)."""
    got, want, (A, Bd, C) = kat_dsd(16384, 256, 2048, 1.0, False, True, dtype,
                                    ex=ex, seed=71 + ex)
    _equal(got, want, "library route")
    nbytes = sp.dsd_workspace_bytes(A.m, False, Bd.m, True, C)
    assert nbytes == 2048 * 256 * 2
    assert sp.dsd_workspace_bytes(A.m, False, Bd.m, False,
                                  sp.Matrix(16384, 256, got)) == 0  # (NN)
    ws = _ws(nbytes)
    events = sp.incall_events()
    for i in range(3):
        got.fill_(float("nan"))
        launches = sp.bt_launches()
        (sp.MatmulEx if ex else sp.Matmul)(A.m, False, Bd.m, True, C, workspace=ws)
        assert sp.bt_launches() == launches + 1
        _equal(got, want, f"dsd nt ws {dtype} ex={ex} call {i}")
    assert sp.incall_events() == events


# ------------------------------------------------ 2. the counter is live --

def test_incall_counter_is_live():
    """Fresh process: the first library-route call allocates (>= 1 event),
    the same call with a workspace causes none."""
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "workspace_child.py")],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["workspace_bytes"] == 4096 * 256 * 2
    assert out["library"]["exact"] and out["workspace"]["exact"]
    assert out["library"]["bt"] == 1 and out["workspace"]["bt"] == 1
    assert out["library"]["incall"] >= 1
    assert out["workspace"]["incall"] == 0


# -------------------------------------- 3. too small or misaligned memory --

@pytest.mark.parametrize("case", ["one_byte_short", "offset_by_8"])
def test_unfit_workspace_keeps_nt_kernel(case, bt_small):
    p = shared_problem(4096)
    nbytes = p.workspace_bytes()
    if case == "one_byte_short":
        ws = _ws(nbytes - 1)
    else:
        ws = _ws(nbytes + 16)[8:]
        assert ws.data_ptr() % 16 == 8 and ws.numel() >= nbytes
    p.clear()
    torch.cuda.synchronize()
    launches, events, held = sp.bt_launches(), sp.incall_events(), sp.retained_bytes()
    p.run(workspace=ws)
    assert sp.bt_launches() == launches, "the transposed path ran"
    assert sp.incall_events() == events
    assert sp.retained_bytes() == held, "fell back to the library buffer"
    p.check(f"sdd nt, workspace {case}")


# ------------------------------------------------------ 4. per-stream route --

def test_stream_registration_route(bt_small):
    p = shared_problem(4096)
    ws = _ws(p.workspace_bytes())
    sp.release_workspaces()  # (no buffer left over for a recycled handle)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    sp.set_stream_workspace(s, ws)
    try:
        p.clear()
        torch.cuda.synchronize()
        launches, held = sp.bt_launches(), sp.retained_bytes()
        p.run(stream=s.cuda_stream)
        assert sp.bt_launches() == launches + 1
        assert sp.retained_bytes() == held
        s.synchronize()
        p.check("registered stream")
    finally:
        sp.set_stream_workspace(s, None)
    # unregistered, a fresh stream: the library route and its buffer
    s2 = torch.cuda.Stream()
    assert s2.cuda_stream != s.cuda_stream
    p.clear()
    torch.cuda.synchronize()
    held = sp.retained_bytes()
    p.run(stream=s2.cuda_stream)
    assert sp.retained_bytes() >= held + p.bt_bytes
    s2.synchronize()
    p.check("library route after unregistering")
    assert sp.release_workspaces() >= p.bt_bytes


def test_stream_registration_rejects_bad_memory():
    ws = _ws(4096)
    s = torch.cuda.Stream()
    with pytest.raises(sp.SputnikError) as e:
        sp.set_stream_workspace(s, ws[8:])
    assert e.value.code == sp.hipErrorInvalidValue
    with pytest.raises(sp.SputnikError) as e:
        sp.set_stream_workspace(s, ws[:0])
    assert e.value.code == sp.hipErrorInvalidValue
    # the C entry point itself: a non-null pointer with zero bytes
    assert sp.lib().sputnik_set_stream_workspace(
        s.cuda_stream, ws.data_ptr(), 0) == sp.hipErrorInvalidValue
    # unregistering a stream that has no registration is not an error
    sp.set_stream_workspace(s, None)


# ------------------------------------------------------- 5. graph capture --

def test_graph_capture_sdd_with_workspace(bt_small):
    """The shape of test_graph_capture_sdd_bt_keeps_nt_kernel with a
    workspace allocated before the capture: the transpose and the product
    land in the graph, nothing is allocated or synchronised."""
    p = SddProblem(16384, 256, 2048, False, "f16", 21)
    ws = _ws(p.workspace_bytes())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        launches, events = sp.bt_launches(), sp.incall_events()
        p.run(workspace=ws)
        launches, events = sp.bt_launches() - launches, sp.incall_events() - events
    assert launches == 1 and events == 0, (launches, events)
    for rep in range(2):
        p.clear()
        g.replay()
        p.check(f"captured sdd nt with workspace, replay {rep}")
    del g


def test_graph_capture_dsd_nt_with_workspace(bt_small):
    got, want, (A, Bd, C) = kat_dsd(16384, 256, 2048, 1.0, False, True, "f16", seed=73)
    ws = _ws(sp.dsd_workspace_bytes(A.m, False, Bd.m, True, C))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        launches, events = sp.bt_launches(), sp.incall_events()
        sp.Matmul(A.m, False, Bd.m, True, C, workspace=ws)
        launches, events = sp.bt_launches() - launches, sp.incall_events() - events
    assert launches == 1 and events == 0, (launches, events)
    for rep in range(2):
        got.fill_(float("nan"))
        g.replay()
        _equal(got, want, f"captured dsd nt with workspace, replay {rep}")
    del g


def test_graph_capture_ops_sdd_uses_graph_pool(bt_small):
    """ops.sdd inside torch.cuda.graph: its workspace comes from the graph's
    private pool, so the captured step runs the transposed path too."""
    p = SddProblem(16384, 256, 2048, False, "f16", 22)
    topo = ops.SparseMatrix((16384, 2048), p.Cs.dev, p.Cs.m.offsets, p.Cs.m.indices)
    a, bt = p.A.dev, p.Bd.dev  # bt: B^T stored [N][K]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # (builds the topology's row indices)
        warm = ops.sdd(a, bt.t(), topo)
    torch.cuda.current_stream().wait_stream(s)
    _equal(warm.data, p.want, "ops.sdd eager")
    torch.cuda.synchronize()
    held = sp.retained_bytes()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        launches = sp.bt_launches()
        out = ops.sdd(a, bt.t(), topo)
        launches = sp.bt_launches() - launches
    assert launches == 1
    assert sp.retained_bytes() == held
    for rep in range(2):
        out.data.fill_(float("nan"))
        g.replay()
        _equal(out.data, p.want, f"captured ops.sdd, replay {rep}")
    del g


# --------------------------------------- 6. two threads, two streams --

def test_two_threads_two_streams_own_workspaces(bt_small):
    probs = [shared_problem(4096), shared_problem(6144)]
    streams = [torch.cuda.Stream() for _ in probs]
    wss = [_ws(p.workspace_bytes()) for p in probs]
    for p, s in zip(probs, streams):
        p.clear()
        s.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    events = sp.incall_events()
    errors = []

    def work(p, s, ws):
        try:
            for _ in range(4):
                p.run(stream=s.cuda_stream, workspace=ws)
        except Exception as e:  # noqa: BLE001 (reported below)
            errors.append(e)

    ts = [threading.Thread(target=work, args=a, daemon=True)
          for a in zip(probs, streams, wss)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=60)
        assert not t.is_alive(), "a thread is stuck in Matmul"
    assert not errors, errors
    assert sp.incall_events() == events
    for p, s in zip(probs, streams):
        s.synchronize()
        p.check(f"two threads n={p.n}")


# ------------------------------------------- 7. release and accounting --

def test_release_and_accounting(bt_small):
    p = shared_problem(4096)
    sp.release_workspaces()
    p.clear()
    p.run()  # library route, current stream
    held = sp.retained_bytes()
    assert held >= p.bt_bytes
    p.check("library route")
    freed = sp.release_workspaces()
    assert freed >= p.bt_bytes
    assert sp.retained_bytes() == held - freed
    assert sp.release_workspaces() == 0
    p.clear()
    p.run()
    p.check("library route after release")
    assert sp.retained_bytes() == held


# ------------------------------------------------------------------ 8. ops --

def test_ops_sdd_never_grows_library_buffers():
    """ops.sdd(a, b.t(), topo) and its backward with the path on (knob 1):
    the library retains nothing more, the transpose ran, and every result is
    bit-equal to the same ops with the path off (knob 0)."""
    rng = np.random.default_rng(81)
    m, k, n = 8192, 256, 4096
    A = IDense(m, k, rng, "f16")
    Bd = IDense(n, k, rng, "f16")  # B^T stored [N][K]
    Cs = ISparse(m, n, 0.6, rng, "f16")
    dc = Cs.dev.clone()  # (integer-valued upstream gradient)
    topo = ops.SparseMatrix((m, n), Cs.dev, Cs.m.offsets, Cs.m.indices)

    def step():
        a = A.dev.clone().requires_grad_(True)
        bt = Bd.dev.clone().requires_grad_(True)
        out = ops.sdd(a, bt.t(), topo)
        out.data.backward(dc)
        torch.cuda.synchronize()
        return out.data.detach(), a.grad, bt.grad

    prev = sp.tuning("sdd_bt_min_mib", 0)
    try:
        launches = sp.bt_launches()
        ref = step()  # (also makes this stream's pair workspaces)
        assert sp.bt_launches() == launches
        sp.tuning("sdd_bt_min_mib", 1)
        held, launches = sp.retained_bytes(), sp.bt_launches()
        got = step()
        assert sp.bt_launches() > launches
        assert sp.retained_bytes() <= held
    finally:
        sp.tuning("sdd_bt_min_mib", prev)
    want = _expect(Cs.blocks_of(A.values.astype(np.float64) @ Bd.values.T), "f16")
    _equal(got[0], want, "ops.sdd forward")
    for name, x, y in zip(("out", "da", "db"), got, ref):
        _equal(x, y, f"ops.sdd {name}: path on vs off")


def test_kat_helpers_still_drive_the_library_route(bt_small):
    """kat_sdd (no workspace) takes the library route: the default did not
    move."""
    sp.release_workspaces()
    launches = sp.bt_launches()
    got, want, plan = kat_sdd(8192, 256, 4096, 0.6, False, True, "f16", seed=5)
    assert plan == 1
    _equal(got, want, "kat_sdd nt")
    assert sp.bt_launches() == launches + 1
    assert sp.retained_bytes() >= 4096 * 256 * 2
