"""The route table: what every kernel-selection query answers for a fixed
list of problems under a fixed list of knob settings.

`rows()` enumerates the problems and asks the library; nothing is launched,
so the operands are uninitialised device tensors of the true size
(torch.empty) and size costs allocation only. The shapes are those of the
KATs that pin each code (tests/test_gpu_kat.py). tests/route_table.json is
the output of this module recorded once, with the CU count it was recorded
on; tests/test_gpu_route_table.py asserts that the library still reproduces
every row, so a change to the dispatcher that moves any route shows up as a
diff of one named row.

Run as a script it prints the table as JSON (or writes it to argv[1]).
"""

import contextlib
import gc
import json
import sys

import torch

import sputnik_amd as sp
from sputnik_amd import matrix_utils as mu

B = mu.BLOCK
TRANSPOSES = [(False, False), (False, True), (True, False), (True, True)]
TNAME = {False: "N", True: "T"}


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _empty(n, dtype=torch.float16):
    return torch.empty(max(int(n), 1), dtype=dtype, device="cuda")


def dense(rows, cols):
    return sp.Matrix(rows, cols, _empty(rows * cols))


def sparse(rows, cols, nb, transposed_meta=True, row_indices=False):
    """A BCSR descriptor of nb stored blocks (topology uninitialised: the
    queries read the descriptor only)."""
    m = sp.BlockMatrix(rows, cols, B, nb * B * B, _empty(nb * B * B),
                       _empty(rows // B + 1, torch.int32),
                       _empty(nb, torch.int16))
    if transposed_meta:
        sp.AllocateTransposeBuffers(m)
    if row_indices:
        sp.AllocateRowIndicesBuffer(m)
    return m


def blocks_at(rows, cols, density):
    return mu.nonzeros_for_density(rows, cols, density) // (B * B)


@contextlib.contextmanager
def knobs(settings):
    """Sets the knobs of one row (the "dsd4w" one through select_dsd_kernel)
    and restores them afterwards, in reverse order."""
    prev = []
    try:
        for name, value in settings:
            if name == "dsd4w":
                prev.append((name, sp.select_dsd_kernel(value)))
            else:
                prev.append((name, sp.tuning(name, value)))
        yield
    finally:
        for name, value in reversed(prev):
            if name == "dsd4w":
                sp.select_dsd_kernel(value)
            else:
                sp.tuning(name, value)


def _knob_id(settings):
    return ",".join(f"{n}={v}" for n, v in settings) or "default"


# ------------------------------------------------------------ DSD / DDS --
# (m, k, n, density of the sparse operand). DSD: A sparse. DDS: B sparse.
SQUARE = (4096, 4096, 4096, 0.5)
PANELS = [(512, 4096, 4096, 0.5), (1024, 4096, 4096, 0.5), (2048, 4096, 4096, 0.5)]
# test_kat_dsd_tall_pipe's shapes (DSD: tall A; the DDS rows mirror them, a
# tall op(B)^T, as test_kat_dds_ex_tall mirrors test_kat_dsd_ex_tall).
TALL = [(300 * 128, 512, 1024, 0.05), (300 * 128, 256, 2048, 0.02),
        (300 * 128, 2048, 512, 0.02), (280 * 128, 4096, 1024, 1.0)]
# test_kat_dsd_nt_bt_transpose's shape (with sdd_bt_min_mib = 1).
BT_DSD = (16384, 256, 2048, 1.0)
REJECTED = (4096, 4096, 4100, 0.5)  # n not a multiple of 8

BT_SMALL = ("sdd_bt_min_mib", 1)

# (shape, knob settings, mode): mode "" plain, "capture" queried while a side
# stream is being captured, "workspace" with a stream workspace registered.
DENSE_OUT_ROWS = (
    [(SQUARE, s, "") for s in ([], [("dsd4w", 0)], [("pairs", 0)],
                               [("tall", 0)], [("tall", 2)],
                               [("tall", 2), ("dsd4w", 0)])] +
    [(p, s, "") for p in PANELS for s in ([], [("dsd4w", 0)], [("split", 0)])] +
    [(t, s, "") for t in TALL
     for s in ([("tall4w", 1)], [("tall4w", 0)], [("tall", 0)],
               [("tall4w", 0), ("dsd4w", 0)])] +
    [(BT_DSD, [BT_SMALL], ""), (BT_DSD, [BT_SMALL], "capture"),
     (BT_DSD, [BT_SMALL], "workspace"), (BT_DSD, [], ""),
     (SQUARE, [], "capture"), (SQUARE, [], "workspace"),
     (REJECTED, [], "")])


def _mirror(shape):
    m, k, n, d = shape
    return (n, k, m, d)


def _dense_out_operands(family, shape, ta, tb):
    m, k, n, density = shape
    if family == "dsd":
        ar, ac = (k, m) if ta else (m, k)
        a = sparse(ar, ac, blocks_at(ar, ac, density))
        b = dense(*((n, k) if tb else (k, n)))
    else:
        a = dense(*((k, m) if ta else (m, k)))
        br, bc = (n, k) if tb else (k, n)
        b = sparse(br, bc, blocks_at(br, bc, density))
    return a, b, dense(m, n)


def _query_dense_out(family, a, ta, b, tb, c, mode):
    plan = sp.dsd_plan if family == "dsd" else sp.dds_plan
    out = {}
    if mode == "capture":
        # begin capture, query, end capture: no product is launched (the
        # fill keeps the captured graph from being empty)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        filler = _empty(16)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            filler.fill_(0)
            out["plan"] = plan(a, ta, b, tb, c, stream=s.cuda_stream)
        del g
    elif mode == "workspace":
        ws = torch.empty(32 << 20, dtype=torch.uint8, device="cuda")
        sp.set_stream_workspace(None, ws)
        try:
            out["plan"] = plan(a, ta, b, tb, c)
            if family == "dsd":
                out["workspace_bytes"] = sp.dsd_workspace_bytes(a, ta, b, tb, c)
        finally:
            sp.set_stream_workspace(None, None)
        return out
    else:
        out["plan"] = plan(a, ta, b, tb, c)
    if family == "dsd":
        out["workspace_bytes"] = sp.dsd_workspace_bytes(a, ta, b, tb, c)
    return out


def dense_out_rows():
    for family in ("dsd", "dds"):
        variants = [("", lambda s: s)]
        if family == "dds":  # the tall / panel side of a DDS is N
            variants.append(("mirrored ", _mirror))
        for label, fn in variants:
            for ta, tb in TRANSPOSES:
                cache = {}
                for shape, settings, mode in DENSE_OUT_ROWS:
                    if label and shape not in PANELS + TALL:
                        continue
                    if family == "dds" and not label and shape in TALL:
                        continue  # (only the mirrored DDS is tall)
                    real = fn(shape)
                    if real not in cache:
                        cache.clear()  # one problem's tensors alive at a time
                        cache[real] = _dense_out_operands(family, real, ta, tb)
                    a, b, c = cache[real]
                    m, k, n, density = real
                    rid = (f"{family} {TNAME[ta]}{TNAME[tb]} {label}{m}x{k}x{n}"
                           f"@{density} [{_knob_id(settings)}]"
                           + (f" ({mode})" if mode else ""))
                    with knobs(settings):
                        yield rid, family, _query_dense_out(family, a, ta, b, tb,
                                                            c, mode)


# ------------------------------------------------------------------ SDD --
def sdd_problems():
    """(name, m, k, n, stored blocks, knob settings, row_indices)."""
    n_cu = cus()
    out = []
    for k in (4096, 8192):  # test_sdd_plan_ksplit_default_gate
        # (knob sdd_ksplit: 1 is off, its lowest value; 8 opts in)
        for ks in (1, 8):
            out.append((4096, k, 4096, 205, [("sdd_ksplit", ks)], True))
    # test_kernel_queries_match_config3 and test_sdd_plan_threshold
    for m, k, n in ((4096, 4096, 4096), (8192, 128, 8192)):
        for nb in (4 * n_cu - 1, 4 * n_cu):
            for s in ([], [("dsd4w", 0)], [("grouped_sdd", 0)]):
                out.append((m, k, n, nb, s, True))
    for m in (2048, 1920):  # test_kat_sdd_grouped_pow2_stride
        out.append((m, 256, 16384, 4 * n_cu + 37, [], True))
        out.append((m, 256, 16384, 4 * n_cu + 37, [("dsd4w", 0)], True))
    for k in (512, 256):  # test_kat_sdd_bt_transpose
        for n in (4096, 6144):
            nb = blocks_at(8192, n, 0.6)
            out.append((8192, k, n, nb, [BT_SMALL], True))
            out.append((8192, k, n, nb, [("sdd_bt_min_mib", 0)], True))
    out.append((8192, 128, 8192, 4 * n_cu, [], False))  # no row_indices
    return out


def sdd_rows():
    for ta, tb in TRANSPOSES:
        cache = {}
        for m, k, n, nb, settings, row_indices in sdd_problems():
            key = (m, k, n, nb, row_indices)
            if key not in cache:
                cache.clear()
                cache[key] = (dense(*((k, m) if ta else (m, k))),
                              dense(*((n, k) if tb else (k, n))),
                              sparse(m, n, nb, transposed_meta=False,
                                     row_indices=row_indices))
            a, b, c = cache[key]
            for act in (0, 1, 2):
                s = settings + [("sdd_act_route", act)]
                rid = (f"sdd {TNAME[ta]}{TNAME[tb]} {m}x{k}x{n} nb={nb}"
                       f"{'' if row_indices else ' no row_indices'}"
                       f" [{_knob_id(s)}]")
                with knobs(s):
                    yield rid, "sdd", {
                        "plan": sp.sdd_plan(a, ta, b, tb, c),
                        "kernel": sp.sdd_kernel(a, ta, b, tb, c),
                        "act_route": sp.sdd_act_route(a, ta, b, tb, c),
                        "workspace_bytes": sp.sdd_workspace_bytes(a, ta, b, tb, c),
                    }


def counters():
    """What a read-only query must leave alone. Graphs that earlier code
    dropped are collected first and their capture workspaces freed
    (capture_workspaces() does that), so that they are not counted as held
    before the enumeration and as gone after it: entering torch.cuda.graph
    collects garbage too."""
    gc.collect()
    torch.cuda.synchronize()
    captures = sp.capture_workspaces()
    return {"retained_bytes": sp.retained_bytes(),
            "incall_events": sp.incall_events(),
            "bt_launches": sp.bt_launches(),
            "capture_workspaces": captures}


def rows():
    """[{"id", "family", "result"}], in a fixed order."""
    out = []
    for gen in (dense_out_rows, sdd_rows):
        for rid, family, result in gen():
            out.append({"id": rid, "family": family, "result": result})
    torch.cuda.empty_cache()
    return out


def table():
    before = counters()
    r = rows()
    after = counters()
    return {"cus": cus(), "counters_unchanged": before == after, "rows": r}


if __name__ == "__main__":
    text = json.dumps(table(), indent=0, sort_keys=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")
    else:
        print(text)
