"""Same-process A/B of the two routes of the transposed-B path (INTEGRATION.md
3b): SDD NT and TT at dim^3 (default 16384) and 50%, on the library route
(the library's own buffer) and on the per-call route (a caller-owned
workspace). Both enqueue the same two launches, so the times should agree;
this measures it. The library route is timed as two separate arms
(library_a, library_b): their difference is the run-to-run spread of this
box, the margin against which the workspace arm is read. Every arm is warmed
up for at least --warm-ms of device time, then timed in interleaved rounds
of --calls back-to-back launches; medians. The outputs of the two routes
are compared bit for bit. Prints one JSON line.

With a package that lacks the workspace API (an older tree named by
SPUTNIK_AMD_TREE) only the library arms run, for a comparison across
versions on one box.

python scripts/ab_bt_workspace.py [--dim 16384] [--density 0.5] [--rounds 7]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("SPUTNIK_AMD_TREE") or ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=16384)
    ap.add_argument("--density", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warm-ms", type=float, default=100.0)
    ap.add_argument("--dtype", default="f16", choices=["f16", "bf16"])
    a = ap.parse_args()
    import numpy as np
    import torch
    import sputnik_amd as sp
    from sputnik_amd import matrix_utils as mu

    assert torch.cuda.is_available(), "needs a GPU: there is no CPU timing"
    has_ws = hasattr(sp, "sdd_workspace_bytes")
    d = a.dim
    dt = {"f16": torch.float16, "bf16": torch.bfloat16}[a.dtype]
    rng = np.random.default_rng(1)
    nb = mu.nonzeros_for_density(d, d, a.density) // (128 * 128)
    off, idx = mu.random_topology(d // 128, d // 128, nb, rng)
    g = torch.Generator(device="cuda").manual_seed(7)

    def dense():
        return torch.randint(-1, 2, (d, d), generator=g, device="cuda",
                             dtype=torch.int8).to(dt)

    x, w = dense(), dense()
    data = torch.empty(nb, 128, 128, dtype=dt, device="cuda")
    C = sp.BlockMatrix(d, d, 128, nb * 128 * 128, data,
                       torch.from_numpy(off.astype(np.int32)).cuda(),
                       torch.from_numpy(idx.astype(np.int16)).cuda())
    sp.AllocateRowIndicesBuffer(C)
    sp.RowIndices(C, C.row_indices)
    A, Bm = sp.Matrix(d, d, x), sp.Matrix(d, d, w)
    flops = 2.0 * nb * 128 * 128 * d
    out = {"op": "sdd", "dim": d, "density": a.density, "dtype": a.dtype,
           "blocks": int(nb), "calls": a.calls, "rounds": a.rounds,
           "has_workspace_api": has_ws, "build": sp.build_hash()}

    def window(fn, calls):
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(calls):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / calls  # us per call

    for trans, ta in (("NT", False), ("TT", True)):
        assert sp.sdd_kernel(A, ta, Bm, True, C) == 4, "the transposed-B path is off"
        arms = {"library_a": lambda: sp.Matmul(A, ta, Bm, True, C)}
        if has_ws:
            nbytes = sp.sdd_workspace_bytes(A, ta, Bm, True, C)
            assert nbytes >= d * d * 2
            ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            arms["workspace"] = lambda: sp.Matmul(A, ta, Bm, True, C, workspace=ws)
        arms["library_b"] = arms["library_a"]
        ref = None
        for name, fn in arms.items():  # warm-up, and the routes' outputs agree
            data.fill_(float("nan"))
            fn()
            torch.cuda.synchronize()
            if ref is None:
                ref = data.clone()
            assert torch.equal(data, ref), f"{trans} {name}: output differs"
            spent = 0.0
            while spent < a.warm_ms * 1e3:
                spent += window(fn, 10) * 10
        if has_ws:
            e0, b0 = sp.incall_events(), sp.bt_launches()
            arms["workspace"]()
            out[f"{trans}_workspace_incall_events"] = sp.incall_events() - e0
            out[f"{trans}_workspace_bt_launches"] = sp.bt_launches() - b0
        ts = {k: [] for k in arms}
        for _ in range(a.rounds):
            for k, fn in arms.items():
                ts[k].append(window(fn, a.calls))
        med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
        for k, v in ts.items():
            out[f"{trans}_{k}"] = {"us": round(med[k], 1), "min": round(min(v), 1),
                                   "max": round(max(v), 1),
                                   "tflops": round(flops / med[k] / 1e6, 1)}
        lib = (med["library_a"] + med["library_b"]) / 2
        out[f"{trans}_spread_pct"] = round(
            100 * abs(med["library_a"] - med["library_b"]) / lib, 2)
        if has_ws:
            out[f"{trans}_workspace_vs_library_pct"] = round(
                100 * (med["workspace"] - lib) / lib, 2)
    if has_ws:
        out["retained_bytes"] = sp.retained_bytes()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
