"""Same-process A/B of the gated SDD products against what callers do today:
two plain Matmuls and torch's silu / mul for the forward pass, one plain
Matmul and torch's silu_backward / mul sequence for the gradient pair, and a
whole GLU expert MLP step composed from ops.sdd, ops.dsd and torch. Protocol
of scripts/ab_sdd_activation.py: one process, every arm warmed for at least
--warm-ms of device time, then --rounds interleaved rounds of --calls
back-to-back calls; medians and ranges. Today's path is timed as two arms
(today_a, today_b): their difference is the in-process spread against which
the other arms are read.

Arms: today_a, auto (knob sdd_act_route = 0), fused (1), two_kernels (2),
today_b. The knob is set before each window, not inside it. Forward keeps
Z2 = x v1 in every arm (training needs it) and includes the plain product
Z1 = x w1 in every arm, so a forward call is two products everywhere. The
gradient arms write dZ2 to a buffer of its own, so every call sees the same
Z2. Calls are enqueued from Python; at the tile shapes it was not verified
that a window is bound by device time rather than by the host's enqueue rate.

Shapes (silu):
    c4_fwd    BASELINE config 4's x . v1 gated by x . w1: bf16, 8192 tokens,
              d_model 4096, 8 experts x d_ff 14336 (7168 blocks), NN
    c4_bwd    its dy . w2^T with w2 stored [8 x 14336, 4096]: NT, (dZ1, dZ2)
    tile_fwd  f16, 2048 x 2048 at 50% (128 blocks), K = 1024: the plain SDD
    tile_bwd  runs the 8-wave k-split tile (sdd_kernel 0)
    g8_fwd    f16, 6144 x 6144 at 50% (1152 blocks), K = 960 (no multiple of
    g8_bwd    128): the plain SDD runs the 8-wave grouped tile (sdd_kernel 1)
    c4_step   ops.glu_mlp forward + backward at config 4 against the same
              step composed from ops.sdd, torch's silu / mul and ops.dsd

The three library arms must agree bit for bit; today's arm agrees within
tests/helpers.RTOL (asserted; --report-mismatch records the number of
elements out of tolerance per output in the line instead). One JSON line per
shape.

python scripts/ab_sdd_gated.py [--shapes c4_fwd,...] [--out profiles/sdd_gated/ab_sdd_gated.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALL = "c4_fwd,c4_bwd,tile_fwd,tile_bwd,g8_fwd,g8_bwd,c4_step"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=ALL)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warm-ms", type=float, default=100.0)
    ap.add_argument("--out", default="")
    ap.add_argument("--report-mismatch", action="store_true",
                    help="record in the line how many elements of today's "
                         "arm are out of tolerance instead of asserting")
    a = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    import sputnik_amd as sp
    from sputnik_amd import matrix_utils as mu
    from sputnik_amd import ops
    from tests.helpers import RTOL

    assert torch.cuda.is_available(), "needs a GPU: there is no CPU timing"
    gen = torch.Generator(device="cuda").manual_seed(17)
    act = "silu"

    def normal(rows, cols, dt, scale):
        return (torch.randn(rows, cols, generator=gen, device="cuda") *
                scale).to(dt)

    def window(fn, calls):
        # (the route knob is set here, outside the timed calls; today's arms
        # do not read it)
        sp.tuning("sdd_act_route", getattr(fn, "route", 0))
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(calls):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / calls  # us per call

    def same(p, q):
        return torch.equal(p.view(torch.int16), q.view(torch.int16))

    def close(got, want, name, what):
        want = want.float()
        tol = RTOL[name] * (want.abs() + want.square().mean().sqrt())
        bad = int(((got.float() - want).abs() > tol).sum())
        if a.report_mismatch:
            return bad
        assert bad == 0, f"{what}: {bad} elements away from today's arm"
        return 0

    def config4():
        return torch.bfloat16, 8192, 4096, 14336, 8

    def product(shape):
        """One SDD problem: (dtype name, X, ta, W [, W1], tb, offsets,
        indices, M, N, K)."""
        grad = shape.endswith("_bwd")
        if shape.startswith("c4_"):
            dt, tokens, dm, dff, ne = config4()
            off, idx = mu.expert_block_diagonal(ne, tokens // ne // 128,
                                                dff // 128)
            x = sp.Matrix(tokens, dm, normal(tokens, dm, dt, 1.0))
            if grad:  # dy . w2^T, w2 stored [ne * dff, dm]
                w = sp.Matrix(ne * dff, dm, normal(ne * dff, dm, dt, 1 / 64))
                return "bf16", x, False, w, None, True, off, idx, tokens, ne * dff, dm
            w = sp.Matrix(dm, ne * dff, normal(dm, ne * dff, dt, 1 / 64))
            w1 = sp.Matrix(dm, ne * dff, normal(dm, ne * dff, dt, 1 / 64))
            return "bf16", x, False, w, w1, False, off, idx, tokens, ne * dff, dm
        d, k = (2048, 1024) if shape.startswith("tile_") else (6144, 960)
        assert shape.startswith(("tile_", "g8_")), shape
        dt = torch.float16
        rng = np.random.default_rng(3)
        nb = mu.nonzeros_for_density(d, d, 0.5) // (128 * 128)
        off, idx = mu.random_topology(d // 128, d // 128, nb, rng)
        x = sp.Matrix(d, k, normal(d, k, dt, 1.0))
        w = sp.Matrix(k, d, normal(k, d, dt, 1 / 32))
        w1 = None if grad else sp.Matrix(k, d, normal(k, d, dt, 1 / 32))
        return "f16", x, False, w, w1, False, off, idx, d, d, k

    def product_arms(shape):
        name, A, ta, Bm, B1, tb, off, idx, m, n, k = product(shape)
        grad = shape.endswith("_bwd")
        dt = {"f16": torch.float16, "bf16": torch.bfloat16}[name]
        nb = int(off[-1])
        offs = torch.from_numpy(off.astype(np.int32)).cuda()
        idxs = torch.from_numpy(idx.astype(np.int16)).cuda()

        def blocks():
            return torch.empty(nb, 128, 128, dtype=dt, device="cuda")

        rows = []

        def desc(data):
            c = sp.BlockMatrix(m, n, 128, nb * 128 * 128, data, offs, idxs)
            if not rows:
                sp.AllocateRowIndicesBuffer(c)
                sp.RowIndices(c, c.row_indices)
                rows.append(c.row_indices)
            c.row_indices = rows[0]
            return c

        out, z1, z2 = blocks(), blocks(), blocks()
        C, Z1, Z2 = desc(out), desc(z1), desc(z2)
        kernel = sp.sdd_kernel(A, ta, Bm, tb, C)
        sp.tuning("sdd_act_route", 0)
        auto_route = sp.sdd_act_route(A, ta, Bm, tb, C)
        if grad:
            # what a forward pass would have left
            z1.copy_(normal(nb * 128, 128, dt, 1.0).view(nb, 128, 128))
            z2.copy_(normal(nb * 128, 128, dt, 1.0).view(nb, 128, 128))
            du = blocks()
            D = desc(blocks())

            def today():
                sp.Matmul(A, ta, Bm, tb, D)
                dz2 = D.data * F.silu(z1)
                dz1 = torch.ops.aten.silu_backward(D.data * z2, z1)
                return dz1, dz2

            def lib(route):
                def run():
                    sp.MatmulGatedGrad(A, ta, Bm, tb, C, act, z1, z2, du)
                    return out, du
                run.route = route
                return run
        else:
            def today():
                sp.Matmul(A, ta, B1, tb, Z1)
                sp.Matmul(A, ta, Bm, tb, Z2)
                return (F.silu(z1) * z2,)

            def lib(route):
                def run():
                    sp.Matmul(A, ta, B1, tb, Z1)
                    sp.MatmulGated(A, ta, Bm, tb, C, act, z1, z2)
                    return (out,)
                run.route = route
                return run
        flops = 2.0 * nb * 128 * 128 * k * (1 if grad else 2)
        info = {"shape": shape, "dtype": name, "grad": grad,
                "transposes": f"{'T' if ta else 'N'}{'T' if tb else 'N'}",
                "mnk": [m, n, k], "blocks": nb, "plain_kernel": int(kernel),
                "auto_route": int(auto_route)}
        return name, today, lib, flops, info

    def step_arms(shape):
        dt, tokens, dm, dff, ne = config4()
        off, idx = mu.expert_block_diagonal(ne, tokens // ne // 128, dff // 128)
        nb = int(off[-1])
        topo = ops.SparseMatrix(
            (tokens, ne * dff),
            torch.empty(nb, 128, 128, dtype=dt, device="cuda"),
            torch.from_numpy(off.astype(np.int32)).cuda(),
            torch.from_numpy(idx.astype(np.int16)).cuda())
        x = normal(tokens, dm, dt, 1.0).requires_grad_(True)
        w1 = normal(dm, ne * dff, dt, 1 / 64).requires_grad_(True)
        v1 = normal(dm, ne * dff, dt, 1 / 64).requires_grad_(True)
        w2 = normal(ne * dff, dm, dt, 1 / 64).requires_grad_(True)
        dy = normal(tokens, dm, dt, 1.0)
        leaves = (x, w1, v1, w2)

        def finish(y):
            for t in leaves:
                t.grad = None
            y.backward(dy)
            return (y.detach(),) + tuple(t.grad for t in leaves)

        def today():
            z1, z2 = ops.sdd(x, w1, topo), ops.sdd(x, v1, topo)
            h = topo.with_data(F.silu(z1.data) * z2.data)
            return finish(ops.dsd(h, w2))

        def lib(route):
            def run():
                return finish(ops.glu_mlp(x, w1, v1, w2, topo, act))
            run.route = route
            return run
        # forward: 2 SDD + 1 DSD; backward: 1 SDD + 1 DSD (dw2) + 2 DDS + 2 DSD
        flops = 2.0 * nb * 128 * 128 * dm * 9
        info = {"shape": shape, "dtype": "bf16", "grad": True,
                "mnk": [tokens, ne * dff, dm], "blocks": nb}
        return "bf16", today, lib, flops, info

    prev_route = sp.tuning("sdd_act_route")
    lines = []
    try:
        for shape in a.shapes.split(","):
            name, today, lib, flops, rec = (
                step_arms(shape) if shape.endswith("_step")
                else product_arms(shape))
            # one call of each arm: the library arms agree bit for bit,
            # today's arm within the tolerance
            want = [t.clone() for t in today()]
            got = {}
            for r in (1, 2, 0):
                sp.tuning("sdd_act_route", r)
                got[r] = [t.clone() for t in lib(r)()]
            torch.cuda.synchronize()
            for r in (2, 0):
                for i, (p, q) in enumerate(zip(got[1], got[r])):
                    assert same(p, q), (shape, r, i)
            mismatch = [close(p, q, name, f"{shape} output {i}")
                        for i, (p, q) in enumerate(zip(got[1], want))]
            del want, got

            arms = {"today_a": today, "auto": lib(0), "fused": lib(1),
                    "two_kernels": lib(2), "today_b": today}
            for fn in arms.values():
                spent = 0.0
                while spent < a.warm_ms * 1e3:
                    spent += window(fn, 5) * 5
            ts = {k_: [] for k_ in arms}
            for _ in range(a.rounds):
                for k_, fn in arms.items():
                    torch.cuda.synchronize()
                    ts[k_].append(window(fn, a.calls))
            med = {k_: sorted(v)[len(v) // 2] for k_, v in ts.items()}
            base = (med["today_a"] + med["today_b"]) / 2
            if a.report_mismatch:
                rec["today_out_of_tolerance"] = mismatch
            rec.update({"calls": a.calls, "rounds": a.rounds,
                        "build": sp.build_hash()})
            for k_, v in ts.items():
                rec[k_] = {"us": round(med[k_], 1), "min": round(min(v), 1),
                           "max": round(max(v), 1),
                           "tflops": round(flops / med[k_] / 1e6, 1)}
            rec["spread_pct"] = round(
                100 * abs(med["today_a"] - med["today_b"]) / base, 2)
            for k_ in ("auto", "fused", "two_kernels"):
                rec[k_ + "_vs_today_pct"] = round(
                    100 * (med[k_] - base) / base, 2)
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
            del today, lib, arms
            torch.cuda.empty_cache()
    finally:
        sp.tuning("sdd_act_route", prev_route)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
