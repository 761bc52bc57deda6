"""Same-process A/B of the SDD activation products against what callers do
today: a plain Matmul into Z followed by torch's gelu (tanh form) for the
forward pass, and a plain Matmul followed by torch's gelu backward for the
gradient. Protocol of scripts/ab_accumulate.py: one process, every arm
warmed for at least --warm-ms of device time, then --rounds interleaved
rounds of --calls back-to-back calls; medians. Today's path is timed as two
arms (today_a, today_b): their difference is the in-process spread against
which the other arms are read.

Arms: today_a, auto (knob sdd_act_route = 0), fused (1), two_kernels (2),
today_b. Forward keeps Z in every arm (training needs it). The knob is set
before each window, not inside it. Calls are enqueued from Python; at the
tile shapes (about 15 us per call) it was not verified that a window is
bound by device time rather than by the host's enqueue rate, which is the
same two launches per call for today's arm and for two_kernels and one for
fused.

Shapes (gelu):
    c4_fwd    BASELINE config 4's x . w1: bf16, 8192 tokens, d_model 4096,
              8 experts x d_ff 14336 (7168 blocks), NN
    c4_bwd    its dy . w2^T with w2 stored [8 x 14336, 4096]: NT, gradient
    tile_fwd  f16, 2048 x 2048 at 50% (128 blocks), K = 1024: the plain SDD
    tile_bwd  runs the 8-wave k-split tile (sdd_kernel 0); forward / gradient
    g8_fwd    f16, 6144 x 6144 at 50% (1152 blocks), K = 960 (no multiple of
    g8_bwd    128): the plain SDD runs the 8-wave grouped tile (sdd_kernel 1)

The three library arms must agree bit for bit; today's arm agrees within
tests/helpers.RTOL (torch evaluates gelu with its own tanh). One JSON line
per shape.

python scripts/ab_sdd_activation.py [--shapes c4_fwd,c4_bwd,tile_fwd,tile_bwd]
                  [--out profiles/sdd_activation/ab_sdd_activation.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c4_fwd,c4_bwd,tile_fwd,tile_bwd")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warm-ms", type=float, default=100.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    import sputnik_amd as sp
    from sputnik_amd import matrix_utils as mu
    from tests.helpers import RTOL

    assert torch.cuda.is_available(), "needs a GPU: there is no CPU timing"
    gen = torch.Generator(device="cuda").manual_seed(11)

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

    def problem(shape):
        """(dtype name, A, ta, B, tb, offsets, indices, M, N, K, grad)"""
        grad = shape.endswith("_bwd")
        if shape.startswith("c4_"):
            dt, tokens, dm, dff, ne = torch.bfloat16, 8192, 4096, 14336, 8
            off, idx = mu.expert_block_diagonal(ne, tokens // ne // 128,
                                                dff // 128)
            x = sp.Matrix(tokens, dm, normal(tokens, dm, dt, 1.0))
            if grad:  # dy . w2^T, w2 stored [ne * dff, dm]
                w = sp.Matrix(ne * dff, dm, normal(ne * dff, dm, dt, 1 / 64))
                return "bf16", x, False, w, True, off, idx, tokens, ne * dff, dm, True
            w = sp.Matrix(dm, ne * dff, normal(dm, ne * dff, dt, 1 / 64))
            return "bf16", x, False, w, False, off, idx, tokens, ne * dff, dm, False
        assert shape.startswith(("tile_", "g8_")), shape
        d, k = (2048, 1024) if shape.startswith("tile_") else (6144, 960)
        dt = torch.float16
        rng = np.random.default_rng(3)
        nb = mu.nonzeros_for_density(d, d, 0.5) // (128 * 128)
        off, idx = mu.random_topology(d // 128, d // 128, nb, rng)
        x = sp.Matrix(d, k, normal(d, k, dt, 1.0))
        w = sp.Matrix(k, d, normal(k, d, dt, 1 / 32))
        return "f16", x, False, w, False, off, idx, d, d, k, grad

    prev_route = sp.tuning("sdd_act_route")
    lines = []
    try:
        for shape in a.shapes.split(","):
            name, A, ta, Bm, tb, off, idx, m, n, k, grad = problem(shape)
            dt = {"f16": torch.float16, "bf16": torch.bfloat16}[name]
            nb = int(off[-1])
            offs = torch.from_numpy(off.astype(np.int32)).cuda()
            idxs = torch.from_numpy(idx.astype(np.int16)).cuda()

            def blocks():
                return torch.empty(nb, 128, 128, dtype=dt, device="cuda")

            def desc(data):
                return sp.BlockMatrix(m, n, 128, nb * 128 * 128, data, offs, idxs)

            out, z = blocks(), blocks()
            C, Zm = desc(out), desc(z)
            sp.AllocateRowIndicesBuffer(C)
            sp.RowIndices(C, C.row_indices)
            Zm.row_indices = C.row_indices
            kernel = sp.sdd_kernel(A, ta, Bm, tb, C)
            sp.tuning("sdd_act_route", 0)
            auto_route = sp.sdd_act_route(A, ta, Bm, tb, C)
            if grad:
                # the pre-activation a forward pass would have left
                z.copy_(normal(nb * 128, 128, dt, 1.0).view(nb, 128, 128))
                G = desc(blocks())
                G.row_indices = C.row_indices

                def today():
                    sp.Matmul(A, ta, Bm, tb, G)
                    return torch.ops.aten.gelu_backward(G.data, z,
                                                        approximate="tanh")

                def lib(route):
                    def run():
                        sp.MatmulActivationGrad(A, ta, Bm, tb, C, "gelu", z)
                        return out
                    run.route = route
                    return run
            else:
                def today():
                    sp.Matmul(A, ta, Bm, tb, Zm)
                    return F.gelu(z, approximate="tanh")

                def lib(route):
                    def run():
                        sp.MatmulActivation(A, ta, Bm, tb, C, "gelu", z)
                        return out
                    run.route = route
                    return run

            # one call of each arm: the library arms agree bit for bit,
            # today's arm within the tolerance
            want = today().float()
            got = {}
            for r in (1, 2, 0):
                sp.tuning("sdd_act_route", r)
                got[r] = lib(r)().clone()
            torch.cuda.synchronize()
            for r in (2, 0):
                assert torch.equal(got[1].view(torch.int16),
                                   got[r].view(torch.int16)), (shape, r)
            tol = RTOL[name] * (want.abs() + want.square().mean().sqrt())
            bad = int(((got[1].float() - want).abs() > tol).sum())
            assert bad == 0, f"{shape}: {bad} elements away from torch's gelu"
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
            flops = 2.0 * nb * 128 * 128 * k
            rec = {"shape": shape, "dtype": name, "grad": grad,
                   "transposes": f"{'T' if ta else 'N'}{'T' if tb else 'N'}",
                   "mnk": [m, n, k], "blocks": nb, "plain_kernel": int(kernel),
                   "auto_route": int(auto_route), "calls": a.calls,
                   "rounds": a.rounds, "build": sp.build_hash()}
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
            del out, z, C, Zm, A, Bm
            torch.cuda.empty_cache()
    finally:
        sp.tuning("sdd_act_route", prev_route)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
