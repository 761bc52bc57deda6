"""Same-process A/B of the MoE token permutation kernels (padded gather,
weighted padded scatter, router-weight gradient; sputnik/block/moe.h) against
the torch formulation a caller has today. Protocol of scripts/ab_sdd_gated.py:
one process, every arm warmed for at least --warm-ms of device time, then
--rounds interleaved rounds of --calls back-to-back calls; medians and ranges.
Today's path is timed as two arms (today_a, today_b): their difference is the
in-process spread against which the library arm is read.

Today's arms:
    gather   torch.zeros(rows, hidden) + index_copy_ of x.index_select(token)
    scatter  y.index_select(row_of) * w, .view(tokens, top_k, hidden).sum(1)
    wgrad    (dout.index_select(token) * y.index_select(row_of)).sum(-1)

Shapes (bf16, 8 experts, uniformly random routing, bf16 router weights, the
padded matrix sized by moe_rows_bound so no arm waits for the host):
    c4_k1   BASELINE config 4's activations: 8192 tokens x 4096, top_k 1
    c4_k2   the same at top_k 2
    big_k2  32768 tokens x 4096, top_k 2: x alone is 256 MiB and the padded
            matrix 512 MiB, past the Infinity Cache

Per kernel the line has microseconds, the achieved rate from the algorithmic
byte count (gather: n rows read + `rows` rows written; scatter: n rows read +
`tokens` rows written; wgrad: n + tokens rows read; metadata and weights are
left out) and that rate as a share of the 6.3 TB/s achievable HBM rate. The
gather arms must agree bit for bit; scatter and wgrad within
tests/helpers.RTOL of today's arm (asserted). One JSON line per shape.

python scripts/ab_moe_permute.py [--shapes c4_k1,...] [--out profiles/moe_permute/ab_moe_permute.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALL = "c4_k1,c4_k2,big_k2"
SHAPES = {"c4_k1": (8192, 4096, 8, 1), "c4_k2": (8192, 4096, 8, 2),
          "big_k2": (32768, 4096, 8, 2)}
HBM_TBS = 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=ALL)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warm-ms", type=float, default=100.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import sputnik_amd as sp
    from sputnik_amd import ops
    from tests.helpers import RTOL

    assert torch.cuda.is_available(), "needs a GPU: there is no CPU timing"
    gen = torch.Generator(device="cuda").manual_seed(23)
    dt = torch.bfloat16

    def window(fn, calls):
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(calls):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / calls  # us per call

    def close(got, want, what):
        want = want.float()
        tol = RTOL["bf16"] * (want.abs() + want.square().mean().sqrt())
        bad = int(((got.float() - want).abs() > tol).sum())
        assert bad == 0, f"{what}: {bad} elements away from today's arm"

    lines = []
    for shape in a.shapes.split(","):
        tokens, hidden, experts, top_k = SHAPES[shape]
        n = tokens * top_k
        rows = ops.moe_rows_bound(n, experts)
        top = torch.randint(0, experts, (tokens, top_k), generator=gen,
                            device="cuda")
        route = ops.moe_route(top, experts, rows)
        x = torch.randn(tokens, hidden, generator=gen, device="cuda").to(dt)
        y = torch.randn(rows, hidden, generator=gen, device="cuda").to(dt)
        dout = torch.randn(tokens, hidden, generator=gen, device="cuda").to(dt)
        w = torch.rand(tokens, top_k, generator=gen, device="cuda").to(dt)
        row_of = route.row_of.long()
        token_of = torch.arange(n, device="cuda") // top_k
        xp, out = torch.empty_like(y), torch.empty_like(x)
        dw = torch.empty_like(w)

        def gather_today():
            o = torch.zeros(rows, hidden, dtype=dt, device="cuda")
            return o.index_copy_(0, row_of, x.index_select(0, token_of))

        def gather_lib():
            sp.PaddedGather(x, route.indices, route.bins, route.padded_bins,
                            xp, top_k)
            return xp

        def scatter_today():
            picked = y.index_select(0, row_of) * w.view(-1, 1)
            return picked.view(tokens, top_k, hidden).sum(1)

        def scatter_lib():
            sp.PaddedScatter(y, route.row_of, out, top_k, weights=w)
            return out

        def wgrad_today():
            return (dout.index_select(0, token_of)
                    * y.index_select(0, row_of)).sum(-1).view(tokens, top_k)

        def wgrad_lib():
            sp.PaddedScatterWeightGrad(dout, y, route.row_of, dw, top_k)
            return dw

        row_bytes = 2 * hidden
        kernels = {
            "gather": (gather_today, gather_lib, (n + rows) * row_bytes),
            "scatter": (scatter_today, scatter_lib, (n + tokens) * row_bytes),
            "wgrad": (wgrad_today, wgrad_lib, (n + tokens) * row_bytes),
        }
        assert torch.equal(gather_today().view(torch.int16),
                           gather_lib().view(torch.int16)), shape
        close(scatter_lib(), scatter_today(), f"{shape} scatter")
        close(wgrad_lib(), wgrad_today(), f"{shape} wgrad")
        torch.cuda.synchronize()

        rec = {"shape": shape, "dtype": "bf16", "tokens": tokens,
               "hidden": hidden, "experts": experts, "top_k": top_k,
               "rows": rows, "calls": a.calls, "rounds": a.rounds,
               "build": sp.build_hash()}
        for kernel, (today, lib, nbytes) in kernels.items():
            arms = {"today_a": today, "lib": lib, "today_b": today}
            for fn in arms.values():
                spent = 0.0
                while spent < a.warm_ms * 1e3:
                    spent += window(fn, 5) * 5
            ts = {k: [] for k in arms}
            for _ in range(a.rounds):
                for k, fn in arms.items():
                    torch.cuda.synchronize()
                    ts[k].append(window(fn, a.calls))
            med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
            base = (med["today_a"] + med["today_b"]) / 2
            r = {"bytes": nbytes}
            for k, v in ts.items():
                tbs = nbytes / med[k] / 1e6
                r[k] = {"us": round(med[k], 1), "min": round(min(v), 1),
                        "max": round(max(v), 1), "tb_s": round(tbs, 2),
                        "hbm_share_pct": round(100 * tbs / HBM_TBS, 1)}
            r["spread_pct"] = round(
                100 * abs(med["today_a"] - med["today_b"]) / base, 2)
            r["lib_vs_today_pct"] = round(100 * (med["lib"] - base) / base, 2)
            rec[kernel] = r
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
        del x, y, dout, xp, out, kernels
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
