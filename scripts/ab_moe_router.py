"""Same-process A/B of the MoE router kernels (RouterTopK, RouterTopKGrad,
MoeSort; sputnik/block/router.h) against the torch formulation a caller has
today. Protocol of scripts/ab_moe_permute.py: one process, every arm warmed
for at least --warm-ms of device time, then --rounds interleaved rounds of
--calls back-to-back calls; medians and ranges. Today's path is timed as two
arms (today_a, today_b): their difference is the in-process spread against
which the library arm is read. No ratio is expected in advance.

Arms (bf16 logits, bf16 weights, renormalised where top_k > 1: at top_k = 1
the renormalised weight is the constant 1 and its gradient rounding noise):
    fwd      today: softmax(logits.float()) -> topk -> / sum -> .to(bf16),
             ids .to(int32); lib: one RouterTopK
    fwd_bwd  today: the same under autograd plus .backward(dweights);
             lib: RouterTopK + RouterTopKGrad
    route    today: ops.moe_route(top int64) = torch.sort(stable) + two
             conversions + MoeBins + MoeRowMap; lib: ops.moe_device_route(top
             int32) = one MoeSort (three launches); both allocate
             their outputs per call, rows = moe_rows_bound (no host sync)

The logits of a row are a random permutation of E distinct multiples of 1/16,
so that torch.topk (on probabilities, tie order unspecified) and RouterTopK
(on logits) must pick the same experts. Compared before timing: ids and every
routing tensor exactly, weights within tests/helpers.RTOL, dlogits likewise.
With --launches the device launches per call are counted with torch.profiler
(null where that does not work).

Shapes: c4_k1 / c4_k2 8192 tokens, 8 experts, top_k 1 / 2 (BASELINE config
4's); e64_k8 and e256_k8 32768 tokens, 64 / 256 experts, top_k 8. One JSON
line per shape.

python scripts/ab_moe_router.py [--shapes c4_k1,...] [--out profiles/moe_router/ab_moe_router.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALL = "c4_k1,c4_k2,e64_k8,e256_k8"
SHAPES = {"c4_k1": (8192, 8, 1), "c4_k2": (8192, 8, 2),
          "e64_k8": (32768, 64, 8), "e256_k8": (32768, 256, 8)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=ALL)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warm-ms", type=float, default=100.0)
    ap.add_argument("--out", default="")
    ap.add_argument("--launches", action="store_true",
                    help="also count device launches per call with "
                         "torch.profiler")
    a = ap.parse_args()
    import torch
    import sputnik_amd as sp
    from sputnik_amd import ops
    from tests.helpers import RTOL

    assert torch.cuda.is_available(), "needs a GPU: there is no CPU timing"
    gen = torch.Generator(device="cuda").manual_seed(29)
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

    def launches(fn):
        if not a.launches:
            return None
        try:
            from torch.profiler import ProfilerActivity, profile
            fn()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            n = sum(1 for ev in prof.events()
                    if str(ev.device_type).endswith("CUDA"))
            return n or None
        except Exception:
            return None

    lines = []
    for shape in a.shapes.split(","):
        tokens, experts, top_k = SHAPES[shape]
        n = tokens * top_k
        norm = top_k > 1
        rows = ops.moe_rows_bound(n, experts)
        values = (torch.arange(experts, device="cuda") - experts // 2) / 16.0
        order = torch.rand(tokens, experts, generator=gen,
                           device="cuda").argsort(1)
        logits = values[order].to(dt).contiguous()
        dweights = torch.randn(tokens, top_k, generator=gen,
                               device="cuda").to(dt)
        top = torch.empty(tokens, top_k, dtype=torch.int32, device="cuda")
        w = torch.empty(tokens, top_k, dtype=dt, device="cuda")
        dlogits = torch.empty_like(logits)

        def today(l):
            p = torch.softmax(l.float(), dim=-1)
            wt, idx = torch.topk(p, top_k, dim=-1)
            if norm:
                wt = wt / wt.sum(dim=-1, keepdim=True)
            return wt.to(dt), idx.to(torch.int32), idx

        def fwd_today():
            return today(logits)

        def fwd_lib():
            sp.RouterTopK(logits, top, w, norm)
            return w, top

        def fwd_bwd_today():
            l = logits.detach().requires_grad_(True)
            wt, _, _ = today(l)
            wt.backward(dweights)
            return l.grad

        def fwd_bwd_lib():
            sp.RouterTopK(logits, top, w, norm)
            sp.RouterTopKGrad(logits, top, dweights, dlogits, norm)
            return dlogits

        w_today, top_today, top64 = fwd_today()
        fwd_lib()
        assert torch.equal(top, top_today), f"{shape}: picks differ"
        close(w, w_today, f"{shape} weights")
        close(fwd_bwd_lib(), fwd_bwd_today(), f"{shape} dlogits")
        top32 = top.clone()

        def route_today():
            return ops.moe_route(top64, experts, rows)

        def route_lib():
            return ops.moe_device_route(top32, experts, rows)

        ra, rb = route_today(), route_lib()
        for name in ("indices", "bin_ids", "bins", "padded_bins",
                     "tokens_per_expert", "row_of"):
            assert torch.equal(getattr(ra, name), getattr(rb, name)), (
                shape, name)
        torch.cuda.synchronize()

        rec = {"shape": shape, "dtype": "bf16", "tokens": tokens,
               "experts": experts, "top_k": top_k, "normalize": norm,
               "rows": rows,
               "calls": a.calls, "rounds": a.rounds,
               "build": sp.build_hash()}
        kernels = {"fwd": (fwd_today, fwd_lib),
                   "fwd_bwd": (fwd_bwd_today, fwd_bwd_lib),
                   "route": (route_today, route_lib)}
        for kernel, (old, lib) in kernels.items():
            arms = {"today_a": old, "lib": lib, "today_b": old}
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
            r = {}
            for k, v in ts.items():
                r[k] = {"us": round(med[k], 1), "min": round(min(v), 1),
                        "max": round(max(v), 1)}
            r["spread_pct"] = round(
                100 * abs(med["today_a"] - med["today_b"]) / base, 2)
            r["lib_vs_today_pct"] = round(100 * (med["lib"] - base) / base, 2)
            r["launches"] = {"today": launches(old), "lib": launches(lib)}
            rec[kernel] = r
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
