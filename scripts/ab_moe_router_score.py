"""Same-process A/B of the sigmoid-score router kernels (RouterScoreTopK,
RouterScoreTopKGrad; sputnik/block/router.h) against the torch formulation of
the DeepSeek-V3 gate a caller has today. Protocol of scripts/ab_moe_router.py:
one process, every arm warmed for at least --warm-ms of device time, then
--rounds interleaved rounds of --calls back-to-back calls; medians and ranges.
Today's path is timed as two arms (today_a, today_b): their difference is the
in-process spread against which the library arm is read. No ratio is expected
in advance.

Arms (bf16 logits, fp32 bias, bf16 weights, renormalised, scale 2.5):
    fwd      today: sigmoid(logits.float()) + bias -> view into groups ->
             topk(2).sum -> topk over the groups -> mask -> topk -> gather ->
             / sum -> * scale -> .to(bf16), ids .to(int32);
             lib: one RouterScoreTopK; softmax: one RouterTopK at the same E
             and top_k, the yardstick for what sigmoid, bias and the group
             step cost
    fwd_bwd  today: the same under autograd plus .backward(dweights);
             lib: RouterScoreTopK + RouterScoreTopKGrad;
             softmax: RouterTopK + RouterTopKGrad

The logits are uniform in [-6, 6] rounded to bf16, the bias uniform in
[-0.5, 0.5]. A row in which, in float64, two neighbouring group scores or two
neighbours among the k + 1 largest eligible selection values are less than
2^-14 apart is replaced by a row that is clear, so that torch.topk (tie order
unspecified, its own fp32 rounding) and RouterScoreTopK must pick the same
experts. Compared before timing: ids exactly, weights and dlogits within
tests/helpers.RTOL.

Shapes: v3 32768 tokens, 256 experts, 8 groups, 4 eligible, top_k 8;
e64_k6 32768 tokens, 64 experts, no groups, top_k 6. One JSON line per shape.

python scripts/ab_moe_router_score.py [--shapes v3,e64_k6] [--out profiles/moe_router_score/ab_moe_router_score.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALL = "v3,e64_k6"
# tokens, experts, top_k, num_groups, topk_groups
SHAPES = {"v3": (32768, 256, 8, 8, 4), "e64_k6": (32768, 64, 6, 1, 1)}
SCALE = 2.5
GAP = 2.0 ** -14


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
    from tests.helpers import RTOL

    assert torch.cuda.is_available(), "needs a GPU: there is no CPU timing"
    gen = torch.Generator(device="cuda").manual_seed(31)
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
        tokens, experts, top_k, groups, top_groups = SHAPES[shape]
        gs = experts // groups
        bias = torch.rand(experts, generator=gen, device="cuda") - 0.5

        def gate(l, ft=torch.float32):
            """(weights, ids, the smallest gap of a decision) in `ft`."""
            s = l.to(ft).sigmoid()
            c = s + bias.to(ft)
            gap = torch.full((tokens,), float("inf"), dtype=ft,
                             device="cuda")
            if groups > 1:
                group = c.view(tokens, groups, gs).topk(2, dim=-1)[0].sum(-1)
                best = group.topk(top_groups, dim=-1)[1]
                on = torch.zeros_like(group, dtype=torch.bool).scatter_(
                    1, best, True)
                mask = on.unsqueeze(-1).expand(tokens, groups, gs).reshape(
                    tokens, experts)
                c = c.masked_fill(~mask, float("-inf"))
                if ft == torch.float64:
                    srt = group.sort(dim=-1, descending=True)[0]
                    gap = (srt[:, :-1] - srt[:, 1:]).min(dim=-1)[0]
            if ft == torch.float64:
                srt = c.topk(top_k + 1, dim=-1)[0]
                gap = torch.minimum(
                    gap, (srt[:, :-1] - srt[:, 1:]).min(dim=-1)[0])
            idx = c.topk(top_k, dim=-1)[1]
            wt = s.gather(1, idx)
            wt = wt / wt.sum(dim=-1, keepdim=True) * SCALE
            return wt, idx, gap

        logits = ((torch.rand(tokens, experts, generator=gen, device="cuda")
                   - 0.5) * 12.0).to(dt).contiguous()
        clear = gate(logits, torch.float64)[2] >= GAP
        replaced = int((~clear).sum())
        assert replaced < tokens // 2, f"{shape}: {replaced} rows not clear"
        good = clear.nonzero().flatten()
        logits[~clear] = logits[good[:replaced]]
        assert bool((gate(logits, torch.float64)[2] >= GAP).all())

        dweights = torch.randn(tokens, top_k, generator=gen,
                               device="cuda").to(dt)
        top = torch.empty(tokens, top_k, dtype=torch.int32, device="cuda")
        top_soft = torch.empty_like(top)
        w = torch.empty(tokens, top_k, dtype=dt, device="cuda")
        dlogits = torch.empty_like(logits)

        def fwd_today():
            wt, idx, _ = gate(logits)
            return wt.to(dt), idx.to(torch.int32)

        def fwd_lib():
            sp.RouterScoreTopK(logits, top, w, bias, groups, top_groups, True,
                               SCALE)
            return w, top

        def fwd_softmax():
            sp.RouterTopK(logits, top_soft, w, True)

        def fwd_bwd_today():
            l = logits.detach().requires_grad_(True)
            wt = gate(l)[0].to(dt)
            wt.backward(dweights)
            return l.grad

        def fwd_bwd_lib():
            sp.RouterScoreTopK(logits, top, w, bias, groups, top_groups, True,
                               SCALE)
            sp.RouterScoreTopKGrad(logits, top, dweights, dlogits, True,
                                   SCALE)
            return dlogits

        def fwd_bwd_softmax():
            sp.RouterTopK(logits, top_soft, w, True)
            sp.RouterTopKGrad(logits, top_soft, dweights, dlogits, True)

        w_today, top_today = fwd_today()
        fwd_lib()
        assert torch.equal(top, top_today), f"{shape}: picks differ"
        assert torch.equal(top.long(), gate(logits, torch.float64)[1])
        close(w, w_today, f"{shape} weights")
        close(fwd_bwd_lib().clone(), fwd_bwd_today(), f"{shape} dlogits")
        torch.cuda.synchronize()

        rec = {"shape": shape, "dtype": "bf16", "tokens": tokens,
               "experts": experts, "top_k": top_k, "num_groups": groups,
               "topk_groups": top_groups, "normalize": True, "scale": SCALE,
               "rows_replaced": replaced, "calls": a.calls,
               "rounds": a.rounds, "build": sp.build_hash()}
        kernels = {"fwd": (fwd_today, fwd_lib, fwd_softmax),
                   "fwd_bwd": (fwd_bwd_today, fwd_bwd_lib, fwd_bwd_softmax)}
        for kernel, (old, lib, soft) in kernels.items():
            arms = {"today_a": old, "lib": lib, "softmax": soft,
                    "today_b": old}
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
            r["lib_vs_softmax_pct"] = round(
                100 * (med["lib"] - med["softmax"]) / med["softmax"], 2)
            rec[kernel] = r
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
