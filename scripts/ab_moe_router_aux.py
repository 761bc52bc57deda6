"""Same-process A/B of the router's auxiliary losses: the statistics taken in
the router's own pass (ops.moe_router_aux + ops.load_balancing_loss +
ops.router_z_loss) against what a caller has today (ops.moe_router with
return_scores, the two losses formed in torch). Protocol of
scripts/ab_moe_router.py: one process, every arm warmed for at least
--warm-ms of device time, then --rounds interleaved rounds of --calls
back-to-back calls; medians and ranges. Today's path is timed as two arms
(today_a, today_b): their difference is the in-process spread against which
the fused arm is read. No ratio is expected in advance.

One call of an arm is a training step's router: forward, both losses, and
backward through the expert weights' gradient and the losses together (bf16
logits, bf16 weights, renormalised, fixed tokens_per_expert):
    today  moe_router(return_scores=True); lb = E / (tokens k) sum_e tpe_e
           mean_t scores_te from the bf16 scores in fp32; z = mean_t
           logsumexp(logits.float())^2; backward
    fused  moe_router_aux; load_balancing_loss(score_sums, tpe) +
           router_z_loss(z_sum); backward

Checked before timing: ids and weights equal bit for bit; the fused arm's
loss and dlogits within the bounds of tests/router_aux_ref.py of a float64
reference; today's arm within tests/helpers.RTOL of it (its load-balancing
loss is formed from rounded scores, so those bounds are not its own). Per
shape: microseconds, device launches per call (torch.profiler, null where
that does not work) and the peak of torch.cuda.max_memory_allocated over one
call, above what was allocated before it.

Shapes of profiles/moe_router/README.md: c4_k2 8192 tokens, 8 experts, top_k
2; e64_k8 and e256_k8 32768 tokens, 64 / 256 experts, top_k 8. One JSON line
per shape.

python scripts/ab_moe_router_aux.py [--shapes c4_k2,...] [--out profiles/moe_router_aux/ab_moe_router_aux.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALL = "c4_k2,e64_k8,e256_k8"
SHAPES = {"c4_k2": (8192, 8, 2), "e64_k8": (32768, 64, 8),
          "e256_k8": (32768, 256, 8)}
LB_WEIGHT, Z_WEIGHT = 0.01, 0.001


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=ALL)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warm-ms", type=float, default=100.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    import sputnik_amd as sp
    from sputnik_amd import ops
    from tests import router_aux_ref as A
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

    def launches(fn):
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

    def peak(fn):
        fn()
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        top = torch.cuda.max_memory_allocated()
        del out
        return top - before

    lines = []
    for shape in a.shapes.split(","):
        tokens, experts, top_k = SHAPES[shape]
        logits = ((torch.rand(tokens, experts, generator=gen, device="cuda")
                   - 0.5) * 16).to(dt).contiguous()
        dweights = torch.randn(tokens, top_k, generator=gen,
                               device="cuda").to(dt)
        _, top0 = ops.moe_router(logits, top_k, True)
        tpe = torch.bincount(top0.reshape(-1).long(),
                             minlength=experts).to(torch.int32)
        tpe_f = tpe.float()
        lb_scale = LB_WEIGHT * experts / (tokens * top_k)

        def today():
            l = logits.detach().requires_grad_(True)
            w, top, scores = ops.moe_router(l, top_k, True, None, True)
            lb = lb_scale * torch.dot(tpe_f, scores.float().mean(0))
            z = Z_WEIGHT * torch.logsumexp(l.float(), -1).square().mean()
            loss = lb + z
            torch.autograd.backward([w, loss], [dweights, None])
            return w, top, loss.detach(), l.grad

        def fused():
            l = logits.detach().requires_grad_(True)
            w, top, sums, zs = ops.moe_router_aux(l, top_k, True)
            loss = (ops.load_balancing_loss(sums, tpe, tokens, top_k,
                                            LB_WEIGHT)
                    + ops.router_z_loss(zs, tokens, Z_WEIGHT))
            torch.autograd.backward([w, loss], [dweights, None])
            return w, top, loss.detach(), l.grad

        w_t, top_t, loss_t, g_t = today()
        w_f, top_f, loss_f, g_f = fused()
        assert torch.equal(top_t, top_f), f"{shape}: picks differ"
        assert torch.equal(w_t, w_f), f"{shape}: weights differ"
        l64 = logits.float().cpu().numpy()
        sums_ref, z_ref, m, lse = A.stats64(l64)
        counts = tpe.cpu().numpy().astype(np.float64)
        dss = lb_scale / tokens * counts
        dz = np.array([Z_WEIGHT / tokens])
        loss_ref = float(dss @ sums_ref + dz[0] * z_ref)
        bound = (float(dss @ A.score_sums_bound(sums_ref, tokens, experts))
                 + dz[0] * A.z_sum_bound(z_ref, m, lse, experts)
                 + (experts + 4) * A.U * abs(loss_ref))
        assert abs(float(loss_f) - loss_ref) <= bound, (
            shape, float(loss_f), loss_ref, bound)
        assert abs(float(loss_t) - loss_ref) <= RTOL["bf16"] * abs(loss_ref), (
            shape, float(loss_t), loss_ref)
        ref, image = A.grad64(l64, top_f.cpu().numpy(),
                              dweights.float().cpu().numpy(), None, dss, dz,
                              True)
        err = np.abs(g_f.float().cpu().numpy().astype(np.float64) - ref)
        assert (err <= A.grad_bound(ref, image, experts, top_k,
                                    "bf16")).all(), f"{shape}: dlogits"
        want = torch.from_numpy(ref).float().cuda()
        tol = RTOL["bf16"] * (want.abs() + want.square().mean().sqrt())
        bad = int(((g_t.float() - want).abs() > tol).sum())
        assert bad == 0, f"{shape}: today's dlogits, {bad} elements away"
        del ref, image, err, want, tol, l64
        torch.cuda.synchronize()

        rec = {"shape": shape, "dtype": "bf16", "tokens": tokens,
               "experts": experts, "top_k": top_k, "calls": a.calls,
               "rounds": a.rounds, "build": sp.build_hash(),
               "loss": {"today": float(loss_t), "fused": float(loss_f),
                        "float64": loss_ref}}
        arms = {"today_a": today, "fused": fused, "today_b": today}
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
        for k, v in ts.items():
            rec[k] = {"us": round(med[k], 1), "min": round(min(v), 1),
                      "max": round(max(v), 1)}
        rec["spread_pct"] = round(
            100 * abs(med["today_a"] - med["today_b"]) / base, 2)
        rec["fused_vs_today_pct"] = round(
            100 * (med["fused"] - base) / base, 2)
        rec["launches"] = {"today": launches(today), "fused": launches(fused)}
        rec["peak_bytes"] = {"today": peak(today), "fused": peak(fused)}
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
