"""Same-process A/B of gradient accumulation into a weight-sized sink: what a
caller does without the accumulating products (a plain MatmulEx into a
preallocated temporary, then sink.add_(tmp)) against MatmulAccumulateEx into
the sink. Protocol of scripts/ab_bt_workspace.py: one process, every arm
warmed for at least --warm-ms of device time, then --rounds interleaved
rounds of --calls back-to-back calls; medians. The baseline is timed as two
arms (baseline_a, baseline_b): their difference is the in-process spread
against which the fused arm is read.

Shapes: the two weight-gradient products of BASELINE config 4 (bf16, 8
experts, 8192 tokens, d_model 4096, d_ff 14336) —
    dds_tn  dw1 = x^T [4096 x 8192] . dh [8192 x 114688, expert topology]
    dsd_tn  dw2 = h^T . dy [8192 x 4096]
— and dsd_tn_4096 (f16, 4096^3 at 50%), where the plain arm runs the 4-wave
kernel. Sink types: the operand type and fp32.

Operands are integers in {-1, 0, 1}, the dense one zero unless k % 4 == 0
(config 4: at most 256 nonzero terms per sum, exact in bf16) or k % 2 == 0
(4096^3: at most 2048, exact in f16), and the sinks start from integers in
[-8, 8]: with an fp32 sink both arms must then agree exactly. With a sink of
the operand type each arm rounds differently (the baseline twice), and they
agree within tests/helpers.RTOL. One JSON line per (shape, sink type).

python scripts/ab_accumulate.py [--shapes dds_tn,dsd_tn,dsd_tn_4096]
                                [--out profiles/accumulate/ab_accumulate.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="dds_tn,dsd_tn,dsd_tn_4096")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warm-ms", type=float, default=100.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    import sputnik_amd as sp
    from sputnik_amd import matrix_utils as mu
    from tests.helpers import RTOL

    assert torch.cuda.is_available(), "needs a GPU: there is no CPU timing"
    gen = torch.Generator(device="cuda").manual_seed(7)

    def ints(rows, cols, dt, k_axis, k_step):
        t = torch.randint(-1, 2, (rows, cols), generator=gen, device="cuda",
                          dtype=torch.int8).to(dt)
        keep = torch.arange(t.shape[k_axis], device="cuda") % k_step == 0
        return t * (keep[:, None] if k_axis == 0 else keep[None, :]).to(dt)

    def sparse(rows, cols, off, idx, dt):
        nb = int(off[-1])
        data = torch.randint(-1, 2, (nb, 128, 128), generator=gen,
                             device="cuda", dtype=torch.int8).to(dt)
        s = sp.BlockMatrix(rows, cols, 128, nb * 128 * 128, data,
                           torch.from_numpy(off.astype(np.int32)).cuda(),
                           torch.from_numpy(idx.astype(np.int16)).cuda())
        sp.AllocateTransposeBuffers(s)
        sp.Transpose(s)
        return s

    def window(fn, calls):
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(calls):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / calls  # us per call

    def problem(shape):
        """(dtype name, a, ta, b, tb, output rows, cols, flops)"""
        if shape in ("dds_tn", "dsd_tn"):
            dt, tokens, dm, cols = torch.bfloat16, 8192, 4096, 8 * 14336
            off, idx = mu.expert_block_diagonal(8, tokens // 8 // 128,
                                                14336 // 128)
            h = sparse(tokens, cols, off, idx, dt)
            flops = 2.0 * int(off[-1]) * 128 * 128 * dm
            if shape == "dds_tn":  # x stored [tokens x d_model], k = tokens
                x = sp.Matrix(tokens, dm, ints(tokens, dm, dt, 0, 4))
                return "bf16", x, True, h, False, dm, cols, flops
            dy = sp.Matrix(tokens, dm, ints(tokens, dm, dt, 0, 4))
            return "bf16", h, True, dy, False, cols, dm, flops
        assert shape == "dsd_tn_4096", shape
        d, dt = 4096, torch.float16
        rng = np.random.default_rng(1)
        nb = mu.nonzeros_for_density(d, d, 0.5) // (128 * 128)
        off, idx = mu.random_topology(d // 128, d // 128, nb, rng)
        s = sparse(d, d, off, idx, dt)
        b = sp.Matrix(d, d, ints(d, d, dt, 0, 2))
        return "f16", s, True, b, False, d, d, 2.0 * nb * 128 * 128 * d

    lines = []
    for shape in a.shapes.split(","):
        name, A, ta, Bm, tb, rows, cols, flops = problem(shape)
        dt = {"f16": torch.float16, "bf16": torch.bfloat16}[name]
        tmp = torch.empty(rows, cols, dtype=dt, device="cuda")
        T = sp.Matrix(rows, cols, tmp)
        # kernel of the plain arm (dsd_plan / dds_plan: 1 = the 4-wave kernel)
        plan = (sp.dsd_plan if isinstance(A, sp.BlockMatrix)
                else sp.dds_plan)(A, ta, Bm, tb, T)
        for sink_dt in (dt, torch.float32):
            sink0 = torch.randint(-8, 9, (rows, cols), generator=gen,
                                  device="cuda", dtype=torch.int8).to(sink_dt)
            sink = sink0.clone()
            S = sp.Matrix(rows, cols, sink)

            def baseline():
                sp.MatmulEx(A, ta, Bm, tb, T)
                sink.add_(tmp)

            def fused():
                sp.MatmulAccumulateEx(A, ta, Bm, tb, S)

            # one call of each arm from the same start: the arms agree
            baseline()
            want = sink.clone()
            sink.copy_(sink0)
            fused()
            torch.cuda.synchronize()
            if sink_dt == torch.float32:
                assert torch.equal(sink, want), f"{shape}: fp32 sinks differ"
            else:
                ref = want.float()
                tol = RTOL[name] * (ref.abs() + ref.square().mean().sqrt())
                bad = int(((sink.float() - ref).abs() > tol).sum())
                assert bad == 0, f"{shape}: {bad} elements out of tolerance"
            del want
            arms = {"baseline_a": baseline, "fused": fused,
                    "baseline_b": baseline}
            for fn in arms.values():
                spent = 0.0
                while spent < a.warm_ms * 1e3:
                    spent += window(fn, 10) * 10
                sink.copy_(sink0)  # (values stay small: no overflow to inf)
            ts = {k: [] for k in arms}
            for _ in range(a.rounds):
                for k, fn in arms.items():
                    sink.copy_(sink0)
                    torch.cuda.synchronize()
                    ts[k].append(window(fn, a.calls))
            med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
            base = (med["baseline_a"] + med["baseline_b"]) / 2
            out = {"shape": shape, "dtype": name,
                   "sink": "f32" if sink_dt == torch.float32 else name,
                   "out_shape": [rows, cols], "plain_plan": int(plan),
                   "calls": a.calls, "rounds": a.rounds,
                   "build": sp.build_hash()}
            for k, v in ts.items():
                out[k] = {"us": round(med[k], 1), "min": round(min(v), 1),
                          "max": round(max(v), 1),
                          "tflops": round(flops / med[k] / 1e6, 1)}
            out["spread_pct"] = round(
                100 * abs(med["baseline_a"] - med["baseline_b"]) / base, 2)
            out["fused_vs_baseline_pct"] = round(
                100 * (med["fused"] - base) / base, 2)
            print(json.dumps(out), flush=True)
            lines.append(json.dumps(out))
            del sink, sink0
        del tmp
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
