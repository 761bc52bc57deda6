"""Same-process timing of the fp8 forward path (sputnik/block/fp8.h) against
the 16-bit SDD and DSD it stands beside: sdd_fp8, dsd_fp8 and the two hot
quantisers (quantize_rows of the gathered activations, quantize_sparse with
gelu of the SDD output) next to ops' raw bf16 sdd and dsd on the same
topology, and the two products in the opt-in fast accumulation
(accumulate="fast", Fp8Accumulate::kFast). With --parent-lib the fp32-mode
products of another build of libsputnik.so (the commit before a change) run
as two more arms of the same process and rounds, through the same Python
path. Recorded, not gated (DESIGN "FP8 forward path").

With --backward the arms are those of the backward pass instead (DESIGN "FP8
backward path"): quantize_tiles of dY and quantize_blocks with the
activation gradient (both axes each), dsd_fp8_wgrad in both modes next to the
16-bit H^T dY (ops' raw dsd of the transposed view), and the whole backward
of ops.mlp_fp8 in both modes next to that of the 16-bit ops.mlp, each as
torch.autograd.grad over a retained graph, so that only backward is timed.
ops.mlp's code is the parent commit's, so it is the baseline as it stands.

With --mx the arms are those of the MX path (sputnik/block/mx.h, DESIGN "MX
forward path"): sdd_mx and dsd_mx for MXFP8 and MXFP4 weights and
quantize_rows_mx, beside the bf16 products and the fast fp8 products; with
--parent-lib the fast fp8 products of that build run as *_parent arms.

With --mx --backward the arms are those of the MX backward pass (DESIGN "MX
backward path"): quantize_tiles_mx of dY and QuantizeBlocksMx with the gelu
gradient (both axes each), dsd_mx_wgrad next to the 16-bit H^T dY and the fast
dsd_fp8_wgrad, and the whole backward of ops.mlp_mx next to ops.mlp's and
ops.mlp_fp8's (both modes). The bf16 and fp8 arms are the parent commit's
code.

With --glu the arms are those of the gated expert's backward pass (DESIGN
"FP8 GLU backward path"): QuantizeBlocksGatedGrad with all four pairs next to
the composed route (BlockGateGrad, then QuantizeBlocks on each of its two
outputs), dsd_fp8_pair next to two dsd_fp8 and a torch add, and the whole
backward of ops.glu_mlp_fp8 in both modes next to that of the 16-bit
ops.glu_mlp. The 16-bit backward writes dU over its saved U and refuses a
second run, so its arm clears that mark before each call: from the second
call on it differentiates through dU in U's place, which moves the values and
not the work.

With --mx --glu --backward the same arms are the MX path's (DESIGN "MX GLU
backward path"): QuantizeBlocksMxGatedGrad next to BlockGateGrad and two
QuantizeBlocksMx, dsd_mx_pair next to two dsd_mx and a torch add, and the
whole backward of ops.glu_mlp_mx next to those of ops.glu_mlp and of
ops.glu_mlp_fp8 in the fast mode.

With --mx --gated the arms are those of the gated expert's first product in
the MX forward path (DESIGN "MX forward path"), per weight format:
glu_chain_*, the three launches sdd_mx, sdd_mx and quantize_sparse_mx with the
gate, next to glu_fused_*, ops.sdd_mx_gated over the same operands.

With --mx --fp4 the arms are those of the MXFP4-activation path (DESIGN "MX
forward path", A4W4): sdd_mx_fp4 and dsd_mx_fp4 next to sdd_mx and dsd_mx
with the same MXFP4 weights (the route those weights took before), and
quantize_rows_mx_fp4 next to quantize_rows_mx.

Protocol: one process, HIP events, every arm warmed for at
least --warm-ms of device time, then --rounds interleaved rounds, each window
long enough to hold at least --load-ms of back-to-back calls; medians and
ranges over the rounds.

Shapes (bf16 outputs, 8 experts, d_model 4096, d_ff 14336, every expert with
the same number of rows, the dMoE topology of ops.expert_topology):
    c4      BASELINE config 4: 8192 rows (1024 per expert), 7168 blocks
    decode  128 rows per expert (1024 rows, 896 blocks): the weights, 0.94 GB
            each in bf16, dominate the traffic

Per arm: microseconds, TFLOP/s from 2 * blocks * 128 * 128 * K for the
products, and for the quantisers the achieved bytes per second (2 bytes read,
1 written per element, 4 per scale) as a share of the 6.3 TB/s achievable HBM
rate. One JSON line per shape.

python scripts/bench_fp8.py [--shapes c4,decode] [--parent-lib PATH]
                            [--out profiles/fp8/bench_fp8.jsonl]
python scripts/bench_fp8.py --mx [--parent-lib PATH]
                            [--out profiles/mx/bench_mx.jsonl]
python scripts/bench_fp8.py --mx --gated
                            [--out profiles/mx/bench_mx_gated.jsonl]
python scripts/bench_fp8.py --mx --fp4
                            [--out profiles/mx/bench_mx_fp4.jsonl]
python scripts/bench_fp8.py --mx --backward
                            [--out profiles/mx/bench_mx_grad.jsonl]
python scripts/bench_fp8.py --glu [--out profiles/fp8/bench_fp8_glu.jsonl]
python scripts/bench_fp8.py --mx --glu --backward
                            [--out profiles/mx/bench_mx_glu.jsonl]
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EXPERTS, D_MODEL, D_FF = 8, 4096, 14336
SHAPES = {"c4": 1024, "decode": 128}  # rows per expert
HBM_TBS = 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c4,decode")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warm-ms", type=float, default=100.0)
    ap.add_argument("--load-ms", type=float, default=100.0)
    ap.add_argument("--parent-lib", default="",
                    help="another libsputnik.so: its sdd_fp8 / dsd_fp8 run as "
                         "the *_parent arms")
    ap.add_argument("--backward", action="store_true",
                    help="time the backward pass instead of the forward one")
    ap.add_argument("--mx", action="store_true",
                    help="time the MX products beside bf16 and fast fp8")
    ap.add_argument("--glu", action="store_true",
                    help="time the gated expert's backward pass")
    ap.add_argument("--gated", action="store_true",
                    help="with --mx: time the fused gated SDD next to its "
                         "three-launch chain")
    ap.add_argument("--fp4", action="store_true",
                    help="with --mx: time the MXFP4-activation products and "
                         "quantiser next to the MXFP8-activation ones")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import sputnik_amd as sp
    from sputnik_amd import ops

    assert torch.cuda.is_available(), "needs a GPU: there is no CPU timing"
    gen = torch.Generator(device="cuda").manual_seed(29)
    dt = torch.bfloat16
    hidden = EXPERTS * D_FF

    def rand(*shape, scale=1.0):
        return (torch.randn(*shape, generator=gen, device="cuda",
                            dtype=torch.float32) * scale).to(dt)

    def window(fn, calls):
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(calls):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / calls  # us per call

    w1, w2 = rand(D_MODEL, hidden, scale=1 / 64), rand(hidden, D_MODEL,
                                                        scale=1 / 64)
    w1q, w2q = ops.quantize_weight(w1), ops.quantize_weight(w2)
    sp.lib()
    parent = None
    if a.parent_lib:
        # (a second copy of the library in this process: its own kernels,
        # the same HIP runtime)
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
        for name in ("sputnik_sdd_fp8", "sputnik_dsd_fp8",
                     "sputnik_sdd_fp8_acc", "sputnik_dsd_fp8_acc"):
            fn = getattr(parent, name)
            fn.argtypes, fn.restype = sp._SIGNATURES[name], ctypes.c_int
        parent.sputnik_build_hash.restype = ctypes.c_char_p

    def through_parent(fn):
        def run():
            ours, sp._lib = sp._lib, parent
            try:
                return fn()
            finally:
                sp._lib = ours
        return run

    lines = []
    for shape in a.shapes.split(","):
        per_expert = SHAPES[shape]
        rows = EXPERTS * per_expert
        padded_bins = torch.arange(1, EXPERTS + 1, dtype=torch.int32,
                                   device="cuda") * per_expert
        topo = ops.expert_topology(padded_bins, D_FF // 128, rows // 128,
                                   dtype=dt)
        blocks = topo.nnz_blocks
        x = rand(rows, D_MODEL)
        xq, xs = ops.quantize_rows(x)
        g16 = topo.with_data(ops._sdd(x, w1, topo))
        h16 = g16.with_data(sp.BlockActivation(g16.data, "gelu"))
        hq = ops.quantize_sparse(g16, "gelu")
        arms = {
            "sdd_bf16": lambda: ops._sdd(x, w1, topo),
            "sdd_fp8": lambda: ops.sdd_fp8(xq, xs, w1q, topo, dt),
            "dsd_bf16": lambda: ops._dsd(h16, w2),
            "dsd_fp8": lambda: ops.dsd_fp8(hq, w2q, dt),
            "sdd_fp8_fast": lambda: ops.sdd_fp8(xq, xs, w1q, topo, dt,
                                                accumulate="fast"),
            "dsd_fp8_fast": lambda: ops.dsd_fp8(hq, w2q, dt,
                                                accumulate="fast"),
            "quantize_rows": lambda: ops.quantize_rows(x),
            "quantize_sparse_gelu": lambda: ops.quantize_sparse(g16, "gelu"),
        }
        if parent is not None:
            arms["sdd_fp8_parent"] = through_parent(arms["sdd_fp8"])
            arms["dsd_fp8_parent"] = through_parent(arms["dsd_fp8"])
        if a.mx and not a.backward:
            mxw = {f: (ops.quantize_weight_mx(w1, format=f),
                       ops.quantize_weight_mx(w2, format=f))
                   for f in ("e4m3", "e2m1")}
            mq, ms = ops.quantize_rows_mx(x)
            hmx = ops.quantize_sparse_mx(g16, "gelu")
            fast = {k: arms[k] for k in ("sdd_fp8_fast", "dsd_fp8_fast")}
            arms = {"sdd_bf16": arms["sdd_bf16"], "dsd_bf16": arms["dsd_bf16"],
                    **fast,
                    "quantize_rows_mx": lambda: ops.quantize_rows_mx(x)}
            for f, (a1, a2) in mxw.items():
                arms[f"sdd_mx_{f}"] = (
                    lambda a1=a1: ops.sdd_mx(mq, ms, a1, topo, dt))
                arms[f"dsd_mx_{f}"] = lambda a2=a2: ops.dsd_mx(hmx, a2, dt)
            if parent is not None:
                for k, fn in fast.items():
                    arms[f"{k}_parent"] = through_parent(fn)
        if a.backward:
            dy = rand(rows, D_MODEL)
            dh16 = g16.with_data(rand(blocks, 128, 128))
            _, _, dyqt, dyst = ops.quantize_tiles(dy, rows=False)
            ht = ops.quantize_sparse_t(g16, "gelu")
            w1t = w1.t().contiguous()

            def backward_of(fn, *leaves):
                leaves = [t.detach().requires_grad_() for t in leaves]
                y = fn(*leaves)
                return lambda: torch.autograd.grad(y, leaves, dy,
                                                   retain_graph=True)

            arms = {
                "quantize_tiles": lambda: ops.quantize_tiles(dy),
                "quantize_blocks_gelu_grad": lambda: ops._lowp_quantize_blocks(
                    ops._FP8, dh16, "act_grad", 1, g16.data, True, True,
                    pow2=False),
                "wgrad_bf16": lambda: ops._dsd(h16.t(), dy),
                "wgrad_fp8": lambda: ops.dsd_fp8_wgrad(ht, dyqt, dyst,
                                                       out_dtype=dt),
                "wgrad_fp8_fast": lambda: ops.dsd_fp8_wgrad(
                    ht, dyqt, dyst, out_dtype=dt, accumulate="fast"),
                "mlp_bf16_backward": backward_of(
                    lambda x_, a_, b_: ops.mlp(x_, a_, b_, topo, "gelu"),
                    x, w1, w2),
                "mlp_fp8_backward": backward_of(
                    lambda x_, a_, b_: ops.mlp_fp8(x_, a_, b_, topo, "gelu"),
                    x, w1t, w2),
                "mlp_fp8_fast_backward": backward_of(
                    lambda x_, a_, b_: ops.mlp_fp8(x_, a_, b_, topo, "gelu",
                                                   "fast"), x, w1t, w2),
            }
        if a.backward and a.mx:
            _, _, myqt, myst = ops.quantize_tiles_mx(dy, rows=False)
            hmt = ops.quantize_sparse_mx_t(g16, "gelu")[1]
            keep = ("wgrad_bf16", "wgrad_fp8_fast", "mlp_bf16_backward",
                    "mlp_fp8_backward", "mlp_fp8_fast_backward")
            arms = {
                "quantize_tiles_mx": lambda: ops.quantize_tiles_mx(dy),
                "quantize_blocks_mx_gelu_grad":
                    lambda: ops._lowp_quantize_blocks(
                        ops._MX, dh16, "act_grad", 1, g16.data, True, True),
                "wgrad_mx": lambda: ops.dsd_mx_wgrad(hmt, myqt, myst,
                                                     out_dtype=dt),
                **{k: arms[k] for k in keep},
                "mlp_mx_backward": backward_of(
                    lambda x_, a_, b_: ops.mlp_mx(x_, a_, b_, topo, "gelu"),
                    x, w1t, w2),
            }
        if a.glu:
            dy = rand(rows, D_MODEL)
            v1 = rand(D_MODEL, hidden, scale=1 / 64)
            d16 = rand(blocks, 128, 128)
            u16 = ops._sdd(x, v1, topo)
            meta = topo._meta
            meta.ensure_transposed(d16)
            w1t, v1t = w1.t().contiguous(), v1.t().contiguous()
            w1q_t = ops.quantize_weight(w1t)      # [F, h]: dX's weights
            v1q_t = ops.quantize_weight(v1t)
            dgq = ops.quantize_sparse(topo.with_data(d16))
            duq = ops.quantize_sparse(topo.with_data(u16))

            def gated_grad_fused():
                dg = ops._lowp_images(ops._FP8, blocks, True, True, "cuda")
                du = ops._lowp_images(ops._FP8, blocks, True, True, "cuda")
                sp.QuantizeBlocksGatedGrad(meta.descriptor(d16), g16.data,
                                           u16, "silu", dg, du)
                return dg, du

            def gated_grad_composed():
                return [ops._lowp_quantize_blocks(
                            ops._FP8, topo.with_data(t), None, None, None,
                            True, True, pow2=False)
                        for t in sp.BlockGateGrad(d16, g16.data, u16, "silu")]

            def backward_of(fn, *leaves, rerun=False):
                leaves = [t.detach().requires_grad_() for t in leaves]
                y = fn(*leaves)

                def run():
                    if rerun:
                        y.grad_fn.z2_consumed = False
                    return torch.autograd.grad(y, leaves, dy,
                                               retain_graph=True)
                return run

            def glu_fp8(mode):
                return lambda x_, a_, b_, c_: ops.glu_mlp_fp8(
                    x_, a_, b_, c_, topo, "silu", mode)

            arms = {
                "gated_grad_fused": gated_grad_fused,
                "gated_grad_composed": gated_grad_composed,
                "pair_fused": lambda: ops.dsd_fp8_pair(dgq, w1q_t, duq, v1q_t,
                                                       dt),
                "pair_composed": lambda: ops.dsd_fp8(dgq, w1q_t, dt)
                + ops.dsd_fp8(duq, v1q_t, dt),
                "glu_bf16_backward": backward_of(
                    lambda x_, a_, b_, c_: ops.glu_mlp(x_, a_, b_, c_, topo,
                                                       "silu"),
                    x, w1, v1, w2, rerun=True),
                "glu_fp8_backward": backward_of(glu_fp8("fp32"), x, w1t, v1t,
                                                w2),
                "glu_fp8_fast_backward": backward_of(glu_fp8("fast"), x, w1t,
                                                     v1t, w2),
            }
        if a.glu and a.mx:
            w1m_t = ops.quantize_weight_mx(w1t)   # [k = F, n = h]
            v1m_t = ops.quantize_weight_mx(v1t)
            dgm = ops.quantize_sparse_mx(topo.with_data(d16))
            dum = ops.quantize_sparse_mx(topo.with_data(u16))

            def gated_grad_mx_fused():
                dg = ops._lowp_images(ops._MX, blocks, True, True, "cuda")
                du = ops._lowp_images(ops._MX, blocks, True, True, "cuda")
                sp.QuantizeBlocksMxGatedGrad(meta.descriptor(d16), g16.data,
                                             u16, "silu", dg, du)
                return dg, du

            def gated_grad_mx_composed():
                return [ops._lowp_quantize_blocks(
                            ops._MX, topo.with_data(t), None, None, None,
                            True, True)
                        for t in sp.BlockGateGrad(d16, g16.data, u16, "silu")]

            arms = {
                "gated_grad_fused": gated_grad_mx_fused,
                "gated_grad_composed": gated_grad_mx_composed,
                "pair_fused": lambda: ops.dsd_mx_pair(dgm, w1m_t, dum, v1m_t,
                                                      dt),
                "pair_composed": lambda: ops.dsd_mx(dgm, w1m_t, dt)
                + ops.dsd_mx(dum, v1m_t, dt),
                "glu_bf16_backward": arms["glu_bf16_backward"],
                "glu_fp8_fast_backward": arms["glu_fp8_fast_backward"],
                "glu_mx_backward": backward_of(
                    lambda x_, a_, b_, c_: ops.glu_mlp_mx(x_, a_, b_, c_,
                                                          topo, "silu"),
                    x, w1t, v1t, w2),
            }
        if a.mx and a.gated:
            v1 = rand(D_MODEL, hidden, scale=1 / 64)
            mq, ms = ops.quantize_rows_mx(x)
            arms = {}
            for f in ("e4m3", "e2m1"):
                gw = ops.quantize_weight_mx(w1, format=f)
                uw = ops.quantize_weight_mx(v1, format=f)

                def chain(gw=gw, uw=uw):
                    g = ops.sdd_mx(mq, ms, gw, topo, dt)
                    u = ops.sdd_mx(mq, ms, uw, topo, dt)
                    return ops.quantize_sparse_mx(u, "silu", gate=g)
                arms[f"glu_chain_{f}"] = chain
                arms[f"glu_fused_{f}"] = (
                    lambda w=ops.MxGluWeight(gw, uw): ops.sdd_mx_gated(
                        mq, ms, w, topo, "silu", out_dtype=dt))
            del v1
        if a.mx and a.fp4:
            m1, m2 = (ops.quantize_weight_mx(w, format="e2m1")
                      for w in (w1, w2))
            mq, ms = ops.quantize_rows_mx(x)
            fq, fs = ops.quantize_rows_mx_fp4(x)
            hmx = ops.quantize_sparse_mx(g16, "gelu")
            hfp4 = ops.quantize_sparse_mx_fp4(g16, "gelu")
            arms = {
                "sdd_mx_e2m1": lambda: ops.sdd_mx(mq, ms, m1, topo, dt),
                "sdd_mx_fp4": lambda: ops.sdd_mx_fp4(fq, fs, m1, topo, dt),
                "dsd_mx_e2m1": lambda: ops.dsd_mx(hmx, m2, dt),
                "dsd_mx_fp4": lambda: ops.dsd_mx_fp4(hfp4, m2, dt),
                "quantize_rows_mx": lambda: ops.quantize_rows_mx(x),
                "quantize_rows_mx_fp4": lambda: ops.quantize_rows_mx_fp4(x),
            }
        calls = {}
        for name, fn in arms.items():
            fn()
            torch.cuda.synchronize()
            once = window(fn, 3)
            calls[name] = max(3, math.ceil(a.load_ms * 1e3 / once))
            spent = 0.0
            while spent < a.warm_ms * 1e3:
                spent += window(fn, calls[name]) * calls[name]
        times = {name: [] for name in arms}
        for _ in range(a.rounds):
            for name, fn in arms.items():
                times[name].append(window(fn, calls[name]))
        flops = 2.0 * blocks * 128 * 128
        work = {name: flops * D_MODEL for name in arms
                if name.startswith(("sdd_", "dsd_", "wgrad_"))}
        # (the backward of an MLP is four products of that size)
        work.update({name: 4 * flops * D_MODEL for name in arms
                     if name.endswith("_backward")})
        # (a gated expert's: six; the paired dX: two)
        work.update({name: (6 if name.endswith("_backward") else 2) * flops
                     * D_MODEL for name in arms
                     if name.startswith(("glu_", "pair_"))})
        # (both axes: 2 bytes read and 2 written per element and two scales
        # per 128; the activation gradient reads Z as well)
        moved = {"quantize_rows": rows * D_MODEL * 3 + rows * D_MODEL // 32,
                 "quantize_rows_mx": rows * D_MODEL * 3
                 + rows * D_MODEL // 32,
                 "quantize_rows_mx_fp4": rows * D_MODEL * 5 // 2
                 + rows * D_MODEL // 32,
                 "quantize_sparse_gelu": blocks * 16384 * 3 + blocks * 512,
                 "quantize_tiles": rows * D_MODEL * 4 + rows * D_MODEL // 16,
                 "quantize_blocks_gelu_grad": blocks * 16384 * 6
                 + blocks * 1024,
                 "quantize_tiles_mx": rows * D_MODEL * 4 + rows * D_MODEL // 16,
                 "quantize_blocks_mx_gelu_grad": blocks * 16384 * 6
                 + blocks * 1024}
        # (the gated gradients' algorithmic bytes, whatever the route: D, G
        # and U read, four byte images and four scale arrays written)
        moved.update({name: blocks * 16384 * 10 + blocks * 2048
                      for name in ("gated_grad_fused", "gated_grad_composed")})
        line = {"shape": shape, "rows": rows, "blocks": blocks,
                "build": sp.build_hash(), "rounds": a.rounds, "arms": {}}
        if parent is not None:
            line["parent_build"] = parent.sputnik_build_hash().decode()
        for name in arms:
            med = statistics.median(times[name])
            arm = {"us": round(med, 2), "min_us": round(min(times[name]), 2),
                   "max_us": round(max(times[name]), 2),
                   "calls": calls[name]}
            if name in work:
                arm["tflops"] = round(work[name] / med / 1e6, 1)
            else:
                tbs = moved[name] / med / 1e6
                arm["tb_per_s"] = round(tbs, 3)
                arm["hbm_share"] = round(tbs / HBM_TBS, 3)
            line["arms"][name] = arm
        us = {name: arm["us"] for name, arm in line["arms"].items()}
        if a.mx and a.fp4:
            line["pass"] = "mx fp4 forward"
            for op in ("sdd", "dsd"):
                line[f"{op}_mx_fp4_over_e2m1"] = round(
                    us[f"{op}_mx_fp4"] / us[f"{op}_mx_e2m1"], 3)
            line["quantize_rows_mx_fp4_over_mx"] = round(
                us["quantize_rows_mx_fp4"] / us["quantize_rows_mx"], 3)
        elif a.mx and a.gated:
            line["pass"] = "mx gated forward"
            for f in ("e4m3", "e2m1"):
                line[f"glu_fused_{f}_over_chain"] = round(
                    us[f"glu_fused_{f}"] / us[f"glu_chain_{f}"], 3)
        elif a.glu:
            line["pass"] = "glu backward"
            for fused in ("gated_grad", "pair"):
                line[f"{fused}_fused_over_composed"] = round(
                    us[f"{fused}_fused"] / us[f"{fused}_composed"], 3)
            if a.mx:
                line["pass"] = "mx glu backward"
                for base in ("bf16", "fp8_fast"):
                    line[f"glu_mx_backward_over_{base}"] = round(
                        us["glu_mx_backward"] / us[f"glu_{base}_backward"], 3)
            for name in () if a.mx else ("glu_fp8_backward",
                                         "glu_fp8_fast_backward"):
                line[f"{name}_over_bf16"] = round(
                    us[name] / us["glu_bf16_backward"], 3)
        elif a.backward and a.mx:
            line["pass"] = "mx backward"
            for base in ("bf16", "fp8_fast"):
                line[f"wgrad_mx_over_{base}"] = round(
                    us["wgrad_mx"] / us[f"wgrad_{base}"], 3)
            for base in ("bf16", "fp8", "fp8_fast"):
                line[f"mlp_mx_backward_over_{base}"] = round(
                    us["mlp_mx_backward"] / us[f"mlp_{base}_backward"], 3)
        elif a.backward:
            line["pass"] = "backward"
            for name in ("wgrad_fp8", "wgrad_fp8_fast"):
                line[f"{name}_over_bf16"] = round(
                    us[name] / us["wgrad_bf16"], 3)
            for name in ("mlp_fp8_backward", "mlp_fp8_fast_backward"):
                line[f"{name}_over_bf16"] = round(
                    us[name] / us["mlp_bf16_backward"], 3)
        for op in (("sdd", "dsd") if a.mx and not a.backward and not a.gated
                   and not a.fp4 else ()):
            for f in ("e4m3", "e2m1"):
                for base in ("bf16", "fp8_fast"):
                    line[f"{op}_mx_{f}_over_{base}"] = round(
                        us[f"{op}_mx_{f}"] / us[f"{op}_{base}"], 3)
            if parent is not None:
                line[f"{op}_fp8_fast_over_parent"] = round(
                    us[f"{op}_fp8_fast"] / us[f"{op}_fp8_fast_parent"], 3)
        for op in () if a.backward or a.mx or a.glu else ("sdd", "dsd"):
            line[f"{op}_fp8_over_bf16"] = round(
                us[f"{op}_fp8"] / us[f"{op}_bf16"], 3)
            line[f"{op}_fp8_fast_over_bf16"] = round(
                us[f"{op}_fp8_fast"] / us[f"{op}_bf16"], 3)
            line[f"{op}_fp8_fast_over_fp8"] = round(
                us[f"{op}_fp8_fast"] / us[f"{op}_fp8"], 3)
            if parent is not None:
                line[f"{op}_fp8_over_parent"] = round(
                    us[f"{op}_fp8"] / us[f"{op}_fp8_parent"], 3)
                line[f"{op}_fp8_fast_over_parent"] = round(
                    us[f"{op}_fp8_fast"] / us[f"{op}_fp8_parent"], 3)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
