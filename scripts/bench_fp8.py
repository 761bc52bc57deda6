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
        for name in ("sputnik_sdd_fp8", "sputnik_dsd_fp8"):
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
                "quantize_blocks_gelu_grad": lambda: ops._quantize_blocks(
                    dh16, "act_grad", 1, g16.data, True, True, False),
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
        # (both axes: 2 bytes read and 2 written per element and two scales
        # per 128; the activation gradient reads Z as well)
        moved = {"quantize_rows": rows * D_MODEL * 3 + rows * D_MODEL // 32,
                 "quantize_sparse_gelu": blocks * 16384 * 3 + blocks * 512,
                 "quantize_tiles": rows * D_MODEL * 4 + rows * D_MODEL // 16,
                 "quantize_blocks_gelu_grad": blocks * 16384 * 6
                 + blocks * 1024}
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
        if a.backward:
            line["pass"] = "backward"
            for name in ("wgrad_fp8", "wgrad_fp8_fast"):
                line[f"{name}_over_bf16"] = round(
                    us[name] / us["wgrad_bf16"], 3)
            for name in ("mlp_fp8_backward", "mlp_fp8_fast_backward"):
                line[f"{name}_over_bf16"] = round(
                    us[name] / us["mlp_bf16_backward"], 3)
        for op in () if a.backward else ("sdd", "dsd"):
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
