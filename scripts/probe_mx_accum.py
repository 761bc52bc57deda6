"""The measurement behind the error term of sputnik/block/mx.h: SddMx (fp16
output, one full 128 x 128 block per 128 rows) against the exact float64
product of the decoded operands, as |C - exact| / sum |terms|, for both weight
formats over three operand families:

    normal     tests/test_gpu_mx.py's random data: bytes quantised from normal
               data whose 32-blocks spread over 16 binades, K = 640
    bytes      uniformly random finite e4m3 bytes (e2m1: nibbles) under scale
               bytes spread over 8 binades each, K = 128
    outlier    one product 2^11 .. 2^17 above its 127 neighbours, at every
               eighth k position, the gap split between the element (up to
               2^8) and the e8m0 scale (up to 2^9) of the operand that carries
               it: A for both formats, B as well for e4m3; K = 128

The ratio includes the rounding of C to fp16 (at most 2^-12 of |exact|), so it
bounds the accumulation error from above. One JSON line per family and
format; a last line gives eps_mx, the smallest power of two at or above twice
the worst ratio, beside eps_fast.

python scripts/probe_mx_accum.py [--out profiles/mx/accum_probe.jsonl]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GAPS = range(11, 18)
POSITIONS = range(0, 128, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    import sputnik_amd as sp
    from tests import fp8_ref as F
    from tests import mx_ref as R
    from tests import test_gpu_mx as T

    assert torch.cuda.is_available(), "needs a GPU"
    rng = np.random.default_rng(41)
    finite = np.array([b for b in range(256) if b & 0x7F != 0x7F], np.uint8)

    def ratio(aq, sa, wc, sw, fmt):
        m, n = aq.shape[0], wc.shape[0]
        topo = (np.arange(m // 128 + 1, dtype=np.int32) * (n // 128),
                np.tile(np.arange(n // 128, dtype=np.int16), m // 128))
        got = T.host(T.sdd_call(aq, sa, wc, sw, fmt, "f16", topo))
        torch.cuda.synchronize()
        exact, absum = T.exact(aq, sa, wc, sw, fmt)
        err = np.abs(got.astype(np.float64)
                     - F.blocks_from_dense(exact, *topo))
        return err / np.maximum(F.blocks_from_dense(absum, *topo), 1e-300)

    def outlier(rows_carry, fmt):
        """[128, 128] codes and [128, 4] scales of the carrying operand (row
        (gap, position) pairs; the spare rows have no outlier) and of the
        plain one: elements 1, scales 2^-6 on the B side."""
        val = np.ones((128, 128))
        sc = np.zeros((128, 4), np.int64)
        pairs = [(g, t) for g in GAPS for t in POSITIONS]
        for row, (gap, t) in enumerate(pairs):
            by_scale = min(9, (gap + 1) // 2)
            blk = t // 32
            sc[row, blk] = by_scale
            val[row, 32 * blk:32 * blk + 32] = 2.0 ** -by_scale
            val[row, t] = 2.0 ** (gap - by_scale)   # times 2^by_scale: 2^gap
        codes = F.encode(val.astype(np.float32))
        plain = (R.encode_e2m1(np.ones((128, 128))) if fmt == "e2m1"
                 and rows_carry == "a" else F.encode(np.ones((128, 128),
                                                             np.float32)))
        zero = np.zeros((128, 4), np.int64)
        if rows_carry == "a":
            return (codes, (sc + 127).astype(np.uint8), plain,
                    (zero + 121).astype(np.uint8)), pairs
        return (plain, (zero + 127).astype(np.uint8), codes,
                (sc + 121).astype(np.uint8)), pairs

    lines, worst_all = [], 0.0
    for fmt in ("e4m3", "e2m1"):
        cases = {"normal": T.random_operands(256, 640, 256, fmt, "f16",
                                             [5, 640])}
        aq = rng.choice(finite, (256, 128))
        wc = (rng.integers(0, 16, (256, 128)).astype(np.uint8)
              if fmt == "e2m1" else rng.choice(finite, (256, 128)))
        # (|sums| stay below 128 * 448 * 448 * 2^-14: inside fp16)
        cases["bytes"] = (aq, rng.integers(113, 121, (256, 4)).astype(np.uint8),
                          wc, rng.integers(113, 121, (256, 4)).astype(np.uint8))
        cases["outlier_a"], pairs = outlier("a", fmt)
        if fmt == "e4m3":
            cases["outlier_b"], _ = outlier("b", fmt)
        for name, o in cases.items():
            r = ratio(*o, fmt)
            worst = float(r.max())
            worst_all = max(worst_all, worst)
            line = {"family": name, "format": fmt, "k": int(o[0].shape[1]),
                    "worst": worst, "log2_worst": round(math.log2(worst), 2),
                    "build": sp.build_hash()}
            if name.startswith("outlier"):
                # (the carrying index is the row of C for A, the column for B)
                r = r[0] if name == "outlier_a" else r[0].T
                per = r[:len(pairs)].reshape(len(GAPS), len(POSITIONS), 128)
                line["log2_worst_by_gap"] = {
                    f"2^{g}": round(math.log2(max(v, 1e-300)), 2)
                    for g, v in zip(GAPS, per.max(axis=(1, 2)).tolist())}
            print(json.dumps(line), flush=True)
            lines.append(line)
    eps = 2.0 ** math.ceil(math.log2(2.0 * worst_all))
    line = {"worst": worst_all, "log2_worst": round(math.log2(worst_all), 2),
            "eps_mx": eps, "log2_eps_mx": int(math.log2(eps)),
            "eps_fast": R.EPS_FAST}
    print(json.dumps(line), flush=True)
    lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
