"""The measurement behind eps_fast of sputnik/block/fp8.h: the interval sums
of Fp8IntervalSums in both modes against the exact float64 dot products of the
decoded bytes, as |P - exact| / sum |products|, over the four seeded operand
families of tests/fp8_fast_ref.py (random finite bytes, bytes quantised from
normal data, one large product among small ones at every k position and ratio
2^-1 .. 2^-17, two cancelling large products in the same and in different
lane groups). It measures the instruction, not the product kernel.

One JSON line per family and mode: the worst ratio and its log2, how many
sums differ from the exact ones, and for the two constructed families the
worst ratio per small-to-large ratio; a last line gives eps_fast, the
smallest power of two at or above twice the worst kFast ratio.

python scripts/probe_fp8_accum.py [--out profiles/fp8/accum_probe.jsonl]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    import sputnik_amd as sp
    from tests import fp8_fast_ref as F

    assert torch.cuda.is_available(), "needs a GPU"

    def sums(aq, bq, mode):
        m, k = aq.shape
        p = torch.empty(k // 128, m, bq.shape[0], dtype=torch.float32,
                        device="cuda")
        sp.Fp8IntervalSums(
            torch.from_numpy(aq).cuda().view(torch.float8_e4m3fn),
            torch.from_numpy(bq).cuda().view(torch.float8_e4m3fn), p,
            accumulate=mode)
        torch.cuda.synchronize()
        return p.cpu().numpy().astype(np.float64)

    lines, worst_fast = [], 0.0
    for name, (aq, bq) in F.families().items():
        exact, absum = F.exact_sums(aq, bq)
        for mode in ("fast", "fp32"):
            p = sums(aq, bq, mode)
            ratio = np.abs(p - exact) / np.where(absum == 0, 1.0, absum)
            worst = float(ratio.max())
            line = {"family": name, "mode": mode, "shape": list(p.shape),
                    "worst": worst,
                    "log2_worst": round(math.log2(worst), 2) if worst else None,
                    "sums_not_exact": int((p != exact).sum()),
                    "build": sp.build_hash()}
            if name in ("large_among_small", "cancelling_large"):
                # rows are (placement,) small exponent a, position t
                per = ratio[0].reshape(-1, len(F.SMALL_EXPONENTS), 128,
                                       ratio.shape[-1]).max(axis=(0, 2, 3))
                line["worst_by_small_over_large"] = {
                    f"2^-{a + 8}": (round(math.log2(v), 2) if v else None)
                    for a, v in zip(F.SMALL_EXPONENTS, per.tolist())}
            if mode == "fast":
                worst_fast = max(worst_fast, worst)
            print(json.dumps(line), flush=True)
            lines.append(line)
    eps = 2.0 ** math.ceil(math.log2(2.0 * worst_fast))
    line = {"worst_fast": worst_fast,
            "log2_worst_fast": round(math.log2(worst_fast), 2),
            "eps_fast": eps, "log2_eps_fast": int(math.log2(eps)),
            "in_tests": F.EPS_FAST}
    print(json.dumps(line), flush=True)
    lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
