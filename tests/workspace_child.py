"""Child process of test_gpu_workspace.test_incall_counter_is_live: in a fresh
process (no transposed-B buffer exists yet) one SDD NT on the library route,
then the same call with a caller-owned workspace. Prints one JSON line with
how far sputnik_incall_events and sputnik_bt_launches moved across each call
and whether each result was exact. Not a test module."""

import json
import sys

import numpy as np
import torch

import sputnik_amd as sp
from tests.test_gpu_kat import IDense, ISparse, _expect


def main():
    sp.tuning("sdd_bt_min_mib", 1)
    rng = np.random.default_rng(31)
    m, k, n = 8192, 256, 4096
    A = IDense(m, k, rng, "f16")
    Bd = IDense(n, k, rng, "f16")
    Cs = ISparse(m, n, 0.6, rng, "f16")
    sp.AllocateRowIndicesBuffer(Cs.m)
    sp.RowIndices(Cs.m, Cs.m.row_indices)
    want = _expect(Cs.blocks_of(A.values.astype(np.float64) @ Bd.values.T), "f16")
    nbytes = sp.sdd_workspace_bytes(A.m, False, Bd.m, True, Cs.m)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    out = {"workspace_bytes": nbytes}
    for name, kw in (("library", {}), ("workspace", {"workspace": ws})):
        Cs.dev.fill_(float("nan"))
        e0, b0 = sp.incall_events(), sp.bt_launches()
        sp.Matmul(A.m, False, Bd.m, True, Cs.m, **kw)
        e1, b1 = sp.incall_events(), sp.bt_launches()
        torch.cuda.synchronize()
        out[name] = {"incall": e1 - e0, "bt": b1 - b0,
                     "exact": bool(torch.equal(Cs.dev, want))}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
