"""CPU: ops.glu_mlp_mx, ops.moe_glu_mlp_mx_train and ops.dsd_mx_pair raise
their argument errors before any device call (every tensor here lives on the
host)."""

import pytest

torch = pytest.importorskip("torch")

from sputnik_amd import ops  # noqa: E402

T, H, F, E = 128, 256, 256, 2
BF16 = torch.bfloat16

# (what, the error, keyword -> replacement); x, w1t, v1t, w2 and topo by name
BAD = [
    ("x_cols", ValueError, {"x": lambda a: a["x"][:, :192]}),
    ("v1t_shape", ValueError, {"v1t": lambda a: a["v1t"][:128]}),
    ("v1t_dim", ValueError, {"v1t": lambda a: a["v1t"][0]}),
    ("w2_shape", ValueError, {"w2": lambda a: a["w2"][:, :128]}),
    ("rows", ValueError, {"x": lambda a: torch.zeros(2 * T, H, dtype=BF16)}),
    ("dtype", TypeError, {"v1t": lambda a: a["v1t"].half()}),
    ("topo_t", TypeError, {"topo": lambda a: a["topo"].t()}),
    ("sink_shape", ValueError, {"dv1t_out": lambda a: torch.zeros(F, 128)}),
    ("sink_dtype", TypeError,
     {"dw2_out": lambda a: torch.zeros(F, H, dtype=torch.float16)}),
]


def _topo():
    return ops.SparseMatrix((T, F), torch.zeros(2, 128, 128, dtype=BF16),
                            torch.tensor([0, 2], dtype=torch.int32),
                            torch.tensor([0, 1], dtype=torch.int16))


@pytest.mark.parametrize("error,change", [b[1:] for b in BAD],
                         ids=[b[0] for b in BAD])
def test_argument_errors(error, change):
    a = {"x": torch.zeros(T, H, dtype=BF16), "topo": _topo()}
    a.update({w: torch.zeros(F, H, dtype=BF16) for w in ("w1t", "v1t", "w2")})
    a.update({k: f(a) for k, f in change.items()})
    x, w1t, v1t, w2, topo = (a.pop(k) for k in ("x", "w1t", "v1t", "w2", "topo"))
    with pytest.raises(error):
        ops.glu_mlp_mx(x, w1t, v1t, w2, topo, **a)
    if "topo" not in change:        # the MoE layer builds its own topology
        with pytest.raises(error):
            ops.moe_glu_mlp_mx_train(
                x, torch.zeros(T, 1, dtype=torch.int32),
                torch.ones(T, 1, dtype=BF16), w1t, v1t, w2, E, **a)


def test_dsd_mx_pair_argument_errors():
    def sparse(topo):
        return ops.MxSparseMatrix(
            topo, torch.zeros(2, 128, 128, dtype=torch.float8_e4m3fn),
            torch.zeros(256, 4, dtype=torch.uint8))

    def weight(k=F, n=H, fmt="e4m3"):
        return ops.MxWeight(torch.zeros(n, k, dtype=torch.float8_e4m3fn),
                            torch.zeros(n, k // 32, dtype=torch.uint8), k, n,
                            fmt)
    topo = _topo()
    sq, w = sparse(topo), weight()
    for error, args in (
            (TypeError, (topo, w, sq, w)),              # not quantised
            (TypeError, (sq, w.q, sq, w)),              # not an MxWeight
            (ValueError, (sq, w, sparse(_topo()), w)),  # another topology
            (ValueError, (sq, w, sq, weight(n=128))),   # the weights differ
            (ValueError, (sq, weight(k=128), sq, weight(k=128))),
            (ValueError, (sq, w, sq, weight(fmt="e2m1"))),
            (TypeError, (sq, w, sq, w, torch.float32))):
        with pytest.raises(error):
            ops.dsd_mx_pair(*args)
