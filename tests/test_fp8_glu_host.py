"""CPU: ops.glu_mlp_fp8 and ops.moe_glu_mlp_fp8_train raise their argument
errors before any device call (every tensor here lives on the host)."""

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
    ("sink_shape", ValueError, {"v1t_grad_out": lambda a: torch.zeros(F, 128)}),
    ("sink_dtype", TypeError,
     {"w2_grad_out": lambda a: torch.zeros(F, H, dtype=torch.float16)}),
    ("accumulate", ValueError, {"accumulate": lambda a: "fp16"}),
]


# (the MoE layer builds its own topology)
CASES = [(moe,) + b[1:] for moe in (False, True) for b in BAD
         if not (moe and b[0] == "topo_t")]
IDS = [("moe-" if moe else "mlp-") + b[0] for moe in (False, True)
       for b in BAD if not (moe and b[0] == "topo_t")]


@pytest.mark.parametrize("moe,error,change", CASES, ids=IDS)
def test_argument_errors(moe, error, change):
    a = {"x": torch.zeros(T, H, dtype=BF16),
         "topo": ops.SparseMatrix((T, F), torch.zeros(2, 128, 128, dtype=BF16),
                                  torch.tensor([0, 2], dtype=torch.int32),
                                  torch.tensor([0, 1], dtype=torch.int16))}
    a.update({w: torch.zeros(F, H, dtype=BF16) for w in ("w1t", "v1t", "w2")})
    a.update({k: f(a) for k, f in change.items()})
    x, w1t, v1t, w2, topo = (a.pop(k) for k in ("x", "w1t", "v1t", "w2", "topo"))
    with pytest.raises(error):
        if moe:
            ops.moe_glu_mlp_fp8_train(
                x, torch.zeros(T, 1, dtype=torch.int32),
                torch.ones(T, 1, dtype=BF16), w1t, v1t, w2, E, **a)
        else:
            ops.glu_mlp_fp8(x, w1t, v1t, w2, topo, **a)
