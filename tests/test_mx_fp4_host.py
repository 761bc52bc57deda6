"""CPU: the MXFP4-activation entry points are exported and the ops raise
their argument errors before any device call."""

import pytest

torch = pytest.importorskip("torch")

import sputnik_amd as sp  # noqa: E402
from sputnik_amd import ops  # noqa: E402

T, K, N = 128, 256, 256
BF16, U8 = torch.bfloat16, torch.uint8


def weight(fmt="e2m1"):
    q = (torch.zeros(N, K // 2, dtype=U8) if fmt == "e2m1"
         else torch.zeros(N, K, dtype=torch.float8_e4m3fn))
    return ops.MxWeight(q, torch.zeros(N, K // 32, dtype=U8), K, N, fmt)


TOPO = ops.SparseMatrix((T, N), torch.zeros(2, 128, 128, dtype=BF16),
                        torch.tensor([0, 2], dtype=torch.int32),
                        torch.tensor([0, 1], dtype=torch.int16))
XQ, XS = torch.zeros(T, K // 2, dtype=U8), torch.zeros(T, K // 32, dtype=U8)
SQ = ops.MxFp4SparseMatrix(TOPO, torch.zeros(2, 128, 64, dtype=U8),
                           torch.zeros(256, 4, dtype=U8))
MXFP8 = ops.MxSparseMatrix(TOPO, torch.zeros(2, 128, 128,
                                             dtype=torch.float8_e4m3fn),
                           torch.zeros(256, 4, dtype=U8))


def test_symbols_exported_with_their_signatures():
    for symbol, args in (("sputnik_quantize_rows_mx_fp4", 10),
                         ("sputnik_sdd_mx_fp4", 8), ("sputnik_dsd_mx_fp4", 7)):
        assert len(getattr(sp.lib(), symbol).argtypes) == args
    assert {"QuantizeRowsMxFp4", "SddMxFp4", "DsdMxFp4"} <= set(sp.__all__)
    assert {"MxFp4SparseMatrix", "quantize_rows_mx_fp4", "sdd_mx_fp4",
            "quantize_sparse_mx_fp4", "dsd_mx_fp4",
            "moe_mlp_mx_fp4"} <= set(ops.__all__)


BAD = [
    ("sdd_e4m3_weight", ValueError,
     lambda: ops.sdd_mx_fp4(XQ, XS, weight("e4m3"), TOPO)),
    ("sdd_topo_t", TypeError, lambda: ops.sdd_mx_fp4(XQ, XS, weight(), TOPO.t())),
    ("sdd_xq_unpacked", ValueError, lambda: ops.sdd_mx_fp4(
        torch.zeros(T, K, dtype=U8), XS, weight(), TOPO)),
    ("dsd_e4m3_weight", ValueError, lambda: ops.dsd_mx_fp4(SQ, weight("e4m3"))),
    ("dsd_mxfp8_operand", TypeError, lambda: ops.dsd_mx_fp4(MXFP8, weight())),
    ("rows_cols", ValueError,
     lambda: ops.quantize_rows_mx_fp4(torch.zeros(4, 192, dtype=BF16))),
    ("q_as_wide_as_x", ValueError, lambda: sp.QuantizeRowsMxFp4(
        torch.zeros(4, 128, dtype=BF16), torch.zeros(4, 128, dtype=U8),
        torch.zeros(4, 4, dtype=U8))),
]


@pytest.mark.parametrize("error,call", [b[1:] for b in BAD],
                         ids=[b[0] for b in BAD])
def test_argument_errors(error, call):
    with pytest.raises(error):
        call()
