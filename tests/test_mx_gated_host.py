"""CPU: SddMxGated's entry point is exported, ops.MxGluWeight checks its parts
and ops.sdd_mx_gated raises its argument errors before any device call."""

import pytest

torch = pytest.importorskip("torch")

import sputnik_amd as sp  # noqa: E402
from sputnik_amd import ops  # noqa: E402

T, K, N = 128, 256, 256
BF16, E4M3 = torch.bfloat16, torch.float8_e4m3fn


def weight(n=N, k=K, fmt="e4m3"):
    q = (torch.zeros(n, k // 2, dtype=torch.uint8) if fmt == "e2m1"
         else torch.zeros(n, k, dtype=E4M3))
    return ops.MxWeight(q, torch.zeros(n, k // 32, dtype=torch.uint8), k, n, fmt)


def test_symbol_exported_with_its_signature():
    assert len(sp.lib().sputnik_sdd_mx_gated.argtypes) == 23
    assert "SddMxGated" in sp.__all__


def test_mx_glu_weight():
    w = ops.MxGluWeight(weight(), weight())
    assert (w.shape, w.row_step, w.format) == ((K, N), 1, "e4m3")
    for fmt in ("e4m3", "e2m1"):
        both = weight(2 * N, K, fmt)
        w = ops.MxGluWeight.from_interleaved(both.q, both.scales, fmt)
        assert (w.shape, w.row_step, w.format) == ((K, N), 2, fmt)
        # views of the tensor as it is: gate the even rows, up the odd ones
        assert w.gate_q.data_ptr() == both.q.data_ptr()
        assert w.up_q.data_ptr() == both.q[1].data_ptr()
        assert w.up_scales.data_ptr() == both.scales[1].data_ptr()
    for error, make in (
            (TypeError, lambda: ops.MxGluWeight(weight(), weight().q)),
            (ValueError, lambda: ops.MxGluWeight(weight(), weight(n=128))),
            (ValueError, lambda: ops.MxGluWeight(weight(), weight(fmt="e2m1"))),
            (ValueError, lambda: ops.MxGluWeight.from_interleaved(
                weight(384).q, weight(384).scales)),      # an odd block count
            (ValueError, lambda: ops.MxGluWeight.from_interleaved(
                weight(512).q, weight(256).scales)),
            (ValueError, lambda: ops.MxGluWeight.from_interleaved(
                weight(512).q, weight(512).scales, "e3m2"))):
        with pytest.raises(error):
            make()


BAD = [
    ("w", TypeError, {"w": weight()}),
    ("topo_t", TypeError, {"topo": lambda t: t.t()}),
    ("xq_cols", ValueError, {"xq": torch.zeros(T, 128, dtype=E4M3)}),
    ("xq_rows", ValueError, {"xq": torch.zeros(2 * T, K, dtype=E4M3)}),
    ("act", ValueError, {"activation": "tanh"}),
    ("clamp_pair", ValueError, {"clamp": 7.0}),
    ("clamp_limit", ValueError, {"clamp": (1.702, 0.0)}),
    ("clamp_alpha", ValueError, {"clamp": (float("nan"), 7.0)}),
    ("b1_shape", ValueError, {"b1": torch.zeros(N + 1, dtype=BF16)}),
    ("bv1_dtype", ValueError, {"bv1": torch.zeros(N, dtype=torch.float16)}),
    ("out_dtype", TypeError, {"out_dtype": torch.float32}),
]


@pytest.mark.parametrize("error,change", [b[1:] for b in BAD],
                         ids=[b[0] for b in BAD])
def test_sdd_mx_gated_argument_errors(error, change):
    topo = ops.SparseMatrix((T, N), torch.zeros(2, 128, 128, dtype=BF16),
                            torch.tensor([0, 2], dtype=torch.int32),
                            torch.tensor([0, 1], dtype=torch.int16))
    a = {"xq": torch.zeros(T, K, dtype=E4M3), "topo": topo,
         "xs": torch.zeros(T, K // 32, dtype=torch.uint8),
         "w": ops.MxGluWeight(weight(), weight())}
    a.update({k: v(topo) if callable(v) else v for k, v in change.items()})
    first = [a.pop(k) for k in ("xq", "xs", "w", "topo")]
    with pytest.raises(error):
        ops.sdd_mx_gated(*first, **a)
