"""CPU: the numpy references of the expert biases (tests/bias_ref.py) checked
against themselves -- the float32 emulations meet, on the very cases the GPU
tests use, the bounds those tests put on the device -- and the argument checks
of the bias entry points, which are raised before the library is called."""

import inspect

import numpy as np
import pytest

from oracle import oracle as O
from tests import bias_ref as R
from tests import moe_ref as M

B = 128
_IDS = ["%dx%d-E%d-%s-h%d" % (*c, h) for c, h in R.scatter_cases()]


def test_bias_stage_is_an_fp32_add_and_one_rounding():
    for dtype in M.DTYPES:
        rng = np.random.default_rng(3)
        x = O.round_to(rng.standard_normal((3, B, B)).astype(np.float32) * 8,
                       dtype)
        x[0, 0, :4] = [0.0, -0.0, 1.0, -1.0]
        idx = [2, 0, 1]
        bias = R.column_bias(3 * B, dtype)
        bias[2 * B:2 * B + 4] = [-0.0, -0.0, -1.0, 1.0]   # block 0's columns
        got = R.bias_stage(x, idx, bias, dtype)
        for b, c in enumerate(idx):
            exact = x[b].astype(np.float64) + bias[c * B:(c + 1) * B]
            assert np.array_equal(got[b], O.round_to(
                exact.astype(np.float32), dtype))
        # exact zeros are +0 whatever the signs of the terms
        assert (got[0, 0, :4].view(np.uint32) == 0).all()
        # a distinct bias per logical column where T can hold it
        n = 3 * B
        assert np.unique(R.column_bias(n, dtype)).size == n


def test_column_sum_references_agree():
    for dtype in M.DTYPES:
        for cols, indices in ((640, [3, 0, 4, 1, 2, 4, 0]), (512, [2, 0, 2])):
            nb = len(indices)
            vals = M.values((nb, B, B), dtype, [nb, cols, 5])
            ref, absum, n = R.column_sum64(vals, indices, cols)
            got = R.column_sum32(vals, indices, cols)
            assert (np.abs(got - ref)
                    <= R.column_sum_bound(ref, absum, n)).all()
            empty = np.setdiff1d(np.arange(cols // B), indices)
            for c in empty:
                assert (n[c * B:(c + 1) * B] == 0).all()
                assert (ref[c * B:(c + 1) * B] == 0).all()


@pytest.mark.parametrize("dtype", M.DTYPES)
@pytest.mark.parametrize("case,hidden", R.scatter_cases(), ids=_IDS)
def test_fp32_references_meet_the_gpu_bounds(case, hidden, dtype):
    tokens, top_k, e, _ = case
    c = M.case_inputs(case, hidden, dtype)
    r = c.route
    rows = M.exact_rows(r)
    b2 = R.case_bias(case, hidden, dtype)
    y = c.y_cols[:rows]
    for w in (None, c.w, c.w32):
        ref64, absum = R.scatter64(y, b2, r, w)
        got = R.scatter32(y, b2, r, w, dtype)
        assert (np.abs(got - ref64)
                <= R.scatter_bound(ref64, absum, top_k, dtype)).all()
        ref, ab, cnt = R.bgrad64(c.dout, r, e, w)
        got = R.bgrad32(c.dout, r, e, w)
        assert (np.abs(got - ref) <= R.bgrad_bound(ref, ab, cnt)).all()
        assert (got[cnt == 0] == 0).all()
    b_abs = R.case_bias_abs(case, hidden, dtype)
    ref, ab = R.wgrad64(c.dout_abs, c.y_rows[:rows], b_abs, r)
    got32 = R.wgrad32(c.dout_abs, c.y_rows[:rows], b_abs, r)
    for out_type in (dtype, "f32"):
        got = got32 if out_type == "f32" else O.round_to(got32, dtype)
        assert (np.abs(got - ref)
                <= M.wgrad_bound(ref, ab, hidden + 1, out_type)).all()


def test_row_expert_and_rows_out_of_range():
    case = (129, 2, 4, "empty")
    r = M.case_route(case)
    rows = M.exact_rows(r)
    e = R.row_expert(r, rows)
    top = M.routing(*case).reshape(-1)
    assert np.array_equal(e, top)
    row_of = np.array(r.row_of)
    row_of[[0, 5]] = [-1, rows]
    e = R.row_expert(r._replace(row_of=row_of), rows)
    assert e[0] == -1 and e[5] == -1 and np.array_equal(e[6:], top[6:])


# ---- argument checks --------------------------------------------------------

torch = pytest.importorskip("torch")


def _topo(ops, dtype=torch.float16):
    offsets = torch.tensor([0, 1, 2], dtype=torch.int32)
    indices = torch.tensor([0, 1], dtype=torch.int16)
    data = torch.zeros(2, B, B, dtype=dtype)
    return ops.SparseMatrix((2 * B, 2 * B), data, offsets, indices)


def _bad_biases(good_shape, dtype=torch.float16):
    """(bias, exception): wrong length, dtype and device."""
    wrong = list(good_shape)
    wrong[-1] += 1
    return [(torch.zeros(wrong, dtype=dtype), ValueError),
            (torch.zeros(good_shape, dtype=torch.float32), TypeError),
            (torch.zeros(good_shape, dtype=dtype, device="meta"), ValueError),
            (np.zeros(good_shape, dtype=np.float16), TypeError)]


def test_column_bias_checks_of_the_sdd_and_mlp_forms():
    from sputnik_amd import ops
    topo = _topo(ops)
    x = torch.zeros(2 * B, 64, dtype=torch.float16)
    w1 = torch.zeros(64, 2 * B, dtype=torch.float16)
    w2 = torch.zeros(2 * B, 64, dtype=torch.float16)
    calls = [
        lambda b: ops.sdd_bias(x, w1, topo, b),
        lambda b: ops.sdd_act_bias(x, w1, topo, "relu", bias=b),
        lambda b: ops.sdd_gated_bias(x, w1, topo, topo, "silu", bias=b),
        lambda b: ops.mlp_bias(x, w1, w2, topo, b1=b),
        lambda b: ops.glu_mlp_bias(x, w1, w1, w2, topo, b1=b),
        lambda b: ops.glu_mlp_bias(x, w1, w1, w2, topo, bv1=b),
    ]
    for call in calls:
        for bias, exc in _bad_biases((2 * B,)):
            with pytest.raises(exc):
                call(bias)
        with pytest.raises(ValueError):        # [1, cols] is not [cols]
            call(torch.zeros(1, 2 * B, dtype=torch.float16))
    with pytest.raises(TypeError):
        ops.sdd_bias(x, w1, topo, None)
    with pytest.raises(ValueError):            # the bias of a .t() view
        ops.sdd_bias(w1.t(), x.t(), topo.t(),
                     torch.zeros(2 * B, dtype=torch.float16))
    with pytest.raises(TypeError):
        ops.column_sum(topo.data)
    with pytest.raises(ValueError):
        ops.column_sum(topo.t())


def test_expert_bias_checks_of_the_moe_forms():
    from sputnik_amd import ops
    tokens, d_model, ffn, e, top_k = 4, 64, B, 2, 1
    dt = torch.float16
    x = torch.zeros(tokens, d_model, dtype=dt)
    w1 = torch.zeros(d_model, e * ffn, dtype=dt)
    w2 = torch.zeros(e * ffn, d_model, dtype=dt)
    top = torch.zeros(tokens, top_k, dtype=torch.int64)
    ew = torch.ones(tokens, top_k, dtype=dt)
    wr = torch.zeros(e, d_model, dtype=dt)

    def mlp(**kw):
        return ops.moe_mlp_bias(x, top, ew, w1, w2, e, **kw)

    def glu(**kw):
        return ops.moe_mlp_bias(x, top, ew, w1, w2, e, v1=w1, **kw)

    for bias, exc in _bad_biases((e * ffn,)):
        with pytest.raises(exc):
            mlp(b1=bias)
        with pytest.raises(exc):
            glu(bv1=bias)
    for bias, exc in _bad_biases((e, d_model)):
        with pytest.raises(exc):
            mlp(b2=bias)
        for layer in (ops.moe_layer_bias, ops.moe_layer_aux_bias,
                      ops.moe_score_layer_bias):
            with pytest.raises(exc):
                layer(x, wr, w1, w2, top_k, b2=bias)
    with pytest.raises(ValueError):            # bv1 without v1
        mlp(bv1=torch.zeros(e * ffn, dtype=dt))
    with pytest.raises(ValueError):            # b2 flat
        mlp(b2=torch.zeros(e * d_model, dtype=dt))


def test_bias_entry_points_and_signatures():
    import sputnik_amd as sp
    from sputnik_amd import ops

    def kwonly(fn):
        return [n for n, p in inspect.signature(fn).parameters.items()
                if p.kind is inspect.Parameter.KEYWORD_ONLY]

    def positional(fn):
        return [n for n, p in inspect.signature(fn).parameters.items()
                if p.kind is not inspect.Parameter.KEYWORD_ONLY]

    # each *_bias form: the bias-free form's arguments, then keyword-only
    # biases that default to None
    for name, extra in (("sdd_act", ["bias"]), ("sdd_gated", ["bias"]),
                        ("mlp", ["b1"]), ("glu_mlp", ["b1", "bv1"]),
                        ("padded_scatter", ["bias"]),
                        ("moe_mlp", ["b1", "bv1", "b2"]),
                        ("moe_layer", ["b1", "bv1", "b2"]),
                        ("moe_layer_aux", ["b1", "bv1", "b2"]),
                        ("moe_score_layer", ["b1", "bv1", "b2"])):
        plain, biased = getattr(ops, name), getattr(ops, name + "_bias")
        assert positional(biased) == positional(plain), name
        assert kwonly(plain) == [] and kwonly(biased) == extra, name
        for k in extra:
            assert inspect.signature(biased).parameters[k].default is None
        assert name + "_bias" in ops.__all__
    assert positional(ops.sdd_bias)[:4] == ["a", "b", "topo", "bias"]
    assert "sdd_bias" in ops.__all__ and "column_sum" in ops.__all__
    for name in ("MatmulBias", "MatmulBiasActivation", "MatmulBiasGated",
                 "BlockColumnSum", "PaddedScatterBias",
                 "PaddedScatterBiasWeightGrad", "PaddedScatterBiasGrad"):
        assert name in sp.__all__ and callable(getattr(sp, name)), name


def test_c_abi_exports_the_bias_entry_points():
    import os
    import subprocess

    import sputnik_amd as sp
    assert os.path.exists(sp.LIB_PATH), "build it: make -C sputnik_amd"
    syms = subprocess.run(["nm", "-D", "--defined-only", sp.LIB_PATH],
                          capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(os.path.dirname(sp.LIB_PATH), "..", "include",
                               "sputnik_amd.h")).read()
    for name in ("sputnik_sdd_bias", "sputnik_sdd_bias_act",
                 "sputnik_sdd_bias_gated", "sputnik_block_column_sum",
                 "sputnik_padded_scatter_bias",
                 "sputnik_padded_scatter_bias_wgrad",
                 "sputnik_padded_scatter_bias_grad"):
        assert f" T {name}\n" in syms, name
        assert f"int {name}(" in header, name
        assert name in sp._SIGNATURES, name
