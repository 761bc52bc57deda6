"""GPU: the MoE ops of sputnik_amd/ops.py: moe_route, MoeRoute.from_megablocks,
padded_gather and padded_scatter with autograd, and moe_mlp.

Forward values of the permutation come from tests/moe_ref.py (numpy); its
gradients and the whole of moe_mlp from fp32 torch with autograd on the same
operands (index_select / index_add, and a dense loop over experts), under
helpers.assert_close. The bit-for-bit comparison of moe_mlp with rows=None
against rows=moe_rows_bound(...) compares the library with itself: it shows
that the trailing zero rows change nothing, it is not a correctness oracle.
"""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from sputnik_amd import ops  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests import moe_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

CASE = (300, 2, 4, "exact")     # tokens, top_k, E, routing (moe_ref.CASES)
HIDDEN = 264


def _dev(a, dtype, grad=False):
    return torch.from_numpy(np.array(a)).to(
        H.torch_dtype(dtype)).cuda().requires_grad_(grad)


def _f32(a):
    return torch.from_numpy(np.array(a)).float().cuda() \
        .requires_grad_(True)


def _np(t):
    return t.detach().float().cpu().numpy()


def _same(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


def _route_equals(route, r, rows):
    for name in ("indices", "bin_ids", "bins", "padded_bins",
                 "tokens_per_expert", "row_of"):
        t = getattr(route, name)
        assert t.dtype == torch.int32 and t.is_cuda, name
        assert np.array_equal(t.cpu().numpy(), getattr(r, name)), name
    assert (route.top_k, route.tokens, route.rows) == (r.top_k, r.tokens, rows)


@pytest.mark.parametrize("case", R.CASES, ids=["%dx%d-E%d-%s" % c
                                               for c in R.CASES])
def test_moe_route_and_from_megablocks(case):
    tokens, top_k, e, kind = case
    r = R.case_route(case)
    top = torch.from_numpy(R.routing(*case)).cuda()
    bound = ops.moe_rows_bound(tokens * top_k, e)
    for rows, expect in ((None, R.exact_rows(r)), (bound, bound),
                         (bound + 128, bound + 128)):
        route = ops.moe_route(top, e, rows)
        _route_equals(route, r, expect)
        # MegaBlocks hands its tensors over as int32 or int64
        for cast in (torch.int32, torch.int64):
            again = ops.MoeRoute.from_megablocks(
                route.indices.to(cast), route.bin_ids.to(cast),
                route.bins.to(cast), route.padded_bins.to(cast), top_k, rows)
            _route_equals(again, r, expect)
    if top_k == 1:
        _route_equals(ops.moe_route(top[:, 0], e), r, R.exact_rows(r))


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("explicit_rows", [False, True])
def test_padded_gather_forward_backward(dtype, explicit_rows):
    c = R.case_inputs(CASE, HIDDEN, dtype)
    r = c.route
    n = r.tokens * r.top_k
    rows = ops.moe_rows_bound(n, CASE[2]) if explicit_rows else None
    route = ops.moe_route(torch.from_numpy(R.routing(*CASE)).cuda(), CASE[2],
                          rows)
    x = _dev(c.x, dtype, True)
    out = ops.padded_gather(x, route)
    assert out.shape == (route.rows, HIDDEN)
    ref = R.gather(c.x, r, route.rows)
    assert np.array_equal(_np(out).view(np.uint32), ref.view(np.uint32))
    dout = _dev(c.y[:route.rows], dtype)
    out.backward(dout)
    # fp32 torch: the same copy as an index_select, differentiated
    x32 = _f32(c.x)
    token_of = torch.arange(n, device="cuda") // r.top_k
    full = torch.zeros(route.rows, HIDDEN, device="cuda").index_add(
        0, torch.from_numpy(np.array(r.row_of)).long().cuda(),
        x32.index_select(0, token_of))
    full.backward(dout.float())
    H.assert_close(_np(x.grad), _np(x32.grad), dtype, "padded_gather dx")


@pytest.mark.parametrize("dtype", R.DTYPES)
@pytest.mark.parametrize("weights", [None, "T", "f32", "f32-flat"])
def test_padded_scatter_forward_backward(dtype, weights):
    c = R.case_inputs(CASE, HIDDEN, dtype)
    r = c.route
    n = r.tokens * r.top_k
    route = ops.moe_route(torch.from_numpy(R.routing(*CASE)).cuda(), CASE[2])
    rows = route.rows
    y = _dev(c.y[:rows], dtype, True)
    if weights is None:
        w = w_np = None
    elif weights == "T":
        w_np = c.w
        w = _dev(c.w.reshape(r.tokens, r.top_k), dtype, True)
    else:
        w_np = c.w32
        shape = (n,) if weights == "f32-flat" else (r.tokens, r.top_k)
        w = torch.from_numpy(np.array(c.w32.reshape(shape))).cuda() \
            .requires_grad_(True)
    out = ops.padded_scatter(y, route, w)
    assert out.shape == (r.tokens, HIDDEN) and out.dtype == y.dtype
    if weights in (None, "T"):
        ref = R.scatter32(c.y, r, w_np, dtype)
        assert np.array_equal(_np(out).view(np.uint32), ref.view(np.uint32))
    else:
        ref, _ = R.scatter64(c.y, r, w_np)
        H.assert_close(_np(out), ref, dtype, "padded_scatter")
    dout = _dev(c.dout, dtype)
    out.backward(dout)

    y32 = _f32(c.y[:rows])
    w32 = None if w is None else _f32(w_np)
    picked = y32.index_select(
        0, torch.from_numpy(np.array(r.row_of)).long().cuda())
    if w32 is not None:
        picked = picked * w32[:, None]
    ref_out = picked.view(r.tokens, r.top_k, HIDDEN).sum(1)
    ref_out.backward(dout.float())
    H.assert_close(_np(y.grad), _np(y32.grad), dtype, "padded_scatter dy")
    if w is not None:
        assert w.grad.shape == w.shape and w.grad.dtype == w.dtype
        H.assert_close(_np(w.grad).reshape(-1), _np(w32.grad),
                       dtype, "padded_scatter dw")


# ---- moe_mlp ----------------------------------------------------------------

TOKENS, D_MODEL, FFN, EXPERTS, TOP_K = 300, 256, 256, 4, 2
_MLP = {}


def _mlp_data():
    """Operands of the moe_mlp test, once: x and dy in {-1, 0, 1}, the expert
    weights in {-1, 0, 1} / 16, the router weights of a token (1/4, 3/4),
    (1/2, 1/2) or (3/4, 1/4).

    Why not random reals: against an fp32 reference, helpers.assert_close
    leaves a chain of bf16 roundings little room at this shape. A CPU
    emulation of the GLU layer in which every stored intermediate (Z1, Z2, H,
    the expert output, the weighted dy, D = dy W2^T, dZ1, dZ2 and each
    result) is correctly rounded to bf16 reaches 0.7-1.16 of the tolerance
    over a few seeds with U(-1, 1) or Gaussian operands, i.e. correct
    arithmetic fails on some seeds. With these operands the products of d_model
    = ffn = 256 terms are multiples of 1/16 (of 1/64 behind the router
    weights) below 16 in magnitude, so Z1, Z2, the weighted dy and nearly
    every D are exact in bf16; the roundings that remain (H, the expert
    output, dZ1, dZ2, the results) keep the same emulation at or below 0.69
    of the tolerance on 8 seeds, for every output and gradient."""
    if not _MLP:
        rng = np.random.default_rng(17)

        def make(*shape, scale=1.0):
            return (rng.integers(-1, 2, shape) * scale).astype(np.float32)
        # distinct experts per token, as a top-k router gives them
        top = np.stack([rng.permutation(EXPERTS)[:TOP_K]
                        for _ in range(TOKENS)])
        first = rng.choice([0.25, 0.5, 0.75], TOKENS).astype(np.float32)
        _MLP.update(
            top=top, gates=np.stack([first, 1 - first], axis=1),
            x=make(TOKENS, D_MODEL),
            w1=make(D_MODEL, EXPERTS * FFN, scale=1 / 16),
            v1=make(D_MODEL, EXPERTS * FFN, scale=1 / 16),
            w2=make(EXPERTS * FFN, D_MODEL, scale=1 / 16),
            dy=make(TOKENS, D_MODEL))
        for v in _MLP.values():
            v.setflags(write=False)
    return _MLP


def _dense_reference(d, glu):
    """y[t] = sum_k gate[t, k] * MLP_{top[t, k]}(x[t]) in fp32 torch: every
    expert applied to every token, then selected. Returns y and the gradients
    in the order x, gates, w1, w2[, v1]."""
    F = torch.nn.functional
    x, gates = _f32(d["x"]), _f32(d["gates"])
    w1, w2 = _f32(d["w1"]), _f32(d["w2"])
    v1 = _f32(d["v1"]) if glu else None
    top = torch.from_numpy(np.array(d["top"])).cuda()
    y = torch.zeros(TOKENS, D_MODEL, device="cuda")
    for e in range(EXPERTS):
        cols = slice(e * FFN, (e + 1) * FFN)
        if glu:
            h = F.silu(x @ w1[:, cols]) * (x @ v1[:, cols])
        else:
            h = F.gelu(x @ w1[:, cols], approximate="tanh")
        share = (gates * (top == e)).sum(1, keepdim=True)
        y = y + share * (h @ w2[cols])
    leaves = [x, gates, w1, w2] + ([v1] if glu else [])
    y.backward(_f32(d["dy"]).detach())
    return y, [t.grad for t in leaves]


@pytest.mark.parametrize("glu", [False, True], ids=["mlp", "glu"])
@pytest.mark.parametrize("gate_dtype", ["f32", "bf16"])
def test_moe_mlp_forward_backward_bf16(glu, gate_dtype):
    d = _mlp_data()
    top = torch.from_numpy(np.array(d["top"])).cuda()
    ref_y, ref_grads = _dense_reference(d, glu)
    bound = ops.moe_rows_bound(TOKENS * TOP_K, EXPERTS)
    outs = []
    for rows in (None, bound):
        x, w1, w2 = (_dev(d[k], "bf16", True) for k in ("x", "w1", "w2"))
        v1 = _dev(d["v1"], "bf16", True) if glu else None
        gates = torch.from_numpy(np.array(d["gates"])).cuda()
        if gate_dtype == "bf16":
            gates = gates.bfloat16()
        gates.requires_grad_(True)
        y = ops.moe_mlp(x, top, gates, w1, w2, EXPERTS, v1=v1, rows=rows)
        assert y.shape == (TOKENS, D_MODEL) and y.dtype == torch.bfloat16
        y.backward(_dev(d["dy"], "bf16"))
        what = f"moe_mlp rows={rows} "
        H.assert_close(_np(y), _np(ref_y), "bf16", what + "y")
        leaves = [x, gates, w1, w2] + ([v1] if glu else [])
        for name, t, g in zip(("dx", "dgates", "dw1", "dw2", "dv1"), leaves,
                              ref_grads):
            assert t.grad is not None and t.grad.shape == t.shape, name
            H.assert_close(_np(t.grad), _np(g), "bf16", what + name)
        outs.append(y.detach())
    assert _same(outs[0], outs[1]), "rows=None and rows=bound differ"


def test_explicit_rows_make_no_host_sync():
    """With explicit rows nothing between the router's output and the
    scattered result waits for the device."""
    c = R.case_inputs(CASE, HIDDEN, "bf16")
    r = c.route
    top = torch.from_numpy(R.routing(*CASE)).cuda()
    x = _dev(c.x, "bf16")
    w = torch.from_numpy(np.array(c.w32.reshape(r.tokens, r.top_k))).cuda()
    rows = ops.moe_rows_bound(r.tokens * r.top_k, CASE[2])
    ops.moe_route(top, CASE[2], rows)           # (first-use initialisation)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        route = ops.moe_route(top, CASE[2], rows)
        xp = ops.padded_gather(x, route)
        y = ops.padded_scatter(xp, route, w)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    ref, _ = R.scatter64(R.gather(c.x, r, rows), r, c.w32)
    H.assert_close(_np(y), ref, "bf16", "gather + scatter")
