"""GPU: the MoE chains of sputnik_amd/ops.py with explicit `rows`, forward
and backward, replayed from a captured graph under routings other than the
one they were captured with, and run on memory that earlier runs left dirty.

What is pinned here is one property: the result of a chain depends on its
current inputs only, whatever the routing at capture time was and whatever
its memory held before. A replay freezes the launch geometry, every address
and every decision taken on the host; only device data may differ. The
padded layout has rows nobody owns (every expert's padding to a multiple of
128, and the slack rows between padded_bins[-1] and `rows`, which
expert_topology gives to the last expert); in a graph's private pool they
hold the previous replay's values.

The oracle is tests/test_gpu_moe_ops.py's: the dense fp32 torch layer under
helpers.assert_close, here at five routings (tests/moe_replay_ref.py) with
the operands of _mlp_data, whose docstring's argument is about the products'
terms and holds for any routing. Everything else is bit equality: a replay
against an eager run of the same inputs on fresh leaves, a run on dirty
memory against the first run. The kernels' own numerics are held by their
own files and are not repeated.

Capture protocol of every graph in this file (_Captured): static tensors for
every input, three eager iterations on a side stream, grads set to None,
then forward and backward inside torch.cuda.graph; y and the leaves' .grad
are the static outputs. No environment variable is set. NaN inputs are
ordinary data for these kernels; a "poison" replay fills the pool's
intermediates with NaN before the next finite replay.
"""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import sputnik_amd as sp  # noqa: E402
from sputnik_amd import ops  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests import moe_ref as M  # noqa: E402
from tests import moe_replay_ref as RR  # noqa: E402
from tests import test_gpu_bias_ops as BO  # noqa: E402
from tests import test_gpu_router_ops as RO  # noqa: E402
from tests.test_gpu_moe_ops import (D_MODEL, EXPERTS, FFN, TOKENS,  # noqa: E402
                                    TOP_K, _dense_reference, _mlp_data)

pytestmark = pytest.mark.gpu

ROWS = ops.moe_rows_bound(TOKENS * TOP_K, EXPERTS)
_INT = {2: torch.int16, 4: torch.int32}
_CACHE = {}


def _routings():
    if "tops" not in _CACHE:
        assert ROWS == 1152
        _CACHE["tops"] = RR.routings(_mlp_data()["top"], EXPERTS)
    return _CACHE["tops"]


def _np(t):
    return t.detach().float().cpu().numpy()


def _bits(t):
    if not t.is_floating_point():
        return t
    return t.contiguous().view(_INT[t.element_size()])


def _assert_same(got, want, what):
    """Two result lists [(name, tensor)] equal bit for bit."""
    assert [n for n, _ in got] == [n for n, _ in want], what
    for (name, a), (_, b) in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name)
        assert torch.equal(_bits(a), _bits(b)), f"{what}: {name} differs"


def _assert_finite(res, what):
    for name, t in res:
        if t.is_floating_point():
            assert torch.isfinite(t.float()).all(), f"{what}: {name}"


def _assert_plus_zero(t, what):
    assert int(_bits(t).count_nonzero()) == 0, f"{what} is not +0 everywhere"


def _get(res, name):
    return dict(res)[name]


# ---- eager run, capture, replay ---------------------------------------------

def _fresh(values, leaves):
    return {k: v.detach().clone().requires_grad_(k in leaves)
            for k, v in values.items()}


def _results(t, outs, leaves):
    return ([(name, o.detach()) for name, o in outs]
            + [("d" + k, t[k].grad) for k in leaves])


def _eager(step, values, leaves):
    """step on fresh leaves on the current stream: [(name, tensor)]."""
    t = _fresh(values, leaves)
    res = _results(t, step(t), leaves)
    for name, r in res:
        assert r is not None, name
    return res


class _Captured:
    """step, forward and backward, captured once over static tensors."""

    def __init__(self, step, values, leaves):
        self.t = t = _fresh(values, leaves)
        # (one side stream for every warm-up of the file)
        side = _CACHE.setdefault("side", torch.cuda.Stream())
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                for k in leaves:
                    t[k].grad = None
                step(t)
        torch.cuda.current_stream().wait_stream(side)
        for k in leaves:
            t[k].grad = None
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            outs = step(t)
        self.static = _results(t, outs, leaves)
        for name, r in self.static:
            assert r is not None, name

    def replay(self, values):
        with torch.no_grad():
            for k, v in values.items():
                self.t[k].copy_(v)
        self.graph.replay()
        torch.cuda.synchronize()
        return [(name, r.clone()) for name, r in self.static]

    def close(self):
        del self.graph, self.static, self.t
        sp.capture_workspaces()  # (frees what the dead graph's launches held)


def _run_sequence(step, leaves, sequence, eager_of, what, after=None):
    """Captures step at sequence[0]'s values and replays the sequence.
    sequence: [(label, values, finite)]; eager_of(label, values) the eager
    result of a finite entry. Checks every finite replay against it bit for
    bit, finiteness right after a poisoned replay, a change in y between
    consecutive finite replays and equal results wherever a label repeats.
    after(label, values, replay result) adds a caller's checks.
    Returns the finite replays' results by label."""
    sp.pair_errors()                                    # (clears the count)
    cap = _Captured(step, sequence[0][1], leaves)
    seen, prev_y, poisoned = {}, None, False
    try:
        for label, values, finite in sequence:
            got = cap.replay(values)
            if not finite:
                poisoned = True
                continue
            where = f"{what}, replay {label}"
            want = eager_of(label, values)
            _assert_same(got, want, where)
            if poisoned:
                _assert_finite(got, where + " (after the poisoned replay)")
                poisoned = False
            y = _get(got, "y")
            assert y.abs().max() > 0, where
            if prev_y is not None:
                assert not torch.equal(_bits(y), _bits(prev_y)), (
                    f"{where}: y is the previous replay's")
            prev_y = y
            if label in seen:
                _assert_same(got, seen[label], where + " (repeated)")
            seen[label] = got
            if after is not None:
                after(label, values, got)
        assert sp.pair_errors() == 0, what
    finally:
        cap.close()
    return seen


# ---- 1. the routings --------------------------------------------------------

def test_routings_cover_the_padded_layouts():
    """Host only: the conditions of moe_replay_ref.check, and the slack of
    0 to 4 block rows they give at this shape."""
    tops = _routings()
    slack = {k: (ROWS - RR.padded_rows(v, EXPERTS)) // 128
             for k, v in tops.items()}
    assert slack["last"] == slack["first"] == 4
    assert set(slack.values()) <= set(range(5))
    assert len(set(slack.values())) >= 3


# ---- 2. eager correctness at every routing ----------------------------------

def _mlp_values(glu, top, x_nan=False):
    d = _mlp_data()
    v = {k: RO._bf16(d[k], False) for k in ("x", "w1", "w2", "dy")}
    if glu:
        v["v1"] = RO._bf16(d["v1"], False)
    if x_nan:
        v["x"] = torch.full_like(v["x"], float("nan"))
    v["gates"] = torch.from_numpy(np.array(d["gates"])).cuda()
    v["top"] = torch.from_numpy(np.array(top)).cuda()
    return v


def _mlp_leaves(glu):
    return ["x", "gates", "w1", "w2"] + (["v1"] if glu else [])


def _mlp_step(device_sort):
    def step(t):
        top = t["top"]
        if device_sort:
            top = ops.moe_device_route(top, EXPERTS, ROWS)
        y = ops.moe_mlp(t["x"], top, t["gates"], t["w1"], t["w2"], EXPERTS,
                        v1=t.get("v1"), rows=ROWS)
        y.backward(t["dy"])
        return [("y", y)]
    return step


def _mlp_eager(glu, name, device_sort):
    """The eager result at one routing, once: the oracle-checked twin of
    the replay tests."""
    key = ("mlp", glu, name, device_sort)
    if key not in _CACHE:
        _CACHE[key] = _eager(_mlp_step(device_sort),
                             _mlp_values(glu, _routings()[name]),
                             _mlp_leaves(glu))
    return _CACHE[key]


def _dense(glu, name):
    key = ("dense", glu, name)
    if key not in _CACHE:
        y, grads = _dense_reference({**_mlp_data(), "top": _routings()[name]},
                                    glu)
        _CACHE[key] = [_np(y)] + [_np(g) for g in grads]
    return _CACHE[key]


def _assert_idle_expert_is_zero(res, what):
    """Routing `first`: the last expert has no token and owns every slack
    row; its slices of the weight gradients are +0."""
    own = slice((EXPERTS - 1) * FFN, EXPERTS * FFN)
    for name, t in res:
        if name in ("dw1", "dv1"):
            _assert_plus_zero(t[:, own], f"{what}: {name} of the idle expert")
        elif name in ("dw2", "dw1t"):
            _assert_plus_zero(t[own], f"{what}: {name} of the idle expert")


@pytest.mark.parametrize("device_sort", [False, True],
                         ids=["moe_route", "moe_device_route"])
@pytest.mark.parametrize("glu", [False, True], ids=["mlp", "glu"])
@pytest.mark.parametrize("name", RR.NAMES)
def test_moe_mlp_against_the_dense_layer_at_every_routing(name, glu,
                                                          device_sort):
    res = _mlp_eager(glu, name, device_sort)
    ref = _dense(glu, name)
    assert [n for n, _ in res] == ["y", "dx", "dgates", "dw1", "dw2"] + \
        (["dv1"] if glu else [])
    for (what, t), r in zip(res, ref):
        H.assert_close(_np(t), r, "bf16", f"moe_mlp at {name}: {what}")
    assert _get(res, "y").shape == (TOKENS, D_MODEL)
    if name == "first":
        _assert_idle_expert_is_zero(res, "moe_mlp at first")


# ---- 3. eager runs on dirty memory ------------------------------------------

@pytest.mark.parametrize("glu", [False, True], ids=["mlp", "glu"])
def test_moe_mlp_on_memory_a_nan_run_left_behind(glu):
    """random, then `last` with x all NaN (every intermediate of the chain
    is NaN in the caching allocator's blocks), its tensors dropped, then
    random again: the same bits as the first run, all finite."""
    tops, step, leaves = _routings(), _mlp_step(True), _mlp_leaves(glu)
    first = [(n, t.clone()) for n, t in
             _eager(step, _mlp_values(glu, tops["random"]), leaves)]
    poisoned = _eager(step, _mlp_values(glu, tops["last"], x_nan=True), leaves)
    assert torch.isnan(_get(poisoned, "y").float()).all()
    assert torch.isnan(_get(poisoned, "dw2").float()).any()
    del poisoned
    again = _eager(step, _mlp_values(glu, tops["random"]), leaves)
    _assert_same(again, first, "moe_mlp on dirty memory")
    _assert_finite(again, "moe_mlp on dirty memory")


# ---- 4. moe_mlp captured, forward and backward ------------------------------

@pytest.mark.parametrize("device_sort", [False, True],
                         ids=["moe_route", "moe_device_route"])
@pytest.mark.parametrize("glu", [False, True], ids=["mlp", "glu"])
def test_moe_mlp_graph_replayed_under_new_routings(glu, device_sort):
    tops = _routings()
    order = ["random", "last", None, "exact", "empty", "first", "random"]
    sequence = [
        (name, _mlp_values(glu, tops[name]), True) if name else
        ("poison", _mlp_values(glu, tops["first"], x_nan=True), False)
        for name in order]

    def after(label, _values, got):
        if label == "first":
            _assert_idle_expert_is_zero(got, "moe_mlp replayed at first")

    seen = _run_sequence(_mlp_step(device_sort), _mlp_leaves(glu), sequence,
                         lambda label, _v: _mlp_eager(glu, label, device_sort),
                         f"moe_mlp graph glu={glu} device_sort={device_sort}",
                         after)
    assert sorted(seen) == sorted(RR.NAMES)


# ---- 5. the layers, captured with backward ----------------------------------

WINNERS = (2, 3)


def _draw(seed, tokens, ones_column=False):
    """x of _mlp_data's recipe, another draw: {-1, 0, 1} as bf16."""
    x = np.random.default_rng([53, seed]).integers(
        -1, 2, (tokens, D_MODEL)).astype(np.float32)
    if ones_column:
        x[:, 0] = 1
    return torch.from_numpy(x).bfloat16().cuda()


def _two_winners(wr):
    """A router weight under which experts 2 and 3 win every token of an x
    whose column 0 is 1: their rows are 8 and 6 in column 0 and zero
    elsewhere (logits 8 and 6, for the sigmoid router both in one group), the
    other rows keep their {-1, 0, 1} / 16 entries with column 0 cleared
    (logits a sum of 255 terms of at most 1/16, a few units at most on
    these draws). The tests assert the outcome: experts 0 and 1 are empty."""
    w = wr.detach().clone()
    w[:, 0] = 0
    for e, v in zip(WINNERS, (8.0, 6.0)):
        w[e] = 0
        w[e, 0] = v
    return w


def _layer_case(kind):
    """(values, leaves, step, router) of one layer. router(values) is the
    eager choice of that layer's router, top_experts [tokens, top_k]."""
    glu = kind in ("glu-bf16", "glu-fp32-scores", "bias", "aux")
    fp32 = kind in ("mlp-fp32", "glu-fp32-scores")
    rd = torch.float32 if fp32 else None
    rows = ROWS
    if kind == "bias":
        d = BO._moe_data()
        v = {k: t.detach()
             for k, t in BO._layer_operands(d, True, True).items()}
        v["dy"] = BO._dev(d["dy"], "bf16")
        top_k, rows = BO.TOP_K, ops.moe_rows_bound(BO.M_TOKENS * BO.TOP_K,
                                                   BO.EXPERTS)
        assert (BO.EXPERTS, BO.D_MODEL) == (EXPERTS, D_MODEL)
    else:
        d = _mlp_data()
        x, wr, w1, w2, v1 = RO._layer_operands(d, glu, rd)
        v = {"x": x.detach(), "wr": wr.detach(), "w1": w1.detach(),
             "w2": w2.detach(), "dy": RO._bf16(d["dy"], False)}
        if glu:
            v["v1"] = v1.detach()
        top_k = TOP_K
    leaves = [k for k in v if k != "dy"]
    score = kind == "score"
    if score:
        v["router_bias"] = torch.zeros(EXPERTS, device="cuda")
    common = dict(rows=rows, normalize=True, router_dtype=rd)

    def step(t):
        args = (t["x"], t["wr"], t["w1"], t["w2"], top_k)
        outs = []
        if kind == "bias":
            y = ops.moe_layer_bias(*args, v1=t["v1"], b1=t["b1"],
                                   bv1=t["bv1"], b2=t["b2"], **common)
        elif kind == "aux":
            y, aux = ops.moe_layer_aux(*args, v1=t["v1"], **common)
            loss = (ops.load_balancing_loss(aux.score_sums,
                                            aux.tokens_per_expert, aux.tokens,
                                            aux.top_k)
                    + ops.router_z_loss(aux.z_sum, aux.tokens))
            torch.autograd.backward([y, loss], [t["dy"], None])
            return [("y", y), ("loss", loss),
                    ("tokens_per_expert", aux.tokens_per_expert)]
        elif score:
            y, scores, tpe = ops.moe_score_layer(
                *args, return_scores=True, router_bias=t["router_bias"],
                num_groups=2, topk_groups=1, **common)
            outs = [("scores", scores), ("tokens_per_expert", tpe)]
        elif kind == "glu-fp32-scores":
            y, scores, tpe = ops.moe_layer(*args, v1=t["v1"],
                                           return_scores=True, **common)
            outs = [("scores", scores), ("tokens_per_expert", tpe)]
        else:
            y = ops.moe_layer(*args, v1=t.get("v1"), **common)
        y.backward(t["dy"])
        return [("y", y)] + outs

    def router(values):
        with torch.no_grad():
            x, wr = values["x"], values["wr"]
            dt = x.dtype if rd is None else rd
            logits = x.to(dt) @ wr.to(dt).t()
            if score:
                return ops.moe_score_router(logits, top_k,
                                            values["router_bias"], 2, 1,
                                            True)[1]
            return ops.moe_router(logits, top_k, True)[1]

    return v, leaves, step, router


LAYERS = ["mlp-bf16", "mlp-fp32", "glu-bf16", "glu-fp32-scores", "bias", "aux",
          "score"]


@pytest.mark.parametrize("kind", LAYERS)
def test_layer_graph_replayed_under_new_routings(kind):
    """The layers from activations to output, where the routing is the
    router's and moves with the inputs: other draws of x; a router weight
    under which two experts win every token (_two_winners); for the sigmoid
    router, a replay in which only the selection bias changes. The poisoned
    replay has NaN expert weights and dy under finite x and router weight,
    so its routing is an ordinary one."""
    base, leaves, step, router = _layer_case(kind)
    tokens = int(base["x"].shape[0])
    nan = {k: torch.full_like(base[k], float("nan"))
           for k in ("w1", "w2", "v1", "dy") if k in base}
    sequence = [
        ("first draw", base, True),
        ("draw 1", {**base, "x": _draw(1, tokens)}, True),
        ("poison", {**base, "x": _draw(2, tokens), **nan}, False),
        ("draw 3", {**base, "x": _draw(3, tokens)}, True)]
    if kind == "score":
        bias = torch.tensor([2.0, 2.0, 0.0, 0.0], device="cuda")
        sequence.append(("bias alone", {**base, "x": _draw(3, tokens),
                                        "router_bias": bias}, True))
    sequence += [
        ("two winners", {**base, "x": _draw(4, tokens, ones_column=True),
                         "wr": _two_winners(base["wr"])}, True),
        ("first draw", base, True)]
    counts = []

    def eager_of(_label, values):
        return _eager(step, values, leaves)

    def after(label, values, got):
        tpe = torch.bincount(router(values).reshape(-1).long(),
                             minlength=EXPERTS)
        if "tokens_per_expert" in dict(got):
            assert torch.equal(_get(got, "tokens_per_expert").long(), tpe), (
                kind, label)
        assert int(tpe.sum()) == tokens * 2
        if counts:
            assert not torch.equal(tpe, counts[-1]), (
                f"{kind}, replay {label}: the routing did not move")
        counts.append(tpe)
        if label == "two winners":
            want = [0] * EXPERTS
            for e in WINNERS:
                want[e] = tokens
            assert tpe.tolist() == want, (kind, tpe.tolist())
        if label == "bias alone":
            assert tpe.tolist() == [tokens, tokens, 0, 0], tpe.tolist()

    _run_sequence(step, leaves, sequence, eager_of, f"layer {kind}", after)
    assert len(counts) == len(sequence) - 1


# ---- 6. fp8 training with slack rows ----------------------------------------

FP8_LEAVES = ["x", "gates", "w1t", "w2"]


def _fp8_values(top, x_nan=False):
    """Real-valued operands (moe_ref.values: magnitudes 2^-10 to 4), so
    that the quantisers' scales differ from tile to tile."""
    if "fp8" not in _CACHE:
        hidden = EXPERTS * FFN
        v = {"x": M.values((TOKENS, D_MODEL), "bf16", [61]),
             "w1t": M.values((hidden, D_MODEL), "bf16", [62]) / np.float32(16),
             "w2": M.values((hidden, D_MODEL), "bf16", [63]) / np.float32(16),
             "dy": M.values((TOKENS, D_MODEL), "bf16", [64])}
        v = {k: torch.from_numpy(np.array(a)).bfloat16().cuda()
             for k, a in v.items()}
        v["gates"] = torch.from_numpy(np.array(_mlp_data()["gates"])).cuda()
        _CACHE["fp8"] = v
    v = dict(_CACHE["fp8"])
    if x_nan:
        v["x"] = torch.full_like(v["x"], float("nan"))
    v["top"] = torch.from_numpy(np.array(top)).cuda()
    return v


def _fp8_step(mode, rows):
    def step(t):
        y = ops.moe_mlp_fp8_train(t["x"], t["top"], t["gates"], t["w1t"],
                                  t["w2"], EXPERTS, rows=rows, accumulate=mode)
        y.backward(t["dy"])
        return [("y", y)]
    return step


def _fp8_eager(mode, name):
    key = ("fp8", mode, name)
    if key not in _CACHE:
        _CACHE[key] = _eager(_fp8_step(mode, ROWS),
                             _fp8_values(_routings()[name]), FP8_LEAVES)
    return _CACHE[key]


@pytest.mark.parametrize("name", ["random", "last", "first"])
@pytest.mark.parametrize("mode", ["fp32", "fast"])
def test_moe_mlp_fp8_train_slack_rows_change_nothing(mode, name):
    """rows = moe_rows_bound against the exact row count, bit for bit in y
    and the four gradients: the weight gradients' extra 128-token intervals
    hold all-zero bytes, and fma(s, 0, acc) leaves acc alone."""
    bound = _fp8_eager(mode, name)
    exact = _eager(_fp8_step(mode, None), _fp8_values(_routings()[name]),
                   FP8_LEAVES)
    _assert_same(bound, exact, f"moe_mlp_fp8_train {mode} at {name}")
    _assert_finite(bound, f"moe_mlp_fp8_train {mode} at {name}")
    for grad in ("dx", "dgates", "dw1t", "dw2"):
        assert _get(bound, grad).abs().max() > 0, grad
    if name == "first":
        _assert_idle_expert_is_zero(bound, "moe_mlp_fp8_train at first")


@pytest.mark.parametrize("mode", ["fp32", "fast"])
def test_moe_mlp_fp8_train_graph_replayed_under_new_routings(mode):
    tops = _routings()
    order = ["random", "last", None, "first", "random"]
    sequence = [
        (name, _fp8_values(tops[name]), True) if name else
        ("poison", _fp8_values(tops["first"], x_nan=True), False)
        for name in order]

    def after(label, _values, got):
        if label == "first":
            _assert_idle_expert_is_zero(got, "moe_mlp_fp8_train replayed at "
                                             "first")

    _run_sequence(_fp8_step(mode, ROWS), FP8_LEAVES, sequence,
                  lambda label, _v: _fp8_eager(mode, label),
                  f"moe_mlp_fp8_train graph {mode}", after)
