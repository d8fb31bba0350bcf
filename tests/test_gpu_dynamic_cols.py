"""Dynamic casts with segments along a non-last dimension (csrc/dynamic_cols.hip): fused=True against the DEFINITION, the
last-dim call with fused=False on x.movedim(dim, -1).contiguous() moved back -- bit patterns of y, the scales and the zero points, no
tolerance.  The shapes are the smallest that reach each way the tile can go wrong (one vector of inner; a partial wave; the deepest
register class with an odd vector count; more than one workgroup along inner with a partial last one; the KIVI form; whole columns)."""
import pytest
import torch

from _data import bits_equal, make

pytestmark = pytest.mark.gpu

# (shape, dim, granularity, group size)
CASES = [((2, 32, 8), 1, "per_group", 16), ((3, 64, 72), 1, "per_group", 32), ((1, 512, 136), 1, "per_group", 256),
         ((2, 128, 1032), 1, "per_group", 128), ((1, 2, 64, 128), -2, "per_group", 32), ((64, 48), 0, "per_group", 64),
         ((64, 48), 0, "per_token", None), ((4, 16, 24), 1, "per_token", None)]
DTYPES = [torch.bfloat16, torch.float16, torch.float32]


@pytest.fixture
def ops(dmx, cuda):
    return dmx.ops


def _same(got, want):
    got, want = (got, want) if isinstance(got, tuple) else ((got,), (want,))
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.is_contiguous() and bits_equal(g, w) == 0


def _fixed(ops, x, fmt, gran, g, sym, dim, fused):
    if fused:
        return ops.dynamic_fixed_qdq(x, fmt, gran, g, sym, return_qparams=True, fused=True, dim=dim)
    xt = x.movedim(dim, -1).contiguous()
    y, sc, zp = ops.dynamic_fixed_qdq(xt, fmt, gran, g, sym, return_qparams=True, fused=False)
    back = lambda q: q.reshape(xt.shape[:-1] + (-1,)).movedim(-1, dim).contiguous()
    return y.movedim(-1, dim).contiguous(), back(sc), back(zp)


def _float(ops, x, fmt, gran, g, pow2, dim, fused):
    if fused:
        return ops.dynamic_float_qdq(x, fmt, gran, g, pow2, return_scale=True, fused=True, dim=dim)
    xt = x.movedim(dim, -1).contiguous()
    y, sc = ops.dynamic_float_qdq(xt, fmt, gran, g, pow2, return_scale=True, fused=False)
    return y.movedim(-1, dim).contiguous(), sc.reshape(xt.shape[:-1] + (-1,)).movedim(-1, dim).contiguous()


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("case", CASES, ids=str)
def test_fixed_cols_equal_the_definition(ops, case, dtype):
    shape, dim, gran, g = case
    x = make("heavy", shape, seed=3, dtype=dtype).cuda()
    for fmt in ("XP[4,0](CSN)", "XP[8,0](CSN)"):
        for sym in (False, True):
            _same(_fixed(ops, x, fmt, gran, g, sym, dim, True), _fixed(ops, x, fmt, gran, g, sym, dim, False))


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("case", CASES, ids=str)
def test_float_cols_equal_the_definition(ops, case, dtype):
    shape, dim, gran, g = case
    x = make("heavy", shape, seed=4, dtype=dtype).cuda()
    for fmt in ("FP[1|4|3,7](FN)", "FP[1|2|1,1](FN)"):
        for pow2 in (False, True):
            _same(_float(ops, x, fmt, gran, g, pow2, dim, True), _float(ops, x, fmt, gran, g, pow2, dim, False))


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_planted_columns_share_a_lane(ops, dtype):
    """adjacent columns of one lane's vector: an all-zero segment (scale eps: the division path), a NaN, a +Inf, an ordinary one"""
    x = make("normal", (2, 32, 16), seed=5, dtype=dtype)
    x[0, :16, 0] = 0.0
    x[0, 3, 1] = float("nan")
    x[0, 5, 2] = float("inf")
    x[1, 16:, 9] = 0.0
    x = x.cuda()
    for sym in (False, True):
        _same(_fixed(ops, x, "XP[8,0](CSN)", "per_group", 16, sym, 1, True), _fixed(ops, x, "XP[8,0](CSN)", "per_group", 16, sym, 1, False))
    _same(_float(ops, x, "FP[1|4|3,7](FN)", "per_group", 16, False, 1, True), _float(ops, x, "FP[1|4|3,7](FN)", "per_group", 16, False, 1, False))


def test_graph_replay_equals_eager(ops):
    x = make("heavy", (1, 2, 64, 128), seed=6, dtype=torch.bfloat16).cuda()
    eager = ops.dynamic_fixed_qdq(x, "XP[4,0](CSN)", "per_group", 32, fused=True, dim=-2)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ops.dynamic_fixed_qdq(x, "XP[4,0](CSN)", "per_group", 32, fused=True, dim=-2)   # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = ops.dynamic_fixed_qdq(x, "XP[4,0](CSN)", "per_group", 32, fused=True, dim=-2)
    for _ in range(3):
        y.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert bits_equal(y, eager) == 0


@pytest.mark.parametrize("shape,g", [((48, 16), 24), ((32, 3), 16)], ids=["S24", "inner3"])
def test_unsupported_geometry_refuses_fused_and_falls_back(ops, shape, g):
    x = make("normal", shape, seed=7, dtype=torch.bfloat16).cuda()
    with pytest.raises(NotImplementedError):
        ops.dynamic_fixed_qdq(x, "XP[8,0](CSN)", "per_group", g, fused=True, dim=0)
    got = ops.dynamic_fixed_qdq(x, "XP[8,0](CSN)", "per_group", g, return_qparams=True, dim=0)
    _same(got, _fixed(ops, x, "XP[8,0](CSN)", "per_group", g, False, 0, False))


def test_castto_with_dim_equals_the_op(dmx, ops):
    x = make("heavy", (1, 2, 64, 128), seed=8, dtype=torch.bfloat16).cuda()
    c = dmx.CastTo(format="XP[4,0](CSN)").to("cuda")
    c.set_dynamic({"per_group": 32, "dim": -2})
    assert c.dynamic == {"per_group": 32, "dim": -2} and not [k for k in c.state_dict() if "dynamic" in k]
    before = dict(dmx._front._dynamic_cols_routes)
    want = ops.dynamic_fixed_qdq(x, "XP[4,0](CSN)", "per_group", 32, symmetric_qscheme=c.qscheme in dmx.cast._SYMMETRIC, dim=-2)
    _same(c(x), want)
    assert dmx._front._dynamic_cols_routes["fused"] == before["fused"] + 2   # (the op and the cast both ran the column kernel)
    f = dmx.CastTo(format="FP[1|4|3,7](FN)").to("cuda")
    f.set_scaling({"per_group": 32, "dim": -2})
    _same(f(x), ops.dynamic_float_qdq(x, "FP[1|4|3,7](FN)", "per_group", 32, dim=-2))
    assert f.scaling == {"per_group": 32, "dim": -2}
