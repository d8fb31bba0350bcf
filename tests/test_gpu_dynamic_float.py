"""GPU tests of the dynamic scaled float cast (csrc/dynamic_float.hip, ops.dynamic_float_qdq, CastTo.set_scaling): the
fused kernel against the CPU checker of tests/_dynamic_float_ref.py (the definition, with the oracle's float cast) and against the
library's own chain of launches on the GPU, bit for bit, the scales included.  The kernel's grid does not loop (a wave takes a fixed
number of vectors; a row or a tile is a wave's or a workgroup's), so there is no multi-tile case to force with DMXQ_PLAN_CUS."""
import pytest
import torch
import torch.nn.functional as F

import _dynamic_float_ref as R
import _large_cases as LC
from _data import bits_equal, make

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=["bf16", "f16", "f32"])
NAMES = ("e4m3", "e4m3_flush", "e5m2", "e2m1")
E4M3 = R.SHORTHAND["e4m3"]


def routes_of(ops):
    """the front end's private route counter (dmx.ops re-exports a front-end module; ops.front(binding) IS one)"""
    return ops._dynamic_float_routes if hasattr(ops, "_dynamic_float_routes") else ops._front._dynamic_float_routes


def fused(ops, x, fmt, granularity="per_token", g=None, pow2=False, **kw):
    """ops.dynamic_float_qdq(..., fused=True), asserting on the host-side route counter that the kernel ran (and the chain did not)"""
    before = dict(routes_of(ops))
    out = ops.dynamic_float_qdq(x, fmt, granularity, g, pow2_scale=pow2, fused=True, **kw)
    assert routes_of(ops)["fused"] == before["fused"] + 1 and routes_of(ops)["chain"] == before["chain"]
    return out


def chain(ops, x, fmt, granularity="per_token", g=None, pow2=False, **kw):
    before = dict(routes_of(ops))
    out = ops.dynamic_float_qdq(x, fmt, granularity, g, pow2_scale=pow2, fused=False, **kw)
    assert routes_of(ops)["chain"] == before["chain"] + 1 and routes_of(ops)["fused"] == before["fused"]
    return out


def check(oracle, ops, x, name, granularity, g, pow2, cuda, rows=None):
    """kernel == checker (the rows `rows` of dim 0 only, where the others hold NaN / Inf) and kernel == chain, outputs and scales"""
    xd = x.to(cuda)
    y, sc = fused(ops, xd, R.SHORTHAND[name], granularity, g, pow2, return_scale=True)
    yc, scc = chain(ops, xd, R.SHORTHAND[name], granularity, g, pow2, return_scale=True)
    assert y.dtype == x.dtype and y.shape == x.shape and sc.dtype == F32 and sc.shape == scc.shape
    what = (name, granularity, g, pow2, tuple(x.shape), x.dtype)
    assert bits_equal(sc, scc) == 0, what
    assert bits_equal(y, yc) == 0, what
    xr = x if rows is None else x[rows]
    want, wsc = R.dynamic_float_ref(oracle, xr, R.FORMATS[name], granularity, g, pow2)
    got, gsc = (y.cpu(), sc.cpu()) if rows is None else (y.cpu()[rows], None)
    if gsc is not None:
        assert gsc.shape == wsc.shape and bits_equal(gsc, wsc) == 0, what
    assert bits_equal(got, want) == 0, what
    return y, sc


# ---------------------------------------------------------------------------------------------------- the kernel's geometries
@pytest.mark.parametrize("name", NAMES)
@DTYPES
def test_groups(dmx, oracle, cuda, dtype, name):
    """segments inside a wave: g = 16, 32, 128, 256 on [3, 2 g] (a single partly filled wave) and [257, 1024] (several workgroups, the
    last one partly past the end), both scale rules"""
    for g in (16, 32, 128, 256):
        for shape in ((3, 2 * g), (257, 1024)):
            x = make("heavy", shape, seed=g + shape[0], dtype=dtype, block=g)
            for pow2 in (False, True):
                check(oracle, dmx.ops, x, name, "per_group", g, pow2, cuda)


def test_groups_deep_grid(dmx, oracle, cuda):
    """[8200, 1024] bf16 = 1,049,600 vectors, more than 2^19: the four-vectors-per-lane build of the group kernel, whose last workgroup
    is only partly filled; 16 .. 256 elements per segment (up to 524,800 segments: the chain runs in pieces)"""
    x = make("heavy", (8200, 1024), seed=3, dtype=BF16)
    for g, pow2 in ((16, False), (32, True), (128, False), (256, True)):
        check(oracle, dmx.ops, x, "e4m3", "per_group", g, pow2, cuda)


@DTYPES
@pytest.mark.parametrize("L", [48, 768, 4096, 8192, 8200, 16384])
def test_whole_rows(dmx, oracle, cuda, L, dtype):
    """short rows (48: lanes idle), a wave per row (768; 4096: 8 sixteen-bit / 16 fp32 vectors per lane, the last a wave takes), a
    workgroup per row (8192, 8200 with idle slots, 16384 with every slot filled)"""
    want_cls = {48: "short_row", 768: "wave_row", 4096: "wave_row"}.get(L, "block_row")
    assert dmx.ops.dynamic_float_class(L, dtype) == want_cls
    x = make("heavy", (5 if L >= 8192 else 67, L), seed=L, dtype=dtype, block=64)
    for name in NAMES:
        for pow2 in (False, True):
            check(oracle, dmx.ops, x, name, "per_token", None, pow2, cuda)


@DTYPES
@pytest.mark.parametrize("g", [32, 64, 128])
def test_tiles(dmx, oracle, cuda, g, dtype):
    """one tile, 2 x 3 tiles (a workgroup of four wave tiles partly past the end), a batch of two matrices; [384, 640] at g = 128"""
    assert dmx.ops.dynamic_float_class(g, dtype, "per_tile") == "tile"
    shapes = [(g, g), (2 * g, 3 * g), (2, 128, 256)] + ([(384, 640)] if g == 128 else [])
    for shape in shapes:
        x = make("heavy", shape, seed=g + len(shape), dtype=dtype, block=32)
        for name in NAMES:
            for pow2 in (False, True):
                y, sc = check(oracle, dmx.ops, x, name, "per_tile", g, pow2, cuda)
                assert tuple(sc.shape) == tuple(shape[:-2]) + (shape[-2] // g, shape[-1] // g)


def test_per_tensor(dmx, oracle, cuda):
    for shape, kernel in (((4, 8, 96), True), ((300, 1000), False)):     # 3072 elements: one row on the kernel; 300 000: the chain
        x = make("heavy", shape, seed=9, dtype=BF16)
        if kernel:
            y, sc = check(oracle, dmx.ops, x, "e4m3", "per_tensor", None, False, cuda)
        else:
            with pytest.raises(NotImplementedError):
                dmx.ops.dynamic_float_qdq(x.to(cuda), E4M3, "per_tensor", fused=True)
            y, sc = dmx.ops.dynamic_float_qdq(x.to(cuda), E4M3, "per_tensor", return_scale=True)
            want, wsc = R.dynamic_float_ref(oracle, x, R.FORMATS["e4m3"], "per_tensor")
            assert bits_equal(y.cpu(), want) == 0 and bits_equal(sc.cpu(), wsc) == 0
        assert sc.shape == (1,)


# ---------------------------------------------------------------------------------------------------- planted segments
REGIMES = [("group", "per_group", 64, (12, 64)), ("short_row", "per_token", None, (12, 48)), ("wave_row", "per_token", None, (12, 776)),
           ("block_row", "per_token", None, (12, 8200)), ("tile", "per_tile", 32, (128, 96))]
ZERO, NAN, INF, DENORMAL, HUGE, TINY_SCALE, BIG_SCALE, NEG_ZERO = range(8)
FINITE = [ZERO, DENORMAL, HUGE, TINY_SCALE, BIG_SCALE, NEG_ZERO, 8, 9, 10, 11]


def planted_segments(S, dtype, seed):
    """twelve segments of S elements: all zero; one NaN; one Inf; all denormal; one element near 3e38 beside tiny ones (its scale is
    above 2^20: the division redo); a maximum of 1e-6 (a scale below 2^-20 for every format here: the redo again); a maximum of 1e30 (3000 in f16); all -0.0; four plain"""
    seg = make("normal", (12, S), seed=seed, dtype=F32)
    seg[ZERO] = 0.0
    seg[NAN, S // 3] = float("nan")
    seg[INF, S // 2] = float("-inf")
    seg[DENORMAL] = seg[DENORMAL].sign() * (1e-40 if dtype != F16 else 6e-8)
    seg[HUGE] = seg[HUGE] * 1e-30
    seg[HUGE, 5] = 3e38 if dtype != F16 else 65000.0
    seg[TINY_SCALE] = (seg[TINY_SCALE] * 1e-7).clamp(-1e-6, 1e-6)
    seg[TINY_SCALE, 7] = -1e-6
    seg[BIG_SCALE, 11] = 1e30 if dtype != F16 else 3000.0
    seg[NEG_ZERO] = -0.0
    out = seg.to(dtype)
    # the canonical quiet NaN of the dtype, by its bits (a vectorised float32 -> bf16 conversion may hand out the all-ones pattern, which
    # the reference's rounding carries over to +0 instead of saturating)
    it, bits = {BF16: (torch.int16, 0x7FC0), F16: (torch.int16, 0x7E00), F32: (torch.int32, 0x7FC00000)}[dtype]
    out.view(it)[NAN, S // 3] = bits
    return out


@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=["bf16", "f16", "f32"])
@pytest.mark.parametrize("regime,granularity,g,shape", REGIMES, ids=[r[0] for r in REGIMES])
def test_planted_segments(dmx, oracle, cuda, regime, granularity, g, shape, dtype):
    zeros = torch.zeros(shape, dtype=dtype)
    seg0, back, _ = R.to_segments(zeros, granularity, g)
    assert seg0.shape[0] == 12
    S = seg0.shape[1]
    seg = planted_segments(S, dtype, seed=len(regime))
    x = back(seg).contiguous()
    assert dmx.ops.dynamic_float_class(g or S, dtype, granularity) == regime
    xd = x.to(cuda)
    for name in ("e4m3", "e4m3_flush", "e2m1"):
        man, exp, bias, flush = R.FORMATS[name]
        for pow2 in (False, True):
            y, sc = fused(dmx.ops, xd, R.SHORTHAND[name], granularity, g, pow2, return_scale=True)
            yc, scc = chain(dmx.ops, xd, R.SHORTHAND[name], granularity, g, pow2, return_scale=True)
            what = (name, pow2)
            assert bits_equal(sc, scc) == 0 and bits_equal(y, yc) == 0, what          # everything, NaN and Inf segments included
            s = sc.reshape(-1).cpu()
            yseg = R.to_segments(y.cpu(), granularity, g)[0]
            # the definition's stated outcomes: scale 1 for an all-zero, a NaN and an Inf segment, whose elements then take the STATIC cast
            assert s[[ZERO, NAN, INF, NEG_ZERO]].tolist() == [1.0] * 4, what
            static = dmx.ops.float_qdq(seg[[ZERO, NAN, INF, NEG_ZERO]].to(cuda).float(), man, exp, bias, flush).to(dtype).cpu()
            assert bits_equal(yseg[[ZERO, NAN, INF, NEG_ZERO]], static) == 0, what
            fmax = R.FMAX[name]
            assert float(yseg[NAN, S // 3]) == fmax and float(yseg[INF, S // 2]) == -fmax, what
            # no NaN anywhere; no Inf either, except that the element near 3e38 may round up past the largest finite value (its quotient
            # rounds up on the format's grid and, under pow2_scale, so does its scale: 4 x 2^126 for FP[1|2|1,1])
            others = [r for r in range(12) if r != HUGE]
            assert not bool(torch.isnan(yseg.float()).any()) and bool(torch.isfinite(yseg[others].float()).all()), what
            assert float(s[TINY_SCALE]) < 2.0 ** -20 and (float(s[BIG_SCALE]) > 2.0 ** 20 or dtype == F16), what
            # the finite segments against the checker, scales included
            want, wsc = R.dynamic_float_ref(oracle, seg[FINITE], R.FORMATS[name], "per_token", None, pow2)
            assert bits_equal(s[FINITE], wsc) == 0, what
            assert bits_equal(yseg[FINITE], want) == 0, what


# ---------------------------------------------------------------------------------------------------- fallbacks, bindings
def test_fallbacks_are_the_chain_and_fused_true_raises(dmx, oracle, cuda):
    ops = dmx.ops
    base = make("heavy", (96, 1056), seed=5, dtype=BF16)
    unaligned = base.to(cuda).reshape(-1)[4:4 + 96 * 1024].reshape(96, 1024)       # 8 bytes past a 16-byte boundary
    assert unaligned.data_ptr() % 16 == 8 and unaligned.is_contiguous()
    x = base[:, :1024].contiguous().to(cuda)
    cases = [("bf16->f32", x, E4M3, "per_token", None, {"out_dtype": F32}),
             ("stochastic", x, "FP[1|4|3,7](_S)", "per_token", None, {"seed": 1234}),
             ("g=48", base[:, :960].contiguous().to(cuda), E4M3, "per_group", 48, {}),
             ("unaligned", unaligned, E4M3, "per_token", None, {}),
             ("tile=48", base[:, :960].contiguous().to(cuda), E4M3, "per_tile", 48, {}),
             ("L=1004", base[:, :1004].contiguous().to(cuda), E4M3, "per_token", None, {})]
    for name, t, fmt, granularity, g, kw in cases:
        with pytest.raises(NotImplementedError):
            ops.dynamic_float_qdq(t, fmt, granularity, g, fused=True, **kw)
        routes = dict(routes_of(ops))
        got = ops.dynamic_float_qdq(t, fmt, granularity, g, **kw)                 # fused=None: falls back
        assert routes_of(ops)["chain"] == routes["chain"] + 1 and routes_of(ops)["fused"] == routes["fused"], name
        assert got.shape == t.shape and got.dtype == kw.get("out_dtype", t.dtype), name
        assert bits_equal(got, chain(ops, t, fmt, granularity, g, **kw)) == 0, name
        if name == "stochastic":     # (an explicit seed: the same draws on both runs; every element between its two neighbours)
            lo = ops.dynamic_float_qdq(t, "FP[1|4|3,7](_D)", granularity, g, fused=False).float()
            hi = ops.dynamic_float_qdq(t, "FP[1|4|3,7](_U)", granularity, g, fused=False).float()
            gf = got.float()
            assert bool(((gf == lo) | (gf == hi)).all()) and bool((gf != lo).any()) and bool((gf != hi).any()), name
            continue
        want, _ = R.dynamic_float_ref(oracle, t.cpu(), R.FORMATS["e4m3"], granularity, g, False, kw.get("out_dtype"))
        assert bits_equal(got.cpu(), want) == 0, name
    # the C entry itself answers DMXQ_ERR_UNSUPPORTED (NotImplementedError through either binding), nothing launched
    t = base[:, :960].contiguous().to(cuda)
    for binding in ("ctypes", "torch"):
        raw = dmx.ops.front(binding)._ops
        with pytest.raises(NotImplementedError):
            raw.dynamic_float_qdq(t, 0, 48, 3, 4, 7, False, 2, False, False, None)        # a group of 48
        with pytest.raises(NotImplementedError):
            raw.dynamic_float_qdq(t, 2, 48, 3, 4, 7, False, 2, False, False, None)        # a tile of 48
        with pytest.raises(NotImplementedError):
            raw.dynamic_float_qdq(t, 1, 960, 3, 4, 7, False, 3, False, False, None)       # stochastic
        with pytest.raises(NotImplementedError):
            raw.dynamic_float_qdq(t, 1, 960, 3, 4, 7, False, 2, False, False, F32)        # bf16 -> f32
        raw.dynamic_float_qdq(t, 1, 48, 3, 4, 7, False, 2, False, False, None)            # rows of 48: a wave per row


def test_both_bindings_return_scale_and_meta(dmx, oracle, cuda):
    x = make("outlier", (64, 384), seed=21, dtype=BF16, block=64)
    xd = x.to(cuda)
    for granularity, g, shape in (("per_token", None, (64,)), ("per_group", 64, (384,)), ("per_tile", 32, (2, 12))):
        want, wsc = R.dynamic_float_ref(oracle, x, R.FORMATS["e4m3"], granularity, g, True)
        for binding in ("ctypes", "torch"):
            f = dmx.ops.front(binding)
            y, sc = fused(f, xd, E4M3, granularity, g, True, return_scale=True)
            assert tuple(sc.shape) == shape and bits_equal(y.cpu(), want) == 0 and bits_equal(sc.cpu(), wsc) == 0, binding
            assert bits_equal(fused(f, xd, E4M3, granularity, g, True), y) == 0                  # without the scales
            yc, scc = chain(f, xd, E4M3, granularity, g, True, return_scale=True)
            assert bits_equal(yc, y) == 0 and bits_equal(scc, sc) == 0 and scc.shape == sc.shape
    # the dispatcher op itself, and its meta kernel
    y, sc = torch.ops.dmxq.dynamic_float_qdq(xd, 2, 32, 3, 4, 7, False, 2, True, True, None)
    assert bits_equal(y.cpu(), want) == 0 and bits_equal(sc.cpu(), wsc) == 0
    m = torch.ops.dmxq.dynamic_float_qdq(xd.to("meta"), 2, 32, 3, 4, 7, False, 2, True, True, None)
    assert all(t.device.type == "meta" for t in m) and m[0].shape == xd.shape and m[0].dtype == BF16 and m[1].shape == (2, 12) and m[1].dtype == F32
    m = torch.ops.dmxq.dynamic_float_qdq(xd.to("meta"), 1, 384, 3, 4, 7, False, 2, False, False, None)
    assert m[1].numel() == 0
    e = dmx.ops.dynamic_float_qdq(xd[:0], E4M3, return_scale=True)
    assert e[0].shape == (0, 384) and e[1].numel() == 0


# ---------------------------------------------------------------------------------------------------- CastTo
def test_castto_scaling_equals_the_op(dmx, cuda):
    x = make("outlier", (64, 768), seed=47, dtype=BF16, block=64).to(cuda)
    for setting, granularity, g, pow2 in (("per_token", "per_token", None, False), ({"per_group": 128}, "per_group", 128, False),
                                          ({"per_tile": 64, "pow2_scale": True}, "per_tile", 64, True), ("per_tensor", "per_tensor", None, False)):
        c = dmx.CastTo(format=E4M3).to(cuda)
        keys = set(c.state_dict())
        static = c(x)
        c.set_scaling(setting)
        got = c(x)
        assert got.dtype == BF16 and bits_equal(got, dmx.ops.dynamic_float_qdq(x, E4M3, granularity, g, pow2_scale=pow2)) == 0
        assert bits_equal(got, static) != 0 and set(c.state_dict()) == keys
        assert bits_equal(c.measure_error(x), dmx.ops.error_stats(x, got)) == 0
        c.disable_fake_quant()
        assert bits_equal(c(x), x) == 0
        c.enable_fake_quant()
        c.set_scaling(None)
        assert bits_equal(c(x), static) == 0


def test_castto_with_a_hadamard_pre_transform(dmx, cuda):
    """rotate (float32) -> scaled cast of the rotated float32 tensor -> rotate back, bit for bit: the one-call shortcut is skipped"""
    x = make("outlier", (40, 256), seed=61, dtype=BF16, block=64).to(cuda)
    for spec, inverse in ((64, True), ({"size": 64, "inverse": False}, False)):
        c = dmx.CastTo(format=E4M3).to(cuda)
        c.set_pre_transform({"hadamard": spec})
        plain = c(x)
        c.set_scaling("per_group", 64)
        r = dmx.ops.hadamard(x, 64, out_dtype=F32)
        if inverse:
            want = dmx.ops.hadamard(fused(dmx.ops, r, E4M3, "per_group", 64), 64, out_dtype=BF16)
        else:
            want = dmx.ops.dynamic_float_qdq(r, E4M3, "per_group", 64, out_dtype=BF16)
        got = c(x)
        assert got.dtype == BF16 and bits_equal(got, want) == 0 and bits_equal(got, plain) != 0
        assert bits_equal(c.measure_error(x), dmx.ops.error_stats(x, got)) == 0


def test_backward_is_the_identity(dmx, cuda):
    x = make("normal", (128, 256), seed=67, dtype=F32)
    g = make("heavy", (128, 256), seed=71, dtype=F32)
    for kw in ({}, {"fused": False}, {"granularity": "per_tile", "group_size": 128}):
        xd = x.to(cuda).requires_grad_(True)
        y = dmx.ops.dynamic_float_qdq(xd, E4M3, **kw)
        y.backward(g.to(cuda))
        assert bits_equal(xd.grad, g) == 0
    xd = x.to(cuda).requires_grad_(True)
    y, sc = dmx.ops.dynamic_float_qdq(xd, E4M3, return_scale=True)
    assert y.requires_grad and not sc.requires_grad
    c = dmx.CastTo(format=E4M3).to(cuda)
    c.set_scaling("per_token")
    for pt in ({}, {"hadamard": 8}):
        c.set_pre_transform(pt)
        xd = x.to(cuda).requires_grad_(True)
        c(xd).backward(g.to(cuda))
        assert bits_equal(xd.grad, g) == 0, pt


# ---------------------------------------------------------------------------------------------------- graph capture, modules
def test_graph_capture(dmx, oracle, cuda):
    x0 = make("normal", (128, 768), seed=73, dtype=BF16)
    x1 = make("outlier", (128, 768), seed=79, dtype=BF16, block=64)
    buf = x0.to(cuda).clone()
    fused(dmx.ops, buf, E4M3)                                            # (warm-up outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_a, sc_a = fused(dmx.ops, buf, E4M3, return_scale=True)
        out_b, sc_b = fused(dmx.ops, buf, E4M3, "per_tile", 128, True, return_scale=True)
        out_c = fused(dmx.ops, buf, E4M3, "per_group", 128)
    for x in (x1, x0):
        buf.copy_(x.to(cuda))
        graph.replay()
        torch.cuda.synchronize()
        want, wsc = R.dynamic_float_ref(oracle, x, R.FORMATS["e4m3"], "per_token")
        assert bits_equal(out_a.cpu(), want) == 0 and bits_equal(sc_a.cpu(), wsc) == 0
        want, wsc = R.dynamic_float_ref(oracle, x, R.FORMATS["e4m3"], "per_tile", 128, True)
        assert bits_equal(out_b.cpu(), want) == 0 and bits_equal(sc_b.cpu(), wsc) == 0
        assert bits_equal(out_c.cpu(), R.dynamic_float_ref(oracle, x, R.FORMATS["e4m3"], "per_group", 128)[0]) == 0


def _fp8_linear(dmx, cuda):
    torch.manual_seed(0)
    m = dmx.nn.Linear(256, 384).to(cuda).to(BF16)
    m.configure({"input_formats": [E4M3], "weight_format": E4M3, "input_scaling": "per_token", "weight_scaling": {"per_tile": 128}})
    return m


def test_linear_fp8_recipe_live_folded_and_graphed(dmx, cuda):
    """Linear(256, 384) with per-token scaled activations and 128 x 128 tile-scaled weights: eager == the two casts by hand + F.linear;
    the batched live weight path, the folded model and GraphedForward give the same bits (a scaled cast drops out of every batched path)"""
    from dmx_compressor_amd.nn import GraphedForward, LiveWeightBatch, _bias_batches, _weight_batches, fold_weights_and_biases
    x = make("heavy", (3, 7, 256), seed=83, dtype=BF16).to(cuda)
    a, b = _fp8_linear(dmx, cuda), _fp8_linear(dmx, cuda)

    def by_hand(m, t):
        xq = dmx.ops.dynamic_float_qdq(t, E4M3, "per_token")
        wq = dmx.ops.dynamic_float_qdq(m.weight.detach(), E4M3, "per_tile", 128)
        return F.linear(xq, wq, m.bias.detach())

    with torch.no_grad():
        y = a(x)
        assert y.dtype == BF16 and bits_equal(y, by_hand(a, x)) == 0
        groups, hyper = _weight_batches([a, b])
        assert not groups and not hyper
        a.bias_cast.set_format(E4M3)
        assert len(_bias_batches([a])) == 1
        a.bias_cast.set_scaling("per_tensor")
        assert not _bias_batches([a])                                    # a scaled bias cast is the module's own business too
        a.bias_cast.set_scaling(None)
        a.bias_cast.set_format("SAME")
        x256 = make("heavy", (5, 256), seed=97, dtype=BF16).to(cuda)
        y256 = make("outlier", (5, 256), seed=101, dtype=BF16, block=64).to(cuda)
        net = torch.nn.Sequential(a, torch.nn.Linear(384, 256, device=cuda, dtype=BF16), b)
        eager, eager_y = net(x256).clone(), net(y256).clone()
        batch = LiveWeightBatch(net)
        try:
            assert bits_equal(net(x256), eager) == 0
        finally:
            batch.remove()
        g = GraphedForward(net, x256)
        assert bits_equal(g(x256), eager) == 0
        assert bits_equal(g(y256), eager_y) == 0                         # replayed on new contents: new scales
        fold_weights_and_biases(net)
        assert repr(a.weight_cast.format) == "SAME"
        assert bits_equal(net(x256), eager) == 0 and bits_equal(net(y256), eager_y) == 0


def test_consumer_link_keeps_a_scaled_cast(dmx, cuda):
    """a producer's output cast is absorbed by a consumer applying the same float format -- not when either of the two is scaled"""
    x = make("heavy", (5, 256), seed=103, dtype=BF16).to(cuda)
    fmt = "FP[1|4|3,7](FN)"
    act = dmx.nn.ReLU()
    act.configure({"output_formats": [fmt]})
    lin = dmx.nn.Linear(256, 128).to(cuda).to(BF16)
    lin.configure({"input_formats": [fmt]})
    dmx.nn.link_consumer(act, lin)
    with torch.no_grad():
        assert act._output_cast_absorbed(x)
        lin.configure({"input_scaling": "per_token"})
        assert not act._output_cast_absorbed(x)
        want = F.linear(dmx.ops.dynamic_float_qdq(dmx.ops.float_qdq(F.relu(x), 3, 4, 7, True), fmt, "per_token"), lin.weight, lin.bias)
        assert bits_equal(lin(act(x)), want) == 0
        lin.configure({"input_scaling": None})
        act.configure({"output_scaling": "per_token"})
        assert not act._output_cast_absorbed(x)
        want = F.linear(dmx.ops.float_qdq(dmx.ops.dynamic_float_qdq(F.relu(x), fmt, "per_token"), 3, 4, 7, True), lin.weight, lin.bias)
        assert bits_equal(lin(act(x)), want) == 0


# ---------------------------------------------------------------------------------------------------- more than 2^31 elements
BIG = (699520, 3072)          # 2,148,925,440 elements; 699520 = 128 * 5465 rows, rows of 3072 (no power of two: tests/_large_cases.py)
LARGE = [LC.case("dynamic_float_per_token", "dynamic_float_qdq", BIG, p=dict(granularity="per_token", gs=None), twin=False),
         # the same elements as 174880 rows of 12288 (1536 vectors: the workgroup-per-row kernel with its LDS exchange)
         LC.case("dynamic_float_per_token_block_row", "dynamic_float_qdq", (174880, 12288), p=dict(granularity="per_token", gs=None), twin=False),
         LC.case("dynamic_float_per_group", "dynamic_float_qdq", BIG, p=dict(granularity="per_group", gs=128), twin=False),
         LC.case("dynamic_float_per_tile", "dynamic_float_qdq", BIG, p=dict(granularity="per_tile", gs=128), unit=128, twin=False)]
_BIG_INPUT = {}


def _big_input(c, dev):
    """ONE input shared by the three cases and left unchanged: heavy-tailed bf16 without a period, a NaN, an Inf, a denormal run and a
    zero run planted in rows beyond element 2^31"""
    if "x" not in _BIG_INPUT:
        x = LC.device_input(c.kind, c.shape, LC.torch_dtype(c.dtype), 1234, dev)
        LC.plant_specials(x, c)
        _BIG_INPUT["x"] = x
    return _BIG_INPUT["x"]


@pytest.mark.parametrize("c", LARGE, ids=[c.name for c in LARGE])
def test_more_than_two_to_the_31_elements_equal_their_chunks(dmx, cuda, c):
    """one call on 2^31 + 2^20 elements and more (64-bit indexing throughout: there is no 32-bit form) against the same call on chunks
    of fewer than 2^31 elements, cut at whole rows / whole tile rows, bit for bit, the scales included"""
    assert LC.numel(c.shape) > LC.MIN_N and all(LC.TWO31 % p and LC.TWO32 % p for p in LC.periods(c))
    free, _ = torch.cuda.mem_get_info()
    held = sum(t.numel() * t.element_size() for t in _BIG_INPUT.values())
    need = LC.peak_bytes(c) - held
    if free < need:
        pytest.skip(f"{c.name}: needs {need / LC.GIB:.1f} GiB of device memory, {free / LC.GIB:.1f} GiB free")
    x = _big_input(LARGE[0], cuda).view(c.shape)
    assert dmx.ops.dynamic_float_class(c.shape[1], x.dtype) == ("block_row" if "block_row" in c.name else "wave_row")
    gran, g = c.p["granularity"], c.p["gs"]
    rows, L = c.shape

    def fn(xs, cut):
        y, sc = fused(dmx.ops, xs[0], E4M3, gran, g, return_scale=True)
        n = xs[0].shape[0]
        sc = sc.repeat_interleave(g, dim=0) if gran == "per_tile" else sc.reshape(n, -1)   # (dim 0: the input's rows)
        return y, sc

    full = fn([x], (0, rows))
    assert full[1].shape == (rows, {"per_token": 1, "per_group": L // 128, "per_tile": L // 128}[gran])
    LC.check_chunks(c, fn, [x], full)
    del full
    if c is LARGE[-1]:
        _BIG_INPUT.clear()
