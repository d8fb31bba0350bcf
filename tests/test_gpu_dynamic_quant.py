"""GPU tests of the dynamic integer cast (csrc/dynamic_quant.hip, ops.dynamic_fixed_qdq, CastTo.set_dynamic): the fused
kernel against the CPU chain of tests/_dynamic_ref.py (finite inputs) and against the library's own three-launch chain on the GPU
(everything, rows with NaN / Inf included), bit for bit, scale and zero point included.  The kernel's grid does not loop (a wave takes
a fixed number of vectors, a row is a wave's or a workgroup's), so there is no multi-tile case to force with DMXQ_PLAN_CUS."""
import pytest
import torch
import torch.nn.functional as F

import _dynamic_ref as R
from _data import bits_equal, make, mismatches_nan_aware

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
INT8, INT4 = "XP[8,0](CSN)", "XP[4,0](CSN)"
SPEC = {INT8: (8, True), INT4: (4, True), "XP[8,0](C_N)": (8, False)}


def routes_of(ops):
    """the front end's private route counter (dmx.ops re-exports a front-end module; ops.front(binding) IS one)"""
    return ops._dynamic_routes if hasattr(ops, "_dynamic_routes") else ops._front._dynamic_routes


def fused(ops, x, fmt, granularity="per_token", group_size=None, qsym=False, **kw):
    """ops.dynamic_fixed_qdq(..., fused=True), asserting on the host-side route counter that the kernel ran (and the chain did not)"""
    before = dict(routes_of(ops))
    out = ops.dynamic_fixed_qdq(x, fmt, granularity, group_size, symmetric_qscheme=qsym, fused=True, **kw)
    assert routes_of(ops)["fused"] == before["fused"] + 1 and routes_of(ops)["chain"] == before["chain"]
    return out


def chain(ops, x, fmt, granularity="per_token", group_size=None, qsym=False, **kw):
    before = dict(routes_of(ops))
    out = ops.dynamic_fixed_qdq(x, fmt, granularity, group_size, symmetric_qscheme=qsym, fused=False, **kw)
    assert routes_of(ops)["chain"] == before["chain"] + 1 and routes_of(ops)["fused"] == before["fused"]
    return out


def check_against_ref(oracle, ops, x, fmt, granularity, group_size, qsym, cuda):
    p, fsym = SPEC[fmt]
    S = R.segment_of(x, granularity, group_size)
    want, wsc, wzp = R.dynamic_ref(oracle, x, p, fsym, S, qsym)
    y, sc, zp = fused(ops, x.to(cuda), fmt, granularity, group_size, qsym, return_qparams=True)
    assert y.dtype == x.dtype and y.shape == x.shape and sc.dtype == F32 and zp.dtype == torch.int64
    assert sc.shape == wsc.shape and zp.shape == wzp.shape
    assert bits_equal(sc.cpu(), wsc) == 0 and bits_equal(zp.cpu(), wzp) == 0
    assert bits_equal(y.cpu(), want) == 0


# ---------------------------------------------------------------------------------------------------- the kernel's three geometries
@pytest.mark.parametrize("qsym", [False, True], ids=["affine", "symmetric"])
@pytest.mark.parametrize("fmt", [INT8, INT4])
@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=["bf16", "f16", "f32"])
def test_groups(dmx, oracle, cuda, dtype, fmt, qsym):
    """segments inside a wave: g = 16 .. 128 on [37, 384], g = 256 on [37, 512] (37 rows: the segment count is no multiple of a wave's
    share, the last workgroup has lanes past the end)"""
    for g in (16, 32, 64, 128, 256):
        x = make("heavy", (37, 512 if g == 256 else 384), seed=g, dtype=dtype, block=g)
        check_against_ref(oracle, dmx.ops, x, fmt, "per_group", g, qsym, cuda)


def test_groups_deep_grid(dmx, oracle, cuda):
    """more than 2^19 vectors: the four-vectors-per-lane build of the group kernel, its last wave partly past the end"""
    x = make("normal", (1027, 4096), seed=3, dtype=BF16)
    check_against_ref(oracle, dmx.ops, x, INT8, "per_group", 128, False, cuda)


def test_more_segments_than_one_reduction_takes(dmx, oracle, cuda):
    """67 200 segments: the kernel in one launch; the chain in pieces of 32 768 segments (group_minmax takes 65 535 groups), joined"""
    x = make("heavy", (2100, 512), seed=11, dtype=BF16)
    check_against_ref(oracle, dmx.ops, x, INT8, "per_group", 16, False, cuda)
    y, sc, zp = fused(dmx.ops, x.to(cuda), INT8, "per_group", 16, return_qparams=True)
    yc, scc, zpc = chain(dmx.ops, x.to(cuda), INT8, "per_group", 16, return_qparams=True)
    assert sc.shape == (67200,) and bits_equal(y, yc) == 0 and bits_equal(sc, scc) == 0 and bits_equal(zp, zpc) == 0


@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=["bf16", "f16", "f32"])
@pytest.mark.parametrize("L", [8, 776, 1024, 4096, 8192, 8200, 14336, 16384])
def test_whole_rows(dmx, oracle, cuda, L, dtype):
    """a wave per row up to 16 vectors per lane (8192 sixteen-bit / 4096 fp32 elements), a workgroup per row beyond; rows that leave
    lanes idle (8, 776, 8200) and rows that fill every slot (1024 .. 16384)"""
    x = make("heavy", (5 if L >= 8192 else 67, L), seed=L, dtype=dtype, block=64)
    for fmt, qsym in ((INT8, False), (INT8, True), (INT4, False), ("XP[8,0](C_N)", False)):
        check_against_ref(oracle, dmx.ops, x, fmt, "per_token", None, qsym, cuda)


# ---------------------------------------------------------------------------------------------------- planted rows
REGIMES = [("group", (12, 256), "per_group", 64), ("short_row", (12, 48), "per_token", None), ("wave_row", (12, 776), "per_token", None), ("block_row", (12, 8200), "per_token", None)]
FINITE_ROWS, SPECIAL_ROWS = list(range(0, 10)), [10, 11]


def planted(shape, dtype, seed):
    x = make("normal", shape, seed=seed, dtype=F32)
    L = shape[1]
    x[0] = 0.0                                   # all zeros: scale = eps, below 2^-20 -> the IEEE-division side of recip_ok
    x[1] = -0.0                                  # all -0.0
    x[2] = 3.5                                   # a constant row
    x[3, L // 3] = 1e30                          # maximum 1e30
    x[4] = (x[4] * 1e-30).clamp(-1e-30, 1e-30)   # maximum 1e-30
    x[4, 5] = 1e-30
    x[5] = x[5].abs() + 0.25                     # all positive: the affine zero point clamps to qmin
    x[6] = -x[6].abs() - 0.25                    # all negative: to qmax
    x[7, ::2] = 0.0                              # a plain row with zeros in it
    x[8] = x[8] * 1e-3
    x[9, 7] = -1e30
    x[10, L // 2] = float("inf")                 # one Inf
    x[11, L - 3] = float("nan")                  # one NaN
    return x.to(dtype)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("regime,shape,granularity,g", REGIMES, ids=[r[0] for r in REGIMES])
def test_planted_rows(dmx, oracle, cuda, regime, shape, granularity, g, dtype):
    x = planted(shape, dtype, seed=len(regime))
    assert dmx.ops.dynamic_class(R.segment_of(x, granularity, g), dtype, granularity != "per_group") == regime
    xd = x.to(cuda)
    for fmt, qsym in ((INT8, False), (INT8, True), (INT4, False)):
        y, sc, zp = fused(dmx.ops, xd, fmt, granularity, g, qsym, return_qparams=True)
        yc, scc, zpc = chain(dmx.ops, xd, fmt, granularity, g, qsym, return_qparams=True)
        assert mismatches_nan_aware(sc, scc) == 0 and bits_equal(zp, zpc) == 0, (fmt, qsym)
        assert mismatches_nan_aware(y, yc) == 0, (fmt, qsym)
        # the NaN / Inf rules of the chain, restated: a NaN makes both extrema NaN, which qparams drops (scale eps); an Inf is an extremum
        per_row = sc.reshape(shape[0], -1).cpu()
        nan_seg = torch.isnan(x.float().reshape(shape[0], per_row.shape[1], -1)).any(-1)[11]
        assert bool((per_row[11][nan_seg] == torch.finfo(F32).eps).all()) and bool(torch.isinf(per_row[10]).any())
        assert float(per_row[0].max()) == torch.finfo(F32).eps and float(per_row[1].max()) == torch.finfo(F32).eps
        if not qsym:
            qmin, qmax = R.qrange(*SPEC[fmt])
            zrow = zp.reshape(shape[0], -1).cpu()
            assert bool((zrow[5] == qmin).all()) and bool((zrow[6] == qmax).all())
        p, fsym = SPEC[fmt]
        want, wsc, wzp = R.dynamic_ref(oracle, x[FINITE_ROWS], p, fsym, R.segment_of(x, granularity, g), qsym)
        n = wsc.numel()
        assert bits_equal(sc.cpu()[:n], wsc) == 0 and bits_equal(zp.cpu()[:n], wzp) == 0, (fmt, qsym)
        assert bits_equal(y.cpu()[FINITE_ROWS], want) == 0, (fmt, qsym)


# ---------------------------------------------------------------------------------------------------- fallbacks
def test_fallbacks_are_the_chain_and_fused_true_raises(dmx, oracle, cuda):
    ops = dmx.ops
    base = make("heavy", (9, 16392), seed=5, dtype=BF16)
    unaligned = base.to(cuda).reshape(-1)[4:4 + 9 * 1024].reshape(9, 1024)       # 8 bytes past a 16-byte boundary
    assert unaligned.data_ptr() % 16 == 8 and unaligned.is_contiguous()
    cases = [("L=1500", base[:, :1500].contiguous().to(cuda), INT8, "per_token", None, {}),
             ("L=16392", base.to(cuda), INT8, "per_token", None, {}),
             ("g=48", base[:, :384].contiguous().to(cuda), INT8, "per_group", 48, {}),
             ("unaligned", unaligned, INT8, "per_token", None, {}),
             ("bf16->f32", base[:, :1024].contiguous().to(cuda), INT8, "per_token", None, {"out_dtype": F32}),
             ("stochastic", base[:, :1024].contiguous().to(cuda), "XP[8,0](CSS)", "per_token", None, {"seed": 1234})]
    for name, x, fmt, granularity, g, kw in cases:
        with pytest.raises(NotImplementedError):
            ops.dynamic_fixed_qdq(x, fmt, granularity, g, fused=True, **kw)
        routes = dict(routes_of(ops))
        got = ops.dynamic_fixed_qdq(x, fmt, granularity, g, **kw)                 # fused=None: falls back
        assert routes_of(ops)["chain"] == routes["chain"] + 1 and routes_of(ops)["fused"] == routes["fused"], name
        assert got.shape == x.shape and got.dtype == kw.get("out_dtype", x.dtype), name
        assert bits_equal(got, chain(ops, x, fmt, granularity, g, **kw)) == 0, name
        if name == "stochastic":     # (an explicit seed: the same draws on both runs; every element between its two neighbours)
            lo = ops.dynamic_fixed_qdq(x, "XP[8,0](CSD)", granularity, g, fused=False)
            hi = ops.dynamic_fixed_qdq(x, "XP[8,0](CSU)", granularity, g, fused=False)
            assert bool(((got == lo) | (got == hi)).all()) and bool((got != lo).any()) and bool((got != hi).any()), name
            continue
        p, fsym = SPEC[fmt]
        want, _, _ = R.dynamic_ref(oracle, x.cpu(), p, fsym, R.segment_of(x, granularity, g), False, kw.get("out_dtype"))
        assert bits_equal(got.cpu(), want) == 0, name
    # the C entry itself answers DMXQ_ERR_UNSUPPORTED (NotImplementedError through either binding), nothing launched
    x = base[:, :384].contiguous().to(cuda)
    for binding in ("ctypes", "torch"):
        raw = dmx.ops.front(binding)._ops
        with pytest.raises(NotImplementedError):
            raw.dynamic_fixed_qdq(x, 48, False, 8, 0, True, True, 2, -127, 127, False, False, None)      # a group of 48
        with pytest.raises(NotImplementedError):
            raw.dynamic_fixed_qdq(x, 384, True, 8, 1, True, True, 2, -127, 127, False, False, None)      # fraction bits
        with pytest.raises(NotImplementedError):
            raw.dynamic_fixed_qdq(x, 384, True, 8, 0, False, True, 2, -127, 127, False, False, None)     # no clamp
        with pytest.raises(NotImplementedError):
            raw.dynamic_fixed_qdq(x, 384, True, 8, 0, True, True, 3, -127, 127, False, False, None)      # stochastic
        raw.dynamic_fixed_qdq(x, 48, True, 8, 0, True, True, 2, -127, 127, False, False, None)           # rows of 48: a wave per row


def test_short_rows(dmx, oracle, cuda):
    """rows of fewer than 64 vectors that are no power of two: a wave per row with idle lanes (class short_row)"""
    for L, dtype in ((48, BF16), (24, F32), (504, F16), (248, F32)):
        assert dmx.ops.dynamic_class(L, dtype, True) == "short_row"
        x = make("heavy", (67, L), seed=L, dtype=dtype)
        for qsym in (False, True):
            check_against_ref(oracle, dmx.ops, x, INT8, "per_token", None, qsym, cuda)


def test_per_tensor_equals_the_chain(dmx, oracle, cuda):
    for shape, kernel in (((4, 8, 96), True), ((300, 1000), False)):     # 3072 elements: one row on the kernel; 300 000: the chain
        x = make("heavy", shape, seed=9, dtype=BF16)
        xd = x.to(cuda)
        if kernel:
            y, sc, zp = fused(dmx.ops, xd, INT8, "per_tensor", return_qparams=True)
        else:
            with pytest.raises(NotImplementedError):
                dmx.ops.dynamic_fixed_qdq(xd, INT8, "per_tensor", fused=True)
            y, sc, zp = dmx.ops.dynamic_fixed_qdq(xd, INT8, "per_tensor", return_qparams=True)
        yc, scc, zpc = chain(dmx.ops, xd, INT8, "per_tensor", return_qparams=True)
        assert sc.numel() == 1 and bits_equal(sc, scc) == 0 and bits_equal(zp, zpc) == 0 and bits_equal(y, yc) == 0
        want, wsc, wzp = R.dynamic_ref(oracle, x, 8, True, x.numel(), False)
        assert bits_equal(y.cpu(), want) == 0 and bits_equal(sc.cpu(), wsc) == 0 and bits_equal(zp.cpu(), wzp) == 0


def test_both_bindings_and_return_qparams(dmx, oracle, cuda):
    x = make("outlier", (37, 776), seed=21, dtype=BF16, block=64)
    xg = make("outlier", (37, 384), seed=22, dtype=F16, block=64)
    for t, granularity, g in ((x, "per_token", None), (xg, "per_group", 64)):
        S = R.segment_of(t, granularity, g)
        want, wsc, wzp = R.dynamic_ref(oracle, t, 8, True, S, False)
        for binding in ("ctypes", "torch"):
            f = dmx.ops.front(binding)
            y, sc, zp = fused(f, t.to(cuda), INT8, granularity, g, return_qparams=True)
            assert bits_equal(y.cpu(), want) == 0 and bits_equal(sc.cpu(), wsc) == 0 and bits_equal(zp.cpu(), wzp) == 0, binding
            assert bits_equal(fused(f, t.to(cuda), INT8, granularity, g), y) == 0                     # without the two outputs
            yc, scc, zpc = chain(f, t.to(cuda), INT8, granularity, g, return_qparams=True)             # the same triple on the chain
            assert bits_equal(yc, y) == 0 and bits_equal(scc, sc) == 0 and bits_equal(zpc, zp) == 0 and scc.shape == sc.shape
    # the dispatcher op itself, and its meta kernel
    xd = x.to(cuda)
    y, sc, zp = torch.ops.dmxq.dynamic_fixed_qdq(xd, 776, True, 8, 0, True, True, 2, -127, 127, False, True, None)
    assert bits_equal(y.cpu(), R.dynamic_ref(oracle, x, 8, True, 776, False)[0]) == 0 and sc.shape == (37,) and zp.shape == (37,)
    m = torch.ops.dmxq.dynamic_fixed_qdq(xd.to("meta"), 776, True, 8, 0, True, True, 2, -127, 127, False, True, None)
    assert all(t.device.type == "meta" for t in m) and m[0].shape == xd.shape and m[0].dtype == BF16
    assert m[1].shape == (37,) and m[1].dtype == F32 and m[2].shape == (37,) and m[2].dtype == torch.int64
    m = torch.ops.dmxq.dynamic_fixed_qdq(xd.to("meta"), 776, True, 8, 0, True, True, 2, -127, 127, False, False, None)
    assert m[1].numel() == 0 and m[2].numel() == 0


# ---------------------------------------------------------------------------------------------------- CastTo
def test_castto_dynamic_equals_the_op_and_leaves_the_buffers(dmx, cuda):
    x = make("outlier", (40, 776), seed=47, dtype=BF16, block=64).to(cuda)
    for qscheme, qsym in ((torch.per_tensor_affine, False), (torch.per_tensor_symmetric, True), (torch.per_channel_symmetric, True)):
        for setting, granularity, g in (("per_token", "per_token", None), ({"per_group": 8}, "per_group", 8), ("per_tensor", "per_tensor", None)):
            c = dmx.CastTo(format=INT8, qscheme=qscheme, ch_axis=0).to(cuda)
            n = 40 if qscheme == torch.per_channel_symmetric else 1       # stored scales, one per row for the per-channel scheme
            c.scale, c.zero_point = torch.full((n,), 0.37, device=cuda), torch.full((n,), 3, dtype=torch.int64, device=cuda)
            sc0, zp0 = c.scale.clone(), c.zero_point.clone()
            static = c(x)
            c.set_dynamic(setting)
            got = c(x)
            assert got.dtype == BF16 and bits_equal(got, dmx.ops.dynamic_fixed_qdq(x, INT8, granularity, g, symmetric_qscheme=qsym)) == 0
            assert bits_equal(got, static) != 0
            assert bits_equal(c.scale, sc0) == 0 and bits_equal(c.zero_point, zp0) == 0 and c.scale.shape == sc0.shape
            assert bits_equal(c.measure_error(x), dmx.ops.error_stats(x, got)) == 0
            c.set_dynamic(None)
            assert bits_equal(c(x), static) == 0


def test_castto_calibration_is_unaffected(dmx, cuda):
    """with the observer on, a dynamic cast calibrates exactly like its static twin: same observer state, same buffers, same output"""
    x = make("heavy", (48, 256), seed=59, dtype=BF16).to(cuda)
    outs = []
    for dyn in (None, "per_token"):
        c = dmx.CastTo(format=INT8).to(cuda)
        c.set_dynamic(dyn)
        c.enable_calibration(True, observer_cls=dmx.MinMaxObserver, qscheme_to_overload=torch.per_channel_symmetric, ch_axis=0)
        y = c(x)
        assert bits_equal(y, x) == 0                                   # observe only
        c.enable_observer()
        c.enable_fake_quant()                                          # both on: observer step + the STATIC cast, as ever
        both = c(x)
        c.enable_calibration(False)
        outs.append((both, c.scale.clone(), c.zero_point.clone(), c.activation_post_process.min_val.clone(), c(x)))
    (a, sc_a, zp_a, mn_a, _), (b, sc_b, zp_b, mn_b, after) = outs
    assert bits_equal(a, b) == 0 and bits_equal(sc_a, sc_b) == 0 and bits_equal(zp_a, zp_b) == 0 and bits_equal(mn_a, mn_b) == 0
    assert sc_a.numel() == 48
    assert bits_equal(after, dmx.ops.dynamic_fixed_qdq(x, INT8, "per_token", symmetric_qscheme=True)) == 0   # observer off: dynamic again


def test_castto_with_a_hadamard_pre_transform(dmx, cuda):
    """rotate (float32) -> dynamic cast of the rotated float32 tensor -> rotate back, bit for bit"""
    x = make("outlier", (40, 256), seed=61, dtype=BF16, block=64).to(cuda)
    for spec, inverse in ((64, True), ({"size": 64, "inverse": False}, False)):
        c = dmx.CastTo(format=INT4).to(cuda)
        c.set_pre_transform({"hadamard": spec})
        c.set_dynamic("per_group", 64)
        r = dmx.ops.hadamard(x, 64, out_dtype=F32)
        if inverse:
            want = dmx.ops.hadamard(fused(dmx.ops, r, INT4, "per_group", 64), 64, out_dtype=BF16)
        else:
            want = dmx.ops.dynamic_fixed_qdq(r, INT4, "per_group", 64, out_dtype=BF16)
        got = c(x)
        assert got.dtype == BF16 and bits_equal(got, want) == 0
        assert bits_equal(c.measure_error(x), dmx.ops.error_stats(x, got)) == 0


def test_backward_is_the_identity(dmx, cuda):
    x = make("normal", (12, 776), seed=67, dtype=F32)
    g = make("heavy", (12, 776), seed=71, dtype=F32)
    for kw in ({}, {"fused": False}):
        xd = x.to(cuda).requires_grad_(True)
        y = dmx.ops.dynamic_fixed_qdq(xd, INT8, **kw)
        y.backward(g.to(cuda))
        assert bits_equal(xd.grad, g) == 0
    xd = x.to(cuda).requires_grad_(True)
    y, sc, zp = dmx.ops.dynamic_fixed_qdq(xd, INT8, return_qparams=True)
    assert y.requires_grad and not sc.requires_grad and not zp.requires_grad
    c = dmx.CastTo(format=INT8).to(cuda)
    c.set_dynamic("per_token")
    for pt in ({}, {"hadamard": 8}):
        c.set_pre_transform(pt)
        xd = x.to(cuda).requires_grad_(True)
        c(xd).backward(g.to(cuda))
        assert bits_equal(xd.grad, g) == 0, pt
    xb = x.to(cuda).to(BF16).requires_grad_(True)
    dmx.ops.dynamic_fixed_qdq(xb, INT8, out_dtype=F32).backward(g.to(cuda))
    assert xb.grad.dtype == BF16 and bits_equal(xb.grad, g.to(BF16)) == 0


# ---------------------------------------------------------------------------------------------------- graph capture
def test_graph_capture(dmx, oracle, cuda):
    x0 = make("normal", (32, 776), seed=73, dtype=BF16)
    x1 = make("outlier", (32, 776), seed=79, dtype=BF16, block=64)
    buf, bufg = x0.to(cuda).clone(), x0[:, :768].contiguous().to(cuda)
    fused(dmx.ops, buf, INT8)                                            # (warm-up outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_a, sc_a, zp_a = fused(dmx.ops, buf, INT8, return_qparams=True)
        out_b = fused(dmx.ops, bufg, INT4, "per_group", 128, qsym=True)
    for x in (x1, x0):
        buf.copy_(x.to(cuda))
        bufg.copy_(x[:, :768].to(cuda))
        graph.replay()
        torch.cuda.synchronize()
        want, wsc, wzp = R.dynamic_ref(oracle, x, 8, True, 776, False)
        assert bits_equal(out_a.cpu(), want) == 0 and bits_equal(sc_a.cpu(), wsc) == 0 and bits_equal(zp_a.cpu(), wzp) == 0
        assert bits_equal(out_a, dmx.ops.dynamic_fixed_qdq(x.to(cuda), INT8)) == 0
        assert bits_equal(out_b.cpu(), R.dynamic_ref(oracle, x[:, :768], 4, True, 128, True)[0]) == 0


# ---------------------------------------------------------------------------------------------------- modules
def _w8a8_linear(dmx, cuda, dynamic):
    torch.manual_seed(0)
    m = dmx.nn.Linear(256, 192).to(cuda).to(BF16)
    m.configure({"input_formats": [INT8], "weight_format": INT8})
    if dynamic:
        m.configure({"input_dynamic": "per_token", "weight_dynamic": "per_token"})
    return m


def test_linear_w8a8_dynamic(dmx, cuda):
    """Linear(256, 192) with per-token dynamic activations and per-output-channel dynamic weights: eager == the two casts by hand +
    F.linear; LiveWeightBatch and GraphedForward give the same bits (the dynamic weight cast drops out of the batched static path)"""
    from dmx_compressor_amd.nn import GraphedForward, LiveWeightBatch, _weight_batches
    x = make("heavy", (3, 7, 256), seed=83, dtype=BF16).to(cuda)
    a, b = _w8a8_linear(dmx, cuda, True), _w8a8_linear(dmx, cuda, True)
    for m in (a, b):                       # stale static buffers that must never be read
        m.weight_cast.scale.fill_(123.0)
        m.input_casts.input_cast.scale.fill_(123.0)

    def by_hand(m, t):
        xq = dmx.ops.dynamic_fixed_qdq(t, INT8, "per_token")
        wq = dmx.ops.dynamic_fixed_qdq(m.weight.detach(), INT8, "per_token")
        return F.linear(xq, wq, m.bias.detach())

    with torch.no_grad():
        y = a(x)
        assert y.dtype == BF16 and bits_equal(y, by_hand(a, x)) == 0
        groups, hyper = _weight_batches([a, b])
        assert not groups and not hyper                                  # a dynamic weight cast is not batched with static scales
        x256 = make("heavy", (5, 256), seed=97, dtype=BF16).to(cuda)
        y256 = make("outlier", (5, 256), seed=101, dtype=BF16, block=64).to(cuda)
        net2 = torch.nn.Sequential(a, torch.nn.Linear(192, 256, device=cuda, dtype=BF16), b)
        eager = net2(x256).clone()
        batch = LiveWeightBatch(net2)
        try:
            assert bits_equal(net2(x256), eager) == 0
        finally:
            batch.remove()
        g = GraphedForward(net2, x256)
        assert bits_equal(g(x256), eager) == 0
        assert bits_equal(g(y256), net2(y256)) == 0                      # replayed on new contents: new scales


def test_static_twin_is_untouched(dmx, cuda):
    """the static-scale twin of the W8A8 module: calibrated scales, the batched weight path still takes it, and its result is the
    static casts by hand (ops.fixed_qdq with the stored scale / zero point) + F.linear"""
    from dmx_compressor_amd.nn import LiveWeightBatch, _weight_batches
    x = make("heavy", (5, 256), seed=97, dtype=BF16).to(cuda)
    a, b = _w8a8_linear(dmx, cuda, False), _w8a8_linear(dmx, cuda, False)
    for m in (a, b):
        for c in (m.input_casts.input_cast, m.weight_cast):
            c.enable_calibration(True, observer_cls=dmx.MinMaxObserver)
        m(x)
        for c in (m.input_casts.input_cast, m.weight_cast):
            c.enable_calibration(False)
            assert c.dynamic is None
    with torch.no_grad():
        ic, wc = a.input_casts.input_cast, a.weight_cast
        xq = dmx.ops.fixed_qdq(x, 8, 0, True, True, "nearest", scale=ic.scale, zero_point=ic.zero_point)
        wq = dmx.ops.fixed_qdq(a.weight.detach(), 8, 0, True, True, "nearest", scale=wc.scale, zero_point=wc.zero_point)
        want = F.linear(xq, wq, a.bias.detach())
        assert bits_equal(a(x), want) == 0
        groups, _ = _weight_batches([a, b])
        assert [len(v) for v in groups.values()] == [2] and next(iter(groups))[0] == "fixed"
        net = torch.nn.Sequential(a, torch.nn.Linear(192, 256, device=cuda, dtype=BF16), b)
        eager = net(x).clone()
        batch = LiveWeightBatch(net)
        try:
            assert bits_equal(net(x), eager) == 0
            assert bits_equal(a(x), want) == 0
        finally:
            batch.remove()
        # one dynamic member: it leaves the batch, the other keeps its static route
        b.configure({"weight_dynamic": "per_token"})
        groups, _ = _weight_batches([a, b])
        assert [ms for ms in groups.values()] == [[a]]
