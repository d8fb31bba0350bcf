"""GPU tests of the codebook casts (csrc/codebook.hip, ops.codebook_qdq / codebook_accumulate / codebook_fit, CastTo.set_codebook;
DESIGN.md §8 "Codebook casts"): the fused kernel against the CPU checker of tests/_codebook_ref.py (the definition) and against the
library's own chain of launches on the GPU, bit for bit on the output, the scales and the indices; the Lloyd statistics against the
checker's float64 sums within the bound of a reordered float64 sum; the fit against the properties of a Lloyd iteration."""
import pytest
import torch
import torch.nn.functional as F

import _codebook_ref as R
import _large_cases as LC
from _data import bits_equal, make

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=["bf16", "f16", "f32"])
TABLES = pytest.mark.parametrize("name", ["nf4", "fp4_e2m1", "irregular5", "two"])
INT4 = "XP[4,0](CSN)"


@pytest.fixture(autouse=True)
def _stop_the_session_after_a_gpu_fault():
    """a HIP error after a test (an illegal access is sticky) ends the session: nothing more is started on a faulted device"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # pragma: no cover
        pytest.exit(f"GPU fault, stopping the session: {e}", returncode=3)


def routes_of(ops):
    return ops._codebook_routes if hasattr(ops, "_codebook_routes") else ops._front._codebook_routes


def fused(ops, x, levels, granularity="per_group", g=64, norm=None, **kw):
    """ops.codebook_qdq(..., fused=True), asserting on the host-side route counter that the kernel ran (and the chain did not)"""
    before = dict(routes_of(ops))
    out = ops.codebook_qdq(x, levels, granularity, g, norm, fused=True, **kw)
    assert routes_of(ops)["fused"] == before["fused"] + 1 and routes_of(ops)["chain"] == before["chain"]
    return out


def chain(ops, x, levels, granularity="per_group", g=64, norm=None, fused_arg=False, **kw):
    before = dict(routes_of(ops))
    out = ops.codebook_qdq(x, levels, granularity, g, norm, fused=fused_arg, **kw)
    assert routes_of(ops)["chain"] == before["chain"] + 1 and routes_of(ops)["fused"] == before["fused"]
    return out


def same3(got, want, what):
    (y, sc, idx), (wy, wsc, widx) = got, want
    assert y.dtype == wy.dtype and y.shape == wy.shape and sc.dtype == F32 and idx.dtype == torch.uint8 and idx.shape == y.shape, what
    assert sc.shape == wsc.shape and bits_equal(sc.cpu(), wsc.cpu()) == 0, what
    assert torch.equal(idx.cpu(), widx.cpu()), what
    assert bits_equal(y.cpu(), wy.cpu()) == 0, what


def check(ops, x, levels, granularity, g, cuda, norm=None):
    """kernel == checker and kernel == chain on y, scale and index"""
    xd = x.to(cuda)
    got = fused(ops, xd, levels, granularity, g, norm, return_scale=True, return_index=True)
    what = (len(levels), granularity, g, norm, tuple(x.shape), x.dtype)
    same3(got, chain(ops, xd, levels, granularity, g, norm, return_scale=True, return_index=True), what + ("chain",))
    same3(got, R.codebook_ref(x, levels, granularity, g, norm), what + ("checker",))
    return got


# ---------------------------------------------------------------------------------------------------- the kernel's geometries
@TABLES
@DTYPES
def test_groups(dmx, cuda, dtype, name):
    """segments inside a wave: g = 16 .. 256 on [3, 2 g] (one partly filled wave) and [257, 1024] (several workgroups, the last partly
    past the end); K = 16, 15 (padded), 5 with a duplicated level, 2"""
    for g in (16, 32, 64, 128, 256):
        assert dmx.ops.codebook_class(g, dtype) == "group"
        check(dmx.ops, make("heavy", (3, 2 * g), seed=g, dtype=dtype, block=g), R.TABLES[name], "per_group", g, cuda)
        check(dmx.ops, make("mixed_nd", (257, 1024), seed=g + 1, dtype=dtype, block=g), R.TABLES[name], "per_group", g, cuda)
    check(dmx.ops, make("zeros", (3, 128), dtype=dtype), R.TABLES[name], "per_group", 64, cuda)


def test_groups_deep_grid(dmx, cuda):
    """[8200, 1024] bf16 = 1,049,600 vectors, more than 2^19: the four-vectors-per-lane build of the group kernel, whose last workgroup is
    only partly filled (up to 524,800 segments: the chain runs in pieces)"""
    x = make("heavy", (8200, 1024), seed=3, dtype=BF16)
    check(dmx.ops, x, R.NF4, "per_group", 64, cuda)
    check(dmx.ops, x, R.IRREGULAR5, "per_group", 16, cuda)


@DTYPES
@pytest.mark.parametrize("L", [48, 768, 4096, 8192, 8200, 16384])
def test_whole_rows(dmx, cuda, L, dtype):
    """short rows (48: lanes idle), a wave per row (768; 4096: the last a wave takes), a workgroup per row (8192 sixteen-bit, 8200 with
    idle slots, 16384 with every slot filled)"""
    V = 4 if dtype == F32 else 8
    want_cls = "short_row" if L // V < 64 else "wave_row" if L // V <= (16 if V == 4 else 8) * 64 else "block_row"
    assert dmx.ops.codebook_class(L, dtype, True) == want_cls == dmx.ops.dynamic_float_class(L, dtype, "per_token")
    x = make("heavy", (5 if L >= 8192 else 67, L), seed=L, dtype=dtype, block=64)
    for name in R.TABLES:
        check(dmx.ops, x, R.TABLES[name], "per_token", None, cuda)


def test_per_tensor(dmx, cuda):
    for shape, kernel in (((4, 8, 96), True), ((300, 1000), False)):     # 3072 elements: one row on the kernel; 300 000: the chain
        x = make("heavy", shape, seed=9, dtype=BF16)
        if kernel:
            y, sc, idx = check(dmx.ops, x, R.NF4, "per_tensor", None, cuda)
        else:
            with pytest.raises(NotImplementedError):
                dmx.ops.codebook_qdq(x.to(cuda), "nf4", "per_tensor", fused=True)
            got = chain(dmx.ops, x.to(cuda), "nf4", "per_tensor", None, fused_arg=None, return_scale=True, return_index=True)
            same3(got, R.codebook_ref(x, R.NF4, "per_tensor"), shape)
            sc = got[1]
        assert sc.shape == (1,)


def test_more_than_2_31_elements(dmx, cuda):
    """[699405, 3072] bf16 = 2,148,572,160 elements in groups of 64: vector and segment indices past 2^31 / 2^25.  The full-size call runs
    first; then regions of fewer than 2^31 elements -- the first rows, 64 rows straddling element 2^31, the last 64 rows -- run as calls
    of their own on contiguous aligned views and must reproduce their rows of the full outputs bit for bit, and the two windows beyond
    the boundary are checked against the CPU checker as well"""
    shape = LC.A
    n = LC.numel(shape)
    assert n > LC.TWO31
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    need = n * (2 + 2 + 1) + n // 64 * 4 + 2 * LC.GIB
    if free < need:
        pytest.skip(f"needs {need / LC.GIB:.1f} GiB of device memory, {free / LC.GIB:.1f} GiB free")
    x = LC.device_input("normal", shape, BF16, 11, cuda)
    y, sc, idx = fused(dmx.ops, x, "nf4", "per_group", 64, return_scale=True, return_index=True)
    torch.cuda.synchronize()
    r2 = LC.TWO31 // shape[1]
    per_row = shape[1] // 64
    for a, b in ((0, 64), (r2 - 32, r2 + 32), (shape[0] - 64, shape[0])):
        ya, sa, ia = fused(dmx.ops, x[a:b], "nf4", "per_group", 64, return_scale=True, return_index=True)
        same3((y[a:b], sc[a * per_row:b * per_row], idx[a:b]), (ya, sa, ia), ("region", a, b))
        if a:
            same3((ya, sa, ia), R.codebook_ref(x[a:b].cpu(), R.NF4, "per_group", 64), ("checker", a, b))
    del x, y, sc, idx
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------- ties, special segments, norm
def _neighbours(t):
    b = t.view(torch.int32)
    return torch.cat([t, (b + 1).view(F32), (b - 1).view(F32)])


@TABLES
def test_ties(dmx, cuda, name):
    """f32 segments whose maximum is exactly the norm, so that s = 1 and u = x: every threshold of the table and its two fp32 neighbours"""
    levels = R.TABLES[name]
    c, t, z = R.table(levels)
    norm = float(R.norm_of(c)[0])
    pts = _neighbours(t)
    x = torch.zeros(2, 64)
    x[0, :pts.numel()] = pts
    x[1, :pts.numel()] = pts.flip(0)
    x[:, -1] = torch.tensor([norm, -norm])
    for gran, g in (("per_group", 64), ("per_token", None)):
        y, sc, idx = check(dmx.ops, x, levels, gran, g, cuda)
        assert torch.equal(sc.cpu(), torch.ones(2))
        for j in range(t.numel()):   # the threshold itself stays on the lower side
            assert int(idx[0, j]) == int((t < t[j]).sum())


@DTYPES
def test_special_segments(dmx, cuda, dtype):
    """all-zero, one NaN, +-Inf, a denormal maximum (s < 2^-126 gives s = 1), scales outside [2^-20, 2^20] and values outside
    div_by_recip's proven range beside an ordinary maximum: the wave-uniform `/` redo"""
    g = 64
    x = make("heavy", (16, g), seed=21, dtype=F32)
    x[0] = 0.0
    x[1, 5] = float("nan")
    x[2, 7] = float("inf")
    x[3, 9] = float("-inf")
    x[4, 0], x[4, 1] = float("inf"), float("-inf")
    x[5] = x[5] * 2.0 ** -135                      # a denormal maximum (fp16: flushed to an all-zero segment, s = 1 as well)
    x[6] = x[6].clamp(-4, 4) * 2.0 ** 40           # s far above 2^20
    x[7] = x[7].clamp(-4, 4) * 2.0 ** -40          # s far below 2^-20
    x[8, :4] = torch.tensor([2.0 ** -110, -2.0 ** -120, 2.0 ** -126, 2.0 ** -140])   # below 2^-100 beside an ordinary maximum
    x[9, :2] = torch.tensor([2.0 ** 110, -2.0 ** 101])                                # above 2^100: s = 2^110 / norm
    x[10, 3] = -0.0
    if dtype == F16:
        x = x.clamp(-65504.0, 65504.0)             # (keeps +-Inf out; rows 2 - 4 get them back below)
        x[2, 7], x[3, 9], x[4, 0], x[4, 1] = float("inf"), float("-inf"), float("inf"), float("-inf")
    x = x.to(dtype)
    for name in ("nf4", "irregular5"):
        y, sc, idx = check(dmx.ops, x, R.TABLES[name], "per_group", g, cuda)
        z = R.table(R.TABLES[name])[2]
        sc = sc.cpu()
        assert sc[0] == 1 and sc[1] == 1 and sc[2] == 1 and sc[3] == 1 and sc[4] == 1
        assert int(idx[1, 5]) == z and int(idx[0, 0]) == z and not bool(torch.isnan(y.float()).any())
        assert int(idx[4, 0]) == len(R.TABLES[name]) - 1 and int(idx[4, 1]) == 0
        check(dmx.ops, x.reshape(4, 4 * g), R.TABLES[name], "per_token", None, cuda)


def test_norm_and_device_tables(dmx, cuda):
    ops = dmx.ops
    x = make("heavy", (67, 768), seed=31, dtype=BF16)
    xd = x.to(cuda)
    for levels in (R.NF4, R.FP4_E2M1, R.IRREGULAR5):
        own = float(max(abs(levels[0]), abs(levels[-1])))
        a = check(ops, x, levels, "per_group", 64, cuda, norm=None)
        b = check(ops, x, levels, "per_group", 64, cuda, norm=own)          # the explicit value of the default: the same bits
        same3(a, b, "explicit default norm")
        c = check(ops, x, levels, "per_token", None, cuda, norm=2.5)        # another norm: the scales change
        assert bits_equal(c[1].cpu(), R.codebook_ref(x, levels, "per_token", None, None)[1]) > 0
        dev = torch.tensor(levels, dtype=F32, device=cuda)                   # a device table: taken as is, the same bits
        for norm in (None, 2.5):
            same3(fused(ops, xd, dev, "per_group", 64, norm, return_scale=True, return_index=True),
                  fused(ops, xd, list(levels), "per_group", 64, norm, return_scale=True, return_index=True), "device table")
            same3(chain(ops, xd, dev, "per_group", 64, norm, return_scale=True, return_index=True),
                  R.codebook_ref(x, levels, "per_group", 64, norm), "device table, chain")
    y = fused(ops, xd, "nf4")                                                # the defaults: per_group 64, y alone
    assert torch.is_tensor(y) and bits_equal(y.cpu(), R.codebook_ref(x, R.NF4)[0]) == 0
    y, idx = fused(ops, xd, "nf4", return_index=True)
    assert idx.dtype == torch.uint8


def test_routing(dmx, cuda):
    """fused=True raises where the kernel does not apply; fused=None takes the chain there and still equals the checker"""
    ops = dmx.ops
    x = make("heavy", (8, 192), seed=41, dtype=BF16)
    xd = x.to(cuda)
    k17 = tuple(torch.linspace(-1, 1, 17).tolist())
    k256 = tuple(torch.linspace(-2, 2, 256).tolist())
    base = torch.zeros(8 * 192 + 8, dtype=BF16, device=cuda)
    view = base[1:1 + 8 * 192].reshape(8, 192)                                # 2 bytes past a 16-byte boundary
    view.copy_(xd)
    assert view.data_ptr() % 16 == 2
    cases = [(xd, k17, "per_group", 64, {}), (xd, k256, "per_token", None, {}), (xd, R.NF4, "per_group", 48, {}),
             (xd, R.NF4, "per_group", 64, {"out_dtype": F32}), (view, R.NF4, "per_group", 64, {})]
    for t, levels, gran, g, kw in cases:
        with pytest.raises(NotImplementedError):
            ops.codebook_qdq(t, levels, gran, g, fused=True, **kw)
        got = chain(ops, t, levels, gran, g, fused_arg=None, return_scale=True, return_index=True, **kw)
        same3(got, R.codebook_ref(x, levels, gran, g, out_dtype=kw.get("out_dtype")), (len(levels), gran, g, kw))
    before = dict(routes_of(ops))
    ops.codebook_qdq(xd, R.NF4, "per_group", 64)                              # fused=None where the kernel applies: the kernel
    assert routes_of(ops)["fused"] == before["fused"] + 1
    xg = xd.clone().requires_grad_(True)                                      # autograd: a straight-through estimator
    gout = make("normal", (8, 192), seed=43, dtype=BF16).to(cuda)
    ops.codebook_qdq(xg, "nf4").backward(gout)
    assert bits_equal(xg.grad, gout) == 0


def _capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()                                                                  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    return graph, out


def test_graph_capture(dmx, cuda):
    """a captured codebook_qdq and a captured codebook_fit iteration (accumulate, the update on the device, the cast with the new table)
    replay to the bits of the eager run: no host round trip on either"""
    ops = dmx.ops
    x0 = make("normal", (128, 768), seed=73, dtype=BF16)
    x1 = make("heavy", (128, 768), seed=79, dtype=BF16)
    buf = x0.to(cuda).clone()
    table = torch.tensor(R.NF4, device=cuda)
    graph, (y, sc, idx) = _capture(lambda: fused(ops, buf, table, "per_group", 64, return_scale=True, return_index=True))
    graph_fit, (c1, norm) = _capture(lambda: ops.codebook_fit(buf, table, "per_group", 64, norm=1.0, iters=1, fused=True))
    for x in (x1, x0):
        buf.copy_(x.to(cuda))
        graph.replay()
        graph_fit.replay()
        torch.cuda.synchronize()
        same3((y, sc, idx), R.codebook_ref(x, R.NF4, "per_group", 64), "replay")
        eager, _ = ops.codebook_fit(x.to(cuda), table, "per_group", 64, norm=1.0, iters=1, fused=True)
        assert norm == 1.0 and bits_equal(c1.cpu(), eager.cpu()) == 0


# ---------------------------------------------------------------------------------------------------- the Lloyd statistics
def _acc_routes(ops):
    return ops._codebook_accumulate_routes if hasattr(ops, "_codebook_accumulate_routes") else ops._front._codebook_accumulate_routes


def _close(A, ref, what):
    """counts equal exactly; the two sums within n 2^-52 sum|terms| of the checker's: the bound of a float64 sum of n terms in any order"""
    W, mag, wsum = ref
    A = A.cpu()
    assert torch.equal(A[:, 2], W[:, 2]), what
    n = W[:, 2]
    assert bool(((A[:, 0] - W[:, 0]).abs() <= n * 2.0 ** -52 * mag).all()), (what, A[:, 0], W[:, 0])
    assert bool(((A[:, 1] - W[:, 1]).abs() <= n * 2.0 ** -52 * wsum).all()), (what, A[:, 1], W[:, 1])


@pytest.mark.parametrize("shape,gran,g,dtype", [((257, 1024), "per_group", 64, BF16), ((3, 32), "per_group", 16, F32), ((67, 768), "per_token", None, F16),
                                                ((5, 8200), "per_token", None, BF16), ((8200, 1024), "per_group", 128, BF16),
                                                ((67, 4096), "per_token", None, F32)])
def test_accumulate(dmx, cuda, shape, gran, g, dtype):
    ops = dmx.ops
    x = make("heavy", shape, seed=shape[1], dtype=dtype)
    x[0, 3] = float("nan")          # its whole segment has s = 1; the NaN itself is skipped
    x[1, 5] = float("inf")          # skipped: u is not finite
    xd = x.to(cuda)
    deep = shape[0] * shape[1] > 1 << 22   # (the four-vectors-per-lane build: one table, the kernel alone -- the checker's sums take seconds there)
    for name in ("nf4",) if deep else ("nf4", "irregular5", "two"):
        levels = R.TABLES[name]
        ref = R.accumulate_ref(x, levels, gran, g)
        before = dict(_acc_routes(ops))
        A = ops.codebook_accumulate(xd, levels, gran, g, fused=True)
        assert _acc_routes(ops)["fused"] == before["fused"] + 1 and A.dtype == torch.float64 and A.shape == (len(levels), 3)
        _close(A, ref, (name, "kernel"))
        assert int(A[:, 2].sum()) < x.numel()                                 # the non-finite quotients were skipped
        again = ops.codebook_accumulate(xd, levels, gran, g, fused=True)
        assert torch.equal(A.cpu().view(torch.int64), again.cpu().view(torch.int64))   # the same input: the same bits
        if deep:
            continue
        _close(ops.codebook_accumulate(xd, levels, gran, g, fused=False), ref, (name, "index_add_"))
        if shape[0] % 2 == 0 or shape[0] > 4:                                 # accumulate=True over two parts == one call on the whole
            h = shape[0] // 2
            B = ops.codebook_accumulate(xd[:h], levels, gran, g, fused=True)
            B2 = ops.codebook_accumulate(xd[h:], levels, gran, g, acc=B, accumulate=True, fused=True)
            assert B2 is B
            _close(B, ref, (name, "two halves"))


def test_accumulate_routing(dmx, cuda):
    ops = dmx.ops
    x = make("heavy", (8, 192), seed=5, dtype=BF16)
    k17 = tuple(torch.linspace(-1, 1, 17).tolist())
    for levels, gran, g in ((k17, "per_group", 64), (R.NF4, "per_group", 48)):
        with pytest.raises(NotImplementedError):
            ops.codebook_accumulate(x.to(cuda), levels, gran, g, fused=True)
        _close(ops.codebook_accumulate(x.to(cuda), levels, gran, g), R.accumulate_ref(x, levels, gran, g), (len(levels), g))


# ---------------------------------------------------------------------------------------------------- the fit
@pytest.mark.parametrize("kind", ["normal", "heavy"])
def test_fit(dmx, cuda, kind):
    """f32 [64, 512], NF4 start, g = 64, 7 iterations.  The CPU restatement's worst ratio of successive errors is 0.99963; the slack of
    1e-5 covers the fp32 rounding of the levels."""
    ops = dmx.ops
    x = make(kind, (64, 512), seed=17, dtype=F32)
    xd = x.to(cuda)
    c, norm, hist = ops.codebook_fit(xd, "nf4", "per_group", 64, iters=7, return_history=True)
    assert norm == 1.0 and c.dtype == F32 and c.shape == (16,) and hist.dtype == torch.float64 and hist.shape == (8,) and hist.is_cuda
    h = hist.cpu().tolist()
    print("codebook_fit history", kind, h)
    assert all(b <= a * (1 + 1e-5) for a, b in zip(h, h[1:])), h
    assert h[-1] < h[0]
    assert bool((c[1:] >= c[:-1]).all())
    row = ops.error_stats(xd, ops.codebook_qdq(xd, c, "per_group", 64, norm))
    assert float(torch.sqrt(row[0] / row[1])) == h[-1]                       # the fitted table with the returned norm reproduces it
    c2, norm2 = ops.codebook_fit(xd, "nf4", "per_group", 64, iters=7)
    assert norm2 == norm and bits_equal(c2.cpu(), c.cpu()) == 0
    # one step against the checker: the float64 sums differ only in order, so the levels agree to 1 fp32 ulp
    one, _ = ops.codebook_fit(xd, "nf4", "per_group", 64, iters=1)
    want = R.lloyd_step(R.NF4, R.accumulate_ref(x, R.NF4, "per_group", 64)[0])
    ulps = (one.cpu().view(torch.int32) - want.view(torch.int32)).abs()
    assert int(ulps.max()) <= 1, (one.cpu(), want)
    # a list of tensors shares one table: the two halves give the table of the whole (the same sums up to their order)
    both, _ = ops.codebook_fit([xd[:32], xd[32:]], "nf4", "per_group", 64, iters=1)
    assert int((both.cpu().view(torch.int32) - want.view(torch.int32)).abs().max()) <= 1


def test_nf4_beats_int4_on_normal_data(dmx, cuda):
    """on normal data the NF4 table has a lower relative L2 error than the symmetric 4-bit integer grid under the same per-group-64
    absolute-maximum scale (the CPU restatement: 0.092 against 0.107, three seeds)"""
    ops = dmx.ops
    x = make("normal", (256, 1024), seed=0, dtype=BF16).to(cuda)
    e = lambda y: float(torch.sqrt((lambda r: r[0] / r[1])(ops.error_stats(x, y))))   # noqa: E731
    nf4 = e(ops.codebook_qdq(x, **ops.NF4))
    int4 = e(ops.dynamic_fixed_qdq(x, INT4, "per_group", 64, symmetric_qscheme=True))
    print("relative L2 error: nf4", nf4, "int4", int4)
    assert nf4 < int4


# ---------------------------------------------------------------------------------------------------- modules
def _linear(dmx, cuda, w, **config):
    m = dmx.nn.Linear(w.shape[1], w.shape[0], bias=False).to(cuda).to(w.dtype)
    with torch.no_grad():
        m.weight.copy_(w.to(cuda))
    m.configure(dict({"weight_format": INT4}, **config))
    return m


def test_linear_with_a_codebook_weight(dmx, cuda):
    ops = dmx.ops
    w = make("normal", (96, 256), seed=51, dtype=BF16)
    x = make("normal", (7, 256), seed=53, dtype=BF16).to(cuda)
    m = _linear(dmx, cuda, w, weight_codebook=ops.NF4)
    with torch.no_grad():
        want = F.linear(x, ops.codebook_qdq(w.to(cuda), **ops.NF4))
        assert bits_equal(m(x), want) == 0
        assert bits_equal(m.weight_cast(m.weight), ops.codebook_qdq(w.to(cuda), **ops.NF4)) == 0
    # measure_error: the error_stats row of that cast
    row = m.weight_cast.measure_error(m.weight)
    assert torch.equal(row.cpu(), ops.error_stats(w.to(cuda), ops.codebook_qdq(w.to(cuda), **ops.NF4)).cpu())
    # fit, save, load into a fresh module: the same forward
    m.weight_cast.fit_codebook(m.weight, iters=4)
    s = m.weight_cast.codebook_setting
    assert s["norm"] == 1.0 and s["per_group"] == 64 and s["codebook"] != list(R.NF4)
    with torch.no_grad():
        fitted = m(x)
        assert bits_equal(fitted, F.linear(x, ops.codebook_qdq(w.to(cuda), m.weight_cast.codebook, "per_group", 64, 1.0))) == 0
        assert bits_equal(fitted, want) > 0
    fresh = _linear(dmx, cuda, torch.zeros_like(w), weight_codebook=ops.NF4)
    fresh.load_state_dict(m.state_dict())
    with torch.no_grad():
        assert bits_equal(fresh(x), fitted) == 0
    after = m.weight_cast.measure_error(m.weight)
    assert float(after[0]) < float(row[0])                                   # the fitted table has the smaller squared error
    # a SAME cast stays the identity; switching the codebook off returns to the format's own arithmetic
    same = dmx.nn.Linear(256, 96, bias=False).to(cuda).to(BF16)
    same.configure({"weight_codebook": ops.NF4})
    with torch.no_grad():
        assert bits_equal(same(x), F.linear(x, same.weight)) == 0
    m.configure({"weight_codebook": None})
    with torch.no_grad():
        assert bits_equal(m.weight_cast(m.weight), dmx.CastTo(format=INT4).to(cuda)(m.weight)) == 0


def test_calibration_refuses_a_codebook_weight(dmx, cuda):
    w = make("normal", (96, 256), seed=57, dtype=BF16)
    m = _linear(dmx, cuda, w, weight_codebook=dmx.ops.NF4)
    with pytest.raises(NotImplementedError, match="codebook"):
        m.fold_weight_and_bias()
    from dmx_compressor_amd import layer_reconstruction as LR
    for cls, args in ((LR.OptimalBrainCompressor, ()), (LR.WandaCalibrator, ()), (LR.AWQCalibrator, (dmx.nn.DmxAWQHyperparams(),))):
        with pytest.raises(NotImplementedError, match="codebook"):
            cls(m, *args)
