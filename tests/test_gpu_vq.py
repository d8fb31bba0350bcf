"""GPU tests of the vector codebook casts (csrc/vq.hip, ops.vq_qdq / vq_accumulate / vq_fit, CastTo.set_vq; DESIGN.md §8 "Vector
codebook casts"): the fused kernel against the CPU checker of tests/_vq_ref.py (the definition) and against the library's own chain of
torch operations on the GPU, bit for bit on the output, the scales and the indices; the k-means statistics against the checker's
float64 sums within the bound of a reordered float64 sum; the fit against the checker's step and the properties of a Lloyd iteration."""
import pytest
import torch
import torch.nn.functional as F

import _large_cases as LC
import _vq_ref as R
from _data import bits_equal, make

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=["bf16", "f16", "f32"])
DIMS = pytest.mark.parametrize("d", [2, 4, 8])
INT4 = "XP[4,0](CSN)"
KS = (2, 16, 200, 256)


@pytest.fixture(autouse=True)
def _stop_the_session_after_a_gpu_fault():
    """a HIP error after a test (an illegal access is sticky) ends the session: nothing more is started on a faulted device"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # pragma: no cover
        pytest.exit(f"GPU fault, stopping the session: {e}", returncode=3)


def rows_of(kind, K, d, seed=0):
    """random: unsorted normal rows; dup: the same with every third row a copy of row 0 and the last row a copy of row 1;
    grid: the product table of a uniform scalar codebook with about K ** (1 / d) levels, at least 2 (ops.vq_grid's rows)"""
    if kind == "grid":
        n = max(2, int(K ** (1.0 / d) + 1e-9))
        while n ** d > 256:
            n -= 1
        return R.grid(torch.linspace(-1.0, 1.0, n, dtype=F32).tolist(), d)
    c = make("normal", (K, d), seed=1000 * d + K + seed, dtype=F32)
    if kind == "dup":
        c[::3] = c[0].clone()
        c[-1] = c[1].clone()
    return c


def routes_of(ops):
    return ops._vq_routes if hasattr(ops, "_vq_routes") else ops._front._vq_routes


def fused(ops, x, rows, granularity="per_group", g=64, norm=None, **kw):
    """ops.vq_qdq(..., fused=True), asserting on the host-side route counter that the kernel ran (and the chain did not)"""
    before = dict(routes_of(ops))
    out = ops.vq_qdq(x, rows, granularity, g, norm, fused=True, **kw)
    assert routes_of(ops)["fused"] == before["fused"] + 1 and routes_of(ops)["chain"] == before["chain"]
    return out


def chain(ops, x, rows, granularity="per_group", g=64, norm=None, fused_arg=False, **kw):
    before = dict(routes_of(ops))
    out = ops.vq_qdq(x, rows, granularity, g, norm, fused=fused_arg, **kw)
    assert routes_of(ops)["chain"] == before["chain"] + 1 and routes_of(ops)["fused"] == before["fused"]
    return out


def same3(got, want, what):
    (y, sc, idx), (wy, wsc, widx) = got, want
    assert y.dtype == wy.dtype and y.shape == wy.shape and sc.dtype == F32 and idx.dtype == torch.uint8 and idx.shape == widx.shape, what
    assert sc.shape == wsc.shape and bits_equal(sc.cpu(), wsc.cpu()) == 0, what
    assert torch.equal(idx.cpu(), widx.cpu()), what
    assert bits_equal(y.cpu(), wy.cpu()) == 0, what


def check(ops, x, rows, granularity, g, cuda, norm=None, kernel=True):
    """kernel == checker and chain == checker on y, scale and index, the checker's answer computed once for both (kernel=False: a call
    the kernel refuses)"""
    xd = x.to(cuda)
    table = rows.to(cuda) if torch.is_tensor(rows) else rows
    K, d = (rows.shape if torch.is_tensor(rows) else (len(rows), len(rows[0])))
    what = (K, d, granularity, g, norm, tuple(x.shape), x.dtype)
    want = R.vq_ref(x, rows, granularity, g, norm)
    assert want[2].shape == tuple(x.shape[:-1]) + (x.shape[-1] // d,)
    same3(chain(ops, xd, table, granularity, g, norm, return_scale=True, return_index=True), want, what + ("chain",))
    if not kernel:
        with pytest.raises(NotImplementedError):
            ops.vq_qdq(xd, table, granularity, g, norm, fused=True)
        return None
    got = fused(ops, xd, table, granularity, g, norm, return_scale=True, return_index=True)
    same3(got, want, what + ("kernel",))
    return got


# ---------------------------------------------------------------------------------------------------- the kernel's geometries
# the smallest shapes that reach each geometry: (shape, granularity, g)
GEOMETRIES = [((4, 256), "per_group", 64), ((3, 192), "per_group", 64), ((300, 256), "per_group", 16), ((300, 256), "per_group", 256),
              ((5, 48), "per_token", None), ((3, 768), "per_token", None), ((2, 8200), "per_token", None), ((2, 520), "per_tensor", None)]


@DIMS
@DTYPES
def test_geometries(dmx, cuda, dtype, d):
    """every geometry, every K, heavy-tailed inputs; the table kind rotates with the case so that random, duplicated and grid tables all
    meet every dtype and d.  float32 with d = 8: the kernel refuses, the chain is held to the checker (K = 256 included)"""
    ops = dmx.ops
    kernel = not (dtype == F32 and d == 8)
    kinds = ("random", "dup", "grid")
    n = 0
    for shape, gran, g in GEOMETRIES:
        x = make("heavy", shape, seed=shape[1] + (g or 0), dtype=dtype, block=g or 64)
        S = {"per_group": g, "per_token": shape[1], "per_tensor": shape[0] * shape[1]}[gran]
        for K in KS:
            assert (ops.vq_class(S, dtype, d, K, gran != "per_group") is not None) == kernel
            check(ops, x, rows_of(kinds[n % 3], K, d), gran, g, cuda, kernel=kernel)
            n += 1


def test_groups_deep_grid(dmx, cuda):
    """[1025, 2048] bf16 = 262,400 vectors, more than 2^18: the four-vectors-per-lane build of the group kernel, whose last workgroup is
    only partly filled; and [1024, 2048], exactly 2^18: the last size of the one-vector build"""
    for rows_n in (1025, 1024):
        x = make("heavy", (rows_n, 2048), seed=3, dtype=BF16)
        check(dmx.ops, x, rows_of("random", 16, 4), "per_group", 64, cuda)
    check(dmx.ops, x[:, :1024].contiguous(), rows_of("dup", 5, 2), "per_group", 16, cuda)


@DIMS
def test_groups_the_kernel_refuses(dmx, cuda, d):
    """g = 24 is no power of two: the chain alone, bit for bit with the checker; fused=None takes it by itself"""
    ops = dmx.ops
    x = make("heavy", (6, 96), seed=d, dtype=BF16, block=24)
    check(ops, x, rows_of("random", 16, d), "per_group", 24, cuda, kernel=False)
    got = chain(ops, x.to(cuda), rows_of("random", 16, d), "per_group", 24, fused_arg=None, return_scale=True, return_index=True)
    same3(got, R.vq_ref(x, rows_of("random", 16, d), "per_group", 24), "fused=None")


def test_per_tensor_beyond_the_kernel(dmx, cuda):
    x = make("heavy", (300, 1000), seed=9, dtype=BF16)                   # 300 000 elements in one segment: the chain
    got = check(dmx.ops, x, rows_of("random", 16, 4), "per_tensor", None, cuda, kernel=False)
    assert got is None


# ---------------------------------------------------------------------------------------------------- ties, special segments, norm
@DIMS
def test_ties_and_special_vectors(dmx, cuda, d):
    """f32 segments whose maximum is exactly the norm, so that s = 1 and u = x.  Rows +-e_0 / 2 and their duplicates: the vectors 0,
    e_1 / 4 and their fp32 neighbours are exact ties or one ulp off them; (NaN, 1, ...), (Inf, 0, ...), -0.0 in the middle of a segment"""
    dtype, g = (BF16 if d == 8 else F32), 64                             # (float32 has no d = 8 kernel; these values are exact in bf16)
    e0 = [0.5] + [0.0] * (d - 1)
    rows = torch.tensor([[-v for v in e0], e0, [-v for v in e0], e0, [0.5] * d])
    x = torch.zeros(6, g)
    x[0, :d] = torch.tensor(e0)                                          # amax = 0.5 = the default norm: s = 1
    x[0, 2 * d + 1] = 0.25                                               # u = e_1 / 4: rows 0 and 1 tie, row 0 wins
    x[0, 3 * d] = 2.0 ** -20                                             # one step towards row 1
    x[0, 4 * d] = -2.0 ** -20                                            # one step towards row 0
    x[0, 5 * d] = -0.0
    x[1] = x[0]
    x[1, 7 * d], x[1, 7 * d + 1] = float("nan"), 1.0                     # the segment's scale falls back to 1 as well
    x[2] = x[0]
    x[2, 6 * d] = float("inf")
    x[3] = x[0]
    x[3, 6 * d] = float("-inf")
    x[4] = 0.0                                                           # an all-zero segment
    x[5, :d] = 2.0 ** -130                                               # a subnormal maximum: s < 2^-126 gives s = 1 (bf16 keeps 2^-130)
    x = x.to(dtype)
    for gran, gg in (("per_group", g), ("per_token", None)):
        y, sc, idx = check(dmx.ops, x, rows, gran, gg, cuda)
        idx, sc = idx.cpu(), sc.cpu()
        z = R.zero_row(R.table(rows))
        assert z == 0 and torch.equal(sc, torch.ones(6))
        assert idx[0].tolist()[:6] == [1, 0, 0, 1, 0, 0]                 # e_0 / 2 itself; the tie at 0; e_1 / 4; the two steps; -0.0
        assert int(idx[1, 7]) == z and int(idx[2, 6]) == z and int(idx[3, 6]) == z and bool((idx[4] == z).all())
        assert not bool(torch.isnan(y.float()).any())


@DTYPES
def test_special_segments(dmx, cuda, dtype):
    """NaN, +-Inf, scales outside [2^-20, 2^20] and values outside div_by_recip's proven range beside an ordinary maximum (the
    wave-uniform `/` redo), squares that overflow: planted in the middle of heavy-tailed segments"""
    g = 64
    x = make("heavy", (12, g), seed=21, dtype=F32)
    x[0] = 0.0
    x[1, 37] = float("nan")
    x[2, 29] = float("inf")
    x[3, 41] = float("-inf")
    x[4, 30], x[4, 33] = float("inf"), float("-inf")
    x[5] = x[5] * 2.0 ** -135
    x[6] = x[6].clamp(-4, 4) * 2.0 ** 40
    x[7] = x[7].clamp(-4, 4) * 2.0 ** -40
    x[8, 20:24] = torch.tensor([2.0 ** -110, -2.0 ** -120, 2.0 ** -126, 2.0 ** -140])
    x[9, 20:22] = torch.tensor([2.0 ** 110, -2.0 ** 101])
    x[10, 35] = -0.0
    if dtype == F16:
        x = x.clamp(-65504.0, 65504.0)
        x[2, 29], x[3, 41], x[4, 30], x[4, 33] = float("inf"), float("-inf"), float("inf"), float("-inf")
    x = x.to(dtype)
    for d in (2, 4) if dtype == F32 else (2, 4, 8):
        rows = rows_of("random", 16, d, seed=5)
        y, sc, idx = check(dmx.ops, x, rows, "per_group", g, cuda)
        z = R.zero_row(R.table(rows))
        sc, idx = sc.cpu(), idx.cpu()
        assert all(float(sc[i]) == 1.0 for i in range(5))
        assert int(idx[1, 37 // d]) == z and int(idx[2, 29 // d]) == z and int(idx[3, 41 // d]) == z and bool((idx[0] == z).all())
        assert not bool(torch.isnan(y.float()).any())
        check(dmx.ops, x.reshape(3, 4 * g), rows, "per_token", None, cuda)
        big = rows * 1e30                                                # u - c of the order 1e30: every square overflows, z everywhere
        _, _, ib = check(dmx.ops, x[6:8].contiguous(), big, "per_group", g, cuda)
        assert bool((ib.cpu() == R.zero_row(R.table(big))).all())


def test_norm_and_device_tables(dmx, cuda):
    ops = dmx.ops
    x = make("heavy", (67, 768), seed=31, dtype=BF16)
    xd = x.to(cuda)
    rows = rows_of("random", 16, 4)
    own = float(rows.abs().max())
    a = check(ops, x, rows, "per_group", 64, cuda, norm=None)
    b = check(ops, x, rows, "per_group", 64, cuda, norm=own)                 # the explicit value of the default: the same bits
    same3(a, b, "explicit default norm")
    c = check(ops, x, rows, "per_token", None, cuda, norm=2.5)               # another norm: the scales change
    assert bits_equal(c[1].cpu(), R.vq_ref(x, rows, "per_token", None, None)[1]) > 0
    for norm in (None, 2.5):                                                 # a list of rows and a CPU tensor: uploaded, the same bits
        same3(fused(ops, xd, rows.tolist(), "per_group", 64, norm, return_scale=True, return_index=True),
              fused(ops, xd, rows.to(cuda), "per_group", 64, norm, return_scale=True, return_index=True), "host table")
    grid = {"grid": "uniform4", "dim": 4}
    same3(fused(ops, xd, grid, return_scale=True, return_index=True), R.vq_ref(x, R.grid(torch.linspace(-1, 1, 4).tolist(), 4)), "grid")
    y = fused(ops, xd, rows)                                                 # the defaults: per_group 64, y alone
    assert torch.is_tensor(y) and bits_equal(y.cpu(), a[0].cpu()) == 0
    y, idx = fused(ops, xd, rows, return_index=True)
    assert idx.dtype == torch.uint8 and idx.shape == (67, 192)
    y2 = fused(ops, xd, rows, per_group=64)
    assert bits_equal(y2, y) == 0


def test_routing(dmx, cuda):
    """fused=True raises where the kernel does not apply; fused=None takes the chain there and still equals the checker"""
    ops = dmx.ops
    x = make("heavy", (8, 192), seed=41, dtype=BF16)
    xd = x.to(cuda)
    rows = rows_of("random", 16, 4)
    base = torch.zeros(8 * 192 + 8, dtype=BF16, device=cuda)
    view = base[1:1 + 8 * 192].reshape(8, 192)                                # 2 bytes past a 16-byte boundary
    view.copy_(xd)
    assert view.data_ptr() % 16 == 2
    cases = [(xd, "per_group", 48, {}), (xd, "per_group", 64, {"out_dtype": F32}), (view, "per_group", 64, {}), (view, "per_token", None, {})]
    for t, gran, g, kw in cases:
        with pytest.raises(NotImplementedError):
            ops.vq_qdq(t, rows, gran, g, fused=True, **kw)
        got = chain(ops, t, rows, gran, g, fused_arg=None, return_scale=True, return_index=True, **kw)
        same3(got, R.vq_ref(x, rows, gran, g, out_dtype=kw.get("out_dtype")), (gran, g, kw))
    before = dict(routes_of(ops))
    ops.vq_qdq(xd, rows, "per_group", 64)                                     # fused=None where the kernel applies and is not listed
    took = "chain" if ops.vq_class(64, BF16, 4, 16) in ops.VQ_CHAIN_BY_DEFAULT else "fused"
    assert routes_of(ops)[took] == before[took] + 1
    xg = xd.clone().requires_grad_(True)                                      # autograd: a straight-through estimator
    gout = make("normal", (8, 192), seed=43, dtype=BF16).to(cuda)
    ops.vq_qdq(xg, rows).backward(gout)
    assert bits_equal(xg.grad, gout) == 0
    e = ops.vq_qdq(torch.empty(0, 64, dtype=BF16, device=cuda), rows, return_index=True)
    assert e[0].shape == (0, 64) and e[1].shape == (0, 16)


def test_more_than_2_31_elements(dmx, cuda):
    """[699405, 3072] bf16 = 2,148,572,160 elements in groups of 64 under a [2, 8] table: vector and segment indices past 2^31 / 2^25.
    The first rows, 64 rows straddling element 2^31 and the last 64 rows of the full-size call against the CPU checker"""
    shape = LC.A
    n = LC.numel(shape)
    assert n > LC.TWO31
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    need = n * (2 + 2) + n // 8 + n // 64 * 4 + 2 * LC.GIB
    if free < need:
        pytest.skip(f"needs {need / LC.GIB:.1f} GiB of device memory, {free / LC.GIB:.1f} GiB free")
    x = LC.device_input("normal", shape, BF16, 11, cuda)
    rows = torch.tensor([[0.5, -0.25, 0.75, 0.0, -0.5, 0.25, -1.0, 1.0], [-0.5, 0.5, -0.25, 0.25, 1.0, -0.75, 0.5, -1.0]])
    y, sc, idx = fused(dmx.ops, x, rows.to(cuda), "per_group", 64, return_scale=True, return_index=True)
    torch.cuda.synchronize()
    assert idx.shape == (shape[0], shape[1] // 8)
    r2 = LC.TWO31 // shape[1]
    per_row = shape[1] // 64
    for a, b in ((0, 64), (r2 - 32, r2 + 32), (shape[0] - 64, shape[0])):
        same3((y[a:b], sc[a * per_row:b * per_row], idx[a:b]), R.vq_ref(x[a:b].cpu(), rows, "per_group", 64), ("checker", a, b))
    del x, y, sc, idx
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------- capture
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
    """a captured cast + accumulate, and a captured vq_fit iteration, replay to the bits of the eager run: no host round trip"""
    ops = dmx.ops
    x0 = make("normal", (128, 768), seed=73, dtype=BF16)
    x1 = make("heavy", (128, 768), seed=79, dtype=BF16)
    buf = x0.to(cuda).clone()
    rows = rows_of("random", 16, 4)
    table = rows.to(cuda)
    acc = torch.zeros(16, 6, dtype=torch.float64, device=cuda)

    def both():
        out = fused(ops, buf, table, "per_group", 64, return_scale=True, return_index=True)
        ops.vq_accumulate(buf, table, "per_group", 64, acc=acc, fused=True)
        return out

    graph, (y, sc, idx) = _capture(both)
    graph_fit, (c1, norm) = _capture(lambda: ops.vq_fit(buf, codebook=table, per_group=64, norm=1.0, iters=1, fused=True))
    for x in (x1, x0):
        buf.copy_(x.to(cuda))
        graph.replay()
        graph_fit.replay()
        torch.cuda.synchronize()
        same3((y, sc, idx), R.vq_ref(x, rows, "per_group", 64), "replay")
        eager = ops.vq_accumulate(x.to(cuda), table, "per_group", 64, fused=True)
        assert torch.equal(acc.cpu().view(torch.int64), eager.cpu().view(torch.int64))
        eager_c, _ = ops.vq_fit(x.to(cuda), codebook=table, per_group=64, norm=1.0, iters=1, fused=True)
        assert norm == 1.0 and bits_equal(c1.cpu(), eager_c.cpu()) == 0


# ---------------------------------------------------------------------------------------------------- the k-means statistics
def _acc_routes(ops):
    return ops._vq_accumulate_routes if hasattr(ops, "_vq_accumulate_routes") else ops._front._vq_accumulate_routes


def _close(A, ref_, d, what):
    """counts equal exactly; every sum within n_k 2^-52 (its magnitude sum) of the checker's: the bound of a float64 sum of n_k terms
    taken in any order"""
    W, mag = ref_
    A = A.cpu()
    assert torch.equal(A[:, d + 1], W[:, d + 1]), what
    n = W[:, d + 1:d + 2]
    assert bool(((A[:, :d + 1] - W[:, :d + 1]).abs() <= n * 2.0 ** -52 * mag).all()), (what, A, W)


@pytest.mark.parametrize("shape,gran,g,dtype,d,K", [
    ((257, 1024), "per_group", 64, BF16, 4, 256), ((3, 32), "per_group", 16, F32, 2, 2), ((67, 768), "per_token", None, F16, 8, 16),
    ((5, 8200), "per_token", None, BF16, 2, 200), ((1025, 2048), "per_group", 128, BF16, 8, 16), ((67, 4096), "per_token", None, F32, 4, 16),
    ((300, 256), "per_group", 16, F16, 2, 256), ((2, 520), "per_tensor", None, BF16, 4, 5)])
def test_accumulate(dmx, cuda, shape, gran, g, dtype, d, K):
    ops = dmx.ops
    x = make("heavy", shape, seed=shape[1], dtype=dtype)
    x[0, 3] = float("nan")          # its whole segment has s = 1; the vector with the NaN is skipped
    x[1, 5] = float("inf")          # skipped: a quotient is not finite
    xd = x.to(cuda)
    rows = rows_of("dup" if K == 5 else "random", K, d)
    table = rows.to(cuda)
    want = R.accumulate_ref(x, rows, gran, g)
    before = dict(_acc_routes(ops))
    A = ops.vq_accumulate(xd, table, gran, g, fused=True)
    assert _acc_routes(ops)["fused"] == before["fused"] + 1 and A.dtype == torch.float64 and A.shape == (K, d + 2)
    _close(A, want, d, "kernel")
    assert int(A[:, d + 1].sum()) < x.numel() // d                         # the non-finite vectors were skipped
    again = ops.vq_accumulate(xd, table, gran, g, fused=True)
    assert torch.equal(A.cpu().view(torch.int64), again.cpu().view(torch.int64))   # the same input: the same bits
    _close(ops.vq_accumulate(xd, table, gran, g, fused=False), want, d, "index_add_")
    if shape[0] > 4:                                                       # accumulate=True over two parts == the sum of the two
        h = shape[0] // 2
        B = ops.vq_accumulate(xd[:h], table, gran, g, fused=True)
        first = B.clone()
        second = ops.vq_accumulate(xd[h:], table, gran, g, fused=True)
        B2 = ops.vq_accumulate(xd[h:], table, gran, g, acc=B, accumulate=True, fused=True)
        assert B2 is B and torch.equal(B.cpu().view(torch.int64), (first + second).cpu().view(torch.int64))
        _close(B, want, d, "two halves")


def test_accumulate_routing(dmx, cuda):
    ops = dmx.ops
    x = make("heavy", (8, 192), seed=5, dtype=BF16)
    rows = rows_of("random", 16, 4)
    with pytest.raises(NotImplementedError):
        ops.vq_accumulate(x.to(cuda), rows, "per_group", 48, fused=True)
    _close(ops.vq_accumulate(x.to(cuda), rows, "per_group", 48), R.accumulate_ref(x, rows, "per_group", 48), 4, "g = 48")
    xf = x.float()
    with pytest.raises(NotImplementedError):
        ops.vq_accumulate(xf.to(cuda), rows_of("random", 16, 8), "per_group", 64, fused=True)
    _close(ops.vq_accumulate(xf.to(cuda), rows_of("random", 16, 8), "per_group", 64), R.accumulate_ref(xf, rows_of("random", 16, 8), "per_group", 64), 8, "f32 d = 8")


# ---------------------------------------------------------------------------------------------------- the fit
@pytest.mark.parametrize("kind,d,K", [("normal", 2, 16), ("heavy", 4, 16), ("normal", 8, 4)])
def test_fit(dmx, cuda, kind, d, K):
    """f32 (bf16 at d = 8) [64, 256], the sample init, g = 64, 6 iterations.  The history may rise by the scalar fit's allowance of 1e-5
    per step: the fp32 rounding of the updated rows."""
    ops = dmx.ops
    dtype = BF16 if d == 8 else F32
    x = make(kind, (64, 256), seed=17, dtype=dtype)
    xd = x.to(cuda)
    c0, norm0 = ops.vq_fit(xd, K, d, per_group=64, iters=0)
    assert norm0 == 1.0 and bits_equal(c0.cpu(), R.sample_init(x, K, d, "per_group", 64)) == 0       # the sample init is the checker's
    c, norm, hist = ops.vq_fit(xd, K, d, per_group=64, iters=6, return_history=True)
    assert norm == 1.0 and c.dtype == F32 and c.shape == (K, d) and hist.dtype == torch.float64 and hist.shape == (7,) and hist.is_cuda
    h = hist.cpu().tolist()
    print("vq_fit history", kind, d, K, h)
    assert all(b <= a * (1 + 1e-5) for a, b in zip(h, h[1:])), h
    assert h[-1] < h[0]
    row = ops.error_stats(xd, ops.vq_qdq(xd, c, "per_group", 64, norm))
    assert float(torch.sqrt(row[0] / row[1])) == h[-1]                       # the fitted table with the returned norm reproduces it
    c2, norm2 = ops.vq_fit(xd, K, d, per_group=64, iters=6)
    assert norm2 == norm and bits_equal(c2.cpu(), c.cpu()) == 0
    # per iteration: the device update of a given A equals the checker's step on that A, bit for bit
    cur = c0
    for _ in range(3):
        A = ops.vq_accumulate(xd, cur, "per_group", 64, 1.0)
        nxt, _ = ops.vq_fit(xd, codebook=cur, per_group=64, norm=1.0, iters=1)
        assert bits_equal(nxt.cpu(), R.kmeans_step(cur.cpu(), A.cpu())) == 0
        cur = nxt
    # a list of tensors shares one table: the two halves give the statistics of the whole up to their order (1 fp32 ulp on the rows)
    both, _ = ops.vq_fit([xd[:32], xd[32:]], codebook=c0, per_group=64, norm=1.0, iters=1)
    one, _ = ops.vq_fit(xd, codebook=c0, per_group=64, norm=1.0, iters=1)
    assert int((both.cpu().view(torch.int32) - one.cpu().view(torch.int32)).abs().max()) <= 1


def test_fitted_pairs_beat_the_scalar_grid_at_the_same_bits(dmx, cuda):
    """64 x 256 correlated pairs (the second of a pair is the first plus a quarter of fresh noise), groups of 64: a fitted K = 16, d = 2
    table (4 bits per pair) against the scalar "uniform4" codebook (2 bits per element) under the same scale rule"""
    ops = dmx.ops
    a = make("normal", (64, 128), seed=7, dtype=F32)
    b = a + 0.25 * make("normal", (64, 128), seed=8, dtype=F32)
    x = torch.stack([a, b], dim=-1).reshape(64, 256).to(cuda)
    e = lambda y: float(torch.sqrt((lambda r: r[0] / r[1])(ops.error_stats(x, y))))   # noqa: E731
    c, norm = ops.vq_fit(x, 16, 2, per_group=64, iters=8)
    vq = e(ops.vq_qdq(x, c, "per_group", 64, norm))
    scalar = e(ops.codebook_qdq(x, "uniform4", "per_group", 64))
    print("relative L2 error at 2 bits per weight: fitted [16, 2] table", vq, "uniform4", scalar)
    assert vq < scalar


# ---------------------------------------------------------------------------------------------------- modules
def _linear(dmx, cuda, w, **config):
    m = dmx.nn.Linear(w.shape[1], w.shape[0], bias=False).to(cuda).to(w.dtype)
    with torch.no_grad():
        m.weight.copy_(w.to(cuda))
    m.configure(dict({"weight_format": INT4}, **config))
    return m


def test_linear_with_a_vq_weight(dmx, cuda):
    ops = dmx.ops
    w = make("normal", (96, 256), seed=51, dtype=BF16)
    x = make("normal", (7, 256), seed=53, dtype=BF16).to(cuda)
    setting = {"codebook": {"grid": "uniform4", "dim": 4}, "per_group": 64}
    table = ops.vq_grid("uniform4", 4)
    m = _linear(dmx, cuda, w, weight_vq=setting)
    with torch.no_grad():
        want = F.linear(x, ops.vq_qdq(w.to(cuda), table, per_group=64))
        assert bits_equal(m(x), want) == 0
        assert bits_equal(m.weight_cast(m.weight), ops.vq_qdq(w.to(cuda), table, per_group=64)) == 0
    # autograd: the cast is a straight-through estimator, so the weight's gradient is that of a plain linear on the cast weight
    xg = x.clone().requires_grad_(True)
    out = m(xg)
    gout = make("normal", tuple(out.shape), seed=55, dtype=BF16).to(cuda)
    out.backward(gout)
    wq = ops.vq_qdq(w.to(cuda), table, per_group=64).requires_grad_(True)
    xr = x.clone().requires_grad_(True)
    F.linear(xr, wq).backward(gout)
    assert bits_equal(m.weight.grad, wq.grad) == 0 and bits_equal(xg.grad, xr.grad) == 0
    # per_token on a weight: per output channel
    t = _linear(dmx, cuda, w, weight_vq={"codebook": table, "granularity": "per_token"})
    with torch.no_grad():
        assert bits_equal(t.weight_cast(t.weight), ops.vq_qdq(w.to(cuda), table, "per_token")) == 0
    # measure_error: the error_stats row of that cast
    row = m.weight_cast.measure_error(m.weight)
    assert torch.equal(row.cpu(), ops.error_stats(w.to(cuda), ops.vq_qdq(w.to(cuda), table, per_group=64)).cpu())
    # fit, save, load into a fresh module: the same forward
    m.weight_cast.fit_vq(m.weight, iters=3)
    s = m.weight_cast.vq_setting
    assert s["norm"] == float(table.abs().max()) and s["per_group"] == 64 and s["codebook"] != table.tolist()
    with torch.no_grad():
        fitted = m(x)
        assert bits_equal(fitted, F.linear(x, ops.vq_qdq(w.to(cuda), m.weight_cast.vq_codebook, "per_group", 64, s["norm"]))) == 0
        assert bits_equal(fitted, want) > 0
    fresh = _linear(dmx, cuda, torch.zeros_like(w), weight_vq=setting)
    fresh.load_state_dict(m.state_dict())
    with torch.no_grad():
        assert bits_equal(fresh(x), fitted) == 0
    after = m.weight_cast.measure_error(m.weight)
    assert float(after[0]) < float(row[0])                                   # the fitted table has the smaller squared error
    # a SAME cast stays the identity; switching the table off returns to the format's own arithmetic
    same = dmx.nn.Linear(256, 96, bias=False).to(cuda).to(BF16)
    same.configure({"weight_vq": setting})
    with torch.no_grad():
        assert bits_equal(same(x), F.linear(x, same.weight)) == 0
    m.configure({"weight_vq": None})
    with torch.no_grad():
        assert bits_equal(m.weight_cast(m.weight), dmx.CastTo(format=INT4).to(cuda)(m.weight)) == 0


def test_activation_casts_with_a_vq_setting(dmx, cuda):
    """input_vq / output_vq: the module's plain route, equal to the op on the activations"""
    ops = dmx.ops
    w = make("normal", (96, 256), seed=61, dtype=BF16)
    x = make("normal", (7, 256), seed=63, dtype=BF16).to(cuda)
    table = rows_of("random", 16, 2)
    m = dmx.nn.Linear(256, 96, bias=False).to(cuda).to(BF16)
    with torch.no_grad():
        m.weight.copy_(w.to(cuda))
    m.configure({"input_formats": [INT4], "output_formats": [INT4], "input_vq": {"codebook": table, "granularity": "per_token"},
                 "output_vq": {"codebook": table, "per_group": 32}})
    with torch.no_grad():
        want = ops.vq_qdq(F.linear(ops.vq_qdq(x, table, "per_token"), w.to(cuda)), table, per_group=32)
        assert bits_equal(m(x), want) == 0
