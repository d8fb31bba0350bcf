"""GPU tests of the outlier-aware dynamic cast (csrc/outlier_quant.hip, ops.outlier_fixed_qdq, CastTo.set_dynamic with "outliers";
DESIGN.md §8 "Outlier-aware dynamic cast"): the kernel (fused=True) and the chain (fused=False) against the CPU checker of
tests/_outlier_ref.py, bit for bit on the output, the scales, the zero points, the outliers' positions and their values; ties, special
values, launch geometry, routing, row independence, autograd, graph capture and the module surface.
Segments whose INLIERS hold a NaN or an Inf (more of them than k) are outside the oracle's chain (tests/_dynamic_ref.py: finite inputs):
there the positions and values are still the checker's, and the cast is held to the definition's own step 2 on the device,
ops.dynamic_fixed_qdq of the segment with zeros in the outliers' places."""
import functools

import pytest
import torch

import _outlier_ref as R
from _data import bits_equal, make, mismatches_nan_aware

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=["bf16", "f16", "f32"])
GROUPS = pytest.mark.parametrize("g", [16, 32, 64, 128, 256])
INT4A = "XP[4,0](C_N)"
E5M10, E4M3 = ("FP[1|5|10,15](FN)", (10, 5, 15, True)), ("FP[1|4|3,7](_N)", (3, 4, 7, False))
V = {BF16: 8, F16: 8, F32: 4}


def fmt_of(p, qsym):
    return f"XP[{p},0](C{'S' if qsym else '_'}N)"


@pytest.fixture(autouse=True)
def _stop_the_session_after_a_gpu_fault():
    """a HIP error after a test (an illegal access is sticky) ends the session: nothing more is started on a faulted device"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # pragma: no cover
        pytest.exit(f"GPU fault, stopping the session: {e}", returncode=3)


def routes_of(ops):
    return ops._outlier_routes if hasattr(ops, "_outlier_routes") else ops._front._outlier_routes


def run(ops, x, fmt, g, k, fused, qsym=False, **kw):
    """ops.outlier_fixed_qdq with qparams and outliers, asserting on the host-side route counter which route ran"""
    before = dict(routes_of(ops))
    out = ops.outlier_fixed_qdq(x, fmt, g, k, symmetric_qscheme=qsym, fused=fused, return_qparams=True, return_outliers=True, **kw)
    took, other = ("fused", "chain") if fused else ("chain", "fused")
    assert routes_of(ops)[took] == before[took] + 1 and routes_of(ops)[other] == before[other]
    return out


def same5(got, want, what, nan_aware=False):
    (y, sc, zp, idx, val), (wy, wsc, wzp, widx, wval) = got, want
    assert y.dtype == wy.dtype and y.shape == wy.shape and sc.dtype == F32 and zp.dtype == torch.int64, what
    assert idx.dtype == torch.int32 and idx.shape == widx.shape and val.dtype == wval.dtype and val.shape == wval.shape, what
    assert torch.equal(idx.cpu(), widx), what
    assert bits_equal(val.cpu(), wval) == 0, what
    assert sc.shape == wsc.shape and bits_equal(sc.cpu(), wsc) == 0, what
    assert bits_equal(zp.cpu(), wzp) == 0, what
    assert (mismatches_nan_aware(y, wy) if nan_aware else bits_equal(y.cpu(), wy)) == 0, what


def tailed(shape, seed, dtype):
    """Student-t(3) data: a few large values per group, finite in every dtype"""
    return R.student_t3(shape, seed).clamp(-3.0e4, 3.0e4).to(dtype)


@functools.lru_cache(maxsize=None)
def _ref(oracle, shape, seed, dtype, g, k, p, qsym, ofmt=None, out_dtype=None):
    """(x, the checker's outputs): computed once per case and shared by the kernel and the chain tests"""
    x = tailed(shape, seed, dtype)
    return x, R.outlier_ref(oracle, x, p, qsym, g, k, qsym, ofmt, out_dtype)


# ---------------------------------------------------------------------------------------------------- the kernel against the checker
@GROUPS
@DTYPES
def test_kernel_matrix(dmx, oracle, cuda, dtype, g):
    """rows of 2 g .. 4 g, 3 .. 7 rows (a partly filled wave); k = 1, 2, 8; 4 and 8 bits; symmetric and affine.  g = 256 bf16 runs the
    32-lane shuffle stage, g = 256 f32 the 64-lane one, g = 16 bf16 the 2-lane group"""
    assert dmx.ops.outlier_class(g, dtype) == "group"
    n = 0
    for k in (1, 2, 8):
        if k >= g:
            continue
        for p in (4, 8):
            for qsym in (False, True):
                shape = (3 + n % 5, (2 + n % 3) * g)
                x, want = _ref(oracle, shape, 10 * g + n, dtype, g, k, p, qsym)
                same5(run(dmx.ops, x.to(cuda), fmt_of(p, qsym), g, k, True, qsym), want, ("kernel", dtype, g, k, p, qsym, shape))
                n += 1


def _tie_groups(g, dtype):
    """one group per row: the cases in which the lower-index rule decides"""
    v = V[dtype]
    rows = []
    rows.append(torch.full((g,), 2.5))                                        # all equal
    rows.append(torch.full((g,), -1.0))
    gen = torch.Generator().manual_seed(g)
    for _ in range(4):
        rows.append(torch.randint(-3, 4, (g,), generator=gen).float())         # nearly every round ties
    a = torch.zeros(g); a[3], a[g - 2] = 7.0, -7.0; rows.append(a)            # +a before -a
    a = torch.zeros(g); a[3], a[g - 2] = -7.0, 7.0; rows.append(a)            # -a before +a
    a = torch.ones(g); a[1], a[v + 1] = 5.0, 5.0; rows.append(a)              # equal maxima in two different lanes
    a = torch.ones(g); a[g - 1], a[g - v - 1] = -5.0, 5.0; rows.append(a)
    a = torch.ones(g); a[v + 2], a[v + 3] = 5.0, -5.0; rows.append(a)         # ... in two elements of one lane's vector
    a = torch.ones(g); a[0], a[v - 1] = -5.0, -5.0; rows.append(a)
    a = torch.ones(g); a[g - 1], a[0] = 5.0, 5.0; rows.append(a)              # ... in the last lane and the first lane of the group
    a = torch.ones(g); a[g - v], a[v - 1] = 5.0, -5.0; rows.append(a)
    a = torch.zeros(g); a[1::2] = -0.0; rows.append(a)                        # +0 / -0 only
    rows.append(-torch.zeros(g))
    a = torch.arange(g).float(); rows.append(a)                               # strictly rising: the last elements
    rows.append(torch.arange(g, 0, -1).float())                               # strictly falling: the first elements
    return torch.stack(rows).to(dtype)


@DTYPES
def test_kernel_ties_go_to_the_lower_index(dmx, oracle, cuda, dtype):
    ops = dmx.ops
    for g in (16, 64, 256):
        x = _tie_groups(g, dtype)
        for k, qsym in ((1, False), (2, True), (3, False), (8, False)):
            want = R.outlier_ref(oracle, x, 4, qsym, g, k, qsym)
            same5(run(ops, x.to(cuda), fmt_of(4, qsym), g, k, True, qsym), want, ("ties", dtype, g, k))
            same5(run(ops, x.to(cuda), fmt_of(4, qsym), g, k, False, qsym), want, ("ties, chain", dtype, g, k))
    # by hand: all-equal -> positions 0 .. k-1; +a / -a -> the lower index first whatever the sign
    x = _tie_groups(64, dtype).to(cuda)
    _, _, _, idx, val = run(ops, x, INT4A, 64, 3, True)
    assert idx[0].tolist() == [0, 1, 2] and idx[6].tolist()[:2] == [3, 62] and idx[7].tolist()[:2] == [3, 62]
    assert val[6].tolist()[:2] == [7.0, -7.0] and val[7].tolist()[:2] == [-7.0, 7.0]


def _special_groups(g, k, dtype):
    """rows of one group each; -> (x, the rows whose inliers are all finite)"""
    tiny = {BF16: 1.0e-40, F16: 3.0e-6, F32: 1.0e-40}[dtype]                  # subnormal in the dtype
    base = R.student_t3((64, g), 77 + g).clamp(-100, 100)
    rows, finite = [], []

    def add(r, ok=True):
        if ok:
            finite.append(len(rows))
        rows.append(r)

    for special in (float("nan"), float("inf"), -float("inf")):
        for count in (k - 1, k, k + 1):
            if count < 1:
                continue
            r = base[len(rows)].clone()
            r[torch.arange(count) * (g // (k + 1)) + 1] = special
            add(r, count <= k)
    r = base[len(rows)].clone(); r[2], r[g - 3], r[5] = float("nan"), float("inf"), -float("inf"); add(r, k >= 3)   # one of each
    add(torch.zeros(g))                                                       # an all-zero group
    r = torch.zeros(g); r[g // 2] = -3.0; add(r)                              # zeros and one value
    add(base[len(rows)] * 0 + tiny * torch.arange(1, g + 1))                  # subnormals only
    r = base[len(rows)].clone() * tiny; r[g - 1] = 1.0; add(r)                # subnormals and one large value
    r = base[len(rows)].clone().clamp(-1, 1); r[:k] = 50.0 + torch.arange(k); add(r)          # the outliers are the first k elements
    r = base[len(rows)].clone().clamp(-1, 1); r[g - k:] = -50.0 - torch.arange(k); add(r)     # ... the last k
    return torch.stack(rows).to(dtype), finite


@DTYPES
def test_kernel_special_values(dmx, oracle, cuda, dtype):
    ops = dmx.ops
    for g, k in ((16, 1), (64, 2), (128, 3), (256, 8)):
        x, finite = _special_groups(g, k, dtype)
        other = [i for i in range(x.shape[0]) if i not in finite]
        wy, wsc, wzp, widx, wval = R.outlier_ref(oracle, x[finite], 4, False, g, k, False)
        for fused in (True, False):
            y, sc, zp, idx, val = run(ops, x.to(cuda), INT4A, g, k, fused)
            what = ("specials", dtype, g, k, fused)
            same5((y[finite], sc[finite], zp[finite], idx[finite], val[finite]), (wy, wsc, wzp, widx, wval), what, nan_aware=True)
            assert bool(torch.isfinite(sc[finite]).all()), what
            # every outlier, in every row, comes back with its own bits
            assert torch.equal(idx.cpu(), R.rank(x, k).to(torch.int32)), what
            assert bits_equal(val.cpu(), x.gather(1, idx.cpu().long())) == 0 and bits_equal(y.gather(1, idx.long()).cpu(), val.cpu()) == 0, what
            # more NaN / Inf than k: the definition's step 2 on the device
            mask = torch.zeros(x.shape, dtype=torch.bool).scatter_(1, idx.cpu().long(), True)
            xin = torch.where(mask, torch.zeros((), dtype=dtype), x)[other].to(cuda)
            dy, dsc, dzp = ops.dynamic_fixed_qdq(xin, INT4A, "per_token", return_qparams=True)
            assert bits_equal(sc[other], dsc) == 0 and bits_equal(zp[other], dzp) == 0, what
            keep = ~mask[other].to(cuda)
            assert mismatches_nan_aware(torch.where(keep, y[other], 0), torch.where(keep, dy, 0)) == 0, what


def test_kernel_one_group_and_several_workgroups(dmx, oracle, cuda):
    ops = dmx.ops
    for dtype, g, k in ((BF16, 16, 1), (F32, 256, 8), (F16, 64, 2)):
        x, want = _ref(oracle, (1, g), 5, dtype, g, k, 4, False)
        same5(run(ops, x.to(cuda), INT4A, g, k, True), want, ("one group", dtype, g))
    # [1031, 512]: an odd count of rows over several workgroups, the last wave partly past the end
    for dtype, g, k in ((BF16, 128, 2), (F32, 32, 4), (F16, 256, 1)):
        x, want = _ref(oracle, (1031, 512), 200 + g, dtype, g, k, 4, False)
        same5(run(ops, x.to(cuda), INT4A, g, k, True), want, ("several workgroups", dtype, g))


def test_kernel_grid_rounds(dmx, oracle, cuda):
    """more waves than the grid holds (6 workgroups per compute unit: 6144 waves on 256 units): [8259, 256] f32 is 8259 waves of vectors,
    [16515, 256] bf16 8258, so the first waves take a second round of the grid-stride loop and the last one is partly filled"""
    for shape, dtype, g, k in (((8259, 256), F32, 64, 2), ((16515, 256), BF16, 128, 3)):
        x, want = _ref(oracle, shape, 7, dtype, g, k, 4, False)
        same5(run(dmx.ops, x.to(cuda), INT4A, g, k, True), want, ("grid rounds", shape, dtype))


def test_kernel_past_two_to_the_31_elements(dmx, oracle, cuda):
    """[2^23 + 64, 256] bf16: byte offsets, vector and group indices past 2^31; spot groups (the first, those around element 2^31, the
    last) against the checker"""
    rows, L, g, k = (1 << 23) + 64, 256, 128, 2
    n = rows * L
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    need = 2 * n * 2 + (n // g) * k * 6 + (1 << 30)
    if free < need:
        pytest.skip(f"needs {need / 2 ** 30:.1f} GiB of device memory, {free / 2 ** 30:.1f} GiB free")
    x = torch.empty(rows, L, dtype=BF16, device=cuda)
    gen = torch.Generator(device=cuda).manual_seed(31)
    for r0 in range(0, rows, 1 << 20):
        x[r0:r0 + (1 << 20)].normal_(generator=gen)
    x[-1, -3] = 300.0
    x[1 << 23, 1] = -200.0                                                    # element 2^31 + 1
    y, sc, zp, idx, val = run(dmx.ops, x, INT4A, g, k, True)
    G = L // g
    for r0, r1 in ((0, 4), ((1 << 23) - 4, (1 << 23) + 4), (rows - 4, rows)):
        wy, wsc, wzp, widx, wval = R.outlier_ref(oracle, x[r0:r1].cpu(), 4, False, g, k, False)
        got = (y[r0:r1], sc[r0 * G:r1 * G], zp[r0 * G:r1 * G], idx[r0 * G:r1 * G], val[r0 * G:r1 * G])
        same5(got, (wy, wsc, wzp, widx, wval), ("past 2^31", r0))
    assert idx[-1].tolist()[0] == g - 3 and float(val[-1, 0]) == 300.0 and idx[(1 << 23) * G].tolist()[0] == 1
    del x, y, sc, zp, idx, val
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_outlier_format(dmx, oracle, cuda, dtype):
    """O(x) = the value itself, or the per-element float cast of it: FP16 (subnormals flushed) on both dtypes, E4M3 on one case"""
    ops = dmx.ops
    cases = [(None, None), E5M10] + ([E4M3] if dtype == F32 else [])
    for name, fields in cases:
        for g, k in ((32, 2), (128, 8)):
            x = tailed((5, 3 * g), 300 + g, dtype)
            x[0, 0] = 7.0e4                                                  # above FP16's largest value: saturates
            x[3], x[4] = x[3] * 1.0e-6, x[4] * 1.0e-9                         # outliers inside and below FP16's subnormals: flushed
            want = R.outlier_ref(oracle, x, 4, False, g, k, False, fields)
            for fused in (True, False):
                same5(run(ops, x.to(cuda), INT4A, g, k, fused, outlier_format=name), want, ("outlier_format", dtype, name, g, k, fused))
    if dtype == F32:   # the formats the kernel leaves to the chain: another rounding, an unsigned format
        x = tailed((5, 96), 9, F32).to(cuda)
        for name in ("FP[1|4|3,7](_U)", "FP[0|4|3,7](_N)"):
            with pytest.raises(NotImplementedError):
                ops.outlier_fixed_qdq(x, INT4A, 32, 2, outlier_format=name, fused=True)
            y = ops.outlier_fixed_qdq(x, INT4A, 32, 2, outlier_format=name)
            assert y.shape == x.shape and bool(torch.isfinite(y).all())


# ---------------------------------------------------------------------------------------------------- the chain against the checker
@DTYPES
def test_chain_matches_the_checker(dmx, oracle, cuda, dtype):
    for g, k, p, qsym, shape in ((64, 2, 4, False, (5, 192)), (16, 1, 8, True, (3, 48)), (256, 8, 4, False, (7, 512)), (128, 4, 4, True, (1031, 512))):
        x, want = _ref(oracle, shape, 400 + g, dtype, g, k, p, qsym)
        same5(run(dmx.ops, x.to(cuda), fmt_of(p, qsym), g, k, False, qsym), want, ("chain", dtype, g, k))


def test_chain_takes_what_the_kernel_refuses(dmx, oracle, cuda):
    ops = dmx.ops
    before = dict(routes_of(ops))

    def refused(x, g, k, **kw):
        with pytest.raises(NotImplementedError):
            ops.outlier_fixed_qdq(x, INT4A, g, k, fused=True, **kw)

    # g = 48: no power of two
    for dtype in (BF16, F32):
        x, want = _ref(oracle, (5, 192), 31, dtype, 48, 3, 4, False)
        refused(x.to(cuda), 48, 3)
        same5(run(ops, x.to(cuda), INT4A, 48, 3, False), want, ("g48", dtype))
        same5(run(ops, x.to(cuda), INT4A, 48, 3, None), want, ("g48 default route", dtype))
    # per_token rows of 200
    x, want = _ref(oracle, (6, 200), 33, BF16, 200, 5, 8, False)
    refused(x.to(cuda), None, 5, granularity="per_token")
    same5(run(ops, x.to(cuda), fmt_of(8, False), None, 5, None, granularity="per_token"), want, "per_token 200")
    # k = 12: more rounds than the kernel runs
    x, want = _ref(oracle, (4, 128), 35, F16, 64, 12, 4, True)
    refused(x.to(cuda), 64, 12)
    same5(run(ops, x.to(cuda), fmt_of(4, True), 64, 12, None, True), want, "k = 12")
    # out_dtype != x.dtype: one rounding of the float32 result, the outliers through .to(out_dtype)
    for dtype, out in ((BF16, F32), (F32, BF16), (F16, F32)):   # (ops.fixed_qdq, the chain's last step, takes no f16 -> bf16)
        x, want = _ref(oracle, (9, 128), 37, dtype, 32, 2, 8, False, None, out)
        refused(x.to(cuda), 32, 2, out_dtype=out)
        same5(run(ops, x.to(cuda), fmt_of(8, False), 32, 2, None, out_dtype=out), want, ("out_dtype", dtype, out))
    # an unaligned view (2 bytes past a 16-byte boundary)
    x, want = _ref(oracle, (9, 128), 39, BF16, 64, 2, 4, False)
    view = torch.zeros(x.numel() + 8, dtype=BF16, device=cuda)[1:1 + x.numel()].reshape(x.shape)
    view.copy_(x.to(cuda))
    assert view.data_ptr() % 16 == 2 and view.is_contiguous()
    refused(view, 64, 2)
    same5(run(ops, view, INT4A, 64, 2, None), want, "unaligned")
    assert routes_of(ops)["fused"] == before["fused"]                          # no refused call ran the kernel


# ---------------------------------------------------------------------------------------------------- further properties
def test_routing_and_returns(dmx, cuda):
    ops = dmx.ops
    x = tailed((8, 1536), 51, BF16).to(cuda)
    before = dict(routes_of(ops))
    y = ops.outlier_fixed_qdq(x, INT4A, 64, 2)                                # fused=None where the kernel applies: the kernel
    assert routes_of(ops)["fused"] == before["fused"] + 1 and routes_of(ops)["chain"] == before["chain"]
    assert ops.outlier_class(64, BF16) not in ops.OUTLIER_CHAIN_BY_DEFAULT
    assert isinstance(y, torch.Tensor) and y.dtype == BF16 and y.shape == x.shape
    y2, sc, zp = ops.outlier_fixed_qdq(x, INT4A, 64, 2, return_qparams=True)
    assert bits_equal(y2, y) == 0 and sc.shape == zp.shape == (x.numel() // 64,) and zp.dtype == torch.int64
    y3, idx, val = ops.outlier_fixed_qdq(x, INT4A, 64, 2, return_outliers=True)
    assert bits_equal(y3, y) == 0 and idx.shape == val.shape == (x.numel() // 64, 2) and idx.dtype == torch.int32 and val.dtype == BF16
    e = ops.outlier_fixed_qdq(x[:0], INT4A, 64, 2, return_qparams=True, return_outliers=True)   # an empty tensor: nothing launched
    assert [t.numel() for t in e] == [0, 0, 0, 0, 0]


def test_both_bindings_the_entry_and_its_meta_kernel(dmx, oracle, cuda):
    for dtype, g, k, ofmt in ((BF16, 64, 2, (None, None)), (F32, 128, 3, E5M10), (F16, 16, 1, (None, None))):
        x = tailed((9, 384), 57, dtype)
        want = R.outlier_ref(oracle, x, 4, False, g, k, False, ofmt[1])
        for binding in ("ctypes", "torch"):
            f = dmx.ops.front(binding)
            same5(run(f, x.to(cuda), INT4A, g, k, True, outlier_format=ofmt[0]), want, (binding, dtype, g, k))
            same5(run(f, x.to(cuda), INT4A, g, k, False, outlier_format=ofmt[0]), want, (binding, "chain", dtype, g, k))
            y = f.outlier_fixed_qdq(x.to(cuda), INT4A, g, k, outlier_format=ofmt[0], fused=True)   # without the four outputs
            assert bits_equal(y.cpu(), want[0]) == 0
    # the C entry itself answers DMXQ_ERR_UNSUPPORTED (NotImplementedError through either binding), nothing launched
    xd = tailed((9, 384), 59, BF16).to(cuda)
    for binding in ("ctypes", "torch"):
        raw = dmx.ops.front(binding)._ops
        for seg, k, frac, rnd, ofmt in ((48, 2, 0, 2, []), (64, 0, 0, 2, []), (64, 9, 0, 2, []), (64, 2, 1, 2, []), (64, 2, 0, 3, []),
                                       (64, 2, 0, 2, [23, 8, 127, 0])):
            with pytest.raises(NotImplementedError):
                raw.outlier_fixed_qdq(xd, seg, k, 4, frac, True, False, rnd, -8, 7, False, ofmt, True, True, None)
    # the dispatcher op and its meta kernel
    out = torch.ops.dmxq.outlier_fixed_qdq(xd, 64, 2, 4, 0, True, False, 2, -8, 7, False, [], True, True, None)
    meta = torch.ops.dmxq.outlier_fixed_qdq(xd.to("meta"), 64, 2, 4, 0, True, False, 2, -8, 7, False, [], True, True, None)
    assert all(m.device.type == "meta" and m.shape == o.shape and m.dtype == o.dtype for m, o in zip(meta, out))
    assert [tuple(t.shape) for t in out] == [(9, 384), (54,), (54,), (54, 2), (54, 2)]
    meta = torch.ops.dmxq.outlier_fixed_qdq(xd.to("meta"), 64, 2, 4, 0, True, False, 2, -8, 7, False, [], False, False, None)
    assert [t.numel() for t in meta[1:]] == [0, 0, 0, 0]


@pytest.mark.parametrize("fused", [True, False, None])
def test_k0_is_the_dynamic_cast(dmx, cuda, fused):
    ops = dmx.ops
    for dtype, g in ((BF16, 64), (F32, 128), (F16, 48)):
        x = tailed((9, 384), 55, dtype).to(cuda)
        if g == 48 and fused:
            continue
        y, sc, zp, idx, val = ops.outlier_fixed_qdq(x, INT4A, g, 0, fused=fused, return_qparams=True, return_outliers=True)
        dy, dsc, dzp = ops.dynamic_fixed_qdq(x, INT4A, "per_group", g, fused=fused, return_qparams=True)
        assert bits_equal(y, dy) == 0 and bits_equal(sc, dsc) == 0 and bits_equal(zp, dzp) == 0
        assert idx.shape == val.shape == (x.numel() // g, 0)


@pytest.mark.parametrize("fused", [True, False])
def test_rows_are_independent(dmx, cuda, fused):
    ops = dmx.ops
    x = tailed((37, 384), 61, BF16).to(cuda)
    y, sc, zp, idx, val = run(ops, x, INT4A, 128, 2, fused)
    for r in (1, 5, 36):
        yr, scr, zpr, idxr, valr = run(ops, x[:r], INT4A, 128, 2, fused)
        G = r * 3
        assert bits_equal(yr, y[:r]) == 0 and bits_equal(scr, sc[:G]) == 0 and bits_equal(zpr, zp[:G]) == 0
        assert torch.equal(idxr, idx[:G]) and bits_equal(valr, val[:G]) == 0


@pytest.mark.parametrize("fused", [True, False])
def test_autograd_is_straight_through(dmx, cuda, fused):
    ops = dmx.ops
    x = tailed((8, 256), 63, BF16).to(cuda).requires_grad_(True)
    gout = make("normal", (8, 256), seed=65, dtype=BF16).to(cuda)
    y, sc, zp, idx, val = ops.outlier_fixed_qdq(x, INT4A, 64, 2, fused=fused, return_qparams=True, return_outliers=True)
    assert y.requires_grad and not sc.requires_grad and not val.requires_grad
    y.backward(gout)
    assert bits_equal(x.grad, gout) == 0


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


def test_graph_capture(dmx, oracle, cuda):
    """one capture of a call (a single stream, no parallel branches), replayed on new data, gives the eager bits: no host round trip"""
    ops = dmx.ops
    x0, want0 = _ref(oracle, (67, 256), 164, BF16, 64, 2, 4, False)
    x1, want1 = _ref(oracle, (67, 256), 165, BF16, 64, 2, 4, False)
    buf = x0.to(cuda).clone()
    graph, out = _capture(lambda: run(ops, buf, INT4A, 64, 2, True))
    for x, want in ((x1, want1), (x0, want0)):
        buf.copy_(x.to(cuda))
        graph.replay()
        torch.cuda.synchronize()
        same5(out, want, "replay")
        same5(out, tuple(t.cpu() for t in run(ops, x.to(cuda), INT4A, 64, 2, True)), "replay against eager")


# ---------------------------------------------------------------------------------------------------- modules
def _linear(dmx, cuda, dtype=BF16, **config):
    m = dmx.nn.Linear(128, 64, bias=True).to(cuda).to(dtype)
    with torch.no_grad():
        m.weight.copy_((R.student_t3((64, 128), 71) * 0.1).to(dtype).to(cuda))
    m.configure(dict({"weight_format": INT4A}, **config))
    return m


def test_module_forward_is_the_hand_built_chain(dmx, cuda):
    ops = dmx.ops
    setting = {"per_group": 64, "outliers": 2}
    m = _linear(dmx, cuda, weight_dynamic=setting, input_formats=["XP[8,0](C_N)"], input_dynamic=setting)
    assert m.weight_cast.dynamic == setting and m.input_casts.input_cast.dynamic == setting
    assert "'outliers': 2" in repr(m.weight_cast) and "'outliers': 2" in repr(m)
    x = tailed((5, 128), 73, BF16).to(cuda)
    before = dict(routes_of(ops))
    with torch.no_grad():
        y = m(x)
        assert routes_of(ops)["fused"] >= before["fused"] + 2 and routes_of(ops)["chain"] == before["chain"]   # both casts took the kernel
        wq = ops.outlier_fixed_qdq(m.weight.detach(), INT4A, 64, 2)
        xq = ops.outlier_fixed_qdq(x, "XP[8,0](C_N)", 64, 2)
        want = torch.nn.functional.linear(xq, wq, m.bias)
        plain = _linear(dmx, cuda, weight_dynamic={"per_group": 64}, input_formats=["XP[8,0](C_N)"], input_dynamic={"per_group": 64})(x)
    assert bits_equal(y, want) == 0 and bits_equal(y, plain) > 0
    assert bits_equal(wq, ops.dynamic_fixed_qdq(m.weight.detach(), INT4A, "per_group", 64)) > 0
    # an outlier format and per-token rows through the module
    m = _linear(dmx, cuda, weight_dynamic={"granularity": "per_token", "outliers": 3, "outlier_format": E5M10[0]})
    with torch.no_grad():
        y = m(x)
        wq = ops.outlier_fixed_qdq(m.weight.detach(), INT4A, None, 3, outlier_format=E5M10[0], granularity="per_token")
        assert bits_equal(y, torch.nn.functional.linear(x, wq, m.bias)) == 0


def test_module_gptq_awq_and_hqq_refuse(dmx, cuda):
    m = _linear(dmx, cuda, weight_dynamic={"per_group": 64, "outliers": 2})
    w0 = m.weight.detach().clone()
    x = tailed((5, 128), 75, BF16).to(cuda)
    with pytest.raises(NotImplementedError, match="outlier"):
        with torch.no_grad(), m.optimal_brain_compressing(dmx.DmxModuleGPTQHyperparams(microblock_size=64, block_size=64)):
            m(x)
    with pytest.raises(NotImplementedError, match="outlier"):
        with torch.no_grad(), m.awq_scaling(dmx.DmxAWQHyperparams()):
            m(x)
    with pytest.raises(NotImplementedError, match="outlier"):
        m.hqq_quantize()
    assert m.obc is None and m.awq is None and not hasattr(m, "hqq_qparams")
    assert bits_equal(m.weight.detach(), w0) == 0 and m.weight_cast._flag("fake_quant_enabled")
    with torch.no_grad():                                                     # the eager forward works as ever
        assert m(x).shape == (5, 64)
