"""The BFP matmul kernels (csrc/bfp_matmul.hip, csrc/bfp_bmm.hip) and the column pack (bfp_pack_cols_kernel, csrc/bfp_pack.hip) on the
case table of tests/_bfp_mm_cases.py, which tests/test_bfp_mm_cases_host.py proves to reach every accumulator slot, edge, block count,
store path, output dtype and precision pair of all 15 classes:

  float64 bound    packed make("heavy") operands: the kernel within the bound of nb - 1 ordered fp32 adds, and == the chain bit for bit
  exact integer    hand-built codes over the full range under one exponent byte: every result an exact fp32, zero tolerance
  exponent range   hand-built bytes from 1 to 254: denormal scales, denormal and vanishing terms, both overflows, Inf - Inf, and the
                   one element on which the fma and multiply-then-add part -- each route against its own exact semantics
                   (tests/_bfp_mm_ref.py), which pins the one documented difference between the routes
  batch pieces, non-contiguous views, the column pack on every input dtype and precision, and every offset past 2^31."""
import functools
from fractions import Fraction

import pytest
import torch

import _bfp_mm_cases as MC
import _bfp_mm_ref as R
import _large_cases as LC
from _data import make, mismatches_nan_aware

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
ALL_SLOTS = [c for c in MC.CASES if c.all_slots]


def _run(ops, op, layout, A, W, pa, pw, B, out=torch.float32, fused=None):
    if op == "mm":
        return ops.bfp_matmul_packed(*A, *W, pa, pw, B, out_dtype=out, fused=fused)
    return ops.bfp_bmm_packed(*A, *W, pa, pw, B, layout, out_dtype=out, fused=fused)


def _class(ops, op, layout, A, W, B):
    return ops.bfp_matmul_class(A[0], W[0], B) if op == "mm" else ops.bfp_bmm_class(A[0], W[0], B, layout)


def _routes(dmx, op):
    return dmx._front._bfp_matmul_routes if op == "mm" else dmx._front._bfp_bmm_routes


# ------------------------------------------------------------------------------------------------ float64 bound
@pytest.mark.parametrize("c,out", [(c, o) for c in MC.CASES for o in c.outs], ids=lambda v: v if isinstance(v, str) else MC.case_id(v))
def test_kernel_within_the_float64_bound_and_equal_to_the_chain(dmx, cuda, c, out):
    ops, kn, K = dmx.ops, c.layout == "kn", c.nb * c.B
    lead = (c.batch,) if c.op == "bmm" else ()
    x = make("normal" if out == "f16" else "heavy", lead + (c.M, K), seed=c.M + K).to(cuda)     # (float16 holds no 2^17 spread)
    w = make("normal", lead + ((K, c.N) if kn else (c.N, K)), seed=c.N + K + 1).to(cuda)
    A, W = ops.bfp_pack(x, c.pa, c.B, True), ops.bfp_pack(w, c.pw, c.B, True, block_dim=-2 if kn else -1)
    assert _class(ops, c.op, c.layout, A, W, c.B) == c.cls
    before = dict(_routes(dmx, c.op))
    y = _run(ops, c.op, c.layout, A, W, c.pa, c.pw, c.B, DT[out], fused=True)
    assert _routes(dmx, c.op)["fused"] == before["fused"] + 1 and _routes(dmx, c.op)["chain"] == before["chain"]
    if c.op == "mm":
        ref, bound = R.ref_and_bound_mm(ops, A, W, c.pa, c.pw, c.B, DT[out])
    else:
        ref, bound = R.ref_and_bound_bmm(ops, A, W, c.layout, c.pa, c.pw, c.B, DT[out])
    err = (y.cpu().double() - ref).abs()
    print(f"{MC.case_id(c)} {out}: max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert y.shape == lead + (c.M, c.N) and y.dtype == DT[out] and bool((err <= bound).all())
    assert mismatches_nan_aware(y, _run(ops, c.op, c.layout, A, W, c.pa, c.pw, c.B, DT[out], fused=False)) == 0


# ------------------------------------------------------------------------------------------------ exact integer
@pytest.mark.parametrize("pa,pw", ((8, 8), (3, 5), (2, 8)))
@pytest.mark.parametrize("c", ALL_SLOTS, ids=MC.case_id)
def test_exact_integer_products_on_every_slot(dmx, cuda, c, pa, pw):
    """all exponent bytes of a call equal, so y = 2^s sum_j P_j with |sum_j P_j| <= nb B 2^(pa + pw - 2) <= 2^22: every partial sum is an
    exact fp32 and no rounding happens anywhere.  Rows and columns of nothing but -2^(p-1) and 2^(p-1) - 1 are planted."""
    ops, kn, K, nbat = dmx.ops, c.layout == "kn", c.nb * c.B, max(c.batch, 1)
    (lo_a, _), (lo_w, hi_w) = R.code_range(pa), R.code_range(pw)
    ca, cw = MC.int8_codes((nbat, c.M, K), pa, 5 + c.B + pa), MC.int8_codes((nbat, c.N, K), pw, 6 + c.B + pw)
    ca[:, 1], ca[:, c.M - 1] = lo_a, lo_a
    cw[:, 1], cw[:, 2], cw[:, c.N - 1] = lo_w, hi_w, lo_w
    byte_a, byte_w = 127, 130
    s = (byte_a - 127 - (pa - 2)) + (byte_w - 127 - (pw - 2))
    total = ca.to(torch.int64) @ cw.to(torch.int64).transpose(-1, -2)                     # int64 on the CPU: sum_j P_j
    assert int(total[0, 1, 1]) == K * lo_a * lo_w == c.nb * c.B << (pa + pw - 2) and int(total[0, 1, 2]) == K * lo_a * hi_w
    assert int(total.abs().max()) <= 1 << 24
    want = (total.double() * 2.0 ** s).to(torch.float32)
    assert torch.equal(want.double(), total.double() * 2.0 ** s)
    ea = torch.full((nbat, c.M, c.nb), byte_a, dtype=torch.uint8)
    ew = torch.full((nbat, c.N, c.nb), byte_w, dtype=torch.uint8)
    if kn:
        cw, ew = cw.transpose(-1, -2).contiguous(), ew.transpose(-1, -2).contiguous()
    A, W = (ca.to(cuda), ea.to(cuda)), (cw.to(cuda), ew.to(cuda))
    if c.op == "mm":
        A, W, want = tuple(t[0] for t in A), tuple(t[0] for t in W), want[0]
    assert _class(ops, c.op, c.layout, A, W, c.B) == c.cls
    y = _run(ops, c.op, c.layout, A, W, pa, pw, c.B, fused=True)
    assert y.dtype == torch.float32 and torch.equal(y.cpu(), want)
    assert torch.equal(_run(ops, c.op, c.layout, A, W, pa, pw, c.B, fused=False).cpu(), want)


# ------------------------------------------------------------------------------------------------ exponent range
@functools.lru_cache(maxsize=None)
def _semantics(B, out, which):
    fn = R.kernel_semantics if which == "kernel" else R.chain_semantics
    return fn(*MC.exponent_range_operands(B), 8, 8, B, DT[out])


@pytest.mark.parametrize("out", ("f32", "f16"))
@pytest.mark.parametrize("cls", MC.CLASSES)
def test_exponent_range_against_each_route_s_exact_semantics(dmx, cuda, cls, out):
    """one small tile per class.  The 128-wide batched classes take the 8 columns nine times over (N = 72); a batched call holds the
    operands and, as its second element, the same with A's rows reversed."""
    ops = dmx.ops
    c = next(k for k in MC.CASES if k.cls == cls)
    B, kn = c.B, c.layout == "kn"
    ca, ea, cw, ew = MC.exponent_range_operands(B)
    reps = 9 if cls.endswith("_n128") else 1
    cw, ew = cw.repeat(reps, 1), ew.repeat(reps, 1)
    want = {w: _semantics(B, out, w).repeat(1, reps) for w in ("kernel", "chain")}
    if c.op == "bmm":
        ca, ea = torch.stack([ca, ca.flip(0)]), torch.stack([ea, ea.flip(0)])
        cw, ew = torch.stack([cw, cw]), torch.stack([ew, ew])
        want = {k: torch.stack([v, v.flip(0)]) for k, v in want.items()}
        if kn:
            cw, ew = cw.transpose(-1, -2).contiguous(), ew.transpose(-1, -2).contiguous()
    A, W = (ca.to(cuda), ea.to(cuda)), (cw.to(cuda), ew.to(cuda))
    assert _class(ops, c.op, c.layout, A, W, B) == cls
    y = _run(ops, c.op, c.layout, A, W, 8, 8, B, DT[out], fused=True)
    z = _run(ops, c.op, c.layout, A, W, 8, 8, B, DT[out], fused=False)
    assert y.dtype == DT[out] and mismatches_nan_aware(y, want["kernel"]) == 0
    assert mismatches_nan_aware(z, want["chain"]) == 0
    y0, z0 = (t.cpu()[0] if c.op == "bmm" else t.cpu() for t in (y, z))
    rows, cols = MC.EXP_NORMAL
    assert mismatches_nan_aware(y0[rows.start:rows.stop, cols.start:cols.stop], z0[rows.start:rows.stop, cols.start:cols.stop]) == 0
    if out == "f32":   # denormal scales, normal terms: also inside the bound of the exact sum
        t = R.exact_terms(*MC.exponent_range_operands(B), 8, 8, B)
        for m in rows:
            for n in cols:
                bound = (MC.EXP_NB - 1) * Fraction(1, 1 << 24) * sum(abs(v) for v in t[m][n]) * (1 + Fraction(1, 1 << 20))
                assert abs(Fraction(float(y0[m, n])) - sum(t[m][n])) <= bound
        # the planted element on which the routes part, and the ones on which they may not
        assert float(y0[MC.EXP_CANCELLED]) == 2.0 ** 127 and float(z0[MC.EXP_CANCELLED]) == float("inf")
        assert float(y0[MC.EXP_POS_INF]) == float("inf") == -float(y0[MC.EXP_NEG_INF]) and bool(torch.isnan(y0[MC.EXP_INF_NAN]))
        assert float(y0[MC.EXP_SECOND_OVERFLOW]) == float("inf") == float(z0[MC.EXP_SECOND_OVERFLOW])


# ------------------------------------------------------------------------------------------------ batch pieces
@pytest.mark.parametrize("layout", MC.LAYOUTS)
def test_batch_beyond_one_grid_runs_in_pieces(dmx, cuda, layout):
    ops, kn = dmx.ops, layout == "kn"
    batch, M, N, K, B = 65540, 1, 4, 32, 32
    assert batch > ops.BFP_BMM_MAX_BATCH
    ca, cw = MC.int8_codes((batch, M, K), 8, 21).to(cuda), MC.int8_codes((batch, K, N) if kn else (batch, N, K), 8, 22).to(cuda)
    ea = MC.bytes_between((batch, M, 1), 110, 140, 23).to(cuda)
    ew = MC.bytes_between((batch, 1, N) if kn else (batch, N, 1), 110, 140, 24).to(cuda)
    assert ops.bfp_bmm_class(ca, cw, B, layout) == f"{layout}_b32_n64"
    before = dict(dmx._front._bfp_bmm_routes)
    y = ops.bfp_bmm_packed(ca, ea, cw, ew, 8, 8, B, layout)
    assert dmx._front._bfp_bmm_routes == dict(before, fused=before["fused"] + 1)
    ref, bound = R.ref_and_bound_bmm(ops, (ca, ea), (cw, ew), layout, 8, 8, B)
    assert y.shape == (batch, M, N) and bool(((y.cpu().double() - ref).abs() <= bound).all())
    parts = [ops.bfp_bmm_packed(ca[a:b], ea[a:b], cw[a:b], ew[a:b], 8, 8, B, layout, fused=True) for a, b in ((0, 40000), (40000, batch))]
    assert torch.equal(y, torch.cat(parts))


# ------------------------------------------------------------------------------------------------ views
@pytest.mark.parametrize("op,layout", (("mm", None), ("bmm", "nk"), ("bmm", "kn")))
def test_non_contiguous_views_give_the_bits_of_their_copies(dmx, cuda, op, layout):
    """codes as a column slice of a wider tensor, exponents as a transposed view: both routes read them as their contiguous copies"""
    ops, kn, B = dmx.ops, layout == "kn", 64
    M, N, K = 33, 36, 2 * B
    lead = (2,) if op == "bmm" else ()
    wide_a = MC.int8_codes(lead + (M, K + 48), 8, 31).to(cuda)
    ws = (K, N) if kn else (N, K)
    wide_w = MC.int8_codes(lead + (ws[0], ws[1] + 48), 8, 32).to(cuda)
    ca, cw = wide_a[..., 16:16 + K], wide_w[..., 16:16 + ws[1]]
    ea = MC.bytes_between(lead + (2, M), 110, 140, 33).to(cuda).transpose(-1, -2)
    ew = MC.bytes_between(lead + ((N, 2) if kn else (2, N)), 110, 140, 34).to(cuda).transpose(-1, -2)
    assert not any(t.is_contiguous() for t in (ca, cw, ea, ew))
    copies = tuple(t.contiguous() for t in (ca, ea, cw, ew))
    for fused in (True, False):
        got = _run(ops, op, layout, (ca, ea), (cw, ew), 8, 8, B, fused=fused)
        assert mismatches_nan_aware(got, _run(ops, op, layout, copies[:2], copies[2:], 8, 8, B, fused=fused)) == 0
    ref, bound = (R.ref_and_bound_mm(ops, copies[:2], copies[2:], 8, 8, B) if op == "mm" else
                  R.ref_and_bound_bmm(ops, copies[:2], copies[2:], layout, 8, 8, B))
    assert bool(((got.cpu().double() - ref).abs() <= bound).all())


# ------------------------------------------------------------------------------------------------ the column pack
@pytest.mark.parametrize("B", MC.BLOCKS)
@pytest.mark.parametrize("dtype", (torch.float16, torch.bfloat16, torch.float32))
def test_column_pack_on_every_input_dtype_and_precision(dmx, cuda, dtype, B):
    ops, routes = dmx.ops, dmx._front._bfp_pack_cols_routes
    den = 6e-8 if dtype == torch.float16 else 1e-40
    den_byte = 103 if dtype == torch.float16 else 0                  # (float16's smallest denormal is 2^-24, a normal float32)
    low = -1.9921875 if dtype == torch.bfloat16 else -1.999          # (-1.999 is -2 in bfloat16)
    for shape in ((5, 2 * B, 40), (2, 3, B, 16)):
        x = make("heavy", shape, seed=B + len(shape), dtype=dtype).to(cuda)
        x[..., :B, 1] = 0.0                                  # an all-zero block
        x[..., :B, 3] = den                                  # a block whose maximum is a denormal
        x[..., 1, 5] = torch.finfo(dtype).max                # a maximum at the largest finite value
        x[..., 2, 7] = float("inf")
        x[..., B - 1, 9] = float("nan")
        x[..., :B, 11] = 0.25
        x[..., 0, 11] = low                                  # rounds to -2^(p-1) quanta, a code only the asymmetric format has
        xt = x.transpose(-1, -2).contiguous()
        for p in (2, 4, 5, 8):
            for symmetric in (True, False):
                before = dict(routes)
                c, e = ops.bfp_pack(x, p, B, symmetric, block_dim=-2)
                assert routes == dict(before, fused=before["fused"] + 1)
                wc, we = ops.bfp_pack(xt, p, B, symmetric)
                assert c.shape == x.shape and e.shape == shape[:-2] + (shape[-2] // B, shape[-1]) and c.is_contiguous() and e.is_contiguous()
                assert torch.equal(c, wc.transpose(-1, -2)) and torch.equal(e, we.transpose(-1, -2)), (shape, p, symmetric)
                assert int(e[..., 0, 1].max()) == 0 and int(e[..., 0, 3].max()) == den_byte and int(e[..., 0, 7].min()) == 255
                assert int(e[..., 0, 9].min()) == 255 and int(e[..., 0, 5].min()) == int(e[..., 0, 5].max()) in (142, 254)
                assert int(c.min()) >= -(1 << (p - 1)) + symmetric and int(c.max()) <= (1 << (p - 1)) - 1
                if not symmetric and not (p == 8 and dtype == torch.bfloat16):   # (bfloat16 at p = 8: -127.5 quanta, a tie)
                    assert int(c[..., 0, 11].max()) == -(1 << (p - 1))
                back = ops.bfp_unpack(c.transpose(-1, -2).contiguous(), e.transpose(-1, -2).contiguous(), p, B, dtype)
                qdq = ops.bfp_qdq(xt, p, B, symmetric=symmetric)
                if den_byte == 0:   # include/dmxq.h: a denormal maximum packs to zeros; unpack == qdq holds for normal finite maxima
                    assert int(back[..., 3, :B].count_nonzero()) == 0
                    back[..., 3, :B] = qdq[..., 3, :B]
                assert mismatches_nan_aware(back, qdq) == 0, (shape, p, symmetric)


# ------------------------------------------------------------------------------------------------ offsets past 2^31
def _need(c):
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    need = MC.large_peak_bytes(c)
    if free < need:
        pytest.skip(f"{c.name}: needs {need / MC.GIB:.1f} GiB of device memory, {free / MC.GIB:.1f} GiB free")


def _device_ints(shape, lo, hi, dtype, g, dev, piece=1 << 27):
    """uniform integers in lo .. hi without a period, generated on the device in pieces from one seeded generator (never `repeat`)"""
    n = LC.numel(shape)
    out = torch.empty(n, dtype=dtype, device=dev)
    for s in range(0, n, piece):
        m = min(piece, n - s)
        out[s:s + m] = torch.randint(lo, hi + 1, (m,), generator=g, device=dev, dtype=dtype)
    return out.view(shape)


def _cut(c, dim, a, b, ca, ea, cw, ew):
    """the operands of rows / columns / batch elements a .. b of the output, as contiguous tensors"""
    if dim == "batch":
        out = tuple(t[a:b] for t in (ca, ea, cw, ew))
    elif dim == "M":
        out = (ca[..., a:b, :], ea[..., a:b, :], cw, ew)
    elif c.layout == "kn":
        out = (ca, ea, cw[..., a:b], ew[..., a:b])
    else:
        out = (ca, ea, cw[..., a:b, :], ew[..., a:b, :])
    return tuple(t.contiguous() for t in out)


def _cut_out(dim, y, a, b):
    return (y[a:b] if dim == "batch" else (y[..., a:b, :] if dim == "M" else y[..., a:b])).contiguous()


@pytest.mark.parametrize("name", [c.name for c in MC.LARGE if c.op != "pack"])
def test_offset_past_2_31(dmx, cuda, name):
    """peak device memory: MC.large_peak_bytes(case) -- ra_K 3.0, rw_K 3.0, m_N_n 9.0, bz_M_K 3.2, kn_row_N 4.1, kn_bz_N_K 3.2,
    out0 9.2 GiB.  One offset family of the kernel exceeds 2^31 + 2^20; every other operand is small."""
    ops, c = dmx.ops, MC.LARGE_BY_NAME[name]
    _need(c)
    kn, nb, out = c.layout == "kn", c.K // c.B, DT[c.out]
    lead = (c.batch,) if c.op == "bmm" else ()
    g = torch.Generator(device=cuda).manual_seed(1000 + len(name))
    ca = _device_ints(lead + (c.M, c.K), -128, 127, torch.int8, g, cuda)
    cw = _device_ints(lead + ((c.K, c.N) if kn else (c.N, c.K)), -128, 127, torch.int8, g, cuda)
    ea = _device_ints(lead + (c.M, nb), 110, 140, torch.uint8, g, cuda)
    ew = _device_ints(lead + ((nb, c.N) if kn else (c.N, nb)), 110, 140, torch.uint8, g, cuda)
    assert max(t.numel() for t in (ca, cw, ea, ew)) > MC.MIN_TARGET or c.M * c.N * max(c.batch, 1) > MC.MIN_TARGET
    assert _class(ops, c.op, c.layout, (ca,), (cw,), c.B) is not None
    before = dict(_routes(dmx, c.op))
    full = _run(ops, c.op, c.layout, (ca, ea), (cw, ew), 8, 8, c.B, out, fused=True)
    assert _routes(dmx, c.op) == dict(before, fused=before["fused"] + 1) and full.shape == lead + (c.M, c.N)
    # 1. the whole output: the same kernel on contiguous slices, every operand of which has fewer than 2^31 elements
    for a, b in MC.large_cuts(c):
        sl = _cut(c, c.cut, a, b, ca, ea, cw, ew)
        assert all(t.is_contiguous() and t.numel() < MC.TWO31 for t in sl) and (b - a) * full.numel() // getattr(c, c.cut) < MC.TWO31
        part = _run(ops, c.op, c.layout, sl[:2], sl[2:], 8, 8, c.B, out, fused=True)
        bad = LC.mismatches_on_device(_cut_out(c.cut, full, a, b), part)
        assert bad == 0, (name, "slice", (a, b), "mismatches", bad)
        del sl, part
    # 2. 64 rows or columns straddling element 2^31, and the last 64: the chain on copies
    for bi, dim, a, b in MC.large_windows(c):
        ops4, y = (ca, ea, cw, ew), full
        if bi is not None:
            ops4, y = _cut(c, "batch", bi, bi + 1, *ops4), _cut_out("batch", full, bi, bi + 1)
        win = _cut(c, dim, a, b, *ops4)
        chain = _run(ops, c.op, c.layout, win[:2], win[2:], 8, 8, c.B, out, fused=False)
        bad = LC.mismatches_on_device(_cut_out(dim, y, a, b), chain)
        assert bad == 0, (name, "window", (bi, dim, a, b), "mismatches", bad)
        del win, chain, ops4, y
    del full, ca, cw, ea, ew
    torch.cuda.empty_cache()


def test_column_pack_offset_past_2_31(dmx, cuda):
    """peak device memory: 9.1 GiB (the bf16 input 4.0, its codes 2.0, and the transposing route on a quarter).  e0 = ob B N + column of
    bfp_pack_cols_kernel exceeds 2^31 + 2^20; the reference is the transposing route on chunks of whole row blocks."""
    ops, c = dmx.ops, MC.LARGE_BY_NAME["pack_cols_e0"]
    _need(c)
    x = LC.device_input("heavy", (1, c.K, c.N), torch.bfloat16, 77, cuda)
    assert x.numel() > MC.MIN_TARGET
    x[0, c.K - 3, 5] = float("nan")               # beyond element 2^31: a NaN, an Inf, an all-zero block and a denormal maximum
    x[0, c.K - 2, 70] = float("inf")
    x[0, c.K - c.B:, 129] = 0.0
    x[0, c.K - c.B:, 300] = 1e-40
    routes = dmx._front._bfp_pack_cols_routes
    before = dict(routes)
    codes, exps = ops.bfp_pack(x, 8, c.B, True, block_dim=-2)
    assert routes == dict(before, fused=before["fused"] + 1)
    assert int(exps[0, -1, 5]) == 255 == int(exps[0, -1, 70]) and int(exps[0, -1, 129]) == 0 == int(exps[0, -1, 300])
    for a, b in MC.large_cuts(c):
        xs = x[:, a:b]
        assert xs.is_contiguous() and xs.data_ptr() % 16 == 0 and xs.numel() < MC.TWO31
        pc, pe = ops.bfp_pack(xs, 8, c.B, True, block_dim=-2, fused=False)
        assert LC.mismatches_on_device(codes[:, a:b], pc) == 0, (a, b)
        assert LC.mismatches_on_device(exps[:, a // c.B:b // c.B], pe) == 0, (a, b)
        del pc, pe
    assert routes["chain"] == before["chain"] + len(MC.large_cuts(c))
    del x, codes, exps
    torch.cuda.empty_cache()
