"""-m gpu: the block-Hadamard rotation fused into the quantize-dequantize casts (csrc/hadamard.hip: dmxq_hadamard_qdq) and what is built
on it: ops.hadamard / ops.hadamard_qdq through both bindings, the "hadamard" pre_transform of CastTo, a Linear with a rotated weight
cast, benchmark.format_sweep(hadamard=...).

The checker is tests/_hadamard_ref.py (the butterfly in torch float32 on the CPU, pinned to the dense matrix by
tests/test_hadamard_host.py) composed with the CPU oracle's casts.  Every comparison is BIT FOR BIT (bits_equal); where a NaN is planted
or generated (Inf - Inf), any NaN matches any NaN (mismatches_nan_aware: sign and payload of a generated NaN are platform-defined).
fused=True everywhere unless stated: a call the kernel does not take raises instead of quietly checking the three-launch chain."""
import ctypes

import pytest
import torch

import _hadamard_ref as R
from _data import bits_equal, make, mismatches_nan_aware

pytestmark = pytest.mark.gpu
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
SIZES = R.SIZES


# ---------------------------------------------------------------------------------------------------- the fused formats and their oracle casts
def _amax_scale(r, p, per_row=False):
    """amax / (2^(p-1) - 1) of the rotated reference r, float32 (one per row with per_row)"""
    a = r.abs().amax(dim=-1) if per_row else r.abs().max().reshape(1)
    return (a / float(2 ** (p - 1) - 1)).to(torch.float32)


def fused_case(O, name, H, x):
    """-> (format shorthand, oracle cast of the rotated float32 reference, keyword arguments of ops.hadamard_qdq); x: the CPU input"""
    r = R.rotate_ref(x, H)
    if name == "bfp8_16":
        return "BFP[8|8]{16}(SN)", lambda t: O.bfp_cast(t, 8, 16), {}
    if name == "bfp4_32_asym":
        return "BFP[4|8]{32}(_N)", lambda t: O.bfp_cast(t, 4, 32, symmetric=False), {}
    if name == "bfp8_H":
        return f"BFP[8|8]{{{H}}}(SN)", lambda t: O.bfp_cast(t, 8, H), {}
    if name == "mxfp4":
        return "MXFP4[E2M1]{32}", lambda t: O.mxfp_cast(t, 1, 2, 32), {}
    if name == "mxfp8":
        return "MXFP8[E4M3]{32}", lambda t: O.mxfp_cast(t, 3, 4, 32), {}
    if name == "fp8":
        return "FP[1|5|2,15](FN)", lambda t: O.floating_point_cast(t, 2, 5, 15, True), {}
    if name in ("xp8", "xp4"):
        p = int(name[2])
        sc, zp = _amax_scale(r, p), torch.zeros(1, dtype=torch.int64)
        return f"XP[{p},0](CSN)", lambda t: O.fixed_point_affine_cast(t, p, 0, True, True, sc, zp), {"scale": sc, "zero_point": zp}
    if name == "xp4_row":
        sc = _amax_scale(r, 4, per_row=True).reshape(-1)
        zp = torch.zeros(sc.numel(), dtype=torch.int64)
        return ("XP[4,0](CSN)", lambda t: O.fixed_point_affine_cast(t.reshape(-1, t.shape[-1]), 4, 0, True, True, sc, zp, ch_axis=0).reshape(t.shape),
                {"scale": sc, "zero_point": zp, "per_row": True})
    raise ValueError(name)


def run_fused(f, x, H, fmt, kw, dev, **more):
    kw = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    return f.hadamard_qdq(x.to(dev), H, fmt, **kw, **more)


# (format, H, dtype, shape): every format at sizes below, at and above its own block, 16-bit and float32 inputs, rows that are no
# multiple of anything and more than one workgroup of 256 lane-vectors
FUSED = [("bfp8_16", 16, BF16, (67, 48)), ("bfp8_16", 64, F32, (67, 192)), ("bfp8_16", 256, BF16, (67, 768)),
         ("bfp4_32_asym", 32, BF16, (67, 96)), ("bfp4_32_asym", 128, F16, (67, 384)),
         ("bfp8_H", 8, BF16, (67, 24)), ("bfp8_H", 64, BF16, (67, 192)), ("bfp8_H", 256, F32, (67, 768)),
         ("mxfp4", 32, BF16, (67, 96)), ("mxfp4", 64, F32, (67, 192)), ("mxfp4", 256, BF16, (67, 768)),
         ("mxfp8", 32, BF16, (67, 96)), ("mxfp8", 128, F32, (67, 384)),
         ("fp8", 8, F32, (67, 24)), ("fp8", 128, BF16, (67, 384)),
         ("xp8", 64, BF16, (67, 192)), ("xp4", 16, F32, (67, 48)), ("xp4", 256, BF16, (67, 768)),
         ("xp4_row", 128, BF16, (130, 384)), ("xp4_row", 128, F32, (130, 384))]


# ---------------------------------------------------------------------------------------------------- rotation only
@pytest.mark.parametrize("H", SIZES)
def test_rotation_only(dmx, cuda, H):
    """every size; bf16 / f16 / float32 in; the same dtype and float32 out; [3, H], [67, 3H], [5, 8H]; four kinds of data"""
    for dt in (BF16, F16, F32):
        for shape in ((3, H), (67, 3 * H), (5, 8 * H)):
            for kind in ("normal", "heavy", "outlier", "mixed_nd"):
                x = make(kind, shape, seed=H + len(kind), dtype=dt, block=H)
                ref = R.rotate_ref(x, H)
                xd = x.to(cuda)
                for od in (dt, F32):
                    got = dmx.ops.hadamard(xd, H, out_dtype=od)
                    assert got.dtype == od and got.shape == x.shape and got.is_contiguous()
                    assert bits_equal(got, ref.to(od)) == 0, (H, dt, shape, kind, od)
                assert bits_equal(dmx.ops.hadamard(xd, H), ref.to(dt)) == 0   # (out_dtype defaults to the input's)


def test_rotation_validation(dmx, cuda):
    x = torch.zeros(4, 96, device=cuda)
    for size in (48, 4, 512):
        with pytest.raises(ValueError):
            dmx.ops.hadamard(x, size)
    with pytest.raises(ValueError):
        dmx.ops.hadamard(x, 64)               # 96 % 64
    with pytest.raises(ValueError):
        dmx.ops.hadamard_qdq(x, 64, "BFP[8|8]{16}(SN)")
    with pytest.raises(ValueError):
        dmx.ops.hadamard(x, 32, dim=2)
    with pytest.raises(dmx.DmxqError):
        dmx.ops.hadamard(x.cpu(), 32)


# ---------------------------------------------------------------------------------------------------- fused formats
@pytest.mark.parametrize("name,H,dt,shape", FUSED, ids=lambda v: str(v).replace("torch.", ""))
def test_fused_formats(dmx, oracle, cuda, name, H, dt, shape):
    """each fused format with and without the inverse rotation, against the reference; fused=None / True / False give the same bits"""
    x = make("outlier", shape, seed=H + shape[0], dtype=dt, block=H)
    fmt, cast, kw = fused_case(oracle, name, H, x)
    for inverse in (True, False):
        want = R.rotated_cast_ref(x, H, cast, inverse, dt)
        got = run_fused(dmx.ops, x, H, fmt, kw, cuda, inverse=inverse, fused=True)
        assert got.dtype == dt and got.shape == x.shape
        assert bits_equal(got, want) == 0, (name, H, dt, inverse, bits_equal(got, want))
        for fused in (None, False):
            assert bits_equal(run_fused(dmx.ops, x, H, fmt, kw, cuda, inverse=inverse, fused=fused), want) == 0, (name, H, inverse, fused)
    want32 = R.rotated_cast_ref(x, H, cast, True, F32)
    assert bits_equal(run_fused(dmx.ops, x, H, fmt, kw, cuda, fused=True, out_dtype=F32), want32) == 0


def test_small_cast_blocks(dmx, oracle, cuda):
    """cast blocks smaller than a lane's vector (2 and 4 elements: one pass of the cast body per sub-block) and of exactly one vector"""
    for dt, H in ((BF16, 32), (F32, 16)):
        x = make("heavy", (9, 4 * H), seed=11, dtype=dt, block=H)
        for B in (2, 4, 8):
            for fmt, cast in ((f"BFP[6|8]{{{B}}}(SN)", lambda t: oracle.bfp_cast(t, 6, B)), (f"MXFP6[E3M2]{{{B}}}", lambda t: oracle.mxfp_cast(t, 2, 3, B))):
                want = R.rotated_cast_ref(x, H, cast, True, dt)
                assert bits_equal(dmx.ops.hadamard_qdq(x.to(cuda), H, fmt, fused=True), want) == 0, (dt, H, fmt)


def test_bare_fixed_point_with_negative_zeros(dmx, oracle, cuda):
    """a FixedPoint format without scale / zero point is scale 1, zero point 0 through the affine form on the kernel AND on the chain:
    the same bits, negative zeros in the rotated tensor included (an all -0.0 block rotates to -0.0 and +0.0)"""
    H = 32
    x = make("normal", (8, 2 * H), seed=97, dtype=F32, block=H) * 3.0
    x[1, :H] = -0.0
    x[2, 5] = -0.0
    r = R.rotate_ref(x, H)
    assert bool(((r == 0) & (r.view(torch.int32) < 0)).any())
    one, zero = torch.ones(1), torch.zeros(1, dtype=torch.int64)
    for inverse in (True, False):
        want = R.rotated_cast_ref(x, H, lambda t: oracle.fixed_point_affine_cast(t, 8, 3, True, True, one, zero), inverse, F32)
        for fused in (True, False, None):
            got = dmx.ops.hadamard_qdq(x.to(cuda), H, "XP[8,+3](CSN)", inverse=inverse, fused=fused)
            assert bits_equal(got, want) == 0, (inverse, fused)


# ---------------------------------------------------------------------------------------------------- planted blocks
POW2_ROWS = ((100, (1, 44, 45, 89)), (4, (1, 2, 3, 5)))   # (v, j of the four blocks): rotated maxima 2^v (1 - j 2^-24)


def _planted(H):
    """[7, 4H] float32, planted BY BLOCK INDEX (row, block): (0, 1) all zero; (1, 0) one NaN; (2, 3) one Inf; (3, 2) a denormal maximum;
    rows 4 and 5: every block a single nonzero element m = 2^v (1 - j 2^-24) / c, whose rotation is +-m c = +-2^v (1 - j 2^-24)
    everywhere (H = 16, 64, 256: c is a power of two and m c is exact) -- a block maximum a few ulps below a power of two, on both
    sides of the float32 log2's rounding rule (oracle.c oracle_floor_log2f: at v = 100 the exponent is bumped for j <= 44, at v = 4 for
    j <= 1); row 6: heavy data"""
    assert H in (16, 64, 256)
    x = make("heavy", (7, 4 * H), seed=3 * H, block=H).clone()
    x[0, H:2 * H] = 0.0
    x[1, 5] = float("nan")
    x[2, 3 * H + 7] = float("inf")
    x[3, 2 * H:3 * H] = make("denormal", (H,), seed=17)
    c = float(R.scale_of(H))
    for row, (v, js) in zip((4, 5), POW2_ROWS):
        x[row] = 0.0
        for b, j in enumerate(js):
            x[row, b * H + (11 * b + 3) % H] = 2.0 ** v * (1.0 - j * 2.0 ** -24) / c * (-1.0 if b & 1 else 1.0)
    return x


@pytest.mark.parametrize("H", (16, 64, 256))
def test_planted_blocks(dmx, oracle, cuda, H):
    x = _planted(H)
    r = R.rotate_ref(x, H)
    assert bool(torch.isnan(r[1, :H]).all()) and bool((r[0, H:2 * H] == 0).all())          # a block with a NaN becomes all NaN
    for row, (v, js) in zip((4, 5), POW2_ROWS):
        assert bool((r[row].abs().reshape(4, H) == torch.tensor([2.0 ** v * (1.0 - j * 2.0 ** -24) for j in js]).reshape(4, 1)).all())
    assert mismatches_nan_aware(dmx.ops.hadamard(x.to(cuda), H), r) == 0
    B = min(32, H)
    sc, zp = torch.tensor([0.05]), torch.zeros(1, dtype=torch.int64)

    def mxfp(man, exp, block):
        """the oracle's MXFP cast, every block of it: oracle_mxfp_qdq is total (a NaN or Inf maximum gives what the reference's float32
        tensor ops give, pinned by tests/golden/blockfmt_classes.npz), so no expected value comes from the library under test; such a
        block stays non-finite"""
        def cast(t):
            q = oracle.mxfp_cast(t, man, exp, block)
            poisoned = ~torch.isfinite(t).reshape(-1, block).all(dim=-1, keepdim=True).expand(-1, block).reshape(t.shape)
            assert not bool(torch.isfinite(q[poisoned]).any())
            return q
        return cast

    cases = [("BFP[8|8]{16}(SN)", lambda t: oracle.bfp_cast(t, 8, 16), {}),
             (f"BFP[4|8]{{{B}}}(_N)", lambda t: oracle.bfp_cast(t, 4, B, symmetric=False), {}),
             (f"MXFP4[E2M1]{{{B}}}", mxfp(1, 2, B), {}),
             (f"MXFP8[E4M3]{{{H}}}", mxfp(3, 4, H), {}),
             ("XP[8,0](CSN)", lambda t: oracle.fixed_point_affine_cast(t, 8, 0, True, True, sc, zp), {"scale": sc, "zero_point": zp})]
    for fmt, cast, kw in cases:
        for inverse in (True, False):
            want = R.rotated_cast_ref(x, H, cast, inverse, F32)
            got = run_fused(dmx.ops, x, H, fmt, kw, cuda, inverse=inverse, fused=True)
            assert mismatches_nan_aware(got, want) == 0, (H, fmt, inverse, mismatches_nan_aware(got, want))
            assert bool(torch.isnan(got[1, :H]).all()), (H, fmt, inverse)          # the block with the NaN is all NaN
            assert bool((got[0, H:2 * H] == 0).all()), (H, fmt, inverse)           # the zero block stays zero
    # FP[1|5|2,15] has no NaN codes: a NaN saturates to +-max with the NaN's SIGN, which after the subtractions of the rotation is
    # platform-defined -- every row but the NaN's (the Inf block rotates to +-Inf with defined signs: a stage only ever pairs an
    # infinite element with a finite one)
    keep = x[[0, 2, 3, 4, 5, 6]]
    assert not bool(torch.isnan(R.rotate_ref(keep, H)).any())
    want = R.rotated_cast_ref(keep, H, lambda t: oracle.floating_point_cast(t, 2, 5, 15, True), True, F32)
    assert bits_equal(dmx.ops.hadamard_qdq(keep.to(cuda), H, "FP[1|5|2,15](FN)", fused=True), want) == 0


# ---------------------------------------------------------------------------------------------------- in place, alignment, other dims, grid
def test_in_place_through_the_c_abi(dmx, oracle, cuda):
    """in == out with equal widths, straight through include/dmxq.h"""
    lib = dmx._lib
    L = lib.lib()
    H = 128
    for dt, code in ((BF16, lib.BF16), (F32, lib.F32)):
        x = make("outlier", (19, 3 * H), seed=23, dtype=dt, block=H)
        want = R.rotated_cast_ref(x, H, lambda t: oracle.bfp_cast(t, 8, 16), True, dt)
        buf = x.to(cuda)
        f = lib.GptqFormat(lib.GPTQ_BFP, 8, 16, 1, 0, 0, 0, 0, 0, 0, 0, 0)
        rc = L.dmxq_hadamard_qdq(lib.ptr(buf), lib.ptr(buf), code, code, 19, 3 * H, H, 1, ctypes.byref(f), None, None, lib.stream_of(buf))
        assert rc == lib.OK
        assert bits_equal(buf, want) == 0
        rot = x.to(cuda)
        assert L.dmxq_hadamard_qdq(lib.ptr(rot), lib.ptr(rot), code, code, 19, 3 * H, H, 0, None, None, None, lib.stream_of(rot)) == lib.OK
        assert bits_equal(rot, R.rotate_ref(x, H).to(dt)) == 0


def test_unaligned_views(dmx, oracle, cuda):
    """a sliced view whose pointer is 4-byte but not 16-byte aligned: the element-wise loads of the same kernel"""
    H = 64
    for dt, off in ((F32, 1), (BF16, 2), (F32, 3)):
        base = make("heavy", (off + 21 * 2 * H,), seed=29, dtype=dt, block=H)
        x = base[off:].reshape(21, 2 * H)
        xd = base.to(cuda)[off:].reshape(21, 2 * H)
        assert xd.is_contiguous() and xd.data_ptr() % 16 != 0 and xd.data_ptr() % 4 == 0
        assert bits_equal(dmx.ops.hadamard(xd, H), R.rotate_ref(x, H).to(dt)) == 0
        want = R.rotated_cast_ref(x, H, lambda t: oracle.mxfp_cast(t, 1, 2, 32), True, dt)
        assert bits_equal(dmx.ops.hadamard_qdq(xd, H, "MXFP4[E2M1]{32}", fused=True), want) == 0


def test_rotated_dimension_not_last(dmx, oracle, cuda):
    """block_dim = 1 on [2, 64, 5, 5]: transposed to the last dimension with a copy, rotated, transposed back (the slow path)"""
    x = make("outlier", (2, 64, 5, 5), seed=31, dtype=BF16, block=16)
    xt = x.movedim(1, -1).contiguous()
    for H in (32, 64):
        want_r = R.rotate_ref(xt, H).movedim(-1, 1).contiguous()
        got = dmx.ops.hadamard(x.to(cuda), H, dim=1, out_dtype=F32)
        assert got.shape == x.shape and got.is_contiguous() and bits_equal(got, want_r) == 0
        want = R.rotated_cast_ref(xt, H, lambda t: oracle.bfp_cast(t, 8, 16), True, BF16).movedim(-1, 1).contiguous()
        for fused in (True, False):
            assert bits_equal(dmx.ops.hadamard_qdq(x.to(cuda), H, "BFP[8|8]{16}(SN)", block_dim=1, fused=fused), want) == 0
        assert bits_equal(dmx.ops.hadamard_qdq(x.to(cuda), H, "BFP[8|8]{16}(SN)", block_dim=-3, fused=True), want) == 0


def test_many_workgroups(dmx, oracle, cuda):
    """The kernel is NOT persistent: one tile of 256 lane-vectors per workgroup and a grid of ceil(vectors / 256) workgroups -- no
    workgroup loops.  H = 64, L = 256, rows from the device's CU count: more than three workgroups per CU, the last one partial."""
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    H, L = 64, 256
    rows = 3 * cus * 8 + 5            # bf16: 8 rows of 256 per workgroup (2048 elements)
    x = make("normal", (rows, L), seed=37, dtype=BF16, block=H)
    want = R.rotated_cast_ref(x, H, lambda t: oracle.mxfp_cast(t, 1, 2, 32), True, BF16)
    assert bits_equal(dmx.ops.hadamard_qdq(x.to(cuda), H, "MXFP4[E2M1]{32}", fused=True), want) == 0
    assert bits_equal(dmx.ops.hadamard(x.to(cuda), H), R.rotate_ref(x, H).to(BF16)) == 0


# ---------------------------------------------------------------------------------------------------- what the kernel does not take
def test_unfused_formats_run_on_the_chain(dmx, oracle, cuda):
    """SBFP and an up-rounding BFP raise NotImplementedError under fused=True and run under fused=None; so do blocks that do not divide the
    rotation size, and per-group affine scales"""
    H = 64
    x = make("outlier", (33, 3 * H), seed=41, dtype=BF16, block=H)
    xd = x.to(cuda)
    r = R.rotate_ref(x, H)
    cases = [("SBFP<XP[8,0](CSN)><FP[0|4|4,7](FN)>{16}", lambda t: oracle.sbfp_cast(t, 8, 16, 4, 4, 7), {}),
             ("BFP[8|8]{16}(SU)", lambda t: oracle.bfp_cast(t, 8, 16, rounding="up"), {}),
             ("BFP[8|8]{48}(SN)", lambda t: oracle.bfp_cast(t, 8, 48), {})]
    g = 11
    mn, mx = oracle.group_minmax(r, 0, g)
    sc = (torch.maximum(mn.abs(), mx.abs()) / 127.0).to(F32)
    zp = torch.zeros(sc.numel(), dtype=torch.int64)
    cases.append(("XP[8,0](CSN)", lambda t: oracle.fixed_point_affine_cast(t, 8, 0, True, True, sc, zp, ch_axis=0, group_size=g),
                  {"scale": sc, "zero_point": zp, "ch_axis": 0, "group_size": g}))
    for fmt, cast, kw in cases:
        with pytest.raises(NotImplementedError):
            run_fused(dmx.ops, x, H, fmt, kw, cuda, fused=True)
        for inverse in (True, False):
            want = R.rotated_cast_ref(x, H, cast, inverse, BF16)
            for fused in (None, False):
                assert bits_equal(run_fused(dmx.ops, x, H, fmt, kw, cuda, inverse=inverse, fused=fused), want) == 0, (fmt, inverse, fused)
    # stochastic rounding runs through the chain: every element is one of its two neighbours on the format's grid, both occur
    with pytest.raises(NotImplementedError):
        dmx.ops.hadamard_qdq(xd, H, "BFP[8|8]{16}(SS)", inverse=False, fused=True)
    lo = R.rotated_cast_ref(x, H, lambda t: oracle.bfp_cast(t, 8, 16, rounding="down"), False, F32)
    hi = R.rotated_cast_ref(x, H, lambda t: oracle.bfp_cast(t, 8, 16, rounding="up"), False, F32)
    a32 = dmx.ops.hadamard_qdq(xd, H, "BFP[8|8]{16}(SS)", inverse=False, out_dtype=F32).cpu()
    assert bool(((a32 == lo) | (a32 == hi)).all())
    assert bool(((a32 == lo) & (lo != hi)).any()) and bool(((a32 == hi) & (lo != hi)).any())


def test_both_bindings(dmx, oracle, cuda):
    for name, H, dt, shape in (FUSED[1], FUSED[8], FUSED[15], FUSED[18]):
        x = make("heavy", shape, seed=43, dtype=dt, block=H)
        fmt, cast, kw = fused_case(oracle, name, H, x)
        want = R.rotated_cast_ref(x, H, cast, True, dt)
        for binding in ("ctypes", "torch"):
            f = dmx.ops.front(binding)
            assert bits_equal(run_fused(f, x, H, fmt, kw, cuda, fused=True), want) == 0, (binding, name)
            assert bits_equal(f.hadamard(x.to(cuda), H, out_dtype=F32), R.rotate_ref(x, H)) == 0
    # the dispatcher op itself, and its meta kernel
    xd = make("normal", (4, 64), seed=1, dtype=BF16).to(cuda)
    y = torch.ops.dmxq.hadamard_qdq(xd, 64, False, [], None, None, None)
    assert bits_equal(y, R.rotate_ref(xd.cpu(), 64).to(BF16)) == 0
    m = torch.ops.dmxq.hadamard_qdq(xd.to("meta"), 64, True, [0, 8, 16, 1, 0, 0, 0, 0, 0, 0, 0, 0], None, None, torch.float32)
    assert m.device.type == "meta" and m.shape == xd.shape and m.dtype == F32


# ---------------------------------------------------------------------------------------------------- CastTo
def test_castto_one_key_transform_equals_the_op(dmx, oracle, cuda):
    x = make("outlier", (40, 256), seed=47, dtype=BF16, block=64)
    xd = x.to(cuda)
    for spec, inverse in ((64, True), ({"size": 64, "inverse": False}, False)):
        for fmt, cast in (("MXFP4[E2M1]{32}", lambda t: oracle.mxfp_cast(t, 1, 2, 32)), ("BFP[8|8]{16}(SN)", lambda t: oracle.bfp_cast(t, 8, 16))):
            c = dmx.CastTo(format=fmt).to(cuda)
            c.set_pre_transform({"hadamard": spec})
            got = c(xd)
            assert got.dtype == BF16
            assert bits_equal(got, dmx.ops.hadamard_qdq(xd, 64, fmt, inverse=inverse, fused=True)) == 0
            assert bits_equal(got, R.rotated_cast_ref(x, 64, cast, inverse, BF16)) == 0


def test_castto_with_shaping_and_shortcut(dmx, oracle, cuda):
    """shaping -> shortcut save -> pre-format -> rotation -> cast -> inverse rotation -> shortcut restore -> inverse shaping ->
    .to(physical dtype), spelled out by hand"""
    x = make("outlier", (6, 128, 10), seed=53, dtype=BF16, block=16)
    c = dmx.CastTo(format="BFP[8|8]{16}(SN)").to(cuda)
    c.set_pre_transform({"shaping": [("permute", (0, 2, 1)), ("flatten", (0, 1))], "noquant_shortcut": [0], "format": "FP[1|5|10,15](FN)",
                         "hadamard": 32})
    got = c(x.to(cuda))
    t = x.permute(0, 2, 1).flatten(0, 1)                              # [60, 128], blocks along the last dimension
    shortcut = t[0].clone()
    t = oracle.floating_point_cast(t.float(), 10, 5, 15, True)        # the pre-format, float32 out
    t = R.rotated_cast_ref(t, 32, lambda v: oracle.bfp_cast(v, 8, 16), True, BF16)
    t[0] = shortcut
    want = t.reshape(6, 10, 128).permute(0, 2, 1).to(BF16)
    assert got.shape == x.shape and got.dtype == BF16
    assert bits_equal(got.contiguous(), want.contiguous()) == 0


def test_castto_minmax_calibration_in_the_rotated_basis(dmx, oracle, cuda):
    x = make("outlier", (48, 128), seed=59, dtype=BF16, block=128)
    r = R.rotate_ref(x, 128)
    for qscheme, ch_axis in ((torch.per_tensor_symmetric, -1), (torch.per_channel_symmetric, 0)):
        c = dmx.CastTo(format="XP[8,0](CSN)").to(cuda)
        c.set_pre_transform({"hadamard": 128})
        c.enable_calibration(True, observer_cls=dmx.MinMaxObserver, qscheme_to_overload=qscheme, ch_axis=ch_axis)
        y = c(x.to(cuda))
        assert bits_equal(y, x) == 0                                    # observe only: the input comes back untouched
        c.enable_calibration(False)
        per_row = qscheme == torch.per_channel_symmetric
        mn = r.amin(dim=-1) if per_row else r.min().reshape(1)
        mx = r.amax(dim=-1) if per_row else r.max().reshape(1)
        sc, zp = dmx.ops.qparams(mn.to(cuda), mx.to(cuda), -127, 127, True)
        assert bits_equal(c.scale.reshape(-1), sc.reshape(-1)) == 0 and bits_equal(c.zero_point.reshape(-1), zp.reshape(-1)) == 0
        sc_c, zp_c = sc.cpu(), zp.cpu()
        cast = (lambda t: oracle.fixed_point_affine_cast(t, 8, 0, True, True, sc_c, zp_c, ch_axis=0)) if per_row else \
               (lambda t: oracle.fixed_point_affine_cast(t, 8, 0, True, True, sc_c, zp_c))
        assert bits_equal(c(x.to(cuda)), R.rotated_cast_ref(x, 128, cast, True, BF16)) == 0


def test_castto_one_call_and_step_by_step_routes_agree(dmx, oracle, cuda):
    """forward takes ONE ops.hadamard_qdq call when "hadamard" is the only key and the step-by-step route (rotation, _quantize,
    rotation) otherwise: the same bits for per-group scales and for a channel axis on a tensor that is not 2-D, and the reference's"""
    x3 = make("outlier", (3, 10, 128), seed=101, dtype=BF16, block=64)
    x2 = make("outlier", (24, 128), seed=103, dtype=BF16, block=64)
    for x, qscheme, ch_axis, group in ((x3, torch.per_channel_symmetric, 1, None), (x2, torch.per_tensor_symmetric, 0, 5),
                                       (x3, torch.per_tensor_symmetric, 1, 4)):
        outs = []
        for extra in ({}, {"noquant_shortcut": None}):
            c = dmx.CastTo(format="XP[8,0](CSN)").to(cuda)
            c.set_pre_transform({"hadamard": 64, **extra})
            c.enable_calibration(True, observer_cls=dmx.MinMaxObserver, qscheme_to_overload=qscheme, ch_axis=ch_axis, group_size=group)
            c(x.to(cuda))
            c.enable_calibration(False)
            outs.append((c(x.to(cuda)), c.scale.detach().cpu().reshape(-1), c.zero_point.detach().cpu().reshape(-1)))
        (a, sc, zp), (b, sc_b, _) = outs
        assert bits_equal(sc, sc_b) == 0 and bits_equal(a, b) == 0, (qscheme, ch_axis, group)
        want = R.rotated_cast_ref(x, 64, lambda t: oracle.fixed_point_affine_cast(t, 8, 0, True, True, sc, zp, ch_axis=ch_axis, group_size=group),
                                  True, BF16)
        assert bits_equal(a, want) == 0, (qscheme, ch_axis, group)


def test_castto_measure_error(dmx, cuda):
    x = make("outlier", (64, 256), seed=61, dtype=BF16, block=64).to(cuda)
    c = dmx.CastTo(format="MXFP4[E2M1]{32}").to(cuda)
    c.set_pre_transform({"hadamard": 64})
    assert bits_equal(c.measure_error(x), dmx.ops.error_stats(x, c(x))) == 0
    c.set_pre_transform({"hadamard": 64, "noquant_shortcut": [0]})
    with pytest.raises(NotImplementedError):
        c.measure_error(x)


def test_backward(dmx, cuda):
    """inverse=False: the gradient is rotate_ref(grad); inverse=True: the incoming gradient (straight-through)"""
    x = make("normal", (12, 128), seed=67, dtype=F32, block=64)
    g = make("heavy", (12, 128), seed=71, dtype=F32, block=64)
    for spec, want in ((64, g), ({"size": 64, "inverse": False}, R.rotate_ref(g, 64))):
        c = dmx.CastTo(format="BFP[8|8]{16}(SN)").to(cuda)
        for extra in ({}, {"noquant_shortcut": None}):   # the one-call path and the step-by-step path of forward
            c.set_pre_transform({"hadamard": spec, **extra})
            xd = x.to(cuda).requires_grad_(True)
            c(xd).backward(g.to(cuda))
            assert bits_equal(xd.grad, want) == 0, (spec, extra)
    xd = x.to(cuda).requires_grad_(True)
    dmx.ops.hadamard(xd, 64).backward(g.to(cuda))
    assert bits_equal(xd.grad, R.rotate_ref(g, 64)) == 0


# ---------------------------------------------------------------------------------------------------- graph capture
def test_graph_capture(dmx, oracle, cuda):
    H = 64
    x0 = make("normal", (32, 256), seed=73, dtype=BF16, block=H)
    x1 = make("outlier", (32, 256), seed=79, dtype=BF16, block=H)
    buf = x0.to(cuda).clone()
    sc, zp = torch.tensor([0.03], device=cuda), torch.zeros(1, dtype=torch.int64, device=cuda)
    dmx.ops.hadamard_qdq(buf, H, "MXFP4[E2M1]{32}", fused=True)        # (warm-up outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_a = dmx.ops.hadamard_qdq(buf, H, "MXFP4[E2M1]{32}", fused=True)
        out_b = dmx.ops.hadamard_qdq(buf, H, "XP[8,0](CSN)", scale=sc, zero_point=zp, inverse=False, fused=True)
    for x in (x1, x0):
        buf.copy_(x.to(cuda))
        graph.replay()
        torch.cuda.synchronize()
        assert bits_equal(out_a, dmx.ops.hadamard_qdq(x.to(cuda), H, "MXFP4[E2M1]{32}", fused=True)) == 0
        assert bits_equal(out_a, R.rotated_cast_ref(x, H, lambda t: oracle.mxfp_cast(t, 1, 2, 32), True, BF16)) == 0
        assert bits_equal(out_b, dmx.ops.hadamard_qdq(x.to(cuda), H, "XP[8,0](CSN)", scale=sc, zero_point=zp, inverse=False, fused=True)) == 0


# ---------------------------------------------------------------------------------------------------- modules
def test_linear_with_a_rotated_weight_cast(dmx, oracle, cuda):
    """forward, fold_weights_and_biases and GPTQ (through the loop: the fused column kernel steps aside for a pre_transform) with
    pre_weight_transform {"hadamard": 64}"""
    torch.manual_seed(0)
    m = dmx.nn.Linear(128, 48).to(cuda)
    m.configure({"weight_format": "MXFP4[E2M1]{32}", "pre_weight_transform": {"hadamard": 64}})
    w = m.weight.detach().cpu().clone()
    want = R.rotated_cast_ref(w, 64, lambda t: oracle.mxfp_cast(t, 1, 2, 32), True, F32)
    x = torch.randn(5, 128, device=cuda)
    with torch.no_grad():
        assert bits_equal(m.weight_hypernet(m.weight), want) == 0
        y = m(x)
        plain = dmx.nn.Linear(128, 48).to(cuda)          # the same module with the rotated cast's result as its weight and no cast
        plain.weight.copy_(want.to(cuda))
        plain.bias.copy_(m.bias)
        assert bits_equal(y, plain(x)) == 0
    g = dmx.nn.Linear(128, 48).to(cuda)
    g.configure({"weight_format": "MXFP4[E2M1]{32}", "pre_weight_transform": {"hadamard": 64}})
    with torch.no_grad():
        g.weight.copy_(m.weight)
        with g.optimal_brain_compressing(dmx.DmxModuleGPTQHyperparams(microblock_size=64, block_size=64)):
            g(torch.randn(2, 40, 128, device=cuda))
        assert g.obc is None and bool(torch.isfinite(g.weight).all()) and bits_equal(g.weight.detach(), m.weight.detach()) != 0
        g(x)
    dmx.nn.fold_weights_and_biases(m)
    assert bits_equal(m.weight.detach(), want) == 0
    with torch.no_grad():
        assert bits_equal(m(x), y) == 0


def test_format_sweep_with_rotations(dmx, cuda):
    x = make("outlier", (64, 512), seed=83, dtype=BF16, block=256).to(cuda)
    fmts = ["BFP[8|8]{16}(SN)", "MXFP4[E2M1]{32}", ("XP[8,0](CSN)", 0.04, 0)]
    got = dmx.format_sweep(x, fmts, hadamard=[None, 64])
    plain = dmx.format_sweep(x, fmts)
    assert list(got) == ["BFP[8|8]{16}(SN)", "MXFP4[E2M1]{32}", "XP[8,0](CSN)", "BFP[8|8]{16}(SN) @H64", "MXFP4[E2M1]{32} @H64", "XP[8,0](CSN) @H64"]
    from dmx_compressor_amd.benchmark import sqnr_db_of
    for k, v in plain.items():
        assert got[k] == v
    for entry in fmts:
        f, sc, zp = entry if isinstance(entry, tuple) else (entry, None, None)
        y = dmx.ops.hadamard_qdq(x, 64, f, scale=sc, zero_point=zp)
        assert got[f"{f} @H64"] == float(sqnr_db_of(dmx.ops.error_stats(x, y)).cpu())
    assert list(dmx.format_sweep(x, fmts[:1], hadamard=128)) == ["BFP[8|8]{16}(SN) @H128"]
