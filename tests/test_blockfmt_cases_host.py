"""Host only: the case table of tests/_blockfmt_cases.py (SBFP and MXFP, csrc/blockfmt.hip).  The oracle equals the plain-torch
restatement of the reference's two `cast` methods on all of it; the table holds, for every format and input dtype, every block class
that dtype can express, a mixed wave for every class that leaves the ordinary path, and both kernels' geometries; and the constants of
the restated predicates are still the ones in the sources.  tests/test_gpu_blockfmt.py runs the same table on the device."""
import os
import re

import numpy as np
import pytest
import torch

import _blockfmt_cases as C
from _data import mismatches_nan_aware

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dmx-compressor_amd", "csrc")
KINDS = [(k, f) for k in ("mxfp", "sbfp") for f in C.FORMATS[k]]
IDS = [f"{k}-{'-'.join(str(int(v)) for v in f)}" for k, f in KINDS]


def src(name):
    return open(os.path.join(CSRC, name)).read()


def test_constants_of_the_restated_predicates_are_the_sources():
    b = src("blockfmt.hip")
    m = re.search(r"near_pow2 = !f\.exact_exponent && \(maxbits & 0x007FFFFFu\) > (0x[0-9A-Fa-f]+)u;", b)
    assert m and int(m.group(1), 16) == C.NEAR_POW2_MANT == 0x00800000 - 88 - 1
    m = re.search(r"const bool ok = f\.xdomain && !near_pow2 && se >= f\.bias && eb <= (\d+);", b)
    assert m and int(m.group(1)) == C.HUGE_EB
    assert re.search(r"fast = f\.clamp != 0 && recip_ok\(s\);", b)
    assert re.search(r"pow2 = \(sb & 0x007FFFFFu\) == 0u && \(sb >> 23\) >= 1u && \(sb >> 23\) <= 253u;", b)
    assert re.search(r"zero = u2f\(maxbits\) == 0\.0f;", b)
    m = re.search(r"if \(inner == 1 && L % B == 0 && pow2 && B >= EPL && B <= (\d+) \* EPL\)", b)
    assert m and int(m.group(1)) == C.ROWS_MAX_LANES
    assert re.search(r"constexpr int EPL = 16 / Elem<DTI>::bytes;", b)
    assert re.search(r"f\.xdomain = \(f\.fast\.usable && std::isfinite\(f\.fast\.max_val\) && f\.bias >= 1\) \? 1 : 0;", b)
    for name, kind in (("SbfpFmt", "sbfp"), ("MxfpFmt", "mxfp")):
        m = re.search(r"struct %s \{ static constexpr int kThreads = (\d+), kUnroll = (\d+)," % name, b)
        assert m and int(m.group(1)) * int(m.group(2)) == C.TILE_VECTORS[kind]
    m = re.search(r"bool recip_ok\(float d\) \{ return d >= ([0-9.e+-]+)f && d <= ([0-9.e+-]+)f; \}", src("common.hpp"))
    assert m and float(m.group(1)) == C.RECIP_LO and float(m.group(2)) == C.RECIP_HI
    fq = src("floatq.hpp")
    assert re.search(r"k\.usable = \(man >= 1 && man <= 20 && min_exp >= -126 && min_exp <= 100\) \? 1 : 0;", fq)
    assert re.search(r"k\.max_ok_bits = \(uint32_t\)\(103 \+ man \+ 127 > 254 \? 254 : 103 \+ man \+ 127\) << 23;", fq)
    mm = src("mxfp_math.hpp")
    # the rounding rule is stated ONCE (mxfp_log2_rounds_up) and asked by both the normal and the denormal branch of mxfp_block_scale
    ms = list(re.finditer(r"jmax = g <= 20 \? \(\((0x[0-9A-F]+)u >> \(8 \* \(g - 17\)\)\) & 0xFFu\) : \(g <= 23 \? \(\((0x[0-9A-F]+)u >> \(8 \* \(g - 21\)\)\) & 0xFFu\) : 0u\);", mm))
    assert len(ms) == 1 and len(re.findall(r"const uint32_t jmax\b", mm)) == 1 and len(re.findall(r"mxfp_log2_rounds_up\(v, ", mm)) == 2
    m = ms[0]
    assert re.search(r"const int g = \(v > 0 && \(a & \(a - 1u\)\) == 0u\) \? 25 - c : 24 - c;", mm)
    lo, hi = int(m.group(1), 16), int(m.group(2), 16)
    assert {g: ((lo >> (8 * (g - 17))) & 0xFF) if g <= 20 else ((hi >> (8 * (g - 21))) & 0xFF) for g in range(17, 24)} == C.JMAX


def test_geometry_restatement():
    bf, f32 = C.DTYPES["bf16"], C.DTYPES["f32"]
    assert (C.elements_per_wave(bf), C.elements_per_wave(C.DTYPES["f16"]), C.elements_per_wave(f32)) == (512, 512, 256)
    assert C.lanes_per_block(32, bf) == 4 and C.lanes_per_block(32, f32) == 8 and C.lanes_per_block(8, bf) == 1
    assert C.rows_path(1024, 1, 32, bf) and C.rows_path(1024, 1, 512, bf) and C.rows_path(512, 1, 256, f32)
    assert not C.rows_path(1024, 1, 1024, bf) and not C.rows_path(1024, 1, 4, bf) and not C.rows_path(1024, 1, 512, f32)
    assert not C.rows_path(1020, 1, 32, bf) and not C.rows_path(960, 1, 24, bf) and not C.rows_path(1024, 5, 32, bf)


def test_format_predicates():
    k = {f: C.mxfp_consts(f) for f in C.MXFP_FORMATS}
    assert [bool(k[f].xdomain) for f in C.MXFP_FORMATS] == [True] * 5 + [False] * 3
    assert [bool(k[f].usable) for f in C.MXFP_FORMATS] == [True] * 5 + [False, False, True]     # (2,1): usable, bias 0
    assert (k[C.MxfpFmt(3, 4)].bias, k[C.MxfpFmt(3, 4)].big_log2) == (7, 8) and k[C.MxfpFmt(2, 1)].bias == 0
    assert not C.mxfp_consts(C.MxfpFmt(3, 8)).xdomain                                          # exponent range of float32: no finite max_val
    one = np.array([0x3F800000], dtype=np.uint32)
    for f in C.MXFP_FORMATS:
        assert bool(C.mxfp_try_fast(one, f, False)[0]) == bool(k[f].xdomain)
    f = C.MxfpFmt(3, 4)
    edge = (k[f].bias + k[f].big_log2) << 23
    probe = np.array([edge, edge - 1, (C.HUGE_EB << 23) | 0x7FFFFF, (C.HUGE_EB + 1) << 23, 0x3F800000 - 88, 0x3F800000 - 89], dtype=np.uint32)
    assert list(C.mxfp_try_fast(probe, f, False)) == [True, False, True, False, True, True]
    assert list(C.mxfp_try_fast(probe, f, True)) == [True, False, False, False, False, True]
    assert list(C.mxfp_classify(probe, f, True)) == ["xdomain", "scale_below_bias", "near_pow2", "huge", "near_pow2", "xdomain"]
    # general path: a scale that is a normal power of two allows the branch-free element form, a denormal / Inf / NaN scale does not
    assert C.mxfp_general_subpath(edge - 1, f, False) == "fast" and C.mxfp_general_subpath(8 << 23, f, False) == "literal"
    assert C.mxfp_general_subpath((9 << 23), f, False) == "fast"
    assert C.mxfp_general_subpath(0, f, False) == "fast" and C.mxfp_general_subpath(0x00012345, f, True) == "literal"
    assert C.mxfp_general_subpath(0x7F800000, f, True) == "literal" and C.mxfp_general_subpath(0x7F7FFFFF, f, True) == "literal"
    assert C.mxfp_general_subpath(0x3F800000, C.MxfpFmt(0, 4), False) == "literal" and C.mxfp_general_subpath(0x3F800000, C.MxfpFmt(2, 1), False) == "fast"
    assert C.log2_rounds_up(0x40FFFFFF) and not C.log2_rounds_up(0x40FFFFFD) and not C.log2_rounds_up(0x3F7FFFFF)
    s = C.SbfpFmt(4, 4, 4, 7, True, True, True)
    mb = C.f32_bits(np.array([0x3F80, 0x4780, 0x1000, 0x7000, 0x3A00, 0x0001, 0, 0x7F80, 0x7FC0]), C.DTYPES["bf16"])
    assert list(C.sbfp_classify(mb, s)) == ["fast", "scaler_saturates", "scale_small", "scale_large", "scaler_flushes", "denormal_max", "zero", "inf", "nan"]
    assert list(C.sbfp_fast(mb, s)) == [True, True, False, False, True, False, False, False, False]
    assert not C.sbfp_fast(mb, C.SbfpFmt(8, 4, 4, 7, True, False, True)).any()


@pytest.mark.parametrize("kind,f", KINDS, ids=IDS)
def test_table_holds_every_class_every_mixed_wave_and_both_geometries(kind, f):
    names = C.MXFP_CLASSES if kind == "mxfp" else C.SBFP_CLASSES
    for dt in C.DTYPES.values():
        o = C.ordinary_class(kind, f)
        want = C.expressible(kind, f, dt)
        assert set(want) <= set(names) and o in want
        # what a dtype cannot express is known: float16 holds no float32 denormal, nothing from 2^105 up and nothing below 2^-24
        must = {"zero", "inf", "nan", o}
        if dt.name != "f16":
            must |= {"denormal_max"} | ({"huge"} if kind == "mxfp" else {"scale_small", "scale_large"})
        if kind == "mxfp" and dt.name == "f32":
            must.add("near_pow2")
        if kind == "mxfp" and dt.name != "f16" and C.mxfp_consts(f).bias >= 2:
            must.add("scale_below_bias")
        if kind == "sbfp" and f.exp < 8:
            must.add("scaler_flushes")
            if dt.name != "f16" or 65504.0 / ((1 << (f.p - 1)) - 1) >= 2.0 ** ((1 << (f.exp - 1)) + 1):   # (float16's largest scale)
                must.add("scaler_saturates")
        assert must <= set(want), (dt.name, must - set(want))
        for B in (32, 16):
            for t in (C.planted(kind, f, dt, B), C.uniform(kind, f, dt, B)):
                pat = t.x.view(dt.t_bits).numpy().view(dt.np_bits)
                cls = C.classify(kind, C.block_maxima(pat, dt, B), f, dt)
                for row, k, c, rep in t.plan:               # every planted block is of the class it was planted as
                    assert cls[row, k] == c, (dt.name, B, row, k, c, cls[row, k], hex(rep))
                assert set(t.rows_class) == set(want)
                assert C.rows_path(t.x.shape[1], 1, B, dt)
            p = C.planted(kind, f, dt, B)
            pat = p.x.view(dt.t_bits).numpy().view(dt.np_bits)
            cls = C.classify(kind, C.block_maxima(pat, dt, B), f, dt)
            planted_at = {(r, k) for r, k, _, _ in p.plan}
            for r in range(cls.shape[0]):                   # ... in a wave of otherwise ordinary blocks, at every position of a wave
                for k in range(cls.shape[1]):
                    assert (r, k) in planted_at or cls[r, k] == o, (dt.name, B, r, k, cls[r, k])
            for c in want:
                pos = {k % p.blocks_per_wave for r, k, cc, _ in p.plan if cc == c}
                assert pos == set(range(p.blocks_per_wave)), (dt.name, B, c)
            waves = C.wave_classes(kind, f, dt, p.x, B)
            for c in want:
                if c != o:
                    assert ("general", frozenset({o, c})) in waves, (dt.name, B, c)
            assert (o, frozenset({o})) in waves
            if kind == "mxfp":                              # both sub-branches of the general path, where the format has both
                sub = {C.mxfp_general_subpath(int(C.f32_bits(np.array([rep]), dt)[0]) & 0x7FFFFFFF, f, dt.name == "f32")
                       for _, _, c, rep in p.plan if c != "xdomain"}
                assert "literal" in sub and (("fast" in sub) == bool(C.mxfp_consts(f).usable)), (dt.name, sub)
        # inner > 1 (the generic kernel's strided blocks): whole table kept, more than one outer index, every class still there
        for inner, B in ((5, 32), (48, 16)):
            x3, rc = C.planted_inner(kind, f, dt, B, inner, 4)
            assert x3.shape[0] >= 2 and x3.shape[1:] == (4 * B, inner) and x3.numel() > 0 and set(rc) == set(want) and len(rc) == x3.shape[0] * inner
            back = C.rows_of(x3)
            cls = C.classify(kind, C.block_maxima(back.view(dt.t_bits).numpy().view(dt.np_bits), dt, B), f, dt)
            assert {c for row in cls for c in row} == set(want) and not C.rows_path(x3.shape[1], inner, B, dt)
        # generic-kernel geometries of the GPU test
        assert not C.rows_path(640, 1, 20, dt) and not C.rows_path(1000, 1, 32, dt) and not C.rows_path(64, 5, 32, dt)
        assert not C.rows_path(128 * C.epl(dt) * 2, 1, 128 * C.epl(dt), dt) and C.rows_path(64 * C.epl(dt) * 2, 1, 64 * C.epl(dt), dt)


@pytest.mark.parametrize("kind,f", KINDS, ids=IDS)
def test_oracle_equals_the_torch_restatement_on_the_whole_table(oracle, kind, f):
    n = 0
    for dt in C.DTYPES.values():
        for B in (32, 16):
            for t in (C.planted(kind, f, dt, B), C.uniform(kind, f, dt, B)):
                want = C.torch_ref(kind, oracle, t.x, f, B)
                got = C.ref(kind, oracle, t.x, f, B)
                bad = mismatches_nan_aware(got, want)
                assert bad == 0, (kind, f, dt.name, B, bad)
                n += t.x.numel()
    assert n > 1_000_000


def test_oracle_equals_the_torch_restatement_on_float32_denormal_maxima(oracle):
    """denormal maxima at and just below every power of two: the oracle's floor(log2) (the C library's log2f) is torch.log2's there,
    and the table holds maxima on both sides of the rounding (k = 2^23 - t rounds up to -126 for t <= 22)"""
    x, ks = C.float32_denormal_blocks()
    m = torch.tensor(ks, dtype=torch.int32).view(torch.float32)
    fl = torch.floor(torch.log2(m)).to(torch.int64)
    exact = torch.tensor([k.bit_length() - 150 for k in ks])
    up = [(1 << 23) - k for k, a, b in zip(ks, fl.tolist(), exact.tolist()) if a != b and k > (1 << 22)]
    assert sorted(up) == list(range(1, 23)) and int((fl != exact).sum()) > 22
    for f in C.MXFP_FORMATS:
        assert mismatches_nan_aware(C.mxfp_ref(oracle, x, f, 32), C.torch_mxfp(oracle, x, f, 32)) == 0, f


def test_x_domain_form_one_exponent_below_its_bound_equals_the_general_path(oracle):
    """Why no test pins try_fast's `se >= bias` against `se >= bias - 1`: at se == bias - 1 the threshold exponent is 0, and the element
    format's first normal binade shares its quantum with the subnormal range, so apply_vec_fast (emulated here in numpy float32, every
    operation rounded; blockfmt.hip:111-125) gives the oracle's bits on every bfloat16 pattern under such a maximum.  The bound is
    where the threshold exponent would turn negative, and the form is still right AT it."""
    def u2f(b):
        return (b & 0xFFFFFFFF).astype(np.uint32).view(np.float32)

    bf = C.DTYPES["bf16"]
    for f in C.MXFP_FORMATS[:5]:
        k = C.mxfp_consts(f)
        eb = k.bias + k.big_log2 - 1
        blocks = np.concatenate([C.pattern_blocks((eb << 7) | man, bf) for man in (0, 0x35, 0x7F)])
        x = C.from_bits(blocks, bf).float()
        xb = x.view(torch.int32).numpy().astype(np.int64) & 0xFFFFFFFF
        se = eb - k.big_log2
        assert se == k.bias - 1
        tb = (se - (k.bias - 1)) << 23                                                   # :111
        k1 = ((23 - f.man) << 23) | 0x00400000                                           # floatq.hpp:37
        maxv = u2f(np.array((((k.big_log2 + 127) << 23) | ((0x007FFFFF >> (23 - f.man)) << (23 - f.man))) + ((se - 127) << 23)))   # :113
        sign, ebx = xb & 0x80000000, xb & 0x7F800000
        with np.errstate(all="ignore"):
            M = u2f(np.maximum(ebx, tb) + k1 + sign)                                     # :121-122
            S = u2f(np.where(ebx < tb, tb | sign, sign))                                 # :123
            q = ((x.numpy() + S).astype(np.float32) + M).astype(np.float32) - (M + S).astype(np.float32)   # :124
            got = np.minimum(np.maximum(q, -maxv), maxv).astype(np.float32)              # :125
        want = C.mxfp_ref(oracle, x, f, 32).numpy()
        assert int((got.view(np.uint32) != want.view(np.uint32)).sum()) == 0, f


def test_pattern_maxima_are_what_they_are_meant_to_be():
    bf, f16 = C.DTYPES["bf16"], C.DTYPES["f16"]
    f = C.MxfpFmt(3, 4)
    m = C.mxfp_pattern_maxima(f, bf)
    cls = list(C.mxfp_classify(C.f32_bits(np.array(m), bf), f, False))
    assert cls == ["xdomain", "xdomain", "xdomain", "scale_below_bias", "xdomain", "huge", "huge", "denormal_max"], cls
    assert set(C.mxfp_classify(C.f32_bits(np.array(C.mxfp_pattern_maxima(f, f16)), f16), f, False)) == {"xdomain"}
    blocks = C.pattern_blocks(m[0], bf)
    assert blocks.shape[1] == 32 and set(np.unique(blocks & 0x7FFF)) == set(range(m[0] + 1)) and int((blocks >> 15).sum()) >= m[0] + 1
    nf = C.nonfinite_blocks(bf)
    assert set(np.unique(nf)) == set(range(0x7F80, 0x8000)) | set(range(0xFF80, 0x10000))
    for s in C.SBFP_FORMATS:
        for dt in (bf, f16):
            mx = C.sbfp_pattern_maxima(s, dt)
            fast = C.sbfp_fast(C.f32_bits(np.array(mx), dt), s)
            if s.clamp and dt is bf:
                assert fast.any() and not fast.all(), (s, mx)
            pat, mb = C.candidates(dt)
            for m_ in mx:                                   # an edge maximum has a neighbour pattern on the other side of recip_ok
                if m_ in (C.native_of(float((1 << (s.p - 1)) - 1), dt), C.native_of(float((1 << (s.p - 1)) - 1) / 8, dt)):
                    continue
                a = C.sbfp_scale(mb[[m_ - 1, m_, m_ + 1]], s).astype(np.float64)
                inside = (a >= C.RECIP_LO) & (a <= C.RECIP_HI)
                assert inside.any() and not inside.all(), (s, dt.name, hex(m_))
    s = C.SbfpFmt(8, 2, 5, 15, True, True, True)
    assert C.native_of(127.0, bf) in C.sbfp_pattern_maxima(s, bf) and float(C.sbfp_scale(C.f32_bits(np.array([C.native_of(127.0, bf)]), bf), s)[0]) == 1.0
