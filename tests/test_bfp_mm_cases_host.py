"""tests/_bfp_mm_cases.py and tests/_bfp_mm_ref.py without a GPU: the case table provably covers the geometry of every BFP matmul class
(every accumulator slot stores, every edge, block count, store path, output dtype and precision pair runs, and the library names the
class the table claims), the exact reference agrees with the chain on the CPU wherever the terms stay in fp32's normal range, and the
planted under / overflow operands reach the regime in which DESIGN.md §8 lets the two routes differ."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import _bfp_mm_cases as MC
import _bfp_mm_ref as R
import _large_cases as LC

BY_CLASS = {c: [k for k in MC.CASES if k.cls == c] for c in MC.CLASSES}


def test_the_table_names_the_fifteen_classes():
    assert len(MC.CLASSES) == 15 == len(set(MC.CLASSES)) and all(BY_CLASS[c] for c in MC.CLASSES)
    assert len({MC.case_id(c) for c in MC.CASES}) == len(MC.CASES)
    for g in MC.GEOMETRY.values():
        assert g.waves[0] * g.rows_per_wave == g.tile[0] == MC.TILE_M and g.waves[1] * 64 == g.tile[1]
        assert g.MT * 16 == g.rows_per_wave and g.NT * 16 == 64 and g.waves[0] * g.waves[1] == 4
        cells = {MC.slot_rc(g, w, mt, nt, l, i) for w in range(4) for mt in range(g.MT) for nt in range(g.NT) for l in range(64) for i in range(4)}
        assert len(cells) == MC.slot_count(g) == g.tile[0] * g.tile[1]      # the slot map is a bijection onto the tile


@pytest.mark.parametrize("cls", MC.CLASSES)
def test_class_is_covered(cls):
    cases, g = BY_CLASS[cls], MC.GEOMETRY[cls]
    tn, odd_ok = g.tile[1], not cls.startswith("kn")
    hit = np.zeros((4, g.MT, g.NT, 64, 4), dtype=bool)
    for c in cases:
        hit |= MC.stored_slots(c)
    assert int(hit.sum()) == MC.slot_count(g) == 4 * g.MT * 4 * 64 * 4
    full = [c for c in cases if c.all_slots]
    assert len(full) == 1 and bool(MC.stored_slots(full[0]).all()) and full[0].M >= 128 and full[0].N >= tn
    assert set(full[0].outs) == set(MC.OUTS) and full[0].nb <= 8 and (full[0].pa, full[0].pw) == (8, 8)
    assert any(c.M % MC.TILE_M and c.M > MC.TILE_M for c in cases)                        # M ragged with blockIdx.y > 0
    if tn == 128:
        assert any(c.N % 128 and c.N > 128 for c in cases)                                # a ragged second N tile
        if cls.startswith("kn"):
            assert {c.N for c in cases if 64 < c.N < 128} >= {68, 124}
        assert cls.startswith("mfma") or all(c.N > 64 for c in cases)                     # (the 2-D op has the one tile width)
    else:
        assert any(c.N < 64 and c.N % 4 == 0 for c in cases) and all(c.N <= 64 for c in cases)
        assert not odd_ok or any(c.N < 64 and c.N % 4 for c in cases)
    nbs = {c.nb for c in cases}
    assert {1, 2} <= nbs and any(n >= 3 and n % 2 for n in nbs)
    assert any(c.N % 4 == 0 for c in cases) and (not odd_ok or any(c.N % 2 for c in cases))
    assert all(c.N % 4 == 0 for c in cases) or odd_ok
    if cls.startswith("mfma"):
        assert all(c.op == "mm" and c.batch == 0 for c in cases)
    else:
        assert any(c.batch >= 2 for c in cases) and any(c.batch == 1 for c in cases)


def test_precision_pairs_across_the_table():
    pairs = {(c.pa, c.pw) for c in MC.CASES}
    assert pairs >= {(8, 8), (8, 4), (4, 4), (2, 2), (3, 5), (8, 2), (5, 8)}
    assert (4, 4) in {(c.pa, c.pw) for c in MC.CASES if c.op == "bmm"}
    for p in range(2, 9):
        lo, hi = R.code_range(p)
        codes = MC.int8_codes((4096,), p, p)
        assert int(codes.min()) == lo == -(1 << (p - 1)) and int(codes.max()) == hi


@pytest.mark.parametrize("c", MC.CASES, ids=MC.case_id)
def test_the_library_names_the_class(dmx, c):
    K = c.nb * c.B
    if c.op == "mm":
        got = dmx.ops.bfp_matmul_class(torch.empty(c.M, K, dtype=torch.int8), torch.empty(c.N, K, dtype=torch.int8), c.B)
    else:
        w = torch.empty((c.batch, K, c.N) if c.layout == "kn" else (c.batch, c.N, K), dtype=torch.int8)
        got = dmx.ops.bfp_bmm_class(torch.empty(c.batch, c.M, K, dtype=torch.int8), w, c.B, c.layout)
    assert got == c.cls


# ------------------------------------------------------------------------------------------------ the exact reference
def test_round_f32_on_integers():
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float64).to(torch.float32))
    for num, den in ((1, 3), (-2, 3), (16777217, 1), (16777219, 1), (33554434, 1), (1, 1 << 140), (3, 1 << 150), (1, 1 << 150),
                     (-1, 1 << 151), ((1 << 24) - 1, 1), (5, 1 << 151)):
        assert R.round_f32(Fraction(num, den)) == f32(num / den), (num, den)      # (every quotient here is exact in float64 or far from a tie)
    assert R.round_f32(Fraction(3, 1 << 150)) == 2.0 ** -148                      # a tie in the denormal range goes to even
    top = (1 << 128) - (1 << 104)
    assert R.round_f32(top) == float(top) and R.round_f32(top + (1 << 103) - 1) == float(top) and R.round_f32(top + (1 << 103)) == math.inf
    assert R.round_f32(-(1 << 128)) == -math.inf
    z = R.round_f32(Fraction(-1, 1 << 151))
    assert z == 0.0 and math.copysign(1.0, z) == -1.0
    assert R.fma_f32(2.0 ** 64, 2.0 ** 64, -2.0 ** 127) == 2.0 ** 127 and R.add_f32(R.mul_f32(2.0 ** 64, 2.0 ** 64), -2.0 ** 127) == math.inf
    assert math.isnan(R.add_f32(math.inf, -math.inf)) and math.isnan(R.mul_f32(0.0, math.inf)) and math.isnan(R.fma_f32(math.inf, 1.0, -math.inf))
    assert math.copysign(1.0, R.add_f32(-0.0, -0.0)) == -1.0 and math.copysign(1.0, R.add_f32(0.0, -0.0)) == 1.0
    assert R.scale_of(0, 8) == 0.0 and math.isnan(R.scale_of(255, 4)) and R.scale_of(1, 8) == 2.0 ** -132 and R.scale_of(254, 2) == 2.0 ** 127


@pytest.mark.parametrize("pa,pw", ((8, 8), (8, 4), (2, 2), (3, 5)))
@pytest.mark.parametrize("B", MC.BLOCKS)
def test_both_semantics_equal_the_chain_in_the_normal_range(dmx, B, pa, pw):
    """random hand-built operands, bytes 100 .. 150: |t_j| in 2^-71 .. 2^62, every term exact -- the two forms and the library's chain
    (run on CPU tensors) agree bit for bit; bytes 0 and 255 planted"""
    M, N, nb = 6, 5, 3
    ca, cw = MC.int8_codes((M, nb * B), pa, B + pa), MC.int8_codes((N, nb * B), pw, B + pw + 1)
    ea, ew = MC.bytes_between((M, nb), 100, 150, B + 2), MC.bytes_between((N, nb), 100, 150, B + 3)
    ea[1, 1], ew[2, 0], ea[4, 2] = 0, 0, 255
    for out_dtype in (torch.float32, torch.bfloat16, torch.float16):
        k = R.kernel_semantics(ca, ea, cw, ew, pa, pw, B, out_dtype)
        c = R.chain_semantics(ca, ea, cw, ew, pa, pw, B, out_dtype)
        lib = dmx._front._bfp_matmul_chain(ca, ea, cw, ew, pa, pw, B, out_dtype)
        assert k.dtype == out_dtype and LC.mismatches_on_device(k, c) == 0 and LC.mismatches_on_device(k, lib) == 0
    assert bool(torch.isnan(k[4]).all()) and not bool(torch.isnan(k[:4]).any())
    # and the exact terms sum to the float64 product of the definition's operands
    t = R.exact_terms(ca, ea, cw, ew, pa, pw, B)
    assert t[4][0][2] is None and t[1][0][1] == 0 and t[0][2][0] == 0
    P = R.block_sums(ca, cw, B)
    assert t[0][0][1] == Fraction(int(P[0, 0, 1])) * Fraction(2) ** (int(ea[0, 1]) + int(ew[0, 1]) - 254 - (pa - 2) - (pw - 2))


def _differs(a, b, rows, cols):
    return [(m, n) for m in rows for n in cols if LC.mismatches_on_device(a[m, n].reshape(1), b[m, n].reshape(1))]


@pytest.mark.parametrize("B", MC.BLOCKS)
def test_planted_operands_reach_the_regime_where_the_routes_may_differ(B):
    ca, ea, cw, ew = MC.exponent_range_operands(B)
    assert ca.shape == (MC.EXP_M, MC.EXP_NB * B) and ew.shape == (MC.EXP_N, MC.EXP_NB)
    k = R.kernel_semantics(ca, ea, cw, ew, 8, 8, B)
    c = R.chain_semantics(ca, ea, cw, ew, 8, 8, B)
    t = R.exact_terms(ca, ea, cw, ew, 8, 8, B)
    # denormal scales, normal terms: route-independent, and inside the bound of the exact sum
    rows, cols = MC.EXP_NORMAL
    assert not _differs(k, c, rows, cols) and int(ea[0:4].max()) <= 8 and int(ea[0:4].min()) >= 1
    for m in rows:
        for n in cols:
            assert all(x == 0 or 2.0 ** -126 <= abs(x) < 2.0 ** 128 for x in t[m][n])
            bound = (MC.EXP_NB - 1) * Fraction(1, 1 << 24) * sum(abs(x) for x in t[m][n]) * (1 + Fraction(1, 1 << 20))
            assert abs(Fraction(float(k[m, n])) - sum(t[m][n])) <= bound
    # a denormal product that needs bits below 2^-149: one rounding and two roundings part on at least one planted element
    rows, cols = MC.EXP_DENORMAL
    assert _differs(k, c, rows, cols)
    for m, n in _differs(k, c, rows, cols):
        assert all(abs(t[m][n][j]) < 2.0 ** -126 for j in (1, 2, 3)) and any((t[m][n][j] * (1 << 149)).denominator > 1 for j in (1, 2, 3))
    # wholly below 2^-149
    (m,), (n,) = MC.EXP_BELOW
    assert all(abs(x) < Fraction(1, 1 << 150) for x in t[m][n]) and float(k[m, n]) == 0.0 == float(c[m, n])
    # the first multiply overflows
    for (m, n), want in ((MC.EXP_POS_INF, math.inf), (MC.EXP_NEG_INF, -math.inf)):
        assert float(k[m, n]) == want == float(c[m, n])
    m, n = MC.EXP_INF_NAN
    assert math.isnan(float(k[m, n])) and math.isnan(float(c[m, n]))
    m, n = MC.EXP_SECOND_OVERFLOW
    assert float(k[m, n]) == math.inf == float(c[m, n]) and abs(float(R.block_sums(ca, cw, B)[m, n, 0])) * 2.0 ** 67 < 2.0 ** 128
    # x sw = 2^128 cancelled by acc = -2^127
    m, n = MC.EXP_CANCELLED
    assert t[m][n][:2] == [-(1 << 127), 1 << 128] and float(k[m, n]) == 2.0 ** 127 and float(c[m, n]) == math.inf
    assert bool(torch.isnan(k[MC.EXP_NAN_ROW]).all()) and bool((k[MC.EXP_ZERO_ROW] == 0).all()) and bool((c[MC.EXP_ZERO_ROW] == 0).all())
    # the 16-bit converts of the same values: 2^127 overflows float16, the denormal sums flush
    h = R.kernel_semantics(ca, ea, cw, ew, 8, 8, B, torch.float16)
    assert float(h[MC.EXP_CANCELLED]) == math.inf and all(float(h[m, n]) == 0.0 for m in MC.EXP_DENORMAL[0] for n in MC.EXP_DENORMAL[1])


# ------------------------------------------------------------------------------------------------ offsets past 2^31
def test_int64_kernels_are_listed():
    assert {"bfp_matmul.hip", "bfp_bmm.hip", "bfp_pack.hip:cols"} <= set(LC.INT64_KERNELS)


@pytest.mark.parametrize("c", MC.LARGE, ids=lambda c: c.name)
def test_large_case_crosses_the_boundary_and_its_slices_do_not(c):
    assert MC.large_target(c) > MC.MIN_TARGET == (1 << 31) + (1 << 20)
    assert MC.large_target(c) == max(MC.large_operands(c))                 # the target IS the case's largest operand
    assert sum(n > MC.TWO31 for n in MC.large_operands(c)) == (2 if c.op == "pack" else 1)     # (the pack: its input and its codes)
    cuts = MC.large_cuts(c)
    assert cuts[0][0] == 0 and cuts[-1][1] == getattr(c, c.cut) and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))
    for cut in cuts:
        assert all(n < MC.TWO31 for n in MC.large_operands(c, cut)), (c.name, cut)
        assert c.op != "pack" or (cut[0] % c.B == 0 and (cut[1] - cut[0]) % c.B == 0)
        assert not (c.layout == "kn" and c.cut == "N") or (cut[0] % 4 == 0 and (cut[1] - cut[0]) % 4 == 0)
    assert MC.large_peak_bytes(c) < MC.MAX_PEAK
    assert c.K % c.B == 0 and (c.layout != "kn" or c.N % 4 == 0)
    # the period rule of tests/_large_cases.py for the multiplier of the leading index: it divides neither 2^31 nor 2^32
    period = MC.large_target(c) // getattr(c, c.target[0])
    assert MC.TWO31 % period and (1 << 32) % period
    if c.op != "pack":
        (bi, dim, a, b), (bl, dl, al, bl_end) = MC.large_windows(c)
        n = getattr(c, dim)
        assert 0 <= a < b <= n and b - a == 64 and (al, bl_end) == (n - 64, n) and dl == dim
        # the first window holds the row / column / output row of element 2^31 of the big tensor
        first = {"ra_K": a * c.K, "rw_K": a * c.K, "m_N_n": a * c.N, "bz_M_K": (bi or 0) * c.M * c.K + a * c.K,
                 "kn_row_N": (MC.TWO31 // c.N) * c.N + a, "kn_bz_N_K": MC.TWO31 // c.N * c.N + a, "out0": (bi or 0) * c.M * c.N + a * c.N}[c.name]
        width = {"ra_K": 64 * c.K, "rw_K": 64 * c.K, "m_N_n": 64 * c.N, "bz_M_K": 64 * c.K, "kn_row_N": 64, "kn_bz_N_K": 64, "out0": 64 * c.N}[c.name]
        assert first <= MC.TWO31 < first + width and (bi is None or 0 < bi < c.batch - 1)
