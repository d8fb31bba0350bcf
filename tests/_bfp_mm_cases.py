"""Case table of the BFP matmul kernels (csrc/bfp_matmul.hip, csrc/bfp_bmm.hip) and the geometry that goes with it, stated as data:
tests/test_bfp_mm_cases_host.py proves without a GPU that the table covers every accumulator slot, edge, block count, store path, output
dtype and precision pair of every class, and tests/test_gpu_bfp_mm_classes.py runs the kernels on it.  Also here: the hand-built
operands of the exponent-range test and the cases with an offset past 2^31.  Nothing here needs a GPU to be imported.

The 15 classes: mfma_b{32,64,128} (2-D) and {nk,kn}_b{32,64,128}_n{64,128} (batched; the 64-wide tile serves N <= 64).

Geometry, written from the comments of the two kernels.  A workgroup of 4 waves of 64 lanes owns a tile of 128 rows x TN columns.
TN = 128: the waves sit 2 x 2 (wave w at (w >> 1, w & 1)) and own 64 x 64 each = MT x 4 = 4 x 4 MFMA tiles of 16 x 16; TN = 64: the
waves sit 4 x 1 and own 32 x 64 each = 2 x 4 MFMA tiles.  In MFMA tile (mt, nt) lane l holds row l % 16 and the four columns
4 (l / 16) + i, i = 0 .. 3.  An accumulator slot is (wave, mt, nt, lane, i)."""
from collections import namedtuple

import numpy as np
import torch

from _data import splitmix64

BLOCKS = (32, 64, 128)
LAYOUTS = ("nk", "kn")
TILE_M = 128
OUTS = ("f32", "bf16", "f16")
PAIRS = ((8, 8), (8, 4), (4, 4), (2, 2), (3, 5), (8, 2), (5, 8))   # (pa, pw) every one of which some case runs
CLASSES = tuple(f"mfma_b{B}" for B in BLOCKS) + tuple(f"{l}_b{B}_n{tn}" for l in LAYOUTS for B in BLOCKS for tn in (128, 64))

Geometry = namedtuple("Geometry", "tile waves rows_per_wave MT NT")
GEOMETRY = {c: (Geometry((TILE_M, 64), (4, 1), 32, 2, 4) if c.endswith("_n64") else Geometry((TILE_M, 128), (2, 2), 64, 4, 4)) for c in CLASSES}


def wave_pos(g, wave):
    """(wm, wn) of a wave in the wave grid"""
    return (wave >> 1, wave & 1) if g.waves == (2, 2) else (wave, 0)


def slot_rc(g, wave, mt, nt, lane, i):
    """(row, column) inside the workgroup's tile of accumulator slot (wave, mt, nt, lane, i)"""
    wm, wn = wave_pos(g, wave)
    return wm * g.MT * 16 + mt * 16 + lane % 16, wn * 64 + nt * 16 + 4 * (lane // 16) + i


def slot_count(g):
    return 4 * g.MT * g.NT * 64 * 4


# cls: the class; op "mm" | "bmm"; layout None | "nk" | "kn"; batch 0 for the 2-D op; outs: the output dtypes the case runs;
# all_slots: the case that stores from every accumulator slot
Case = namedtuple("Case", "cls op layout B batch M N nb pa pw outs all_slots")


def _cases():
    out, k = [], 0

    def add(cls, op, layout, B, batch, M, N, nb, all_slots=False):
        nonlocal k
        pa, pw = (8, 8) if all_slots else PAIRS[k % len(PAIRS)]     # (the all-slots case: B 2^(2p-2) = 2^21 in the exact test)
        k += not all_slots
        out.append(Case(cls, op, layout, B, batch, M, N, nb, pa, pw, OUTS if all_slots else ("f32",), all_slots))

    for B in BLOCKS:
        c = f"mfma_b{B}"
        add(c, "mm", None, B, 0, 130, 132, 2, True)      # every slot; a ragged second tile along M and along N; 16-byte stores
        add(c, "mm", None, B, 0, 130, 133, 3)            # N odd: element stores
        add(c, "mm", None, B, 0, 17, 33, 1)              # one step (B = 128: two from one block): the double buffer never flips
    for layout in LAYOUTS:
        odd = layout == "nk"                             # ("kn" takes N % 4 == 0 only)
        for B in BLOCKS:
            c = f"{layout}_b{B}_n128"
            add(c, "bmm", layout, B, 2, 130, 132, 2, True)
            add(c, "bmm", layout, B, 3 if odd else 1, 130, 133 if odd else 124, 3)   # "kn": one tile, column groups clamped to N - 4
            add(c, "bmm", layout, B, 1 if odd else 2, 17, 68, 1)
            c = f"{layout}_b{B}_n64"
            add(c, "bmm", layout, B, 2, 130, 64, 2, True)     # M >= 128 and N = 64: waves 2 and 3 store; a ragged second M tile
            add(c, "bmm", layout, B, 2, 260, 36, 3)           # N < 64, a multiple of 4; three M tiles
            add(c, "bmm", layout, B, 1, 33, 37 if odd else 4, 1)
    return tuple(out)


CASES = _cases()


def case_id(c):
    return f"{c.cls}-{c.batch}x{c.M}x{c.N}x{c.nb}b-p{c.pa}{c.pw}"


def tile_n(c):
    return GEOMETRY[c.cls].tile[1]


def stored_slots(c):
    """bool [wave, mt, nt, lane, i]: the slots that store at least one element in some workgroup of the case"""
    g = GEOMETRY[c.cls]
    hit = np.zeros((4, g.MT, g.NT, 64, 4), dtype=bool)
    for wave in range(4):
        for mt in range(g.MT):
            for nt in range(g.NT):
                for lane in range(64):
                    for i in range(4):
                        r, col = slot_rc(g, wave, mt, nt, lane, i)
                        hit[wave, mt, nt, lane, i] = any(by + r < c.M for by in range(0, c.M, TILE_M)) and \
                            any(bx + col < c.N for bx in range(0, c.N, g.tile[1]))
    return hit


def int8_codes(shape, p, seed):
    """codes uniform over the FULL range of precision p, -2^(p-1) included (a function of the seed and the linear index only)"""
    n = int(np.prod(shape))
    r = splitmix64(np.arange(n, dtype=np.uint64), seed) >> np.uint64(20)
    return torch.from_numpy(((r % np.uint64(1 << p)).astype(np.int64) - (1 << (p - 1))).astype(np.int8)).reshape(shape)


def bytes_between(shape, lo, hi, seed):
    """exponent bytes uniform in lo .. hi"""
    n = int(np.prod(shape))
    r = splitmix64(np.arange(n, dtype=np.uint64), seed) >> np.uint64(20)
    return torch.from_numpy(((r % np.uint64(hi - lo + 1)).astype(np.int64) + lo).astype(np.uint8)).reshape(shape)


# ------------------------------------------------------------------------------------------------ the exponent-range operands
EXP_M, EXP_N, EXP_NB, EXP_P = 16, 8, 4, 8
# regions of the [16, 8] result, as (rows, columns)
EXP_NORMAL = (range(0, 4), range(0, 2))       # denormal A scales (bytes 1 .. 8) against bytes 200 .. 240: every term normal and exact
EXP_DENORMAL = (range(4, 8), range(2, 4))     # a normal first term near 2^-124, then products that need bits below 2^-149
EXP_BELOW = (range(8, 9), range(5, 6))        # every term wholly below 2^-149
EXP_POS_INF, EXP_NEG_INF, EXP_INF_NAN = (9, 6), (10, 6), (11, 6)   # the first multiply overflows: +Inf, -Inf, +Inf then -Inf
EXP_SECOND_OVERFLOW = (12, 7)                 # x sw >= 2^128 with acc = 0: +Inf on both routes
EXP_CANCELLED = (13, 7)                       # acc = -2^127, then x sw = 2^128: the fma gives 2^127, multiply-then-add +Inf
EXP_NAN_ROW, EXP_ZERO_ROW = 14, 15            # a byte 255; bytes 0 only


def exponent_range_operands(B):
    """hand-built (ca [16, 4 B], ea [16, 4], cw [8, 4 B], ew [8, 4]) at precision (8, 8): the scale of byte e is 2^(e - 133).
    With b = log2 B, codes all a against codes all w give P = B a w."""
    b = {32: 5, 64: 6, 128: 7}[B]
    K = EXP_NB * B
    ca, cw = int8_codes((EXP_M, K), 8, 11 + B), int8_codes((EXP_N, K), 8, 12 + B)
    ea = torch.empty((EXP_M, EXP_NB), dtype=torch.uint8)
    ew = torch.empty((EXP_N, EXP_NB), dtype=torch.uint8)
    ea[0:4] = bytes_between((4, EXP_NB), 1, 8, 13 + B)
    ew[0:2] = bytes_between((2, EXP_NB), 200, 240, 14 + B)
    ea[4:8] = torch.tensor([16, 1, 1, 1], dtype=torch.uint8)        # P 2^-140, about 2^-124; then P 2^-163: a few units of 2^-149
    ew[2:4] = torch.tensor([110, 102, 102, 102], dtype=torch.uint8)
    ew[4] = torch.tensor([110, 60, 60, 60], dtype=torch.uint8)      # blocks 1 .. 3 of every row lie below 2^-149
    ew[5] = 60
    ea[8] = 1                                                        # against column 5: P 2^-205
    ca[9], ca[10] = 100, -100
    ea[9] = ea[10] = torch.tensor([254, 127, 127, 127], dtype=torch.uint8)      # x = P 2^121 overflows
    ca[11, :B], ca[11, B:2 * B] = 100, -100
    ea[11] = torch.tensor([254, 254, 133, 133], dtype=torch.uint8)
    cw[6] = 100
    ew[6] = torch.tensor([254, 254, 127, 127], dtype=torch.uint8)
    ca[12] = 64
    ea[12] = torch.tensor([200, 127, 127, 127], dtype=torch.uint8)  # x = 2^(12 + b) 2^67 is finite; times 2^121 it is not
    cw[7] = 64
    ew[7] = torch.tensor([254, 254, 100, 100], dtype=torch.uint8)
    ca[13, :B], ca[13, B:2 * B] = -64, 64
    ea[13] = torch.tensor([127 - b, 128 - b, 0, 0], dtype=torch.uint8)   # t_0 = -2^(12 + b) 2^(-6 - b) 2^121 = -2^127, x_1 sw_1 = +2^128
    ea[14] = torch.tensor([255, 127, 127, 127], dtype=torch.uint8)
    ea[15] = 0
    return ca, ea, cw, ew


# ------------------------------------------------------------------------------------------------ offsets past 2^31
TWO31 = 1 << 31
MIN_TARGET = TWO31 + (1 << 20)
GIB = 1 << 30
MAX_PEAK = 24 * GIB
# name: the offset family; op "mm" | "bmm" | "pack"; dims: batch (0 for the 2-D op), M, N, K; out: the output dtype;
# target: the factors whose product is the largest value of the offset; cut: the dimension the slices are taken along, parts: how many;
# copies: the slices of the big operand are copies (a cut along a dimension that is not the leading one)
Large = namedtuple("Large", "name op layout B batch M N K out target cut parts copies")
LARGE = (
    Large("ra_K", "mm", None, 64, 0, 65600, 16, 32896, "f32", ("M", "K"), "M", 2, False),
    Large("rw_K", "mm", None, 128, 0, 16, 65600, 32896, "f32", ("N", "K"), "N", 2, False),
    Large("m_N_n", "mm", None, 64, 0, 65600, 32900, 64, "bf16", ("M", "N"), "M", 2, False),
    Large("bz_M_K", "bmm", "nk", 32, 520, 2050, 8, 2048, "f32", ("batch", "M", "K"), "batch", 2, False),
    Large("kn_row_N", "bmm", "kn", 64, 1, 16, 32772, 65664, "f32", ("K", "N"), "N", 2, True),
    Large("kn_bz_N_K", "bmm", "kn", 128, 520, 16, 2052, 2048, "f32", ("batch", "N", "K"), "batch", 2, False),
    Large("out0", "bmm", "kn", 32, 520, 2050, 2052, 32, "f16", ("batch", "M", "N"), "batch", 2, False),
    Large("pack_cols_e0", "pack", None, 64, 1, 0, 32776, 65664, "bf16", ("K", "N"), "K", 4, False),
)
LARGE_BY_NAME = {c.name: c for c in LARGE}
OUT_BYTES = {"f32": 4, "bf16": 2, "f16": 2}


def large_target(c):
    n = 1
    for d in c.target:
        n *= getattr(c, d)
    return n


def large_operands(c, cut=None):
    """element counts of (A codes, A exponents, W codes, W exponents, output) of the call, or of its slice when `cut` = (a, b) along
    c.cut; the column pack: (input, codes, exponents)"""
    d = dict(batch=max(c.batch, 1), M=c.M, N=c.N, K=c.K)
    if cut is not None:
        d[c.cut] = cut[1] - cut[0]
    nb = d["K"] // c.B
    if c.op == "pack":
        return d["batch"] * d["K"] * d["N"], d["batch"] * d["K"] * d["N"], d["batch"] * nb * d["N"]
    return (d["batch"] * d["M"] * d["K"], d["batch"] * d["M"] * nb, d["batch"] * d["N"] * d["K"], d["batch"] * d["N"] * nb,
            d["batch"] * d["M"] * d["N"])


def large_cuts(c):
    """[(a, b)] along c.cut: c.parts slices, at whole blocks of the column pack's K and whole column groups of a "kn" W"""
    n = getattr(c, c.cut)
    unit = c.B if c.op == "pack" else (4 if c.layout == "kn" and c.cut == "N" else 1)     # ("kn" takes N % 4 == 0)
    step = -(-n // c.parts // unit) * unit
    return [(a, min(a + step, n)) for a in range(0, n, step)]


def large_windows(c):
    """[(batch index or None, dim, a, b)]: 64 rows ("M") or columns ("N") of the output whose operand rows, columns or output elements
    straddle element 2^31 of the case's big tensor, and the last 64 (of the last batch element)"""
    bi, e = None, TWO31
    if c.name in ("ra_K", "m_N_n"):
        dim, idx = "M", e // (c.K if c.name == "ra_K" else c.N)
    elif c.name == "rw_K":
        dim, idx = "N", e // c.K
    elif c.name == "bz_M_K":
        bi, rem = divmod(e, c.M * c.K)
        dim, idx = "M", rem // c.K
    elif c.name == "kn_row_N":
        dim, idx = "N", e % c.N                      # (every column of W[K, N] crosses the boundary along K; this one holds element 2^31)
    elif c.name == "kn_bz_N_K":
        bi, rem = divmod(e, c.K * c.N)
        dim, idx = "N", rem % c.N
    elif c.name == "out0":
        bi, rem = divmod(e, c.M * c.N)
        dim, idx = "M", rem // c.N
    else:
        raise ValueError(c.name)
    n = getattr(c, dim)
    a = max(0, min(idx - 32, n - 64))
    return [(bi, dim, a, a + 64), (None if bi is None else c.batch - 1, dim, n - 64, n)]


def large_peak_bytes(c):
    """device memory the test of the case holds at once: the operands, the full output, one slice's operands (copies only) and output,
    and 1 GiB for the pieces in which inputs are generated, the chain's windows and the comparison.  The column pack's reference route
    transposes a slice: the slice in bf16, its codes twice, its exponents."""
    ob = OUT_BYTES[c.out]
    cut = max(large_cuts(c), key=lambda ab: ab[1] - ab[0])
    if c.op == "pack":
        x, codes, exps = large_operands(c)
        sx, sc, se = large_operands(c, cut)
        return x * ob + codes + exps + sx * ob + 2 * sc + 2 * se + GIB
    a, ea, w, ew, y = large_operands(c)
    sa, sea, sw, sew, sy = large_operands(c, cut)
    return a + ea + w + ew + y * ob + (sa + sea + sw + sew if c.copies else 0) + 2 * sy * ob + GIB
