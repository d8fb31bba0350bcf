"""Case table of the composite block formats (csrc/blockfmt.hip: dmxq_sbfp_qdq, dmxq_mxfp_qdq): a restatement, in plain Python, of the
predicates by which the kernels choose a path for a block, a wave and a tensor; the classes of block maxima those predicates separate;
builders that plant a block of every class at every position of a wave; and the two references (the oracle, and a plain-torch
restatement of the reference's two `cast` methods beside it).  Imported by tests/test_blockfmt_cases_host.py (host only: the table
holds every class, the oracle equals the torch restatement on all of it, the constants below are still the sources'),
tests/test_gpu_blockfmt.py, tests/test_golden.py and oracle/gen_golden_blockfmt.py.

A block CLASS is a function of (bit pattern of the block's max|x| as float32, format, input dtype).  The kernels decide per WAVE:
a wave is `xdomain` (MXFP) only when every one of its blocks is; SBFP decides per lane, so a block there is `fast` on its own.

Nothing here needs a GPU; every input is a function of (format, dtype, geometry) through the counter generator of tests/_data.py."""
from collections import namedtuple

import numpy as np
import torch

from _data import make, splitmix64

# ------------------------------------------------------------------------------------------------ dtypes
Dt = namedtuple("Dt", "name torch np_bits t_bits mant inf itemsize")
DTYPES = {
    "bf16": Dt("bf16", torch.bfloat16, np.uint16, torch.int16, 7, 0x7F80, 2),
    "f16": Dt("f16", torch.float16, np.uint16, torch.int16, 10, 0x7C00, 2),
    "f32": Dt("f32", torch.float32, np.uint32, torch.int32, 23, 0x7F800000, 4),
}
BY_TORCH = {d.torch: d for d in DTYPES.values()}


def from_bits(pat, dt):
    """native bit patterns (numpy unsigned) -> tensor of dt"""
    a = np.ascontiguousarray(pat.astype(dt.np_bits))
    return torch.from_numpy(a.view(np.int16 if dt.itemsize == 2 else np.int32)).view(dt.torch)


def f32_bits(pat, dt):
    """native bit patterns -> the float32 bit patterns the kernels see after load1 (numpy uint32)"""
    return from_bits(pat, dt).float().contiguous().view(torch.int32).numpy().view(np.uint32).copy()


# ------------------------------------------------------------------------------------------------ constants of the sources
# (tests/test_blockfmt_cases_host.py reads each back from the file and line named, so an edit there fails the host suite)
NEAR_POW2_MANT = 0x007FFFA7   # blockfmt.hip:108 try_fast: float32 maxima with a mantissa above this (88 ulps below a power of two)
HUGE_EB = 231                 # blockfmt.hip:109 try_fast: eb <= 231 (maxima below 2^105)
RECIP_LO, RECIP_HI = 2.0 ** -20, 2.0 ** 20   # common.hpp:412 recip_ok
ROWS_MAX_LANES = 64           # blockfmt.hip:212 launch_blockfmt: B <= 64 * EPL
JMAX = {17: 88, 18: 44, 19: 22, 20: 11, 21: 5, 22: 2, 23: 1}   # mxfp_math.hpp:29 mxfp_log2_rounds_up (g -> jmax; 0 above)
TILE_VECTORS = {"mxfp": 256 * 8, "sbfp": 128 * 8}   # blockfmt.hip:28-29 kThreads * kUnroll


# ------------------------------------------------------------------------------------------------ geometry
def epl(dt):
    """blockfmt.hip:209 EPL: elements of one 16-byte vector"""
    return 16 // dt.itemsize


def elements_per_wave(dt):
    """64 lanes x one vector: 512 sixteen-bit, 256 float32"""
    return 64 * epl(dt)


def lanes_per_block(B, dt):
    """blockfmt.hip:213 lpb = B / EPL"""
    return B // epl(dt)


def rows_path(L, inner, B, dt):
    """blockfmt.hip:211-212 launch_blockfmt: the streaming rows path, else the generic kernel"""
    pow2 = B & (B - 1) == 0
    return inner == 1 and L % B == 0 and pow2 and B >= epl(dt) and B <= ROWS_MAX_LANES * epl(dt)


# ------------------------------------------------------------------------------------------------ MXFP
MxfpFmt = namedtuple("MxfpFmt", "man exp")
MxfpK = namedtuple("MxfpK", "bias big_log2 usable xdomain max_ok_field")
MXFP_FORMATS = [MxfpFmt(3, 4), MxfpFmt(2, 5), MxfpFmt(1, 2), MxfpFmt(2, 3), MxfpFmt(3, 2),
                MxfpFmt(0, 4), MxfpFmt(21, 5), MxfpFmt(2, 1)]   # the last three: never x-domain
MXFP_CLASSES = ("xdomain", "general_fast", "general_literal", "zero", "denormal_max", "scale_below_bias", "huge", "inf", "nan", "near_pow2")


def mxfp_consts(f):
    big_log2 = 1 << (f.exp - 1)            # mxfp_math.hpp:18
    bias = big_log2 - 1                    # mxfp_math.hpp:19
    min_exp = -(bias - 1)                  # floatq.hpp:33
    usable = 1 <= f.man <= 20 and -126 <= min_exp <= 100    # floatq.hpp:35 make_float_fast().usable
    finite_max = big_log2 + 127 < 255      # floatq.hpp:39-41 max_val finite
    xdomain = usable and finite_max and bias >= 1           # blockfmt.hip:266 f.xdomain
    return MxfpK(bias, big_log2, usable, xdomain, min(254, 103 + f.man + 127))   # floatq.hpp:38 max_ok_bits >> 23


def mxfp_try_fast(mb, f, f32_input):
    """blockfmt.hip:106-110 try_fast's per-block condition (the wave takes the x-domain path iff it holds for all its blocks)"""
    k = mxfp_consts(f)
    mb = np.asarray(mb, dtype=np.uint32)
    eb = (mb >> 23).astype(np.int64)
    se = eb - k.big_log2
    near_pow2 = np.logical_and(f32_input, (mb & 0x007FFFFF) > NEAR_POW2_MANT)     # :108 (exact_exponent = 16-bit input, :265)
    return np.logical_and.reduce([np.full(mb.shape, bool(k.xdomain)), ~near_pow2, se >= k.bias, eb <= HUGE_EB])   # :109


def mxfp_classify(mb, f, f32_input):
    """class NAME of each block maximum (float32 bit patterns)"""
    k = mxfp_consts(f)
    mb = np.asarray(mb, dtype=np.uint32)
    eb = (mb >> 23).astype(np.int64)
    ordinary = "xdomain" if k.xdomain else ("general_fast" if k.usable else "general_literal")
    out = np.full(mb.shape, ordinary, dtype=object)
    if f32_input:
        out[(mb & 0x007FFFFF) > NEAR_POW2_MANT] = "near_pow2"
    out[eb - k.big_log2 < k.bias] = "scale_below_bias"
    out[eb > HUGE_EB] = "huge"
    out[eb == 0] = "denormal_max"
    out[mb == 0] = "zero"
    out[mb == 0x7F800000] = "inf"
    out[mb > 0x7F800000] = "nan"
    return out


def log2_rounds_up(mb):
    """mxfp_math.hpp:24-31, 42-44: the float32 log2 of a normal maximum 2^v (1 - j 2^-24) rounds to the integer v"""
    eb, man = mb >> 23, mb & 0x007FFFFF
    v = eb - 126
    if not 1 <= eb <= 254 or man == 0 or v == 0:
        return False
    a, j = abs(v), 0x00800000 - man
    c = a.bit_length() - 1
    g = 25 - c if (v > 0 and a & (a - 1) == 0) else 24 - c
    return j <= JMAX.get(g, 0)


def mxfp_general_subpath(mb, f, f32_input):
    """MxfpBlock::setup + apply_vec (blockfmt.hip:128-154) for ONE block of the general path: "fast" when the block itself allows
    the branch-free element form (the wave takes it only when every lane does), else "literal" (mxfp_q1 per element)"""
    k = mxfp_consts(f)
    mb = int(mb)
    eb = mb >> 23
    zero = mb == 0                                             # :129
    pow2 = False
    if 1 <= eb <= 254:                                         # mxfp_math.hpp:41
        if f32_input and log2_rounds_up(mb):
            eb += 1
        se = eb - k.big_log2                                   # :45
        pow2 = eb != 255 and 1 <= se <= 253                    # :46-48, blockfmt.hip:132
        v_field = (mb >> 23) - se + 127                        # exponent field of max * inv (:133, :145)
    else:
        v_field = 0 if zero else 255                           # denormal / Inf / NaN maxima: the scale is no normal power of two
    float_fast_ok = v_field <= k.max_ok_field                  # floatq.hpp:50-53, for the block's largest element
    return "fast" if k.usable and (pow2 or zero) and float_fast_ok else "literal"   # :141-146


# ------------------------------------------------------------------------------------------------ SBFP
SbfpFmt = namedtuple("SbfpFmt", "p man exp bias flush clamp symmetric")
SBFP_FORMATS = [SbfpFmt(4, 4, 4, 7, True, True, True), SbfpFmt(8, 2, 5, 15, True, True, True), SbfpFmt(2, 4, 4, 7, True, True, True),
                SbfpFmt(8, 4, 4, 7, False, True, True), SbfpFmt(8, 4, 4, 7, True, False, True), SbfpFmt(8, 4, 4, 7, True, True, False),
                SbfpFmt(24, 7, 8, 127, False, False, True)]
SBFP_CLASSES = ("fast", "scale_small", "scale_large", "unclamped", "zero", "nan", "inf", "denormal_max", "scaler_saturates", "scaler_flushes")


def sbfp_scale(mb, f):
    """blockfmt.hip:36 s = max / man_scaling (:252 man_scaling = 2^(p-1) - 1), float32"""
    m = np.asarray(mb, dtype=np.uint32).view(np.float32)
    with np.errstate(all="ignore"):
        return (m / np.float32((1 << (f.p - 1)) - 1)).astype(np.float32)


def sbfp_fast(mb, f):
    """blockfmt.hip:39 SbfpBlock::setup: fast = clamp && recip_ok(s)"""
    s = sbfp_scale(mb, f)
    with np.errstate(all="ignore"):
        return np.logical_and(bool(f.clamp), (s >= np.float32(RECIP_LO)) & (s <= np.float32(RECIP_HI)))


def sbfp_classify(mb, f):
    mb = np.asarray(mb, dtype=np.uint32)
    s = sbfp_scale(mb, f)
    sb = s.view(np.uint32).astype(np.int64)
    # the scaler cast float_q1(s) (oracle.c float_q1): nearest-even on the bit pattern, saturation above exponent 2^(e-1), and
    # the subnormal range below 2^min_exp (flushed, or rounded to the format's subnormal grid)
    drop = 23 - f.man
    half, mask = 1 << (drop - 1), (1 << drop) - 1
    tie_even = ((sb & mask) == half) & (((sb >> drop) & 1) == 0)
    qb = (sb + np.where(tie_even, 0, half)) & ~mask
    saturates = (qb >> 23) > (1 << (f.exp - 1)) + 127
    flushes = (sb >> 23) - 127 < -(f.bias - 1)
    out = np.full(mb.shape, "fast" if f.clamp else "unclamped", dtype=object)
    out[flushes] = "scaler_flushes"
    out[saturates] = "scaler_saturates"
    with np.errstate(all="ignore"):
        out[s > np.float32(RECIP_HI)] = "scale_large"
        out[s < np.float32(RECIP_LO)] = "scale_small"
    out[(mb >> 23) == 0] = "denormal_max"
    out[mb == 0] = "zero"
    out[mb == 0x7F800000] = "inf"
    out[mb > 0x7F800000] = "nan"
    return out


def classify(kind, mb, f, dt):
    return mxfp_classify(mb, f, dt.name == "f32") if kind == "mxfp" else sbfp_classify(mb, f)


def ordinary_class(kind, f):
    if kind == "sbfp":
        return "fast" if f.clamp else "unclamped"
    k = mxfp_consts(f)
    return "xdomain" if k.xdomain else ("general_fast" if k.usable else "general_literal")


# ------------------------------------------------------------------------------------------------ candidate maxima, representatives
_CAND = {}


def candidates(dt):
    """native magnitudes a block maximum is drawn from: EVERY 16-bit magnitude; for float32 every exponent field with mantissas at
    both ends, in the middle and 1 .. 89 ulps below the next power of two.  Returns (native patterns, float32 bit patterns)."""
    if dt.name not in _CAND:
        if dt.itemsize == 2:
            pat = np.arange(0, 0x8000, dtype=np.uint32)
        else:
            mans = np.array([0, 1, 0x123456, 0x400000, 0x6ABCDE, 0x7FFFA6, 0x7FFFA7, 0x7FFFA8, 0x7FFFD4, 0x7FFFFB, 0x7FFFFE, 0x7FFFFF], dtype=np.uint32)
            pat = (np.arange(0, 256, dtype=np.uint32)[:, None] << 23 | mans[None, :]).reshape(-1)
        _CAND[dt.name] = (pat, f32_bits(pat, dt))
    return _CAND[dt.name]


def expressible(kind, f, dt):
    """the classes that some maximum of dtype dt falls into"""
    return sorted(set(classify(kind, candidates(dt)[1], f, dt)))


def representatives(kind, f, dt, cls, n=4):
    """up to n native maxima of class cls: the smallest, the largest and evenly spaced ones between (deterministic)"""
    pat, mb = candidates(dt)
    idx = np.nonzero(classify(kind, mb, f, dt) == cls)[0]
    if cls == ordinary_class(kind, f):           # ordinary blocks: keep to the middle of the range (the far ends belong to other tests)
        keep = idx[(mb[idx] >> 23 >= 100) & (mb[idx] >> 23 <= 140)]
        idx = keep if keep.size else idx
    if idx.size == 0:
        return []
    pick = sorted({int(idx[(idx.size - 1) * i // max(n - 1, 1)]) for i in range(n)})
    return [int(pat[i]) for i in pick]


# ------------------------------------------------------------------------------------------------ blocks
def _rand(n, salt):
    return splitmix64(np.arange(n, dtype=np.uint64), 0xB10C + salt)


def block_of(native_max, dt, B, salt):
    """B native patterns whose largest magnitude is native_max (finite): the maximum at a salt-dependent position, -max on odd salts,
    the rest a third each from the top three binades below it, from all patterns below it (zeros of both signs and the dtype's
    denormals among them) and from the lowest patterns; random signs"""
    r = _rand(B, salt)
    m = int(native_max)
    v = (r >> np.uint64(8)).astype(np.uint64)
    top = m - (v % np.uint64(min(m, 3 << dt.mant) + 1)).astype(np.int64)
    anyp = (v % np.uint64(m + 1)).astype(np.int64)
    low = (v % np.uint64(min(m, 4 << dt.mant) + 1)).astype(np.int64)
    kind = (r & np.uint64(3)).astype(np.int64)
    mag = np.where(kind <= 1, top, np.where(kind == 2, anyp, low))
    mag[(salt * 7 + 3) % B] = m
    sign = ((r >> np.uint64(40)) & np.uint64(1)).astype(np.int64)
    sign[(salt * 7 + 3) % B] = salt & 1
    return (mag | sign << (8 * dt.itemsize - 1)).astype(dt.np_bits)


def special_block(cls, rep, dt, B, salt, anchor):
    """a block of one of the classes whose maximum is no finite nonzero number; anchor: native maximum of the finite part"""
    sbit = 1 << (8 * dt.itemsize - 1)
    if cls == "zero":                                    # signed zeros (a zero MXFP block keeps them)
        return (((_rand(B, salt) >> np.uint64(17)) & np.uint64(1)).astype(np.int64) * sbit).astype(dt.np_bits)
    b = block_of(anchor, dt, B, salt).astype(np.int64)
    p = (salt * 5 + 1) % B
    if cls == "inf":                                     # one or two infinities of either sign among finite elements
        b[p] = dt.inf | (sbit if salt & 1 else 0)
        if salt & 2:
            b[(p + B // 2) % B] = dt.inf | (0 if salt & 1 else sbit)
    else:                                                # NaN (quiet, either sign), sometimes beside an infinity
        b[p] = rep | (sbit if salt & 1 else 0)
        if salt & 2:
            b[(p + 3) % B] = dt.inf
    return b.astype(dt.np_bits)


def make_block(kind, f, dt, cls, rep, B, salt):
    if cls in ("zero", "inf", "nan"):
        return special_block(cls, rep, dt, B, salt, ordinary_anchor(kind, f, dt))
    return block_of(rep, dt, B, salt)


# ------------------------------------------------------------------------------------------------ ordinary data
def ordinary_window(kind, f, dt):
    """[lo, hi] for the maximum of an ordinary block: inside it every block is `xdomain` / `fast` (or `unclamped`) whatever else it
    holds.  MXFP: all of the middle of the float range; SBFP: the scale s = max / (2^(p-1) - 1) inside recip_ok's interval and
    inside the scaler format's normal range."""
    top = 60000.0 if dt.name == "f16" else 2.0 ** 100
    if kind == "mxfp":
        return 2.0 ** -12, min(top, 2.0 ** 40)
    ms = float((1 << (f.p - 1)) - 1)
    s_lo = max(RECIP_LO, 2.0 ** -(f.bias - 1)) * 2.0
    s_hi = min(RECIP_HI, 2.0 ** (1 << (f.exp - 1)) * 1.5) / 2.0
    return s_lo * ms, min(top, s_hi * ms)


def ordinary_anchor(kind, f, dt):
    """native pattern of the geometric middle of ordinary_window"""
    lo, hi = ordinary_window(kind, f, dt)
    t = torch.tensor([(lo * hi) ** 0.5]).to(dt.torch)
    return int(t.view(dt.t_bits).numpy().view(dt.np_bits)[0])


def ordinary(kind, f, dt, rows, nblk, B, seed=0):
    """[rows, nblk * B] of make("heavy") scaled into ordinary_window: clamped below its top, one element per block lifted to the
    window's middle where the block's own maximum lies under it.  Returns native patterns."""
    lo, hi = ordinary_window(kind, f, dt)
    mid = (lo * hi) ** 0.5
    x = make("heavy", (rows, nblk, B), seed=seed + 31 * B, dtype=torch.float32, block=B).double() * (mid / 16.0)
    x = x.clamp(-hi, hi)
    low = x.abs().amax(-1) < mid
    r = (splitmix64(np.arange(rows * nblk, dtype=np.uint64), seed + 5) % np.uint64(B)).astype(np.int64).reshape(rows, nblk)
    pos = torch.from_numpy(r)
    lift = torch.where(low, torch.tensor(mid, dtype=torch.float64), x.gather(-1, pos[..., None])[..., 0].abs())
    sgn = torch.where(x.gather(-1, pos[..., None])[..., 0] < 0, -1.0, 1.0)
    x.scatter_(-1, pos[..., None], (lift * sgn)[..., None])
    t = x.float().to(dt.torch).reshape(rows, nblk * B).contiguous()
    return t.view(dt.t_bits).numpy().view(dt.np_bits).copy()


def block_maxima(pat, dt, B):
    """float32 bit patterns of max|x| of each block of B of [rows, L] native patterns (L % B == 0); a NaN wins"""
    a = f32_bits(pat, dt).reshape(pat.shape[0], -1, B) & np.uint32(0x7FFFFFFF)
    return a.max(-1)


# ------------------------------------------------------------------------------------------------ the table
Planted = namedtuple("Planted", "x rows_class blocks_per_wave plan")   # plan: [(row, block index, class, native rep)]


def class_list(kind, f, dt):
    """(class, representatives) for every class dt can express under f, the ordinary class first"""
    o = ordinary_class(kind, f)
    names = [o] + [c for c in expressible(kind, f, dt) if c != o]
    return [(c, representatives(kind, f, dt, c)) for c in names]


def planted(kind, f, dt, B, rows=None, width=None, seed=0):
    """For every class: `rows` rows of ordinary data `width` elements long, row r holding ONE block of the class in each of its
    waves, at block position r % blocks_per_wave -- so every class sits at every position of a wave, in a wave of otherwise
    ordinary blocks.  Defaults: rows = 2 * blocks_per_wave, width = two waves.  Classes are stacked along dim 0."""
    bpw = max(1, elements_per_wave(dt) // B)             # (a block wider than a wave: the generic kernel, one position)
    rows = 2 * bpw if rows is None else rows
    width = 2 * elements_per_wave(dt) if width is None else width
    assert width % B == 0
    nblk = width // B
    cl = class_list(kind, f, dt)
    x = ordinary(kind, f, dt, rows * len(cl), nblk, B, seed)
    plan, rows_class = [], []
    for ci, (cls, reps) in enumerate(cl):
        for r in range(rows):
            row = ci * rows + r
            rows_class.append(cls)
            for w in range(0, nblk, bpw):
                k = w + r % bpw
                if k >= nblk:
                    continue
                rep = reps[(r // bpw + r + w // bpw) % len(reps)]
                x[row, k * B:(k + 1) * B] = make_block(kind, f, dt, cls, rep, B, row * 131 + k)
                plan.append((row, k, cls, rep))
    return Planted(from_bits(x, dt), rows_class, bpw, plan)


def planted_inner(kind, f, dt, B, inner, nblk):
    """[outer, nblk * B, inner] with blocks along dim 1 (the generic kernel: element stride `inner`): row r of a planted table becomes
    column r % inner of outer index r // inner.  At least two outer indices; the table is padded to a whole number of them with its
    own first rows, never cut.  Returns (tensor, class of each table row)."""
    n_classes = len(class_list(kind, f, dt))
    t = planted(kind, f, dt, B, max(8, -(-2 * inner // n_classes)), nblk * B)
    pad = -t.x.shape[0] % inner
    x = torch.cat([t.x, t.x[:pad]])
    return x.reshape(-1, inner, nblk * B).movedim(-1, 1).contiguous(), list(t.rows_class) + list(t.rows_class[:pad])


def rows_of(y3):
    """[outer, L, inner] back to the [rows, L] layout of the planted table"""
    return y3.movedim(1, -1).reshape(-1, y3.shape[1]).contiguous()


def uniform(kind, f, dt, B, rows_per_class=4, width=None, seed=0):
    """rows made of one class only: rows_per_class rows per class, one wave wide by default, row i built on representative i"""
    width = elements_per_wave(dt) if width is None else width
    nblk = width // B
    cl = class_list(kind, f, dt)
    x = np.zeros((rows_per_class * len(cl), width), dtype=dt.np_bits)
    plan, rows_class = [], []
    for ci, (cls, reps) in enumerate(cl):
        for r in range(rows_per_class):
            row = ci * rows_per_class + r
            rows_class.append(cls)
            for k in range(nblk):
                rep = reps[(r + (k if len(reps) > rows_per_class else 0)) % len(reps)]
                x[row, k * B:(k + 1) * B] = make_block(kind, f, dt, cls, rep, B, row * 977 + k)
                plan.append((row, k, cls, rep))
    return Planted(from_bits(x, dt), rows_class, elements_per_wave(dt) // B, plan)


def planted_at(kind, f, dt, B, nblk, where, seed=0):
    """[nblk, B]: ordinary blocks with the classes of class_list planted, in turn, at the block indices `where`"""
    cl = [(c, reps) for c, reps in class_list(kind, f, dt) if c != ordinary_class(kind, f)]
    x = ordinary(kind, f, dt, nblk, 1, B, seed)
    plan = []
    for i, k in enumerate(where):
        cls, reps = cl[i % len(cl)]
        rep = reps[(i // len(cl)) % len(reps)]
        x[k] = make_block(kind, f, dt, cls, rep, B, k * 29 + i)
        plan.append((k, 0, cls, rep))
    return Planted(from_bits(x, dt), None, elements_per_wave(dt) // B, plan)


def wave_classes(kind, f, dt, x, B):
    """set of (wave class, classes of the wave's blocks) over the waves of a [rows, L] tensor on the rows path, L a whole number of
    waves: a wave is `xdomain` only when every block of it is"""
    pat = x.contiguous().view(dt.t_bits).numpy().view(dt.np_bits)
    cls = classify(kind, block_maxima(pat, dt, B), f, dt)
    bpw = max(1, elements_per_wave(dt) // B)
    flat = cls.reshape(-1)
    out = set()
    for w in range(0, flat.size, bpw):
        blk = frozenset(flat[w:w + bpw])
        o = ordinary_class(kind, f)
        out.add((o if blk == {o} else "general", blk))
    return out


def float32_denormal_blocks(B=32):
    """[n, B] float32: one block per denormal maximum k 2^-149 at and just below every power of two -- k = 2^n - t, n = 1 .. 23,
    t = 0 .. 3, and every t up to 96 below 2^-126, where the reference's float32 log2 rounds up to the integer for t <= 22
    (mxfp_math.hpp mxfp_block_scale's denormal branch; the device's log2f does not round there as the CPU's does)"""
    ks = sorted({(1 << n) - t for n in range(1, 24) for t in range(4)} | {(1 << 23) - t for t in range(1, 97)})
    ks = [k for k in ks if 1 <= k < (1 << 23)]
    return from_bits(np.stack([block_of(k, DTYPES["f32"], B, 3 * i + 1) for i, k in enumerate(ks)]), DTYPES["f32"]), ks


# ------------------------------------------------------------------------------------------------ every 16-bit pattern
def pattern_blocks(native_max, dt, B=32):
    """every finite 16-bit pattern (both signs) of magnitude <= native_max as the non-maximum elements of blocks of B whose element 0
    is the maximum; the last block is filled up with the maximum itself"""
    assert dt.itemsize == 2
    m = int(native_max)
    mags = np.arange(0, m + 1, dtype=np.int64)
    pats = np.concatenate([mags, mags | 0x8000])
    n = -(-pats.size // (B - 1))
    body = np.full(n * (B - 1), m, dtype=np.int64)
    body[:pats.size] = pats
    out = np.empty((n, B), dtype=np.int64)
    out[:, 0] = m
    out[:, 1:] = body.reshape(n, B - 1)
    return out.astype(np.uint16)


def nonfinite_blocks(dt, B=32):
    """every Inf and NaN pattern of a 16-bit dtype, in blocks of their own"""
    mags = np.arange(dt.inf, 0x8000, dtype=np.int64)
    pats = np.concatenate([mags, mags | 0x8000])
    n = -(-pats.size // B)
    body = np.full(n * B, dt.inf + 1, dtype=np.int64)
    body[:pats.size] = pats
    return body.reshape(n, B).astype(np.uint16)


def native_of(value, dt):
    """native magnitude pattern of a float, or None when dt does not hold it exactly"""
    t = torch.tensor([value], dtype=torch.float64).to(dt.torch)
    if not bool(torch.isfinite(t.double()).all()) or float(t.double()[0]) != float(value):
        return None
    return int(t.view(dt.t_bits).numpy().view(dt.np_bits)[0]) & 0x7FFF if dt.itemsize == 2 else None


def mxfp_pattern_maxima(f, dt):
    """maxima of test_every_16_bit_pattern (those dt holds exactly): 1.0; all-ones mantissa; the smallest x-domain block maximum
    2^(bias + big_log2 - 127) and the pattern below it; 2^104 (2 - 2^-7); 2^105; the largest finite value; a denormal"""
    k = mxfp_consts(f)
    one = native_of(1.0, dt)
    out = [one, one | ((1 << dt.mant) - 1)]
    lo = native_of(2.0 ** (k.bias + k.big_log2 - 127), dt)
    if lo is not None and lo > 1:
        out += [lo, lo - 1]
    out += [native_of(2.0 ** 104 * (2.0 - 2.0 ** -7), dt), native_of(2.0 ** 105, dt), dt.inf - 1]
    if dt.name == "bf16":
        out.append(0x0023)             # a bfloat16 denormal (35 x 2^-133)
    return [m for m in out if m is not None]


def sbfp_pattern_maxima(f, dt):
    """(2^(p-1) - 1) * 2^e (the block scale is a power of two, quotients fall on k + 0.5) for e = 0 and -3, where dt holds it; and
    one maximum on each side of both ends of recip_ok's interval for s"""
    ms = float((1 << (f.p - 1)) - 1)
    out = [native_of(ms, dt), native_of(ms / 8.0, dt)]
    pat, mb = candidates(dt)
    fin = mb < 0x7F800000
    s = sbfp_scale(mb, f).astype(np.float64)
    for edge, below in ((RECIP_LO, True), (RECIP_LO, False), (RECIP_HI, True), (RECIP_HI, False)):
        # ends of the interval are INSIDE it (common.hpp:412 >=, <=): `inside` is monotone in the pattern
        idx = np.nonzero(fin & ((s < edge) if edge == RECIP_LO and below else (s >= edge) if edge == RECIP_LO else
                                (s <= edge) if below else (s > edge)))[0]
        if idx.size and idx.size != int(fin.sum()):
            out.append(int(pat[idx[-1] if below else idx[0]]))
    return sorted({m for m in out if m is not None and m > 0})


def n_pattern_maxima(kind, f, dt):
    """how many maxima test_every_16_bit_pattern must get.  MXFP: all eight in bfloat16; float16 holds 1.0, the all-ones mantissa and
    its largest finite value only (nothing at 2^-96 or below, at 2^104 or above, no float32 denormal).  SBFP: two power-of-two-scale
    maxima and the four edges of recip_ok in bfloat16; float16 ends below s = 2^20 (two edges less); at p = 24 the maximum 2^23 - 1
    and its eighth need 23 significant bits (two less in both)."""
    if kind == "mxfp":
        return 8 if dt.name == "bf16" else 3
    return (6 if dt.name == "bf16" else 4) - (2 if f.p == 24 else 0)


# ------------------------------------------------------------------------------------------------ references
def mxfp_ref(O, x, f, B, block_dim=-1):
    """the oracle (oracle/oracle.c oracle_mxfp_qdq): float32 result"""
    return O.mxfp_cast(x, f.man, f.exp, B, block_dim)


def sbfp_ref(O, x, f, B, block_dim=-1):
    """the oracle (oracle/oracle.c oracle_sbfp_qdq): float32 result"""
    return O.sbfp_cast(x, f.p, B, f.man, f.exp, f.bias, f.flush, f.clamp, f.symmetric, block_dim)


def ref(kind, O, x, f, B, block_dim=-1):
    return (mxfp_ref if kind == "mxfp" else sbfp_ref)(O, x, f, B, block_dim)


def torch_mxfp(O, x, f, B):
    """numerical/format.py:545-564 MXFP.cast restated with block-wise torch float32 ops on [rows, L] (blocks along the last dim), the
    element cast by the oracle's floating_point_cast.  All-zero blocks keep their zeros with their signs (the reference
    returns NaN there)."""
    k = mxfp_consts(f)
    x = x.float()
    out = torch.empty_like(x)
    big = torch.tensor(2.0 ** k.big_log2, dtype=torch.float32)
    for b0 in range(0, x.shape[-1], B):
        c = x[:, b0:b0 + B]
        m = torch.max(torch.abs(c), dim=-1, keepdim=True)[0]                       # :541-543
        s = 2 ** torch.floor(torch.log2(m)) / big                                  # :552-553
        y = O.floating_point_cast((c / s).contiguous(), f.man, f.exp, k.bias, False) * s   # :558
        out[:, b0:b0 + B] = torch.where(m == 0, c * 0.0, y)
    return out


def torch_sbfp(O, x, f, B):
    """numerical/format.py:453-479 ScaledBlockFloatingPoint.cast restated the same way"""
    x = x.float()
    out = torch.empty_like(x)
    ms = float((1 << (f.p - 1)) - 1)                                               # :429-431
    for b0 in range(0, x.shape[-1], B):
        c = x[:, b0:b0 + B].contiguous()
        s = torch.max(torch.abs(c), dim=-1, keepdim=True)[0] / ms                  # :463
        q = O.fixed_point_cast((c / s).contiguous(), f.p, 0, f.clamp, f.symmetric) * O.floating_point_cast(s.contiguous(), f.man, f.exp, f.bias, f.flush, unsigned=True)   # :469-470
        out[:, b0:b0 + B] = torch.where(s > 0.0, q, c)                             # :467-472
    return out


def torch_ref(kind, O, x, f, B):
    return (torch_mxfp if kind == "mxfp" else torch_sbfp)(O, x, f, B)


FORMATS = {"mxfp": MXFP_FORMATS, "sbfp": SBFP_FORMATS}

# ------------------------------------------------------------------------------------------------ the fixture of the reference's casts
# tests/golden/blockfmt_classes.npz (oracle/gen_golden_blockfmt.py): (shorthand, kind, format, block size)
GOLDEN_CASES = [("MXFP8[E4M3]{32}", "mxfp", MxfpFmt(3, 4), 32), ("MXFP8[E5M2]{32}", "mxfp", MxfpFmt(2, 5), 32),
                ("MXFP6[E3M2]{32}", "mxfp", MxfpFmt(2, 3), 32), ("MXFP4[E2M1]{32}", "mxfp", MxfpFmt(1, 2), 32),
                ("SBFP<XP[4,0](CSN)><FP[0|4|4,7](FN)>{16}", "sbfp", SbfpFmt(4, 4, 4, 7, True, True, True), 16)]   # the last: SBFP12_16
GOLDEN_DTYPES = ("f32", "bf16")


def golden_table(kind, f, dt, B):
    """the planted table at its smallest: one wave per row, every class at every block position of it"""
    return planted(kind, f, dt, B, rows=elements_per_wave(dt) // B, width=elements_per_wave(dt))


def zero_block_mask(x, B):
    """elements of the all-zero blocks of a [rows, L] tensor (L % B == 0)"""
    z = (x.float().reshape(x.shape[0], -1, B) == 0).all(-1, keepdim=True)
    return z.expand(-1, -1, B).reshape(x.shape)


def run_lib(kind, ops, x, f, B, block_dim=-1, out_dtype=None):
    """the library's public call for a case"""
    if kind == "mxfp":
        return ops.mxfp_qdq(x, f.man, f.exp, B, block_dim, out_dtype=out_dtype)
    return ops.sbfp_qdq(x, f.p, B, f.man, f.exp, f.bias, f.flush, f.clamp, f.symmetric, block_dim, out_dtype=out_dtype)
