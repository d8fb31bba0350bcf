"""The sparsity kernels' case tables: the adversarial score alphabet, the group sets built from it, the truths, the kernel route of
dmxq_nm_mask (csrc/nm_mask.hip) restated in Python, and the N:M and top-k case tables that tests/test_sparse_cases_host.py (no GPU) holds
against the library's own answers and tests/test_gpu_sparse_routes.py runs on the device.  No GPU is needed to import this module.

The N:M rank rule -- ascending STABLE order, -0 == +0, every NaN equal and largest -- is written down in five places of the library
(csrc/nm_rank.hpp; the run-time loops of nm_mask_anyM_kernel; hn_sort_key and the unrolled loops of csrc/hypernet_rows.hpp; the "same
group" loop of hs_rows8 in csrc/hypernet.hip; the multi-tensor chain over the rows kernel).  The truth here is none of them: it is the
reference's own statement, `argsort(score.reshape(-1, M), dim=1, stable=True)[:, :M - K]` scattered as zeros into ones, in float32 on
the CPU.

The route restatement (nm_route) is written from the comments of include/dmxq.h and csrc/nm_mask.hip, NOT by asking the library."""
import functools
from collections import namedtuple

import numpy as np
import torch

from _data import make, splitmix64, uniform

F32, F16, BF16 = 0, 1, 2
T32, T16, TB16 = torch.float32, torch.float16, torch.bfloat16
DTYPES = (T32, T16, TB16)
CODE = {T32: F32, T16: F16, TB16: BF16}
DT_NAMES = {T32: "f32", T16: "f16", TB16: "bf16", None: "-"}
OK, ERR_BAD_ARG = 0, 1

NONE, TYPED, F32_MASK, VECTOR, GROUP_M, ANY_M = "none", "typed", "f32_mask", "vector", "group_m", "any_m"
ROUTES = (TYPED, F32_MASK, VECTOR, GROUP_M, ANY_M)
ROUTE_CODE = {NONE: 0, TYPED: 1, F32_MASK: 2, VECTOR: 3, GROUP_M: 4, ANY_M: 5}     # dmxq_nm_route (include/dmxq.h)
BAD_ARG = "bad_arg"

THREADS = 256            # a workgroup: four waves of 64
GRID_CAP = 2048          # DMXQ_GRID_CAP (csrc/common.hpp kMaxBlocks): grid-stride kernels take further rounds beyond it
TOPK_CHUNK = 2048        # csrc/topk.hip: a workgroup's chunk, 8 consecutive scores per thread
TOPK_SCAN_ROUND = 256    # topk_scan_kernel scans the chunk counts 256 at a time, a carry between the rounds

# ------------------------------------------------------------------------------------------------------------------ the alphabet
SYMBOLS = ("-inf", "-max", "-1", "-mind", "-0", "+0", "+mind", "1", "1+eps", "max", "+inf", "nan", "-nan")
S_NEG_MIND, S_NEG0, S_POS0, S_POS_MIND, S_ONE, S_NAN, S_NEG_NAN = 3, 4, 5, 6, 7, 11, 12
# bit patterns of (min denormal, 1, 1 + eps, max finite, inf, a quiet NaN) and of the sign
_BITS = {T32: ((0x00000001, 0x3F800000, 0x3F800001, 0x7F7FFFFF, 0x7F800000, 0x7FC00000), 0x80000000, np.uint32, np.int32),
         T16: ((0x0001, 0x3C00, 0x3C01, 0x7BFF, 0x7C00, 0x7E00), 0x8000, np.uint16, np.int16),
         TB16: ((0x0001, 0x3F80, 0x3F81, 0x7F7F, 0x7F80, 0x7FC0), 0x8000, np.uint16, np.int16)}


def from_bits(bits, dtype):
    """unsigned bit patterns -> a tensor of `dtype`"""
    _, _, u, i = _BITS[dtype]
    return torch.from_numpy(np.ascontiguousarray(np.asarray(bits).astype(u)).view(i)).view(dtype)


def alphabet(dtype):
    """the 13 symbols of SYMBOLS in `dtype`; the negative NaN is the NaN's pattern with the sign bit OR-ed in"""
    (mind, one, onee, mx, inf, nan), sign, _, _ = _BITS[dtype]
    return from_bits([sign | inf, sign | mx, sign | one, sign | mind, sign, 0, mind, one, onee, mx, inf, nan, sign | nan], dtype)


# ---------------------------------------------------------------------------------------------------------------- the group sets
M8_RANDOM, OTHER_RANDOM = 20000, 4096
M16_PAIRS = ((S_NEG0, S_POS0), (S_ONE, S_NAN), (S_NEG_MIND, S_POS0))
GROUP_SET_MS = (2, 4, 8, 16, 1, 3, 12, 32, 64)


def _two_symbol(a, b, M):
    """all 2^M assignments of the symbols a (bit clear) and b (bit set) to M positions"""
    bits = (np.arange(1 << M, dtype=np.int64)[:, None] >> np.arange(M)) & 1
    return np.where(bits == 1, b, a).astype(np.uint8)


def _random_groups(count, M, seed):
    return (splitmix64(np.arange(count * M, dtype=np.uint64), seed) % np.uint64(len(SYMBOLS))).astype(np.uint8).reshape(count, M)


@functools.lru_cache(maxsize=None)
def group_indices(M):
    """uint8 [groups, M]: the symbol index of every position of every group of the set for this M
       2, 4   all 13^M groups;
       8      for every unordered pair of symbols (the equal-comparing pairs -0 / +0 and NaN / -NaN among them) all 256 assignments of the
              pair to the 8 positions -- a group of one symbol alone is assignment 0 --, plus 20 000 seeded random groups;
       16     all 65 536 two-symbol assignments of (-0, +0), (1, NaN), (-min denormal, +0);
       else   4096 seeded random groups."""
    S = len(SYMBOLS)
    if M in (2, 4):
        return np.ascontiguousarray(np.indices((S,) * M).reshape(M, -1).T.astype(np.uint8))
    if M == 8:
        pairs = [_two_symbol(a, b, 8) for a in range(S) for b in range(a + 1, S)]
        return np.concatenate(pairs + [_random_groups(M8_RANDOM, 8, 0x8888)])
    if M == 16:
        return np.concatenate([_two_symbol(a, b, 16) for a, b in M16_PAIRS])
    return _random_groups(OTHER_RANDOM, M, 0x1000 + M)


def ks_for(M):
    """every K for M <= 8; 1, 5, 8, 15, 16 for M = 16; 1, M // 2 (or 1), M otherwise"""
    if M <= 8:
        return tuple(range(1, M + 1))
    if M == 16:
        return (1, 5, 8, 15, 16)
    return tuple(sorted({1, M // 2 or 1, M}))


def group_scores(M, dtype):
    """the whole group set as a [groups, M] score tensor"""
    return alphabet(dtype)[torch.from_numpy(group_indices(M).astype(np.int64))]


@functools.lru_cache(maxsize=None)
def _shuffle(M):
    G = len(group_indices(M))
    return np.argsort(splitmix64(np.arange(G, dtype=np.uint64), 0x5EED + M), kind="stable")


def row_group_indices(M, n_groups):
    """n_groups groups for one table row: the set in a fixed seeded order (so that a short row is a sample of the whole set and not its
    first, least varied groups), truncated, or tiled when the row is longer than the set"""
    idx = group_indices(M)
    return idx[_shuffle(M)[np.arange(n_groups) % len(idx)]]


def place(groups, outer, L, inner):
    """[outer * (L / M) * inner, M] groups -> the [outer, L, inner] tensor whose groups run along L with stride `inner`, in the order
    (outer, group along L, inner position)"""
    M = groups.shape[1]
    return groups.reshape(outer, L // M, inner, M).permute(0, 1, 3, 2).reshape(outer, L, inner).contiguous()


def split3(shape, dim):
    d = dim % len(shape)
    return int(np.prod(shape[:d], dtype=np.int64)), int(shape[d]), int(np.prod(shape[d + 1:], dtype=np.int64))


# -------------------------------------------------------------------------------------------------------------------- the truths
class NmTruth:
    """The reference's statement on the CPU in float32, sorted once per score and asked for every K:
    argsort(score.reshape(-1, M), dim=1, stable=True)[:, :M - K] scattered as zeros into ones (groups along block_dim)."""

    def __init__(self, score, M, block_dim=-1):
        s = score.detach().cpu().to(T32).movedim(block_dim, -1)
        self.M, self.block_dim, self.shape = M, block_dim, s.shape
        self.order = torch.argsort(s.reshape(-1, M), dim=1, stable=True)

    def mask(self, K, dtype=T32):
        m = torch.ones(self.order.shape, dtype=T32)
        m.scatter_(1, self.order[:, :self.M - K], 0.0)
        return m.reshape(self.shape).movedim(-1, self.block_dim).contiguous().to(dtype)


def nm_truth(score, K, M, block_dim=-1, dtype=None):
    return NmTruth(score, M, block_dim).mask(K, dtype or score.dtype)


def density_for(n, n_zero):
    """a density whose int(n * (1 - density)), the reference's zero count (sparse.py:116), is exactly n_zero"""
    d = 1.0 - (n_zero + 0.5) / n
    assert int(n * (1.0 - d)) == n_zero, (n, n_zero)
    return d


def topk_truth(oracle, score, n_zero):
    """oracle.topk_mask (a stable argsort: lowest index first among ties, -0 == +0, NaN largest) with the zero count given exactly"""
    if n_zero == 0:
        return torch.ones_like(score)
    return oracle.topk_mask(score, density_for(score.numel(), n_zero))


# ------------------------------------------------------------------------------------------------- the route of dmxq_nm_mask
# (x, score -> y) dtype triples of the typed mask-and-multiply (csrc/hypernet.hip)
TYPED_TRIPLES = ((TB16, TB16, TB16), (T16, T16, T16), (T32, T32, T32), (TB16, T32, T32), (T16, T32, T32), (TB16, T32, TB16))
_TYPED_CODES = frozenset((CODE[x], CODE[s], CODE[y]) for x, s, y in TYPED_TRIPLES)


def nm_route(dts, dtx, dtm, dty, outer, L, inner, K, M, a_score, a_x, a_mask, a_y):
    """The route of one dmxq_nm_mask call from dtype codes, sizes and the four base addresses (0 / None = NULL: that output is not
    wanted): one of ROUTES, NONE for an empty tensor, BAD_ARG where the entry refuses the arguments."""
    valid = lambda d: d in (F32, F16, BF16)
    al = lambda a: a % 16 == 0
    if not valid(dts) or outer < 0 or L < 0 or inner < 0:
        return BAD_ARG
    if M < 1 or M > 64 or K < 1 or K > M or L % M:
        return BAD_ARG
    if a_mask and not valid(dtm):
        return BAD_ARG
    if a_y and (not valid(dty) or not valid(dtx) or not a_x):
        return BAD_ARG
    if not a_mask and not a_y:
        return BAD_ARG
    n = outer * L * inner
    if n == 0:
        return NONE
    if not a_score:
        return BAD_ARG
    flat = inner == 1 and M in (2, 4, 8, 16) and n % 16 == 0 and al(a_score) and (not a_x or al(a_x)) and (not a_mask or al(a_mask)) \
        and (not a_y or al(a_y))
    if flat and a_y and not a_mask and M <= 8 and (dtx, dts, dty) in _TYPED_CODES:
        return TYPED
    if flat and a_mask and not a_y and dts == F32 and dtm == F32 and M <= 8:
        return F32_MASK
    if flat:
        return VECTOR
    return GROUP_M if M in (2, 4, 8, 16) else ANY_M


def tile_elements(route, M):
    """elements (TYPED, F32_MASK, VECTOR) or groups (GROUP_M, ANY_M) one workgroup takes per pass"""
    if route == TYPED:
        return THREADS * 4 * 8          # 256 lanes x 4 units x 8 elements
    if route == F32_MASK:
        return THREADS * 4 * 4          # 1024 16-byte vectors
    if route == VECTOR:
        return THREADS * 2 * (16 if M == 16 else 8)
    return THREADS                      # a lane per group


# --------------------------------------------------------------------------------------------------------- the N:M case table
# off_score / off_x: the bytes by which the view handed to the op starts off the 16-byte grid (0: an allocation's own base)
NmCase = namedtuple("NmCase", "route sdt xdt mdt out_dtype want_mask want_y M shape block_dim off_score off_x ks")


def ydt_of(c):
    """the dtype y must have: out_dtype, or torch's promotion of (x, score)"""
    return c.out_dtype or torch.promote_types(c.xdt, c.sdt)


def geometry(c):
    return split3(c.shape, c.block_dim)


def work_items(c):
    """what tile_elements counts"""
    n = int(np.prod(c.shape))
    return n if c.route in (TYPED, F32_MASK, VECTOR) else n // c.M


def edge(c):
    """"cap": more workgroups than the grid cap; "exact": a whole number of workgroup tiles; "partial": a clamped / guarded last tile"""
    t = tile_elements(c.route, c.M)
    w = work_items(c)
    if c.route not in (TYPED, F32_MASK) and -(-w // t) > GRID_CAP:     # (those two launch one workgroup per tile, whatever the size)
        return "cap"
    return "exact" if w % t == 0 else "partial"


def case_id(c):
    tag = f"{c.route}-{DT_NAMES[c.xdt]}.{DT_NAMES[c.sdt]}-m{DT_NAMES[c.mdt] if c.want_mask else '-'}-y{DT_NAMES[ydt_of(c)] if c.want_y else '-'}"
    return f"{tag}-M{c.M}-{'x'.join(map(str, c.shape))}-d{c.block_dim}" + (f"-so{c.off_score}" if c.off_score else "") + (f"-xo{c.off_x}" if c.off_x else "")


def _case(route, sdt, M, shape, xdt=None, mdt=None, out_dtype=None, want_mask=None, block_dim=-1, off_score=0, off_x=0, ks=None):
    want_y = xdt is not None
    want_mask = (not want_y) if want_mask is None else want_mask
    return NmCase(route, sdt, xdt, (mdt or sdt) if want_mask else None, out_dtype, want_mask, want_y, M, tuple(shape), block_dim, off_score,
                  off_x, tuple(ks or ks_for(M)))


VECTOR_CAP_N = GRID_CAP * 4096 + 4096 + 16      # bf16 -> bf16, M = 4: two workgroups of the capped grid take a second round
GROUP_CAP_GROUPS = GRID_CAP * THREADS + 3       # M = 2: 524 288 + 3 groups, one workgroup more than the cap


@functools.lru_cache(maxsize=None)
def nm_table():
    rows = []
    # TYPED: y only on the six compiled triples; tails of the 8192-element tile are clamped loads
    for xdt, sdt, ydt in TYPED_TRIPLES:
        od = ydt if ydt != torch.promote_types(xdt, sdt) else None
        for M in (2, 4, 8):
            for n in (16, 8192 - 16, 8192, 8192 + 16, 3 * 8192 + 48):
                rows.append(_case(TYPED, sdt, M, (n,), xdt=xdt, out_dtype=od))
    # F32_MASK: float32 score -> float32 mask; M = 8 exchanges vectors between lane pairs and clamps the tail to the last pair
    for M in (2, 4, 8):
        for n in (16, 4096 - 16, 4096, 4096 + 16, 2 * 4096 + 16):
            rows.append(_case(F32_MASK, T32, M, (n,)))
    # VECTOR
    pairs = [(s, m) for s in DTYPES for m in DTYPES if s != m]
    for M in (2, 4, 8, 16):
        P = tile_elements(VECTOR, M)
        for i, (s, m) in enumerate(pairs):                      # mask only, mask dtype != score dtype
            rows.append(_case(VECTOR, s, M, (P + 16,), mdt=m))
            if i < 2:
                rows.append(_case(VECTOR, s, M, (P - 16,), mdt=m))
                rows.append(_case(VECTOR, s, M, (P,), mdt=m))
        for s in (TB16, T16):                                   # mask only, one 16-bit dtype throughout
            rows.append(_case(VECTOR, s, M, (P + 16,)))
        for x, s in ((TB16, T32), (T32, TB16), (T16, TB16)):    # mask and y together, mixed dtypes
            rows.append(_case(VECTOR, s, M, (P + 16,), xdt=x, want_mask=True))
        rows.append(_case(VECTOR, T32, M, (P,), xdt=TB16, want_mask=True))
        if M == 16:                                             # the typed route and the float32-mask kernel stop at M = 8
            for n in (P - 16, P, P + 16):
                rows.append(_case(VECTOR, T32, M, (n,)))
            for x, s in ((TB16, TB16), (T32, T32), (TB16, T32)):
                rows.append(_case(VECTOR, s, M, (P + 16,), xdt=x))
        else:                                                   # y only on triples the typed route refuses
            for x, s in ((T32, TB16), (T32, T16), (T16, TB16)):
                rows.append(_case(VECTOR, s, M, (P + 16,), xdt=x))
    rows.append(_case(VECTOR, TB16, 4, (VECTOR_CAP_N,)))
    # GROUP_M: a lane per group, scalar accesses
    for M in (2, 4, 8, 16):
        for i, s in enumerate(DTYPES):
            rows.append(_case(GROUP_M, s, M, (M * 256, 3), block_dim=0))                       # inner = 3, 768 groups
            rows.append(_case(GROUP_M, s, M, (M * 85, 3), block_dim=0, xdt=DTYPES[(i + 1) % 3]))   # 255 groups, mixed-dtype y
            rows.append(_case(GROUP_M, s, M, (3, M * 5, 7), block_dim=-2, xdt=s, want_mask=True))  # inner = 7 through block_dim = -2
            rows.append(_case(GROUP_M, s, M, (M * 256,), off_score=4))                         # a score view 4 bytes into its allocation
            rows.append(_case(GROUP_M, s, M, (M * 304,), xdt=s, off_x=4))                      # x alone off the grid
            if M != 16:                                                                        # (with M = 16, n is a multiple of 16)
                rows.append(_case(GROUP_M, s, M, (3, 8)))                                      # n % 16 = 8
    rows.append(_case(GROUP_M, T32, 2, (2 * GROUP_CAP_GROUPS,)))
    # ANY_M: run-time loops
    for M in (1, 3, 12, 32, 64):
        for i, s in enumerate(DTYPES):
            rows.append(_case(ANY_M, s, M, (M * 256,)))
            rows.append(_case(ANY_M, s, M, (M * 77,), xdt=DTYPES[(i + 2) % 3], want_mask=True))
            rows.append(_case(ANY_M, s, M, (M * 51, 5), block_dim=0))
            rows.append(_case(ANY_M, s, M, (2, M * 3, 5), block_dim=1, xdt=s))
    return tuple(rows)


def nm_scores(c):
    """the row's scores: its share of the M-group set in the row's score dtype and layout (CPU, contiguous)"""
    outer, L, inner = geometry(c)
    idx = row_group_indices(c.M, outer * (L // c.M) * inner)
    groups = alphabet(c.sdt)[torch.from_numpy(idx.astype(np.int64))]
    return place(groups, outer, L, inner).reshape(c.shape)


def nm_x(c):
    """seeded normal data (finite; negative at about half of the masked positions, so that -0.0 appears in y)"""
    return make("normal", c.shape, seed=int(np.prod(c.shape)) % 9973 + c.M, dtype=c.xdt)


def nm_addresses(c):
    """made-up base addresses (score, x, mask, y) with the row's alignment, for the host query; 0 = not wanted"""
    return (0x100000 + c.off_score, (0x500000 + c.off_x) if c.want_y else 0, 0x900000 if c.want_mask else 0, 0xD00000 if c.want_y else 0)


def nm_route_of_case(c):
    outer, L, inner = geometry(c)
    return nm_route(CODE[c.sdt], CODE[c.xdt] if c.want_y else 0, CODE[c.mdt] if c.want_mask else 0, CODE[ydt_of(c)] if c.want_y else 0, outer, L,
                    inner, c.ks[0], c.M, *nm_addresses(c))


# --------------------------------------------------------------------------------------------------------- the top-k case table
# kind: how topk_score builds the scores; T: the key the threshold must land on ("nan", or a float; None: not pinned);
# marks: "scan2" = more than 256 chunks (the scan's second round), "cap" = more chunks than the grid cap, "closed" = a closed-form truth
TopkCase = namedtuple("TopkCase", "name kind n n_zeros sdt xdt mdt want_mask want_y off_score off_x T marks")


def topk_chunks(n):
    return -(-n // TOPK_CHUNK)


def _tk(name, kind, n, n_zeros, sdt=T32, xdt=None, mdt=None, want_mask=True, off_score=0, off_x=0, T=None, marks=()):
    return TopkCase(name, kind, n, tuple(n_zeros), sdt, xdt, (mdt or sdt) if want_mask else None, want_mask, xdt is not None, off_score, off_x, T,
                    tuple(marks))


CONST_N = (TOPK_CHUNK * TOPK_SCAN_ROUND + TOPK_CHUNK + 5, TOPK_CHUNK * GRID_CAP + TOPK_CHUNK + 5)
SPARSE_N = 3 * TOPK_CHUNK + 5
SPECIAL_N = 2051
ALIGN_N = 2048 + 9
RADIX_BASE = 0x3F800000
SPECIALS = ("nan", "+inf", "-inf", "zero", "denormal", "allneg")


def _third(n, r):
    """how many i < n have i % 3 == r"""
    return (n - r + 2) // 3


def _const_n_zeros(n):
    R = TOPK_CHUNK * TOPK_SCAN_ROUND
    return (1, 7, 8, 9, 511, 512, 513, 2047, 2048, 2049, R - 1, R, R + 1, n - 1, n)


@functools.lru_cache(maxsize=None)
def topk_table():
    rows = []
    # constant score: every key ties, the whole decision is the index-ordered path; truth arange(n) >= n_zero
    rows.append(_tk("const-scan2", "const", CONST_N[0], _const_n_zeros(CONST_N[0]), xdt=TB16, marks=("scan2", "closed", "large")))
    rows.append(_tk("const-cap", "const", CONST_N[1], _const_n_zeros(CONST_N[1]), marks=("scan2", "cap", "closed", "large")))
    # sparse ties: i % 3 == 0 is T, 1 below, 2 above: uneven per-lane tie counts across wave and chunk edges
    n, below, ties = SPARSE_N, _third(SPARSE_N, 1), _third(SPARSE_N, 0)
    rows.append(_tk("sparse-ties", "sparse", n, [below + r for r in (1, 170, 171, 683, ties - 1)], T=1.0))
    # the threshold on a special key, partial ties, n % 8 != 0
    for sdt in DTYPES:
        for sp in SPECIALS:
            n, r = SPECIAL_N, 300
            nz = {"nan": n - _third(n, 0) + r, "+inf": n - _third(n, 0) + r, "-inf": r, "zero": None, "denormal": _third(n, 1) + r,
                  "allneg": _third(n, 1) + r}[sp]
            if sp == "zero":    # the negative ones of the other two thirds lie below it
                s = topk_score(_tk("", "special:zero", n, (), sdt=sdt)).float()
                nz = int((s < 0).sum()) + r
            (mind, *_), _, _, _ = _BITS[sdt]
            T = {"nan": "nan", "+inf": float("inf"), "-inf": float("-inf"), "zero": 0.0, "denormal": float(from_bits([mind], sdt).float()[0]),
                 "allneg": -1.0}[sp]
            rows.append(_tk(f"special-{sp}-{DT_NAMES[sdt]}", f"special:{sp}", n, (nz,), sdt=sdt, xdt=sdt if sp in ("nan", "zero") else None, T=T))
    # radix digits (float32): bit patterns RADIX_BASE + perm(i) * stride; digits of 11, 11 and 10 bits.  stride 1 with 5000 patterns:
    # the level-0 digit is shared, levels 1 and 2 decide.  stride 2^10: 5000 patterns reach bits 21 and 22, so levels 0 and 1 decide
    # together; with 2048 patterns level 1 decides alone.  stride 2^21: level 0 alone -- 500 patterns, the most that stay finite.
    for count, shift in ((5000, 0), (5000, 10), (2048, 10), (500, 21)):
        for neg in (0, 1):
            nzs = sorted({1, 2, count // 5, 1023 if count > 1100 else 63, 1024 if count > 1100 else 64, 1025 if count > 1100 else 65,
                          count // 2, count - 1, count})
            rows.append(_tk(f"radix-{count}-s{shift}" + ("-neg" if neg else ""), f"radix:{count}:{shift}:{neg}", count, nzs, marks=("closed",)))
    # alignment and dtypes at n = 2048 + 9: heavy ties on a coarse lattice
    n, nzs = ALIGN_N, (ALIGN_N // 3, ALIGN_N // 2 + 1)
    for s in DTYPES:
        eb = 4 if s == T32 else 2
        rows.append(_tk(f"align-score-off-{DT_NAMES[s]}", "lattice", n, nzs, sdt=s, off_score=eb))                 # vec == 0
        rows.append(_tk(f"align-score-off-y-{DT_NAMES[s]}", "lattice", n, nzs, sdt=s, xdt=s, off_score=eb))
        rows.append(_tk(f"align-x-off-{DT_NAMES[s]}", "lattice", n, nzs, sdt=s, xdt=s, want_mask=False, off_x=eb))  # x alone off the grid
        rows.append(_tk(f"mask-only-{DT_NAMES[s]}", "lattice", n, nzs, sdt=s))
        rows.append(_tk(f"y-only-{DT_NAMES[s]}", "lattice", n, nzs, sdt=s, xdt=s, want_mask=False))
        rows.append(_tk(f"both-{DT_NAMES[s]}", "lattice", n, nzs, sdt=s, xdt=s))
    for s, m in ((T32, TB16), (TB16, T32), (T16, TB16)):
        rows.append(_tk(f"mask-{DT_NAMES[m]}-of-{DT_NAMES[s]}", "lattice", n, nzs, sdt=s, mdt=m))
    for x, s in ((TB16, T32), (T32, TB16), (T16, TB16)):
        rows.append(_tk(f"x-{DT_NAMES[x]}-score-{DT_NAMES[s]}", "lattice", n, nzs, sdt=s, xdt=x))
    return tuple(rows)


def radix_perm(count, shift, neg):
    return np.argsort(splitmix64(np.arange(count, dtype=np.uint64), 0xAD1 + shift + 64 * neg), kind="stable").astype(np.int64)


def topk_score(c):
    """the row's scores (CPU, contiguous, the row's score dtype)"""
    n, kind = c.n, c.kind
    i = np.arange(n)
    if kind == "const":
        return torch.ones(n, dtype=c.sdt)
    if kind == "lattice":
        k = (splitmix64(i.astype(np.uint64), 0x7A77) % np.uint64(31)).astype(np.int64) - 15
        return torch.from_numpy(k.astype(np.float32) / 4.0).to(c.sdt)
    if kind.startswith("radix:"):
        _, count, shift, neg = kind.split(":")
        bits = RADIX_BASE + (radix_perm(int(count), int(shift), int(neg)) << int(shift))
        return from_bits(bits | (0x80000000 if int(neg) else 0), T32)
    r = torch.from_numpy(uniform(n, 0x70BC).astype(np.float32))
    m = torch.from_numpy(i % 3)
    if kind == "sparse":
        return torch.where(m == 0, torch.ones(n), torch.where(m == 1, r * 0.75, 1.25 + r)).to(c.sdt)
    sp = kind.split(":")[1]
    (mind, _, _, _, inf, nan), sign, _, _ = _BITS[c.sdt]
    alt = (i // 3) % 2 == 1                                         # every other special carries the sign bit
    if sp in ("nan", "+inf", "-inf", "zero"):
        pat = {"nan": nan, "+inf": inf, "-inf": sign | inf, "zero": 0}[sp]
        special = from_bits(np.where(alt & (sp in ("nan", "zero")), sign | pat, pat), c.sdt)
        other = (r * 4.0 - 2.0).to(c.sdt)
    elif sp == "denormal":                                          # below: negatives, both zeros, the negative denormal; above: normals
        special = from_bits(np.full(n, mind), c.sdt)
        low = torch.stack([-r - 0.5, from_bits(np.full(n, sign | mind), c.sdt).float(), torch.zeros(n), -torch.zeros(n)])
        other = torch.where(m == 1, low[torch.from_numpy((i // 3) % 4), torch.arange(n)], r + 0.5).to(c.sdt)
    else:                                                           # an all-negative tensor, ties at -1
        special = torch.full((n,), -1.0, dtype=c.sdt)
        other = torch.where(m == 1, -1.5 - r, -0.125 - r * 0.5).to(c.sdt)
    return torch.where(m == 0, special, other)


def topk_closed_form(c, n_zero):
    """the keep mask (bool) of the rows marked "closed", None otherwise"""
    if c.kind == "const":
        return torch.arange(c.n) >= n_zero
    if c.kind.startswith("radix:"):
        _, count, shift, neg = c.kind.split(":")
        perm = torch.from_numpy(radix_perm(int(count), int(shift), int(neg)))
        return (perm < c.n - n_zero) if int(neg) else (perm >= n_zero)
    return None


def topk_x(c):
    return make("normal", (c.n,), seed=c.n % 9973 + 1, dtype=c.xdt)


def radix_levels(c):
    """the digit levels (0, 1, 2: bits 31-21, 20-10, 9-0 of the key) in which the scores of a radix row differ"""
    b = topk_score(c).view(torch.int32).numpy().astype(np.int64) & 0xFFFFFFFF
    key = np.where(b & 0x80000000, ~b & 0xFFFFFFFF, b | 0x80000000)
    return tuple(lv for lv, (sh, bits) in enumerate(((21, 11), (10, 11), (0, 10))) if len(np.unique((key >> sh) & ((1 << bits) - 1))) > 1)
