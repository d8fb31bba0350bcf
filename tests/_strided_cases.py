"""Case table of the strided-block BFP kernels (csrc/bfp_slab.hip, bfp_cols.hip, bfp_smallinner.hip) and a restatement, in plain
Python, of the rules by which their launchers accept, refuse and shape a call.  Imported by tests/test_strided_block_cases.py (host
only: the table provably covers every form of the slab kernel), tests/test_gpu_strided_blocks.py and tests/test_gpu_round6.py (the
GPU tests assert through the internal entries' return codes that the restatement still describes the kernels), and run as a
script by the child processes of test_gpu_strided_blocks.py (DMXQ_PLAN_CUS / DMXQ_SLAB_PERSIST are read once per process).

Nothing here needs a GPU to be imported; torch is imported by the functions that use it.

Not covered anywhere, on purpose: the column kernel's 64-bit index form (ColsIdx.small == 0, bfp_cols.hip launch_cols_geom) needs
2^31 lane slots -- at 8 elements per lane and B <= 128 that is a tensor of tens of GiB, more than a test may allocate.  The other
kernels' 64-bit index forms run in tests/test_gpu_large_index.py (table: tests/_large_cases.py), which leaves out, for the same
reason or because they take a process of their own: hist_observer.hip:98 narrow == false (2^32 16-byte vectors), stream.hpp:452 (the
stream kernels' tile count beyond 32 bits) and DMXQ_INPUT_HYPERNET_TILED (read once per process)."""
from collections import namedtuple

ERR_UNSUPPORTED = 2
KIB = 1024
DTYPE_NAMES = ("bf16", "f16")
# (precision, symmetric): 8 / 16 lie on either side of bfp_single_rounding_ok for both 16-bit dtypes (bfp_math.hpp: bf16 <= 14,
# f16 <= 11), symmetric / asymmetric: together with the dtype these select the DT x ASYM x FAST instantiations of every form
VARIANTS = ((8, True), (8, False), (16, True), (16, False))

SlabGeom = namedtuple("SlabGeom", "accepted reason B per Q pitch lds lanes nvl NV nblk tail tiles halved")


def single_rounding_ok(dtype_name, wl):
    return wl <= (14 if dtype_name == "bf16" else 11)


def slab_geometry(outer, L, inner, B, wl=8):
    """dmxq_internal_bfp_slab (csrc/bfp_slab.hip) for a 16-bit tensor, same dtype in and out, nearest rounding, 16-byte aligned
    pointers: what the launcher decides, line by line."""
    def no(reason):
        return SlabGeom(False, reason, B, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, False)
    # :206  inner < 64 || odd || > 2^20 || L < 1 || L > 2^30 || B not a power of two in [8, 256] || wl outside [2, 20]
    if inner < 64 or inner & 1 or inner > (1 << 20) or L < 1 or L > (1 << 30) or B & (B - 1) or B < 8 or B > 256 or wl > 20 or wl < 2:
        return no("scope")
    # :210  while (B > 8 && L <= B / 2) B /= 2
    nominal = B
    while B > 8 and L <= B // 2:
        B //= 2
    # :211  per = B >= 128 ? B / 4 : (B >= 64 ? 16 : 8);  :212  Q = B / per
    per = B // 4 if B >= 128 else (16 if B >= 64 else 8)
    Q = B // per
    # :214  pitch = (inner / 2 + 3) & ~3;  :215  Q > 1: pitch += 4 until pitch % 32 == 32 / Q
    pitch = (inner // 2 + 3) & ~3
    if Q > 1:
        while pitch % 32 != 32 // Q:
            pitch += 4
    # :216  nblk, tail;  :217  lds = B * pitch * 4;  :218  lds > 150 KiB refused
    nblk, tail = (L + B - 1) // B, L % B
    lds = B * pitch * 4
    if lds > 150 * KIB:
        return no("slab over 150 KiB")
    # :220  the three alignment refusals: a full tile, an outer index, a ragged tile must each be whole 16-byte vectors
    if (B * inner) % 8:
        return no("full tile is not whole vectors")
    if outer > 1 and (L * inner) % 8:
        return no("outer index is not whole vectors")
    if (tail * inner) % 8:
        return no("ragged tile is not whole vectors")
    # :221-222  tiles = outer * nblk in [1, 2^31)
    tiles = outer * nblk
    if tiles < 1 or tiles > 0x7FFFFFFF:
        return no("tile count")
    # :226  big = lds > 64 KiB;  :227  threads;  :228  nvl;  :229  nvl > 16 || (big && (nvl > 8 || per == 64)) refused
    lanes = 1024 if lds > 64 * KIB else 256
    nvl = ((B * inner) // 8 + lanes - 1) // lanes
    if nvl > 16 or (lanes == 1024 and (nvl > 8 or per == 64)):
        return no("too many vectors per lane")
    # :247-250  NV: 8 at 1024 lanes; 4 / 8 / 16 at 256
    NV = 8 if lanes == 1024 else (4 if nvl <= 4 else (8 if nvl <= 8 else 16))
    return SlabGeom(True, "", B, per, Q, pitch, lds, lanes, nvl, NV, nblk, tail, tiles, B != nominal)


def block_geometry(outer, L, B):
    """tiles of B rows (after the halving that every strided-block launcher applies) for placing specials in tensors that are not
    the slab kernel's"""
    while B > 8 and L <= B // 2:
        B //= 2
    nblk = (L + B - 1) // B
    return SlabGeom(False, "not a slab case", B, 0, 0, 0, 0, 0, 0, 0, nblk, L % B, outer * nblk, False)


def slab_preferred(inner, B):
    """bfp.hip:200-211 slab_preferred (no DMXQ_SLAB override): :210  (inner * 2) % 128 != 0 && B * inner * 2 >= 16 KiB, with the
    NOMINAL block size; :294 asks it for inner >= 64 only"""
    return inner >= 64 and (inner * 2) % 128 != 0 and B * inner * 2 >= 16 * KIB


def slab_grid_max(cus, lds):
    """upper bound of the persistent grid: slab_resident() caps at 8 workgroups per CU (:197) and a CU has 160 KiB of LDS"""
    return cus * min(8, (160 * KIB) // lds)


def cols_accepts(inner, B, in_itemsize, in_place):
    """dmxq_internal_bfp_cols (bfp_cols.hip:286-296) for aligned pointers and wl <= 22"""
    epl = 16 // in_itemsize
    if inner % epl and (inner < epl or in_place):
        return False
    return B in (8, 16, 32, 64, 128)


def smallinner_accepts(L, inner, B):
    """dmxq_internal_bfp_smallinner (bfp_smallinner.hip:129-143), 16-bit same dtype, nearest, aligned, wl <= 20"""
    if inner < 2 or inner > 63 or L < B or B & (B - 1) or B < 8 or B > 256:
        return False
    tail = L % B
    if tail and ((tail * inner) % 8 or inner < 16 or (L * inner) % 8):
        return False
    return 48 * KIB // ((B * inner + 2) * 2) >= 1


Case = namedtuple("Case", "name rest B outer note")
# Blocks run along dim 1 of [outer, *rest]; `outer` is the small size the table test runs (the loop tests size it themselves).
SLAB_TABLE = [
    # ---- accepted, 256 lanes (slabs up to 64 KiB)
    Case("s256_per16", (128, 14, 14), 64, 3, "B = 64: 16 rows per lane, Q = 4, NV = 8"),
    Case("s256_per16_ragged", (100, 14, 14), 64, 3, "ragged last block of 36 rows"),
    Case("s256_per16_nv4", (64, 10, 10), 64, 2, "12.5 KiB slab, NV = 4: accepted, not preferred (public route: column kernel)"),
    Case("s256_per8_q1", (20, 1030), 8, 3, "B = 8: one lane per column pair, ragged last block of 4 rows"),
    Case("s256_per8_q2", (48, 28, 28), 16, 2, "B = 16: two lanes per column pair"),
    Case("s256_per8_q4", (96, 28, 28), 32, 2, "B = 32: four lanes per column pair, NV = 16"),
    Case("s256_per32_ragged", (192, 14, 14), 128, 2, "B = 128: 32 rows per lane, 192 = 128 + 64"),
    Case("s256_per64", (768, 8, 9), 256, 2, "B = 256: 64 rows per lane (inner 72: the only extents where it fits)"),
    Case("s256_per64_ragged", (740, 8, 9), 256, 2, "B = 256 with a last block of 228 rows"),
    Case("s256_halved", (12, 14, 14), 64, 5, "L = 12 <= B / 2: B halves to 16 (one ragged block of 12 rows), NV = 4"),
    # ---- accepted, 1024 lanes (slabs of 64 .. 150 KiB): the persistent form
    Case("s1024_per16", (512, 28, 28), 64, 1, "98 KiB slab: the shape the kernel was written for"),
    Case("s1024_per16_ragged", (96, 28, 28), 64, 2, "nblk = 2: every other tile is ragged (32 rows)"),
    Case("s1024_per8_q4", (96, 34, 34), 32, 1, "73 KiB slab"),
    Case("s1024_per8_q2", (48, 46, 46), 16, 1, "67 KiB slab"),
    Case("s1024_per8_q1", (24, 4100), 8, 1, "64.1 KiB slab"),
    Case("s1024_per32", (384, 18, 18), 128, 1, "84 KiB slab"),
    Case("s1024_per32_ragged", (320, 18, 18), 128, 1, "84 KiB slab, 320 = 2 x 128 + 64"),
    # ---- refused by the slab kernel: the public route computes them elsewhere
    Case("r_over_cap", (512, 18, 18), 256, 1, "168 KiB slab > 150 KiB (and B = 256 is not the column kernel's either: generic kernel)"),
    Case("r_whole_lines", (64, 56, 56), 64, 2, "394 KiB slab; whole-line rows are the column kernel's anyway"),
    Case("r_rgb", (3, 224, 224), 64, 2, "L = 3: B halves to 8, 784 KiB slab: column kernel"),
    Case("r_ragged_tail_vectors", (69, 14, 14), 64, 2, "last block of 5 rows x 196 = 980 elements: not whole vectors"),
    Case("r_odd_inner", (64, 15, 15), 64, 2, "odd inner: column kernel, unaligned form"),
    Case("r_per64_1024", (256, 12, 12), 256, 2, "B = 256 with a 72 KiB slab would need 1024 lanes x 64 rows: refused"),
]
SLAB_BY_NAME = {c.name: c for c in SLAB_TABLE}

# forms that the accepted cases of SLAB_TABLE must contain (tests/test_strided_block_cases.py): (lanes, PER), (lanes, "NV", n), ...
REQUIRED_FORMS = (
    [("lanes-per", 256, p) for p in (8, 16, 32, 64)] + [("lanes-nv", 256, n) for n in (4, 8, 16)] + [("lanes-q", 256, q) for q in (1, 2, 4)]
    + [("lanes-per-q", 1024, 8, q) for q in (1, 2, 4)] + [("lanes-per", 1024, 16), ("lanes-per", 1024, 32)]
    + [("ragged", 256), ("ragged", 1024), ("halved",)])


def case_geometry(case, outer=None):
    o = case.outer if outer is None else outer
    L = case.rest[0]
    inner = 1
    for s in case.rest[1:]:
        inner *= s
    return o, L, inner, slab_geometry(o, L, inner, case.B)


def forms_of(table):
    """the set of forms (see REQUIRED_FORMS) the ACCEPTED cases of `table` run"""
    forms = set()
    for c in table:
        g = case_geometry(c)[3]
        if not g.accepted:
            continue
        forms |= {("lanes-per", g.lanes, g.per), ("lanes-nv", g.lanes, g.NV), ("lanes-q", g.lanes, g.Q), ("lanes-per-q", g.lanes, g.per, g.Q)}
        if g.tail:
            forms.add(("ragged", g.lanes))
        if g.halved:
            forms.add(("halved",))
    return forms


def outer_for(case, min_tiles, grid_max):
    """smallest outer with at least `min_tiles` tiles and a tile count that is no multiple of `grid_max` (uneven trip counts)"""
    nblk = case_geometry(case)[3].nblk
    o = max(1, -(-min_tiles // nblk))
    if nblk % grid_max == 0:      # (every tile count is a multiple of the grid: nothing to choose)
        return o
    while (o * nblk) % grid_max == 0:
        o += 1
    return o


# ------------------------------------------------------------------------------------------------ inputs: specials placed by TILE
def tile_rows(t, g, L):
    """tile index -> (outer index, first row, rows) as slab_tile() (bfp_slab.hip:46-54) decomposes it"""
    o, blk = divmod(t, g.nblk)
    r0 = blk * g.B
    return o, r0, min(g.B, L - r0)


def literal_tile(t):
    """about every other tile, in no pattern that a grid size divides, carries a NaN block (the literal path)"""
    return ((t * 0x9E3779B1) >> 13) & 1 == 1


def literal_tiles(tiles, grids, always=()):
    """the set of tiles that carry a NaN block: literal_tile(), adjusted so that for EVERY persistent grid size in `grids` some
    workgroup runs literal -> fast -> literal and another fast -> literal -> fast tiles back to back (t, t + grid, t + 2 grid)"""
    pinned = {t: True for t in always}           # (tiles that carry specials, a NaN among them, whatever this decides)
    lit = lambda t: pinned.get(t, literal_tile(t))
    for g in grids:
        assert tiles > 2 * g, (tiles, g)
        for pat in ((True, False, True), (False, True, False)):
            ts = [t for t in range(tiles - 2 * g) if all(lit(t + k * g) == pat[k] for k in range(3))]
            if not ts:
                ts = [t for t in range(tiles - 2 * g) if all(pinned.get(t + k * g, pat[k]) == pat[k] for k in range(3))]
            assert ts, (tiles, g, pat)
            for k in range(3):
                pinned[ts[0] + k * g] = pat[k]
    return {t for t in range(tiles) if lit(t)}


def plant_specials(x3, g, special_tiles, nan_tiles):
    """x3: the [outer, L, inner] view of the input, edited in place.  special_tiles get an all-zero block, a block with a denormal
    maximum, Inf, NaN and the largest finite values; nan_tiles one NaN at a tile-dependent place."""
    import torch
    bf = x3.dtype == torch.bfloat16
    big, den = (3.0e38, 1e-40) if bf else (65504.0, 6e-8)
    L, inner = x3.shape[1], x3.shape[2]
    c = lambda k: k % inner                          # (inner extents of 3 / 9 fold the columns onto each other: still specials)
    for t in special_tiles:
        o, r0, rows = tile_rows(t, g, L)
        x3[o, r0:r0 + rows, c(0)] = 0.0              # all-zero block ...
        x3[o, r0:r0 + rows, c(1)] = den              # ... sharing its lane with a block whose maximum is a denormal
        x3[o, r0:r0 + rows, c(8)] = 0.0              # all-zero block next to an ordinary one
        x3[o, r0:r0 + rows, c(11)] = -den
        x3[o, r0 + rows // 2, c(11)] = 3 * den
        x3[o, r0 + rows // 2, c(2)] = float("inf")
        x3[o, r0, c(6)] = big
        x3[o, r0 + rows - 1, inner - 1] = -big
        x3[o, r0, c(inner + 61)] = float("-inf")
        x3[o, r0 + rows - 1, c(5)] = float("nan")
    for t in nan_tiles:
        o, r0, rows = tile_rows(t, g, L)
        x3[o, r0 + (t * 40503) % rows, c(12 + t * 2654435761)] = float("nan")


def nan_in_tiles(want3, g, tiles):
    import torch
    L = want3.shape[1]
    for t in tiles:
        o, r0, rows = tile_rows(t, g, L)
        if not bool(torch.isnan(want3[o, r0:r0 + rows].float()).any()):
            return False
    return True


def loop_input(case, outer, dtype, grid_max, grid_candidates, seed=0, base=None):
    """heavy-tailed [outer, *rest] tensor for a persistent-loop run: special blocks in the first tile of the second round, in a
    later tile and in the last (ragged, where L % B != 0) tile; NaN blocks in every literal_tile()"""
    import torch

    from _data import make_chunked
    o, L, inner, g = case_geometry(case, outer)
    if not g.accepted:
        g = block_geometry(outer, L, case.B)
    x = (make_chunked("heavy", (outer, L, inner), seed, torch.float32) if base is None else base)
    if dtype == torch.float16:
        x = x.clamp(-65504.0, 65504.0)
    x = x.to(dtype)
    specials = sorted({min(grid_max, g.tiles - 1), min(grid_max + 1, g.tiles - 1), min(2 * grid_max + 1, g.tiles - 1), g.tiles - 1})
    nans = sorted(literal_tiles(g.tiles, grid_candidates, specials) - set(specials))
    plant_specials(x, g, specials, nans)
    return x.reshape((outer,) + tuple(case.rest)), g, specials, nans


# ------------------------------------------------------------------------------------------------ the internal entries
def entry(lib, kernel, src, dst, outer, L, inner, B, wl, sym):
    """dmxq_internal_bfp_{slab,cols,smallinner} on torch's current stream; returns the status code"""
    import ctypes

    import torch

    from dmx_compressor_amd import _lib
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    fn = getattr(lib, "dmxq_internal_bfp_" + kernel)
    head = [vp, vp, i32, i32, i64, i64, i64, i64, i32, i32, i32]
    fn.argtypes = head + ([ctypes.c_uint64, vp] if kernel == "cols" else [vp])
    fn.restype = i32
    s = vp(torch.cuda.current_stream().cuda_stream)
    args = (vp(src.data_ptr()), vp(dst.data_ptr()), _lib.dtype_code(src.dtype), _lib.dtype_code(dst.dtype), outer, L, inner, B, wl, 2, int(sym))
    return fn(*args, 0, s) if kernel == "cols" else fn(*args, s)


def mismatches(got, want):
    """mismatches_nan_aware(got, want), with a short cut for large tensors: identical bit patterns are zero mismatches"""
    import torch

    from _data import mismatches_nan_aware
    if got.dtype == want.dtype and got.shape == want.shape:
        it = {2: torch.int16, 4: torch.int32}[got.element_size()]
        if torch.equal(got.contiguous().view(it), want.to(got.device).contiguous().view(it)):
            return 0
    return mismatches_nan_aware(got, want)


def check_slab_loop(dmx, oracle, case, x, g, dtype, variants, tag):
    """one looped slab case: public route, the slab entry out of place and in place (out == in), the column kernel's entry, each
    against the oracle"""
    import torch
    lib = dmx._lib.lib()
    dev = torch.device("cuda:0")
    xd = x.to(dev)
    outer, L, inner = dmx._lib.split3(x.shape, 1)
    assert slab_preferred(inner, case.B)
    for wl, sym in variants:
        want = oracle.bfp_cast(x, wl, case.B, 1, sym).to(dtype)
        what = (tag, case.name, tuple(x.shape), str(dtype), wl, sym)
        assert mismatches(dmx.ops.bfp_qdq(xd, wl, case.B, 1, sym), want) == 0, ("public",) + what
        out = torch.zeros_like(xd)
        assert entry(lib, "slab", xd, out, outer, L, inner, case.B, wl, sym) == 0, what
        assert mismatches(out, want) == 0, ("slab",) + what
        t = xd.clone()
        assert entry(lib, "slab", t, t, outer, L, inner, case.B, wl, sym) == 0, what
        assert mismatches(t, want) == 0, ("slab in place",) + what
        if cols_accepts(inner, case.B, 2, False):
            out.zero_()
            assert entry(lib, "cols", xd, out, outer, L, inner, case.B, wl, sym) == 0, what
            assert mismatches(out, want) == 0, ("cols",) + what
    return want


def child_main(mode):
    """the body of one child process of tests/test_gpu_strided_blocks.py (its environment selects the plan)"""
    import os
    import sys

    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import dmx_compressor_amd as dmx
    import oracle as O
    O.build()
    cus = int(os.environ.get("DMXQ_PLAN_CUS", "0"))
    lanes = 256 if mode == "persist256" else 1024
    n = 0
    for case in SLAB_TABLE:
        g0 = case_geometry(case)[3]
        if not g0.accepted or g0.lanes != lanes or not slab_preferred(case_geometry(case)[2], case.B):
            continue
        if mode == "persist0":       # one tile per workgroup: any grid
            gm, outer = 1, max(2, -(-7 // g0.nblk))
        else:
            assert cus > 0
            gm = slab_grid_max(cus, g0.lds)
            outer = outer_for(case, max(6 * gm + 1, 49 if mode == "persist256" else 0), gm)   # (3 x grid_max + 1 asked; twice that leaves room to place the tile patterns)
        for dtype in (torch.bfloat16, torch.float16):
            x, g, specials, nans = loop_input(case, outer, dtype, gm, [k * cus for k in range(1, 9) if k * cus <= gm] if cus else [], seed=len(case.name) + case.B)
            if mode != "persist0":
                assert g.tiles >= 3 * gm + 1 and max(specials) >= gm and (g.tiles % gm != 0 or g.nblk % gm == 0)
            want = check_slab_loop(dmx, O, case, x, g, dtype, VARIANTS, mode)
            assert nan_in_tiles(want.reshape(x.shape[0], x.shape[1], -1), g, specials + nans[:64])
            n += 1
            print(f"ok {mode} cus={cus} {case.name} {str(dtype)} outer={outer} tiles={g.tiles} grid_max={gm} min_trips={g.tiles // gm}", flush=True)
    torch.cuda.synchronize()
    print(f"OK {n}")


if __name__ == "__main__":
    import sys
    child_main(sys.argv[1])
