"""-m gpu: the three strided-block BFP kernels (csrc/bfp_slab.hip, bfp_cols.hip, bfp_smallinner.hip) against the CPU oracle, with the
kernel that ran KNOWN: every case goes through the public route (dmx.ops.bfp_qdq) and through the internal entry of the kernel it is
meant for, whose return code is asserted (0, or DMXQ_ERR_UNSUPPORTED where the case shows a refusal).  The case table and the
restatement of the launch rules are tests/_strided_cases.py; tests/test_strided_block_cases.py proves on the host that the table
holds every form of the slab kernel.  Here: the table on the device; grids with more tiles than resident workgroups (the persistent
loop of the 1024-lane slab kernel: in process on the device's own CU count, and in child processes planned for 2 / 3 CUs); the
shapes of tools/bench_conv_shapes.py and of the Whisper Conv1d stem at their real sizes.  Comparisons are bit-exact
(mismatches_nan_aware == 0).  Not here: the column kernel's 64-bit index form (see _strided_cases.py)."""
import os
import subprocess
import sys

import pytest
import torch

import _strided_cases as S
from _data import make_chunked

pytestmark = pytest.mark.gpu
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("case", S.SLAB_TABLE, ids=[c.name for c in S.SLAB_TABLE])
def test_slab_table_case_runs_the_kernel_it_names(dmx, cuda, oracle, case, dtype):
    """accepted by the restatement <=> dmxq_internal_bfp_slab returns 0 (else DMXQ_ERR_UNSUPPORTED); oracle bits from the slab entry out
    of place and in place, from the public route, and from the column kernel's entry (the fallback of a slab launch that cannot be made)"""
    lib = dmx._lib.lib()
    x, g, specials, nans = S.loop_input(case, case.outer, dtype, 0, [], seed=case.B + case.rest[0])
    outer, L, inner = dmx._lib.split3(x.shape, 1)
    accepted = S.slab_geometry(outer, L, inner, case.B).accepted
    assert accepted == (not case.name.startswith("r_"))
    xd = x.to(cuda)
    for wl, sym in S.VARIANTS:
        want = oracle.bfp_cast(x, wl, case.B, 1, sym).to(dtype)
        assert S.nan_in_tiles(want.reshape(outer, L, inner), g if accepted else S.block_geometry(outer, L, case.B), specials)
        what = (case.name, wl, sym)
        assert S.mismatches(dmx.ops.bfp_qdq(xd, wl, case.B, 1, sym), want) == 0, ("public",) + what
        out = torch.zeros_like(xd)
        rc = S.entry(lib, "slab", xd, out, outer, L, inner, case.B, wl, sym)
        assert rc == (0 if accepted else S.ERR_UNSUPPORTED), what
        if accepted:
            assert S.mismatches(out, want) == 0, ("slab",) + what
            t = xd.clone()
            assert S.entry(lib, "slab", t, t, outer, L, inner, case.B, wl, sym) == 0
            assert S.mismatches(t, want) == 0, ("slab in place",) + what
        out.zero_()
        rc = S.entry(lib, "cols", xd, out, outer, L, inner, case.B, wl, sym)
        assert rc == (0 if S.cols_accepts(inner, case.B, 2, False) else S.ERR_UNSUPPORTED), what
        if rc == 0:
            assert S.mismatches(out, want) == 0, ("cols",) + what


# ------------------------------------------------------------------------------------------------ more tiles than the grid, in process
_LOOP = [("s1024_per16", BF16), ("s1024_per16", F16), ("s1024_per8_q1", BF16), ("s1024_per32_ragged", F16)]


@pytest.mark.parametrize("name,dtype", _LOOP, ids=[f"{n}-{str(d)[6:]}" for n, d in _LOOP])
def test_slab_persistent_loop_on_this_device(dmx, cuda, oracle, name, dtype):
    """1024-lane cases sized from the device's CU count: tiles >= 2.5 x grid_max and no multiple of it, so every workgroup of the
    one-round grid loops and trip counts differ.  grid_max = CUs x min(8, 160 KiB / slab) bounds the launcher's grid from above."""
    case = S.SLAB_BY_NAME[name]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    g0 = S.case_geometry(case)[3]
    gm = S.slab_grid_max(cus, g0.lds)
    outer = S.outer_for(case, -(-5 * gm // 2), gm)
    x, g, specials, nans = S.loop_input(case, outer, dtype, gm, [k * cus for k in range(1, 9) if k * cus <= gm], seed=7)
    assert g.lanes == 1024 and 2 * g.tiles >= 5 * gm and g.tiles % gm != 0 and max(specials) >= gm and specials[-1] == g.tiles - 1
    print(f"{name} {dtype} CUs={cus} outer={outer} tiles={g.tiles} grid_max={gm} min_trips={g.tiles // gm}")
    want = S.check_slab_loop(dmx, oracle, case, x, g, dtype, ((8, True), (8, False), (16, False)), "loop")
    assert S.nan_in_tiles(want.reshape(outer, x.shape[1], -1), g, specials + [t for t in nans if t >= gm][:32] + nans[:32])


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_slab_on_64_512_28_28(dmx, cuda, oracle, dtype):
    """the shape the slab kernel was written for and that the benchmarks time: 512 tiles of 98 KiB"""
    case = S.SLAB_BY_NAME["s1024_per16"]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    x, g, specials, nans = S.loop_input(case, 64, dtype, cus, [], seed=11)
    assert g.tiles == 512
    want = S.check_slab_loop(dmx, oracle, case, x, g, dtype, ((8, True), (8, False)), "64x512x28x28")
    assert S.nan_in_tiles(want.reshape(64, 512, -1), g, specials + nans[-16:])


# ------------------------------------------------------------------------------------------------ ... in child processes
def _child(mode, env_add, timeout):
    env = dict(os.environ, **env_add)
    for k in ("DMXQ_SLAB", "DMXQ_SLAB_PERSIST", "DMXQ_PLAN_CUS"):
        if k not in env_add:
            env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_strided_cases.py"), mode], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=timeout)
    print(p.stdout)
    assert p.returncode == 0 and "\nOK " in p.stdout, (mode, env_add, p.returncode, p.stdout[-1500:], p.stderr[-3000:])
    return int(p.stdout.rsplit("\nOK ", 1)[1].split()[0])


def test_slab_persistent_loop_planned_for_three_and_two_cus(cuda):
    """DMXQ_PLAN_CUS=3 / 2 (read once per process: child processes): every 1024-lane case of the table with at least 3 x grid_max + 1
    tiles, both dtypes, every variant, out of place and in place.  With 3 CUs the grid is odd: on s1024_per16_ragged (nblk = 2) every
    workgroup alternates between a full and a ragged tile, in both orders.  The first child that fails ends the test."""
    n_cases = sum(1 for c in S.SLAB_TABLE if S.case_geometry(c)[3].accepted and S.case_geometry(c)[3].lanes == 1024)
    assert n_cases == 7
    for cus in ("3", "2"):
        assert _child("plan_cus", {"DMXQ_PLAN_CUS": cus}, 420) == 2 * n_cases


def test_slab_forced_persistent_256_lanes_and_one_tile_per_workgroup_1024(cuda):
    """DMXQ_SLAB_PERSIST=1 DMXQ_PLAN_CUS=2: the same loop in the 256-lane builds (grid <= 16, at least 49 tiles), every preferred 256-lane
    case of the table; then DMXQ_SLAB_PERSIST=0 on the 1024-lane cases (one tile per workgroup)"""
    n256 = sum(1 for c in S.SLAB_TABLE if S.case_geometry(c)[3].accepted and S.case_geometry(c)[3].lanes == 256 and S.slab_preferred(S.case_geometry(c)[2], c.B))
    assert n256 == 9
    assert _child("persist256", {"DMXQ_SLAB_PERSIST": "1", "DMXQ_PLAN_CUS": "2"}, 420) == 2 * n256
    assert _child("persist0", {"DMXQ_SLAB_PERSIST": "0"}, 420) == 14


# ------------------------------------------------------------------------------------------------ the three kernels at real shapes
REAL = [
    # shape, dim, B, kernel meant, dtypes
    ((256, 1024, 14, 14), 1, 64, "slab", (BF16,)),            # slab, 256 lanes, 4096 tiles
    ((64, 1024, 14, 14), 1, 64, "slab", (F16,)),              # ... 1024 tiles
    ((64, 256, 56, 56), 1, 64, "cols", (BF16, F16)),          # whole-line rows: RPL 8 x RS 8
    ((64, 3, 224, 224), 1, 64, "cols", (BF16, F16)),          # L = 3
    ((64, 2048, 7, 7), 1, 64, "smallinner", (BF16, F16)),     # inner 49, LPB = 4
    ((64, 2048, 7, 7), 1, 16, "smallinner", (F16,)),          # LPB = 1
    ((512, 512, 3, 3), 1, 64, "smallinner", (BF16, F16)),     # inner 9
    ((512, 512, 3, 3), 1, 16, "smallinner", (BF16,)),
    ((1280, 1280, 3), 1, 64, "smallinner", (BF16, F16)),      # inner 3
    ((1280, 1280, 3), 1, 16, "smallinner", (F16,)),
    ((8, 12, 1500, 64), -2, 64, "cols", (BF16, F16)),         # attention operands along the sequence, ragged 1500
    ((8, 32, 2048, 128), -2, 64, "cols", (BF16,)),
    ((8, 32, 2048, 128), -2, 128, "cols", (F16,)),
    ((4, 80, 3000), 1, 64, "cols", (F32, BF16)),              # Whisper Conv1d stem: ragged 80 = 64 + 16
    ((2, 768, 3000), 1, 64, "cols", (F32, BF16)),
]
_base = {}


def _real_input(shape, dtype):
    """one float32 generation per shape (kept for the module), dtypes sliced from it; specials in the second, a middle and the last tile"""
    if shape not in _base:
        _base.clear()                                          # (neighbouring cases share a shape: one tensor alive at a time)
        _base[shape] = make_chunked("heavy", shape, seed=len(shape) + shape[1], dtype=F32)
    x = _base[shape]
    if dtype == F16:
        x = x.clamp(-65504.0, 65504.0)
    return x.to(dtype)


@pytest.mark.parametrize("shape,dim,B,kernel,dtypes", REAL, ids=[f"{'x'.join(map(str, s))}-B{b}-{k}" for s, d, b, k, _ in REAL])
def test_strided_kernels_at_real_shapes(dmx, cuda, oracle, shape, dim, B, kernel, dtypes):
    lib = dmx._lib.lib()
    outer, L, inner = dmx._lib.split3(shape, dim)
    sg = S.slab_geometry(outer, L, inner, B)
    meant = {"slab": sg.accepted and S.slab_preferred(inner, B), "smallinner": S.smallinner_accepts(L, inner, B),
             "cols": S.cols_accepts(inner, B, 2, True) and not (sg.accepted and S.slab_preferred(inner, B)) and inner >= 64}[kernel]
    assert meant, "the table no longer describes the routing"
    bg = S.block_geometry(outer, L, B)
    specials = [1, bg.tiles // 2, bg.tiles - 1]
    for dtype in dtypes:
        x = _real_input(shape, dtype).clone()
        if dtype != F32:
            S.plant_specials(x.reshape(outer, L, inner), bg, specials, [t for t in range(0, bg.tiles, 97)])
        else:
            x.reshape(outer, L, inner)[0, 0, 5] = float("nan")
        xd = x.to(cuda)
        for wl, sym in ((8, True), (8, False)):
            want = oracle.bfp_cast(x, wl, B, dim, sym).to(dtype)
            assert dtype == F32 or S.nan_in_tiles(want.reshape(outer, L, inner), bg, specials)
            what = (shape, dim, B, kernel, str(dtype), wl, sym)
            assert S.mismatches(dmx.ops.bfp_qdq(xd, wl, B, dim, sym), want) == 0, ("public",) + what
            out = torch.zeros_like(xd)
            for k in ("slab", "smallinner", "cols"):
                accepts = {"slab": sg.accepted, "smallinner": S.smallinner_accepts(L, inner, B), "cols": S.cols_accepts(inner, B, x.element_size(), False)}[k]
                if dtype == F32 and k != "cols":
                    accepts = False
                if k != kernel and not (k == "cols" and kernel == "slab") and accepts:
                    continue                                   # (accepted, but neither the kernel meant nor its fallback: not this test's)
                out.zero_()
                rc = S.entry(lib, k, xd, out, outer, L, inner, B, wl, sym)
                assert rc == (0 if accepts else S.ERR_UNSUPPORTED), (k,) + what
                if rc == 0:
                    assert S.mismatches(out, want) == 0, (k,) + what
            if dtype != F32 and (kernel != "cols" or S.cols_accepts(inner, B, 2, True)):
                t = xd.clone()                                 # in place through the entry of the kernel meant
                assert S.entry(lib, kernel, t, t, outer, L, inner, B, wl, sym) == 0, what
                assert S.mismatches(t, want) == 0, ("in place",) + what
        if dtype == BF16:                                      # one widening run per shape
            want = oracle.bfp_cast(x, 8, B, dim, True).float()
            got = dmx.ops.bfp_qdq(xd, 8, B, dim, True, out_dtype=F32)
            assert got.dtype == F32 and S.mismatches(got, want) == 0, ("widening", shape, dim, B)
    del xd
