"""SBFP and MXFP (csrc/blockfmt.hip: dmxq_sbfp_qdq, dmxq_mxfp_qdq) on every block class, kernel path and dtype pair of
tests/_blockfmt_cases.py, bit-exact against the oracle: NaN positions agree and -0.0 differs from +0.0.  The host half
(tests/test_blockfmt_cases_host.py) proves that the tables hold every class at every position of a wave and that the oracle equals a
plain-torch restatement of the reference's casts on them; here the kernels' three MXFP paths (x-domain, general with the branch-free
element form, general per element) and SBFP's packed and redo paths have to agree with it."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _blockfmt_cases as C
from _data import mismatches_nan_aware

pytestmark = pytest.mark.gpu

KINDS = [(k, f) for k in ("mxfp", "sbfp") for f in C.FORMATS[k]]
IDS = [f"{k}-{'-'.join(str(int(v)) for v in f)}" for k, f in KINDS]
PAIRS = [("bf16", "bf16"), ("f16", "f16"), ("f32", "f32"), ("bf16", "f32"), ("f16", "f32"), ("f32", "bf16"), ("f32", "f16")]   # blockfmt.hip:227-233


@functools.lru_cache(maxsize=None)
def planted(kind, f, dtn, B, rows=None, width=None):
    return C.planted(kind, f, C.DTYPES[dtn], B, rows, width)


def compare(got, want, what, rows_class=None):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = mismatches_nan_aware(got, want)
    if bad:
        g, w = got.detach().cpu().float(), want.float()
        diff = ((g.view(torch.int32) != w.view(torch.int32)) & ~(torch.isnan(g) & torch.isnan(w))).reshape(g.shape[0], -1)
        rows = diff.any(-1).nonzero().flatten().tolist()
        where = sorted({rows_class[r] for r in rows}) if rows_class is not None else rows[:8]
        i = diff.reshape(-1).nonzero().flatten()[0].item()
        assert bad == 0, (what, bad, "classes / rows:", where, "first:", i, float(g.reshape(-1)[i]), float(w.reshape(-1)[i]))


def check(kind, dmx, oracle, cuda, x, f, B, dim=-1, out_dtype=None, what=(), rows_class=None):
    assert x.numel() > 0, what                                                          # (no case may be empty)
    want = C.ref(kind, oracle, x, f, B, dim).to(out_dtype or x.dtype).contiguous()     # (float32 reference rounded once)
    got = C.run_lib(kind, dmx.ops, x.to(cuda), f, B, dim, out_dtype)
    compare(got, want, (kind, tuple(f), str(x.dtype), tuple(x.shape), B, dim) + tuple(what), rows_class)
    return want


@pytest.mark.parametrize("dtn", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("kind,f", KINDS, ids=IDS)
def test_uniform_waves(dmx, oracle, cuda, kind, f, dtn):
    """every class in whole waves of its own: [4 * n_classes, one wave], B = 32"""
    dt = C.DTYPES[dtn]
    t = C.uniform(kind, f, dt, 32)
    assert t.x.shape == (4 * len(C.class_list(kind, f, dt)), C.elements_per_wave(dt))
    check(kind, dmx, oracle, cuda, t.x, f, 32, rows_class=t.rows_class)


@pytest.mark.parametrize("B", [32, 16])
@pytest.mark.parametrize("dtn", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("kind,f", KINDS, ids=IDS)
def test_mixed_waves(dmx, oracle, cuda, kind, f, dtn, B):
    """one block of every class at every block position of a wave of ordinary blocks (two waves per row): the ordinary blocks of such
    a wave take the general path and must agree with the x-domain path the same data takes elsewhere"""
    dt = C.DTYPES[dtn]
    t = planted(kind, f, dtn, B)
    assert t.x.shape[0] == 2 * t.blocks_per_wave * len(C.class_list(kind, f, dt)) and t.x.shape[1] == 2 * C.elements_per_wave(dt)
    want = check(kind, dmx, oracle, cuda, t.x, f, B, rows_class=t.rows_class)
    if kind == "mxfp":   # the ordinary data alone (every wave x-domain, where the format has the path) gives the same bits for the ordinary blocks
        o = C.from_bits(C.ordinary(kind, f, dt, t.x.shape[0], t.x.shape[1] // B, B), dt)
        alone = C.run_lib(kind, dmx.ops, o.to(cuda), f, B).cpu()
        keep = torch.ones(t.x.shape[0], t.x.shape[1] // B, dtype=torch.bool)
        for r, k, _, _ in t.plan:
            keep[r, k] = False
        keep = keep[:, :, None].expand(-1, -1, B).reshape(t.x.shape)
        assert mismatches_nan_aware(alone[keep], want[keep]) == 0


@pytest.mark.parametrize("dtn", ["bf16", "f16"])
@pytest.mark.parametrize("kind,f", KINDS, ids=IDS)
def test_every_16_bit_pattern(dmx, oracle, cuda, kind, f, dtn):
    """all 65,536 patterns as the non-maximum elements of blocks of 32 whose element 0 is a chosen maximum (the patterns of magnitude
    up to it); NaN and Inf patterns in blocks of their own"""
    dt = C.DTYPES[dtn]
    maxima = C.mxfp_pattern_maxima(f, dt) if kind == "mxfp" else C.sbfp_pattern_maxima(f, dt)
    assert len(maxima) == C.n_pattern_maxima(kind, f, dt), [hex(m) for m in maxima]     # (maxima the dtype does not hold exactly drop out)
    parts = [C.pattern_blocks(m, dt) for m in maxima] + [C.nonfinite_blocks(dt)]
    names = sum(([hex(m)] * p.shape[0] for m, p in zip(maxima + [dt.inf], parts)), [])
    x = C.from_bits(np.concatenate(parts), dt)
    check(kind, dmx, oracle, cuda, x, f, 32, rows_class=names)


@pytest.mark.parametrize("f", C.MXFP_FORMATS, ids=[f"{f.man}-{f.exp}" for f in C.MXFP_FORMATS])
def test_float32_denormal_maxima_near_powers_of_two(dmx, oracle, cuda, f):
    """mxfp_block_scale's denormal branch: maxima k 2^-149 at and just below every power of two, on both sides of the point where the
    reference's float32 log2 rounds up to the integer; rows path and generic kernel"""
    x, ks = C.float32_denormal_blocks()
    names = [hex(k) for k in ks]
    check("mxfp", dmx, oracle, cuda, x, f, 32, rows_class=names)
    check("mxfp", dmx, oracle, cuda, x[:, :24].contiguous(), f, 24, rows_class=names)


@pytest.mark.parametrize("kind,f", KINDS, ids=IDS)
def test_dtype_pairs(dmx, oracle, cuda, kind, f):
    """the seven instantiations of dispatch_blockfmt on the mixed-wave tensor; the widening pairs run kFixedVector (8 elements in,
    32 bytes out per lane)"""
    for i, o in PAIRS:
        t = planted(kind, f, i, 32)
        check(kind, dmx, oracle, cuda, t.x, f, 32, out_dtype=C.DTYPES[o].torch, what=(i, o), rows_class=t.rows_class)


@pytest.mark.parametrize("dtn", ["bf16", "f32"])
@pytest.mark.parametrize("kind,f", KINDS, ids=IDS)
def test_block_sizes_and_generic_kernel(dmx, oracle, cuda, kind, f, dtn):
    """one lane per block, two, a whole wave; the generic kernel for B = 128 * EPL, B = 20 / 24, ragged rows and inner > 1 -- each on
    planted data"""
    dt = C.DTYPES[dtn]
    e = C.epl(dt)
    for B, rows_kernel in ((e, True), (2 * e, True), (64 * e, True), (128 * e, False), (20, False), (24, False)):
        bpw = max(1, C.elements_per_wave(dt) // B)
        t = planted(kind, f, dtn, B, bpw, bpw * B * 2)
        assert C.rows_path(t.x.shape[1], 1, B, dt) == rows_kernel
        check(kind, dmx, oracle, cuda, t.x, f, B, what=("B",), rows_class=t.rows_class)
    t = planted(kind, f, dtn, 32, 4, 2 * C.elements_per_wave(dt))
    ragged = t.x[:, :t.x.shape[1] - 13].contiguous()                                        # L % B != 0
    assert not C.rows_path(ragged.shape[1], 1, 32, dt)
    check(kind, dmx, oracle, cuda, ragged, f, 32, what=("ragged",), rows_class=t.rows_class)
    for inner, dim, nblk, B in ((5, -2, 4, 32), (48, 1, 11, 16)):
        x3, rows_class = C.planted_inner(kind, f, dt, B, inner, nblk)                      # [outer, L, inner], blocks along dim 1
        assert x3.shape[0] >= 2 and x3.shape[2] == inner and set(rows_class) == {c for c, _ in C.class_list(kind, f, dt)}
        assert not C.rows_path(x3.shape[1], inner, B, dt)
        want = C.ref(kind, oracle, x3, f, B, dim).to(dt.torch).contiguous()
        got = C.run_lib(kind, dmx.ops, x3.to(cuda), f, B, dim)
        assert got.shape == x3.shape
        compare(C.rows_of(got.cpu()), C.rows_of(want), (kind, tuple(f), dtn, tuple(x3.shape), B, dim, "inner", inner), rows_class)


@pytest.mark.parametrize("dtn", ["bf16", "f32"])
@pytest.mark.parametrize("kind,f", KINDS, ids=IDS)
def test_tiles(dmx, oracle, cuda, kind, f, dtn):
    """one block only; and three tiles of the streaming skeleton plus five blocks -- the last wave partly filled --, special blocks in
    the last wave and on both sides of each tile seam"""
    dt = C.DTYPES[dtn]
    B = 32
    for cls, reps in C.class_list(kind, f, dt):
        for i, rep in enumerate(reps):
            x = C.from_bits(C.make_block(kind, f, dt, cls, rep, B, 11 + i)[None, :], dt)
            check(kind, dmx, oracle, cuda, x, f, B, what=("one block", cls, hex(rep)))
    tb = C.TILE_VECTORS[kind] * C.epl(dt) // B                                              # blocks per tile
    nblk = 3 * tb + 5
    assert nblk * B <= 1 << 20
    where = [0, tb - 1, tb, 2 * tb - 1, 2 * tb, 3 * tb - 1] + [3 * tb + i for i in range(5)]
    t = C.planted_at(kind, f, dt, B, nblk, where)
    assert len({c for _, _, c, _ in t.plan}) == len(C.class_list(kind, f, dt)) - 1           # every class but the ordinary one is planted
    check(kind, dmx, oracle, cuda, t.x, f, B, what=("tiles",))
    check(kind, dmx, oracle, cuda, t.x.reshape(1, -1), f, B, what=("tiles, one row",))


@pytest.mark.parametrize("dtn", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("kind", ["mxfp", "sbfp"])
def test_in_place_and_unaligned(dmx, oracle, cuda, kind, dtn):
    """through include/dmxq.h: out == in for the three same-dtype pairs, and a contiguous view one element into its allocation, on the
    rows path and on the generic kernel"""
    from dmx_compressor_amd import _lib
    L = _lib.lib()
    vp = ctypes.c_void_p
    dt = C.DTYPES[dtn]
    code = _lib.dtype_code(dt.torch)

    def call(f, src, dst, outer, Ld, inner, B):
        s = vp(torch.cuda.current_stream().cuda_stream)
        if kind == "mxfp":
            return L.dmxq_mxfp_qdq(vp(src.data_ptr()), vp(dst.data_ptr()), code, code, outer, Ld, inner, B, f.man, f.exp, s)
        return L.dmxq_sbfp_qdq(vp(src.data_ptr()), vp(dst.data_ptr()), code, code, outer, Ld, inner, B, f.p, int(f.clamp), int(f.symmetric),
                               f.man, f.exp, f.bias, int(f.flush), s)

    for f in C.FORMATS[kind][:2] + C.FORMATS[kind][-1:]:
        for B, width, rows_kernel in ((32, 2 * C.elements_per_wave(dt), True), (24, 24 * 20, False)):
            t = planted(kind, f, dtn, B, 3, width)
            x = t.x
            assert C.rows_path(x.shape[1], 1, B, dt) == rows_kernel
            want = C.ref(kind, oracle, x, f, B).to(dt.torch)
            what = (kind, tuple(f), dtn, B)
            buf = x.to(cuda)
            assert call(f, buf, buf, x.shape[0], x.shape[1], 1, B) == 0
            compare(buf, want, ("in place",) + what, t.rows_class)
            for in_place in (False, True):
                store = torch.zeros(x.numel() + 8, dtype=dt.torch, device=cuda)
                view = store[1:1 + x.numel()].reshape(x.shape)
                view.copy_(x)
                assert view.data_ptr() % 16 == dt.itemsize and view.is_contiguous()
                out = view if in_place else torch.zeros(x.numel() + 8, dtype=dt.torch, device=cuda)[1:1 + x.numel()].reshape(x.shape)
                assert call(f, view, out, x.shape[0], x.shape[1], 1, B) == 0
                compare(out, want, ("unaligned", in_place) + what, t.rows_class)
                assert float(store[0]) == 0.0 and bool((store[1 + x.numel():] == 0).all())   # nothing written outside the view
