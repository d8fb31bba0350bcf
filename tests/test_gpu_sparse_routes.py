"""-m gpu: N:M and top-k sparsity on every kernel route and on every copy of the rank rule (tests/_sparse_cases.py), bit-exact.

  * the N:M case table, one test per route of dmxq_nm_mask: mask and / or y against the stable-argsort truth for every K, K kept per
    group, the declared output dtype, -0.0 in y where a negative x was masked, and the library's class query with the real device
    pointers naming the route the table names;
  * every group set through the mask op itself (M = 16 and the run-time-loop Ms in full);
  * the M = 2, 4, 8 group sets, every K, through the other copies of the rule: the fused weight chain (typed rows kernel), its
    multi-tensor form, the strided chain and Wanda;
  * the top-k case table through the backend entry that takes n_zero: constant scores past the scan's second round and the grid cap,
    sparse ties, thresholds on the NaN key / +-inf / +-0 / a denormal / a negative value, chosen radix digits, alignments and dtypes."""
import numpy as np
import pytest
import torch

import _sparse_cases as S
from _data import bits_equal, make

pytestmark = pytest.mark.gpu
T32, T16, TB16 = S.T32, S.T16, S.TB16


def dev_view(t, off_bytes, device):
    """t on the device as a contiguous view that starts off_bytes after a 16-byte aligned allocation base"""
    k = off_bytes // t.element_size()
    assert k * t.element_size() == off_bytes
    buf = torch.empty(t.numel() + k + 16, dtype=t.dtype, device=device)
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == off_bytes % 16
    return v


# ------------------------------------------------------------------------------------------------------------------ N:M table
@pytest.mark.parametrize("route", S.ROUTES)
def test_nm_table(dmx, cuda, route):
    ops = dmx.ops
    scores = {}
    n_neg_zero = 0
    for c in S.nm_table():
        if c.route != route:
            continue
        cid = S.case_id(c)
        key = (c.M, c.sdt, c.shape, c.block_dim)
        if key not in scores:
            s = S.nm_scores(c)
            scores[key] = (s, S.NmTruth(s, c.M, c.block_dim))
        s_cpu, truth = scores[key]
        s = dev_view(s_cpu, c.off_score, cuda)
        x_cpu = S.nm_x(c) if c.want_y else None
        x = dev_view(x_cpu, c.off_x, cuda) if c.want_y else None
        # the dispatcher's own decision for these very tensors
        assert ops.nm_mask_class(s, c.ks[0], c.M, c.block_dim, x=x, mask_dtype=c.mdt, out_dtype=c.out_dtype, return_mask=c.want_mask) == route, cid
        for K in c.ks:
            if c.want_y:
                got = ops.nm_sparsify(x, s, K, c.M, c.block_dim, out_dtype=c.out_dtype, return_mask=c.want_mask)
                y, mask = got if c.want_mask else (got, None)
            else:
                y, mask = None, ops.nm_mask(s, K, c.M, c.block_dim, mask_dtype=c.mdt)
            m32 = truth.mask(K)
            if c.want_mask:
                assert mask.dtype == c.mdt and mask.shape == s.shape, cid
                assert bits_equal(mask, m32.to(c.mdt)) == 0, (cid, K)
                per_group = mask.float().movedim(c.block_dim, -1).reshape(-1, c.M).sum(1)
                assert bool((per_group == K).all()), (cid, K)
            if c.want_y:
                want = (x_cpu * m32.to(c.sdt)).to(S.ydt_of(c))      # torch's promotion of (x, mask in the score's dtype), then out_dtype
                assert y.dtype == S.ydt_of(c) and want.dtype == y.dtype, cid
                assert bits_equal(y, want) == 0, (cid, K)
                gone = (m32 == 0) & (x_cpu.float() < 0)
                if bool(gone.any()):
                    yc = y.cpu()
                    assert bool((yc[gone].float() == 0).all()) and bool(torch.signbit(yc[gone].float()).all()), (cid, K)
                    n_neg_zero += int(gone.sum())
    assert scores
    assert n_neg_zero > 0 or route == S.F32_MASK     # (the float32-mask kernel writes no y)


@pytest.mark.parametrize("M", S.GROUP_SET_MS)
def test_every_group_set_through_the_mask_op(dmx, cuda, M):
    """the whole set of every M, every K: flat and aligned (float32-mask / vector kernels, or the run-time loops), in the three dtypes
    for M <= 8, and once more along a strided dim (the per-group kernel) for M = 2, 4, 8"""
    ops = dmx.ops
    for dt in (S.DTYPES if M <= 8 else (T32,)):
        score = S.group_scores(M, dt)
        G = score.shape[0]
        flat = score[torch.arange(-(-G // 16) * 16) % G].reshape(-1).contiguous()      # (the flat route needs whole 16-element units)
        truth = S.NmTruth(flat, M)
        s = flat.to(cuda)
        want_route = (S.F32_MASK if dt == T32 and M <= 8 else S.VECTOR) if M in (2, 4, 8, 16) else S.ANY_M
        assert ops.nm_mask_class(s, 1, M) == want_route
        for K in S.ks_for(M):
            assert bits_equal(ops.nm_mask(s, K, M), truth.mask(K, dt)) == 0, (M, dt, K)
        if M in (2, 4, 8):
            strided = S.place(score[:G - G % 3], 1, (G // 3) * M, 3)[0]      # [L, 3], groups along dim 0
            ts = S.NmTruth(strided, M, 0)
            sd = strided.to(cuda)
            assert ops.nm_mask_class(sd, 1, M, 0) == S.GROUP_M
            for K in S.ks_for(M):
                assert bits_equal(ops.nm_mask(sd, K, M, 0), ts.mask(K, dt)) == 0, (M, dt, K)


# --------------------------------------------------------------------------------------- the other copies of the rank rule
HN_B, HN_WL = 64, 8      # BFP[8|8]{64}, symmetric


def _padded_groups(M, dtype, multiple):
    """the M-group set as a flat score, tiled up to a whole number of `multiple` elements"""
    n_groups = -(-len(S.group_indices(M)) * M // multiple) * multiple // M
    idx = S.group_indices(M)[np.arange(n_groups) % len(S.group_indices(M))]
    return S.alphabet(dtype)[torch.from_numpy(idx.astype(np.int64))]


@pytest.mark.parametrize("wdt,sdt", [(TB16, T32), (T16, T16)], ids=["bf16w-f32s", "f16w-f16s"])
@pytest.mark.parametrize("M", [2, 4, 8])
def test_group_sets_through_the_fused_weight_chain(dmx, cuda, oracle, M, wdt, sdt):
    """ops.weight_hypernet (the typed rows kernel: hn_sort_key and its own unrolled loops) and ops.weight_hypernet_multi on three
    tensors of unequal size, against oracle.bfp_cast(w * truth_mask): finite weights, only the scores carry the specials"""
    ops = dmx.ops
    score = _padded_groups(M, sdt, HN_B).reshape(-1, HN_B)
    rows = score.shape[0]
    w = make("normal", (rows, HN_B), seed=40 + M, dtype=wdt)
    truth = S.NmTruth(score, M)
    cuts = (0, rows // 7, rows // 7 + rows // 3, rows)
    wd, sd = w.to(cuda), score.to(cuda)
    parts_w = [wd[a:b].contiguous() for a, b in zip(cuts, cuts[1:])]
    parts_s = [sd[a:b].contiguous() for a, b in zip(cuts, cuts[1:])]
    assert len({p.shape[0] for p in parts_w}) == 3
    for K in S.ks_for(M):
        want = oracle.bfp_cast(w * truth.mask(K, sdt), HN_WL, HN_B).to(wdt)
        got = ops.weight_hypernet(wd, HN_WL, HN_B, True, sd, K, M, out_dtype=wdt)
        assert got is not None and got.dtype == wdt, "the table's shapes are fusable"
        assert bits_equal(got, want) == 0, (M, K)
        multi = ops.weight_hypernet_multi(parts_w, HN_WL, HN_B, True, parts_s, K, M, out_dtype=wdt)
        assert multi is not None and len(multi) == 3
        assert bits_equal(torch.cat(multi), want) == 0, (M, K)


@pytest.mark.parametrize("wdt,sdt", [(TB16, T32), (T16, T16)], ids=["bf16w-f32s", "f16w-f16s"])
@pytest.mark.parametrize("M", [2, 4, 8])
def test_group_sets_through_the_strided_chain(dmx, cuda, oracle, M, wdt, sdt):
    """block_dim = 1 on an [outer, L, inner = 3] weight: the "same group" loop of hs_rows8 (csrc/hypernet.hip)"""
    ops = dmx.ops
    L, inner = HN_B, 3
    groups = _padded_groups(M, sdt, L * inner)
    outer = groups.numel() // (L * inner)
    score = S.place(groups, outer, L, inner)
    w = make("normal", (outer, L, inner), seed=50 + M, dtype=wdt)
    truth = S.NmTruth(score, M, 1)
    wd, sd = w.to(cuda), score.to(cuda)
    for K in S.ks_for(M):
        want = oracle.bfp_cast(w * truth.mask(K, sdt), HN_WL, HN_B, block_dim=1).to(wdt).contiguous()
        got = ops.weight_hypernet(wd, HN_WL, HN_B, True, sd, K, M, out_dtype=wdt, block_dim=1)
        assert got is not None and got.dtype == wdt, "the table's shapes are fusable"
        assert bits_equal(got, want) == 0, (M, K)


# the finite weights whose magnitudes are the non-negative half of the alphabet (0, min denormal, 1, 1 + eps, max finite), by symbol:
# -inf / +inf stand for -(1 + eps) / 1 + eps, the NaNs for the two zeros, so that equal magnitudes of both signs meet in a group
WANDA_SYMBOL = (8, 1, 2, 3, 4, 5, 6, 7, 8, 9, 8, 5, 4)
WANDA_NEGATIVE = (True, True, True, True, True, False, False, False, False, False, False, False, True)


@pytest.mark.parametrize("wdt", [TB16, T32, T16], ids=["bf16", "f32", "f16"])
@pytest.mark.parametrize("M", [2, 4, 8])
def test_group_sets_through_wanda(dmx, cuda, M, wdt):
    """ops.wanda_nm_sparsify with a unit activation norm: the score |w| is formed in registers (csrc/wanda.hip over nm_rank.hpp;
    M = 2 is the front end's chain over the mask op)"""
    ops = dmx.ops
    a = S.alphabet(wdt)
    mag = a[torch.tensor(WANDA_SYMBOL)].abs()
    sym = torch.where(torch.tensor(WANDA_NEGATIVE), -mag, mag)
    assert bool(torch.isfinite(sym.float()).all()) and sorted(set(sym.float().abs().tolist())) == sorted(set(a[5:10].float().tolist()))
    n_groups = -(-len(S.group_indices(M)) * M // 64) * 64 // M
    idx = S.group_indices(M)[np.arange(n_groups) % len(S.group_indices(M))]
    w = sym[torch.from_numpy(idx.astype(np.int64))].reshape(-1, 64).contiguous()
    truth = S.NmTruth(w.float().abs(), M)
    wd = w.to(cuda)
    norm = torch.ones(64, device=cuda)
    ydt = torch.promote_types(wdt, T32)
    for K in S.ks_for(M):
        y, mask = ops.wanda_nm_sparsify(wd, norm, K, M, return_mask=True, fused=True if M != 2 else None)
        m32 = truth.mask(K)
        assert mask.dtype == T32 and bits_equal(mask, m32) == 0, (M, K)
        assert y.dtype == ydt and bits_equal(y, w.to(ydt) * m32) == 0, (M, K)


# ------------------------------------------------------------------------------------------------------------------ top-k table
def _topk(dmx, c, s, x, n_zero):
    """the backend entry the front end's _topk calls: the zero count itself, no density rounded on the way"""
    mask, y = dmx.ops._front._ops.topk_mask(s, x, n_zero, c.want_mask, c.want_y, c.mdt, None)
    return (mask if c.want_mask else None), (y if c.want_y else None)


def _check_topk(dmx, cuda, oracle, c):
    s_cpu = S.topk_score(c)
    x_cpu = S.topk_x(c) if c.want_y else None
    s = dev_view(s_cpu, c.off_score, cuda)
    x = dev_view(x_cpu, c.off_x, cuda) if c.want_y else None
    for nz in c.n_zeros:
        keep = S.topk_closed_form(c, nz)
        keep = keep if keep is not None else S.topk_truth(oracle, s_cpu, nz).float() != 0
        assert int(keep.sum()) == c.n - nz
        mask, y = _topk(dmx, c, s, x, nz)
        if c.want_mask:
            assert mask.dtype == c.mdt and bits_equal(mask, keep.to(c.mdt)) == 0, (c.name, nz)
            assert int(mask.float().sum()) == c.n - nz, (c.name, nz)
        if c.want_y:
            ydt = torch.promote_types(c.xdt, c.sdt)
            assert y.dtype == ydt and bits_equal(y, x_cpu * keep.to(c.sdt)) == 0, (c.name, nz)
            assert int((y != 0).sum()) <= c.n - nz, (c.name, nz)


_SMALL_TOPK = [c for c in S.topk_table() if "large" not in c.marks]
_LARGE_TOPK = [c for c in S.topk_table() if "large" in c.marks]


@pytest.mark.parametrize("group", ["sparse", "special", "radix", "lattice"])
def test_topk_table(dmx, cuda, oracle, group):
    cases = [c for c in _SMALL_TOPK if c.kind.split(":")[0] == group]
    assert cases
    for c in cases:
        _check_topk(dmx, cuda, oracle, c)
    assert sum(len([c for c in _SMALL_TOPK if c.kind.split(":")[0] == g]) for g in ("sparse", "special", "radix", "lattice")) == len(_SMALL_TOPK)


@pytest.mark.parametrize("c", _LARGE_TOPK, ids=[c.name for c in _LARGE_TOPK])
def test_topk_constant_score(dmx, cuda, c):
    """every key ties: the index-ordered path alone decides, across the scan's second round of 256 chunks and (the second row) past the
    grid cap of the chunk loops; truth arange(n) >= n_zero, compared on the device"""
    s = S.topk_score(c).to(cuda)
    x_cpu = S.topk_x(c) if c.want_y else None
    x = x_cpu.to(cuda) if c.want_y else None
    ar = torch.arange(c.n, device=cuda)
    assert len(c.n_zeros) == 15
    for nz in c.n_zeros:
        keep = ar >= nz
        mask, y = _topk(dmx, c, s, x, nz)
        assert mask.dtype == c.mdt and bool(torch.equal(mask, keep.to(c.mdt))), (c.name, nz)
        assert int(mask.sum()) == c.n - nz, (c.name, nz)
        if c.want_y:
            want = x * keep.to(c.sdt)
            it = torch.int32 if want.element_size() == 4 else torch.int16
            assert y.dtype == want.dtype and bool(torch.equal(y.view(it), want.view(it))), (c.name, nz)
