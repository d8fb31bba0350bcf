"""No GPU: the sparsity case tables (tests/_sparse_cases.py) against the library's own answers.
  * the Python restatement of dmxq_nm_mask's kernel choice against dmxq_nm_mask_class (the function the entry decides with; a host
    function that launches nothing) over M 1..64, every dtype and output combination, inner 1 and 3, n % 16 in {0, 8, 4} and each of the
    four bases on and off the 16-byte grid, with made-up addresses;
  * the N:M table reaches every route, every typed triple and, per route, a partial and an exact last tile -- and every row's declared
    route is the library's answer for the row's real geometry;
  * the top-k rows' chunk counts are the library's (dmxq_topk_workspace_bytes), past the scan round and the grid cap where marked;
  * the two truths agree: the stable argsort with oracle.nm_mask on every group set, the closed forms with oracle.topk_mask."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _sparse_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _asker(dmx):
    """route(dts, dtx, dtm, dty, outer, L, inner, K, M, a_score, a_x, a_mask, a_y) through the library: a route name or S.BAD_ARG"""
    L, lib = dmx._lib.lib(), dmx._lib
    route = ctypes.c_int(0)
    ref = ctypes.byref(route)
    names = {v: k for k, v in S.ROUTE_CODE.items()}

    def ask(dts, dtx, dtm, dty, outer, Ln, inner, K, M, a_score, a_x, a_mask, a_y):
        st = L.dmxq_nm_mask_class(dts, dtx, dtm, dty, outer, Ln, inner, K, M, a_score or None, a_x or None, a_mask or None, a_y or None, ref)
        assert st in (lib.OK, lib.ERR_BAD_ARG), st
        return names[route.value] if st == lib.OK else S.BAD_ARG

    return ask


def _length(M, inner, rem):
    """the smallest L = M * g with (L * inner) % 16 == rem, or None"""
    for g in range(1, 17):
        if (M * g * inner) % 16 == rem:
            return M * g
    return None


def test_route_restatement_equals_the_library(dmx):
    ask = _asker(dmx)
    bases = (0x100000, 0x500000, 0x900000, 0xD00000)
    outputs = ([(True, False, 0, m, 0) for m in range(3)] + [(False, True, x, 0, y) for x in range(3) for y in range(3)]
               + [(True, True, x, m, y) for x in range(3) for m in range(3) for y in range(3)])
    seen, n = set(), 0
    for M in range(1, 65):
        for inner in (1, 3):
            for rem in (0, 8, 4):
                Ln = _length(M, inner, rem)
                if Ln is None:
                    continue
                for dts in range(3):
                    for want_mask, want_y, dtx, dtm, dty in outputs:
                        for mis in range(16):
                            a = [b + (4 if mis >> k & 1 else 0) for k, b in enumerate(bases)]
                            if not want_y:
                                a[1] = a[3] = 0
                            if not want_mask:
                                a[2] = 0
                            args = (dts, dtx, dtm, dty, 1, Ln, inner, (M + 1) // 2, M, *a)
                            got, want = ask(*args), S.nm_route(*args)
                            assert got == want, (args, got, want)
                            seen.add(got)
                            n += 1
    assert seen == set(S.ROUTES) and n > 400000


def test_route_argument_errors_and_empty_tensors(dmx):
    """the class function refuses what dmxq_nm_mask refuses, and the entry returns the same status without a GPU"""
    ask, L, lib = _asker(dmx), dmx._lib.lib(), dmx._lib
    p = 0x100000
    ok = [S.F32, S.F32, S.F32, S.F32, 2, 16, 1, 2, 4, p, p, p, p]
    assert ask(*ok) == S.VECTOR
    for pos, bad in ((0, 3), (0, -1), (1, 7), (2, 5), (3, 9), (4, -1), (5, -4), (6, -1), (7, 0), (7, 5), (8, 0), (8, 65), (8, 3), (9, 0), (10, 0)):
        args = list(ok)
        args[pos] = bad
        assert ask(*args) == S.nm_route(*args) == S.BAD_ARG, (pos, bad)
        dts, dtx, dtm, dty, outer, Ln, inner, K, M, a_s, a_x, a_m, a_y = (v or None if i >= 9 else v for i, v in enumerate(args))
        assert L.dmxq_nm_mask(a_s, dts, a_x, dtx, a_m, dtm, a_y, dty, outer, Ln, inner, K, M, None) == lib.ERR_BAD_ARG, (pos, bad)
    none = list(ok)
    none[10] = none[12] = 0     # mask only: x is not needed, and its dtype is not looked at
    none[1] = none[3] = 7
    assert ask(*none) == S.nm_route(*none) == S.F32_MASK
    none[11] = 0                # no output at all
    assert ask(*none) == S.nm_route(*none) == S.BAD_ARG
    for pos in (4, 5, 6):       # an empty tensor: nothing to launch, whatever the addresses
        args = list(ok)
        args[pos] = 0
        args[9] = 0
        assert ask(*args) == S.nm_route(*args) == S.NONE
    assert L.dmxq_nm_mask_class(*ok[:9], *ok[9:], None) == lib.ERR_BAD_ARG
    assert (lib.NM_NONE, lib.NM_TYPED, lib.NM_F32_MASK, lib.NM_VECTOR, lib.NM_GROUP_M, lib.NM_ANY_M) == tuple(S.ROUTE_CODE[r] for r in (S.NONE,) + S.ROUTES)
    assert lib.NM_ROUTE_NAMES == {v: k for k, v in S.ROUTE_CODE.items()}
    header = open(os.path.join(ROOT, "include", "dmxq.h")).read()
    assert int(re.search(r"#define DMXQ_GRID_CAP (\d+)", header).group(1)) == S.GRID_CAP == lib.GRID_CAP


def test_ops_nm_mask_class_on_cpu_tensors(dmx):
    """the front end's query takes tensors on any device: dtypes, sizes and base alignment only"""
    ops = dmx.ops
    s32, sb = torch.zeros(4, 64), torch.zeros(4, 64, dtype=torch.bfloat16)
    assert "nm_mask_class" in ops.__all__
    assert ops.nm_mask_class(s32, 2, 4) == S.F32_MASK and ops.nm_mask_class(sb, 2, 4) == S.VECTOR
    assert ops.nm_mask_class(s32, 2, 4, x=sb) == S.TYPED and ops.nm_mask_class(s32, 2, 4, x=sb, out_dtype=torch.bfloat16) == S.TYPED
    assert ops.nm_mask_class(sb, 2, 4, x=s32) == S.VECTOR and ops.nm_mask_class(s32, 2, 4, x=sb, return_mask=True) == S.VECTOR
    assert ops.nm_mask_class(s32, 2, 4, block_dim=0) == S.GROUP_M and ops.nm_mask_class(torch.zeros(4, 63), 2, 3) == S.ANY_M
    assert ops.nm_mask_class(torch.zeros(260)[1:257], 2, 4) == S.GROUP_M      # a view 4 bytes into its allocation
    assert ops.nm_mask_class(torch.zeros(0, 64), 2, 4) == S.NONE
    with pytest.raises(dmx.DmxqError):
        ops.nm_mask_class(s32, 5, 4)


def test_nm_table_reaches_every_route_triple_and_edge(dmx):
    ask = _asker(dmx)
    table = S.nm_table()
    assert len({S.case_id(c) for c in table}) == len(table)
    assert {c.route for c in table} == set(S.ROUTES)
    assert {(c.xdt, c.sdt, S.ydt_of(c), c.M) for c in table if c.route == S.TYPED} == {t + (M,) for t in S.TYPED_TRIPLES for M in (2, 4, 8)}
    for route in S.ROUTES:
        edges = {S.edge(c) for c in table if c.route == route}
        assert {"partial", "exact"} <= edges, (route, edges)
        assert ("cap" in edges) == (route in (S.VECTOR, S.GROUP_M)), (route, edges)
    for c in table:
        outer, L, inner = S.geometry(c)
        args = (S.CODE[c.sdt], S.CODE[c.xdt] if c.want_y else 0, S.CODE[c.mdt] if c.want_mask else 0, S.CODE[S.ydt_of(c)] if c.want_y else 0, outer,
                L, inner, c.ks[0], c.M, *S.nm_addresses(c))
        assert ask(*args) == S.nm_route_of_case(c) == c.route, S.case_id(c)
        assert c.ks == S.ks_for(c.M)
    # what the table promises of each route, by name
    by = lambda route: [c for c in table if c.route == route]
    assert {c.shape[0] for c in by(S.TYPED)} == {16, 8192 - 16, 8192, 8192 + 16, 3 * 8192 + 48}
    assert {(c.M, c.shape[0]) for c in by(S.F32_MASK)} == {(M, n) for M in (2, 4, 8) for n in (16, 4080, 4096, 4112, 8208)}
    vec = by(S.VECTOR)
    assert {(c.sdt, c.mdt) for c in vec if c.want_mask and not c.want_y and c.sdt != c.mdt} == {(s, m) for s in S.DTYPES for m in S.DTYPES if s != m}
    assert {c.M for c in vec if c.want_mask and c.want_y and c.xdt != c.sdt} == {2, 4, 8, 16}
    assert any(c.xdt == S.T32 and c.sdt == S.TB16 and not c.want_mask for c in vec)
    assert [(c.sdt, c.mdt, c.M, c.shape) for c in vec if S.edge(c) == "cap"] == [(S.TB16, S.TB16, 4, (2048 * 4096 + 4096 + 16,))]
    grp = by(S.GROUP_M)
    for M in (2, 4, 8, 16):
        mine = [c for c in grp if c.M == M]
        assert {S.geometry(c)[2] for c in mine} >= {1, 3, 7} and {c.block_dim for c in mine} >= {0, -2}
        assert {c.sdt for c in mine if c.off_score == 4} == set(S.DTYPES) and {c.sdt for c in mine if c.off_x == 4} == set(S.DTYPES)
        assert all(int(np.prod(c.shape)) % 16 == 0 and S.geometry(c)[2] == 1 for c in mine if c.off_score or c.off_x)   # misalignment alone decides
        assert M == 16 or any(int(np.prod(c.shape)) % 16 and S.geometry(c)[2] == 1 for c in mine)
    assert [(c.M, int(np.prod(c.shape)) // c.M) for c in grp if S.edge(c) == "cap"] == [(2, 524288 + 3)]
    assert {(c.M, S.geometry(c)[2], c.sdt) for c in by(S.ANY_M)} >= {(M, i, s) for M in (1, 3, 12, 32, 64) for i in (1, 5) for s in S.DTYPES}


def test_group_sets_are_the_ones_described():
    S13 = len(S.SYMBOLS)
    assert S13 == 13
    for dt in S.DTYPES:
        a = S.alphabet(dt)
        f = a.double()
        fi = torch.finfo(dt)
        mind = fi.tiny * fi.eps     # the smallest denormal
        assert f[:11].tolist() == [-float("inf"), -fi.max, -1.0, -mind, 0.0, 0.0, mind, 1.0, 1.0 + fi.eps, fi.max, float("inf")]
        assert bool(torch.isnan(f[11:]).all()) and (a.view(torch.int32 if dt == torch.float32 else torch.int16) < 0).tolist() == [True] * 5 + [False] * 7 + [True]
    assert len(S.group_indices(2)) == 169 and len(S.group_indices(4)) == 28561
    assert len({bytes(g) for g in S.group_indices(4)}) == 28561
    g8 = S.group_indices(8)
    assert len(g8) == 78 * 256 + 20000
    pairs = {tuple(sorted(set(g))) for g in g8[:78 * 256].tolist()}
    assert {p for p in pairs if len(p) == 2} == {(a, b) for a in range(13) for b in range(a + 1, 13)} and {p for p in pairs if len(p) == 1} == {(a,) for a in range(13)}
    g16 = S.group_indices(16)
    assert len(g16) == 3 * 65536 and [tuple(sorted(set(g16[k * 65536:(k + 1) * 65536].ravel().tolist()))) for k in range(3)] == [(4, 5), (7, 11), (3, 5)]
    for M in (1, 3, 12, 32, 64):
        assert S.group_indices(M).shape == (4096, M)
    assert [S.ks_for(M) for M in (1, 2, 3, 8, 12, 16, 64)] == [(1,), (1, 2), (1, 2, 3), tuple(range(1, 9)), (1, 6, 12), (1, 5, 8, 15, 16), (1, 32, 64)]
    # a short row is a sample of the whole set: a 256-group row of M = 8 already holds every symbol at every position
    idx = S.row_group_indices(8, 256)
    assert all(len(set(idx[:, p].tolist())) == 13 for p in range(8))


def test_stable_argsort_truth_equals_the_oracle_on_every_group_set(oracle):
    for M in S.GROUP_SET_MS:
        for dt in S.DTYPES:
            score = S.group_scores(M, dt)
            truth = S.NmTruth(score, M)
            for K in S.ks_for(M):
                want = oracle.nm_mask(score, K, M)
                got = truth.mask(K, dt)
                assert want.dtype == dt and torch.equal(got, want), (M, dt, K)
                assert bool((got.float().sum(1) == K).all())


def test_truth_follows_the_layout(oracle):
    """groups along another dim than the last: the placed group set's truth is the placed truth"""
    groups = S.group_scores(4, torch.float32)[:2 * 5 * 3]
    score = S.place(groups, 2, 20, 3)
    for K in (1, 2, 3):
        flat = S.nm_truth(groups, K, 4)
        assert torch.equal(S.nm_truth(score, K, 4, block_dim=1), S.place(flat, 2, 20, 3))
        assert torch.equal(S.nm_truth(score, K, 4, block_dim=1), oracle.nm_mask(score, K, 4, 1))


def test_topk_geometry_is_the_librarys(dmx):
    L = dmx._lib.lib()
    table = S.topk_table()
    assert len({c.name for c in table}) == len(table)
    for c in table:
        chunks = (L.dmxq_topk_workspace_bytes(c.n) - 64 - 8192) // 8
        assert chunks == S.topk_chunks(c.n), c.name
        assert ("scan2" in c.marks) == (chunks > S.TOPK_SCAN_ROUND) and ("cap" in c.marks) == (chunks > S.GRID_CAP), c.name
        assert all(0 <= z <= c.n for z in c.n_zeros) and c.n_zeros
        assert ("closed" in c.marks) == (S.topk_closed_form(c, c.n_zeros[0]) is not None)
    assert [c.n for c in table if "scan2" in c.marks] == [2048 * 256 + 2048 + 5, 2048 * 2048 + 2048 + 5]
    assert [c.n for c in table if "cap" in c.marks] == [2048 * 2048 + 2048 + 5]
    assert any(c.off_score and c.sdt == dt for c in table for dt in S.DTYPES) and any(c.off_x for c in table)
    assert any(c.want_mask and c.mdt != c.sdt for c in table) and any(c.want_y and c.xdt != c.sdt for c in table)
    assert {(c.want_mask, c.want_y) for c in table} == {(True, False), (False, True), (True, True)}


def _sorted_keys(score):
    """float32 scores ascending, NaN last (numpy's order)"""
    return np.sort(score.float().numpy(), kind="stable")


def test_topk_rows_put_the_threshold_where_they_say(dmx):
    """sparse ties and the special rows: the n_zero-th smallest score is the named key, and only some of its ties are zeroed"""
    for c in S.topk_table():
        if c.T is None:
            continue
        s = _sorted_keys(S.topk_score(c))
        for nz in c.n_zeros:
            t = s[nz - 1]
            if c.T == "nan":
                assert np.isnan(t), c.name
                below, ties = int((~np.isnan(s)).sum()), int(np.isnan(s).sum())
            else:
                assert t == np.float32(c.T), (c.name, t)
                below, ties = int((s < t).sum()), int((s == t).sum())
            assert 1 <= nz - below < ties, (c.name, nz, below, ties)
        if c.name.startswith("special"):
            assert c.n % 8 != 0
            raw = S.topk_score(c)
            if c.T == "nan" or c.T == 0.0:      # both signs of the special
                sel = torch.isnan(raw.float()) if c.T == "nan" else raw.float() == 0
                assert set((raw.view(torch.int32 if c.sdt == torch.float32 else torch.int16) < 0)[sel].tolist()) == {True, False}, c.name
            if c.name.startswith("special-allneg"):
                assert bool((raw.float() < 0).all())
            if c.name.startswith("special-denormal"):
                assert 0 < c.T < float(torch.finfo(c.sdt).tiny)
    sparse = next(c for c in S.topk_table() if c.kind == "sparse")
    assert [z - S._third(sparse.n, 1) for z in sparse.n_zeros] == [1, 170, 171, 683, S._third(sparse.n, 0) - 1]


def test_radix_rows_decide_in_the_named_digits():
    want = {(5000, 0): (1, 2), (5000, 10): (0, 1), (2048, 10): (1,), (500, 21): (0,)}
    seen = set()
    for c in S.topk_table():
        if c.kind.startswith("radix:"):
            _, count, shift, neg = c.kind.split(":")
            assert S.radix_levels(c) == want[int(count), int(shift)], c.name
            s = S.topk_score(c)
            assert bool(torch.isfinite(s).all()) and bool(((s < 0) == bool(int(neg))).all()) and len(torch.unique(s)) == c.n
            seen.add((int(count), int(shift), int(neg)))
    assert len(seen) == 8


def test_closed_form_topk_truths_equal_the_oracle(oracle):
    for c in S.topk_table():
        if "closed" not in c.marks:
            continue
        score = S.topk_score(c)
        for nz in (c.n_zeros if "cap" not in c.marks else c.n_zeros[8:9]):    # n > 4 M: one density suffices
            keep = S.topk_closed_form(c, nz)
            assert torch.equal(S.topk_truth(oracle, score, nz), keep.to(score.dtype)), (c.name, nz)
            assert int(keep.sum()) == c.n - nz
