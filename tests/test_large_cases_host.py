"""Host-only proof that the table of tests/_large_cases.py does what it is for: every case is beyond the 32-bit boundary, its chunks are
not, the chunk boundaries fall on whole rows, groups and blocks, no period of its index decode divides 2^31 or 2^32, and every 64-bit
branch named by the table is run by some case."""
import pytest

import _large_cases as LC

FULL = LC.ALL
TWINS = [LC.under(c) for c in LC.ALL if c.twin]


@pytest.mark.parametrize("c", FULL, ids=lambda c: c.name)
def test_case_is_beyond_the_boundary_and_its_chunks_are_not(c):
    n = LC.numel(c.shape)
    assert n > LC.MIN_N, (c.name, n)
    if c.op == "topk_mask":
        assert LC.TWO31 < n < LC.TWO32
    ch = LC.chunks(c)
    assert ch[0][0] == 0 and ch[-1][1] == c.shape[0] and all(a[1] == b[0] for a, b in zip(ch, ch[1:]))
    assert all(0 < (b - a) * LC.row_len(c) < LC.TWO31 for a, b in ch), (c.name, ch)
    # the 2^31 boundary lies INSIDE a chunk (not at its first element): the chunk's own indices restart from zero there
    assert any(a * LC.row_len(c) < LC.TWO31 < b * LC.row_len(c) for a, b in ch)


@pytest.mark.parametrize("c", TWINS, ids=lambda c: c.name)
def test_twin_is_the_largest_whole_row_tensor_under_the_boundary(c):
    n, rl = LC.numel(c.shape), LC.row_len(c)
    assert n < LC.TWO31 <= n + rl * c.unit, (c.name, n)
    assert all((b - a) * rl < LC.TWO31 // 2 + rl * c.unit for a, b in LC.chunks(c, LC.TWO31 // 2 + rl * c.unit))


@pytest.mark.parametrize("c", FULL + TWINS, ids=lambda c: c.name)
def test_chunks_and_windows_are_whole_rows_groups_and_blocks_and_aligned(c):
    rl, p = LC.row_len(c), c.p
    assert c.shape[0] % c.unit == 0 or c.unit == 8, c.name          # (unit 8: alignment only, the last chunk may end anywhere)
    if c.op in ("rope", "topk_mask"):       # (no row windows: a refusal, and a flat tensor with an analytic reference)
        return
    cuts = [a for a, _ in LC.chunks(c)] + ([w[0] for w in LC.windows(c)] if "col_window" not in p else [])
    for a in cuts:
        assert a % c.unit == 0 or a == c.shape[0], (c.name, a)
        if p.get("gs") and (p.get("ch_axis") == 0 or c.op.endswith("_multi")):
            assert a % p["gs"] == 0 or a == c.shape[0], (c.name, a)              # whole scale groups along the rows
        for item in (LC.ITEM[c.dtype], LC.ITEM[c.out]) + ((c.extra,) if c.extra else ()):
            assert (a * rl * item) % 16 == 0, (c.name, a, item)                  # every chunk is a 16-byte aligned view
    if len(c.shape) == 2:
        L = c.shape[1]
        for key in ("B", "M", "H"):
            if p.get(key) and c.op != "bfp_qdq":
                assert L % p[key] == 0, (c.name, key)                            # whole blocks in every row: a row cut is a block cut
        if c.op == "bfp_pack":
            assert ((L // p["B"]) * 1) % 16 == 0                                 # the exponent rows are aligned views too
        if p.get("granularity") == "per_group":
            assert L % p["gs"] == 0
    if len(c.shape) == 3 and p.get("gs"):
        assert c.shape[1] % p["gs"] == 0
    if "col_window" in p:
        for r, c0, w in LC.windows(c):
            assert 0 <= r < c.shape[0] and c0 % p["B"] == 0 and w % p["B"] == 0 and 0 <= c0 and c0 + w <= rl
    else:
        for a, b in LC.windows(c):
            assert 0 <= a < b <= c.shape[0] and b - a <= 64 + c.unit
        if c in FULL:
            a, b = LC.windows(c)[0]
            assert a * rl < LC.TWO31 < b * rl, c.name                            # the first window straddles element 2^31
    if c.specials:
        rows = LC.special_rows(c)
        wins = LC.windows(c)
        assert all(0 <= r < c.shape[0] and not any(a <= r < b for a, b in wins) for r in rows), c.name
        if c in FULL:
            assert all(r * rl > LC.TWO31 for r in rows), c.name                  # each special lies beyond the boundary
        assert rl >= 512


@pytest.mark.parametrize("c", FULL, ids=lambda c: c.name)
def test_no_period_of_the_index_decode_divides_two_to_the_31_or_32(c):
    ps = LC.periods(c)
    assert ps or len(c.shape) == 1, c.name
    for P in ps:
        assert LC.TWO31 % P != 0 and LC.TWO32 % P != 0, (c.name, P)
    if len(c.shape) >= 2:
        assert c.shape[0] % 256 != 0, c.name


def test_every_listed_branch_is_the_target_of_a_case():
    hit = {t for c in LC.ALL for t in c.targets}
    assert hit <= set(LC.BRANCHES), hit - set(LC.BRANCHES)
    assert set(LC.BRANCHES) <= hit, set(LC.BRANCHES) - hit
    assert len({c.name for c in LC.ALL}) == len(LC.ALL)


def test_memory_need_is_computed_from_the_case_and_stays_under_24_gib():
    for c in LC.ALL:
        assert LC.peak_bytes(c) <= 24 * LC.GIB, (c.name, LC.peak_bytes(c) / LC.GIB)
