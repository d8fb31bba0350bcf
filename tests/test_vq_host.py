"""Host tests (no GPU) of the vector codebook casts (ops.vq_*, CastTo.set_vq; DESIGN.md §8 "Vector codebook casts"): the vocabulary and
its ValueErrors, the exclusivity rules, the buffers, the configure keys, every procedure's refusal, the C entries' answers with
libdmxq.so loaded on the CPU, and the properties of the CPU checker itself (tests/_vq_ref.py), which the GPU tests compare the kernels
against."""
import ctypes

import pytest
import torch

import _vq_ref as R
from _data import make

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
INT4 = "XP[4,0](CSN)"
PAIRS = [[-1.0, -1.0], [-1.0, 1.0], [1.0, -1.0], [1.0, 1.0], [0.0, 0.0]]
GRID = {"codebook": {"grid": "uniform4", "dim": 4}, "per_group": 64}


# ------------------------------------------------------------------------------------------------ tables and the check
def test_grid_and_check_vocabulary(dmx):
    ops = dmx.ops
    g = ops.vq_grid("uniform4", 4)
    assert g.dtype == F32 and g.shape == (256, 4) and not g.is_cuda
    assert torch.equal(g, R.grid(torch.linspace(-1, 1, 4).tolist(), 4))          # lexicographic: the first component varies slowest
    assert g[0].tolist() == [-1.0] * 4 and g[1].tolist() == [-1.0, -1.0, -1.0, float(torch.linspace(-1, 1, 4)[1])] and g[255].tolist() == [1.0] * 4
    assert ops.vq_grid("nf4", 2).shape == (256, 2) and ops.vq_grid([0.0, 1.0], 8).shape == (256, 8)
    assert torch.equal(ops.vq_grid((-0.5, 0.25, 1.0), 2), R.grid((-0.5, 0.25, 1.0), 2))
    for bad in (("nf4", 4), ("uniform4", 8), ("uniform4", 3), ("uniform4", True), ("nope", 2), ([1.0, 0.0], 2), ([0.0, float("nan")], 2)):
        with pytest.raises(ValueError):
            ops.vq_grid(*bad)
    table, K, d, gran, gs, norm = ops.vq_check(PAIRS, None, "per_group", 64, None)
    assert (K, d, gran, gs, norm) == (5, 2, "per_group", 64, None) and table == tuple(tuple(r) for r in PAIRS)
    assert ops.vq_check(torch.tensor(PAIRS), 2, "per_token", 64, 3)[1:] == (5, 2, "per_token", None, 3.0)
    assert ops.vq_check({"grid": "nf4", "dim": 2}, granularity="per_tensor")[1:3] == (256, 2)
    unsorted_dup = [[1.0, 0.0], [-1.0, 0.5], [1.0, 0.0], [0.25, 0.25]]             # no order is required, duplicate rows are allowed
    assert ops.vq_check(unsorted_dup)[1:3] == (4, 2)
    assert ops.VQ_DIMS == (2, 4, 8) and ops.VQ_CHAIN_BY_DEFAULT <= {"group", "short_row", "wave_row", "block_row"}


@pytest.mark.parametrize("bad", [
    dict(codebook="nf4"), dict(codebook=3), dict(codebook=[[0.0, 1.0]]), dict(codebook=[[0.0, 1.0]] * 257), dict(codebook=[[0.0], [1.0]]),
    dict(codebook=[[0.0] * 3] * 4), dict(codebook=[[0.0] * 16] * 4), dict(codebook=[[0.0, 1.0], [1.0]]), dict(codebook=[[0.0, float("nan")], [1.0, 0.0]]),
    dict(codebook=[[0.0, float("inf")], [1.0, 0.0]]), dict(codebook=[[0.0, "a"], [1.0, 0.0]]), dict(codebook=torch.zeros(4)),
    dict(codebook=torch.zeros(4, 2, dtype=torch.int32)), dict(codebook=torch.zeros(4, 2, 2)), dict(codebook={"grid": "nf4"}),
    dict(codebook={"grid": "nf4", "dim": 4}), dict(codebook=PAIRS, dim=4), dict(codebook=PAIRS, granularity="per_tile"),
    dict(codebook=PAIRS, granularity="per_group", group_size=0), dict(codebook=PAIRS, granularity="per_group", group_size=None),
    dict(codebook=PAIRS, granularity="per_group", group_size=7), dict(codebook=[[0.0] * 8] * 2, granularity="per_group", group_size=12),
    dict(codebook=PAIRS, norm=0.0), dict(codebook=PAIRS, norm=-1.0), dict(codebook=PAIRS, norm=float("inf")),
    dict(codebook=PAIRS, norm=float("nan")), dict(codebook=PAIRS, norm="1"),
])
def test_check_refuses(dmx, bad):
    with pytest.raises(ValueError):
        dmx.ops.vq_check(**bad)


def test_codebook_check_still_refuses_a_table(dmx):
    with pytest.raises(ValueError):
        dmx.ops.codebook_check(torch.zeros(2, 2))
    with pytest.raises(ValueError):
        dmx.ops.codebook_check(PAIRS)


def test_front_end_errors_come_before_any_gpu_use(dmx):
    ops, x = dmx.ops, torch.zeros(4, 96, dtype=BF16)   # (a CPU tensor: a ValueError must come before the DmxqError of a non-GPU tensor)
    with pytest.raises(ValueError, match="multiple of the group size"):
        ops.vq_qdq(x, PAIRS, "per_group", 64)
    with pytest.raises(ValueError, match="multiple of the table's d"):
        ops.vq_qdq(torch.zeros(4, 100, dtype=BF16), [[0.0] * 8] * 2, "per_token")
    with pytest.raises(ValueError, match="multiple of the table's d"):
        ops.vq_qdq(torch.zeros(3, 5, dtype=BF16), [[0.0] * 4] * 2, "per_tensor")
    with pytest.raises(ValueError):
        ops.vq_qdq(x, "nf4")
    with pytest.raises(ValueError):
        ops.vq_qdq(x, PAIRS, "per_token", per_group=32)
    with pytest.raises(ValueError):
        ops.vq_accumulate(x, PAIRS, "per_group", 64)
    with pytest.raises(ValueError):
        ops.vq_accumulate(x, PAIRS, "per_group", 32, accumulate=True)              # accumulate=True needs acc
    with pytest.raises(ValueError):
        ops.vq_accumulate(x, PAIRS, "per_group", 32, acc=torch.zeros(5, 3, dtype=torch.float64))
    for bad in (dict(), dict(K=16), dict(dim=2), dict(K=1, dim=2), dict(K=257, dim=2), dict(K=16, dim=3), dict(K=16, dim=2, iters=-1),
                dict(K=16, dim=2, iters=1.5), dict(K=16, dim=4, per_group=6), dict(K=16, dim=2, norm=-1.0), dict(codebook=PAIRS, dim=4),
                dict(codebook=PAIRS, K=4), dict(codebook=[[0.0, float("nan")], [1.0, 1.0]]), dict(K=16, dim=2, per_group=64)):
        with pytest.raises(ValueError):
            ops.vq_fit(x, **bad)
    with pytest.raises(ValueError):
        ops.vq_fit([], K=4, dim=2)
    with pytest.raises(dmx.DmxqError):
        ops.vq_qdq(x, PAIRS, "per_group", 32)
    with pytest.raises(dmx.DmxqError):
        ops.vq_qdq(x, {"grid": "uniform4", "dim": 4}, per_group=32)
    with pytest.raises(dmx.DmxqError):
        ops.vq_accumulate(x, PAIRS, "per_token")
    with pytest.raises(dmx.DmxqError):
        ops.vq_fit(x, K=4, dim=2, per_group=32)


def test_class_over_a_grid_of_calls(dmx):
    """vq_class tells what the kernel takes: codebook_class's geometry wherever the table fits a 16-byte vector, None elsewhere"""
    ops = dmx.ops
    for dtype in (BF16, F16, F32):
        for d in (2, 4, 8):
            for K in (2, 16, 200, 256):
                for S in (8, 16, 24, 32, 48, 64, 128, 256, 512, 768, 4096, 8192, 8200, 16384, 16392):
                    takes = not (dtype == F32 and d == 8)
                    for rows in (False, True):
                        want = ops.codebook_class(S, dtype, rows) if takes else None
                        assert ops.vq_class(S, dtype, d, K, rows) == want, (dtype, d, K, S, rows)
    assert ops.vq_class(64, BF16, 4, 256) == "group" and ops.vq_class(24, BF16, 2, 16) is None
    assert ops.vq_class(8200, BF16, 8, 2, True) == "block_row" and ops.vq_class(768, F16, 2, 16, True) == "wave_row"
    assert ops.vq_class(48, BF16, 2, 16, True) == "short_row"
    for bad in ((64, BF16, 3, 16), (64, BF16, 16, 16), (64, BF16, 2, 1), (64, BF16, 2, 257)):
        assert ops.vq_class(*bad) is None


# ------------------------------------------------------------------------------------------------ CastTo.set_vq
def test_set_vq_vocabulary_buffers_and_repr(dmx):
    c = dmx.CastTo(format=INT4)
    four = sorted(c.state_dict())
    assert len(four) == 4 and c.vq_setting is None and "vq" not in repr(c)
    c.set_vq(GRID)
    assert sorted(c.state_dict()) == sorted(four + ["vq_codebook", "vq_norm"])
    assert c.vq_codebook.dtype == F32 and c.vq_codebook.shape == (256, 4) and c.vq_norm.shape == (1,) and float(c.vq_norm) == 0.0
    assert torch.equal(c.vq_codebook, dmx.ops.vq_grid("uniform4", 4))
    assert c.vq_setting == GRID and "vq = {'codebook': {'grid': 'uniform4', 'dim': 4}, 'per_group': 64}" in repr(c)
    c.set_vq(c.vq_setting)   # the property gives the spelling the setter accepts
    c.set_vq({"codebook": PAIRS, "granularity": "per_token", "norm": 2})
    assert c.vq_setting == {"codebook": PAIRS, "granularity": "per_token", "norm": 2.0} and float(c.vq_norm) == 2.0
    assert "<5 rows of 2>" in repr(c) and "per_token" in repr(c)
    c.set_vq(c.vq_setting)
    c.set_vq({"codebook": torch.tensor(PAIRS), "granularity": "per_group", "group_size": 32})
    assert c.vq_setting == {"codebook": PAIRS, "per_group": 32} and c.vq_codebook.shape == (5, 2)
    c.set_vq(None)
    assert sorted(c.state_dict()) == four and c.vq_setting is None
    for bad in (PAIRS, {"per_group": 64}, {"codebook": PAIRS, "block": 3}, {"codebook": PAIRS, "per_group": 64, "group_size": 64},
                {"codebook": PAIRS, "per_group": 64, "granularity": "per_token"}, {"codebook": PAIRS, "granularity": "per_token", "group_size": 8},
                {"codebook": "nf4"}, {"codebook": [[0.0] * 3] * 2}, {"codebook": PAIRS, "norm": -3}, {"codebook": PAIRS, "per_group": 7},
                {"codebook": {"grid": "nf4", "dim": 4}}):
        with pytest.raises(ValueError):
            c.set_vq(bad)
    assert sorted(c.state_dict()) == four   # a refused setting leaves nothing behind
    with pytest.raises(ValueError):
        c.fit_vq(torch.zeros(4, 64))        # nothing set
    same = dmx.CastTo()                     # a SAME cast stays the identity
    same.set_vq(GRID)
    x = make("normal", (4, 64), seed=1, dtype=F32)
    assert torch.equal(same(x), x)


def test_set_vq_is_exclusive_both_ways(dmx):
    ops = dmx.ops
    c = dmx.CastTo(format=INT4)
    c.set_vq(GRID)
    with pytest.raises(ValueError):
        c.set_codebook(ops.NF4)
    with pytest.raises(ValueError):
        c.set_dynamic("per_token")
    with pytest.raises(ValueError):
        c.set_scaling("per_token")
    with pytest.raises(ValueError):
        c.set_learnable("per_tensor")
    with pytest.raises(ValueError):
        c.set_pre_transform({"hadamard": 64})
    assert "hadamard" not in c.pre_transform and "codebook" not in c.state_dict()
    c.set_codebook(None), c.set_dynamic(None), c.set_scaling(None), c.set_learnable(None)   # switching OFF what is off stays legal
    for setup in (lambda k: k.set_codebook(ops.NF4), lambda k: k.set_dynamic("per_token"), lambda k: k.set_learnable("per_tensor"),
                  lambda k: k.set_pre_transform({"hadamard": 64})):
        k = dmx.CastTo(format=INT4)
        setup(k)
        with pytest.raises(ValueError):
            k.set_vq(GRID)
        assert "vq_codebook" not in k.state_dict() and k.vq_setting is None
    k = dmx.CastTo(format="FP[1|4|3,7](FN)")
    k.set_scaling({"per_group": 64})
    with pytest.raises(ValueError):
        k.set_vq(GRID)


def test_state_dict_round_trip_carries_table_and_norm(dmx):
    a = dmx.CastTo(format=INT4)
    a.set_vq(GRID)
    with torch.no_grad():
        a.vq_codebook.copy_(make("normal", (256, 4), seed=3, dtype=F32))
        a.vq_norm.fill_(1.0)
    b = dmx.CastTo(format=INT4)
    b.set_vq(GRID)
    b.load_state_dict(a.state_dict())
    assert torch.equal(b.vq_codebook, a.vq_codebook)
    s = b.vq_setting
    assert s["norm"] == 1.0 and s["per_group"] == 64 and s["codebook"] == a.vq_codebook.tolist()   # no longer the grid: the loaded rows
    c = dmx.CastTo(format=INT4)
    c.set_vq(GRID)
    c.load_state_dict(dmx.CastTo(format=INT4).state_dict(), strict=False)   # nothing about a table: the setting stays
    assert c.vq_setting == GRID
    d = dmx.CastTo(format=INT4)
    d.set_vq(GRID)
    d.load_state_dict(c.state_dict())                                       # the grid's own values: still the grid
    assert d.vq_setting == GRID


def test_configure_keys_and_cast_dict(dmx):
    m = dmx.nn.Linear(64, 8)
    token = {"codebook": PAIRS, "granularity": "per_token"}
    m.configure({"weight_format": INT4, "input_formats": [INT4], "weight_vq": GRID, "input_vq": token, "output_vq": None})
    assert m.weight_cast.vq_setting == GRID
    assert m.input_casts.input_cast.vq_setting == token
    assert all(c.vq_setting is None for c in m.output_casts.values())
    assert "weight_cast.vq_codebook" in m.state_dict() and "weight_cast.vq_norm" in m.state_dict() and "vq = " in repr(m)
    m.configure({"weight_vq": None, "input_vq": [None]})
    assert m.weight_cast.vq_setting is None and "weight_cast.vq_codebook" not in m.state_dict()
    assert m.input_casts.input_cast.vq_setting is None
    with pytest.raises(ValueError):
        m.input_casts.set_vq([GRID, GRID])
    with pytest.raises(ValueError):
        m.input_casts.set_vq("grid")


def test_every_procedure_refuses_a_vq_weight_cast(dmx):
    from dmx_compressor_amd import layer_reconstruction as LR
    m = dmx.nn.Linear(64, 8)
    LR.refuse_vq_weight_cast(m, "GPTQ")
    m.configure({"weight_format": INT4, "weight_vq": GRID})
    for what in ("GPTQ", "AWQ", "AWQ clipping", "Wanda", "HQQ", "AdaRound", "folding the weight"):
        with pytest.raises(NotImplementedError, match="vector codebook"):
            LR.refuse_vq_weight_cast(m, what)
    with pytest.raises(NotImplementedError, match="vector codebook"):
        m.fold_weight_and_bias()
    for cls, args in ((LR.OptimalBrainCompressor, ()), (LR.WandaCalibrator, ()), (LR.AWQCalibrator, (dmx.nn.DmxAWQHyperparams(),))):
        with pytest.raises(NotImplementedError, match="vector codebook"):
            cls(m, *args)
    import inspect
    src = inspect.getsource(LR)
    for what in ("GPTQ", "Wanda", "AWQ", "HQQ", "AWQ clipping", "AdaRound"):   # the call sits beside each procedure's other refusals
        assert f'refuse_vq_weight_cast(module, "{what}")' in src, what


# ------------------------------------------------------------------------------------------------ the C entries, on the CPU
def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def test_c_entries_answer_as_specified(dmx):
    from dmx_compressor_amd import _lib
    L = _lib.lib()
    OK, BAD, UNS = 0, 1, 2
    bf, f32 = _lib.dtype_code(BF16), _lib.dtype_code(F32)
    x, y = torch.zeros(256, dtype=BF16), torch.zeros(256, dtype=BF16)
    tb, acc, ws = torch.zeros(256, 8), torch.zeros(256, 10, dtype=torch.float64), torch.zeros(1 << 16, dtype=torch.float64)
    idx = torch.zeros(256, dtype=torch.uint8)
    assert x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0 and idx.data_ptr() % 16 == 0

    def qdq(in_=x, out=y, di=bf, do=bf, mode=0, n=4, S=64, table=tb, d=4, K=16, norm=0.0, index=None):
        return L.dmxq_vq_qdq(in_ if isinstance(in_, (ctypes.c_void_p, type(None))) else _p(in_), out if out is None else _p(out), di, do,
                             mode, n, S, table if table is None else _p(table), d, K, norm, None, index, None)

    def accu(in_=x, di=bf, mode=0, n=4, S=64, table=tb, d=4, K=16, norm=0.0, a=acc, w=ws):
        return L.dmxq_vq_accumulate(in_ if isinstance(in_, (ctypes.c_void_p, type(None))) else _p(in_), di, mode, n, S,
                                    table if table is None else _p(table), d, K, norm, a if a is None else _p(a), 0, w if w is None else _p(w), None)

    for call in (qdq, accu):
        assert call(S=48, n=5) == UNS                              # a group that is no power of two
        assert call(S=20, n=5, mode=1) == UNS                      # a row that is no multiple of a 16-byte vector
        assert call(in_=ctypes.c_void_p(x.data_ptr() + 2), n=3) == UNS   # a misaligned base
        assert call(in_=torch.zeros(256), di=f32, d=8) == UNS      # float32 takes d = 2 and 4
        assert call(in_=None) == BAD and call(table=None) == BAD   # null pointers
        assert call(K=1) == BAD and call(K=257) == BAD and call(n=-1) == BAD and call(mode=2) == BAD and call(di=99) == BAD
        assert call(d=3) == BAD and call(d=1) == BAD and call(d=16) == BAD and call(d=8, S=60, mode=1) == BAD   # a vector would straddle a segment
        assert call(norm=float("nan")) == BAD and call(norm=float("inf")) == BAD
        assert call(n=0) == OK                                     # an empty tensor: nothing launched
    assert qdq(do=f32) == UNS and qdq(di=f32, do=bf) == UNS        # mixed dtypes
    assert qdq(out=None) == BAD and qdq(do=99) == BAD
    assert qdq(index=ctypes.c_void_p(idx.data_ptr() + 8)) == UNS   # a misaligned index output
    assert accu(a=None) == BAD and accu(w=None) == BAD
    assert L.dmxq_vq_class(bf, 0, 64, 4, 256) == 1 and L.dmxq_vq_class(bf, 0, 48, 4, 256) == 0 and L.dmxq_vq_class(bf, 2, 64, 4, 256) == 0
    assert L.dmxq_vq_class(f32, 0, 64, 8, 256) == 0 and L.dmxq_vq_class(f32, 0, 64, 4, 256) == 1 and L.dmxq_vq_class(99, 0, 64, 4, 256) == 0
    assert L.dmxq_vq_workspace_bytes.restype is ctypes.c_int64
    assert L.dmxq_vq_workspace_bytes(bf, 0, 4, 64, 4, 16) == 16 * 6 * 8 and L.dmxq_vq_workspace_bytes(bf, 0, 4, 48, 4, 16) == 0
    assert L.dmxq_vq_workspace_bytes(bf, 0, 1 << 24, 64, 8, 256) == 2 * 256 * 256 * 10 * 8   # capped: two workgroups on each of 256 CUs
    assert L.dmxq_abi_version() == 4                               # an addition: the version stays


# ------------------------------------------------------------------------------------------------ the checker itself
def test_checker_ties_and_duplicates():
    """with s = 1 (the segment's maximum is the norm) u = x: a vector at the same distance from two rows keeps the lower index, in either
    order of the rows; of duplicate rows the first one wins"""
    x = torch.tensor([[0.0, 0.0, 0.5, 0.0, -0.5, 0.0, 0.25, 0.0]])      # norm 0.5: amax 0.5 gives s = 1
    for rows in ([[-0.5, 0.0], [0.5, 0.0]], [[0.5, 0.0], [-0.5, 0.0]]):
        y, s, idx = R.vq_ref(x, rows, "per_token")
        assert float(s[0]) == 1.0 and int(idx[0, 0]) == 0                # u = (0, 0): both at 0.25, index 0
        assert int(idx[0, 1]) == (1 if rows[0][0] < 0 else 0) and int(idx[0, 2]) == (0 if rows[0][0] < 0 else 1)
        assert y[0, :2].tolist() == rows[0]
    dup = [[0.25, 0.0], [0.5, 0.0], [0.25, 0.0], [-0.5, 0.0], [0.5, 0.0]]
    y, s, idx = R.vq_ref(x, dup, "per_token")
    assert float(s[0]) == 1.0 and idx[0].tolist() == [0, 1, 3, 0]        # rows 2 and 4 never win
    assert R.zero_row(R.table(dup)) == 0 and R.zero_row(R.table([[1.0, 0.0], [0.0, 0.5], [0.5, 0.0]])) == 1   # the lowest of equal minima


def test_checker_special_vectors_take_z():
    rows = [[1.0, 1.0], [0.25, -0.25], [-1.0, 0.5]]                      # z = 1, the default norm 1
    assert R.zero_row(R.table(rows)) == 1
    nan, inf = float("nan"), float("inf")
    y, s, idx = R.vq_ref(torch.tensor([[nan, 1.0, 1.0, 1.0]]), rows, "per_token")
    assert float(s[0]) == 1.0 and idx[0].tolist() == [1, 0]              # (NaN, 1) takes z; the segment's scale fell back to 1
    y, s, idx = R.vq_ref(torch.tensor([[inf, 0.0, -1.0, 0.5]]), rows, "per_token")
    assert float(s[0]) == 1.0 and idx[0].tolist() == [1, 2] and y[0].tolist() == [0.25, -0.25, -1.0, 0.5]   # (Inf, 0): every distance +Inf
    y, s, idx = R.vq_ref(torch.tensor([[3e38, 3e38, 1.0, 1.0]]), rows, "per_token", norm=3e38)
    assert float(s[0]) == 1.0 and idx[0].tolist() == [1, 0]              # the squares overflow: every distance +Inf, z
    y, s, idx = R.vq_ref(torch.zeros(2, 8, dtype=BF16), rows, "per_group", 4)
    assert torch.equal(s, torch.ones(4)) and bool((idx == 1).all())      # an all-zero segment: s = 1, every vector takes z
    assert y.dtype == BF16 and y[0].tolist() == [0.25, -0.25] * 4
    x = torch.full((1, 16), 2.0 ** -140)
    assert float(R.vq_ref(x, rows, "per_token")[1][0]) == 1.0            # a denormal maximum: s < 2^-126 gives 1


def test_checker_lookup_and_index_shape():
    x = make("heavy", (8, 128), seed=2, dtype=F32)
    for d, K in ((2, 16), (4, 200), (8, 2)):
        c = make("normal", (K, d), seed=K, dtype=F32)
        for norm in (None, 3.0):
            y, s, idx = R.vq_ref(x, c, "per_group", 32, norm)
            assert idx.dtype == torch.uint8 and idx.shape == (8, 128 // d) and int(idx.max()) < K
            assert torch.equal(c[idx.long()].reshape(-1, 32) * s[:, None], y.reshape(-1, 32)), (d, K)
            # the chosen row is a nearest row: no row is closer in the definition's own arithmetic
            u = (x.reshape(-1, 32) / s[:, None]).reshape(-1, d)
            D = torch.stack([R.distance(u, c[k]) for k in range(K)], dim=1)
            assert torch.equal(D.gather(1, idx.long().reshape(-1, 1))[:, 0], D.min(dim=1).values)


def test_checker_statistics_and_one_exact_step():
    """the statistics skip the vectors with a non-finite quotient; and one EXACT Lloyd step never raises the float64 error: with the
    assignment fixed the float64 centroid minimises sum w |u - c|^2 over every cell (allowance 1e-12: the float64 rounding of sums of
    up to 2^14 terms), and re-assigning every vector to a nearest row lowers each term (allowance 1e-6: the fp32 distances the
    definition compares carry a relative error of a few 2^-24, so a near-tie may pick the row that is that much farther)"""
    x = make("heavy", (64, 256), seed=5, dtype=F32)
    x[3, 7] = float("nan")
    x[9, 100] = float("inf")
    for d, K in ((2, 16), (4, 16), (8, 4)):
        c = R.sample_init(x[16:], K, d, "per_group", 64)
        A, mag = R.accumulate_ref(x, c, "per_group", 64, 1.0)
        seg, _, s, u, idx, _ = R.parts(x, c, "per_group", 64, 1.0)
        uv = u.reshape(-1, d)
        fin = torch.isfinite(uv).all(dim=1)
        assert int(A[:, d + 1].sum()) == int(fin.sum()) < uv.shape[0] and A.shape == (K, d + 2) and mag.shape == (K, d + 1)
        assert bool((mag[:, :d] >= A[:, :d].abs()).all()) and torch.equal(mag[:, d], A[:, d])
        w = (s.double() ** 2)[:, None].expand(-1, 64 // d).reshape(-1)[fin]
        ud, k = uv[fin].double(), idx.reshape(-1)[fin]

        def err(table64, assign):
            return float((w * ((ud - table64[assign]) ** 2).sum(dim=1)).sum())

        before = err(c.double(), k)
        exact = torch.where(A[:, d + 1:] > 0, A[:, :d] / A[:, d:d + 1], c.double())
        assert err(exact, k) <= before * (1 + 1e-12)
        c1 = R.kmeans_step(c, A)
        assert torch.equal(c1, exact.float())
        k1 = R.parts(x, c1, "per_group", 64, 1.0)[4].reshape(-1)[fin]
        assert err(c1.double(), k1) <= err(c1.double(), k) * (1 + 1e-6)
        empty = R.kmeans_step(c, torch.zeros(K, d + 2, dtype=torch.float64))
        assert torch.equal(empty, c)                                     # an empty row keeps its value


def test_checker_fit_history():
    for kind, d, K in (("normal", 2, 16), ("heavy", 4, 8)):
        x = make(kind, (32, 256), seed=d + K, dtype=F32)
        c0 = R.sample_init(x, K, d, "per_group", 64)
        c, norm, hist = R.fit_ref(x, c0, "per_group", 64, 1.0, iters=5)
        assert norm == 1.0 and len(hist) == 6 and c.shape == (K, d)
        assert all(b <= a * (1 + 1e-5) for a, b in zip(hist, hist[1:])), (kind, hist)   # the scalar fit's allowance: fp32 rounding of the rows
        assert hist[-1] < hist[0]
