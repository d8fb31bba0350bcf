"""Host tests (no GPU) of the codebook casts (ops.codebook_*, CastTo.set_codebook; DESIGN.md §8 "Codebook casts"): the vocabulary and its
ValueErrors, the exclusivity rules, the buffers, the configure keys, the C entries' refusals with libdmxq.so loaded on the CPU, and
the properties of the CPU checker itself (tests/_codebook_ref.py), which the GPU tests compare the kernels against."""
import ctypes
import math

import pytest
import torch

import _codebook_ref as R
from _data import make

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
INT4 = "XP[4,0](CSN)"


# ------------------------------------------------------------------------------------------------ named tables and the check
def test_named_tables(dmx):
    ops = dmx.ops
    assert tuple(ops.CODEBOOKS["nf4"]) == R.NF4 and len(R.NF4) == 16
    for v in ops.CODEBOOKS["nf4"]:
        assert float(torch.tensor(v, dtype=F32)) == v   # exactly representable in float32
    assert tuple(ops.CODEBOOKS["fp4_e2m1"]) == R.FP4_E2M1 and len(R.FP4_E2M1) == 15
    assert ops.CODEBOOKS["uniform"](5) == (-1.0, -0.5, 0.0, 0.5, 1.0)
    assert ops.CODEBOOKS["uniform"](16) == tuple(torch.linspace(-1, 1, 16, dtype=F32).tolist())
    assert ops.NF4 == {"codebook": "nf4", "per_group": 64}
    lv, g, gs, norm = ops.codebook_check("uniform8", "per_token", 64, None)
    assert len(lv) == 8 and (g, gs, norm) == ("per_token", None, None)
    assert ops.codebook_check([0, 1, 1, 2], "per_group", 32, 3)[1:] == ("per_group", 32, 3.0)


@pytest.mark.parametrize("bad", [
    dict(codebook="nf5"), dict(codebook="uniform"), dict(codebook=[1.0, 0.5]), dict(codebook=[0.0, float("nan")]),
    dict(codebook=[0.0, float("inf")]), dict(codebook=[0.5]), dict(codebook=list(range(257))), dict(codebook=torch.zeros(2, 2)),
    dict(codebook=3), dict(codebook="nf4", granularity="per_tile"), dict(codebook="nf4", granularity="per_group", group_size=0),
    dict(codebook="nf4", granularity="per_group", group_size=None), dict(codebook="nf4", norm=0.0), dict(codebook="nf4", norm=-1.0),
    dict(codebook="nf4", norm=float("inf")), dict(codebook="nf4", norm=float("nan")), dict(codebook="nf4", norm="1"),
])
def test_check_refuses(dmx, bad):
    with pytest.raises(ValueError):
        dmx.ops.codebook_check(**bad)


def test_front_end_errors_come_before_any_gpu_use(dmx):
    ops, x = dmx.ops, torch.zeros(4, 96, dtype=BF16)   # (a CPU tensor: a ValueError must come before the DmxqError of a non-GPU tensor)
    with pytest.raises(ValueError, match="multiple of the group size"):
        ops.codebook_qdq(x, "nf4", "per_group", 64)
    with pytest.raises(ValueError):
        ops.codebook_qdq(x, "nope")
    with pytest.raises(ValueError):
        ops.codebook_accumulate(x, "nf4", "per_group", 64)
    with pytest.raises(ValueError):
        ops.codebook_fit(x, [1.0, 0.0], "per_group", 32)
    with pytest.raises(ValueError):
        ops.codebook_fit([], "nf4")
    with pytest.raises(ValueError):
        ops.codebook_qdq(x, "nf4", "per_token", per_group=32)
    with pytest.raises(dmx.DmxqError):
        ops.codebook_qdq(x, "nf4", "per_group", 32)
    with pytest.raises(dmx.DmxqError):
        ops.codebook_qdq(torch.zeros(4, 128, dtype=BF16), **ops.NF4)   # the ready setting unpacks into the call


def test_class_follows_the_dynamic_float_cast(dmx):
    ops = dmx.ops
    for dtype in (BF16, F16, F32):
        for S in (8, 16, 32, 48, 64, 128, 256, 512, 768, 4096, 8192, 8200, 16384, 16392):
            assert ops.codebook_class(S, dtype, False) == ops.dynamic_float_class(S, dtype, "per_group"), (S, dtype)
            assert ops.codebook_class(S, dtype, True) == ops.dynamic_float_class(S, dtype, "per_token"), (S, dtype)
    assert ops.codebook_class(64, BF16) == "group" and ops.codebook_class(48, BF16) is None
    assert ops.codebook_class(8192, BF16, True) == "block_row" and ops.codebook_class(4096, F32, True) == "wave_row"
    assert ops.CODEBOOK_CHAIN_BY_DEFAULT <= {"group", "short_row", "wave_row", "block_row"}


# ------------------------------------------------------------------------------------------------ CastTo.set_codebook
def test_set_codebook_vocabulary_and_buffers(dmx):
    ops = dmx.ops
    c = dmx.CastTo(format=INT4)
    four = sorted(c.state_dict())
    assert len(four) == 4 and c.codebook_setting is None and "codebook" not in repr(c)
    c.set_codebook(ops.NF4)
    assert sorted(c.state_dict()) == sorted(four + ["codebook", "codebook_norm"])
    assert c.codebook.dtype == F32 and tuple(c.codebook.tolist()) == R.NF4
    assert c.codebook_setting == ops.NF4 and "codebook = {'codebook': 'nf4', 'per_group': 64}" in repr(c)
    c.set_codebook(c.codebook_setting)   # the property gives the spelling the setter accepts
    c.set_codebook({"codebook": [-1.0, 0.0, 0.5], "granularity": "per_token", "norm": 2})
    assert c.codebook_setting == {"codebook": [-1.0, 0.0, 0.5], "granularity": "per_token", "norm": 2.0}
    assert "<3 levels>" in repr(c) and "per_token" in repr(c)
    c.set_codebook(c.codebook_setting)
    c.set_codebook({"codebook": "fp4_e2m1", "granularity": "per_group", "group_size": 32})
    assert c.codebook_setting == {"codebook": "fp4_e2m1", "per_group": 32} and c.codebook.shape == (15,)
    c.set_codebook(None)
    assert sorted(c.state_dict()) == four and c.codebook_setting is None
    for bad in ("nf4", {"per_group": 64}, {"codebook": "nf4", "block": 3}, {"codebook": "nf4", "per_group": 64, "group_size": 64},
                {"codebook": "nf4", "per_group": 64, "granularity": "per_token"}, {"codebook": "nf4", "granularity": "per_token", "group_size": 8},
                {"codebook": "zzz"}, {"codebook": [2.0, 1.0]}, {"codebook": "nf4", "norm": -3}, {"codebook": "nf4", "per_group": -1}):
        with pytest.raises(ValueError):
            c.set_codebook(bad)
    assert sorted(c.state_dict()) == four   # a refused setting leaves nothing behind


def test_set_codebook_is_exclusive_both_ways(dmx):
    ops = dmx.ops
    c = dmx.CastTo(format=INT4)
    c.set_codebook(ops.NF4)
    with pytest.raises(ValueError):
        c.set_dynamic("per_token")
    with pytest.raises(ValueError):
        c.set_scaling("per_token")
    with pytest.raises(ValueError):
        c.set_learnable("per_tensor")
    with pytest.raises(ValueError):
        c.set_pre_transform({"hadamard": 64})
    assert "hadamard" not in c.pre_transform
    c.set_dynamic(None), c.set_scaling(None), c.set_learnable(None)   # switching OFF what is off stays legal
    for setup in (lambda k: k.set_dynamic("per_token"), lambda k: k.set_learnable("per_tensor"), lambda k: k.set_pre_transform({"hadamard": 64})):
        k = dmx.CastTo(format=INT4)
        setup(k)
        with pytest.raises(ValueError):
            k.set_codebook(ops.NF4)
        assert "codebook" not in k.state_dict()
    k = dmx.CastTo(format="FP[1|4|3,7](FN)")
    k.set_scaling({"per_group": 64})
    with pytest.raises(ValueError):
        k.set_codebook(ops.NF4)


def test_state_dict_round_trip_carries_table_and_norm(dmx):
    ops = dmx.ops
    a = dmx.CastTo(format=INT4)
    a.set_codebook(ops.NF4)
    with torch.no_grad():
        a.codebook.copy_(torch.linspace(-0.9, 1.1, 16))
        a.codebook_norm.fill_(1.0)
    b = dmx.CastTo(format=INT4)
    b.set_codebook(ops.NF4)
    b.load_state_dict(a.state_dict())
    assert torch.equal(b.codebook, a.codebook)
    s = b.codebook_setting
    assert s["norm"] == 1.0 and s["per_group"] == 64 and s["codebook"] == a.codebook.tolist()   # no longer "nf4": the loaded levels
    c = dmx.CastTo(format=INT4)
    c.set_codebook(ops.NF4)
    c.load_state_dict(dmx.CastTo(format=INT4).state_dict(), strict=False)   # nothing about a table: the setting stays
    assert c.codebook_setting == ops.NF4


def test_configure_keys_and_cast_dict(dmx):
    ops = dmx.ops
    m = dmx.nn.Linear(64, 8)
    m.configure({"weight_format": INT4, "input_formats": [INT4], "weight_codebook": ops.NF4,
                 "input_codebook": {"codebook": "fp4_e2m1", "granularity": "per_token"}, "output_codebook": None})
    assert m.weight_cast.codebook_setting == ops.NF4
    assert m.input_casts.input_cast.codebook_setting == {"codebook": "fp4_e2m1", "granularity": "per_token"}
    assert all(c.codebook_setting is None for c in m.output_casts.values())
    assert "weight_cast.codebook" in m.state_dict() and "codebook = " in repr(m)
    m.configure({"weight_codebook": None, "input_codebook": [None]})
    assert m.weight_cast.codebook_setting is None and "weight_cast.codebook" not in m.state_dict()
    assert m.input_casts.input_cast.codebook_setting is None
    with pytest.raises(ValueError):
        m.input_casts.set_codebook([ops.NF4, ops.NF4])
    with pytest.raises(ValueError):
        m.input_casts.set_codebook("nf4")


def test_calibration_procedures_refuse_a_codebook_weight_cast(dmx):
    from dmx_compressor_amd.layer_reconstruction import refuse_codebook_weight_cast
    m = dmx.nn.Linear(64, 8)
    refuse_codebook_weight_cast(m, "GPTQ")
    m.configure({"weight_format": INT4, "weight_codebook": dmx.ops.NF4})
    for what in ("GPTQ", "AWQ", "Wanda", "folding the weight"):
        with pytest.raises(NotImplementedError, match="codebook"):
            refuse_codebook_weight_cast(m, what)
    with pytest.raises(NotImplementedError, match="codebook"):
        m.fold_weight_and_bias()


# ------------------------------------------------------------------------------------------------ the C entries, on the CPU
def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def test_c_entries_refuse_as_specified(dmx):
    from dmx_compressor_amd import _lib
    L = _lib.lib()
    OK, BAD, UNS = 0, 1, 2
    bf, f32 = _lib.dtype_code(BF16), _lib.dtype_code(F32)
    x, y = torch.zeros(256, dtype=BF16), torch.zeros(256, dtype=BF16)
    lv, acc, ws = torch.tensor(R.NF4), torch.zeros(16, 3, dtype=torch.float64), torch.zeros(1 << 16, dtype=torch.float64)
    idx = torch.zeros(256, dtype=torch.uint8)
    assert x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0 and idx.data_ptr() % 16 == 0

    def qdq(in_=x, out=y, di=bf, do=bf, mode=0, n=4, S=64, lev=lv, K=16, norm=0.0, index=None):
        return L.dmxq_codebook_qdq(in_ if isinstance(in_, (ctypes.c_void_p, type(None))) else _p(in_), out if out is None else _p(out), di, do,
                                   mode, n, S, lev if lev is None else _p(lev), K, norm, None, index, None)

    def accu(in_=x, di=bf, mode=0, n=4, S=64, lev=lv, K=16, norm=0.0, a=acc, w=ws):
        return L.dmxq_codebook_accumulate(in_ if isinstance(in_, (ctypes.c_void_p, type(None))) else _p(in_), di, mode, n, S,
                                          lev if lev is None else _p(lev), K, norm, a if a is None else _p(a), 0, w if w is None else _p(w), None)

    for call in (qdq, accu):
        assert call(K=17) == UNS                                   # more levels than the kernels hold
        assert call(S=48, n=5) == UNS                              # a group that is no power of two
        assert call(in_=ctypes.c_void_p(x.data_ptr() + 2), n=3) == UNS   # a misaligned base
        assert call(in_=None) == BAD and call(lev=None) == BAD     # null pointers
        assert call(K=1) == BAD and call(K=257) == BAD and call(n=-1) == BAD and call(mode=2) == BAD and call(di=99) == BAD
        assert call(norm=float("nan")) == BAD and call(norm=float("inf")) == BAD
        assert call(n=0) == OK                                     # an empty tensor: nothing launched
    assert qdq(do=f32) == UNS and qdq(di=f32, do=bf) == UNS        # mixed dtypes
    assert qdq(out=None) == BAD and qdq(do=99) == BAD
    assert qdq(index=ctypes.c_void_p(idx.data_ptr() + 8)) == UNS   # a misaligned index output
    assert accu(a=None) == BAD and accu(w=None) == BAD
    assert L.dmxq_codebook_class(bf, 0, 64) == 1 and L.dmxq_codebook_class(bf, 0, 48) == 0 and L.dmxq_codebook_class(bf, 2, 64) == 0
    assert L.dmxq_codebook_workspace_bytes.restype is ctypes.c_int64
    assert L.dmxq_codebook_workspace_bytes(bf, 0, 4, 64) == 48 * 8 and L.dmxq_codebook_workspace_bytes(bf, 0, 4, 48) == 0
    assert L.dmxq_codebook_workspace_bytes(bf, 0, 1 << 24, 64) == 4 * 256 * 48 * 8   # capped: four workgroups on each of 256 CUs
    assert L.dmxq_abi_version() == 4


# ------------------------------------------------------------------------------------------------ the checker itself
def _neighbours(t):
    b = t.view(torch.int32)
    return torch.cat([t, (b + 1).view(F32), (b - 1).view(F32)])


@pytest.mark.parametrize("name", sorted(R.TABLES))
def test_checker_ties_nan_inf(name):
    levels = R.TABLES[name]
    c, t, z = R.table(levels)
    norm = float(R.norm_of(c)[0])
    pts = torch.cat([_neighbours(t), torch.tensor([float("inf"), float("-inf")])])
    S = 64
    x = torch.zeros(S)
    x[:pts.numel()] = pts
    x[-1] = norm   # the maximum IS the norm: s = 1 and u = x
    finite = x.clone()
    finite[torch.isinf(x)] = 0.0
    y, s, idx = R.codebook_ref(finite.reshape(1, S), levels, "per_token")
    assert float(s[0]) == 1.0
    for j in range(t.numel()):   # a tie goes to the lower level; one ulp above goes up
        first = int((t == t[j]).nonzero()[0])            # (duplicated thresholds: the count passes all of them at once)
        last = int((t == t[j]).nonzero()[-1])
        assert int(idx[0, j]) == (t < t[j]).sum() == first
        above = _neighbours(t[j:j + 1])[1 if t[j] >= 0 else 2]
        assert above > t[j]
        k = int(R.codebook_ref(torch.cat([above.reshape(1), torch.tensor([norm])]).reshape(1, 2), levels, "per_token")[2][0, 0])
        assert k == last + 1
    assert torch.equal(c[idx.long()[0]] * s[0], y[0])            # levels[idx] * scale == y
    # +-Inf saturate, NaN goes to z -- inside a segment whose maximum is not finite, so s = 1
    xi = torch.tensor([[float("inf"), float("-inf"), 0.25, -3.0]])
    y, s, idx = R.codebook_ref(xi, levels, "per_token")
    assert float(s[0]) == 1.0 and idx[0, 0] == len(levels) - 1 and idx[0, 1] == 0
    xn = torch.tensor([[float("nan"), 0.25, -3.0, 1.0]])
    y, s, idx = R.codebook_ref(xn, levels, "per_token")
    assert float(s[0]) == 1.0 and idx[0, 0] == z and float(y[0, 0]) == float(c[z])
    assert z == min(range(len(levels)), key=lambda i: (abs(levels[i]), i))


def test_checker_special_segments():
    y, s, idx = R.codebook_ref(torch.zeros(2, 64, dtype=BF16), R.NF4, "per_group", 64)
    assert torch.equal(s, torch.ones(2)) and bool((idx == 7).all()) and bool((y == 0).all())   # a zero segment: s = 1, y = c_z = 0
    y, s, idx = R.codebook_ref(torch.zeros(1, 16), R.TWO, "per_token")
    assert float(s[0]) == 1.0 and bool((idx == 0).all()) and bool((y == -0.5).all())          # c_z is not always 0
    x = torch.full((1, 16), 2.0 ** -140)
    assert float(R.codebook_ref(x, R.NF4, "per_token")[1][0]) == 1.0                            # a denormal maximum: s < 2^-126 gives 1
    x = make("heavy", (8, 128), seed=2, dtype=F32)
    for name, levels in R.TABLES.items():
        for norm in (None, 3.0):
            y, s, idx = R.codebook_ref(x, levels, "per_group", 32, norm)
            c = torch.tensor(levels)
            assert torch.equal(c[idx.long()].reshape(-1, 32) * s[:, None], y.reshape(-1, 32)), name
            assert idx.dtype == torch.uint8 and int(idx.max()) < len(levels)


def test_checker_statistics_and_lloyd_history():
    x = make("heavy", (64, 512), seed=5, dtype=F32)
    x[3, 7] = float("nan")
    x[9, 100] = float("inf")
    A, mag, wsum = R.accumulate_ref(x, R.NF4, "per_group", 64)
    seg, _, s, u, idx, c = R.parts(x, R.NF4, "per_group", 64)
    assert int(A[:, 2].sum()) == int(torch.isfinite(u).sum()) < x.numel()     # a non-finite u is skipped
    assert bool((mag >= A[:, 0].abs()).all())
    for kind in ("normal", "heavy"):
        for g, K in ((16, 4), (64, 16), (512, 8)):
            xs = make(kind, (64, 512), seed=g + K, dtype=F32)
            start = R.NF4 if K == 16 else tuple(torch.linspace(-1, 1, K).tolist())
            c, norm, hist = R.fit_ref(xs, start, "per_group", g, None, iters=7)
            assert norm == 1.0 and len(hist) == 8
            assert all(b <= a * (1 + 1e-6) for a, b in zip(hist, hist[1:])), (kind, g, K, hist)   # non-increasing
            assert hist[-1] < hist[0] and bool((c[1:] >= c[:-1]).all())
            assert all(math.isfinite(h) for h in hist)
