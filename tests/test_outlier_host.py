"""Host tests (no GPU) of the outlier-aware dynamic cast (ops.outlier_fixed_qdq, CastTo.set_dynamic with "outliers"; DESIGN.md §8
"Outlier-aware dynamic cast"): the argument checks that need no GPU, the storage-cost helper, the module settings and their read-back,
the refusals of GPTQ / AWQ / HQQ, and the properties of the CPU checker itself (tests/_outlier_ref.py), which the GPU tests compare
the kernel and the chain against."""
import math

import pytest
import torch

import _dynamic_ref as D
import _outlier_ref as R

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
INT4A = "XP[4,0](C_N)"
E5M10 = "FP[1|5|10,15](FN)"


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


# ------------------------------------------------------------------------------------------------ argument checks (no GPU)
def test_outlier_check_accepts_and_normalises(dmx):
    ops = dmx.ops
    fmt, g, k, of = ops.outlier_check(INT4A, 128, 2)
    assert repr(fmt) == INT4A and (g, k, of) == (128, 2, None)
    fmt, g, k, of = ops.outlier_check("XP[8,0](CSN)", None, 5, E5M10, "per_token")
    assert g is None and k == 5 and repr(of) == E5M10
    assert ops.outlier_check(INT4A, 16, 0)[2] == 0 and ops.outlier_check(INT4A, 16, 15)[2] == 15
    assert ops.OUTLIER_CHAIN_BY_DEFAULT is not None and ops.OUTLIER_KERNEL_MAX_K == 8
    assert ops._front._outlier_routes.keys() == {"fused", "chain"}
    for name in ("outlier_fixed_qdq", "outlier_check", "outlier_class", "outlier_bits_per_element", "OUTLIER_CHAIN_BY_DEFAULT"):
        assert name in ops.__all__ and hasattr(ops, name)


@pytest.mark.parametrize("bad", [
    dict(fmt="XP[4,1](CSN)"), dict(fmt="XP[4,0](_SN)"), dict(fmt="FP[1|4|3,7](FN)"), dict(fmt="BFP[8|8]{64}(SN)"), dict(fmt=4),
    dict(k=-1), dict(k=128), dict(k=200), dict(k=2.0), dict(k=True), dict(k=None),
    dict(group_size=0), dict(group_size=64.0), dict(group_size=None), dict(group_size=True),
    dict(outlier_format="XP[8,0](CSN)"), dict(outlier_format="BFP[8|8]{64}(SN)"), dict(outlier_format=16), dict(outlier_format="FP[1|8|23,127](_N)"),
    dict(granularity="per_tensor", group_size=None), dict(granularity="per_token"), dict(granularity="per_tile"),
])
def test_outlier_check_refuses(dmx, bad):
    with pytest.raises(ValueError):
        dmx.ops.outlier_check(**{"fmt": INT4A, "group_size": 128, "k": 2, **bad})


def test_front_end_errors_come_before_any_gpu_use(dmx):
    ops, x = dmx.ops, torch.zeros(4, 96, dtype=BF16)   # (a CPU tensor: a ValueError must come before the DmxqError of a non-GPU tensor)
    with pytest.raises(ValueError, match="multiple of the group size"):
        ops.outlier_fixed_qdq(x, INT4A, 64, 2)
    with pytest.raises(ValueError, match="smaller than the segment"):
        ops.outlier_fixed_qdq(x, INT4A, 32, 32)
    with pytest.raises(ValueError, match="smaller than the segment"):
        ops.outlier_fixed_qdq(x, INT4A, None, 96, granularity="per_token")
    with pytest.raises(ValueError):
        ops.outlier_fixed_qdq(x, INT4A, 32, -1)
    with pytest.raises(ValueError):
        ops.outlier_fixed_qdq(x, "FP[1|4|3,7](FN)", 32, 1)
    with pytest.raises(ValueError):
        ops.outlier_fixed_qdq(x, INT4A, 32, 1, outlier_format="XP[8,0](CSN)")
    with pytest.raises(ValueError):
        ops.outlier_fixed_qdq(torch.zeros(()), INT4A, 32, 1)
    for k in (0, 1):
        with pytest.raises(dmx.DmxqError):
            ops.outlier_fixed_qdq(x, INT4A, 32, k)
    with pytest.raises(dmx.DmxqError):
        ops.outlier_fixed_qdq(x, INT4A, None, 3, granularity="per_token")


def test_outlier_class_is_the_dynamic_casts_group_rule(dmx):
    ops = dmx.ops
    for dt in (BF16, F16, F32):
        for g in (1, 4, 8, 16, 24, 32, 48, 64, 128, 200, 256, 512, 1024):
            want = ops.dynamic_class(g, dt, False)
            assert ops.outlier_class(g, dt) == want and want in ("group", None)
        for g in (16, 32, 64, 128, 256):
            assert ops.outlier_class(g, dt) == "group"
    assert ops.outlier_class(0, BF16) is None


def test_bits_per_element_on_hand_computed_cases(dmx):
    b = dmx.ops.outlier_bits_per_element
    assert b(INT4A, 128, 2) == 4 + (16 + 4 + 2 * 23) / 128                      # the example of DESIGN.md: 4.515625
    assert b(INT4A, 128, 0) == 4 + 20 / 128                                       # no outliers: the scale and the zero point alone
    assert b(INT4A, 128, 2, symmetric_qscheme=True) == 4 + (16 + 2 * 23) / 128    # a symmetric scheme stores no zero point
    assert b("XP[8,0](CSN)", 16, 1, outlier_bits=8, scale_bits=32, zero_point_bits=0) == 8 + (32 + 0 + 1 * (8 + 4)) / 16
    assert b("XP[3,0](C_N)", 256, 8) == 3 + (16 + 3 + 8 * (16 + 8)) / 256
    assert b("XP[4,0](C_N)", 48, 4) == 4 + (16 + 4 + 4 * (16 + 6)) / 48           # ceil(log2 48) = 6
    for bad in (dict(k=128), dict(k=-1), dict(group_size=0), dict(fmt="FP[1|4|3,7](FN)")):
        with pytest.raises(ValueError):
            b(**{"fmt": INT4A, "group_size": 128, "k": 2, **bad})


# ------------------------------------------------------------------------------------------------ CastTo / module settings
OLD_SPELLINGS = [(None, None), (False, None), ("per_token", "per_token"), ("per_tensor", "per_tensor"), ({"per_group": 64}, {"per_group": 64}),
                 ({"per_group": 16}, {"per_group": 16})]


def test_every_earlier_set_dynamic_spelling_reads_back_unchanged(dmx):
    for fmt in ("SAME", "XP[8,0](CSN)", INT4A):
        c = dmx.CastTo(format=fmt)
        for setting, want in OLD_SPELLINGS:
            c.set_dynamic(setting)
            assert c.dynamic == want and c._outliers is None
            assert c._dynamic == (None if want is None else (("per_group", want["per_group"]) if isinstance(want, dict) else (want, None)))
        c.set_dynamic("per_group", 32)
        assert c.dynamic == {"per_group": 32} and c._dynamic == ("per_group", 32)
        r = repr(c)
        assert "dynamic = {'per_group': 32}" in r and "outlier" not in r
        c.set_dynamic(None)
        assert "dynamic" not in repr(c)
    for bad in ({"per_group": 0}, {"per_token": 1}, {"granularity": "per_token"}, "per_row", {"per_group": 64, "x": 1}):
        with pytest.raises(ValueError):
            dmx.CastTo(format=INT4A).set_dynamic(bad)


def test_set_dynamic_with_outliers_parses_and_reads_back(dmx):
    c = dmx.CastTo(format=INT4A)
    c.set_dynamic({"per_group": 64, "outliers": 2})
    assert c.dynamic == {"per_group": 64, "outliers": 2} and c._dynamic == ("per_group", 64)
    assert c._outliers == {"k": 2, "outlier_format": None}
    assert "dynamic = {'per_group': 64, 'outliers': 2}" in repr(c)
    c.set_dynamic({"per_group": 128, "outliers": 4, "outlier_format": E5M10})
    assert c.dynamic == {"per_group": 128, "outliers": 4, "outlier_format": E5M10} and repr(c._outliers["outlier_format"]) == E5M10
    assert E5M10 in repr(c)
    c.set_dynamic(c.dynamic)                                                  # the read-back is a setting
    assert c.dynamic == {"per_group": 128, "outliers": 4, "outlier_format": E5M10}
    c.set_dynamic({"granularity": "per_token", "outliers": 3})
    assert c.dynamic == {"granularity": "per_token", "outliers": 3} and c._dynamic == ("per_token", None)
    c.set_dynamic({"per_group": 64, "outliers": 0})                           # k = 0 is the plain setting
    assert c.dynamic == {"per_group": 64} and c._outliers is None
    c.set_dynamic({"per_group": 64, "outliers": 2})
    c.set_dynamic("per_token")                                                # a plain setting clears the outliers
    assert c.dynamic == "per_token" and c._outliers is None
    c.set_dynamic({"per_group": 64, "outliers": 2})
    c.set_dynamic(None)
    assert c.dynamic is None and c._outliers is None and c._dynamic is None
    for bad in ({"per_group": 64, "outliers": 64}, {"per_group": 64, "outliers": -1}, {"per_group": 64, "outliers": 1.0},
                {"per_group": 64, "outlier_format": E5M10}, {"granularity": "per_tensor", "outliers": 1},
                {"per_group": 64, "outliers": 1, "outlier_format": "XP[8,0](CSN)"}, {"outliers": 2},
                {"per_group": 64, "granularity": "per_token", "outliers": 1}):
        with pytest.raises(ValueError):
            c.set_dynamic(bad)
        assert c.dynamic is None                                              # a refused setting leaves the cast as it was
    # the format is re-checked when it comes later, and a float format is refused as for any dynamic cast
    s = dmx.CastTo(format="SAME")
    s.set_dynamic({"per_group": 64, "outliers": 2})
    s.set_format(INT4A)
    assert s.dynamic == {"per_group": 64, "outliers": 2}
    with pytest.raises(ValueError):
        s.set_format("FP[1|4|3,7](FN)")
    assert repr(s.format) == INT4A


def test_exclusive_sources_stay_exclusive(dmx):
    c = dmx.CastTo(format=INT4A)
    c.set_learnable("per_token", like=torch.zeros(4, 64))
    with pytest.raises(ValueError, match="learned"):
        c.set_dynamic({"per_group": 64, "outliers": 2})
    c = dmx.CastTo(format=INT4A)
    c.set_dynamic({"per_group": 64, "outliers": 2})
    with pytest.raises(ValueError):
        c.set_learnable("per_token", like=torch.zeros(4, 64))
    with pytest.raises(ValueError):
        c.set_codebook(dmx.ops.NF4)
    assert c.dynamic == {"per_group": 64, "outliers": 2}


def _linear(dmx, **config):
    m = dmx.nn.Linear(128, 16)
    m.configure(dict({"weight_format": INT4A, "input_formats": ["XP[8,0](C_N)"]}, **config))
    return m


def test_configure_carries_the_dict_and_adds_no_state(dmx):
    plain = _linear(dmx)
    keys = list(plain.state_dict().keys())
    setting = {"per_group": 64, "outliers": 2}
    m = _linear(dmx, weight_dynamic=setting, input_dynamic=dict(setting, outlier_format=E5M10),
                output_formats=["XP[8,0](C_N)"], output_dynamic={"granularity": "per_token", "outliers": 1})
    assert m.weight_cast.dynamic == setting and setting == {"per_group": 64, "outliers": 2}   # (the caller's dict is not modified)
    assert m.input_casts.input_cast.dynamic == {"per_group": 64, "outliers": 2, "outlier_format": E5M10}
    assert m.output_casts.output_cast.dynamic == {"granularity": "per_token", "outliers": 1}
    assert list(m.state_dict().keys()) == keys
    assert "'outliers': 2" in repr(m)
    m.configure({"weight_dynamic": {"per_group": 64}})
    assert m.weight_cast.dynamic == {"per_group": 64} and m.weight_cast._outliers is None


def test_gptq_awq_and_hqq_refuse_an_outlier_weight_cast(dmx):
    from dmx_compressor_amd import layer_reconstruction as LR
    setting = {"per_group": 64, "outliers": 2}
    m = _linear(dmx, weight_dynamic=setting)
    w0 = m.weight.detach().clone()
    for what in ("GPTQ", "AWQ", "HQQ"):
        with pytest.raises(NotImplementedError, match=what):
            LR.refuse_outlier_weight_cast(m, what)
    with pytest.raises(NotImplementedError, match="outlier"):
        with m.optimal_brain_compressing(None):
            pass
    assert m.obc is None and m.weight_cast._flag("fake_quant_enabled")
    with pytest.raises(NotImplementedError, match="outlier"):
        with m.awq_scaling(dmx.DmxAWQHyperparams()):
            pass
    assert m.awq is None
    with pytest.raises(NotImplementedError, match="outlier"):
        m.hqq_quantize()
    assert torch.equal(m.weight.detach(), w0) and not hasattr(m, "hqq_qparams") and m.weight_cast._flag("fake_quant_enabled")
    # without the outliers none of the three refuses for that reason
    LR.refuse_outlier_weight_cast(_linear(dmx, weight_dynamic={"per_group": 64}), "GPTQ")
    LR.refuse_outlier_weight_cast(dmx.nn.ReLU(), "GPTQ")


# ------------------------------------------------------------------------------------------------ the checker's own properties
@pytest.fixture(scope="module")
def heavy():
    return R.student_t3((256, 128), 2024)


def test_ref_k0_is_the_dynamic_ref(oracle, heavy):
    for g, qsym in ((128, False), (16, False), (64, True)):
        y, sc, zp, idx, val = R.outlier_ref(oracle, heavy, 4, False, g, 0, qsym)
        y0, sc0, zp0 = D.dynamic_ref(oracle, heavy, 4, False, g, qsym)
        assert torch.equal(_bits(y), _bits(y0)) and torch.equal(sc, sc0) and torch.equal(zp, zp0)
        assert idx.shape == (heavy.numel() // g, 0) and val.shape == idx.shape


@pytest.mark.parametrize("g", [128, 16])
def test_ref_error_falls_with_outliers(oracle, heavy, g):
    e = {k: R.rel_l2(heavy, R.outlier_ref(oracle, heavy, 4, False, g, k, False)[0]) for k in (0, 1, 2, 4, 8)}
    print(f"Student-t(3) [256,128] XP[4,0] affine g={g}: relative L2 " + ", ".join(f"k={k}: {v:.4f}" for k, v in e.items()))
    assert e[2] < e[0]
    assert e[8] < e[4] < e[2] < e[1] < e[0]


def test_ref_outliers_come_back_bit_identical(oracle, heavy):
    for dtype in (F32, BF16, F16):
        x = heavy.to(dtype)
        y, sc, zp, idx, val = R.outlier_ref(oracle, x, 4, False, 32, 3, False)
        assert y.dtype == dtype and idx.dtype == torch.int32 and idx.shape == (x.numel() // 32, 3) and val.dtype == dtype
        x2, y2 = x.reshape(-1, 32), y.reshape(-1, 32)
        assert torch.equal(_bits(y2.gather(1, idx.long())), _bits(x2.gather(1, idx.long()))) and torch.equal(_bits(val), _bits(x2.gather(1, idx.long())))
        # they are the three largest magnitudes, in order, and every other element is no larger than the third
        mag = x2.float().abs()
        top = mag.gather(1, idx.long())
        assert bool((top[:, 0] >= top[:, 1]).all()) and bool((top[:, 1] >= top[:, 2]).all())
        rest = mag.scatter(1, idx.long(), -1.0)
        assert bool((rest.amax(1) <= top[:, 2]).all())


def test_ref_ties_go_to_the_lower_index():
    x = torch.tensor([[1.0, -2.0, 2.0, 0.5, -2.0, 2.0, 0.0, -0.0]])
    assert R.rank(x, 4).tolist() == [[1, 2, 4, 5]]
    assert R.rank(torch.zeros(1, 8), 3).tolist() == [[0, 1, 2]]
    assert R.rank(torch.tensor([[0.0, float("inf"), float("nan"), -float("inf"), 3.0e38]]), 4).tolist() == [[2, 1, 3, 4]]


@pytest.mark.parametrize("planted", [float("inf"), -float("inf"), float("nan")])
def test_ref_a_planted_special_leaves_the_scale_of_the_rest(oracle, heavy, planted):
    g = 64
    x = heavy.clone()
    spots = [(0, 5), (3, 64), (200, 127)]
    for r, c in spots:
        x[r, c] = planted
    removed = x.clone()
    for r, c in spots:
        removed[r, c] = 0.0                                                   # the group with the planted element removed
    for k in (1, 2):
        y, sc, zp, idx, val = R.outlier_ref(oracle, x, 4, False, g, k, False)
        _, sc0, zp0, idx0, _ = R.outlier_ref(oracle, removed, 4, False, g, k - 1, False)
        assert bool(torch.isfinite(sc).all())
        for r, c in spots:
            s = r * 2 + c // g
            assert int(idx[s, 0]) == c % g                                    # the special ranks first
            assert float(sc[s]) == float(sc0[s]) and int(zp[s]) == int(zp0[s])
            got = y[r, c]
            assert (math.isnan(float(got)) and math.isnan(planted)) or float(got) == planted
        keep = torch.ones(sc.numel(), dtype=torch.bool)
        keep[[r * 2 + c // g for r, c in spots]] = False
        assert bool(torch.isfinite(y.reshape(-1, g)[keep]).all())
