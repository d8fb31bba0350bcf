"""Dynamic casts along a non-last dimension, the host side (no GPU): the class query over the supported / refused grid, the ValueError
refusals of the `dim` argument before any GPU use, and the header / SIGNATURES / ABI agreement of the three new entries."""
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32


@pytest.mark.parametrize("S,dtype,inner,want", [
    (16, BF, 8, "cols_r8"), (32, HF, 72, "cols_r8"), (64, F32, 4, "cols_r8"), (128, BF, 4096, "cols_r16"), (128, F32, 8, "cols_r16"),
    (256, F32, 136, "cols_r16w16"), (256, BF, 136, "cols_r16w16"), (256, HF, 8, "cols_r16w16"),
    (8, BF, 8, None), (512, F32, 8, None), (24, BF, 8, None), (48, F32, 4, None),   # not a power of two from 16 to 256
    (32, BF, 3, None), (32, BF, 12, None), (32, F32, 6, None), (32, F32, 0, None), (32, BF, 1, None)])   # inner: no whole 16-byte vectors
def test_dynamic_cols_class(dmx, S, dtype, inner, want):
    assert dmx.ops.dynamic_cols_class(S, dtype, inner) == want


@pytest.mark.parametrize("op,fmt", [("dynamic_fixed_qdq", "XP[8,0](CSN)"), ("dynamic_float_qdq", "FP[1|4|3,7](FN)")])
def test_dim_refusals_need_no_gpu(dmx, op, fmt):
    f = getattr(dmx.ops, op)
    x = torch.zeros(4, 48, 16)   # (a CPU tensor: every refusal below comes before the GPU check)
    with pytest.raises(ValueError, match="multiple of the group size"):
        f(x, fmt, "per_group", 32, dim=1)
    with pytest.raises(ValueError, match="per_group' / 'per_token' only"):
        f(x, fmt, "per_tensor", dim=0)
    with pytest.raises(ValueError, match="dim must be an integer"):
        f(x, fmt, "per_token", dim=3)
    if op == "dynamic_float_qdq":
        with pytest.raises(ValueError, match="per_group' / 'per_token' only"):
            f(x, fmt, "per_tile", 16, dim=-2)
    # the last dimension by any spelling is the old path: it gets as far as the GPU check
    with pytest.raises(dmx.DmxqError):
        f(x, fmt, "per_token", dim=2)
    with pytest.raises(dmx.DmxqError):
        f(x, fmt, "per_group", 16, dim=1)   # (a valid column call: refused for the CPU tensor only)


INT4, E4M3 = "XP[4,0](CSN)", "FP[1|4|3,7](FN)"


@pytest.mark.parametrize("setter,fmt,setting", [
    ("set_dynamic", INT4, {"per_group": 32, "dim": -2}), ("set_dynamic", INT4, {"granularity": "per_token", "dim": 0}),
    ("set_dynamic", INT4, {"per_group": 32, "dim": -1}), ("set_dynamic", INT4, {"per_group": 16, "outliers": 2, "dim": -1}),
    ("set_scaling", E4M3, {"per_group": 128, "dim": 0}), ("set_scaling", E4M3, {"granularity": "per_token", "dim": -2}),
    ("set_scaling", E4M3, {"per_group": 64, "pow2_scale": True, "dim": 1}),
    # without "dim": read back byte for byte as before
    ("set_dynamic", INT4, "per_token"), ("set_dynamic", INT4, "per_tensor"), ("set_dynamic", INT4, {"per_group": 32}),
    ("set_dynamic", INT4, {"per_group": 16, "outliers": 2}), ("set_scaling", E4M3, "per_token"), ("set_scaling", E4M3, {"per_tile": 32}),
    ("set_scaling", E4M3, {"per_group": 64, "pow2_scale": True}), ("set_scaling", E4M3, {"granularity": "per_token", "pow2_scale": True})])
def test_setting_round_trip(dmx, setter, fmt, setting):
    c = dmx.CastTo(format=fmt)
    getattr(c, setter)(setting)
    assert (c.dynamic if setter == "set_dynamic" else c.scaling) == setting
    assert not [k for k in c.state_dict() if "dim" in k] and len(c.state_dict()) == len(dmx.CastTo(format=fmt).state_dict())
    getattr(c, setter)(None)
    assert c.dynamic is None and c.scaling is None and c._dynamic_dim is None and c._scaling_dim is None


def test_configure_carries_the_setting(dmx):
    m = dmx.nn.Linear(64, 32)
    wd, idyn, osc = {"per_group": 32, "dim": 0}, {"granularity": "per_token", "dim": -2}, {"per_group": 16, "dim": -2}
    m.configure({"weight_format": INT4, "input_formats": [INT4], "output_formats": [E4M3], "weight_dynamic": wd, "input_dynamic": idyn,
                 "output_scaling": osc})
    assert m.weight_cast.dynamic == wd and m.input_casts.input_cast.dynamic == idyn
    assert all(c.scaling == osc for c in m.output_casts.values())
    m2 = dmx.nn.Linear(64, 32)
    m2.configure({"weight_format": E4M3, "input_formats": [E4M3], "output_formats": [INT4], "weight_scaling": wd, "input_scaling": idyn,
                  "output_dynamic": osc})
    assert m2.weight_cast.scaling == wd and m2.input_casts.input_cast.scaling == idyn
    assert all(c.dynamic == osc for c in m2.output_casts.values())
    assert set(m.state_dict()) == set(dmx.nn.Linear(64, 32).state_dict())


@pytest.mark.parametrize("setter,fmt,setting,match", [
    ("set_dynamic", INT4, {"per_group": 32, "outliers": 2, "dim": -2}, "outliers"),
    ("set_dynamic", INT4, {"granularity": "per_tensor", "dim": -2}, "per_tensor"),
    ("set_dynamic", INT4, {"per_group": 32, "dim": 1.0}, "integer"), ("set_dynamic", INT4, {"dim": -2}, "expected|granularity"),
    ("set_scaling", E4M3, {"per_group": 16, "scale_format": "FP[1|4|3,7](_N)", "dim": -2}, "scale_format"),
    ("set_scaling", E4M3, {"per_tile": 32, "dim": -2}, "per_tile")])
def test_set_time_refusals(dmx, setter, fmt, setting, match):
    c = dmx.CastTo(format=fmt)
    with pytest.raises(ValueError, match=match):
        getattr(c, setter)(setting)
    assert c.dynamic is None and c.scaling is None


@pytest.mark.parametrize("key", ["hadamard", "hadamard_row"])
def test_hadamard_refusals_in_either_order(dmx, key):
    spec = {key: 64 if key == "hadamard" else True}
    c = dmx.CastTo(format=INT4)
    c.set_dynamic({"per_group": 32, "dim": -2})
    with pytest.raises(ValueError, match="hadamard"):
        c.set_pre_transform(spec)
    assert key not in c.pre_transform
    c = dmx.CastTo(format=INT4)
    c.set_pre_transform(spec)
    with pytest.raises(ValueError, match="hadamard"):
        c.set_dynamic({"per_group": 32, "dim": -2})
    c.set_dynamic({"per_group": 32, "dim": -1})   # the last dimension, spelled out: accepted
    # a non-negative dim: only the tensor's rank can tell, so the refusal comes at the first forward, before any GPU use
    c.set_dynamic({"per_group": 32, "dim": 0})
    with pytest.raises(ValueError, match="hadamard"):
        c(torch.zeros(64, 64))
    o = dmx.CastTo(format=INT4)
    o.set_dynamic({"per_group": 16, "outliers": 2, "dim": 0})
    with pytest.raises(ValueError, match="outliers"):
        o(torch.zeros(64, 64))


def test_consumers_refuse_through_one_check(dmx):
    from dmx_compressor_amd import layer_reconstruction as LR
    m = dmx.nn.Linear(64, 32)
    m.configure({"weight_format": INT4, "weight_dynamic": {"per_group": 32, "dim": 0}})
    before = {k: v.clone() for k, v in m.state_dict().items()}
    calls = [lambda: LR.OptimalBrainCompressor(m), lambda: LR.WandaCalibrator(m), lambda: LR.AWQCalibrator(m, dmx.nn.DmxAWQHyperparams()),
             lambda: LR.refuse_awq_clip(m), lambda: LR.refuse_hqq(m), lambda: LR.refuse_adaround(m), m.fold_weight_and_bias]
    for call in calls:
        with pytest.raises(dmx.DmxqError, match="runs along the last dimension"):
            call()
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())
    m = dmx.nn.Linear(64, 32)   # (a scaled float weight cast: the calibrations refuse it anyway; folding reads it through the same check)
    m.configure({"weight_format": E4M3, "weight_scaling": {"per_group": 32, "dim": -2}})
    with pytest.raises(dmx.DmxqError, match="runs along the last dimension"):
        m.fold_weight_and_bias()
    m = dmx.nn.Linear(64, 32)
    m.configure({"weight_format": INT4, "weight_dynamic": {"per_group": 32, "dim": 1}})   # the last dimension of the 2-d weight: not refused
    LR.refuse_cols_weight_cast(m, "GPTQ")
    LR.OptimalBrainCompressor(m)


def test_header_signatures_and_abi(dmx):
    src = open(os.path.join(ROOT, "include", "dmxq.h")).read()
    L = dmx._lib.lib()
    for name in ("dmxq_dynamic_cols_class", "dmxq_dynamic_fixed_qdq_cols", "dmxq_dynamic_float_qdq_cols"):
        assert f"int {name}(" in src and name in dmx._lib.SIGNATURES and hasattr(L, name)
        assert src.split(f"int {name}(")[1].split(")")[0].count(",") + 1 == len(dmx._lib.SIGNATURES[name])
    assert L.dmxq_abi_version() == 4
    # refused before any launch, no device involved: a segment of 24, and in == out
    buf = torch.zeros(128, 16)
    p = buf.data_ptr()
    assert L.dmxq_dynamic_fixed_qdq_cols(p, p + 4096, 0, 0, 1, 48, 16, 24, 8, 0, 1, 1, 2, -127, 127, 1, None, None, None) == 2
    assert L.dmxq_dynamic_fixed_qdq_cols(p, p, 0, 0, 1, 64, 16, 16, 8, 0, 1, 1, 2, -127, 127, 1, None, None, None) == 1
