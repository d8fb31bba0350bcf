"""CPU-side tests (-m "not gpu") of the dynamic scaled float cast: the host-side vocabulary -- CastTo.set_scaling, CastToDict, the three
configure keys, the argument errors of ops.dynamic_float_qdq that need no GPU, the geometry the library reports -- and the properties
of the checker of tests/test_gpu_dynamic_float.py (tests/_dynamic_float_ref.py: the definition in torch with the oracle's float cast)."""
import pytest
import torch

import _dynamic_float_ref as R
from _data import bits_equal, make

E4M3, E5M2, E2M1, INT8 = "FP[1|4|3,7](FN)", "FP[1|5|2,15](_N)", "FP[1|2|1,1](_N)", "XP[8,0](CSN)"


def test_fmax_table(dmx, oracle):
    """fmax = 2^(2^(e-1)) (2 - 2^-m), and it IS the largest output of the oracle's cast"""
    for name, want in (("e4m3", 480.0), ("e5m2", 114688.0), ("e2m1", 6.0)):
        man, exp, bias, flush = R.FORMATS[name]
        assert R.fmax_of(man, exp) == want == R.FMAX[name]
        assert dmx.ops.dynamic_float_fmax(dmx.Format.from_shorthand(R.SHORTHAND[name])) == want
        big = torch.tensor([3e38, -3e38, want, want * 1.5])
        assert oracle.floating_point_cast(big, man, exp, bias, flush).tolist() == [want, -want, want, want]


def test_set_scaling_validation(dmx):
    c = dmx.CastTo(format=E4M3)
    assert c.scaling is None
    for bad in ("per_row", "tile", 3, ("per_token",)):
        with pytest.raises(ValueError):
            c.set_scaling(bad)
    for gran in ("per_group", "per_tile"):
        for bad_g in (None, 0, -8, 2.0, True, "128"):
            with pytest.raises(ValueError):
                c.set_scaling(gran, bad_g)
    with pytest.raises(ValueError):
        c.set_scaling("per_token", 128)           # a group size without per_group / per_tile
    with pytest.raises(ValueError):
        c.set_scaling({"per_group": 64, "x": 1})
    with pytest.raises(ValueError):
        c.set_scaling({"per_group": 64, "per_tile": 64})
    with pytest.raises(ValueError):
        c.set_scaling(None, 64)
    with pytest.raises(ValueError):
        c.set_scaling("per_token", pow2_scale=1)  # not a bool
    with pytest.raises(ValueError):
        c.set_scaling(None, pow2_scale=True)
    assert c.scaling is None                       # nothing above took effect
    c.set_scaling("per_token")
    assert c.scaling == "per_token"
    c.set_scaling("per_group", 128)
    assert c.scaling == {"per_group": 128}
    c.set_scaling({"per_tile": 64})
    assert c.scaling == {"per_tile": 64}
    c.set_scaling(("per_group", 32))               # the pair, as the definition writes a segment
    assert c.scaling == {"per_group": 32}
    with pytest.raises(ValueError):
        c.set_scaling(("per_group", 32), 64)
    assert c.scaling == {"per_group": 32}
    c.set_scaling({"per_tile": 128, "pow2_scale": True})
    assert c.scaling == {"per_tile": 128, "pow2_scale": True}
    c.set_scaling("per_tensor", pow2_scale=True)
    assert c.scaling == {"granularity": "per_tensor", "pow2_scale": True}
    c.set_scaling(c.scaling)                       # the property's spelling is accepted back
    assert c.scaling == {"granularity": "per_tensor", "pow2_scale": True}
    assert "scaling" in repr(c)
    c.set_scaling(None)
    assert c.scaling is None and "scaling" not in repr(c)


def test_scaling_is_a_plain_attribute(dmx):
    c = dmx.CastTo(format=E4M3)
    keys = set(c.state_dict())
    c.set_scaling("per_token")
    assert set(c.state_dict()) == keys and not any("scaling" in k for k in keys)
    assert "_scaling" not in dict(c.named_buffers())


def test_formats_that_cannot_be_scaled_in_both_orders(dmx):
    """refused in set_scaling when the format is there, in set_format when it comes second; a SAME cast accepts the setting"""
    for fmt in (INT8, "BFP[8|8]{16}(SN)", "FP[0|4|4,7](FN)", "FP[1|8|7,127](FN)", "MXFP8[E4M3]{32}"):
        c = dmx.CastTo(format=fmt)
        with pytest.raises(ValueError):
            c.set_scaling("per_token")
        assert c.scaling is None
        c = dmx.CastTo()                           # SAME
        c.set_scaling({"per_group": 32})
        with pytest.raises(ValueError):
            c.set_format(fmt)
        assert repr(c.format) == "SAME"
        c.set_format(E5M2)
        assert repr(c.format) == E5M2 and c.scaling == {"per_group": 32}
    c = dmx.CastTo(format=E4M3)
    c.set_scaling("per_token")
    c.set_format("SAME")                           # back to SAME is always possible
    c.set_format(E2M1)


def test_set_dynamic_still_refuses_float_formats(dmx):
    for fmt in (E4M3, E5M2, E2M1):
        c = dmx.CastTo(format=fmt)
        with pytest.raises(ValueError):
            c.set_dynamic("per_token")
        with pytest.raises(ValueError):
            dmx.ops.dynamic_check(fmt, "per_token")
        c.set_scaling("per_token")                 # the float formats' own setting
        assert c.dynamic is None and c.scaling == "per_token"
    c = dmx.CastTo(format=INT8)
    c.set_dynamic("per_token")
    assert c.dynamic == "per_token" and c.scaling is None


def test_cast_dict_and_configure(dmx):
    lin = dmx.nn.Linear(64, 32)
    lin.configure(dict(input_formats=[E4M3], weight_format=E4M3, output_formats=[E5M2], input_scaling="per_token",
                       weight_scaling={"per_tile": 32}, output_scaling={"per_group": 16, "pow2_scale": True}))
    assert lin.input_casts.input_cast.scaling == "per_token"
    assert lin.weight_cast.scaling == {"per_tile": 32}
    assert lin.output_casts.output_cast.scaling == {"per_group": 16, "pow2_scale": True}
    assert not any("scaling" in k for k in lin.state_dict())
    lin.configure(dict(input_scaling=None))
    assert lin.input_casts.input_cast.scaling is None and lin.weight_cast.scaling == {"per_tile": 32}
    with pytest.raises(ValueError):
        lin.configure(dict(weight_scaling="per_channel"))
    with pytest.raises(ValueError):
        lin.configure(dict(weight_format=INT8))    # the format comes second
    add = dmx.nn.ResAdd()
    add.configure(dict(input_formats=[E4M3, E4M3]))
    add.input_casts.set_scaling(["per_token", None])
    assert [c.scaling for c in add.input_casts.values()] == ["per_token", None]
    add.input_casts.set_scaling({"per_group": 32})
    assert [c.scaling for c in add.input_casts.values()] == [{"per_group": 32}] * 2
    keys = list(add.input_casts.keys())
    add.input_casts.set_scaling({keys[1]: "per_tensor"})
    assert [c.scaling for c in add.input_casts.values()] == [{"per_group": 32}, "per_tensor"]
    with pytest.raises(ValueError):
        add.input_casts.set_scaling(["per_token"])
    with pytest.raises(RuntimeError):
        add.input_casts.set_scaling({"no_such_cast": "per_token"})
    with pytest.raises(ValueError):
        add.input_casts.set_scaling(3)


def test_gptq_refuses_a_scaled_weight_cast(dmx):
    lin = dmx.nn.Linear(64, 32)
    lin.configure(dict(weight_format=E4M3, weight_scaling="per_token"))
    with pytest.raises(NotImplementedError, match="scaled"):
        with lin.optimal_brain_compressing(None):
            pass
    assert lin.weight_cast._flag("fake_quant_enabled")   # refused before any switch was touched


def test_op_value_errors_on_a_cpu_tensor(dmx):
    """every ValueError comes before the device is looked at (a CPU tensor that passes them all fails as any op does: DmxqError)"""
    f = dmx.ops.dynamic_float_qdq
    x = torch.randn(4, 64, 96)
    for fmt in (INT8, "BFP[8|8]{16}(SN)", "FP[0|4|4,7](FN)", "FP[1|8|7,127](FN)", "FP[1|8|23,127](_N)"):
        with pytest.raises(ValueError):
            f(x, fmt)
    with pytest.raises(ValueError):
        f(x, E4M3, "per_channel")
    with pytest.raises(ValueError):
        f(x, E4M3, "per_group")                    # no group size
    with pytest.raises(ValueError):
        f(x, E4M3, "per_tile", 0)
    with pytest.raises(ValueError):
        f(x, E4M3, "per_token", 32)                # a group size that goes with nothing
    with pytest.raises(ValueError):
        f(x, E4M3, "per_group", 64)                # 96 % 64
    with pytest.raises(ValueError):
        f(x, E4M3, "per_tile", 64)                 # 96 % 64
    with pytest.raises(ValueError):
        f(x.transpose(1, 2), E4M3, "per_tile", 64)
    with pytest.raises(ValueError):
        f(torch.randn(64), E4M3, "per_tile", 32)   # tiles need two dims
    with pytest.raises(ValueError):
        f(torch.tensor(1.0), E4M3)
    for ok in (dict(granularity="per_token"), dict(granularity="per_group", group_size=48), dict(granularity="per_tile", group_size=32),
               dict(granularity="per_tensor", pow2_scale=True)):
        with pytest.raises(dmx.DmxqError):
            f(x, E4M3, **ok)


def test_dynamic_float_class(dmx):
    """the geometry the library itself reports (no GPU): groups are powers of two from 16 to 256; rows any multiple of a 16-byte vector
    up to 16384 -- a wave's while they fit 8 sixteen-bit (16 fp32) vectors per lane, a workgroup's beyond; tiles 32 / 64 / 128"""
    cls = dmx.ops.dynamic_float_class
    rows16 = {16: "group", 48: "short_row", 128: "group", 256: "group", 768: "wave_row", 4096: "wave_row", 8192: "block_row",
              8200: "block_row", 16384: "block_row", 16392: None, 4100: None}
    for dt in (torch.bfloat16, torch.float16):
        assert {s: cls(s, dt, "per_token") for s in rows16} == rows16
        assert cls(4104, dt, "per_token") == "block_row" and cls(4096, dt, "per_tensor") == "wave_row"
    rows32 = {16: "group", 48: "short_row", 128: "group", 256: "group", 768: "wave_row", 4096: "wave_row", 4100: "block_row",
              8192: "block_row", 8200: "block_row", 16384: "block_row", 16392: None, 4098: None}
    assert {s: cls(s, torch.float32, "per_token") for s in rows32} == rows32
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        assert [cls(g, dt, "per_group") for g in (8, 16, 32, 48, 64, 128, 256, 512, 8192)] == \
            [None, "group", "group", None, "group", "group", "group", None, None]
        assert [cls(g, dt, "per_tile") for g in (16, 32, 48, 64, 128, 256)] == [None, "tile", None, "tile", "tile", None]
    assert dmx.ops.DYNAMIC_FLOAT_CHAIN_BY_DEFAULT <= {"group", "short_row", "wave_row", "block_row", "tile"}


def test_c_entry_argument_checks_without_gpu(dmx):
    import ctypes
    L, lib = dmx._lib.lib(), dmx._lib
    null, one, odd = ctypes.c_void_p(None), ctypes.c_void_p(16), ctypes.c_void_p(24)
    GROUP, ROWS, TILE = 0, 1, 2

    def call(i=one, o=one, di=lib.BF16, do=lib.BF16, mode=ROWS, n=4, seg=64, rows=0, cols=0, man=3, exp=4, bias=7, flush=0,
             rnd=lib.ROUND_NEAREST, pow2=0):
        return L.dmxq_dynamic_float_qdq(i, o, di, do, mode, n, seg, rows, cols, man, exp, bias, flush, rnd, pow2, null, null)

    assert call(n=0) == lib.OK
    assert call(i=null) == lib.ERR_BAD_ARG
    assert call(di=7) == lib.ERR_BAD_ARG
    assert call(mode=3) == lib.ERR_BAD_ARG
    assert call(exp=8) == lib.ERR_BAD_ARG                       # fp32's exponent range: no finite maximum
    assert call(n=-1) == lib.ERR_BAD_ARG
    assert call(mode=TILE, seg=32, rows=64, cols=48, n=2) == lib.ERR_BAD_ARG    # 48 % 32
    assert call(mode=TILE, seg=32, rows=64, cols=64, n=3) == lib.ERR_BAD_ARG    # four tiles, not three
    # nothing launched, the caller's chain: (none of these touches the GPU)
    assert call(do=lib.F32) == lib.ERR_UNSUPPORTED
    assert call(rnd=lib.ROUND_STOCHASTIC) == lib.ERR_UNSUPPORTED
    assert call(i=odd) == lib.ERR_UNSUPPORTED
    assert call(mode=GROUP, seg=48) == lib.ERR_UNSUPPORTED
    assert call(seg=16392) == lib.ERR_UNSUPPORTED
    assert call(mode=TILE, seg=48, rows=96, cols=96, n=4) == lib.ERR_UNSUPPORTED
    assert call(man=23) == lib.ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ the checker's own properties
@pytest.mark.parametrize("name", ["e4m3", "e4m3_flush", "e5m2", "e2m1"])
@pytest.mark.parametrize("gran,g", [("per_token", None), ("per_group", 16), ("per_tile", 32), ("per_tensor", None)])
def test_checker_properties(oracle, name, gran, g):
    """heavy-tailed bf16 data with an all-zero segment: scale 1 and zeros there; with pow2_scale no |x / s| exceeds fmax and every scale
    is a power of two at least amax / fmax; finite input gives finite output; without pow2_scale the segment's maximum lands on fmax"""
    fmt, fmax = R.FORMATS[name], R.FMAX[name]
    x = make("heavy", (2, 64, 96), seed=3, dtype=torch.bfloat16)
    if gran == "per_tile":
        x[0, :32, :32] = 0
    elif gran != "per_tensor":
        x[0, 0] = 0
    seg, _, sc_shape = R.to_segments(x.float(), gran, g)
    amax = seg.abs().amax(dim=1)
    for pow2 in (False, True):
        y, s = R.dynamic_float_ref(oracle, x, fmt, gran, g, pow2)
        assert y.dtype == x.dtype and y.shape == x.shape and tuple(s.shape) == sc_shape and s.dtype == torch.float32
        assert bool(torch.isfinite(y.float()).all())
        s = s.reshape(-1)
        if gran != "per_tensor":
            assert float(s[0]) == 1.0 and float(amax[0]) == 0.0
            yseg, _, _ = R.to_segments(y.float(), gran, g)
            assert bits_equal(yseg[0], torch.zeros_like(yseg[0])) == 0
        live = amax > 0
        exact = amax[live].double() / fmax
        if pow2:
            assert bool((s.view(torch.int32) & 0x007FFFFF == 0).all())                 # powers of two
            assert bool((s[live].double() >= exact).all()) and bool((s[live].double() < 2 * exact * (1 + 2.0 ** -23)).all())
            assert float((seg / s[:, None]).abs().max()) <= fmax
        else:
            assert bool(((s[live].double() - exact).abs() <= exact * 2.0 ** -24).all())   # one rounding of the quotient
            q = oracle.floating_point_cast((seg / s[:, None].expand_as(seg)).contiguous(), *fmt)
            assert bool((q.abs().amax(dim=1)[live] == fmax).all())


def test_checker_special_segments(oracle):
    """the definition's stated outcomes: a NaN or an Inf anywhere in a segment makes its scale 1, and float_q saturates both; a
    segment of denormals falls below 2^-126 and gets scale 1 as well unless pow2_scale rounds its scale up to 2^-126; the pow2 rule on the bits rounds UP and leaves powers of two"""
    fmt, fmax = R.FORMATS["e4m3"], 480.0
    x = torch.full((5, 32), 3.0)
    x[0, 5] = float("nan")
    x[1, 7] = float("-inf")
    x[2] = 1e-40
    x[3, 0] = 3e38
    x[3, 1:] = 1e-3
    for pow2 in (False, True):
        y, s = R.dynamic_float_ref(oracle, x, fmt, "per_token", None, pow2)
        assert s[:2].tolist() == [1.0, 1.0] and float(s[2]) == (2.0 ** -126 if pow2 else 1.0)
        assert float(y[0, 5]) == fmax and float(y[1, 7]) == -fmax and float(y[0, 0]) == 3.0 and float(y[1, 0]) == 3.0
        assert bool((y[2] == 0).all()) != pow2     # (scaled by 2^-126 the denormals land on the format's subnormal grid)
        assert bool(torch.isfinite(y).all())
        assert float(y[3, 1]) == 0.0 and abs(float(y[3, 0]) / 3e38 - 1) < 2.0 ** -3
    amax = torch.tensor([480.0, 481.0, 960.0, 0.0, float("inf"), float("nan"), 1e-40])
    assert R.scale_rule(amax, fmax, True).tolist() == [1.0, 2.0, 2.0, 1.0, 1.0, 1.0, 2.0 ** -126]
    assert R.scale_rule(amax, fmax, False)[[0, 2, 3, 4, 5, 6]].tolist() == [1.0, 2.0, 1.0, 1.0, 1.0, 1.0]
