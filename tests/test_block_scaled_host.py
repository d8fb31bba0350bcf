"""CPU-side tests (-m "not gpu") of the two-level block-scaled float cast: the argument errors of ops.block_scaled_float_qdq that need no
GPU, the new keys of CastTo.set_scaling / CastToDict / configure (the old forms unchanged), the class and the argument checks of the C
entry, and the properties of the checker of tests/test_gpu_block_scaled.py (tests/_block_scaled_ref.py: the definition in torch with
the oracle's float cast)."""
import os

import pytest
import torch

import _block_scaled_ref as R
import _dynamic_float_ref as DR

E4M3, E5M2, E2M1, INT8 = "FP[1|4|3,7](_N)", "FP[1|5|2,15](_N)", "FP[1|2|1,1](_N)", "XP[8,0](CSN)"


# ------------------------------------------------------------------------------------------------ the op's argument errors
def test_op_value_errors_on_a_cpu_tensor(dmx):
    """every ValueError comes before the device is looked at (a CPU tensor that passes them all fails as any op does: DmxqError)"""
    f = dmx.ops.block_scaled_float_qdq
    x = torch.randn(4, 96)
    for fmt in (INT8, "BFP[8|8]{16}(SN)", "FP[0|4|4,7](FN)", "FP[1|8|7,127](FN)"):
        with pytest.raises(ValueError, match="format"):
            f(x, fmt, 16, E4M3)                                   # an element format that cannot be scaled
    for sf in (INT8, "BFP[8|8]{16}(SN)", "MXFP8[E4M3]{32}"):
        with pytest.raises(ValueError, match="scale_format must be a FloatingPoint"):
            f(x, E2M1, 16, sf)
    with pytest.raises(ValueError, match="8 exponent bits"):
        f(x, E2M1, 16, "FP[1|8|7,127](_N)")
    with pytest.raises(ValueError, match="round to nearest"):
        f(x, E2M1, 16, "FP[1|4|3,7](_S)")
    for bad in (0, -1.0, 481.0, float("nan"), float("inf"), "448", True):
        with pytest.raises(ValueError, match=r"scale_max must be a number in \(0, 480\]"):
            f(x, E2M1, 16, E4M3, scale_max=bad)
    for bad in ("static", [1.0], torch.ones(2), True):
        with pytest.raises(ValueError, match="tensor_scale must be"):
            f(x, E2M1, 16, E4M3, tensor_scale=bad)
    for bad_g in (None, 0, -16, 16.0, True):
        with pytest.raises(ValueError, match="group_size"):
            f(x, E2M1, bad_g, E4M3)
    with pytest.raises(ValueError, match="not a multiple of the group size 64"):
        f(x, E2M1, 64, E4M3)                                      # 96 % 64
    with pytest.raises(ValueError):
        f(torch.tensor(1.0), E2M1, 16, E4M3)
    with pytest.raises(ValueError, match="scale_max"):
        dmx.ops.block_scaled_tensor_scale(x, E2M1, E4M3, 500.0)
    for ok in (dict(), dict(scale_max=448.0), dict(scale_max=480), dict(tensor_scale=None), dict(tensor_scale=0.5),
               dict(scale_format=E5M2, scale_max=114688.0)):
        kw = dict(scale_format=E4M3)
        kw.update(ok)
        with pytest.raises(dmx.DmxqError):
            f(x, E2M1, 16, **kw)
    with pytest.raises(dmx.DmxqError):
        dmx.ops.block_scaled_tensor_scale(x, E2M1, E4M3, 448.0)


def test_nvfp4_setting(dmx):
    assert dmx.ops.NVFP4 == {"per_group": 16, "scale_format": "FP[1|4|3,7](_N)", "scale_max": 448.0, "tensor_scale": "dynamic"}
    fmt, sf, smax = dmx.ops.block_scaled_check(E2M1, 16, dmx.ops.NVFP4["scale_format"], dmx.ops.NVFP4["scale_max"])
    assert repr(fmt) == E2M1 and repr(sf) == E4M3 and smax == 448.0
    assert dmx.ops.block_scaled_check(E2M1, 16, E4M3)[2] == 480.0          # the default cap: the scale format's largest value
    assert dmx.ops.BLOCK_SCALED_CHAIN_BY_DEFAULT <= {"group"}


# ------------------------------------------------------------------------------------------------ set_scaling
def test_set_scaling_old_forms_unchanged(dmx):
    c = dmx.CastTo(format=E4M3)
    for setting, want in (("per_token", "per_token"), ({"per_group": 128}, {"per_group": 128}), ({"per_tile": 64}, {"per_tile": 64}),
                          ({"per_group": 32, "pow2_scale": True}, {"per_group": 32, "pow2_scale": True}),
                          ({"granularity": "per_tensor", "pow2_scale": True}, {"granularity": "per_tensor", "pow2_scale": True})):
        c.set_scaling(setting)
        assert c.scaling == want and c._block_scale is None
        assert f"scaling = {want!r}" in repr(c) and "scale_format" not in repr(c)
    c.set_scaling(None)
    assert c.scaling is None and c._block_scale is None and "scaling" not in repr(c)


def test_set_scaling_new_keys(dmx):
    c = dmx.CastTo(format=E2M1)
    c.set_scaling(dmx.ops.NVFP4)
    assert c.scaling == dmx.ops.NVFP4 and c._scaling == ("per_group", 16, False)
    assert "scale_format" in repr(c) and "448" in repr(c)
    c.set_scaling(c.scaling)                                      # the property's spelling is accepted back
    assert c.scaling == dmx.ops.NVFP4
    c.set_scaling({"per_group": 32, "scale_format": E5M2})        # the defaults: the format's largest value, a dynamic tensor scale
    assert c.scaling == {"per_group": 32, "scale_format": E5M2, "scale_max": 114688.0, "tensor_scale": "dynamic"}
    c.set_scaling({"per_group": 32, "scale_format": E4M3, "tensor_scale": None})
    assert c.scaling["tensor_scale"] is None and c.scaling["scale_max"] == 480.0
    before = c.scaling
    # the new keys only with per_group, not with pow2_scale, and never without a scale_format: each error names the remedy
    with pytest.raises(ValueError, match="per_group"):
        c.set_scaling({"granularity": "per_token", "scale_format": E4M3})
    with pytest.raises(ValueError, match="per_group"):
        c.set_scaling({"per_tile": 32, "scale_format": E4M3})
    with pytest.raises(ValueError, match="drop pow2_scale"):
        c.set_scaling({"per_group": 16, "scale_format": E4M3, "pow2_scale": True})
    with pytest.raises(ValueError, match="add 'scale_format'"):
        c.set_scaling({"per_group": 16, "scale_max": 448.0})
    with pytest.raises(ValueError, match="add 'scale_format'"):
        c.set_scaling({"per_group": 16, "tensor_scale": None})
    with pytest.raises(ValueError, match="scale_max"):
        c.set_scaling({"per_group": 16, "scale_format": E4M3, "scale_max": 500.0})
    with pytest.raises(ValueError, match="scale_format"):
        c.set_scaling({"per_group": 16, "scale_format": INT8})
    with pytest.raises(ValueError, match="tensor_scale"):
        c.set_scaling({"per_group": 16, "scale_format": E4M3, "tensor_scale": "static"})
    assert c.scaling == before                                    # nothing above took effect
    keys = set(c.state_dict())
    c.set_scaling(dmx.ops.NVFP4)
    assert set(c.state_dict()) == keys and "_block_scale" not in dict(c.named_buffers())
    c.set_scaling({"per_group": 16})                              # a plain setting clears the block keys
    assert c.scaling == {"per_group": 16} and c._block_scale is None
    # a format that cannot be scaled is refused in either order; SAME accepts the setting
    c = dmx.CastTo()
    c.set_scaling(dmx.ops.NVFP4)
    with pytest.raises(ValueError):
        c.set_format(INT8)
    c.set_format(E2M1)
    assert c.scaling == dmx.ops.NVFP4


def test_cast_dict_and_configure(dmx):
    lin = dmx.nn.Linear(64, 32)
    keys = set(lin.state_dict())
    lin.configure(dict(input_formats=[E2M1], weight_format=E2M1, output_formats=[E4M3], input_scaling=dmx.ops.NVFP4,
                       weight_scaling=dict(dmx.ops.NVFP4, tensor_scale=None), output_scaling={"per_group": 32, "scale_format": E5M2}))
    assert lin.input_casts.input_cast.scaling == dmx.ops.NVFP4
    assert lin.weight_cast.scaling == dict(dmx.ops.NVFP4, tensor_scale=None)
    assert lin.output_casts.output_cast.scaling["scale_format"] == E5M2
    assert set(lin.state_dict()) == keys
    with pytest.raises(ValueError):
        lin.configure(dict(weight_scaling={"per_tile": 32, "scale_format": E4M3}))
    add = dmx.nn.ResAdd()
    add.configure(dict(input_formats=[E2M1, E2M1]))
    add.input_casts.set_scaling(dmx.ops.NVFP4)                    # one setting for every cast
    assert [c.scaling for c in add.input_casts.values()] == [dmx.ops.NVFP4] * 2
    add.input_casts.set_scaling([None, dmx.ops.NVFP4])
    assert [c.scaling for c in add.input_casts.values()] == [None, dmx.ops.NVFP4]


def test_gptq_refuses_a_block_scaled_weight_cast(dmx):
    lin = dmx.nn.Linear(64, 32)
    lin.configure(dict(weight_format=E2M1, weight_scaling=dmx.ops.NVFP4))
    with pytest.raises(NotImplementedError, match="scaled"):
        with lin.optimal_brain_compressing(None):
            pass
    assert lin.weight_cast._flag("fake_quant_enabled")


# ------------------------------------------------------------------------------------------------ the library's host functions
def _have_lib(dmx):
    return os.path.exists(dmx.LIB_PATH)


def test_block_scaled_float_class(dmx):
    if not _have_lib(dmx):
        pytest.skip("libdmxq.so is not built")
    cls = dmx.ops.block_scaled_float_class
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        assert [cls(g, dt) for g in (4, 8, 16, 32, 48, 64, 128, 256, 512, 8192)] == \
            [None, None, "group", "group", None, "group", "group", "group", None, None]


def test_c_entry_argument_checks_without_gpu(dmx):
    if not _have_lib(dmx):
        pytest.skip("libdmxq.so is not built")
    import ctypes
    L, lib = dmx._lib.lib(), dmx._lib
    null, one, odd = ctypes.c_void_p(None), ctypes.c_void_p(16), ctypes.c_void_p(24)

    def call(i=one, o=one, di=lib.BF16, do=lib.BF16, n=4, g=16, man=1, exp=2, bias=1, flush=0, rnd=lib.ROUND_NEAREST, sman=3, sexp=4,
             sbias=7, sflush=0, srnd=lib.ROUND_NEAREST, smax=448.0):
        return L.dmxq_block_scaled_float_qdq(i, o, di, do, n, g, man, exp, bias, flush, rnd, sman, sexp, sbias, sflush, srnd, smax, null, null,
                                             null, null)

    assert call(n=0) == lib.OK
    assert call(i=null) == lib.ERR_BAD_ARG
    assert call(di=7) == lib.ERR_BAD_ARG
    assert call(n=-1) == lib.ERR_BAD_ARG
    assert call(exp=8) == lib.ERR_BAD_ARG and call(exp=0) == lib.ERR_BAD_ARG
    assert call(sexp=8) == lib.ERR_BAD_ARG and call(sexp=0) == lib.ERR_BAD_ARG
    assert call(rnd=9) == lib.ERR_BAD_ARG and call(srnd=9) == lib.ERR_BAD_ARG
    for bad in (0.0, -1.0, 481.0, float("nan"), float("inf")):
        assert call(smax=bad) == lib.ERR_BAD_ARG
    assert call(smax=480.0, n=0) == lib.OK
    # nothing launched, the caller's chain: (none of these touches the GPU)
    assert call(do=lib.F32) == lib.ERR_UNSUPPORTED
    assert call(rnd=lib.ROUND_STOCHASTIC) == lib.ERR_UNSUPPORTED
    assert call(srnd=lib.ROUND_STOCHASTIC) == lib.ERR_UNSUPPORTED
    assert call(i=odd) == lib.ERR_UNSUPPORTED and call(o=odd) == lib.ERR_UNSUPPORTED
    assert call(g=8) == lib.ERR_UNSUPPORTED and call(g=48) == lib.ERR_UNSUPPORTED and call(g=512) == lib.ERR_UNSUPPORTED
    assert call(man=23) == lib.ERR_UNSUPPORTED and call(sman=23) == lib.ERR_UNSUPPORTED


def test_c_tensor_scale_argument_checks_without_gpu(dmx):
    if not _have_lib(dmx):
        pytest.skip("libdmxq.so is not built")
    import ctypes
    L, lib = dmx._lib.lib(), dmx._lib
    null, one, odd = ctypes.c_void_p(None), ctypes.c_void_p(16), ctypes.c_void_p(24)

    def call(i=one, dt=lib.BF16, n=64, fmax=6.0, smax=448.0, t=one):
        return L.dmxq_block_scaled_tensor_scale(i, dt, n, fmax, smax, t, null)

    assert call(i=null) == lib.ERR_BAD_ARG and call(t=null) == lib.ERR_BAD_ARG
    assert call(dt=7) == lib.ERR_BAD_ARG and call(n=-8) == lib.ERR_BAD_ARG
    for bad in (0.0, -6.0, float("nan"), float("inf")):
        assert call(fmax=bad) == lib.ERR_BAD_ARG and call(smax=bad) == lib.ERR_BAD_ARG
    # nothing launched, the caller's existing reduction: (none of these touches the GPU)
    assert call(i=odd) == lib.ERR_UNSUPPORTED
    assert call(n=60) == lib.ERR_UNSUPPORTED and call(dt=lib.F32, n=62) == lib.ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ the checker's own properties
@pytest.fixture(scope="module")
def issue_case(oracle):
    torch.manual_seed(0)
    x = torch.randn(257, 1024) * torch.exp(2 * torch.randn(257, 1))
    return x, R.block_scaled_ref(oracle, x, R.FORMATS["e2m1"], 16, R.SCALE_FORMATS["e4m3"], 448.0)


def rel_l2(x, y):
    return float(((y.double() - x.double()) ** 2).sum().sqrt() / (x.double() ** 2).sum().sqrt())


def test_checker_scale_codes(oracle, issue_case):
    """every sq is a value of the scale format and <= 448; exactly one group -- the one that holds the tensor's maximum -- has sq == 448"""
    x, (y, s, sq, t) = issue_case
    assert y.shape == x.shape and y.dtype == x.dtype and s.shape == sq.shape == (257 * 64,) and t.shape == (1,)
    assert torch.equal(oracle.floating_point_cast(sq.clone(), *R.SCALE_FORMATS["e4m3"]), sq)
    assert float(sq.max()) == 448.0 and float(sq.min()) >= 0.0
    assert int((sq == 448.0).sum()) == 1
    assert int(torch.argmax(sq)) == int(torch.argmax(x.abs().reshape(-1, 16).amax(dim=1)))
    A = x.abs().max().reshape(1)
    assert torch.equal(t, (A / torch.full_like(A, 6.0)) / torch.full_like(A, 448.0))
    assert torch.equal(s, torch.where(sq * t >= 2.0 ** -126, sq * t, torch.zeros_like(s)))
    assert not torch.isnan(y).any() and torch.isfinite(y).all()


def test_checker_elements_on_the_grid(oracle, issue_case):
    """every y / s is a value of E2M1 (groups whose scale is unusable hold zeros)"""
    x, (y, s, sq, t) = issue_case
    live = s > 0
    grid = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
    # (y / s itself rounds once more: an element is on the grid when it IS one of the eight products grid value * s, each one fp32 multiply)
    products = grid[None, None, :] * s[live][:, None, None].expand(-1, 1, 8)
    assert bool((y.reshape(-1, 16)[live].abs()[:, :, None] == products).any(dim=2).all())
    assert bool((y.reshape(-1, 16)[~live] == 0).all())


def test_checker_error_between_the_two_existing_casts(oracle, issue_case):
    """the quantised scale costs accuracy against the float32 scale and gains against the power-of-two scale"""
    x, (y, s, sq, t) = issue_case
    f32 = rel_l2(x, DR.dynamic_float_ref(oracle, x, DR.FORMATS["e2m1"], "per_group", 16, False)[0])
    pow2 = rel_l2(x, DR.dynamic_float_ref(oracle, x, DR.FORMATS["e2m1"], "per_group", 16, True)[0])
    mine = rel_l2(x, y)
    print(f"relative L2 error: float32 scale {f32:.4f}, E4M3 scale capped at 448 {mine:.4f}, pow2_scale {pow2:.4f}")
    assert f32 < mine < pow2


def test_checker_special_groups(oracle):
    """the definition's stated outcomes: no NaN in the output; a NaN or Inf group gets sq = scale_max; a NaN anywhere makes the dynamic t
    1; an all-zero group and a group whose scale code is 0 hold signed zeros and report s = 0"""
    fmt, sf = R.FORMATS["e2m1"], R.SCALE_FORMATS["e4m3"]
    x = torch.full((6, 16), 3.0)
    x[0, 5] = float("nan")
    x[1, 7] = float("-inf")
    x[2] = 0.0
    x[3] = -0.0
    x[4] = 1e-40
    y, s, sq, t = R.block_scaled_ref(oracle, x, fmt, 16, sf, 448.0)
    assert float(t) == 1.0 and not torch.isnan(y).any()
    assert sq.tolist()[:4] == [448.0, 448.0, 0.0, 0.0] and s.tolist()[:4] == [448.0, 448.0, 0.0, 0.0]
    assert float(y[0, 5]) == 6.0 * 448.0 and float(y[1, 7]) == -6.0 * 448.0
    for r in (2, 3, 4):      # zeros carrying the sign bit of the unscaled cast of the elements
        assert bool((y[r] == 0).all()) and torch.equal(torch.signbit(y[r]), torch.signbit(oracle.floating_point_cast(x[r].clone(), *fmt)))
    assert float(s[4]) == 0.0 and bool((y[4] == 0).all())
    # without the NaN / Inf rows: the maximum's group sits on scale_max, a group 2^-25 below it falls to scale code 0
    x = torch.full((3, 16), 3.0)
    x[1] = -3.0 * 2.0 ** -25
    x[2, 3] = -96.0
    y, s, sq, t = R.block_scaled_ref(oracle, x, fmt, 16, sf, 448.0)
    assert float(sq[2]) == 448.0 and float(sq[1]) == 0.0 and float(s[1]) == 0.0
    assert bool((y[1] == 0).all()) and torch.equal(torch.signbit(y[1]), torch.signbit(oracle.floating_point_cast(x[1].clone(), *fmt)))
    assert float(y[2, 3]) == -96.0
    # a static t so small that every scale code is capped: elements saturate at +-fmax * s
    y, s, sq, t = R.block_scaled_ref(oracle, x, fmt, 16, sf, 448.0, tensor_scale=2.0 ** -40)
    assert sq.tolist() == [448.0] * 3 and float(y[2, 3]) == -6.0 * 448.0 * 2.0 ** -40
    for bad in (0.0, float("nan"), float("inf"), -1.0, 1e-39):
        assert float(R.block_scaled_ref(oracle, x, fmt, 16, sf, 448.0, tensor_scale=bad)[3]) == 1.0
