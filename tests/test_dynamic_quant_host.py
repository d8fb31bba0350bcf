"""CPU-side tests (-m "not gpu") of the dynamic integer cast: the checker of tests/test_gpu_dynamic_quant.py (tests/_dynamic_ref.py: the
oracle's three steps) against a plain-torch restatement of the reference's two formulas, and the host-side vocabulary --
CastTo.set_dynamic, the three configure keys, the argument errors of ops.dynamic_fixed_qdq that need no GPU."""
import pytest
import torch

import _dynamic_ref as R
from _data import bits_equal, make


@pytest.mark.parametrize("qsym", [False, True], ids=["affine", "symmetric"])
@pytest.mark.parametrize("precision,fsym", [(8, True), (8, False), (4, True)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_helper_is_the_two_reference_formulas(oracle, dtype, precision, fsym, qsym):
    """per-row and per-group segments of small finite tensors (heavy tails, ties on the rounding lattice, an all-zero, an all-positive
    and an all-negative row): oracle chain == torch restatement, bit for bit, scale and zero point included"""
    for kind, S in (("heavy", 40), ("ties", 16), ("normal", 8)):
        x = make(kind, (9, 80), seed=precision + S, dtype=dtype)
        x[2] = 0
        x[3] = x[3].abs() + 1
        x[4] = -x[4].abs() - 1
        want, wsc, wzp = R.torch_restatement(x, precision, fsym, S, qsym)
        got, sc, zp = R.dynamic_ref(oracle, x, precision, fsym, S, qsym)
        assert got.dtype == dtype and got.shape == x.shape
        assert bits_equal(sc, wsc) == 0 and bits_equal(zp, wzp) == 0, (kind, S)
        assert bits_equal(got, want) == 0, (kind, S)
        if not qsym:
            assert int(zp[3 * 80 // S]) == R.qrange(precision, fsym)[0]   # an all-positive segment: the zero point clamps to qmin
            assert int(zp[4 * 80 // S]) == R.qrange(precision, fsym)[1]   # an all-negative one: to qmax
        assert float(sc[2 * 80 // S]) == torch.finfo(torch.float32).eps   # an all-zero segment: the scale falls to eps


def test_set_dynamic_validation(dmx):
    c = dmx.CastTo(format="XP[8,0](CSN)")
    assert c.dynamic is None
    for bad in ("per_row", "token", 3, ("per_token",)):
        with pytest.raises(ValueError):
            c.set_dynamic(bad)
    for bad_g in (None, 0, -8, 2.0, True, "128"):
        with pytest.raises(ValueError):
            c.set_dynamic("per_group", bad_g)
    with pytest.raises(ValueError):
        c.set_dynamic("per_token", 128)          # a group size without per_group
    with pytest.raises(ValueError):
        c.set_dynamic({"per_group": 64, "x": 1})
    with pytest.raises(ValueError):
        c.set_dynamic(None, 64)
    assert c.dynamic is None                      # nothing above took effect
    c.set_dynamic("per_token")
    assert c.dynamic == "per_token"
    c.set_dynamic("per_group", 128)
    assert c.dynamic == {"per_group": 128}
    c.set_dynamic({"per_group": 32})
    assert c.dynamic == {"per_group": 32}
    c.set_dynamic("per_tensor")
    assert c.dynamic == "per_tensor"
    c.set_dynamic(None)
    assert c.dynamic is None


def test_dynamic_needs_an_integer_range_whichever_comes_second(dmx):
    for fmt in ("BFP[8|8]{64}(SN)", "FP[1|5|2,15](FN)", "XP[8,2](CSN)", "XP[8,0](_SN)"):
        c = dmx.CastTo(format=fmt)
        with pytest.raises(ValueError):
            c.set_dynamic("per_token")            # the format came first
        assert c.dynamic is None
        c = dmx.CastTo()                          # still SAME: the setting is accepted ...
        c.set_dynamic("per_token")
        with pytest.raises(ValueError):
            c.set_format(fmt)                     # ... and the format that comes second is refused
        assert isinstance(c.format, dmx.Same) and c.dynamic == "per_token"
        c.set_format("XP[4,0](CSN)")
        assert c.dynamic == "per_token" and c.format.precision == 4
        c.set_dynamic(None)
        c.set_format(fmt)                         # not dynamic any more: any format


def test_state_dict_and_repr(dmx):
    plain, dyn = dmx.CastTo(format="XP[8,0](CSN)"), dmx.CastTo(format="XP[8,0](CSN)")
    before = plain.extra_repr()
    dyn.set_dynamic("per_group", 64)
    assert list(dyn.state_dict().keys()) == list(plain.state_dict().keys())
    assert "dynamic" not in before and plain.extra_repr() == before
    assert dyn.extra_repr() == before + ", dynamic = {'per_group': 64}"
    dyn.set_dynamic("per_token")
    assert dyn.extra_repr() == before + ", dynamic = 'per_token'"
    dyn.set_dynamic(None)
    assert dyn.extra_repr() == before
    m, m0 = dmx.nn.Linear(16, 8), dmx.nn.Linear(16, 8)
    m.configure(dict(input_formats=["XP[8,0](CSN)"], weight_format="XP[8,0](CSN)", input_dynamic="per_token", weight_dynamic="per_token"))
    m0.configure(dict(input_formats=["XP[8,0](CSN)"], weight_format="XP[8,0](CSN)"))
    assert list(m.state_dict().keys()) == list(m0.state_dict().keys())
    m2 = dmx.nn.Linear(16, 8)
    m2.load_state_dict(m.state_dict())            # and a round trip through it


def test_configure_keys(dmx):
    m = dmx.nn.Linear(32, 16)
    fmts = dict(input_formats=["XP[8,0](CSN)"], output_formats=["XP[8,0](CSN)"], weight_format="XP[4,0](CSN)")
    m.configure(dict(fmts, input_dynamic="per_token", output_dynamic={"per_group": 16}, weight_dynamic="per_tensor"))
    assert m.input_casts.input_cast.dynamic == "per_token"
    assert m.output_casts.output_cast.dynamic == {"per_group": 16}
    assert m.weight_cast.dynamic == "per_tensor"
    m.configure(dict(input_dynamic=[None], output_dynamic={"output_cast": "per_token"}, weight_dynamic=None))
    assert m.input_casts.input_cast.dynamic is None
    assert m.output_casts.output_cast.dynamic == "per_token"
    assert m.weight_cast.dynamic is None
    with pytest.raises(ValueError):
        m.configure(dict(weight_dynamic="per_channel"))
    with pytest.raises(RuntimeError):
        m.configure(dict(input_dynamic={"no_such_cast": "per_token"}))
    two = dmx.nn.ResAdd()
    two.configure(dict(input_formats=["XP[8,0](CSN)", "XP[8,0](CSN)"], input_dynamic=["per_token", {"per_group": 32}]))
    assert [c.dynamic for c in two.input_casts.values()] == ["per_token", {"per_group": 32}]
    two.configure(dict(input_dynamic="per_tensor"))          # one setting: every cast of the group
    assert [c.dynamic for c in two.input_casts.values()] == ["per_tensor", "per_tensor"]
    # format and dynamic in one config: the format is set first, so a format without an integer range is refused
    bad = dmx.nn.Linear(32, 16)
    with pytest.raises(ValueError):
        bad.configure(dict(weight_format="BFP[8|8]{64}(SN)", weight_dynamic="per_token"))


def test_op_argument_errors_need_no_gpu(dmx):
    """every ValueError of ops.dynamic_fixed_qdq is raised before the tensor's device is looked at: a CPU tensor gets them, and only a
    valid call gets as far as the library's no-CPU-path error"""
    x = torch.zeros(4, 96)
    f = dmx.ops.dynamic_fixed_qdq
    with pytest.raises(ValueError):
        f(x, "BFP[8|8]{64}(SN)")
    with pytest.raises(ValueError):
        f(x, "XP[8,1](CSN)")
    with pytest.raises(ValueError):
        f(x, "XP[8,0](CSN)", "per_channel")
    with pytest.raises(ValueError):
        f(x, "XP[8,0](CSN)", "per_group")
    with pytest.raises(ValueError):
        f(x, "XP[8,0](CSN)", "per_group", 64)                # 96 % 64
    with pytest.raises(ValueError):
        f(x, "XP[8,0](CSN)", "per_token", 32)
    with pytest.raises(ValueError):
        f(torch.zeros(()), "XP[8,0](CSN)")
    with pytest.raises(dmx.DmxqError):
        f(x, "XP[8,0](CSN)", "per_group", 32)                # valid: the library has no CPU path
    assert dmx.ops.dynamic_class(128, torch.bfloat16, False) == "group"
    assert dmx.ops.dynamic_class(48, torch.bfloat16, False) is None and dmx.ops.dynamic_class(48, torch.bfloat16, True) == "short_row"
    assert dmx.ops.dynamic_class(8192, torch.bfloat16, True) == "wave_row" and dmx.ops.dynamic_class(8200, torch.bfloat16, True) == "block_row"
    assert dmx.ops.dynamic_class(4096, torch.float32, True) == "wave_row" and dmx.ops.dynamic_class(4100, torch.float32, True) == "block_row"
    assert dmx.ops.dynamic_class(1500, torch.bfloat16, True) is None and dmx.ops.dynamic_class(16392, torch.bfloat16, True) is None
    assert dmx.ops.dynamic_class(504, torch.bfloat16, True) == "short_row" and dmx.ops.dynamic_class(520, torch.bfloat16, True) == "wave_row"
    assert "DYNAMIC_ROUTES" not in dir(dmx.ops)              # the route counter of the tests is not part of the public surface
