"""Learned step size casts (LSQ / LSQ+; DESIGN.md §8 "Learned step size") without a GPU: (a) the tests' reference (_lsq_ref.py) against
torch's own CPU learnable fake-quantize ops; (b) everything that answers or raises before any GPU use."""
import ctypes

import pytest
import torch

from _lsq_ref import lsq_ref, sum_bound

CASES = [("p8_affine", -128, 127), ("p4_affine", -8, 7), ("p4_symmetric_range", -7, 7)]
N_SEG, S = 6, 64


def _inputs(qmin, qmax, n_seg=N_SEG):
    """x = (k + f) s - zq s with integer k from two steps below qmin to two steps above qmax and |f| <= 0.375 (<= 0.4: torch rounds
    x * (1 / s) + zp, this library x / s + zq; that far from a tie both give k).  s are powers of two, f multiples of 1 / 8 and g
    multiples of 1 / 16: every per-element operation of either library is then EXACT (x * (1 / s) = x / s, (xfq - x) / s = q - v, the
    products have < 24 bits), so the two results can differ by nothing but the order and width of the sums -- which is what the bound
    covers (torch sums its float32 terms in float32: exact here, the terms being multiples of 2^-12 below 2^11)."""
    gen = torch.Generator().manual_seed(1234 + qmax)
    s = torch.tensor([2.0 ** e for e in (-5, -3, -2, -1, 0, 1)][:n_seg])
    zq = torch.tensor([0, 1, -2, 3, qmin + 1, qmax - 1][:n_seg]).float().clamp(qmin, qmax)
    k = torch.randint(qmin - 2, qmax + 3, (n_seg, S), generator=gen).float()
    k[:, 0], k[:, 1], k[:, 2] = qmin - 2, qmax + 2, zq   # every segment holds all three kinds
    f = torch.randint(-3, 4, (n_seg, S), generator=gen).float() / 8
    g = torch.randint(-32, 33, (n_seg, S), generator=gen).float() / 16
    x = (k + f) * s[:, None] - zq[:, None] * s[:, None]
    return x, g, s, zq, k


def _pos_zero(t):
    """torch forms dx as dy * mask, whose zero carries dy's sign, where the definition selects (in ? g : 0) and gives +0; and a v in
    (-0.5, 0) rounds to -0, which this library's forward keeps through (q - zq) * s and torch's does not.  The sign of a zero is the
    one thing taken out of the bit-for-bit comparisons of y and dx (-0 + 0 = +0, every other value is unchanged)"""
    return t + 0.0


def _close(got, ref, n, abs_t, k=1.0):
    return bool(((got.double() - ref.double()).abs() <= sum_bound(ref, n, abs_t, k)).all())


@pytest.mark.parametrize("name,qmin,qmax", CASES)
@pytest.mark.parametrize("grad_factor", [1.0, 0.125])
def test_reference_matches_torch_per_channel(name, qmin, qmax, grad_factor):
    x, g, s, zq, k = _inputs(qmin, qmax)
    assert (k < qmin).any() and (k > qmax).any() and ((k >= qmin) & (k <= qmax)).any()
    assert (zq != 0).any() and (zq >= qmin).all() and (zq <= qmax).all()
    y, dx, ds, dz, abs_ts, abs_tz = lsq_ref(x, g, s, zq, qmin, qmax, k=grad_factor)
    xt, st, zt = x.clone().requires_grad_(), s.clone().requires_grad_(), zq.clone().requires_grad_()
    yt = torch._fake_quantize_learnable_per_channel_affine(xt, st, zt, 0, qmin, qmax, grad_factor)
    yt.backward(g)
    assert torch.equal(_pos_zero(yt.detach()).view(torch.int32), _pos_zero(y).view(torch.int32))
    assert torch.equal(_pos_zero(xt.grad).view(torch.int32), dx.view(torch.int32))
    assert (dx == 0).any() and (dx != 0).any()
    assert _close(st.grad, ds, S, abs_ts, grad_factor), (st.grad, ds)
    assert _close(zt.grad, dz, S, abs_tz, grad_factor), (zt.grad, dz)


@pytest.mark.parametrize("name,qmin,qmax", CASES)
def test_reference_matches_torch_per_tensor(name, qmin, qmax):
    x, g, s, zq, k = _inputs(qmin, qmax)
    x, g, k = x[1:2], g[1:2], k[1:2]
    s, zq = s[1:2], zq[1:2]   # (scale 2^-3, zero point 1)
    assert (k < qmin).any() and (k > qmax).any() and ((k >= qmin) & (k <= qmax)).any()
    y, dx, ds, dz, abs_ts, abs_tz = lsq_ref(x, g, s, zq, qmin, qmax)
    xt, st, zt = x.clone().requires_grad_(), s.clone().requires_grad_(), zq.clone().requires_grad_()
    yt = torch._fake_quantize_learnable_per_tensor_affine(xt, st, zt, qmin, qmax, 1.0)
    yt.backward(g)
    assert torch.equal(_pos_zero(yt.detach()).view(torch.int32), _pos_zero(y).view(torch.int32))
    assert torch.equal(_pos_zero(xt.grad).view(torch.int32), dx.view(torch.int32))
    assert _close(st.grad, ds, S, abs_ts) and _close(zt.grad, dz, S, abs_tz)


@pytest.mark.parametrize("name,qmin,qmax", CASES)
def test_reference_y_and_dx_match_torch_on_general_scales(name, qmin, qmax):
    """arbitrary scales and fractions |f| <= 0.4: torch's x * (1 / s) + zp and this library's x / s + zq differ in the last bits, but
    both round to k, so y and dx agree bit for bit (up to the sign of a zero); ds / dz are NOT compared here: torch's float32
    (xfq - x) / s differs from q - v in the last places, which the bound of a reordered sum does not cover"""
    gen = torch.Generator().manual_seed(77 + qmax)
    s = torch.rand(N_SEG, generator=gen) * 0.1 + 0.01
    zq = torch.tensor([0, 1, -2, 3, qmin + 1, qmax - 1]).float().clamp(qmin, qmax)
    k = torch.randint(qmin - 2, qmax + 3, (N_SEG, S), generator=gen).float()
    k[:, 0], k[:, 1], k[:, 2] = qmin - 2, qmax + 2, zq
    f = (torch.rand(N_SEG, S, generator=gen) - 0.5) * 0.8
    g = torch.randn(N_SEG, S, generator=gen)
    x = (k + f) * s[:, None] - zq[:, None] * s[:, None]
    y, dx, _, _, _, _ = lsq_ref(x, g, s, zq, qmin, qmax)
    xt, st, zt = x.clone().requires_grad_(), s.clone().requires_grad_(), zq.clone().requires_grad_()
    yt = torch._fake_quantize_learnable_per_channel_affine(xt, st, zt, 0, qmin, qmax, 1.0)
    yt.backward(g)
    assert torch.equal(_pos_zero(yt.detach()).view(torch.int32), _pos_zero(y).view(torch.int32))
    assert torch.equal(_pos_zero(xt.grad).view(torch.int32), dx.view(torch.int32))
    assert (dx == 0).any() and (dx != 0).any()


def test_learnable_and_hadamard_are_refused_in_either_order(dmx):
    w = torch.zeros(32, 64)
    c = dmx.CastTo("XP[4,0](CSN)")
    c.set_pre_transform({"hadamard": 64})
    with pytest.raises(ValueError, match="hadamard"):
        c.set_learnable("per_token", like=w)
    assert c.learnable is None and not any("learned" in k for k in c.state_dict())
    d = dmx.CastTo("XP[4,0](CSN)")
    d.set_learnable("per_token", like=w)
    with pytest.raises(ValueError, match="hadamard"):
        d.set_pre_transform({"hadamard": 64})
    assert "hadamard" not in d.pre_transform
    m = dmx.nn.Linear(64, 32, bias=False)
    with pytest.raises(ValueError, match="hadamard"):
        m.configure({"weight_format": "XP[4,0](CSN)", "weight_learnable": "per_token", "pre_weight_transform": {"hadamard": 64}})


def test_reference_nan_outcomes():
    """a NaN x: dx 0 there and ds NaN for its segment; a NaN g: ds NaN, and the NaN is passed on as dx where the element is inside"""
    x, g, s, zq, _ = _inputs(-8, 7)
    x[0, 5] = float("nan")
    g[1, 3] = float("nan")
    x[1, 3] = 0.0   # inside
    _, dx, ds, dz, _, _ = lsq_ref(x, g, s, zq, -8, 7)
    assert dx[0, 5] == 0 and torch.isnan(ds[0]) and torch.isnan(ds[1]) and torch.isnan(dx[1, 3])
    assert not torch.isnan(ds[2:]).any()


# ---------------------------------------------------------------------------------------------------- (b) validation, no GPU
def test_class_and_scratch_queries_answer_without_gpu(dmx):
    ops = dmx.ops
    assert ops.lsq_class(128, torch.bfloat16, "per_group") == "group"
    assert ops.lsq_class(16, torch.float32, "per_group") == "group" and ops.lsq_class(24, torch.bfloat16, "per_group") is None
    assert ops.lsq_class(48, torch.bfloat16, "per_token") == "short_row"
    assert ops.lsq_class(768, torch.bfloat16, "per_token") == "wave_row"
    assert ops.lsq_class(8192, torch.bfloat16, "per_token") == "wave_row" and ops.lsq_class(8200, torch.bfloat16, "per_token") == "block_row"
    assert ops.lsq_class(16384, torch.float32, "per_token") == "block_row" and ops.lsq_class(16392, torch.bfloat16, "per_token") is None
    assert ops.lsq_class(8, torch.bfloat16, "per_tensor") == "tensor" and ops.lsq_class(1 << 33, torch.float16, "per_tensor") == "tensor"
    assert ops.lsq_class(12, torch.bfloat16, "per_tensor") is None and ops.lsq_class(12, torch.float32, "per_tensor") == "tensor"
    L = dmx._lib.lib()
    one = L.dmxq_lsq_scratch_bytes(8)
    assert one == 16 and L.dmxq_lsq_scratch_bytes(0) == 16 and L.dmxq_lsq_scratch_bytes(-1) == 0
    n = 8
    while L.dmxq_lsq_scratch_bytes(n) == one:
        n *= 2
    assert L.dmxq_lsq_scratch_bytes(n) == 2 * one and ops.lsq_scratch_bytes(n) == 2 * one
    assert L.dmxq_lsq_scratch_bytes(1 << 40) % 16 == 0   # (capped by the device's size, a whole number of rows)


def test_entry_refuses_before_any_launch(dmx):
    L, lib = dmx._lib.lib(), dmx._lib
    null, p = ctypes.c_void_p(None), ctypes.c_void_p(4096)

    def call(x=p, g=p, dx=p, dt=(lib.BF16, lib.BF16, lib.BF16), n=4, seg=128, mode=0, prec=4, rnd=lib.ROUND_NEAREST, q=(-8, 7), scratch=null, sb=0):
        return L.dmxq_lsq_backward(x, g, dx, dt[0], dt[1], dt[2], n, seg, mode, prec, rnd, q[0], q[1], p, p, 1.0, 1, p, p, scratch, sb, null)

    assert call(n=0) == lib.OK
    assert call(x=null) == lib.ERR_BAD_ARG and call(q=(7, 7)) == lib.ERR_BAD_ARG and call(dt=(9, lib.BF16, lib.BF16)) == lib.ERR_BAD_ARG
    assert call(mode=2, n=2, seg=4096) == lib.ERR_BAD_ARG
    assert call(x=ctypes.c_void_p(4098)) == lib.ERR_UNSUPPORTED            # a base that is not 16-byte aligned
    assert call(seg=24) == lib.ERR_UNSUPPORTED and call(seg=20) == lib.ERR_UNSUPPORTED   # outside the classes / not whole vectors
    assert call(seg=16392, mode=1) == lib.ERR_UNSUPPORTED
    assert call(dt=(lib.BF16, lib.F32, lib.BF16)) == lib.ERR_UNSUPPORTED   # mixed dtypes
    assert call(rnd=lib.ROUND_STOCHASTIC) == lib.ERR_UNSUPPORTED and call(prec=23) == lib.ERR_UNSUPPORTED
    assert call(mode=2, n=1, seg=4096) == lib.ERR_UNSUPPORTED               # the tensor class without scratch
    assert call(mode=2, n=1, seg=1 << 20, scratch=p, sb=16) == lib.ERR_BAD_ARG   # a scratch smaller than the query says


def test_front_end_raises_value_errors_on_cpu_tensors(dmx):
    ops = dmx.ops
    x, g = torch.zeros(4, 64), torch.zeros(4, 64)
    s, z = torch.ones(4), torch.zeros(4)
    with pytest.raises(ValueError, match="granularity"):
        ops.lsq_backward(x, g, s, z, "XP[4,0](CSN)", "per_row")
    with pytest.raises(ValueError, match="multiple of the group size"):
        ops.lsq_backward(x, g, torch.ones(12), torch.zeros(12), "XP[4,0](CSN)", "per_group", 24)
    with pytest.raises(ValueError, match="FixedPoint"):
        ops.lsq_backward(x, g, s, z, "FP[1|4|3,7](FN)", "per_token")
    with pytest.raises(ValueError, match="FixedPoint"):
        ops.lsq_fixed_qdq(x, s, z, "BFP[8|8]{64}(SN)", "per_token")
    with pytest.raises(ValueError, match="one per segment"):
        ops.lsq_fixed_qdq(x, torch.ones(3), z, "XP[4,0](CSN)", "per_token")
    with pytest.raises(ValueError, match="grad_scale"):
        ops.lsq_fixed_qdq(x, s, z, "XP[4,0](CSN)", "per_token", grad_scale="esser")
    with pytest.raises(ValueError, match="granularity"):
        ops.lsq_class(64, torch.float32, "per_row")
    assert ops.lsq_grad_factor("lsq", 64, 7) == 1.0 / (64 * 7) ** 0.5 and ops.lsq_grad_factor(None, 64, 7) == 1.0
    assert ops.lsq_grad_factor(0.25, 64, 7) == 0.25
    with pytest.raises(dmx.DmxqError):   # valid arguments, but no CPU path
        ops.lsq_backward(x, g, s, z, "XP[4,0](CSN)", "per_token")


def test_set_learnable_validation_and_state_dict(dmx):
    w = torch.zeros(32, 64)
    plain = dmx.CastTo("XP[4,0](CSN)")
    keys = set(plain.state_dict())
    assert {"scale", "zero_point", "fake_quant_enabled", "observer_enabled"} <= keys
    assert not any("learned" in k for k in keys) and plain.learnable is None and "learnable" not in plain.extra_repr()
    assert keys - {"scale", "zero_point", "fake_quant_enabled", "observer_enabled"} == \
        {"activation_post_process." + k for k in plain.activation_post_process.state_dict()}
    assert [n for n, _ in plain.named_parameters()] == []

    c = dmx.CastTo("XP[4,0](CSN)")
    c.set_learnable({"per_group": 16}, like=w, learn_zero_point=True)
    assert c.learned_scale.shape == (128,) and c.learned_zero_point.shape == (128,) and c.learned_zero_point.requires_grad
    assert c.learned_scale.dtype == torch.float32 and c._learnable_pending   # (a CPU weight: the values come with the first forward)
    assert set(c.state_dict()) == keys | {"learned_scale", "learned_zero_point"}
    assert c.learnable == {"granularity": {"per_group": 16}, "learn_zero_point": True, "grad_scale": "lsq", "init": "minmax"}
    assert "learnable" in c.extra_repr()
    with pytest.raises(ValueError, match="exclusive"):
        c.set_dynamic("per_token")
    with pytest.raises(ValueError, match="exclusive"):
        c.set_scaling("per_token")
    sd = {k: v.clone() for k, v in c.state_dict().items()}
    sd["learned_scale"] += 1.0
    c.load_state_dict(sd)
    assert not c._learnable_pending and float(c.learned_scale.detach()[0]) == 2.0
    c.set_learnable(None)
    assert set(c.state_dict()) == keys and c.learnable is None and [n for n, _ in c.named_parameters()] == []
    c.set_dynamic("per_token")   # (allowed again)

    d = dmx.CastTo("XP[4,0](CSN)")
    d.set_dynamic("per_token")
    with pytest.raises(ValueError, match="exclusive"):
        d.set_learnable("per_token", like=w)
    e = dmx.CastTo("FP[1|4|3,7](FN)")
    e.set_scaling("per_token")
    with pytest.raises(ValueError, match="exclusive"):
        e.set_learnable("per_tensor")

    a = dmx.CastTo("XP[8,0](CSN)")
    with pytest.raises(ValueError, match="per_tensor"):
        a.set_learnable("per_token")           # an activation cast: no tensor to take a shape from
    with pytest.raises(ValueError, match="per_tensor"):
        a.set_learnable({"per_group": 16})
    a.set_learnable("per_tensor")
    assert a.learned_scale.shape == (1,) and not a.learned_zero_point.requires_grad
    for bad in (dict(granularity="per_row", like=w), dict(granularity="per_group", group_size=24, like=w),
                dict(granularity="per_token", like=w, init="kmeans"), dict(granularity="per_token", like=w, grad_scale="x")):
        with pytest.raises(ValueError):
            dmx.CastTo("XP[4,0](CSN)").set_learnable(**bad)
    with pytest.raises(ValueError, match="FixedPoint"):
        dmx.CastTo("FP[1|4|3,7](FN)").set_learnable("per_tensor")
    f = dmx.CastTo("SAME")
    f.set_learnable("per_tensor")
    with pytest.raises(ValueError, match="FixedPoint"):
        f.set_format("FP[1|4|3,7](FN)")
    f.set_format("XP[4,0](CSN)")
