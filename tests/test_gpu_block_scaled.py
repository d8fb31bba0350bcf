"""GPU tests of the two-level block-scaled float cast (csrc/block_scaled_float.hip, ops.block_scaled_float_qdq, CastTo.set_scaling with
a scale_format): the fused kernel against the library's own chain of launches on the GPU and against the CPU checker of
tests/_block_scaled_ref.py (the definition, with the oracle's float cast), bit for bit -- the outputs, the scales and the scale codes.
Every comparison is bits_equal == 0."""
import pytest
import torch
import torch.nn.functional as F

import _block_scaled_ref as R
from _data import bits_equal, make

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=["bf16", "f16", "f32"])
ELEMENTS = ("e2m1", "e4m3", "e5m2")
SCALES = (("e4m3", 448.0), ("e4m3", 480.0), ("e5m2", None))      # (scale format, scale_max; None: the format's largest value)
E2M1, E4M3 = R.SHORTHAND["e2m1"], R.SHORTHAND["e4m3"]
SF = R.SCALE_SHORTHAND["e4m3"]


def routes_of(ops):
    """the front end's private route counter (dmx.ops re-exports a front-end module; ops.front(binding) IS one)"""
    return ops._block_scaled_routes if hasattr(ops, "_block_scaled_routes") else ops._front._block_scaled_routes


def fused(ops, x, fmt, g, sf, smax=None, t="dynamic", **kw):
    """ops.block_scaled_float_qdq(..., fused=True), asserting on the host-side route counter that the kernel ran (and the chain did not)"""
    before = dict(routes_of(ops))
    out = ops.block_scaled_float_qdq(x, fmt, g, sf, smax, t, fused=True, **kw)
    assert routes_of(ops)["fused"] == before["fused"] + 1 and routes_of(ops)["chain"] == before["chain"]
    return out


def chain(ops, x, fmt, g, sf, smax=None, t="dynamic", **kw):
    before = dict(routes_of(ops))
    out = ops.block_scaled_float_qdq(x, fmt, g, sf, smax, t, fused=False, **kw)
    assert routes_of(ops)["chain"] == before["chain"] + 1 and routes_of(ops)["fused"] == before["fused"]
    return out


def same(a, b, what):
    assert len(a) == len(b) == 4
    for i, (u, v) in enumerate(zip(a, b)):
        assert u.shape == v.shape and u.dtype == v.dtype, (what, i)
        assert bits_equal(u.cpu(), v.cpu()) == 0, (what, ("y", "scale", "scale_code_value", "tensor_scale")[i])


def check(oracle, ops, x, xd, name, g, sname, smax, t):
    """kernel == chain == checker: y, scale, scale_code_value and tensor_scale.  t: "dynamic", None, a float or a CPU float32 tensor
    (sent to the device for the op)"""
    td = t.to(xd.device) if isinstance(t, torch.Tensor) else t
    what = (name, g, sname, smax, t, tuple(x.shape), x.dtype)
    got = fused(ops, xd, R.SHORTHAND[name], g, R.SCALE_SHORTHAND[sname], smax, td, return_scale=True)
    assert got[0].dtype == x.dtype and got[0].shape == x.shape and got[1].shape == got[2].shape == (x.numel() // g,)
    assert got[3].shape == (1,) and got[1].dtype == got[2].dtype == got[3].dtype == F32
    same(got, chain(ops, xd, R.SHORTHAND[name], g, R.SCALE_SHORTHAND[sname], smax, td, return_scale=True), what)
    same(got, R.block_scaled_ref(oracle, x, R.FORMATS[name], g, R.SCALE_FORMATS[sname], smax, t), what)
    return got


# ---------------------------------------------------------------------------------------------------- agreement
@pytest.mark.parametrize("name", ELEMENTS)
@DTYPES
def test_kernel_chain_and_checker_agree(dmx, oracle, cuda, dtype, name):
    """g = 16, 32, 128, 256 on [3, 2 g] (a single partly filled wave) and [257, 1024] (several workgroups, the last one partly past the
    end); E4M3 scales capped at 448 and at 480, E5M2 scales; a dynamic, an absent and a static device tensor scale"""
    static = torch.tensor([0.0123], dtype=F32)
    for g in (16, 32, 128, 256):
        assert dmx.ops.block_scaled_float_class(g, dtype) == "group"
        for shape in ((3, 2 * g), (257, 1024)):
            x = make("heavy", shape, seed=g + shape[0], dtype=dtype, block=g)
            xd = x.to(cuda)
            for sname, smax in SCALES:
                for t in ("dynamic", None, static):
                    check(oracle, dmx.ops, x, xd, name, g, sname, smax, t)


@pytest.mark.parametrize("g", [16, 256])
def test_deep_grid(dmx, oracle, cuda, g):
    """[8200, 1024] bf16 = 1,049,600 vectors, more than 2^19: the four-vectors-per-lane build, whose last workgroup is only partly
    filled; up to 524,800 groups: the chain runs in pieces"""
    x = make("heavy", (8200, 1024), seed=3, dtype=BF16)
    check(oracle, dmx.ops, x, x.to(cuda), "e2m1", g, "e4m3", 448.0, "dynamic")


# ---------------------------------------------------------------------------------------------------- special groups
def planted(dtype, specials, big):
    """[64, 256]: rows 0 .. 7 carry the planted groups of 16 (the rest is plain data of magnitude ~1); specials: a NaN and both
    infinities; big: the tensor's maximum is close to the dtype's largest finite value, else 1000"""
    x = make("normal", (64, 256), seed=11, dtype=F32)
    x[0, :16] = 0.0                                            # an all-zero group
    x[1, :16] = -0.0                                           # a group of -0
    x[4, :16] = x[4, :16].sign() * (1e-40 if dtype != F16 else 6e-8)   # float32 denormals (f16: its own, fp32 has none that f16 holds)
    top = (3e38 if dtype != F16 else 65000.0) if big else 1000.0
    x[6, 32:48] = x[6, 32:48] * top / 8
    x[6, 37] = -top                                            # the group that holds the tensor's maximum
    x[5, :16] = torch.where(torch.arange(16) % 2 == 0, 1.0, -1.0) * top * 2.0 ** -25   # 2^-25 below it: the scale code is 0
    if specials:
        x[2, 21] = float("nan")
        x[3, 3] = float("inf")
        x[3, 40] = float("-inf")
    out = x.to(dtype)
    if specials:   # the canonical quiet NaN of the dtype, by its bits
        it, bits = {BF16: (torch.int16, 0x7FC0), F16: (torch.int16, 0x7E00), F32: (torch.int32, 0x7FC00000)}[dtype]
        out.view(it)[2, 21] = bits
    return out


@DTYPES
@pytest.mark.parametrize("name", ["e2m1", "e4m3"])
def test_special_groups(dmx, oracle, cuda, name, dtype):
    fmax, smax = R.FMAX[name], 448.0

    def signed_zeros(y, x, r):
        """the group's outputs are zeros carrying the sign bit of the unscaled cast of its elements"""
        q = oracle.floating_point_cast(x[r, :16].float().contiguous(), *R.FORMATS[name])
        return bool((y[r, :16] == 0).all()) and torch.equal(torch.signbit(y[r, :16]), torch.signbit(q))

    grp = lambda v, r, c: v.reshape(64, 16, -1)[r, c]            # noqa: E731  (row r, group c of a [64 * 16, ...] result)
    # (1) finite data with a moderate maximum: a live tensor scale
    x = planted(dtype, False, False)
    y, s, sq, t = (v.cpu() for v in check(oracle, dmx.ops, x, x.to(cuda), name, 16, "e4m3", smax, "dynamic"))
    assert not torch.isnan(y.float()).any() and float(t) != 1.0
    assert float(grp(sq, 6, 2)) == smax and int((sq == smax).sum()) == 1          # the maximum's group sits on scale_max
    for r in (0, 1, 4, 5):                                                          # zero, -0, denormal, 2^-25 below the maximum
        assert float(grp(sq, r, 0)) == 0.0 and float(grp(s, r, 0)) == 0.0, r
        assert signed_zeros(y, x, r), r
    # (2) the same with the maximum close to the dtype's largest finite value
    x = planted(dtype, False, True)
    y, s, sq, t = (v.cpu() for v in check(oracle, dmx.ops, x, x.to(cuda), name, 16, "e4m3", smax, "dynamic"))
    assert not torch.isnan(y.float()).any() and float(grp(sq, 6, 2)) == smax
    # (3) a NaN and both infinities: the dynamic tensor scale reads back as 1, their groups get sq = scale_max, the output holds no NaN
    for big in (False, True):
        x = planted(dtype, True, big)
        y, s, sq, t = (v.cpu() for v in check(oracle, dmx.ops, x, x.to(cuda), name, 16, "e4m3", smax, "dynamic"))
        assert float(t) == 1.0 and not torch.isnan(y.float()).any()
        assert float(grp(sq, 2, 1)) == smax and float(grp(sq, 3, 0)) == smax and float(grp(sq, 3, 2)) == smax
        top = float(torch.tensor(fmax * smax).to(dtype))                           # (E4M3 elements in f16: 480 * 448 rounds to Inf)
        assert float(y[2, 21]) == top and float(y[3, 3]) == top and float(y[3, 40]) == -top
        assert float(grp(s, 0, 0)) == 0.0 and signed_zeros(y, x, 0) and signed_zeros(y, x, 1)
        check(oracle, dmx.ops, x, x.to(cuda), name, 16, "e4m3", smax, None)
        check(oracle, dmx.ops, x, x.to(cuda), name, 16, "e5m2", None, "dynamic")


# ---------------------------------------------------------------------------------------------------- a static tensor scale
@DTYPES
def test_static_tensor_scale(dmx, oracle, cuda, dtype):
    ops = dmx.ops
    x = make("normal", (40, 512), seed=17, dtype=dtype)
    xd = x.to(cuda)
    other = make("normal", (40, 512), seed=19, dtype=dtype).to(cuda)
    # a sensible one: calibrated on other data of the same kind (step 1 alone), as a device tensor that is never read back
    t = ops.block_scaled_tensor_scale(other, E2M1, SF, 448.0)
    assert t.shape == (1,) and t.dtype == F32 and t.is_cuda
    assert bits_equal(t.cpu(), R.tensor_scale_ref(other.cpu(), R.FORMATS["e2m1"], 448.0)) == 0
    # step 1 alone on tensors the library's own reduction refuses (no whole 16-byte vectors; an unaligned base): the existing reduction,
    # same bits -- and on several workgroups with a NaN (t = 1)
    big = make("heavy", (1031, 1000), seed=23, dtype=dtype)
    for v in (big.reshape(-1)[:1031 * 1000 - 3], big.reshape(-1)[4:4 + 8192], big):
        assert bits_equal(ops.block_scaled_tensor_scale(v.to(cuda) if v.numel() != 8192 else big.to(cuda).reshape(-1)[4:4 + 8192], E2M1, SF, 448.0).cpu(),
                          R.tensor_scale_ref(v, R.FORMATS["e2m1"], 448.0)) == 0, tuple(v.shape)
    big[1030, 999] = float("nan")
    assert float(ops.block_scaled_tensor_scale(big.to(cuda), E2M1, SF, 448.0)) == 1.0
    y, s, sq, tt = check(oracle, ops, x, xd, "e2m1", 16, "e4m3", 448.0, t.cpu())
    assert bits_equal(tt, t) == 0 and 0 < float(sq.min()) and float(sq.max()) <= 448.0
    assert bits_equal(fused(ops, xd, E2M1, 16, SF, 448.0, t), y) == 0                    # without the scales: t goes to the kernel as it is
    assert bits_equal(fused(ops, xd, E2M1, 16, SF, 448.0, float(t)), y) == 0             # the same value as a Python float
    # so small that every scale code is capped at scale_max: the elements saturate at +-fmax * s
    tiny = 2.0 ** -30
    y, s, sq, tt = (v.cpu() for v in check(oracle, ops, x, xd, "e2m1", 16, "e4m3", 448.0, tiny))
    assert bool((sq == 448.0).all()) and bool((s == 448.0 * tiny).all()) and float(tt) == tiny
    assert float(y.float().abs().max()) == 6.0 * 448.0 * tiny
    big = x.float().abs() >= 6.0 * 448.0 * tiny
    assert bool(big.any()) and bool((y.float()[big] == torch.sign(x.float()[big]) * 6.0 * 448.0 * tiny).all())
    # 0, NaN, Inf (and a negative or denormal value) are treated as 1
    want = check(oracle, ops, x, xd, "e2m1", 16, "e4m3", 448.0, None)
    for bad in (0.0, float("nan"), float("inf"), -2.0, 1e-39):
        for form in (bad, torch.tensor([bad], dtype=F32)):
            got = check(oracle, ops, x, xd, "e2m1", 16, "e4m3", 448.0, form)
            same(got, want, bad)
            assert float(got[3]) == 1.0
            td = form.to(cuda) if isinstance(form, torch.Tensor) else form
            assert bits_equal(fused(ops, xd, E2M1, 16, SF, 448.0, td), want[0]) == 0      # (the kernel's own rule: t is not pre-treated)


# ---------------------------------------------------------------------------------------------------- refusals, bindings
def test_refusals_fall_back_to_the_chain(dmx, oracle, cuda):
    ops = dmx.ops
    base = make("heavy", (96, 1056), seed=5, dtype=BF16)
    unaligned = base.to(cuda).reshape(-1)[4:4 + 96 * 1024].reshape(96, 1024)       # 8 bytes past a 16-byte boundary
    assert unaligned.data_ptr() % 16 == 8 and unaligned.is_contiguous()
    x = base[:, :1024].contiguous().to(cuda)
    cases = [("g=8", x, E2M1, 8, {}),
             ("g=48", base[:, :960].contiguous().to(cuda), E2M1, 48, {}),
             ("unaligned", unaligned, E2M1, 16, {}),
             ("stochastic", x, "FP[1|2|1,1](_S)", 16, {"seed": 1234}),
             ("bf16->f32", x, E2M1, 16, {"out_dtype": F32})]
    for name, t, fmt, g, kw in cases:
        with pytest.raises(NotImplementedError):
            ops.block_scaled_float_qdq(t, fmt, g, SF, 448.0, fused=True, **kw)
        routes = dict(routes_of(ops))
        got = ops.block_scaled_float_qdq(t, fmt, g, SF, 448.0, return_scale=True, **kw)        # fused=None: falls back
        assert routes_of(ops)["chain"] == routes["chain"] + 1 and routes_of(ops)["fused"] == routes["fused"], name
        assert got[0].shape == t.shape and got[0].dtype == kw.get("out_dtype", t.dtype), name
        same(got, chain(ops, t, fmt, g, SF, 448.0, return_scale=True, **kw), name)
        if name != "stochastic":
            same(got, R.block_scaled_ref(oracle, t.cpu(), R.FORMATS["e2m1"], g, R.SCALE_FORMATS["e4m3"], 448.0, out_dtype=kw.get("out_dtype")), name)
    # the C entry itself answers DMXQ_ERR_UNSUPPORTED (NotImplementedError through either binding), nothing launched
    e2m1, e4m3 = [1, 2, 1, 0, 2], [3, 4, 7, 0, 2]
    for binding in ("ctypes", "torch"):
        raw = dmx.ops.front(binding)._ops
        with pytest.raises(NotImplementedError):
            raw.block_scaled_float_qdq(x, 8, e2m1, e4m3, 448.0, None, False, False, None)
        with pytest.raises(NotImplementedError):
            raw.block_scaled_float_qdq(x, 16, [1, 2, 1, 0, 3], e4m3, 448.0, None, False, False, None)     # stochastic
        with pytest.raises(NotImplementedError):
            raw.block_scaled_float_qdq(x, 16, e2m1, e4m3, 448.0, None, False, False, F32)
        with pytest.raises(NotImplementedError):
            raw.block_scaled_float_qdq(unaligned, 16, e2m1, e4m3, 448.0, None, False, False, None)


def test_both_bindings_and_meta(dmx, oracle, cuda):
    x = make("outlier", (64, 384), seed=21, dtype=BF16, block=64)
    xd = x.to(cuda)
    want = R.block_scaled_ref(oracle, x, R.FORMATS["e2m1"], 16, R.SCALE_FORMATS["e4m3"], 448.0)
    for binding in ("ctypes", "torch"):
        f = dmx.ops.front(binding)
        same(fused(f, xd, E2M1, 16, SF, 448.0, return_scale=True), want, binding)
        same(chain(f, xd, E2M1, 16, SF, 448.0, return_scale=True), want, binding)
        assert bits_equal(fused(f, xd, E2M1, 16, SF, 448.0).cpu(), want[0]) == 0         # without the scales
        assert bits_equal(f.block_scaled_float_qdq(xd, E2M1, **{k.replace("per_group", "group_size"): v for k, v in f.NVFP4.items()}).cpu(),
                          want[0]) == 0                                                   # ops.NVFP4's keys are the op's arguments
    # the dispatcher op itself, and its meta kernel
    t = want[3].to(cuda)
    y, s, sq = torch.ops.dmxq.block_scaled_float_qdq(xd, 16, [1, 2, 1, 0, 2], [3, 4, 7, 0, 2], 448.0, t, True, True, None)
    same((y, s, sq, t), want, "dispatcher")
    m = torch.ops.dmxq.block_scaled_float_qdq(xd.to("meta"), 16, [1, 2, 1, 0, 2], [3, 4, 7, 0, 2], 448.0, None, True, False, None)
    assert all(v.device.type == "meta" for v in m) and m[0].shape == xd.shape and m[0].dtype == BF16
    assert m[1].shape == (64 * 24,) and m[1].dtype == F32 and m[2].numel() == 0
    e = dmx.ops.block_scaled_float_qdq(xd[:0], E2M1, 16, SF, return_scale=True)
    assert e[0].shape == (0, 384) and e[1].numel() == 0 and e[2].numel() == 0 and float(e[3]) == 1.0


# ---------------------------------------------------------------------------------------------------- CastTo, modules
def test_linear_with_the_nvfp4_setting(dmx, cuda):
    """CastTo.set_scaling(ops.NVFP4) on a Linear's input and weight casts through configure: the forward is the op applied by hand"""
    ops = dmx.ops
    torch.manual_seed(0)
    m = dmx.nn.Linear(256, 384).to(cuda).to(BF16)
    keys = set(m.state_dict())
    m.configure({"input_formats": [E2M1], "weight_format": E2M1, "input_scaling": ops.NVFP4, "weight_scaling": ops.NVFP4})
    assert set(m.state_dict()) == keys
    assert m.input_casts.input_cast.scaling == ops.NVFP4 and m.weight_cast.scaling == ops.NVFP4
    assert "'scale_format': 'FP[1|4|3,7](_N)'" in repr(m.weight_cast) and "'scale_max': 448.0" in repr(m) and "'per_group': 16" in repr(m)
    x = make("heavy", (3, 7, 256), seed=83, dtype=BF16).to(cuda)
    nv = lambda v: ops.block_scaled_float_qdq(v, E2M1, 16, SF, 448.0, "dynamic")   # noqa: E731
    with torch.no_grad():
        y = m(x)
        assert y.dtype == BF16 and bits_equal(y, F.linear(nv(x), nv(m.weight.detach()), m.bias.detach())) == 0
        c = m.input_casts.input_cast
        assert bits_equal(c(x), nv(x)) == 0
        assert bits_equal(c.measure_error(x), ops.error_stats(x, nv(x))) == 0
        assert bits_equal(c(x), ops.dynamic_float_qdq(x, E2M1, "per_group", 16)) != 0      # not the float32-scale cast
        # the step-by-step Hadamard route: rotate (float32) -> the op on the rotated tensor -> rotate back
        c.set_pre_transform({"hadamard": 64})
        r = ops.hadamard(x, 64, out_dtype=F32)
        want = ops.hadamard(ops.block_scaled_float_qdq(r, E2M1, 16, SF, 448.0), 64, out_dtype=BF16)
        assert bits_equal(c(x), want) == 0
        assert bits_equal(c.measure_error(x), ops.error_stats(x, want)) == 0
        c.set_pre_transform({})
        c.set_scaling(None)
        assert bits_equal(c(x), ops.float_qdq(x, 1, 2, 1, False)) == 0
    with pytest.raises(NotImplementedError, match="scaled"):
        with m.optimal_brain_compressing(None):
            pass


def test_backward_is_the_identity(dmx, cuda):
    x = make("normal", (128, 256), seed=67, dtype=F32)
    g = make("heavy", (128, 256), seed=71, dtype=F32)
    for kw in ({}, {"fused": False}, {"tensor_scale": None}):
        xd = x.to(cuda).requires_grad_(True)
        y = dmx.ops.block_scaled_float_qdq(xd, E2M1, 16, SF, 448.0, **kw)
        y.backward(g.to(cuda))
        assert bits_equal(xd.grad, g) == 0
    xd = x.to(cuda).requires_grad_(True)
    y, s, sq, t = dmx.ops.block_scaled_float_qdq(xd, E2M1, 16, SF, return_scale=True)
    assert y.requires_grad and not s.requires_grad and not sq.requires_grad and not t.requires_grad
    c = dmx.CastTo(format=E2M1).to(cuda)
    c.set_scaling(dmx.ops.NVFP4)
    xd = x.to(cuda).requires_grad_(True)
    c(xd).backward(g.to(cuda))
    assert bits_equal(xd.grad, g) == 0


def test_graph_capture(dmx, oracle, cuda):
    """one capture after a warm-up, replayed once: the eager bits on both routes (no allocation-free guarantee is needed for that: the
    capture's allocations are the graph's own; nothing synchronises with the host)"""
    x0 = make("normal", (128, 768), seed=73, dtype=BF16)
    x1 = make("outlier", (128, 768), seed=79, dtype=BF16, block=64)
    buf = x0.to(cuda).clone()
    fused(dmx.ops, buf, E2M1, 16, SF, 448.0)                              # (warm-up outside the capture)
    chain(dmx.ops, buf, E2M1, 16, SF, 448.0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_f = fused(dmx.ops, buf, E2M1, 16, SF, 448.0, return_scale=True)
        out_c = chain(dmx.ops, buf, E2M1, 16, SF, 448.0, return_scale=True)
    buf.copy_(x1.to(cuda))
    graph.replay()
    torch.cuda.synchronize()
    eager = fused(dmx.ops, buf, E2M1, 16, SF, 448.0, return_scale=True)
    same(out_f, eager, "fused")
    same(out_c, eager, "chain")
    same(out_f, R.block_scaled_ref(oracle, x1, R.FORMATS["e2m1"], 16, R.SCALE_FORMATS["e4m3"], 448.0), "checker")
