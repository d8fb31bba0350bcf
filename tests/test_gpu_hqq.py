"""GPU tests of HQQ (csrc/hqq.hip, ops.hqq_qdq, DmxModule.hqq_quantize; DESIGN.md §8 "HQQ"): the kernel (fused=True) and the chain of
torch operations (fused=False) against the CPU checker of tests/_hqq_ref.py (the definition), bit for bit on the output (up to the
sign of a zero, NaN positions equal), the scales, the zero points and the codes; routing, row independence, graph capture and the
module surface."""
import functools

import pytest
import torch

import _hqq_ref as R
from _data import bits_equal, make

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=["bf16", "f16", "f32"])
GROUPS = pytest.mark.parametrize("g", [16, 32, 64, 128, 256])
FORMATS = [(p, sym) for p in (2, 3, 4, 8) for sym in (True, False)]
INT4 = "XP[4,0](CSN)"


def fmt_of(p, sym):
    return f"XP[{p},0](C{'S' if sym else '_'}N)"


@pytest.fixture(autouse=True)
def _stop_the_session_after_a_gpu_fault():
    """a HIP error after a test (an illegal access is sticky) ends the session: nothing more is started on a faulted device"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # pragma: no cover
        pytest.exit(f"GPU fault, stopping the session: {e}", returncode=3)


def routes_of(ops):
    return ops._hqq_routes if hasattr(ops, "_hqq_routes") else ops._front._hqq_routes


def run(ops, x, fmt, g, fused, **kw):
    """ops.hqq_qdq with qparams and codes, asserting on the host-side route counter which route ran"""
    before = dict(routes_of(ops))
    out = ops.hqq_qdq(x, fmt, g, fused=fused, return_qparams=True, return_codes=True, **kw)
    took, other = ("fused", "chain") if fused else ("chain", "fused")
    assert routes_of(ops)[took] == before[took] + 1 and routes_of(ops)[other] == before[other]
    return out


def same_values(a, b):
    """equal up to the sign of a zero, NaN positions equal"""
    a, b = a.detach().cpu().float(), b.detach().cpu().float()
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


def same4(got, want, what):
    (y, sc, zero, codes), (wy, wsc, wzero, wcodes) = got, want
    assert y.dtype == wy.dtype and sc.dtype == F32 and zero.dtype == F32 and codes.dtype == torch.uint8 and codes.shape == y.shape, what
    assert sc.shape == wsc.shape and bits_equal(sc.cpu(), wsc.cpu()) == 0, what
    assert same_values(zero, wzero), what
    assert torch.equal(codes.cpu(), wcodes.cpu()), what
    assert same_values(y, wy), what


def data(kind, shape, seed, dtype, g):
    """the two magnitude classes: "small" near 1e-2 (the shrink zeroes every residual), "large" near 1 .. 10 (it does not)"""
    x = make("normal", shape, seed=seed, dtype=F32)
    return (x * (0.01 if kind == "small" else 4.0)).to(dtype)


@functools.lru_cache(maxsize=None)
def _ref(kind, shape, seed, dtype, g, p, sym, lp, iters, planted, out_dtype=None):
    """(x, the checker's outputs): computed once per case and shared by the kernel and the chain tests"""
    x = data(kind, shape, seed, dtype, g)
    if planted:
        x, _ = R.plant(x, g)
    return x, R.hqq_ref(x, *R.qrange(p, sym), g, lp, iters=iters, out_dtype=out_dtype)


def check_kernel(ops, cuda, kind, shape, seed, dtype, g, p, sym, lp, iters, planted=False):
    x, want = _ref(kind, shape, seed, dtype, g, p, sym, lp, iters, planted)
    got = run(ops, x.to(cuda), fmt_of(p, sym), g, True, lp_norm=lp, iters=iters)
    same4(got, want, ("kernel", kind, shape, dtype, g, p, sym, lp, iters, planted))


def check_chain(ops, cuda, kind, shape, seed, dtype, g, p, sym, lp, iters, planted=False):
    x, want = _ref(kind, shape, seed, dtype, g, p, sym, lp, iters, planted)
    got = run(ops, x.to(cuda), fmt_of(p, sym), g, False, lp_norm=lp, iters=iters)
    same4(got, want, ("chain", kind, shape, dtype, g, p, sym, lp, iters, planted))


# ---------------------------------------------------------------------------------------------------- the kernel against the checker
@GROUPS
@DTYPES
def test_kernel_every_format_norm_and_iteration_count(dmx, cuda, dtype, g):
    """[3, 2 g]: 6 groups, one partly filled wave; every format, both norms, iters 0 / 1 / 20, both magnitude classes"""
    assert dmx.ops.hqq_class(g, dtype) == "group"
    for p, sym in FORMATS:
        for lp in (0.5, 1.0):
            for iters in (0, 1, 20):
                for kind in ("small", "large"):
                    check_kernel(dmx.ops, cuda, kind, (3, 2 * g), g + p, dtype, g, p, sym, lp, iters)


@GROUPS
@DTYPES
def test_kernel_odd_counts_and_special_groups(dmx, cuda, dtype, g):
    """[67, 256] with the special groups planted first, in the middle and last; a rotating choice of format and norm per (dtype, g)"""
    k = [16, 32, 64, 128, 256].index(g) + {BF16: 0, F16: 1, F32: 2}[dtype]
    for j, kind in enumerate(("small", "large")):
        p, sym = FORMATS[(k + 3 * j) % len(FORMATS)]
        lp = (0.5, 1.0)[(k + j) % 2]
        check_kernel(dmx.ops, cuda, kind, (67, 256), 100 + g, dtype, g, p, sym, lp, 20, planted=True)
        check_kernel(dmx.ops, cuda, kind, (67, 256), 100 + g, dtype, g, p, sym, 1.5 - lp, 1, planted=True)


@GROUPS
@DTYPES
def test_kernel_several_workgroups(dmx, cuda, dtype, g):
    """[1031, 512]: an odd count of rows over several workgroups, the last wave partly past the end"""
    k = [16, 32, 64, 128, 256].index(g) + {BF16: 0, F16: 1, F32: 2}[dtype]
    p, sym = FORMATS[(k + 5) % len(FORMATS)]
    check_kernel(dmx.ops, cuda, ("large", "small")[k % 2], (1031, 512), 200 + g, dtype, g, p, sym, (0.5, 1.0)[k % 2], 20, planted=True)


def test_kernel_grid_rounds(dmx, cuda):
    """more waves than the grid holds (4 workgroups per compute unit: 4096 waves on 256 units): [4131, 256] f32 is 4131 waves of
    vectors, [8259, 256] bf16 4130, so the first waves take a second round of the grid-stride loop and the last one is partly filled"""
    check_kernel(dmx.ops, cuda, "large", (4131, 256), 7, F32, 64, 4, False, 0.5, 2, planted=True)
    check_kernel(dmx.ops, cuda, "large", (8259, 256), 9, BF16, 128, 3, True, 1.0, 1, planted=True)


# ---------------------------------------------------------------------------------------------------- the chain against the checker
@DTYPES
@pytest.mark.parametrize("lp", [0.5, 1.0])
def test_chain_matches_the_checker(dmx, cuda, dtype, lp):
    for g, shape in ((64, (67, 256)), (16, (3, 32)), (256, (67, 256))):
        for kind in ("small", "large"):
            check_chain(dmx.ops, cuda, kind, shape, 100 + g if shape[0] == 67 else g + 4, dtype, g, 4, True, lp, 20, planted=shape[0] == 67)
    check_chain(dmx.ops, cuda, "large", (1031, 512), 264, dtype, 64, 2, False, lp, 1, planted=True)


@pytest.mark.parametrize("lp", [0.5, 1.0])
def test_chain_other_group_sizes_views_and_dtypes(dmx, cuda, lp):
    ops = dmx.ops
    # g = 48: no power of two (the tree carries an odd level's last value up); the kernel refuses it
    for dtype in (BF16, F32):
        x, want = _ref("large", (5, 192), 31, dtype, 48, 3, False, lp, 20, True)
        same4(run(ops, x.to(cuda), fmt_of(3, False), 48, False, lp_norm=lp, iters=20), want, ("g48", dtype, lp))
        same4(run(ops, x.to(cuda), fmt_of(3, False), 48, None, lp_norm=lp, iters=20), want, ("g48 default route", dtype, lp))
    # an unaligned view (2 bytes past a 16-byte boundary): the default route is the chain
    x, want = _ref("large", (9, 128), 33, BF16, 64, 4, True, lp, 5, False)
    big = torch.zeros(x.numel() + 8, dtype=BF16, device=cuda)
    view = big[1:1 + x.numel()].reshape(x.shape)
    view.copy_(x.to(cuda))
    assert view.data_ptr() % 16 == 2 and view.is_contiguous()
    same4(run(ops, view, INT4, 64, None, lp_norm=lp, iters=5), want, ("unaligned", lp))
    # out_dtype != x.dtype: one rounding of the float32 result to the other dtype
    for dtype, out in ((BF16, F32), (F32, BF16), (F16, BF16)):
        x, want = _ref("large", (9, 128), 35, dtype, 32, 8, False, lp, 5, False, out)
        same4(run(ops, x.to(cuda), fmt_of(8, False), 32, None, lp_norm=lp, iters=5, out_dtype=out), want, ("out_dtype", dtype, out, lp))


def test_chain_general_norm_is_checked_without_bits(dmx, cuda):
    """lp_norm = 0.7 goes through torch.pow, which is not pinned to the bit: codes in range, y reconstructs from (codes, scale, zero)
    bit for bit, and no group's L1 error (of the float32 values the codes stand for) exceeds that of the iters=0 call"""
    ops = dmx.ops
    for dtype, g, (p, sym) in ((BF16, 64, (4, True)), (F32, 48, (3, False)), (F16, 128, (2, False))):
        qmin, qmax = R.qrange(p, sym)
        x = data("large", (33, 384), 41, dtype, g)
        y, sc, zero, codes = run(ops, x.to(cuda), fmt_of(p, sym), g, False, lp_norm=0.7, iters=20)
        _, sc0, zero0, codes0 = run(ops, x.to(cuda), fmt_of(p, sym), g, False, lp_norm=0.7, iters=0)
        assert int(codes.max()) <= qmax - qmin

        def rebuilt(c, z, s):
            q = c.cpu().reshape(-1, g).float() + torch.full((1, 1), float(qmin))
            return (q - z.cpu()[:, None]) * s.cpu()[:, None]

        r, r0 = rebuilt(codes, zero, sc), rebuilt(codes0, zero0, sc0)
        assert bits_equal(r.to(dtype).reshape(x.shape), y.cpu()) == 0
        # the definition's errors are those of the float32 values, before the one rounding to the output dtype
        W = x.float().reshape(-1, g)
        assert bool((R.tree_sum((W - r).abs()) <= R.tree_sum((W - r0).abs())).all())
        with pytest.raises(NotImplementedError):
            ops.hqq_qdq(x.to(cuda), fmt_of(p, sym), g, lp_norm=0.7, fused=True)


# ---------------------------------------------------------------------------------------------------- routing
def test_routing(dmx, cuda):
    ops = dmx.ops
    x = data("large", (8, 1536), 51, BF16, 64).to(cuda)
    before = dict(routes_of(ops))
    refused = [dict(group_size=48), dict(group_size=8), dict(group_size=512), dict(lp_norm=0.7), dict(lp_norm=0.25), dict(out_dtype=F32)]
    for kw in refused:
        with pytest.raises(NotImplementedError):
            ops.hqq_qdq(x, INT4, **{"group_size": 64, **kw}, fused=True)
    view = torch.zeros(x.numel() + 8, dtype=BF16, device=cuda)[1:1 + x.numel()].reshape(x.shape)
    with pytest.raises(NotImplementedError):
        ops.hqq_qdq(view, INT4, 64, fused=True)
    assert routes_of(ops) == before                                           # nothing ran on either route
    y = ops.hqq_qdq(x, INT4, 64)                                              # fused=None where the kernel applies: the kernel
    assert routes_of(ops)["fused"] == before["fused"] + 1 and routes_of(ops)["chain"] == before["chain"]
    assert ops.hqq_class(64, BF16) not in ops.HQQ_CHAIN_BY_DEFAULT
    assert isinstance(y, torch.Tensor) and y.dtype == BF16 and y.shape == x.shape
    y2, sc, zero = ops.hqq_qdq(x, INT4, 64, return_qparams=True)
    assert bits_equal(y2, y) == 0 and sc.shape == zero.shape == (x.numel() // 64,)
    y3, codes = ops.hqq_qdq(x, INT4, 64, return_codes=True)
    assert bits_equal(y3, y) == 0 and codes.dtype == torch.uint8 and codes.shape == x.shape
    e = ops.hqq_qdq(x[:0], INT4, 64, return_qparams=True, return_codes=True)  # an empty tensor: nothing launched
    assert [t.numel() for t in e] == [0, 0, 0, 0]
    xg = x.clone().requires_grad_(True)                                       # autograd: a straight-through estimator
    gout = data("large", (8, 1536), 53, BF16, 64).to(cuda)
    ops.hqq_qdq(xg, INT4, 64).backward(gout)
    assert bits_equal(xg.grad, gout) == 0


@pytest.mark.parametrize("fused", [True, False])
def test_rows_are_independent(dmx, cuda, fused):
    """hqq_qdq(x[:k]) is the first k rows of hqq_qdq(x): what sharding a weight by rows needs"""
    ops = dmx.ops
    x = data("large", (37, 384), 61, BF16, 128).to(cuda)
    y, sc, zero, codes = run(ops, x, INT4, 128, fused)
    for k in (1, 5, 36):
        yk, sck, zk, ck = run(ops, x[:k], INT4, 128, fused)
        G = k * 3
        assert bits_equal(yk, y[:k]) == 0 and bits_equal(sck, sc[:G]) == 0 and bits_equal(zk, zero[:G]) == 0 and torch.equal(ck, codes[:k])


def _capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()                                                                  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    return graph, out


def test_graph_capture(dmx, cuda):
    """one capture of a call (a single stream, no parallel branches), replayed on new data, gives the eager bits: no host round trip"""
    ops = dmx.ops
    x0, want0 = _ref("large", (67, 256), 164, BF16, 64, 4, True, 0.5, 20, True)
    x1, want1 = _ref("small", (67, 256), 164, BF16, 64, 4, True, 0.5, 20, True)
    buf = x0.to(cuda).clone()
    graph, out = _capture(lambda: run(ops, buf, INT4, 64, True))
    for x, want in ((x1, want1), (x0, want0)):
        buf.copy_(x.to(cuda))
        graph.replay()
        torch.cuda.synchronize()
        same4(out, want, "replay")
        same4(out, run(ops, x.to(cuda), INT4, 64, True), "replay against eager")


# ---------------------------------------------------------------------------------------------------- modules
def _module(dmx, cuda, kind, dtype, seed=71, **config):
    if kind == "linear":
        m = dmx.nn.Linear(128, 64, bias=True)
    else:
        m = dmx.nn.Conv2d(8, 6, 4, bias=False)   # the [6, 128] view of its weight
    m = m.to(cuda).to(dtype)
    with torch.no_grad():
        m.weight.copy_((make("normal", tuple(m.weight.shape), seed=seed, dtype=F32) * 0.5).to(dtype).to(cuda))
    m.configure(dict({"weight_format": INT4}, **config))
    return m


def _input(kind, dtype, cuda):
    shape = (5, 128) if kind == "linear" else (2, 8, 9, 9)
    return make("normal", shape, seed=73, dtype=dtype).to(cuda)


@pytest.mark.parametrize("kind,dtype", [("linear", BF16), ("linear", F32), ("conv", BF16)])
def test_module_hqq_quantize(dmx, cuda, kind, dtype):
    ops = dmx.ops
    m = _module(dmx, cuda, kind, dtype)
    keys = list(m.state_dict().keys())
    w0 = m.weight.detach().clone()
    rows = w0.shape[0]
    want, sc, zero = ops.hqq_qdq(w0.reshape(rows, -1), INT4, 64, return_qparams=True)
    assert m.weight_cast._flag("fake_quant_enabled")
    m.hqq_quantize()
    assert bits_equal(m.weight.detach(), want.reshape(w0.shape)) == 0 and bits_equal(m.weight.detach(), w0) > 0
    qp = m.hqq_qparams
    assert set(qp) == {"scale", "zero", "group_size"} and qp["group_size"] == 64
    assert qp["scale"].shape == qp["zero"].shape == (rows, 2) and qp["scale"].dtype == qp["zero"].dtype == F32
    assert bits_equal(qp["scale"].reshape(-1), sc) == 0 and bits_equal(qp["zero"].reshape(-1), zero) == 0
    assert not m.weight_cast._flag("fake_quant_enabled")
    assert list(m.state_dict().keys()) == keys
    # the forward: the same module built with that weight and the cast disabled
    other = _module(dmx, cuda, kind, dtype, seed=79)
    other.load_state_dict(m.state_dict())
    other.weight_cast.disable_fake_quant()
    x = _input(kind, dtype, cuda)
    with torch.no_grad():
        assert bits_equal(m(x), other(x)) == 0


def test_module_group_size_and_hyperparams(dmx, cuda):
    ops = dmx.ops
    H = dmx.DmxHQQHyperparams
    # group_size None takes the weight cast's own per-group size
    m = _module(dmx, cuda, "linear", BF16, weight_dynamic={"per_group": 32})
    w0 = m.weight.detach().clone()
    m.hqq_quantize(H(lp_norm=1.0, iters=5))
    assert m.hqq_qparams["group_size"] == 32 and m.hqq_qparams["scale"].shape == (64, 4)
    assert bits_equal(m.weight.detach(), ops.hqq_qdq(w0, INT4, 32, lp_norm=1.0, iters=5)) == 0
    # an explicit size wins; 128 is the whole row
    m = _module(dmx, cuda, "linear", BF16, weight_dynamic={"per_group": 32})
    m.hqq_quantize(H(group_size=128))
    assert m.hqq_qparams["group_size"] == 128 and m.hqq_qparams["zero"].shape == (64, 1)
    # a module that is neither Linear nor Conv2d: nothing happens
    r = dmx.nn.ReLU()
    r.hqq_quantize()
    assert not hasattr(r, "hqq_qparams")
    with pytest.raises(TypeError):
        m.hqq_quantize(dict(group_size=64))


def test_module_refusals(dmx, cuda):
    H = dmx.DmxHQQHyperparams

    def untouched(m, w0):
        assert bits_equal(m.weight.detach(), w0) == 0 and not hasattr(m, "hqq_qparams") and m.weight_cast._flag("fake_quant_enabled")

    for config, exc in ((dict(weight_codebook=dmx.ops.NF4), NotImplementedError),
                        (dict(weight_learnable="per_token"), NotImplementedError),
                        (dict(weight_format="FP[1|4|3,7](_N)", weight_scaling="per_token"), NotImplementedError),
                        (dict(pre_weight_transform={"hadamard": 64}), dmx.DmxqError),
                        (dict(weight_storage_format="BFP[8|8]{64}(SN)"), dmx.DmxqError),
                        (dict(weight_format="BFP[8|8]{64}(SN)"), dmx.DmxqError),
                        (dict(weight_format="XP[4,0](CSS)"), dmx.DmxqError),
                        (dict(weight_format="XP[4,1](CSN)"), dmx.DmxqError)):
        m = _module(dmx, cuda, "linear", BF16, **config)
        w0 = m.weight.detach().clone()
        with pytest.raises(exc):
            m.hqq_quantize()
        untouched(m, w0)
    # an observer that is calibrating
    m = _module(dmx, cuda, "linear", BF16)
    w0 = m.weight.detach().clone()
    m.weight_cast.enable_calibration(True)
    with pytest.raises(dmx.DmxqError, match="calibrating"):
        m.hqq_quantize()
    m.weight_cast.enable_calibration(False)
    # a group size that does not divide the input width
    m = _module(dmx, cuda, "linear", BF16)
    with pytest.raises(ValueError, match="divide"):
        m.hqq_quantize(H(group_size=48))
    untouched(m, w0)


def test_recipe_gives_the_methods_weight(dmx, cuda):
    H = dmx.DmxHQQHyperparams
    a, b = _module(dmx, cuda, "linear", BF16), _module(dmx, cuda, "linear", BF16)
    c = _module(dmx, cuda, "conv", BF16)
    hp = H(group_size=64, iters=7)
    a.hqq_quantize(hp)
    model = torch.nn.Sequential(b)
    with dmx.DmxHQQRecipe(lambda mod: {b: hp, c: H()}).applied_to(model):
        assert not hasattr(b, "hqq_qparams")                                  # the work happens on leaving the context
    assert bits_equal(b.weight.detach(), a.weight.detach()) == 0
    assert bits_equal(b.hqq_qparams["zero"], a.hqq_qparams["zero"]) == 0 and not b.weight_cast._flag("fake_quant_enabled")
    assert c.hqq_qparams["scale"].shape == (6, 2)
    with b.hqq_quantizing(hp) as same:
        assert same is b
