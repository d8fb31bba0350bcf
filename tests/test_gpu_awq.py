"""-m gpu: AWQ -- ops.channel_sumabs, ops.awq_scaled_error (kernel = chain = CPU definition, bit for bit),
ops.awq_candidate_scales, ops.awq_search, DmxModule.awq_scaling and DmxAWQRecipe -- against tests/_awq_ref.py.

channel_sumabs is compared EXACTLY: the inputs are values with 2^-4 <= |x| < 2^4 that are multiples of 2^-11 (bf16) or 2^-14 (f16), so a
float64 sum of a few thousand magnitudes is exact in any order.  The loss tolerance is the inner-product bound of a float32 GEMM
(_awq_ref.loss_bound), the 0.75 improvement factor a condition on the data that tests/test_awq_host.py asserts on the reference."""
import math

import pytest
import torch

import _awq_ref as A
import _wanda_ref as W
from _data import bits_equal

pytestmark = pytest.mark.gpu
F = torch.nn.functional
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = {"bf16": BF16, "f16": F16, "f32": F32}
INT4, INT8, INT8_AFFINE_RANGE, INT4_AFFINE_RANGE = "XP[4,0](CSN)", "XP[8,0](CSN)", "XP[8,0](C_N)", "XP[4,0](C_N)"
# (format, precision, the format's symmetric flag, symmetric_qscheme)
FORMAT_CASES = [(INT4, 4, True, False), (INT8, 8, True, True), (INT8_AFFINE_RANGE, 8, False, False), (INT4_AFFINE_RANGE, 4, False, True)]


def _routes(dmx):
    return dmx.ops._front._awq_routes


def _same_bits(got, want):
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    return bits_equal(got, want) == 0


# ------------------------------------------------------------------------------------------------ channel_sumabs
@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("shape", [(4096, 64), (33, 24), (257, 776)], ids=lambda s: "x".join(map(str, s)))
def test_channel_sumabs_is_exact_and_does_not_depend_on_order_or_batching(dmx, cuda, shape, dtype):
    x = W.exact_values(shape, DTYPES[dtype], 3 + sum(shape))
    want = A.sumabs_ref([x])
    dx = x.to(cuda)
    got = dmx.ops.channel_sumabs(dx)
    assert got.dtype == torch.float64 and got.shape == (shape[-1],) and got.device.type == "cuda"
    assert torch.equal(got.cpu(), want), float((got.cpu() - want).abs().max())
    assert torch.equal(dmx.ops.channel_sumabs(dx.flip(0).contiguous()).cpu(), want)
    out = torch.zeros(shape[-1], dtype=torch.float64, device=cuda)
    cut = shape[0] // 3 + 1
    for part in (dx[:cut], dx[cut:]):
        assert dmx.ops.channel_sumabs(part, out=out) is out
    assert torch.equal(out.cpu(), want)
    # it is not the sum of squares
    assert not torch.equal(dmx.ops.channel_sumsq(dx).cpu(), want)


def test_channel_sumabs_scalar_lane_form_of_an_unaligned_view(dmx, cuda):
    x = W.exact_values((37, 64), BF16, 5)
    buf = torch.zeros(37 * 64 + 1, dtype=BF16, device=cuda)
    view = buf[1:].view(37, 64)
    view.copy_(x)
    assert view.data_ptr() % 16 != 0
    assert torch.equal(dmx.ops.channel_sumabs(view).cpu(), A.sumabs_ref([x]))


# ------------------------------------------------------------------------------------------------ awq_scaled_error
def _weight(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.05 * torch.randn(shape, generator=g)).to(dtype)


def _scale(L, seed):
    """distinct values per column, spanning 1e-4 .. 1e4"""
    g = torch.Generator().manual_seed(seed)
    s = torch.exp(torch.linspace(math.log(1e-4), math.log(1e4), L, dtype=torch.float64)).float()
    assert s.unique().numel() == L
    return s[torch.randperm(L, generator=g)].contiguous()


def _both_routes(dmx, w, s, fmt, group, qsym):
    """-> (d, wq) of the kernel, after checking the chain's against them bit for bit and the route counter"""
    routes = _routes(dmx)
    out = {}
    for fused in (True, False):
        before = dict(routes)
        out[fused] = dmx.ops.awq_scaled_error(w, s, fmt, group, symmetric_qscheme=qsym, return_wq=True, fused=fused)
        took = "fused" if fused else "chain"
        assert routes[took] == before[took] + 1 and sum(routes.values()) == sum(before.values()) + 1, (fused, before, routes)
    (d, wq), (dc, wqc) = out[True], out[False]
    assert d.dtype == F32 and wq.dtype == w.dtype and d.shape == w.shape == wq.shape
    assert _same_bits(wq, wqc), ("wq: kernel against chain", int(bits_equal(wq, wqc)))
    assert _same_bits(d, dc), ("d: kernel against chain", int(bits_equal(d, dc)))
    # d alone (wq_out = NULL) is the same d
    assert _same_bits(dmx.ops.awq_scaled_error(w, s, fmt, group, symmetric_qscheme=qsym, fused=True), d)
    return d, wq


SHAPES = [(3, 128), (5, 768), (1, 256), (257, 384)]


@pytest.mark.parametrize("group", [16, 32, 64, 128, 256])
@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
def test_kernel_chain_and_reference_agree(dmx, cuda, oracle, dtype, group):
    dt = DTYPES[dtype]
    ran = 0
    for shape in SHAPES:
        if shape[1] % group:
            continue
        assert dmx.ops.awq_class(dt, shape[1], group)
        w, s = _weight(shape, dt, 11 + group + shape[0]), _scale(shape[1], group)
        dw, ds = w.to(cuda), s.to(cuda)
        for fmt, prec, fsym, qsym in FORMAT_CASES:
            d, wq = _both_routes(dmx, dw, ds, fmt, group, qsym)
            rd, rwq = A.error_ref(oracle, w, s, prec, fsym, group, qsym)
            assert torch.isfinite(rd).all()
            assert _same_bits(wq, rwq), ("wq against the reference", shape, fmt, qsym, int(bits_equal(wq.cpu(), rwq)))
            assert _same_bits(d, rd), ("d against the reference", shape, fmt, qsym, int(bits_equal(d.cpu(), rd)))
            ran += 1
    assert ran >= 8


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
def test_planted_groups_zero_denormal_and_overflow(dmx, cuda, oracle, dtype):
    dt = DTYPES[dtype]
    group, shape = 32, (6, 128)
    w, s = _weight(shape, dt, 3), _scale(128, 4)
    w[1, 32:64] = 0.0                                   # an all-zero group: the eps scale, the division route
    w[2, 0:32] = -0.0
    tiny = {BF16: 1e-40, F32: 1e-40, F16: 3e-7}[dt]     # a group of denormals of the dtype
    w[3, 64:96] = torch.tensor(tiny).to(dt) * torch.arange(1, 33).to(dt)
    assert bool((w[3, 64:96].float().abs() < {F16: 2.0 ** -14}.get(dt, 2.0 ** -126)).all()) and bool((w[3, 64:96] != 0).all())
    s[64:96] = s[64:96].clamp(max=1.0)                  # (they stay denormal after the scaling)
    for fmt, prec, fsym, qsym in FORMAT_CASES[:3]:
        d, wq = _both_routes(dmx, w.to(cuda), s.to(cuda), fmt, group, qsym)
        rd, rwq = A.error_ref(oracle, w, s, prec, fsym, group, qsym)
        assert _same_bits(wq, rwq) and _same_bits(d, rd), (fmt, qsym)
        assert bool((wq[1, 32:64] == 0).all()) and bool((d[1, 32:64] == 0).all())
    if dt == F16:   # w s overflows to Inf in float16: the group's scale is Inf; kernel and chain agree on every bit, NaN positions included
        w[4, 5], s[5] = 100.0, 1e4
        assert torch.isinf((w[4, 5].float() * s[5]).to(F16))
        d, wq = _both_routes(dmx, w.to(cuda), s.to(cuda), INT4, group, False)
        assert not torch.isfinite(d[4, :32]).all() and torch.isfinite(d[4, 32:]).all() and torch.isfinite(d[:4]).all()


def test_rejected_classes_run_the_chain(dmx, cuda, oracle):
    routes = _routes(dmx)

    def chain_by_default(w, s, fmt, group):
        with pytest.raises(NotImplementedError):
            dmx.ops.awq_scaled_error(w, s, fmt, group, fused=True)
        before = dict(routes)
        got = dmx.ops.awq_scaled_error(w, s, fmt, group, return_wq=True)
        assert routes["chain"] == before["chain"] + 1 and routes["fused"] == before["fused"]
        return got

    # g = 48: no power of two
    w, s = _weight((4, 192), BF16, 1), _scale(192, 2)
    assert not dmx.ops.awq_class(BF16, 192, 48)
    d, wq = chain_by_default(w.to(cuda), s.to(cuda), INT4, 48)
    rd, rwq = A.error_ref(oracle, w, s, 4, True, 48, False)
    assert _same_bits(d, rd) and _same_bits(wq, rwq)
    want = dmx.ops.awq_scaled_error(w.to(cuda), s.to(cuda), INT4, 48, return_wq=True, fused=False)
    assert _same_bits(d, want[0]) and _same_bits(wq, want[1])
    # a misaligned view of a weight the kernel would take
    w, s = _weight((3, 128), BF16, 5), _scale(128, 6)
    buf = torch.zeros(3 * 128 + 1, dtype=BF16, device=cuda)
    view = buf[1:].view(3, 128)
    view.copy_(w)
    assert dmx.ops.awq_class(BF16, 128, 32) and view.data_ptr() % 16 != 0
    d, wq = chain_by_default(view, s.to(cuda), INT4, 32)
    rd, rwq = A.error_ref(oracle, w, s, 4, True, 32, False)
    assert _same_bits(d, rd) and _same_bits(wq, rwq)
    # stochastic rounding: the chain's (with its own draws); every value lies between the round-down and the round-up cast
    dw, ds = w.to(cuda), s.to(cuda)
    d, wq = chain_by_default(dw, ds, "XP[4,0](CSS)", 32)
    lo = dmx.ops.awq_scaled_error(dw, ds, "XP[4,0](CSD)", 32, return_wq=True)[1]
    hi = dmx.ops.awq_scaled_error(dw, ds, "XP[4,0](CSU)", 32, return_wq=True)[1]
    assert bool(((wq >= lo) & (wq <= hi)).all())


def test_awq_scaled_error_above_two_to_the_31_elements(dmx, cuda, oracle):
    import _large_cases as LC
    rows, L = 524289, 4096
    assert rows * L > 2 ** 31
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    need = rows * L * (2 + 2 + 4) + (1 << 30)
    if free < need:
        pytest.skip(f"needs {need / 2 ** 30:.1f} GiB of device memory, {free / 2 ** 30:.1f} GiB free")
    w = LC.device_input("weight", (rows, L), BF16, 18, cuda)
    s = _scale(L, 19)
    before = dict(_routes(dmx))
    d, wq = dmx.ops.awq_scaled_error(w, s.to(cuda), INT4, 128, return_wq=True, fused=True)
    assert _routes(dmx)["fused"] == before["fused"] + 1
    picked = list(range(rows - 8, rows)) + [0, 1, 65537, 262143, 262144, 400001, 524279, 524280]   # (row 524288 begins at element 2^31)
    idx = torch.tensor(picked, device=cuda)
    wr, dr, wqr = w[idx].cpu(), d[idx].cpu(), wq[idx].cpu()
    del w, d, wq
    torch.cuda.empty_cache()
    rd, rwq = A.error_ref(oracle, wr, s, 4, True, 128, False)
    assert _same_bits(wqr, rwq) and _same_bits(dr, rd)


# ------------------------------------------------------------------------------------------------ candidate scales
def test_candidate_scales_within_four_ulps_of_the_float64_formula(dmx, cuda):
    """4 float32 ulps: the project's SmoothQuant allowance for powf on different libms.  x_mean lies in [0.5, 2] (|ln x| <= 0.7: the
    float32 rounding of the exponent k / n_grid moves x ** r by at most 0.7 r 2^-24 relative) with one dead channel, which the clamp
    holds at 1e-4 in every row but the first."""
    g = torch.Generator().manual_seed(0)
    x_mean = torch.rand(768, generator=g) * 1.5 + 0.5
    x_mean[17] = 0.0
    got = dmx.ops.awq_candidate_scales(x_mean.to(cuda), 20)
    assert got.dtype == F32 and got.shape == (20, 768) and got.device.type == "cuda" and got.is_contiguous()
    assert torch.equal(got[0].cpu(), torch.ones(768))
    want = A.candidate_scales_f64(x_mean, 20)
    ulp = torch.exp2(torch.floor(torch.log2(want.abs())) - 23)
    off = ((got.cpu().double() - want).abs() / ulp).max().item()
    print(f"candidate scales: largest distance from the float64 formula {off:.3f} ulps")
    assert off <= 4.0
    # through a scale cast
    cast = dmx.CastTo(format="FP[1|5|10,15](FN)").to(cuda)
    through = dmx.ops.awq_candidate_scales(x_mean.to(cuda), 4, scale_cast=cast)
    assert _same_bits(through, torch.stack([cast(r) for r in dmx.ops.awq_candidate_scales(x_mean.to(cuda), 4)]))


# ------------------------------------------------------------------------------------------------ the search
def test_losses_within_the_gemm_bound_and_the_choice_within_it_of_the_minimum(dmx, cuda):
    w, _, x = A.dataset(0, BF16)
    dw, dx = w.to(cuda), x.to(cuda)
    gram = (dx.float().t() @ dx.float()) / x.shape[0]
    scales = dmx.ops.awq_candidate_scales(A.x_mean_ref([x]).to(cuda), 20)
    seen = []

    def fn(k, s):
        seen.append(dmx.ops.awq_scaled_error(dw, s, INT4, A.GROUP))
        return seen[-1]

    losses, best = dmx.ops.awq_search(dw, gram, scales, fn)
    assert losses.dtype == torch.float64 and losses.shape == (20,) and losses.device.type == "cuda"
    assert best.dtype == torch.int64 and best.dim() == 0 and best.device.type == "cuda"
    assert len(seen) == 20
    want = [A.loss64(d, gram) for d in seen]
    bound = [A.loss_bound(d, gram) for d in seen]
    for k in range(20):
        print(f"candidate {k}: loss {float(losses[k]):.6e}, float64 {want[k]:.6e}, difference {abs(float(losses[k]) - want[k]):.2e}, bound {bound[k]:.2e}")
        assert abs(float(losses[k]) - want[k]) <= bound[k], k
    b, a = int(best), min(range(20), key=lambda k: want[k])
    assert want[b] <= want[a] + max(bound[a], bound[b])
    # no finite loss: index 0; a NaN or Inf loss is never chosen
    nan_fn = lambda k, s: torch.full(w.shape, float("nan"), device=cuda)
    losses, best = dmx.ops.awq_search(dw, gram, scales[:3], nan_fn)
    assert torch.isnan(losses).all() and int(best) == 0
    some = lambda k, s: torch.full(w.shape, float("inf") if k != 2 else 1.0, device=cuda)
    assert int(dmx.ops.awq_search(dw, gram, scales[:4], some)[1]) == 2


# ------------------------------------------------------------------------------------------------ module
def _linear(dmx, cuda, dt, w, b, config=None):
    m = dmx.nn.Linear(w.shape[1], w.shape[0]).to(cuda, dt).eval()
    with torch.no_grad():
        m.weight.copy_(w)
        m.bias.copy_(b)
    m.configure(config or {"weight_format": INT4, "weight_dynamic": {"per_group": A.GROUP}})
    return m


def _calibrate(dmx, m, batches, hp=None):
    with torch.no_grad(), m.awq_scaling(hp or dmx.DmxAWQHyperparams()) as ctx:
        assert ctx is m and isinstance(m.awq, dmx.AWQCalibrator)
        for t in batches:
            m(t)
    assert m.awq is None


def _effective_error(m, x, w):
    """the float64 output error of the module's weight as its GEMM sees it, brought back through the scale"""
    with torch.no_grad():
        wq = m.weight_hypernet(m.weight).double().cpu()
    sq = m.smoothquant
    if sq._flag("enabled"):
        wq = wq / sq.scale.double().cpu()
    return A.output_error64(x, w, wq)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("seed", A.SEEDS)
def test_awq_scaling_on_a_linear(dmx, cuda, seed, dtype):
    dt = DTYPES[dtype]
    w, b, x = A.dataset(seed, dt)
    m = _linear(dmx, cuda, dt, w, b)
    dx = x.to(cuda)
    batches = [dx[:40], dx[40:].reshape(2, 28, A.IN)]
    before = dict(_routes(dmx))
    _calibrate(dmx, m, batches)
    assert _routes(dmx)["fused"] == before["fused"] + 20 and _routes(dmx)["chain"] == before["chain"]
    sq = m.smoothquant
    assert sq._flag("enabled") and not sq._flag("fused_to_weight") and not sq._flag("dynamic")
    assert m.awq_n_tokens == A.TOKENS
    assert _same_bits(m.awq_x_mean, A.x_mean_ref([x]))
    assert m.awq_losses.dtype == torch.float64 and m.awq_losses.shape == (20,) and m.awq_losses.device.type == "cuda"
    assert m.awq_best.dtype == torch.int64 and m.awq_best.dim() == 0 and m.awq_best.device.type == "cuda"
    scales = dmx.ops.awq_candidate_scales(m.awq_x_mean, 20, sq.scale_cast)
    assert _same_bits(sq.scale, scales[int(m.awq_best)])
    assert torch.equal(m.weight.detach().cpu(), w) and sq._scalar("migration_strength") == 0.5
    assert not any("awq" in k for k in m.state_dict())
    # the forward is the forward of a module whose SmoothQuant scale was set to that vector by hand
    twin = _linear(dmx, cuda, dt, w, b)
    twin.smoothquant.scale = scales[int(m.awq_best)].clone()
    twin.smoothquant.enable(True)
    probe = torch.randn(7, A.IN, generator=torch.Generator().manual_seed(50 + seed)).to(dt).to(cuda)
    with torch.no_grad():
        out = m(probe)
        assert _same_bits(out, twin(probe))
    # a later forward observed nothing
    assert m.awq is None and m.awq_n_tokens == A.TOKENS
    # the improvement: at most 0.75 of plain round-to-nearest's output error
    rtn = _linear(dmx, cuda, dt, w, b)
    e_awq, e_rtn = _effective_error(m, x, w), _effective_error(rtn, x, w)
    print(f"seed {seed} {dtype}: best {int(m.awq_best)}, output error {e_awq:.6e} against round-to-nearest {e_rtn:.6e}: ratio {e_awq / e_rtn:.4f}")
    assert e_awq <= 0.75 * e_rtn
    # a state_dict round trip restores the scale
    fresh = _linear(dmx, cuda, dt, w, b)
    fresh.smoothquant.scale = torch.ones(A.IN, device=cuda)
    fresh.load_state_dict(m.state_dict())
    assert fresh.smoothquant._flag("enabled") and _same_bits(fresh.smoothquant.scale, sq.scale)
    with torch.no_grad():
        assert _same_bits(fresh(probe), out)


def test_reset_false_continues_the_sums(dmx, cuda):
    w, b, x = A.dataset(1, BF16)
    dx = x.to(cuda)
    m = _linear(dmx, cuda, BF16, w, b)
    _calibrate(dmx, m, [dx[:40]])
    assert m.awq_n_tokens == 40
    m.smoothquant.disable()
    _calibrate(dmx, m, [dx[40:]], dmx.DmxAWQHyperparams(reset=False))
    assert m.awq_n_tokens == A.TOKENS
    assert torch.equal(m.awq_sumabs.cpu(), A.sumabs_ref([x]))
    assert _same_bits(m.awq_x_mean, A.x_mean_ref([x]))
    # the running mean of x^T x over both contexts is the mean over all tokens, up to float32 rounding
    g64 = A.gram64([x])
    assert float((m.awq_gram.double().cpu() - g64).abs().max()) <= 1e-5 * float(g64.abs().max())
    whole = _linear(dmx, cuda, BF16, w, b)
    _calibrate(dmx, whole, [dx])
    assert int(whole.awq_best) == int(m.awq_best)   # (the runner-up lies 0.4 % above the best: tests/test_awq_host.py)
    m.smoothquant.disable()
    _calibrate(dmx, m, [dx[40:]])   # reset=True: the second part alone
    assert m.awq_n_tokens == A.TOKENS - 40 and torch.equal(m.awq_sumabs.cpu(), A.sumabs_ref([x[40:]]))


def test_fuse_to_weight_folds_the_scale_in(dmx, cuda):
    w, b, x = A.dataset(2, BF16)
    dx = x.to(cuda)
    m = _linear(dmx, cuda, BF16, w, b)
    _calibrate(dmx, m, [dx])
    fused = _linear(dmx, cuda, BF16, w, b)
    _calibrate(dmx, fused, [dx], dmx.DmxAWQHyperparams(fuse_to_weight=True))
    sq = fused.smoothquant
    assert sq._flag("enabled") and sq._flag("fused_to_weight") and _same_bits(sq.scale, m.smoothquant.scale)
    assert _same_bits(fused.weight.detach(), dmx.ops.scale_channels(w.to(cuda), sq.scale, -1, False, BF16))
    with torch.no_grad():
        assert _same_bits(fused(dx), m(dx))
    with pytest.raises(dmx.DmxqError, match="fused"):   # a second search on the folded weight is refused
        with fused.awq_scaling(dmx.DmxAWQHyperparams()):
            pass


def test_a_weight_cast_outside_the_kernel_runs_the_modules_own_stages(dmx, cuda):
    w, b, x = A.dataset(3, BF16)
    dx = x.to(cuda)
    m = _linear(dmx, cuda, BF16, w, b, {"weight_format": dmx.format.BFP16_64})
    before = dict(_routes(dmx))
    _calibrate(dmx, m, [dx])
    assert _routes(dmx) == before   # neither route of awq_scaled_error: the stages themselves
    losses, best = m.awq_losses.cpu(), int(m.awq_best)
    print(f"BFP16_64: best {best}, losses[best] / losses[0] = {float(losses[best] / losses[0]):.4f}")
    assert bool(torch.isfinite(losses).all()) and float(losses[best]) <= float(losses[0])
    # candidate 0 is the plain cast's error
    with torch.no_grad():
        d0 = m.weight_cast(m.weight.detach()).float() - m.weight.detach().float()
    assert abs(float(losses[0]) - A.loss64(d0, m.awq_gram)) <= A.loss_bound(d0, m.awq_gram)
    assert m.smoothquant._flag("enabled")
    assert _same_bits(m.smoothquant.scale, dmx.ops.awq_candidate_scales(m.awq_x_mean, 20, m.smoothquant.scale_cast)[best])


def test_observe_under_a_graph_warm_up_and_a_single_capture(dmx, cuda):
    w, b, x = A.dataset(4, BF16)
    dx = x.to(cuda)
    first, second = dx[:40].contiguous(), dx[40:].contiguous()
    m = _linear(dmx, cuda, BF16, w, b)
    with torch.no_grad(), m.awq_scaling(dmx.DmxAWQHyperparams()):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m(first)                       # warm-up outside the capture: observed
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            m(second)                      # captured once ...
        g.replay()                         # ... and run once
        torch.cuda.synchronize()
        assert m.awq.n_tokens == A.TOKENS
    assert torch.equal(m.awq_sumabs.cpu(), A.sumabs_ref([x]))
    g64 = A.gram64([x])
    assert float((m.awq_gram.double().cpu() - g64).abs().max()) <= 1e-5 * float(g64.abs().max())
    eager = _linear(dmx, cuda, BF16, w, b)
    _calibrate(dmx, eager, [first, second])
    assert _same_bits(m.awq_gram, eager.awq_gram) and _same_bits(m.smoothquant.scale, eager.smoothquant.scale)


def test_recipe_gives_each_linear_its_own_scale(dmx, cuda):
    torch.manual_seed(4)
    model = torch.nn.Sequential(dmx.nn.Linear(256, 128), dmx.nn.Linear(128, 16)).to(cuda, BF16).eval()
    for layer in model:
        layer.configure({"weight_format": INT4, "weight_dynamic": {"per_group": 64}})
    recipe = dmx.DmxAWQRecipe(lambda mdl: {l: dmx.DmxAWQHyperparams(n_grid=5) for l in mdl})
    _, _, x = A.dataset(0, BF16)
    with torch.no_grad(), recipe.applied_to(model) as entered:
        assert len(entered) == 2 and all(l.awq is not None for l in model)
        model(x.to(cuda))
    for layer, fin in zip(model, (256, 128)):
        assert layer.awq is None and layer.smoothquant._flag("enabled")
        assert layer.smoothquant.scale.shape == (fin,) and layer.awq_losses.shape == (5,) and layer.awq_n_tokens == A.TOKENS
