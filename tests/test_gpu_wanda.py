"""-m gpu: Wanda -- ops.channel_sumsq, ops.wanda_score / ops.wanda_nm_sparsify, DmxModule.wanda_pruning and
DmxWandaRecipe -- against the definition in CPU torch (tests/_wanda_ref.py), bit for bit.

channel_sumsq is compared EXACTLY: the inputs are values with 2^-4 <= |x| < 2^4 whose squares are multiples of 2^-22 (bf16) or 2^-28
(f16), so a float64 sum of a few thousand of them is exact in any order (and a float32 accumulation is not: the same tests fail on
one).  The one randn float32 case is bounded by rows * 2^-52 relative, the bound of a float64 sum of exact terms in any order."""
import pytest
import torch

import _wanda_ref as R
from _data import bits_equal

pytestmark = pytest.mark.gpu
F = torch.nn.functional
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = {"bf16": BF16, "f16": F16, "f32": F32}


def _routes(dmx):
    return dmx.ops._front._wanda_routes


def _same_bits(got, want):
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    return bits_equal(got, want) == 0


# ------------------------------------------------------------------------------------------------ channel_sumsq
SUMSQ_SHAPES = [(1, 8), (3, 40), (257, 1032), (4099, 768), (2, 130, 256)]
_INPUTS = {}


def _exact(shape, dtype, seed=0):
    key = (shape, dtype, seed)
    if key not in _INPUTS:
        x = R.exact_values(shape, dtype, seed + sum(shape))
        _INPUTS[key] = (x, R.sumsq_ref([x]))
    return _INPUTS[key]


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("shape", SUMSQ_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_channel_sumsq_is_exact(dmx, cuda, shape, dtype):
    x, want = _exact(shape, DTYPES[dtype])
    got = dmx.ops.channel_sumsq(x.to(cuda))
    assert got.dtype == torch.float64 and got.shape == (shape[-1],) and got.device.type == "cuda"
    assert torch.equal(got.cpu(), want), float((got.cpu() - want).abs().max())


def test_channel_sumsq_generic_form_channels_that_are_not_whole_vectors(dmx, cuda):
    x, want = _exact((5, 13), BF16)
    assert torch.equal(dmx.ops.channel_sumsq(x.to(cuda)).cpu(), want)
    x, want = _exact((70, 13), F16)
    assert torch.equal(dmx.ops.channel_sumsq(x.to(cuda)).cpu(), want)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_channel_sumsq_unaligned_pointer(dmx, cuda, dtype):
    x, want = _exact((37, 64), DTYPES[dtype])
    buf = torch.zeros(37 * 64 + 1, dtype=x.dtype, device=cuda)
    view = buf[1:].view(37, 64)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    assert torch.equal(dmx.ops.channel_sumsq(view).cpu(), want)


def test_channel_sumsq_non_contiguous_input(dmx, cuda):
    x, _ = _exact((64, 40), BF16)
    xt = x.to(cuda).t()   # [40, 64], channels strided
    assert not xt.is_contiguous()
    assert torch.equal(dmx.ops.channel_sumsq(xt).cpu(), R.sumsq_ref([x.t()]))


def test_channel_sumsq_accumulates_batches_into_out(dmx, cuda):
    batches = [R.exact_values(s, BF16, 10 + i) for i, s in enumerate([(5, 64), (2, 7, 64), (1, 64)])]
    out = torch.zeros(64, dtype=torch.float64, device=cuda)
    for b in batches:
        assert dmx.ops.channel_sumsq(b.to(cuda), out=out) is out
    want = R.sumsq_ref(batches)
    assert torch.equal(out.cpu(), want)
    cat = torch.cat([b.reshape(-1, 64) for b in batches])
    assert torch.equal(dmx.ops.channel_sumsq(cat.to(cuda)).cpu(), want)


def test_channel_sumsq_f32_inputs_holding_bf16_values_are_exact(dmx, cuda):
    for shape in [(3, 40), (4099, 768), (5, 13)]:
        x, want = _exact(shape, F32)
        assert torch.equal(dmx.ops.channel_sumsq(x.to(cuda)).cpu(), want), shape


def test_channel_sumsq_randn_f32_within_the_float64_summation_bound(dmx, cuda):
    rows = 4099
    x = torch.randn(rows, 768, generator=torch.Generator().manual_seed(3))
    want = R.sumsq_ref([x])
    dx = x.to(cuda)
    got = dmx.ops.channel_sumsq(dx)
    rel = ((got.cpu() - want).abs() / want).max().item()
    print(f"channel_sumsq randn f32 [{rows}, 768]: largest relative difference {rel:.3e}, bound {rows * 2.0 ** -52:.3e}")
    assert rel <= rows * 2.0 ** -52
    # the same call twice, and the scalar-load form of the same data: equal bits (a fixed order that does not depend on the form)
    assert torch.equal(dmx.ops.channel_sumsq(dx), got)
    buf = torch.empty(rows * 768 + 1, dtype=F32, device=cuda)
    view = buf[1:].view(rows, 768)
    view.copy_(dx)
    assert torch.equal(dmx.ops.channel_sumsq(view), got)


def test_channel_sumsq_under_a_captured_graph_adds_on_every_replay(dmx, cuda):
    x, want = _exact((257, 1032), BF16)
    dx = x.to(cuda)
    out = torch.zeros(1032, dtype=torch.float64, device=cuda)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dmx.ops.channel_sumsq(dx, out=out)   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    out.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dmx.ops.channel_sumsq(dx, out=out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), 2 * want)


# ------------------------------------------------------------------------------------------------ wanda_nm_sparsify
def _weight(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(shape, generator=g)
    w[..., ::5] = (w[..., ::5] * 4).round() / 4   # ties inside groups
    return w.to(dtype)


def _norm(L, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(L, generator=g) * 3 + 0.25).round(decimals=1).float()   # a few equal norms


def _check_against_ref(dmx, cuda, oracle, w, an, K, M, fused_class=True):
    score, mask, y = R.wanda_ref(w, an, K, M, oracle)
    dw, dan = w.to(cuda), an.to(cuda)
    routes = _routes(dmx)
    for fused in ((True, False) if fused_class else (None, False)):
        before = dict(routes)
        gy, gm, gs = dmx.ops.wanda_nm_sparsify(dw, dan, K, M, return_mask=True, return_score=True, fused=fused)
        took = "fused" if fused else "chain"
        assert routes[took] == before[took] + 1 and sum(routes.values()) == sum(before.values()) + 1, (fused, before, routes)
        assert _same_bits(gs, score), ("score", fused)
        assert _same_bits(gm, mask), ("mask", fused)
        assert _same_bits(gy, y), ("y", fused)
    return score, mask, y


@pytest.mark.parametrize("shape", [(1, 16), (3, 64), (257, 1024)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("KM", [(2, 4), (1, 4), (4, 8), (2, 8), (8, 16)], ids=lambda km: f"{km[0]}of{km[1]}")
def test_wanda_nm_sparsify_kernel_chain_and_reference_agree(dmx, cuda, oracle, KM, dtype, shape):
    K, M = KM
    assert dmx.ops.wanda_class(DTYPES[dtype], shape[1], M)
    _check_against_ref(dmx, cuda, oracle, _weight(shape, DTYPES[dtype], 7 + M), _norm(shape[1], K), K, M)


def test_wanda_chain_class_shape_5x24_4of8(dmx, cuda, oracle):
    """rows of 24 bf16 elements are not whole 16-element spans: fused=True raises, fused=None runs the chain"""
    w, an = _weight((5, 24), BF16, 1), _norm(24, 2)
    assert not dmx.ops.wanda_class(BF16, 24, 8)
    with pytest.raises(NotImplementedError):
        dmx.ops.wanda_nm_sparsify(w.to(cuda), an.to(cuda), 4, 8, fused=True)
    _check_against_ref(dmx, cuda, oracle, w, an, 4, 8, fused_class=False)   # fused=None runs the chain


def test_wanda_4x40_8of16_is_refused_and_an_8of16_chain_class_runs_the_chain(dmx, cuda, oracle):
    """[4, 40] with 8:16: 16 does not divide 40, so no N:M mask exists on any route (dmxq_nm_mask refuses it too) -- fused=True raises, and
    so do fused=None and fused=False.  The chain class of 8:16 that does exist is a tensor the kernel cannot take for its alignment: the
    same weight two bytes into a buffer, where fused=True raises and fused=None runs the chain."""
    w, an = _weight((4, 40), BF16, 1), _norm(40, 2)
    assert not dmx.ops.wanda_class(BF16, 40, 16)
    for fused in (True, None, False):
        with pytest.raises(ValueError):
            dmx.ops.wanda_nm_sparsify(w.to(cuda), an.to(cuda), 8, 16, fused=fused)
    w, an = _weight((4, 48), BF16, 3), _norm(48, 4)
    buf = torch.zeros(4 * 48 + 1, dtype=BF16, device=cuda)
    view = buf[1:].view(4, 48)
    view.copy_(w)
    with pytest.raises(NotImplementedError):
        dmx.ops.wanda_nm_sparsify(view, an.to(cuda), 8, 16, fused=True)
    score, mask, y = R.wanda_ref(w, an, 8, 16, oracle)
    before = dict(_routes(dmx))
    gy, gm, gs = dmx.ops.wanda_nm_sparsify(view, an.to(cuda), 8, 16, return_mask=True, return_score=True)
    assert _routes(dmx)["chain"] == before["chain"] + 1 and _routes(dmx)["fused"] == before["fused"]
    assert _same_bits(gs, score) and _same_bits(gm, mask) and _same_bits(gy, y)


def test_wanda_unaligned_weight_goes_to_the_chain(dmx, cuda, oracle):
    w, an = _weight((3, 64), BF16, 5), _norm(64, 6)
    buf = torch.zeros(3 * 64 + 1, dtype=BF16, device=cuda)
    view = buf[1:].view(3, 64)
    view.copy_(w)
    with pytest.raises(NotImplementedError):
        dmx.ops.wanda_nm_sparsify(view, an.to(cuda), 2, 4, fused=True)
    before = dict(_routes(dmx))
    y = dmx.ops.wanda_nm_sparsify(view, an.to(cuda), 2, 4)
    assert _routes(dmx)["chain"] == before["chain"] + 1
    assert _same_bits(y, R.wanda_ref(w, an, 2, 4, oracle)[2])


def test_wanda_planted_rows(dmx, cuda, oracle):
    nan, inf = float("nan"), float("inf")
    L = 32
    w = _weight((8, L), BF16, 11)
    an = torch.full((L,), 2.0)
    w[0] = 1.5                      # all-equal weights, equal norms: ties go by index
    an[8] = 0.0                     # a zero-norm (dead) column
    an[9] = inf                     # an Inf norm
    an[17] = nan                    # a NaN norm: its column ranks highest
    w[1, 3] = nan                   # a NaN weight
    w[2, :8] = -0.0                 # -0.0 weights: y keeps the sign
    w[3, 4] = 3e38                  # x norm 4 overflows: the score is Inf
    w[3, 5] = -3e38
    an[4] = an[5] = 4.0
    w[4, 9] = 0.0                   # 0 x Inf = NaN
    for K, M in [(2, 4), (4, 8), (8, 16)]:
        score, mask, y = _check_against_ref(dmx, cuda, oracle, w, an, K, M)
        # the argsort form of the rule gives what the oracle gives on these rows
        assert torch.equal(R.nm_ref(score, K, M), mask)
    score, mask, y = R.wanda_ref(w, an, 2, 4, oracle)
    assert mask[0, 12:16].tolist() == [0.0, 0.0, 1.0, 1.0] and mask[0, 24:32].tolist() == [0.0, 0.0, 1.0, 1.0] * 2
    assert bool((score[:, 8] == 0).all()) and torch.isnan(score[4, 9])
    assert torch.isinf(score[3, 4]) and torch.isinf(score[3, 5]) and mask[3, 4:8].tolist() == [1.0, 1.0, 0.0, 0.0]
    assert torch.isnan(score[:, 17]).all() and bool((mask[:, 17] == 1).all())
    assert mask[1, 3] == 1 and torch.isnan(y[1, 3])
    zeroed = (mask[2, :8] == 0)
    assert bool((torch.signbit(y[2, :8])).all()) and bool(zeroed.any())


def test_wanda_each_output_alone_and_score_only(dmx, cuda, oracle):
    w, an = _weight((3, 64), F16, 21), _norm(64, 22)
    score, mask, y = R.wanda_ref(w, an, 4, 8, oracle)
    dw, dan = w.to(cuda), an.to(cuda)
    for fused in (True, False):
        assert _same_bits(dmx.ops.wanda_nm_sparsify(dw, dan, 4, 8, fused=fused), y)
        assert _same_bits(dmx.ops.wanda_nm_sparsify(dw, dan, 4, 8, return_mask=True, return_y=False, fused=fused), mask)
        assert _same_bits(dmx.ops.wanda_nm_sparsify(dw, dan, 4, 8, return_score=True, return_y=False, fused=fused), score)
        # K = M = 0: the score only
        before = dict(_routes(dmx))
        assert _same_bits(dmx.ops.wanda_score(dw, dan, fused=fused), score)
        assert _same_bits(dmx.ops.wanda_nm_sparsify(dw, dan, 0, 0, return_score=True, return_y=False, fused=fused), score)
        assert _routes(dmx)["fused" if fused else "chain"] == before["fused" if fused else "chain"] + 2
        # y in the weight's own dtype
        assert _same_bits(dmx.ops.wanda_nm_sparsify(dw, dan, 4, 8, fused=fused, out_dtype=F16), y.to(F16))


def test_wanda_above_two_to_the_31_elements(dmx, cuda, oracle):
    import _large_cases as LC
    rows, L = 524289, 4096
    assert rows * L > 2 ** 31
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    need = 2 * rows * L * 2 + (1 << 30)
    if free < need:
        pytest.skip(f"needs {need / 2 ** 30:.1f} GiB of device memory, {free / 2 ** 30:.1f} GiB free")
    w = LC.device_input("weight", (rows, L), BF16, 16, cuda)
    an = _norm(L, 17)
    before = dict(_routes(dmx))
    y = dmx.ops.wanda_nm_sparsify(w, an.to(cuda), 2, 4, fused=True, out_dtype=BF16)
    assert _routes(dmx)["fused"] == before["fused"] + 1
    picked = list(range(rows - 8, rows)) + [0, 1, 65537, 262143, 262144, 400001, 524279, 524280]   # (row 524288 begins at element 2^31)
    idx = torch.tensor(picked, device=cuda)
    wr, yr = w[idx].cpu(), y[idx].cpu()
    del w, y
    torch.cuda.empty_cache()
    want = R.wanda_ref(wr, an, 2, 4, oracle)[2].to(BF16)
    assert _same_bits(yr, want)


# ------------------------------------------------------------------------------------------------ module
SPARSE = "BTOPK{2:4,-1}(U)"
BATCH_SHAPES = [(5, 64), (2, 7, 64), (1, 64)]


def _linear(dmx, cuda, dtype, sparseness=SPARSE, fin=64, fout=32, seed=0):
    torch.manual_seed(seed)
    m = dmx.nn.Linear(fin, fout).to(cuda, dtype).eval()
    m.configure({"weight_sparseness": sparseness})
    return m


def _batches(dtype, seed=0, shapes=BATCH_SHAPES):
    g = torch.Generator().manual_seed(100 + seed)
    return [torch.randn(s, generator=g).to(dtype) for s in shapes]


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_wanda_pruning_on_a_linear(dmx, cuda, oracle, dtype):
    dt = DTYPES[dtype]
    m = _linear(dmx, cuda, dt)
    w0 = m.weight.detach().clone()
    batches = _batches(dt)
    with torch.no_grad(), m.wanda_pruning(dmx.DmxWandaHyperparams()) as ctx:
        assert ctx is m and m.wanda is not None
        for b in batches:
            m(b.to(cuda))
        assert m.wanda.n_tokens == 5 + 14 + 1
    assert m.wanda is None
    an = R.act_norm_ref(R.sumsq_ref(batches))
    score, mask, y = R.wanda_ref(w0, an, 2, 4, oracle)
    sp = m.weight_sparsifier
    assert isinstance(sp.score, torch.nn.Parameter) and sp.score.device == m.weight.device and sp.score.shape == m.weight.shape
    assert _same_bits(m.wanda_act_norm, an)
    assert _same_bits(sp.score.detach(), score)
    assert _same_bits(sp.mask, mask)
    assert "wanda_act_norm" not in m.state_dict() and not any("wanda" in k for k in m.state_dict())
    assert not sp.plastic
    # the weight Parameter is unchanged; the effective weight and the forward are those of W * mask
    assert torch.equal(m.weight.detach(), w0)
    x = _batches(dt, seed=9, shapes=[(6, 64)])[0].to(cuda)
    with torch.no_grad():
        assert _same_bits(m.effective_weight, y)
        out = m(x)
        want = F.linear(x, (w0 * mask.to(cuda)).to(dt), m.bias.detach())
    assert torch.equal(out, want)
    # a later forward observed nothing
    assert m.wanda is None and m.wanda_n_tokens == 20 and _same_bits(m.wanda_act_norm, an)
    # a state_dict round trip into a fresh module reproduces the mask
    fresh = _linear(dmx, cuda, dt, seed=5)
    with torch.no_grad():
        fresh(x)   # (the lazy sparsifier takes the weight's shape at its first forward)
    fresh.load_state_dict(m.state_dict())
    with torch.no_grad():
        assert torch.equal(fresh(x), want)
    assert _same_bits(fresh.weight_sparsifier.mask, mask)


def test_wanda_reset_false_continues_the_accumulation(dmx, cuda, oracle):
    m = _linear(dmx, cuda, BF16)
    a, b = _batches(BF16, 1), _batches(BF16, 2)
    with torch.no_grad():
        with m.wanda_pruning(dmx.DmxWandaHyperparams()):
            for t in a:
                m(t.to(cuda))
        with m.wanda_pruning(dmx.DmxWandaHyperparams(reset=False)):
            for t in b:
                m(t.to(cuda))
    assert m.wanda_n_tokens == 40
    an = R.act_norm_ref(R.sumsq_ref(a + b))
    assert _same_bits(m.weight_sparsifier.score.detach(), R.score_ref(m.weight, an))
    with torch.no_grad(), m.wanda_pruning(dmx.DmxWandaHyperparams()):   # reset=True: b alone
        for t in b:
            m(t.to(cuda))
    assert m.wanda_n_tokens == 20
    assert _same_bits(m.weight_sparsifier.score.detach(), R.score_ref(m.weight, R.act_norm_ref(R.sumsq_ref(b))))


def test_wanda_topk_sparseness_gets_the_score_and_the_global_mask_follows(dmx, cuda):
    m = _linear(dmx, cuda, F32, sparseness="TOPK{0.5}(U)")   # (float32 weights: no two scores tie)
    batches = _batches(F32, 3)
    before = dict(_routes(dmx))
    with torch.no_grad(), m.wanda_pruning(dmx.DmxWandaHyperparams()):
        for t in batches:
            m(t.to(cuda))
    assert _routes(dmx)["fused"] == before["fused"] + 1
    score = R.score_ref(m.weight, R.act_norm_ref(R.sumsq_ref(batches)))
    assert _same_bits(m.weight_sparsifier.score.detach(), score)
    flat = score.flatten()
    assert flat.unique().numel() == flat.numel()   # no ties: the global rule is unambiguous
    want = torch.ones_like(flat)
    want[torch.argsort(flat, stable=True)[:flat.numel() // 2]] = 0.0
    assert torch.equal(m.weight_sparsifier.mask.cpu(), want.reshape(score.shape))
    with torch.no_grad():
        m(batches[0].to(cuda))
    assert torch.equal(m.weight_sparsifier.mask.cpu(), want.reshape(score.shape))


def test_wanda_recipe_gives_each_linear_its_own_statistics(dmx, cuda, oracle):
    torch.manual_seed(4)
    model = torch.nn.Sequential(dmx.nn.Linear(64, 32), dmx.nn.Linear(32, 16)).to(cuda, BF16).eval()
    for layer in model:
        layer.configure({"weight_sparseness": SPARSE})
    seen = {layer: [] for layer in model}
    hooks = [layer.register_forward_pre_hook(lambda mod, args: seen[mod].append(args[0].detach().cpu())) for layer in model]
    recipe = dmx.DmxWandaRecipe(lambda mdl: {l: dmx.DmxWandaHyperparams() for l in mdl if isinstance(l, dmx.nn.Linear)})
    with torch.no_grad(), recipe.applied_to(model) as entered:
        assert len(entered) == 2 and all(l.wanda is not None for l in model)
        for t in _batches(BF16, 6):
            model(t.to(cuda))
    for h in hooks:
        h.remove()
    for layer in model:
        assert layer.wanda is None
        an = R.act_norm_ref(R.sumsq_ref(seen[layer]))
        score, mask, _ = R.wanda_ref(layer.weight, an, 2, 4, oracle)
        assert _same_bits(layer.weight_sparsifier.score.detach(), score)
        assert _same_bits(layer.weight_sparsifier.mask, mask)
    assert model[0].wanda_act_norm.shape == (64,) and model[1].wanda_act_norm.shape == (32,)


def test_wanda_leaving_without_a_forward_raises_and_keeps_the_score(dmx, cuda):
    m = _linear(dmx, cuda, BF16)
    with torch.no_grad():
        m(_batches(BF16, 7)[0].to(cuda))
    score0 = m.weight_sparsifier.score.detach().clone()
    with pytest.raises(RuntimeError, match="no calibration token"):
        with m.wanda_pruning(dmx.DmxWandaHyperparams()):
            pass
    assert m.wanda is None
    assert torch.equal(m.weight_sparsifier.score.detach(), score0)


def test_wanda_score_through_the_fused_weight_hypernet_with_basic_casts(dmx, cuda):
    f = dmx.format
    m = _linear(dmx, cuda, BF16)
    m.configure(dict(input_formats=[f.BFP16_64], weight_format=f.BFP16_64, bias_format=f.BFP32_1, output_formats=[f.FLOAT16]))
    with torch.no_grad(), m.wanda_pruning(dmx.DmxWandaHyperparams()):
        for t in _batches(BF16, 8):
            m(t.to(cuda))
    with torch.no_grad():
        assert m._fused_weight_plan(m.weight) is not None
        fused = m.weight_hypernet(m.weight, BF16)
        m.fuse_weight_hypernet = False
        chain = m.weight_hypernet(m.weight).to(BF16)
    assert _same_bits(fused.to(BF16), chain)
