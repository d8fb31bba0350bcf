"""GPU tests of AWQ weight clipping (csrc/awq_clip.hip, ops.awq_clip, DmxModule.awq_clipping, DmxAWQHyperparams.clip; DESIGN.md §8 "AWQ
clipping"): the kernel (fused=True), the chain of torch operations (fused=False) and the CPU checker of tests/_awq_clip_ref.py (the
definition) agree bit for bit on y, best, clip and losses (a NaN matching any NaN); geometry, planted groups, the index convention of
the blocks, ties, routing, in-place output, graph capture and the module surface."""
import pytest
import torch

import _awq_clip_ref as R

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
INT4 = "XP[4,0](CSN)"


def fmt_of(p, sym=True):
    return f"XP[{p},0](C{'S' if sym else '_'}N)"


@pytest.fixture(autouse=True)
def _stop_the_session_after_a_gpu_fault():
    """a HIP error after a test (an illegal access is sticky) ends the session: nothing more is started on a faulted device"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # pragma: no cover
        pytest.exit(f"GPU fault, stopping the session: {e}", returncode=3)


def routes_of(dmx):
    return dmx.ops._front._awq_clip_routes


def run(dmx, w, blocks, fmt, g, fused, took=None, **kw):
    """ops.awq_clip with every output, asserting on the host-side route counter which route ran"""
    before = dict(routes_of(dmx))
    out = dmx.ops.awq_clip(w, blocks, fmt, g, fused=fused, return_best=True, return_clip=True, return_losses=True, **kw)
    took = took or ("fused" if fused else "chain")
    other = "chain" if took == "fused" else "fused"
    assert routes_of(dmx)[took] == before[took] + 1 and routes_of(dmx)[other] == before[other]
    return out


def same4(got, want, what):
    (y, best, clip, losses), (wy, wbest, wclip, wlosses) = got, want[:4]
    assert y.dtype == wy.dtype and best.dtype == torch.uint8 and clip.dtype == F32 and losses.dtype == F32, what
    assert torch.equal(best.cpu(), wbest), f"{what}: best"
    assert R.same(clip, wclip), f"{what}: clip"
    assert R.same(losses, wlosses), f"{what}: losses"
    assert R.same(y, wy), f"{what}: y"


def check_both(dmx, cuda, w, blocks, p, g, sym, want, what, ratios=None):
    dw, db = w.to(cuda), blocks.to(cuda)
    kw = {} if ratios is None else {"ratios": ratios}
    same4(run(dmx, dw, db, fmt_of(p), g, True, symmetric_qscheme=sym, **kw), want, f"{what} kernel")
    same4(run(dmx, dw, db, fmt_of(p), g, False, symmetric_qscheme=sym, **kw), want, f"{what} chain")
    assert torch.equal(dw.cpu().view(torch.int16 if w.element_size() == 2 else torch.int32),
                       w.view(torch.int16 if w.element_size() == 2 else torch.int32))     # the input is not written


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_kernel_chain_and_checker_agree(dmx, cuda, case):
    """rows 1, 3, 9 x L = g, 3 g per case; tests/test_awq_clip_host.py shows that the cases with p <= 4 are not vacuous"""
    g, p, sym, dt = case
    for w, blocks, want in R.case_data(case):
        check_both(dmx, cuda, w, blocks, p, g, sym, want, f"{R.case_id(case)} {list(w.shape)}")
        if p == 8:
            assert int(want[1].max()) == 0


def test_more_rows_than_a_slab_and_a_partial_last_pass(dmx, cuda):
    """g = 16: a workgroup takes 64 rows per pass and the grid holds at most 4 workgroups per compute unit, divided over the 3 column
    groups: 22,001 rows are 344 passes per column group, more than the grid has workgroups for it on 256 compute units (342), so
    workgroups loop; the last pass holds 49 rows"""
    g, rows = 16, 22001
    w, blocks = R.dataset(rows, 3 * g, g, seed=77, dtype=BF16)
    want = R.clip_ref(w, blocks, R.clip_ratios(), 4, True, g, False)
    assert len(want[1].unique()) >= 3
    same4(run(dmx, w.to(cuda), blocks.to(cuda), INT4, g, True), want, "22001 x 48 kernel")


@pytest.mark.parametrize("g,dtype", [(16, BF16), (32, F16), (64, F32), (128, BF16)], ids=["g16-bf16", "g32-f16", "g64-f32", "g128-bf16"])
def test_planted_groups(dmx, cuda, g, dtype):
    """all-zero, NaN, +Inf, -Inf and constant groups at the first, middle and last positions: the first four keep their bits with best 0,
    clip = max |W| and NaN losses, and their neighbours in the same wave are untouched by them"""
    w, blocks = R.dataset(9, 3 * g, g, seed=g, dtype=dtype)
    wp, spots = R.plant(w, g)
    want = R.clip_ref(wp, blocks, R.clip_ratios(), 3, True, g, False)
    for name in ("zero", "nan", "pinf", "ninf"):
        for i in spots[name]:
            assert int(want[1].reshape(-1)[i]) == 0 and bool(torch.isnan(want[3].reshape(-1, 10)[i]).all())
    check_both(dmx, cuda, wp, blocks, 3, g, False, want, f"planted g{g}")


def test_a_block_that_is_not_symmetric_pins_the_index_convention(dmx, cuda):
    g = 32
    w, blocks = R.dataset(9, 3 * g, g, seed=5, dtype=F32)
    skew = (blocks + torch.triu(torch.ones(g, g), 1)[None] * blocks.abs().mean()).contiguous()
    want = R.clip_ref(w, skew, R.clip_ratios(), 3, True, g, False)
    assert not R.same(want[3], R.clip_ref(w, skew.transpose(1, 2).contiguous(), R.clip_ratios(), 3, True, g, False)[3])
    check_both(dmx, cuda, w, skew, 3, g, False, want, "skew blocks")


def test_all_zero_blocks_and_repeated_ratios(dmx, cuda):
    g = 16
    w, blocks = R.dataset(9, 3 * g, g, seed=6, dtype=BF16)
    zero = torch.zeros_like(blocks)
    want = R.clip_ref(w, zero, R.clip_ratios(), 2, True, g, False)
    assert bool((want[3] == 0).all()) and int(want[1].max()) == 0          # every loss is 0: candidate 0
    check_both(dmx, cuda, w, zero, 2, g, False, want, "zero blocks")
    r = torch.tensor([1.0, 0.7, 0.7, 0.5])
    want = R.clip_ref(w, blocks, r, 2, True, g, False)
    picked = want[1].unique().tolist()
    assert 1 in picked and 2 not in picked                                 # the tie goes to the lower index
    check_both(dmx, cuda, w, blocks, 2, g, False, want, "repeated ratio", ratios=r)
    check_both(dmx, cuda, w, blocks, 2, g, False, want, "repeated ratio as a list", ratios=[1.0, 0.7, 0.7, 0.5])
    check_both(dmx, cuda, w, blocks, 2, g, False, want, "repeated ratio on the device", ratios=r.to(cuda))


def test_in_place_output(dmx, cuda):
    g = 64
    w, blocks = R.dataset(9, 3 * g, g, seed=8, dtype=BF16)
    want = R.clip_ref(w, blocks, R.clip_ratios(), 3, True, g, False)
    for fused in (True, False):
        dw = w.to(cuda)
        got = run(dmx, dw, blocks.to(cuda), fmt_of(3), g, fused, out=dw)
        assert got[0].data_ptr() == dw.data_ptr()
        same4(got, want, f"out=w fused={fused}")
    y_only = dmx.ops.awq_clip(w.to(cuda), blocks.to(cuda), fmt_of(3), g)
    assert isinstance(y_only, torch.Tensor) and R.same(y_only, want[0])
    y, clip = dmx.ops.awq_clip(w.to(cuda), blocks.to(cuda), fmt_of(3), g, return_clip=True)
    assert R.same(clip, want[2])


def test_what_the_kernel_does_not_take_runs_the_chain(dmx, cuda):
    # an unaligned view: the chain under fused=None, NotImplementedError under fused=True
    g = 16
    w, blocks = R.dataset(3, 3 * g, g, seed=9, dtype=BF16)
    want = R.clip_ref(w, blocks, R.clip_ratios(), 4, True, g, False)
    buf = torch.zeros(3 * 3 * g + 8, dtype=BF16, device=cuda)
    view = buf[1:1 + 3 * 3 * g].view(3, 3 * g)
    view.copy_(w)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    same4(run(dmx, view, blocks.to(cuda), INT4, g, None, took="chain"), want, "unaligned view")
    with pytest.raises(NotImplementedError):
        dmx.ops.awq_clip(view, blocks.to(cuda), INT4, g, fused=True)
    # g = 256
    g = 256
    w, blocks = R.dataset(2, g, g, seed=10, dtype=F16)
    want = R.clip_ref(w, blocks, R.clip_ratios(), 3, True, g, True)
    assert not dmx.ops.awq_clip_class(F16, g, g)
    same4(run(dmx, w.to(cuda), blocks.to(cuda), fmt_of(3), g, None, took="chain", symmetric_qscheme=True), want, "g 256")
    with pytest.raises(NotImplementedError):
        dmx.ops.awq_clip(w.to(cuda), blocks.to(cuda), fmt_of(3), g, fused=True)
    # and what it takes goes to it by default unless the measurement table says otherwise
    g = 64
    w, blocks = R.dataset(3, g, g, seed=11, dtype=BF16)
    took = "chain" if g in dmx.ops.AWQ_CLIP_CHAIN_BY_DEFAULT else "fused"
    same4(run(dmx, w.to(cuda), blocks.to(cuda), INT4, g, None, took=took), R.clip_ref(w, blocks, R.clip_ratios(), 4, True, g, False), "default route")


def test_both_bindings_make_the_same_call(dmx, cuda):
    g = 16
    w, blocks = R.dataset(9, 3 * g, g, seed=14, dtype=F16)
    want = R.clip_ref(w, blocks, R.clip_ratios(), 3, True, g, True)
    for binding in ("torch", "ctypes"):
        front = dmx.ops.front(binding)
        before = dict(front._awq_clip_routes)
        got = front.awq_clip(w.to(cuda), blocks.to(cuda), fmt_of(3), g, symmetric_qscheme=True, fused=True, return_best=True, return_clip=True,
                             return_losses=True)
        assert front._awq_clip_routes["fused"] == before["fused"] + 1
        same4(got, want, binding)
        y_only = front.awq_clip(w.to(cuda), blocks.to(cuda), fmt_of(3), g, symmetric_qscheme=True, fused=True)
        assert R.same(y_only, want[0])


def test_capture_and_replay(dmx, cuda):
    g = 32
    w, blocks = R.dataset(9, 3 * g, g, seed=12, dtype=BF16)
    w2, _ = R.dataset(9, 3 * g, g, seed=13, dtype=BF16)
    ratios = R.clip_ratios()
    dw, db = w.to(cuda), blocks.to(cuda)
    run(dmx, dw, db, fmt_of(3), g, True)                     # (warm-up: the code object, the device copy of the ratios)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = dmx.ops.awq_clip(dw, db, fmt_of(3), g, fused=True, return_best=True, return_clip=True, return_losses=True)
    dw.copy_(w2.to(cuda))                                    # other data in the captured input
    graph.replay()
    torch.cuda.synchronize()
    same4(got, R.clip_ref(w2, blocks, ratios, 3, True, g, False), "replay")


# ------------------------------------------------------------------------------------------------ module
IN, OUT, G = 64, 32, 16


def _module_data(seed, dtype):
    gen = torch.Generator().manual_seed(9000 + seed)
    w = (0.05 * torch.randn(OUT, IN, generator=gen)).to(dtype)
    b = (0.05 * torch.randn(OUT, generator=gen)).to(dtype)
    x = (torch.randn(96, IN, generator=gen) * (1.0 + 3.0 * torch.rand(IN, generator=gen))).to(dtype)
    return w, b, x


def _linear(dmx, cuda, dt, w, b):
    m = dmx.nn.Linear(IN, OUT).to(cuda, dt).eval()
    with torch.no_grad():
        m.weight.copy_(w)
        m.bias.copy_(b)
    m.configure({"weight_format": INT4, "weight_dynamic": {"per_group": G}})
    return m


def _blocks_by_hand(dmx, batches):
    """AWQClipCalibrator's running mean, spelled with the same torch operations"""
    blocks, n = None, 0
    with dmx.ops._front._full_fp32_matmul():
        for t in batches:
            x = t.reshape(-1, IN).float()
            k = x.shape[0]
            x = x * (1.0 / (n + k) ** 0.5)
            x = x.reshape(k, IN // G, G).transpose(0, 1)
            blocks = torch.zeros(IN // G, G, G, device=t.device) if blocks is None else blocks
            blocks *= n / (n + k)
            blocks.baddbmm_(x.transpose(1, 2), x)
            n += k
    return blocks


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_awq_clipping_on_a_linear(dmx, cuda, dtype):
    w, b, x = _module_data(0, dtype)
    m = _linear(dmx, cuda, dtype, w, b)
    dx = x.to(cuda)
    batches = [dx[:40], dx[40:].reshape(2, 28, IN)]
    with torch.no_grad(), m.awq_clipping(dmx.DmxAWQClipHyperparams()) as ctx:
        assert ctx is m and isinstance(m.awq_clipper, dmx.AWQClipCalibrator)
        for t in batches:
            m(t)
    assert m.awq_clipper is None and m.awq_clip_n_tokens == 96
    blocks = _blocks_by_hand(dmx, batches)
    assert R.same(m.awq_clip_blocks, blocks)
    # the blocks are the diagonal blocks of the inputs' second moment (float32 GEMMs in another order: close, not bitwise)
    ref = R.moment_blocks(x.float(), G)
    assert float((blocks.cpu() - ref).abs().max()) <= 1e-4 * float(ref.abs().max())
    # the weight equals ops.awq_clip of the old weight with the accumulated blocks -- and the checker's
    y, best, clip, losses = dmx.ops.awq_clip(w.to(cuda), blocks, INT4, G, return_best=True, return_clip=True, return_losses=True)
    assert R.same(m.weight.detach(), y) and torch.equal(m.awq_clip["best"], best) and R.same(m.awq_clip["clip"], clip)
    assert m.awq_clip["group_size"] == G and torch.equal(m.awq_clip["ratios"], R.clip_ratios())
    want = R.clip_ref(w, blocks, R.clip_ratios(), 4, True, G, False)
    same4((y, best, clip, losses), want, "module")
    assert len(best.unique()) >= 3
    # the summed per-group loss did not rise
    chosen = losses.gather(-1, best.long()[..., None])[..., 0]
    assert bool((chosen <= losses[..., 0]).all()) and float(chosen.double().sum()) < float(losses[..., 0].double().sum())
    # the forward's weight cast of the new weight equals the search's q
    with torch.no_grad():
        wq = m.weight_hypernet(m.weight)
    assert R.same(wq.float(), want[4])
    assert m.weight_cast._flag("fake_quant_enabled") and m.weight_cast.dynamic == {"per_group": G}
    assert not any("awq" in k for k in m.state_dict())
    # reset=False continues the statistics
    with torch.no_grad(), m.awq_clipping(dmx.DmxAWQClipHyperparams(reset=False)):
        m(dx[:8])
    assert m.awq_clip_n_tokens == 104


def test_awq_scaling_with_and_without_a_clip(dmx, cuda):
    w, b, x = _module_data(1, BF16)
    dx = x.to(cuda)

    def calibrated(hp):
        m = _linear(dmx, cuda, BF16, w, b)
        with torch.no_grad(), m.awq_scaling(hp):
            m(dx)
        return m

    plain = calibrated(dmx.DmxAWQHyperparams(n_grid=8, fuse_to_weight=True))
    assert plain.awq_clip is None and plain.awq_clip_blocks is None
    # clip=None: today's bits -- the fuse done by hand on a twin
    twin = calibrated(dmx.DmxAWQHyperparams(n_grid=8))
    twin.smoothquant.fuse_to_weight(twin.weight)
    assert R.same(plain.weight.detach(), twin.weight.detach()) and R.same(plain.smoothquant.scale, twin.smoothquant.scale)
    # with a clip: scaling, fusing and clipping done by hand
    m = calibrated(dmx.DmxAWQHyperparams(n_grid=8, fuse_to_weight=True, clip=dmx.DmxAWQClipHyperparams(n_grid=10)))
    assert R.same(m.smoothquant.scale, plain.smoothquant.scale) and m.awq_clip_n_tokens == 96
    s = plain.smoothquant.scale.detach().float()
    blocks = dmx.ops.awq_gram_blocks(plain.awq_gram / s[:, None] / s[None, :], G)
    ratios = dmx.ops.awq_clip_ratios(10, 0.5)
    y, best, clip = dmx.ops.awq_clip(plain.weight.detach(), blocks, INT4, G, ratios, return_best=True, return_clip=True)
    assert R.same(m.awq_clip_blocks, blocks)
    assert R.same(m.weight.detach(), y) and torch.equal(m.awq_clip["best"], best) and R.same(m.awq_clip["clip"], clip)
    assert torch.equal(m.awq_clip["ratios"], ratios) and ratios.numel() == 5
    same4((y, best, clip, dmx.ops.awq_clip(plain.weight.detach(), blocks, INT4, G, ratios, return_losses=True)[1]),
          R.clip_ref(plain.weight.detach(), blocks, ratios, 4, True, G, False), "after the fuse")
    assert int(best.max()) > 0
