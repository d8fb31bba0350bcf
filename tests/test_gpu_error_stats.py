"""-m gpu: the error statistics on the device (csrc/error_stats.hip: dmxq_error_stats, dmxq_cast_error) and what is built on them
(ops.error_stats / ops.cast_error through both bindings, CastTo.measure_error, benchmark.compute_error / measure_model_error /
format_sweep).  The checker is tests/_error_ref.py, the float64 restatement pinned to the reference's compute_error by
tests/test_error_stats_host.py, and torch's own expressions; cast_error is checked against error_stats of the library's own cast.

Bounds: count and max_abs_err are exact (bit-equal).  A sum of n non-negative fp64 terms in ANY order is within (n - 1) 2^-53 relative of
the exact sum, so two orders differ by at most n 2^-52 relative: that is the bound on sum_sq_err / sum_sq_ref everywhere below."""
import copy
import ctypes
import math

import pytest
import torch

import _error_ref as R
from _data import make_chunked

pytestmark = pytest.mark.gpu
BINDINGS = ("torch", "ctypes")
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
ERR_UNSUPPORTED = 2


def _i64(t):
    return t.detach().cpu().contiguous().view(torch.int64)


def assert_rows(got, want, n, what):
    """got / want: float64 [4]; count and max bit-equal (NaN == NaN), the sums within n 2^-52 relative (non-finite: the same)"""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    print(what, "got", got.tolist(), "want", want.tolist())
    assert got[3].item() == want[3].item() == float(n), what
    gm, wm = got[2].item(), want[2].item()
    assert (math.isnan(gm) and math.isnan(wm)) or _i64(got[2:3]).item() == _i64(want[2:3] + 0.0).item(), (what, gm, wm)
    for j in (0, 1):
        g, w = got[j].item(), want[j].item()
        if math.isnan(w) or math.isinf(w):
            assert (math.isnan(g) and math.isnan(w)) or g == w, (what, j, g, w)
        else:
            assert abs(g - w) <= R.sum_bound(n) * abs(w), (what, j, g, w, abs(g - w) / max(abs(w), 1e-300))


_BASE = {}


def base(n, seed):
    """n + 1 seeded float32 values on the CPU (one spare element for the offset views)"""
    if (n, seed) not in _BASE:
        _BASE[(n, seed)] = make_chunked("normal", (n + 1,), seed=seed)
    return _BASE[(n, seed)]


# ---------------------------------------------------------------------------------------------------- error_stats
@pytest.mark.parametrize("n", [1, 7, 4096, (1 << 20) + 3, 4096 * 4096])
@pytest.mark.parametrize("dr,dt", [(a, b) for a in (F32, F16, BF16) for b in (F32, F16, BF16)], ids=lambda d: str(d).split(".")[-1])
def test_error_stats_against_the_float64_restatement(dmx, cuda, dr, dt, n):
    r = base(n, 101)[:n].to(dr)
    t = (base(n, 101)[:n] + 0.01 * base(n, 202)[:n]).to(dt)
    want = R.error_row_ref(r, t)
    rd, td = r.to(cuda), t.to(cuda)
    torch_max = (rd - td).float().abs().max().double().cpu()
    assert _i64(torch_max.reshape(1)).item() == _i64(want[2:3]).item()
    for binding in BINDINGS:
        got = dmx.ops.front(binding).error_stats(rd, td)
        assert got.dtype == torch.float64 and got.shape == (4,) and got.device == rd.device
        assert_rows(got, want, n, (binding, dr, dt, n))


@pytest.mark.parametrize("dr,dt", [(BF16, BF16), (F32, F16), (F16, F32)], ids=lambda d: str(d).split(".")[-1])
def test_error_stats_on_views(dmx, cuda, dr, dt):
    """a view offset by one element (not 16-byte aligned: the element-wise kernel), on either side and on both; a non-dense view"""
    n = (1 << 16) + 5
    rb = base(n, 303).to(dr).to(cuda)
    tb = (base(n, 303) + 0.02 * base(n, 404)).to(dt).to(cuda)
    for binding in BINDINGS:
        f = dmx.ops.front(binding)
        for ro, to in ((1, 1), (1, 0), (0, 1)):
            r, t = rb[ro:ro + n], tb[to:to + n]
            assert_rows(f.error_stats(r, t), R.error_row_ref(r, t), n, (binding, "offset", ro, to))
        r2, t2 = rb[:n - 5].reshape(256, 256).t(), tb[:n - 5].reshape(256, 256).t()
        assert_rows(f.error_stats(r2, t2), R.error_row_ref(r2.contiguous(), t2.contiguous()), n - 5, (binding, "transposed"))
        with pytest.raises(ValueError):
            f.error_stats(rb[:8], tb[:9])


@pytest.mark.parametrize("binding", BINDINGS)
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=lambda d: str(d).split(".")[-1])
def test_non_finite_values_follow_the_nan_rule(dmx, cuda, binding, dtype):
    f = dmx.ops.front(binding)
    n = 4096 + 24
    r = base(n, 505)[:n].to(dtype)
    t = (base(n, 505)[:n] * 1.01).to(dtype)
    inf = float("inf")
    for name, edit_r, edit_t in (("nan in test", None, (777, float("nan"))), ("nan in ref", (4100, float("nan")), None),
                                 ("inf against inf", (5, inf), (5, inf)), ("inf against finite", (2049, inf), None),
                                 ("-inf against finite in test", None, (n - 1, -inf))):
        rr, tt = r.clone(), t.clone()
        if edit_r:
            rr[edit_r[0]] = edit_r[1]
        if edit_t:
            tt[edit_t[0]] = edit_t[1]
        want = R.error_row_ref(rr, tt)
        got = f.error_stats(rr.to(cuda), tt.to(cuda))
        assert_rows(got, want, n, (binding, dtype, name))
        g = got.cpu()
        if name in ("nan in test", "nan in ref", "inf against inf"):
            assert math.isnan(g[0].item()) and math.isnan(g[2].item()), name   # any NaN difference: sum_sq_err and max_abs_err are NaN
        else:
            assert g[0].item() == inf and g[2].item() == inf, name


def test_two_calls_give_the_same_bits(dmx, cuda):
    x = make_chunked("normal", (2048, 4096), seed=7).to(BF16).to(cuda)
    y = dmx.CastTo("BFP[8|8]{16}(SN)")(x)
    fmts = ["BFP[8|8]{16}(SN)", "BFP[4|8]{32}(SN)", "FP[1|4|3,7](_N)"]
    for binding in BINDINGS:
        f = dmx.ops.front(binding)
        a, b = f.error_stats(x, y), f.error_stats(x, y)
        assert torch.equal(_i64(a), _i64(b))
        c, d = f.cast_error(x, fmts), f.cast_error(x, fmts)
        assert torch.equal(_i64(c), _i64(d))
    assert torch.equal(_i64(dmx.ops.front("torch").cast_error(x, fmts)), _i64(dmx.ops.front("ctypes").cast_error(x, fmts)))


@pytest.mark.parametrize("binding", BINDINGS)
def test_accumulate_over_batches_equals_the_concatenation(dmx, cuda, binding):
    f = dmx.ops.front(binding)
    sizes = [(1 << 18) + 3, 1 << 12, (1 << 19) + 8]
    rs = [base(n, 600 + i)[:n].to(BF16) * (i + 1) for i, n in enumerate(sizes)]
    ts = [(r.float() * 1.03).to(BF16) for r in rs]
    row = torch.zeros(4, dtype=torch.float64, device=cuda)
    for r, t in zip(rs, ts):
        out = f.error_stats(r.to(cuda), t.to(cuda), out=row, accumulate=True)
        assert out is row
    want = R.error_row_ref(torch.cat(rs), torch.cat(ts))
    assert_rows(row, want, sum(sizes), (binding, "accumulate"))
    with pytest.raises(ValueError):
        f.error_stats(rs[0].to(cuda), ts[0].to(cuda), accumulate=True)   # nothing to merge into
    # cast_error accumulates the same way: two halves of a tensor against the whole
    x = make_chunked("normal", (512, 1024), seed=9).to(cuda)
    fmts = ["BFP[8|8]{64}(SN)", "FP[1|5|2,15](_N)"]
    rows = f.cast_error(x[:256], fmts)
    f.cast_error(x[256:], fmts, out=rows, accumulate=True)
    whole = f.cast_error(x, fmts)
    for k in range(2):
        assert_rows(rows[k], whole[k], x.numel(), (binding, "cast_error accumulate", k))
    # formats the kernel takes on either side of one it does not: the fused rows are gathered, merged and written back
    mixed = ["BFP[8|8]{64}(SN)", dmx.format.MXFP8_E4M3K32, "FP[1|5|2,15](_N)", "BFP[4|8]{32}(SN)"]
    rows = f.cast_error(x[:256], mixed)
    f.cast_error(x[256:], mixed, out=rows, accumulate=True)
    whole = f.cast_error(x, mixed)
    for k in range(4):
        assert_rows(rows[k], whole[k], x.numel(), (binding, "cast_error accumulate, fused rows apart", k))
        assert_rows(whole[k], dmx.ops.error_stats(x, dmx.CastTo(mixed[k]).to(cuda)(x)), x.numel(), (binding, "mixed", k))
    # n == 0: the identity row, or an accumulated row left as it is
    empty = torch.empty(0, dtype=BF16, device=cuda)
    assert f.error_stats(empty, empty).tolist() == [0.0, 0.0, 0.0, 0.0]
    before = row.clone()
    f.error_stats(empty, empty, out=row, accumulate=True)
    assert torch.equal(_i64(before), _i64(row))


def test_error_stats_and_cast_error_capture_into_one_graph(dmx, cuda):
    """no allocation the caching allocator cannot serve from the graph's pool, no host synchronisation: one capture of both calls on a
    single stream, replayed on new data, equals the eager calls bit for bit"""
    xs = [make_chunked("normal", (768, 1024), seed=40 + b).to(BF16).to(cuda) * (1 + b) for b in range(3)]
    c = dmx.CastTo("XP[8,0](CSN)").to(cuda)
    c.enable_calibration(True, dmx.MinMaxObserver, torch.per_tensor_affine)
    c(xs[0])
    c.enable_calibration(False)
    fmts = ["BFP[8|8]{16}(SN)", "FP[1|4|3,7](_N)", ("XP[8,0](CSN)", c.scale, c.zero_point)]
    ref_fmt = dmx.CastTo("BFP[6|8]{32}(SN)")
    x, y = xs[0].clone(), ref_fmt(xs[0])
    e_row = torch.zeros(4, dtype=torch.float64, device=cuda)
    c_rows = torch.zeros(3, 4, dtype=torch.float64, device=cuda)
    dmx.ops.error_stats(x, y, out=e_row)      # eager warm-up
    dmx.ops.cast_error(x, fmts, out=c_rows)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dmx.ops.error_stats(x, y, out=e_row)
        dmx.ops.cast_error(x, fmts, out=c_rows)
    for xb in xs[1:]:
        x.copy_(xb)
        y.copy_(ref_fmt(xb))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_i64(e_row), _i64(dmx.ops.error_stats(xb, ref_fmt(xb))))
        assert torch.equal(_i64(c_rows), _i64(dmx.ops.cast_error(xb, fmts)))


# ---------------------------------------------------------------------------------------------------- cast_error
BFP_LIST = ["BFP[8|8]{16}(SN)", "BFP[4|8]{32}(SN)", "BFP[8|8]{64}(SN)", "BFP[6|8]{16}(_N)", "BFP[8|8]{128}(SN)"]


def _formats(dmx, cuda, x, which):
    """(entries for cast_error, CastTo per entry) -- the FixedPoint ones with a MinMax scale of x"""
    names = {"k1": BFP_LIST[:1], "k4": BFP_LIST[:4], "bfp5": BFP_LIST,
             "k8": BFP_LIST + ["AFLOAT8", "FLOAT16", "INT8"], "elementwise": ["AFLOAT8", "FLOAT16", "INT8", "INT4"]}[which]
    entries, casts = [], []
    for nm in names:
        fmt = getattr(dmx.format, nm) if hasattr(dmx.format, nm) else dmx.Format.from_shorthand(nm)
        c = dmx.CastTo(fmt).to(cuda)
        if isinstance(fmt, dmx.FixedPoint):
            c.enable_calibration(True, dmx.MinMaxObserver, torch.per_tensor_affine)
            c(x)
            c.enable_calibration(False)
            entries.append((fmt, c.scale, c.zero_point))
        else:
            entries.append(fmt)
        casts.append(c)
    return entries, casts


def _c_entry_rc(dmx, x, entries):
    """dmxq_cast_error called directly: its return code says which path ops.cast_error takes for these formats on this tensor"""
    from dmx_compressor_amd import _front
    lib, L = dmx._lib, dmx._lib.lib()
    fmts = [e[0] if isinstance(e, tuple) else e for e in entries]
    arr = (lib.GptqFormat * len(fmts))(*[lib.GptqFormat(*_front.gptq_fields(f)) for f in fmts])
    K = len(fmts)
    scale = torch.cat([e[1].float().reshape(1) if isinstance(e, tuple) else torch.ones(1, device=x.device) for e in entries])
    zp = torch.cat([e[2].long().reshape(1) if isinstance(e, tuple) else torch.zeros(1, dtype=torch.int64, device=x.device) for e in entries])
    stats = torch.zeros(K, 4, dtype=torch.float64, device=x.device)
    nbytes = L.dmxq_error_scratch_bytes(x.numel(), K)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    rc = L.dmxq_cast_error(lib.ptr(x), lib.dtype_code(x.dtype), x.numel() // x.shape[-1], x.shape[-1], ctypes.cast(arr, ctypes.c_void_p), K,
                           lib.ptr(scale), lib.ptr(zp), 0, lib.ptr(stats), lib.ptr(scratch), nbytes, lib.stream_of(x))
    torch.cuda.synchronize()
    return rc, stats


def _loop_shape():
    """more chunks than one round of the largest grid holds, and no multiple of it: every wave of the kernel's grid-stride loop goes
    round more than twice and the trip counts differ (grid <= 8 workgroups per CU, 4 waves, 4 chunks of 512 elements per round)"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per_round = cus * 8 * 4 * 4 * 512
    L = 4096
    rows = -(-5 * per_round // (2 * L)) + 3
    return rows, L


SHAPES = {"4096x4096_bf16": ((4096, 4096), BF16), "1536x768_f32": ((1536, 768), F32), "3x40_f16": ((3, 40), F16), "loop_bf16": (None, BF16)}


@pytest.mark.parametrize("which", ["k1", "k4", "bfp5", "k8", "elementwise"])
@pytest.mark.parametrize("shape_name", list(SHAPES))
def test_cast_error_equals_error_stats_of_the_cast(dmx, cuda, shape_name, which):
    shape, dtype = SHAPES[shape_name]
    shape = shape or _loop_shape()
    x = (make_chunked("normal", shape, seed=len(shape_name) + 3) * 0.7).to(dtype).to(cuda)
    n, L = x.numel(), shape[-1]
    entries, casts = _formats(dmx, cuda, x, which)
    fused = L % 8 == 0 and all(L % e.block_size == 0 for e in entries if isinstance(e, dmx.BlockFloatingPoint))
    rc, direct = _c_entry_rc(dmx, x, entries)
    assert rc == (0 if fused else ERR_UNSUPPORTED), (shape_name, which, rc)
    want = [dmx.ops.error_stats(x, c(x)) for c in casts]
    for binding in BINDINGS:
        got = dmx.ops.front(binding).cast_error(x, entries)
        assert got.shape == (len(entries), 4) and got.dtype == torch.float64
        for k in range(len(entries)):
            assert_rows(got[k], want[k], n, (binding, shape_name, which, k, repr(casts[k].format)))
        if fused:
            # the C entry's own rows: the fused kernel is what answered.  (A format native to x's dtype -- FLOAT16 on a float16 tensor --
            # is the identity, which the front answers by error_stats(x, x): its sum_sq_ref may be summed in another order.)
            kept = [k for k, c in enumerate(casts) if not (isinstance(c.format, dmx.FloatingPoint) and c.format.native_of() == x.dtype)]
            assert len(kept) >= len(casts) - 1 and torch.equal(_i64(got[kept]), _i64(direct[kept]))
    # CastTo.measure_error: the row of the cast's own format, block_dim and scale / zero point
    for k, c in enumerate(casts):
        assert_rows(c.measure_error(x), want[k], n, ("measure_error", shape_name, which, k))


@pytest.mark.parametrize("binding", BINDINGS)
def test_cast_error_fallbacks_answer_under_the_same_contract(dmx, cuda, binding):
    f = dmx.ops.front(binding)
    x = (make_chunked("normal", (64, 1536), seed=77) * 0.9).to(BF16).to(cuda)

    def check(x, entries, block_dim, what):
        got = f.cast_error(x, entries, block_dim=block_dim)
        for k, e in enumerate(entries):
            y = dmx.CastTo(e, block_dim=block_dim).to(cuda)(x)
            assert_rows(got[k], dmx.ops.error_stats(x, y), x.numel(), (binding, what, k))

    check(x, ["BFP[8|8]{16}(SN)", "BFP[4|8]{32}(SN)"], 0, "block_dim 0")
    check(x, [dmx.format.MXFP8_E4M3K32, dmx.format.SBFP12_16, "BFP[8|8]{16}(SN)"], -1, "mxfp / sbfp next to a fused format")
    check(x, ["BFP[8|8]{16}(SU)", "BFP[8|8]{16}(SD)"], -1, "up / down rounding")
    x1500 = (make_chunked("normal", (48, 1500), seed=78)).to(F16).to(cuda)
    rc, _ = _c_entry_rc(dmx, x1500, [dmx.Format.from_shorthand("BFP[8|8]{16}(SN)")])
    assert rc == ERR_UNSUPPORTED
    check(x1500, ["BFP[8|8]{16}(SN)", "FP[1|4|3,7](_N)"], -1, "L = 1500, ragged blocks of 16")
    eleven = ["BFP[%d|8]{%d}(SN)" % (p, b) for p, b in ((8, 16), (8, 32), (8, 64), (8, 128), (6, 16), (6, 32), (6, 64), (4, 16), (4, 32))] \
        + ["FP[1|4|3,7](_N)", "FP[1|5|2,15](_N)"]
    check(x, eleven, -1, "K = 11 in groups")
    with pytest.raises(NotImplementedError):
        f.cast_error(x, ["BFP[8|8]{16}(SS)"])
    with pytest.raises(NotImplementedError):
        f.cast_error(x, ["BFP[8|8]{16}(SN)", "FP[1|4|3,7](_S)"])


@pytest.mark.parametrize("how", ["per_channel", "per_group"])
def test_measure_error_of_a_per_channel_or_per_group_fixed_point_cast(dmx, cuda, how):
    """one scale per output channel / per group of 16 rows: not a cast_error format -- the cast's own launch, then error_stats"""
    W = (make_chunked("normal", (48, 40), seed=8) * torch.linspace(0.1, 3.0, 48)[:, None]).to(cuda)
    c = dmx.CastTo(format=dmx.format.INT8, ch_axis=0).to(cuda)
    if how == "per_channel":
        c.enable_calibration(True, dmx.MinMaxObserver, torch.per_channel_symmetric, ch_axis=0)
    else:
        c.enable_calibration(True, dmx.MinMaxObserver, torch.per_tensor_symmetric, group_size=16, ch_axis=0)
    c(W)
    c.enable_calibration(False)
    assert c.scale.numel() == (48 if how == "per_channel" else 3)
    y = c(W)
    got = c.measure_error(W)
    assert_rows(got, R.error_row_ref(W.cpu(), y.cpu()), W.numel(), ("measure_error", how))
    assert torch.equal(_i64(got), _i64(dmx.ops.error_stats(W, y)))
    # nearest rounding and nothing clipped (|x / scale| <= 127): at most half a step, plus the fp32 rounding of x / scale (<= 127 * 2^-24
    # of a step) and of the product back
    assert 0 < got[0].item() and got[2].item() <= c.scale.max().item() * (0.5 + 127 * 2.0 ** -22)
    assert (c._flag("fake_quant_enabled"), c._flag("observer_enabled")) == (True, False)


# ---------------------------------------------------------------------------------------------------- modules and models
def _toy(dmx, cuda, seed=5):
    m = torch.nn.Sequential(dmx.nn.Linear(256, 512), dmx.nn.Linear(512, 128))
    with torch.no_grad():
        for i, lin in enumerate(m):
            lin.weight.copy_(make_chunked("normal", tuple(lin.weight.shape), seed=seed + i) * 0.05)
            lin.bias.copy_(make_chunked("normal", tuple(lin.bias.shape), seed=seed + 10 + i) * 0.01)
    return m.to(cuda)


def test_measure_error_and_format_sweep_on_a_toy_model(dmx, cuda):
    m = _toy(dmx, cuda)
    dmx.configure_model(m, *dmx.config_rules.BASIC)
    f8, f4 = "BFP[8|8]{64}(SN)", "BFP[4|8]{64}(SN)"
    sweep = dmx.format_sweep(m, [f8, f4])
    assert list(sweep) == ["0", "1"] and all(list(v) == [f8, f4] for v in sweep.values())
    for name, lin in m.named_children():
        w = lin.weight.detach()
        rows = dmx.ops.cast_error(w, [f8, f4], block_dim=lin.weight_cast.block_dim)
        assert torch.equal(_i64(lin.weight_cast.measure_error(w)), _i64(dmx.ops.cast_error(w, [lin.weight_cast.format], block_dim=lin.weight_cast.block_dim)[0]))
        assert torch.equal(_i64(lin.weight_cast.measure_error(w)), _i64(rows[0]))   # (BASIC's weight format is BFP16_64 = f8)
        db = (10.0 * torch.log10(rows[:, 1] / rows[:, 0])).cpu().tolist()
        assert sweep[name][f8] == db[0] and sweep[name][f4] == db[1]
        r = rows.cpu()
        print(name, "sqnr dB", db, "rows", r.tolist())
        # the 8-bit grid refines the 4-bit one and clips later: its error is no larger element by element, so in every statistic
        assert r[0, 0] <= r[1, 0] and r[0, 2] <= r[1, 2] and r[0, 1] == r[1, 1] and r[0, 3] == r[1, 3] == w.numel()
        assert db[0] >= db[1]
    t = dmx.format_sweep(m[0].weight.detach(), [f8, f4])
    assert t == sweep["0"]
    flags = [(c._flag("fake_quant_enabled"), c._flag("observer_enabled")) for c in m.modules() if isinstance(c, dmx.CastTo)]
    assert all(fl == (True, False) for fl in flags)   # measuring touches neither switch


def test_measure_model_error_against_hand_captured_tensors(dmx, cuda):
    ref = _toy(dmx, cuda)                       # BASELINE: every cast is SAME
    dmx.configure_model(ref, *dmx.config_rules.BASELINE)
    test = copy.deepcopy(ref)
    dmx.configure_model(test, *dmx.config_rules.BASIC)
    x = make_chunked("normal", (32, 256), seed=91).to(cuda)

    def runner(model):
        return model(x)

    report = dmx.measure_model_error(ref, {"basic": test}, runner)
    assert list(report) == ["basic"] and set(report["basic"]) == {"cumulative", "per_layer", "input", "final_output_error"}
    r = report["basic"]
    print(report.table)
    assert isinstance(report.table, str) and "basic(per_layer)" in report.table and "final_output_error" in report.table
    for kind in ("cumulative", "per_layer", "input"):
        assert list(r[kind]) == ["0", "1"] and all(set(v) == {"mse", "maxdelta"} for v in r[kind].values())
    assert r["input"]["0"] == {"mse": 0.0, "maxdelta": 0.0}       # both models see the same x
    assert r["per_layer"]["0"] == r["cumulative"]["0"]            # ... so the first layer's own error is all there is
    assert r["cumulative"]["1"]["mse"] > 0 and r["input"]["1"] == r["cumulative"]["0"]   # layer 1's input is layer 0's output

    # by hand: forward hooks on both models, compute_error on what they saw
    def capture(model):
        seen, hooks = {}, []
        for name, mod in model.named_children():
            hooks.append(mod.register_forward_hook(lambda _m, a, kw, out, name=name: seen.__setitem__(name, ((a, kw), out)), with_kwargs=True))
        with torch.no_grad():
            final = model(x)
        for h in hooks:
            h.remove()
        return seen, final

    seen_ref, final_ref = capture(ref)
    seen_test, final_test = capture(test)
    assert r["final_output_error"] == dmx.compute_error(final_test, final_ref)
    for name, mod in test.named_children():
        assert r["input"][name] == dmx.compute_error(seen_ref[name][0], seen_test[name][0]), name
        assert r["cumulative"][name] == dmx.compute_error(seen_ref[name][1], seen_test[name][1]), name
        with torch.no_grad():
            clean = mod(*seen_ref[name][0][0], **seen_ref[name][0][1])
        assert r["per_layer"][name] == dmx.compute_error(seen_ref[name][1], clean), name
    assert all(len(mod._forward_hooks) == 0 for mod in list(ref) + list(test))
    # GPU tensors and their CPU copies: the same meaning (mse up to the order and width of the sums)
    a, b = seen_ref["1"][1], seen_test["1"][1]
    g, c = dmx.compute_error([a, {"k": a}], [b, {"k": b}]), dmx.compute_error([a.cpu(), {"k": a.cpu()}], [b.cpu(), {"k": b.cpu()}])
    assert g["maxdelta"] == c["maxdelta"] and abs(g["mse"] - c["mse"]) <= a.numel() * 2.0 ** -24 * c["mse"]


def test_compute_error_takes_tensors_of_any_dtype(dmx, cuda):
    """token ids, position ids, masks and float64 next to the float tensors: the reference's expressions take them all, and so does a
    collection on the GPU (the kernel's three dtypes through ops.error_stats, the others through torch on the device)"""
    ids = torch.arange(0, 4096, dtype=torch.int64).reshape(8, 512) % 97
    ids2 = ids.clone()
    ids2[3, 100] += 5
    ids2[7, 511] -= 9
    f = make_chunked("normal", (64, 96), seed=31)
    g = f + 0.01 * make_chunked("normal", (64, 96), seed=32)
    mask, mask2 = ids % 3 == 0, ids % 6 == 0
    a = {"ids": ids, "h": (f.to(BF16), f.double()), "mask": mask, "pos": [ids.to(torch.int32)], "skipped": "text"}
    b = {"ids": ids2, "h": (g.to(BF16), g.double()), "mask": mask2, "pos": [ids2.to(torch.int32)], "skipped": None}

    def to_gpu(c):
        return {k: (type(v)(t.to(cuda) for t in v) if isinstance(v, (tuple, list)) else v.to(cuda) if isinstance(v, torch.Tensor) else v)
                for k, v in c.items()}

    got, want = dmx.compute_error(to_gpu(a), to_gpu(b)), dmx.compute_error(a, b)
    print("any dtype", got, want)
    assert want["maxdelta"] == 9.0 and got["maxdelta"] == want["maxdelta"]
    # the int pairs' squares are small integers (exact in any order); the float pairs as in the test above
    assert abs(got["mse"] - want["mse"]) <= f.numel() * 2.0 ** -24 * want["mse"]
    assert dmx.compute_maxdelta_error([ids.to(cuda)], [ids2.to(cuda)]) == 9.0
    assert dmx.compute_mse_error([ids.to(cuda)], [ids2.to(cuda)]) == (25 + 81) / 4096
    assert dmx.compute_error(mask.to(cuda), mask2.to(cuda)) == dmx.compute_error(mask.float(), mask2.float())


def test_measure_model_error_on_a_model_that_starts_with_an_embedding(dmx, cuda):
    """by default every DmxModule is visited, so the recorded inputs of an Embedding -- int64 token ids -- are compared too"""
    def model():
        m = torch.nn.Sequential(dmx.nn.Embedding(97, 256), dmx.nn.Linear(256, 128))
        with torch.no_grad():
            m[0].weight.copy_(make_chunked("normal", (97, 256), seed=61) * 0.5)
            m[1].weight.copy_(make_chunked("normal", (128, 256), seed=62) * 0.05)
            m[1].bias.copy_(make_chunked("normal", (128,), seed=63) * 0.01)
        return m.to(cuda)

    ref = model()
    dmx.configure_model(ref, *dmx.config_rules.BASELINE)
    test = copy.deepcopy(ref)
    dmx.configure_model(test, *dmx.config_rules.BASIC)
    ids = (torch.arange(0, 32 * 16, dtype=torch.int64).reshape(32, 16) * 7 % 97).to(cuda)
    report = dmx.measure_model_error(ref, {"basic": test}, lambda m: m(ids))
    r = report["basic"]
    print(report.table)
    assert list(r["input"]) == ["0", "1"]
    assert r["input"]["0"] == {"mse": 0.0, "maxdelta": 0.0}       # the same ids
    assert r["per_layer"]["0"] == r["cumulative"]["0"] and r["input"]["1"] == r["cumulative"]["0"]
    with torch.no_grad():
        e_ref, e_test = ref[0](ids), test[0](ids)
        assert r["cumulative"]["0"] == dmx.compute_error(e_ref, e_test)
        assert r["per_layer"]["1"] == dmx.compute_error(ref[1](e_ref), test[1](e_ref))
        assert r["final_output_error"] == dmx.compute_error(test(ids), ref(ids))
    assert r["final_output_error"]["mse"] > 0
