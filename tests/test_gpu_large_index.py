"""-m gpu: every kernel's 64-bit index path, on tensors of more than 2^31 elements (case table, period rule and what is left out on
purpose -- bfp_cols ColsIdx.small == 0, hist_observer.hip:98 narrow == false, stream.hpp:452, DMXQ_INPUT_HYPERNET_TILED, the refusing side
of bfp.hip:387: tens of GiB or another process each -- in tests/_large_cases.py).

One harness over the table:
  * the input is generated on the device, random and without a period, with a NaN, an Inf, a denormal block and an all-zero block
    planted in rows beyond element 2^31;
  * the full-size call runs FIRST (no stale memory can hold its answer); then every chunk of fewer than 2^31 elements -- the 32-bit
    form that the rest of the suite pins to the oracle -- runs on a contiguous aligned view and must reproduce its rows of the full
    output bit for bit: EVERY element of the output is compared;
  * two windows, 64 rows straddling element 2^31 and the last 64 rows, are checked against the CPU oracle as the op's own tests do it,
    so that the chain does not rest on the library alone;
  * reductions are compared with their per-chunk results combined on the host (min of mins, max of maxes, int64 sums), exactly;
  * every case runs again just under the boundary (the 32-bit forms at their largest values).
The primary input of a case is kept for the next case of the same shape (one slot, freed at the end of the module); every test frees
everything else, empties the cache and skips -- with the reason -- only when less device memory is free than the case needs."""
import ctypes
import math

import pytest
import torch

import _large_cases as LC
from _data import err_in_ulps, mismatches_nan_aware, outside_cast_bracket

pytestmark = pytest.mark.gpu
F = torch.nn.functional
BF16, F32 = torch.bfloat16, torch.float32
INT8 = "XP[8,0](CSN)"
FP16_FMT, E4M3_FMT = "FP[1|5|10,15](FN)", "FP[1|4|3,7](_N)"
TAIL = 1 << 20


# ------------------------------------------------------------------------------------------------ plumbing
@pytest.fixture(autouse=True)
def _stop_the_session_after_a_gpu_fault():
    """a HIP error after a test (an illegal access is sticky) ends the session: nothing more is started on a faulted device"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # pragma: no cover
        pytest.exit(f"GPU fault, stopping the session: {e}", returncode=3)


_SLOT = {}


@pytest.fixture(scope="module", autouse=True)
def _free_the_input_slot():
    yield
    _SLOT.clear()
    torch.cuda.empty_cache()


def _seed(c):
    return sum(ord(ch) for ch in c.kind + c.dtype) + c.shape[-1]


def _need(c):
    _SLOT_key = _key(c)
    if _SLOT and next(iter(_SLOT)) != _SLOT_key:
        _SLOT.clear()
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    held = sum(t.numel() * t.element_size() for t in _SLOT.values())
    need = LC.peak_bytes(c) - held
    if free < need:
        pytest.skip(f"{c.name}: needs {need / LC.GIB:.1f} GiB of device memory, {free / LC.GIB:.1f} GiB free")


def _key(c):
    full = LC.BY_NAME.get(c.name.replace("_under", "")) or LC.SPECIAL_BY_NAME[c.name.replace("_under", "")]
    return (c.kind, full.shape, c.dtype, c.specials)


def _primary(c, dev):
    """the case's first big input: the full-size tensor of its shape class (a twin takes the leading rows of it)"""
    key = _key(c)
    if key not in _SLOT:
        _SLOT.clear()
        torch.cuda.empty_cache()
        full = c._replace(shape=key[1])
        x = LC.device_input(c.kind, key[1], LC.torch_dtype(c.dtype), _seed(c), dev)
        if c.specials:
            LC.plant_specials(x, full)
        _SLOT[key] = x
    return _SLOT[key][:c.shape[0]]


def _second(c, kind, dtype, dev, salt=1):
    return LC.device_input(kind, c.shape, dtype, _seed(c) + 1000 * salt, dev)


def _cpu_gen(seed):
    return torch.Generator().manual_seed(seed)


def _fmt(dmx, s):
    return dmx.Format.from_shorthand(s)


def _cpu_cast(O, f):
    return lambda x: O.floating_point_cast(x, f.mantissa, f.exponent, f.bias, f.flush_subnormal).to(x.dtype)


def _window_views(c, ts, w):
    if len(w) == 3:
        r, c0, n = w
        return [t[r:r + 1, c0:c0 + n] for t in ts]
    return [t[w[0]:w[1]] for t in ts]


def _window_aux(c, aux, w):
    """the per-column / per-row-group tensors of `aux` cut to a window (per-column ones only for a column window)"""
    out = dict(aux)
    if len(w) == 3:
        for k, v in aux.items():
            if torch.is_tensor(v) and v.dim() == 1 and v.shape[0] == c.shape[-1]:
                out[k] = v[w[1]:w[1] + w[2]]
        return out
    return OPS[c.op].cut(c, aux, w[0], w[1])


class Op:
    """one op of the table: inputs(c, dev) -> (big tensors cut along dim 0, small tensors); run -> tuple of big outputs;
    cut: the small tensors that belong to rows [a, b); check: one oracle window (CPU tensors)"""
    def inputs(self, c, dev, dmx):
        return [_primary(c, dev)], {}

    def cut(self, c, aux, a, b):
        return aux

    def check(self, O, dmx, c, xs, aux, got):
        want = self.ref(O, dmx, c, xs, aux)
        for k, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape, (c.name, k, g.shape, w.shape)
            assert mismatches_nan_aware(g, w.to(g.dtype) if g.is_floating_point() else w) == 0, (c.name, "oracle window, output", k)


class FixedQdq(Op):
    def inputs(self, c, dev, dmx):
        ax = c.p["ch_axis"] % len(c.shape)
        G = c.shape[ax] // (c.p["gs"] or 1)
        g = _cpu_gen(G)
        sc = (torch.rand(G, generator=g) * 0.2 + 0.01)
        zp = torch.randint(-9, 10, (G,), generator=g)
        return [_primary(c, dev)], {"scale": sc.to(dev), "zp": zp.to(dev)}

    def cut(self, c, aux, a, b):
        if c.p["ch_axis"] != 0:
            return aux
        gs = c.p["gs"] or 1
        assert a % gs == 0
        return {"scale": aux["scale"][a // gs:-(-b // gs)], "zp": aux["zp"][a // gs:-(-b // gs)]}

    def run(self, ops, c, xs, aux):
        return (ops.fixed_qdq(xs[0], 8, 0, True, True, scale=aux["scale"], zero_point=aux["zp"], ch_axis=c.p["ch_axis"], group_size=c.p["gs"]),)

    def ref(self, O, dmx, c, xs, aux):
        return (O.fixed_point_affine_cast(xs[0], 8, 0, True, True, aux["scale"], aux["zp"], ch_axis=c.p["ch_axis"], group_size=c.p["gs"]).to(xs[0].dtype),)


class ScaleChannels(Op):
    def inputs(self, c, dev, dmx):
        C = c.shape[c.p["ch_axis"]]
        return [_primary(c, dev)], {"scale": (torch.rand(C, generator=_cpu_gen(C)) + 0.5).to(dev)}

    def run(self, ops, c, xs, aux):
        return (ops.scale_channels(xs[0], aux["scale"], c.p["ch_axis"], c.p["divide"], out_dtype=LC.torch_dtype(c.out)),)

    def ref(self, O, dmx, c, xs, aux):
        sh = [1] * xs[0].dim()
        sh[c.p["ch_axis"]] = -1
        s = aux["scale"].view(sh)
        return ((xs[0].float() / s if c.p["divide"] else xs[0].float() * s).to(LC.torch_dtype(c.out)),)


class WeightHypernet(Op):
    def inputs(self, c, dev, dmx):
        xs = [_primary(c, dev)]
        if c.p["M"]:
            xs.append(_second(c, "uniform", LC.torch_dtype(c.p["score"]), dev))
        aux = {"sq": (torch.rand(c.shape[1], generator=_cpu_gen(3)) * 3 + 0.1).to(dev)} if c.p["scale"] else {}
        return xs, aux

    def run(self, ops, c, xs, aux):
        p = c.p
        y = ops.weight_hypernet(xs[0], 8, p["B"], True, xs[1] if p["M"] else None, p["K"], p["M"], aux.get("sq"), out_dtype=LC.torch_dtype(c.out))
        assert y is not None, c.name
        return (y,)

    def ref(self, O, dmx, c, xs, aux):      # the reference's dtype flow, as tests/test_gpu_round4.py states it
        p, x = c.p, xs[0]
        if p["M"]:
            x = O.sparsify(x, xs[1], p["K"], p["M"])
        if p["scale"]:
            x = (x.float() * aux["sq"]).to(x.dtype)
        return (O.bfp_cast(x, 8, p["B"], -1, True).to(x.dtype),)


class NmSparsify(Op):
    def inputs(self, c, dev, dmx):
        return [_primary(c, dev), _second(c, "uniform", LC.torch_dtype(c.dtype), dev)], {}

    def run(self, ops, c, xs, aux):
        return (ops.nm_sparsify(xs[0], xs[1], c.p["K"], c.p["M"]),)

    def ref(self, O, dmx, c, xs, aux):
        return (O.sparsify(xs[0], xs[1], c.p["K"], c.p["M"]),)


class NmMask(Op):
    def run(self, ops, c, xs, aux):
        return (ops.nm_mask(xs[0], c.p["K"], c.p["M"]),)

    def ref(self, O, dmx, c, xs, aux):
        return (O.nm_mask(xs[0], c.p["K"], c.p["M"]),)


class InputHypernet(Op):
    def inputs(self, c, dev, dmx):
        L = c.shape[1]
        sq = torch.empty(L)
        for s in range(0, L, 1 << 22):      # (rows of 50 M columns: the scales in pieces too)
            sq[s:s + (1 << 22)] = torch.rand(min(1 << 22, L - s), generator=_cpu_gen(s + 5)) * 3 + 0.1
        return [_primary(c, dev)], {"sq": sq.to(dev)}

    def run(self, ops, c, xs, aux):
        y = ops.input_hypernet(xs[0], aux["sq"], 8, c.p["B"], True)
        assert y is not None and y.dtype == F32, c.name
        return (y,)

    def ref(self, O, dmx, c, xs, aux):
        return (O.bfp_cast(xs[0].float() / aux["sq"], 8, c.p["B"], -1, True),)


class Sbfp(Op):
    def run(self, ops, c, xs, aux):
        return (ops.sbfp_qdq(xs[0], 8, c.p["B"], 2, 5, 15, True, True, True, -1),)

    def ref(self, O, dmx, c, xs, aux):
        return (O.sbfp_cast(xs[0], 8, c.p["B"], 2, 5, 15, True, True, True, -1).to(xs[0].dtype),)


class Mxfp(Op):
    def run(self, ops, c, xs, aux):
        return (ops.mxfp_qdq(xs[0], 3, 4, c.p["B"]),)

    def ref(self, O, dmx, c, xs, aux):
        return (O.mxfp_cast(xs[0], 3, 4, c.p["B"]).to(xs[0].dtype),)


class Bfp(Op):
    def run(self, ops, c, xs, aux):
        return (ops.bfp_qdq(xs[0], 8, c.p["B"]),)

    def ref(self, O, dmx, c, xs, aux):
        return (O.bfp_cast(xs[0], 8, c.p["B"]).to(xs[0].dtype),)


class FloatQdq(Op):
    def run(self, ops, c, xs, aux):
        return (ops.float_qdq(xs[0], 3, 4, 7, False),)

    def ref(self, O, dmx, c, xs, aux):
        return (O.floating_point_cast(xs[0], 3, 4, 7, False).to(xs[0].dtype),)


class BfpPack(Op):
    def run(self, ops, c, xs, aux):
        mant, exps = ops.bfp_pack(xs[0], 8, c.p["B"], True)
        return (mant, exps, ops.bfp_unpack(mant, exps, 8, c.p["B"], xs[0].dtype))

    def ref(self, O, dmx, c, xs, aux):
        mant, exps = O.bfp_pack(xs[0], 8, c.p["B"], True)
        return (mant, exps, O.bfp_cast(xs[0], 8, c.p["B"]).to(xs[0].dtype))


class DynamicFixed(Op):
    def run(self, ops, c, xs, aux):
        return (ops.dynamic_fixed_qdq(xs[0], INT8, c.p["granularity"], c.p["gs"]),)

    def ref(self, O, dmx, c, xs, aux):
        from _dynamic_ref import dynamic_ref
        S = c.p["gs"] or xs[0].shape[-1]
        return (dynamic_ref(O, xs[0], 8, True, S, False)[0],)


class HadamardQdq(Op):
    def run(self, ops, c, xs, aux):
        return (ops.hadamard_qdq(xs[0], c.p["H"], "BFP[8|8]{%d}(SN)" % c.p["B"]),)

    def ref(self, O, dmx, c, xs, aux):
        from _hadamard_ref import rotated_cast_ref
        return (rotated_cast_ref(xs[0], c.p["H"], lambda r: O.bfp_cast(r, 8, c.p["B"]), True, xs[0].dtype),)


class RowFunction(Op):
    """softmax / layernorm / rmsnorm: the tolerance of the op's own test (1 ulp of a 16-bit output against float64 rounded once)"""
    def __init__(self, kind):
        self.kind = kind

    def inputs(self, c, dev, dmx):
        L, dt = c.shape[1], LC.torch_dtype(c.dtype)
        w = (torch.randn(L, generator=_cpu_gen(12)) * 0.1 + 1).to(dt).to(dev)
        b = (torch.randn(L, generator=_cpu_gen(13)) * 0.1).to(dt).to(dev)
        return [_primary(c, dev)], {"w": w, "b": b}

    def run(self, ops, c, xs, aux):
        L = c.shape[1]
        if self.kind == "softmax":
            return (ops.softmax(xs[0], -1),)
        if self.kind == "layernorm":
            return (ops.layernorm(xs[0], (L,), aux["w"], aux["b"], 1e-5),)
        return (ops.rmsnorm(xs[0], (L,), aux["w"], 1e-6),)

    def check(self, O, dmx, c, xs, aux, got):
        x, L, dt = xs[0], c.shape[1], xs[0].dtype
        xd = x.double()
        if self.kind == "softmax":
            assert err_in_ulps(got[0], F.softmax(xd, -1), dt) <= 1.0, c.name
        elif self.kind == "layernorm":
            w, b = aux["w"].double(), aux["b"].double()
            truth = F.layer_norm(xd, (L,), w, b, 1e-5)
            mu, rstd = xd.mean(-1, keepdim=True), (xd.var(-1, unbiased=False, keepdim=True) + 1e-5).rsqrt()
            floor = (xd.abs().amax(-1, keepdim=True) + mu.abs()) * rstd * w.abs() + b.abs()
            assert err_in_ulps(got[0], truth, dt, floor=floor) <= 1.0, c.name
        else:
            assert err_in_ulps(got[0], F.rms_norm(xd, (L,), aux["w"].double(), 1e-6), dt) <= 1.0, c.name


class UnaryCast(Op):
    def run(self, ops, c, xs, aux):
        f = _fmt(aux["dmx"], FP16_FMT)
        y = ops.unary_cast(xs[0], "gelu", f, f)
        assert y is not None
        return (y,)

    def inputs(self, c, dev, dmx):
        return [_primary(c, dev)], {"dmx": dmx}

    def check(self, O, dmx, c, xs, aux, got):     # the contract of tests/test_gpu_act_cast.py test_unary_cast_contract
        f = _fmt(dmx, FP16_FMT)
        cin = _cpu_cast(O, f)(xs[0])
        n_ulp = 2 if xs[0].dtype == F32 else 1
        assert outside_cast_bracket(got[0], F.gelu(cin.double()), _cpu_cast(O, f), xs[0].dtype, n_ulp, cin.double().abs() / 2) == 0, c.name


class Lut16(Op):
    def inputs(self, c, dev, dmx):
        x = _primary(c, dev)
        return [x], {"table": dmx.ops.unary_cast_table(x[:1], "gelu")}

    def run(self, ops, c, xs, aux):
        y = ops.lut16_apply(xs[0], aux["table"])
        assert y is not None
        return (y,)

    def ref(self, O, dmx, c, xs, aux):
        return (aux["table"].view(xs[0].dtype)[xs[0].contiguous().view(torch.int16).long() & 0xFFFF],)


class BinaryCast(Op):
    def inputs(self, c, dev, dmx):
        return [_primary(c, dev), _second(c, "normal", LC.torch_dtype(c.dtype), dev)], {"dmx": dmx}

    def run(self, ops, c, xs, aux):
        f = _fmt(aux["dmx"], FP16_FMT)
        y = ops.binary_cast(xs[0], xs[1], "add", f, f, f)
        assert y is not None
        return (y,)

    def ref(self, O, dmx, c, xs, aux):
        cast = _cpu_cast(O, _fmt(dmx, FP16_FMT))
        return (cast(cast(xs[0]) + cast(xs[1])),)


class ReluCast(Op):
    def inputs(self, c, dev, dmx):
        return [_primary(c, dev)], {"dmx": dmx}

    def run(self, ops, c, xs, aux):
        f = _fmt(aux["dmx"], FP16_FMT)
        y = ops.relu_cast(xs[0], f, f)
        assert y is not None
        return (y,)

    def ref(self, O, dmx, c, xs, aux):
        cast = _cpu_cast(O, _fmt(dmx, FP16_FMT))
        return (cast(torch.relu(cast(xs[0]))),)


OPS = {"fixed_qdq": FixedQdq(), "scale_channels": ScaleChannels(), "weight_hypernet": WeightHypernet(), "nm_sparsify": NmSparsify(),
       "nm_mask": NmMask(), "input_hypernet": InputHypernet(), "sbfp_qdq": Sbfp(), "mxfp_qdq": Mxfp(), "bfp_qdq": Bfp(), "float_qdq": FloatQdq(),
       "bfp_pack": BfpPack(), "dynamic_fixed_qdq": DynamicFixed(), "hadamard_qdq": HadamardQdq(), "softmax": RowFunction("softmax"),
       "layernorm": RowFunction("layernorm"), "rmsnorm": RowFunction("rmsnorm"), "unary_cast": UnaryCast(), "lut16_apply": Lut16(),
       "binary_cast": BinaryCast(), "relu_cast": ReluCast()}


def _cpu(v):
    return v.cpu() if torch.is_tensor(v) else v


def run_case(dmx, O, dev, c):
    """full-size call first, then every chunk bit for bit, then the two oracle windows"""
    op = OPS[c.op]
    xs, aux = op.inputs(c, dev, dmx)
    full = op.run(dmx.ops, c, xs, aux)
    assert all(f.shape[0] == c.shape[0] and f.is_contiguous() for f in full), c.name
    LC.check_chunks(c, lambda views, ab: op.run(dmx.ops, c, views, op.cut(c, aux, *ab)), xs, full)
    seen = set()
    for w in LC.windows(c):
        if w in seen:
            continue
        seen.add(w)
        xw = [v.cpu() for v in _window_views(c, xs, w)]
        aw = {k: _cpu(v) for k, v in _window_aux(c, aux, w).items()}
        got = [v.cpu() for v in _window_views(c, full, w)]
        op.check(O, dmx, c, xw, aw, got)
    del xs, aux, full


def _ordered(cases):
    """cases of one input class next to each other: the input slot is generated once per class"""
    return sorted(cases, key=lambda c: (c.kind, c.shape[1:], c.dtype, c.specials, "_under" in c.name))


TABLE = _ordered(LC.CASES + [LC.under(c) for c in LC.CASES if c.twin])


@pytest.mark.parametrize("c", TABLE, ids=lambda c: c.name)
def test_full_size_call_equals_its_chunks_and_the_oracle(dmx, cuda, oracle, c):
    _need(c)
    try:
        run_case(dmx, oracle, cuda, c)
    finally:
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ rope: the refusal and the largest accepted size
def _sp(name, twin):
    c = LC.SPECIAL_BY_NAME[name]
    return LC.under(c) if twin else c


@pytest.mark.parametrize("twin", [False, True], ids=["full", "under"])
def test_rope_refuses_two_to_the_31_elements_and_runs_just_under(dmx, cuda, twin):
    """rope.hip:87: 2^31 elements and more are refused (ops.rope returns None, the caller keeps torch's own ops); the largest whole batch
    under it runs with FastDiv31 numerators at their largest and equals its chunks and torch's own formula"""
    c = _sp("rope_refusal", twin)
    _need(c)
    x = _primary(c, cuda)
    B, H, S, D = x.shape
    g = torch.Generator(device=cuda).manual_seed(4)
    cos = torch.randn(LC.SPECIAL_BY_NAME["rope_refusal"].shape[0], S, D, generator=g, device=cuda).to(BF16)[:B]
    sin = torch.randn(LC.SPECIAL_BY_NAME["rope_refusal"].shape[0], S, D, generator=g, device=cuda).to(BF16)[:B]
    try:
        full = dmx.ops.rope(x, cos, sin, 1)
        if not twin:
            assert x.numel() >= LC.TWO31 and full is None
            return
        assert x.numel() < LC.TWO31 and full is not None
        LC.check_chunks(c, lambda v, ab: (dmx.ops.rope(v[0], cos[ab[0]:ab[1]], sin[ab[0]:ab[1]], 1),), [x], (full,), None)
        for b, h in ((0, 0), (B - 1, H - 1)):
            xc, cc, sc = x[b, h].cpu(), cos[b].cpu(), sin[b].cpu()
            rot = torch.cat((-xc[..., D // 2:], xc[..., :D // 2]), dim=-1)
            assert mismatches_nan_aware(full[b, h], (xc * cc) + (rot * sc)) == 0, (b, h)
    finally:
        del x, cos, sin
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ reductions
def _combine_minmax(parts, cat):
    if cat:
        return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    mn, mx = parts[0]
    for a, b in parts[1:]:
        mn, mx = torch.minimum(mn, a), torch.maximum(mx, b)
    return mn, mx


@pytest.mark.parametrize("twin", [False, True], ids=["full", "under"])
@pytest.mark.parametrize("name", ["channel_maxabs_plane", "channel_maxabs_lastdim", "channel_maxabs_axis1", "group_minmax_axis1", "group_minmax_rows"])
def test_channel_reductions_equal_their_chunks_combined(dmx, cuda, name, twin):
    """max of maxes / min of mins over the chunks (channels along dim 0: the chunks' results joined), bit for bit.  channel_maxabs_plane
    has plane = C * inner >= 2^31 (reduce.hip:486)."""
    c = _sp(name, twin)
    _need(c)
    x = _primary(c, cuda)
    ax, cat = c.p["ch_axis"], c.p["ch_axis"] == 0
    try:
        if c.op == "channel_maxabs":
            full = dmx.ops.channel_maxabs(x, ax)
            parts = [dmx.ops.channel_maxabs(x[a:b], ax) for a, b in LC.chunks(c)]
            want = torch.cat(parts) if cat else torch.stack(parts).amax(0) if not c.specials else _nanmax(parts)
            assert LC.mismatches_on_device(full, want) == 0, c.name
        else:
            full = dmx.ops.group_minmax(x, ax, c.p["gs"])
            want = _combine_minmax([dmx.ops.group_minmax(x[a:b], ax, c.p["gs"]) for a, b in LC.chunks(c)], cat)
            assert torch.equal(full[0].view(torch.int32), want[0].view(torch.int32)) and torch.equal(full[1].view(torch.int32), want[1].view(torch.int32)), c.name
            assert full[0].numel() == c.shape[ax] // c.p["gs"]
    finally:
        del x
        torch.cuda.empty_cache()


def _nanmax(parts):
    m = parts[0]
    for p in parts[1:]:
        m = torch.maximum(m, p)      # (propagates NaN, as the kernel's integer maximum of |x| patterns does)
    return m


@pytest.mark.parametrize("twin", [False, True], ids=["full", "under"])
def test_histc_equals_the_int64_sum_of_its_chunks(dmx, cuda, twin):
    c = _sp("histc", twin)
    _need(c)
    x = _primary(c, cuda)
    try:
        full = dmx.ops.histc(x, c.p["bins"], -8.0, 8.0)
        total = torch.zeros(c.p["bins"], dtype=torch.int64, device=cuda)
        for a, b in LC.chunks(c, 1 << 29):       # (pieces small enough that every float32 count of a piece is exact: < 2^24 per bin)
            part = dmx.ops.histc(x[a:b], c.p["bins"], -8.0, 8.0)
            assert float(part.max()) < 2 ** 24
            total += part.to(torch.int64)
        assert int(total.sum()) <= x.numel() and int(total.sum()) > 0.99 * x.numel()
        assert torch.equal(full, total.to(F32)), c.name      # converted to float32 ONCE
    finally:
        del x
        torch.cuda.empty_cache()


def _combine_rows(rows):
    r = torch.stack(rows).double()
    return torch.stack([r[:, 0].sum(), r[:, 1].sum(), r[:, 2].max(), r[:, 3].sum()])


@pytest.mark.parametrize("twin", [False, True], ids=["full", "under"])
def test_error_stats_equal_their_chunks_combined_exactly(dmx, cuda, twin):
    """inputs on a dyadic grid (multiples of 2^-6 below 4: exact in bf16): every squared error is a multiple of 2^-12 and every sum exact
    in float64 in ANY order, so the full-size row equals the combined rows with no tolerance, and count == n"""
    c = _sp("error_stats", twin)
    _need(c)
    r = _primary(c, cuda)
    t = _second(c, "dyadic", BF16, cuda)
    try:
        full = dmx.ops.error_stats(r, t)
        want = _combine_rows([dmx.ops.error_stats(r[a:b], t[a:b]) for a, b in LC.chunks(c)])
        assert torch.equal(full.cpu(), want.cpu()), (full.tolist(), want.tolist())
        assert float(full[3]) == r.numel() and float(full[0]) > 0
    finally:
        del r, t
        torch.cuda.empty_cache()


@pytest.mark.parametrize("twin", [False, True], ids=["full", "under"])
def test_cast_error_equals_its_chunks_combined_exactly(dmx, cuda, twin):
    """the fused sweep on the dyadic grid: BFP and E4M3 results and the INT8 grid of step 2^-5 are dyadic too, so the rows are exact"""
    c = _sp("cast_error", twin)
    _need(c)
    x = _primary(c, cuda)
    fmts = ["BFP[8|8]{64}(SN)", E4M3_FMT, (INT8, 0.03125, 0)]
    try:
        full = dmx.ops.cast_error(x, fmts)
        parts = [dmx.ops.cast_error(x[a:b], fmts) for a, b in LC.chunks(c)]
        for k in range(len(fmts)):
            want = _combine_rows([p[k] for p in parts])
            assert torch.equal(full[k].cpu(), want.cpu()), (k, full[k].tolist(), want.tolist())
            assert float(full[k][3]) == x.numel()
        assert float(full[1][0]) > 0
    finally:
        del x
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ topk_mask between 2^31 and 2^32
def _topk_values(a, b, dev):
    i = torch.arange(a, b, dtype=torch.int64, device=dev)
    return ((i * 2654435761) & 0xFFFFFFFF) >> 24          # 256 values, every one exact in bf16, in no pattern with a short period


def _density_for(n, n_zero):
    d = 1.0 - n_zero / n
    for _ in range(64):
        got = int(n * (1.0 - d))
        if got == n_zero:
            return d
        d = math.nextafter(d, 0.0 if got < n_zero else 1.0)
    raise AssertionError((n, n_zero))


def test_topk_mask_between_two_to_the_31_and_32_elements(dmx, cuda):
    """analytic reference: the scores take 256 values with counted multiplicities, so the threshold value and the 'ties lowest index
    first' cut follow from n_zero alone; one density ends inside a tie run, one exactly at the end of one.  n = 2^32 is refused through
    the raw ABI before any pointer is used (topk.hip:315)."""
    c = LC.SPECIAL_BY_NAME["topk_mask"]
    _SLOT.clear()
    _need(c)
    n, piece = c.shape[0], 1 << 27
    assert LC.TWO31 < n < LC.TWO32
    score = torch.empty(n, dtype=BF16, device=cuda)
    counts = torch.zeros(256, dtype=torch.int64, device=cuda)
    for a in range(0, n, piece):
        v = _topk_values(a, min(a + piece, n), cuda)
        counts += torch.bincount(v, minlength=256)
        score[a:a + piece] = v.to(BF16)
    cum = torch.cumsum(counts, 0).cpu().tolist()
    assert cum[-1] == n
    try:
        inside = int(n * (1.0 - 0.37))
        for n_zero in (inside, cum[150]):
            t = next(k for k in range(256) if cum[k] >= n_zero)            # the threshold value
            ties_to_zero = n_zero - (cum[t - 1] if t else 0)                 # ... of whose occurrences the lowest indices are zeroed
            if n_zero == inside:
                assert 0 < ties_to_zero < cum[t] - cum[t - 1]
            else:
                assert ties_to_zero == cum[t] - cum[t - 1]
            mask = dmx.ops.topk_mask(score, _density_for(n, n_zero))
            assert mask.dtype == BF16 and mask.shape == score.shape
            seen_ties, bad, ones = 0, 0, 0
            for a in range(0, n, piece):
                v = _topk_values(a, min(a + piece, n), cuda)
                tie = v == t
                rank = torch.cumsum(tie, 0) - 1 + seen_ties
                want = (v > t) | (tie & (rank >= ties_to_zero))
                seen_ties += int(tie.sum())
                got = mask[a:a + piece]
                bad += int((got != want.to(BF16)).sum())
                ones += int(want.sum())
            assert ones == n - n_zero
            assert bad == 0, (n_zero, t, ties_to_zero, bad)
            del mask
        from dmx_compressor_amd import _lib
        L = _lib.lib()
        vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
        L.dmxq_topk_mask.argtypes = [vp, i32, vp, i32, vp, i32, vp, i32, i64, i64, vp, vp]
        L.dmxq_topk_mask.restype = i32
        tiny = torch.zeros(64, dtype=BF16, device=cuda)
        ws = torch.zeros(64, dtype=torch.int64, device=cuda)
        rc = L.dmxq_topk_mask(vp(tiny.data_ptr()), _lib.BF16, None, 0, vp(tiny.data_ptr()), _lib.BF16, None, 0, 1 << 32, 5, vp(ws.data_ptr()),
                              vp(torch.cuda.current_stream().cuda_stream))
        assert rc == 2      # DMXQ_ERR_UNSUPPORTED
    finally:
        del score
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ index-keyed random streams
def _tails(n):
    """the last 2^20 elements, and 2^20 elements straddling 2^31"""
    return [(n - TAIL, n), (LC.TWO31 - TAIL // 2, LC.TWO31 + TAIL // 2)]


def test_bernoulli_mask_draws_are_keyed_by_the_64_bit_index(dmx, cuda, oracle):
    c = LC.SPECIAL_BY_NAME["bernoulli_mask"]
    _need(c)
    score = _primary(c, cuda).view(-1)
    try:
        mask = dmx.ops.bernoulli_mask(score, seed=77)
        for a, b in _tails(score.numel()):
            want = oracle.bernoulli_mask(score[a:b].cpu(), 77, start=a)
            assert mismatches_nan_aware(mask[a:b], want) == 0, (a, b)
            assert 0.3 < float(want.float().mean()) < 0.7
        # ... and the same draws must not come back 2^31 elements earlier (a stream keyed by a truncated index would repeat)
        a = score.numel() - TAIL
        assert not torch.equal(dmx.ops.bernoulli_mask(score[a:], seed=77), mask[a:])
    finally:
        del score
        torch.cuda.empty_cache()


@pytest.mark.parametrize("name", ["float_qdq_stochastic", "fixed_qdq_stochastic"])
def test_stochastic_rounding_draws_are_keyed_by_the_64_bit_index(dmx, cuda, oracle, name):
    c = LC.SPECIAL_BY_NAME[name]
    _need(c)
    x = _primary(c, cuda).view(-1)
    try:
        if name == "float_qdq_stochastic":
            full = dmx.ops.float_qdq(x, 3, 4, 7, False, rounding="stochastic", seed=5)
            ref = lambda t, a: oracle.float_quantize(t, 3, 4, 7, False, "stochastic", 5, start=a).to(BF16)
            sub = lambda t: dmx.ops.float_qdq(t, 3, 4, 7, False, rounding="stochastic", seed=5)
        else:
            full = dmx.ops.fixed_qdq(x, 8, 4, True, True, "stochastic", seed=5)
            ref = lambda t, a: oracle.fixed_point_cast(t, 8, 4, True, True, "stochastic", 5, start=a).to(BF16)
            sub = lambda t: dmx.ops.fixed_qdq(t, 8, 4, True, True, "stochastic", seed=5)
        for a, b in _tails(x.numel()):
            assert mismatches_nan_aware(full[a:b], ref(x[a:b].cpu(), a)) == 0, (name, a, b)
        a = x.numel() - TAIL
        assert not torch.equal(sub(x[a:]), full[a:])      # (the slice on its own starts the stream at index 0: other draws)
    finally:
        del x
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ the *_multi entries
SMALL = ((30, 64), (45, 128), (15, 3072))


def _multi_set(c, dev):
    big = _primary(c, dev)
    return [big] + [LC.device_input(c.kind, s, BF16, 40 + i, dev) for i, s in enumerate(SMALL)]


def _chunked(c, fn, big):
    return torch.cat([fn(big[a:b], (a, b)) for a, b in LC.chunks(c)])


def _assert_set(c, got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype and LC.mismatches_on_device(g, w) == 0, (c.name, "member", i)


@pytest.mark.parametrize("name", ["multi_hypernet", "multi_bfp", "multi_float"])
def test_multi_entries_with_one_huge_member_give_the_per_tensor_results(dmx, cuda, name):
    """one tensor of more than 2^31 elements and three small ones: exactly the single-tensor results (the huge member's: its chunks')"""
    c = LC.SPECIAL_BY_NAME[name]
    _need(c)
    ts = _multi_set(c, cuda)
    ops = dmx.ops
    try:
        if name == "multi_hypernet":
            got = ops.weight_hypernet_multi(ts, 8, 64)
            one = lambda t, ab=None: ops.weight_hypernet(t, 8, 64)
        elif name == "multi_bfp":
            got = ops.bfp_qdq_multi(ts, 8, 16)
            one = lambda t, ab=None: ops.bfp_qdq(t, 8, 16)
        else:
            got = ops.float_qdq_multi(ts, 3, 4, 7, False)
            one = lambda t, ab=None: ops.float_qdq(t, 3, 4, 7, False)
        assert got is not None
        _assert_set(c, got[1:], [one(t) for t in ts[1:]])
        LC.check_chunks(c, lambda v, ab: (one(v[0]),), [ts[0]], (got[0],))
    finally:
        del ts
        torch.cuda.empty_cache()


def _affine(t, gs, dev):
    G = t.shape[0] // gs
    g = _cpu_gen(G)
    return (torch.rand(G, generator=g) * 0.2 + 0.01).to(dev), torch.randint(-9, 10, (G,), generator=g).to(dev)


@pytest.mark.parametrize("name", ["multi_fixed", "multi_fixed_float"])
def test_fixed_multi_entries_with_one_huge_member_give_the_per_tensor_results(dmx, cuda, name):
    """fixed_qdq_multi, and fixed_float_qdq_multi with the huge member once in either list (fixed_multi.hip:152 / :159)"""
    c = LC.SPECIAL_BY_NAME[name]
    _need(c)
    ts = _multi_set(c, cuda)
    ops, gs = dmx.ops, c.p["gs"]
    qs = [_affine(t, gs, cuda) for t in ts]
    sc, zp = [q[0] for q in qs], [q[1] for q in qs]
    fixed1 = lambda t, s, z: ops.fixed_qdq(t, 8, 0, True, True, scale=s, zero_point=z, ch_axis=0, group_size=gs)
    float1 = lambda t: ops.float_qdq(t, 3, 4, 7, False)
    big_fixed = lambda v, ab: (fixed1(v[0], sc[0][ab[0] // gs:-(-ab[1] // gs)], zp[0][ab[0] // gs:-(-ab[1] // gs)]),)
    try:
        if name == "multi_fixed":
            got = ops.fixed_qdq_multi(ts, 8, 0, True, True, sc, zp, group_size=gs)
            _assert_set(c, got[1:], [fixed1(t, s, z) for t, s, z in zip(ts[1:], sc[1:], zp[1:])])
            LC.check_chunks(c, big_fixed, [ts[0]], (got[0],))
        else:
            a, b = ops.fixed_float_qdq_multi(ts, 8, 0, True, True, sc, zp, gs, ts[1:], 3, 4, 7, False)      # the huge member among the fixed
            _assert_set(c, a[1:], [fixed1(t, s, z) for t, s, z in zip(ts[1:], sc[1:], zp[1:])])
            _assert_set(c, b, [float1(t) for t in ts[1:]])
            LC.check_chunks(c, big_fixed, [ts[0]], (a[0],))
            del a, b
            a, b = ops.fixed_float_qdq_multi(ts[1:], 8, 0, True, True, sc[1:], zp[1:], gs, ts, 3, 4, 7, False)  # ... and among the floats
            _assert_set(c, a, [fixed1(t, s, z) for t, s, z in zip(ts[1:], sc[1:], zp[1:])])
            _assert_set(c, b[1:], [float1(t) for t in ts[1:]])
            LC.check_chunks(c, lambda v, ab: (float1(v[0]),), [ts[0]], (b[0],))
    finally:
        del ts
        torch.cuda.empty_cache()
