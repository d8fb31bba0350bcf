"""-m gpu: softmax, LayerNorm and RMSNorm on EVERY kernel class their dispatch can select (tests/_row_cases.py: the table of classes,
each with the smallest row length and base misalignment that selects it), through the C ABI with the real device pointers:

  * the library's class query (dmxq_row_class_of, the dispatch's own decision) must name the class the table names;
  * float64 truth within the tolerances of the older row tests (tests/_row_truth.py), on rows PLANTED along the class's geometry --
    one spike per per-lane slot boundary, a heavy last vector / tail / first vector -- so that a dropped, doubled or mis-indexed
    lane-vector is a gross error and not a fraction of an ulp, plus a random, a half-masked and a fully masked row;
  * ragged row counts (1, a workgroup's share less one, two shares and three) over all planted rows;
  * in place (out == in) bit-equal to out of place;
  * the fused BFP forms bit for bit the two launches, under every fused-cast kind of the table, on accepted block sizes; refused sizes
    and ragged rows are refused, the front end answers None and its two launches give the chain's bits;
  * more rows than one round of the grid, and the one-pass variants for tensors of 26-32 MiB."""
import ctypes

import pytest
import torch

import _row_cases as R
from _data import bits_equal, err_in_ulps, make, outside_cast_bracket, ulp_of
from _row_truth import cpu_cast_canonical_nan, ln_truth, rms_truth, row_n_ulp, tol

pytestmark = pytest.mark.gpu
F = torch.nn.functional
vp = ctypes.c_void_p
TORCH_DT = {R.F32: torch.float32, R.F16: torch.float16, R.BF16: torch.bfloat16}
OTHER = {R.F32: R.BF16, R.F16: R.F32, R.BF16: R.F16}
FMT = {"SAME": None, "FLOAT16": "FP[1|5|10,15](FN)", "FP21": "FP[1|8|20,127](FN)"}   # FP21: an output cast that keeps > 16 mantissa bits
EPS = {R.SOFTMAX: 0.0, R.LAYERNORM: 1e-5, R.RMSNORM: 1e-6}
# the pair of casts that stands for each fused-cast kind of the table (R.cast_kinds): the BFP tests run every kind, so a kind that
# selects another instantiation (float32 softmax: FAST32 or not) cannot go unlaunched
PAIR_OF_KIND = {R.CAST_RANGE: ("FLOAT16", "FLOAT16"), R.CAST_MAN16: ("FLOAT16", "FLOAT16"), R.CAST_GENERAL: ("SAME", "SAME")}
WL = 8      # BFP precision of the fused epilogue tests
NPART = 2   # every (form, dtype) runs its classes in NPART slices, to keep a single test within a few seconds


# ---------------------------------------------------------------------------------------------------------------- planted rows
def _geometry(cls, dtype, cols):
    """(E, V, L) along which the rows are planted; the fallbacks walk a row with 256 threads, one element each"""
    if cls.family in (R.WAVE, R.BLOCK):
        return cls.epl, cls.vpl, cls.lpr
    return 1, min(-(-cols // R.THREADS), 4), R.THREADS


def planted_rows(op, cls, dtype, cols, seed):
    """[P, cols] rows of `dtype` (see the module docstring); softmax: background -30, spike +10, heavy regions 0; norms: background 0,
    spike 1, heavy regions alternating +1 / -1"""
    E, V, Lr = _geometry(cls, dtype, cols)
    soft = op == R.SOFTMAX
    bg, spike = (-30.0, 10.0) if soft else (0.0, 1.0)
    nvf, nv = cols // E, -(-cols // E)
    pos = {0, E - 1, E, (nv - 1) * E, cols - E, cols - 2, cols - 1}
    pos |= {i * Lr * E for i in range(V)} | {i * Lr * E + (Lr - 1) * E for i in range(V)}
    pos = sorted(p for p in pos if 0 <= p < cols)
    rows = []
    for p in pos:
        r = torch.full((cols,), bg)
        r[p] = spike
        rows.append(r)
    alt = torch.ones(cols)
    alt[1::2] = -1.0
    tail = cols - nvf * E
    regions = [(max(nvf - 1, 0) * E, max(nvf, 1) * E if nvf else cols),          # the last whole vector
               (nvf * E, cols) if tail else (cols - max(E // 2, 1), cols),         # the partial tail alone (no tail: the last half vector)
               (0, min(E, cols))]                                                  # the first vector
    for lo, hi in regions:
        r = torch.full((cols,), bg)
        r[lo:hi] = 0.0 if soft else alt[lo:hi]
        rows.append(r)
    rnd = make("normal", (2, cols), seed=seed) * 2
    if soft:
        rnd[1, : cols // 2] = float("-inf")                 # a half-masked row
        rows += [rnd[0], rnd[1], torch.full((cols,), float("-inf"))]   # ... and a fully masked one: NaN in torch too
    else:
        rnd[1] += 0.5
        rows += [rnd[0], rnd[1]]
    return torch.stack(rows).to(dtype)


def batches(P, cls):
    """row index lists: the ragged counts of the class, the largest repeated until every planted row has run"""
    counts = R.row_counts(cls)
    out = [[i % P for i in range(n)] for n in counts[:-1]]
    n, start = counts[-1], 0
    while start < P:
        out.append([(start + i) % P for i in range(n)])
        start += n
    return out


# ---------------------------------------------------------------------------------------------------------------- the C ABI
class Abi:
    def __init__(self, dmx, cuda):
        self.lib, self.L, self.dev, self.dmx = dmx._lib, dmx._lib.lib(), cuda, dmx
        self.fmts = {k: None if v is None else dmx.Format.from_shorthand(v) for k, v in FMT.items()}
        self.structs = {k: None if f is None else self.lib.FloatFmt(f.mantissa, f.exponent, f.bias, int(f.flush_subnormal))
                        for k, f in self.fmts.items()}

    def fptr(self, name):
        s = self.structs[name]
        return None if s is None else ctypes.cast(ctypes.pointer(s), vp)

    def view(self, t, off):
        """a device copy of t that starts `off` bytes off the 16-byte grid"""
        pad = off // t.element_size()
        buf = torch.empty(t.numel() + 16, dtype=t.dtype, device=self.dev)
        assert buf.data_ptr() % 16 == 0
        v = buf[pad: pad + t.numel()].view(t.shape)
        v.copy_(t)
        return v

    def query(self, op, x, out, w, b, cast, bfp=0):
        cls = self.lib.RowClass()
        rows, cols = x.shape
        dtw = self.lib.dtype_code(w.dtype) if w is not None else self.lib.dtype_code(x.dtype)
        st = self.L.dmxq_row_class_of(op, self.lib.dtype_code(x.dtype), self.lib.dtype_code(out.dtype), dtw, rows, cols, vp(x.data_ptr()),
                                      vp(out.data_ptr()), self.lib.ptr(w), self.lib.ptr(b), cast, bfp, ctypes.byref(cls))
        assert st == self.lib.OK
        return R.RowClass(*cls.key())

    def run(self, op, x, out, w=None, b=None, pair=None, clamp=float("-inf"), bfp=0):
        """one launch; returns the status"""
        L, lib = self.L, self.lib
        rows, cols = x.shape
        dti, dto, s = lib.dtype_code(x.dtype), lib.dtype_code(out.dtype), lib.stream_of(x)
        xin, xo = vp(x.data_ptr()), vp(out.data_ptr())
        dtw = lib.dtype_code(w.dtype) if w is not None else dti
        eps = EPS[op]
        if pair is None:
            if op == R.SOFTMAX:
                return L.dmxq_softmax(xin, xo, dti, dto, rows, cols, clamp, s)
            if op == R.LAYERNORM:
                return L.dmxq_layernorm(xin, xo, dti, dto, rows, cols, lib.ptr(w), lib.ptr(b), dtw, eps, s)
            return L.dmxq_rmsnorm(xin, xo, dti, dto, rows, cols, lib.ptr(w), dtw, eps, s)
        fi, fo = self.fptr(pair[0]), self.fptr(pair[1])
        tail = (bfp, WL, s) if bfp else (s,)
        if op == R.SOFTMAX:
            return (L.dmxq_softmax_cast_bfp if bfp else L.dmxq_softmax_cast)(xin, xo, dti, rows, cols, clamp, fi, fo, *tail)
        if op == R.LAYERNORM:
            return (L.dmxq_layernorm_cast_bfp if bfp else L.dmxq_layernorm_cast)(xin, xo, dti, rows, cols, lib.ptr(w), lib.ptr(b), eps, fi, fo, *tail)
        return (L.dmxq_rmsnorm_cast_bfp if bfp else L.dmxq_rmsnorm_cast)(xin, xo, dti, rows, cols, lib.ptr(w), eps, fi, fo, *tail)

    def front(self, op, x, w, b, pair, then_bfp=None, clamp=float("-inf")):
        """the front end's fused-cast op (None = not fusable: the caller runs the two launches)"""
        ops, fi, fo, cols = self.dmx.ops, self.fmts[pair[0]], self.fmts[pair[1]], x.shape[-1]
        if op == R.SOFTMAX:
            return ops.softmax_cast(x, -1, fi, fo, None if clamp == float("-inf") else clamp, then_bfp=then_bfp)
        if op == R.LAYERNORM:
            return ops.layernorm_cast(x, (cols,), w, b, EPS[op], fi, fo, then_bfp=then_bfp)
        return ops.rmsnorm_cast(x, (cols,), w, EPS[op], fi, fo, then_bfp=then_bfp)

    def bfp_qdq(self, x, out, block):
        rows, cols = x.shape
        dt = self.lib.dtype_code(x.dtype)
        return self.L.dmxq_bfp_qdq(vp(x.data_ptr()), vp(out.data_ptr()), dt, dt, rows, cols, 1, block, WL, self.lib.ROUND_NEAREST, 1, 0, self.lib.stream_of(x))


@pytest.fixture(scope="module")
def abi(dmx, cuda):
    return Abi(dmx, cuda)


def cast_kind(dtype, pair, abi):
    if pair is None:
        return R.CAST_NONE
    if dtype != R.F32:
        return R.CAST_RANGE
    fo = abi.fmts[pair[1]]
    return R.CAST_MAN16 if fo is not None and fo.mantissa <= 16 else R.CAST_GENERAL


def params_of(op, dtype, cols, wb, mixed):
    """weight / bias of the case (wb: 2 = both, 1 = weight only, 0 = neither); mixed: parameters of another dtype"""
    if op == R.SOFTMAX or wb == 0:
        return None, None
    dt = TORCH_DT[OTHER[dtype] if mixed else dtype]
    w = (make("normal", (cols,), seed=12) * 0.1 + 1).to(dt)
    b = (make("normal", (cols,), seed=13) * 0.1).to(dt) if (wb == 2 and op == R.LAYERNORM) else None
    return w, b


def truth_of(op, x, w, b, pair, clamp, abi, oracle):
    """(float64 truth, floor of the cancelling terms or None) of the planted rows"""
    c = x if pair is None else cpu_cast_canonical_nan(oracle, abi.fmts[pair[0]])(x)
    if op == R.SOFTMAX:
        cd = c.double()
        return F.softmax(cd.clamp(min=clamp) if clamp > float("-inf") else cd, -1), None
    if op == R.LAYERNORM:
        return ln_truth(c, x.shape[-1], w, b, EPS[op])
    return rms_truth(c, x.shape[-1], w, EPS[op]), None


def _worst(got, truth, out_dtype, cast_o, n_ulp, floor, k=6):
    """for a failure message: the k elements farthest outside [cast(truth - n ulp), cast(truth + n ulp)], as (row, col, got, lo, hi)"""
    g, t = got.detach().cpu().double(), truth.detach().cpu().double()
    u = ulp_of(t, out_dtype, floor) * n_ulp
    tz = torch.where(torch.isnan(t), torch.zeros_like(t), t)
    lo, hi = cast_o((tz - u).to(out_dtype)).double(), cast_o((tz + u).to(out_dtype)).double()
    d = torch.where(torch.isnan(t) | ((g >= lo) & (g <= hi)), torch.zeros_like(g), torch.maximum(lo - g, g - hi)).nan_to_num(float("inf"))
    want = cast_o(t.to(out_dtype)).double()     # NaN truth: what the cast makes of a NaN, by magnitude
    d = torch.where(torch.isnan(t) & ~(torch.isnan(want) & torch.isnan(g)) & ~(g.abs() == want.abs()), torch.full_like(d, float("inf")), d)
    top = [i for i in torch.topk(d.flatten(), min(k, d.numel())).indices.tolist() if float(d.flatten()[i]) > 0]
    return [(i // g.shape[1], i % g.shape[1], float(g.flatten()[i]), float(lo.flatten()[i]), float(hi.flatten()[i])) for i in top]


def check_truth(op, got, truth, floor, out_dtype, pair, abi, oracle, what):
    name = R.OP_NAMES[op]
    if pair is None:
        bound = row_n_ulp("rmsnorm", out_dtype, None) if op == R.RMSNORM else tol(name, out_dtype)
        e = err_in_ulps(got, truth, out_dtype, floor=floor)
        assert e <= bound, (what, "ulps", e, "allowed", bound, _worst(got, truth, out_dtype, lambda t: t, bound, floor))
    else:
        fo = abi.fmts[pair[1]]
        bad = outside_cast_bracket(got, truth, cpu_cast_canonical_nan(oracle, fo), out_dtype, row_n_ulp(name, out_dtype, fo), floor)
        assert bad == 0, (what, "elements outside the cast bracket", bad, _worst(got, truth, out_dtype, cpu_cast_canonical_nan(oracle, fo), row_n_ulp(name, out_dtype, fo), floor))


def run_case(abi, oracle, case, pair=None, clamp=float("-inf"), wb=2, with_bfp=False):
    """every check of one table case under one variant of its form"""
    op, dtype, cols, cls = case.op, case.dtype, case.cols, case.cls
    tdt = TORCH_DT[dtype]
    odt = TORCH_DT[OTHER[dtype]] if (case.mixed and op == R.SOFTMAX) else tdt
    ck = cast_kind(dtype, pair, abi)
    X = planted_rows(op, cls, tdt, cols, seed=cols + 7 * dtype)
    w, b = params_of(op, dtype, cols, 2 if case.mixed else wb, case.mixed)
    truth, floor = truth_of(op, X, w, b, pair, clamp, abi, oracle)
    wg, bg = (None if t is None else abi.view(t, case.off) for t in (w, b))
    what = (R.OP_NAMES[op], R.DT_NAMES[dtype], "cols", cols, "off", case.off, "mixed", case.mixed, pair, clamp, "wb", wb)
    for idx in batches(X.shape[0], cls):
        x = abi.view(X[idx], case.off)
        out = abi.view(torch.zeros(len(idx), cols, dtype=odt), case.off)
        assert abi.query(op, x, out, wg, bg, ck) == cls, (what, len(idx), abi.query(op, x, out, wg, bg, ck), cls)
        assert abi.run(op, x, out, wg, bg, pair, clamp) == abi.lib.OK, what
        check_truth(op, out, truth[idx], None if floor is None else floor[idx], odt, pair, abi, oracle, what + ("rows", len(idx)))
        if odt == tdt:      # in place: the same class, the same bits
            assert abi.query(op, x, x, wg, bg, ck) == cls, (what, "in-place class")
            assert abi.run(op, x, x, wg, bg, pair, clamp) == abi.lib.OK, what
            assert bits_equal(x, out) == 0, (what, "in place differs from out of place", len(idx))
    if not with_bfp:
        return
    # the fused BFP epilogue on the last (largest) batch: bit for bit the module's launch followed by dmxq_bfp_qdq
    x = abi.view(X[idx], case.off)
    two, chain, fused = (abi.view(torch.zeros(len(idx), cols, dtype=tdt), case.off) for _ in range(3))
    assert abi.run(op, x, two, wg, bg, pair, clamp) == abi.lib.OK
    def routed(B):
        """a refused size: the front end answers None, and its two launches give the bits of the chain"""
        assert abi.front(op, x, wg, bg, pair, (WL, B), clamp) is None, (what, "BFP", B)
        assert abi.bfp_qdq(two, chain, B) == abi.lib.OK
        assert bits_equal(abi.dmx.ops.bfp_qdq(abi.front(op, x, wg, bg, pair, None, clamp), WL, B), chain) == 0, (what, "the two launches", B)

    if cls.rag:      # ragged rows: the fused form refuses every size, the caller runs the two launches
        assert abi.query(op, x, fused, wg, bg, ck, 16) == R.REFUSED
        assert abi.run(op, x, fused, wg, bg, pair, clamp, bfp=16) == abi.lib.ERR_UNSUPPORTED, what
        routed(16)
        return
    ok, refused = R.bfp_blocks(cls)
    for B in ok:
        want = cls._replace(bfpout=1, grid=R.G_PERSISTENT if cls.grid == R.G_MODULE_ONE_PASS else cls.grid)
        assert abi.query(op, x, fused, wg, bg, ck, B) == want, (what, "BFP", B)
        assert abi.bfp_qdq(two, chain, B) == abi.lib.OK
        assert abi.run(op, x, fused, wg, bg, pair, clamp, bfp=B) == abi.lib.OK, (what, "BFP", B)
        assert bits_equal(fused, chain) == 0, (what, "fused BFP differs from the two launches", B)
        xi = x.clone() if case.off == 0 else abi.view(X[idx], case.off)
        assert abi.run(op, xi, xi, wg, bg, pair, clamp, bfp=B) == abi.lib.OK
        assert bits_equal(xi, fused) == 0, (what, "fused BFP in place", B)
    for B in refused:   # nothing is launched: the caller runs the two launches
        fused.fill_(7.0)
        assert abi.query(op, x, fused, wg, bg, ck, B) == R.REFUSED, (what, "BFP", B)
        assert abi.run(op, x, fused, wg, bg, pair, clamp, bfp=B) == abi.lib.ERR_UNSUPPORTED, (what, "BFP", B)
        assert bool((fused == 7.0).all()), (what, "a refused call wrote", B)
        routed(B)


def run_cases(abi, oracle, cases, **variant):
    """every case runs, so that a failure names ALL the classes that fail (a HIP error is no AssertionError and ends the test at once)"""
    failed = []
    for case in cases:
        try:
            run_case(abi, oracle, case, **variant)
        except AssertionError as e:
            failed.append(f"{case.cls} cols={case.cols} off={case.off}: {str(e)[:900]}")
    assert not failed, f"{len(failed)} of {len(cases)} classes fail:\n" + "\n".join(failed)


def cases_of(op, dtype, kind, part):
    cs = R.launched(R.table(op, dtype, kind))
    assert cs, (op, dtype, kind)
    return cs[part::NPART]


DTYPES = [R.F32, R.F16, R.BF16]


@pytest.mark.parametrize("part", range(NPART))
@pytest.mark.parametrize("dtype", DTYPES, ids=[R.DT_NAMES[d] for d in DTYPES])
@pytest.mark.parametrize("clamp", [float("-inf"), -20.0], ids=["noclamp", "clamp"])
def test_softmax(abi, oracle, dtype, clamp, part):
    """input_clamp = -20 lifts the planted background (-30) and every masked element (-inf) to -20: the clamp is exercised on all of them,
    and the planted rows stay planted -- 16384 background terms still add up to 2e-9 of the spike, far below an fp32 ulp, so a dropped
    or doubled lane-vector of a heavy row remains a gross error.  (A clamp near the data, -1, would turn every planted row into a nearly
    uniform one, where such an error hides again -- and where the float32 row sum of thousands of EQUAL terms rounds the same way at
    every step: measured 9 ulps on rows of 2564 and 12 on rows of 16385 elements, against the 8 that tests/_row_truth.py states from
    random rows.)"""
    run_cases(abi, oracle, cases_of(R.SOFTMAX, dtype, R.CAST_NONE, part), clamp=clamp)


@pytest.mark.parametrize("part", range(NPART))
@pytest.mark.parametrize("dtype,pair", [(d, p) for d in DTYPES for p in [("FLOAT16", "FLOAT16"), ("SAME", "SAME")] + ([("FLOAT16", "FP21")] if d == R.F32 else [])],
                         ids=lambda v: R.DT_NAMES[v] if isinstance(v, int) else "-".join(v))
def test_softmax_cast(abi, oracle, dtype, pair, part):
    """FLOAT16 / FLOAT16: range-only casts on 16-bit rows, the FAST32 kernel on float32; SAME / SAME; float32 behind an output cast of 20
    mantissa bits: the general cast kernel"""
    kind = cast_kind(dtype, pair, abi)
    assert kind == (R.CAST_RANGE if dtype != R.F32 else (R.CAST_MAN16 if pair[1] == "FLOAT16" else R.CAST_GENERAL))
    cases = cases_of(R.SOFTMAX, dtype, kind, part)
    assert all(c.cls.fast32 == int(kind == R.CAST_MAN16 and not c.cls.rag) for c in cases)
    run_cases(abi, oracle, cases, pair=pair)


def _kinds(op):
    return [(d, k) for d in DTYPES for k in R.cast_kinds(op, d)]


def _kind_id(v):
    return "-".join((R.DT_NAMES[v[0]], {R.CAST_RANGE: "range", R.CAST_MAN16: "man16", R.CAST_GENERAL: "general"}[v[1]]))


@pytest.mark.parametrize("part", range(NPART))
@pytest.mark.parametrize("dtype_kind", _kinds(R.SOFTMAX), ids=_kind_id)
def test_softmax_cast_bfp(abi, oracle, dtype_kind, part):
    """every fused-cast kind of the table: on float32 the FAST32 + BFPOUT kernel (FLOAT16 / FLOAT16) and the plain BFPOUT one (SAME / SAME)"""
    dtype, kind = dtype_kind
    pair = PAIR_OF_KIND[kind]
    assert cast_kind(dtype, pair, abi) == kind
    run_cases(abi, oracle, cases_of(R.SOFTMAX, dtype, kind, part), pair=pair, with_bfp=True)


@pytest.mark.parametrize("part", range(NPART))
@pytest.mark.parametrize("dtype", DTYPES, ids=[R.DT_NAMES[d] for d in DTYPES])
@pytest.mark.parametrize("op,wb", [(R.LAYERNORM, 2), (R.LAYERNORM, 1), (R.LAYERNORM, 0), (R.RMSNORM, 1), (R.RMSNORM, 0)],
                         ids=["layernorm-weight+bias", "layernorm-weight", "layernorm-plain", "rmsnorm-weight", "rmsnorm-plain"])
def test_norm(abi, oracle, op, wb, dtype, part):
    run_cases(abi, oracle, cases_of(op, dtype, R.CAST_NONE, part), wb=wb)


@pytest.mark.parametrize("part", range(NPART))
@pytest.mark.parametrize("dtype", DTYPES, ids=[R.DT_NAMES[d] for d in DTYPES])
@pytest.mark.parametrize("op,pair,wb", [(R.LAYERNORM, ("FLOAT16", "FLOAT16"), 2), (R.LAYERNORM, ("FLOAT16", "FLOAT16"), 1),
                                        (R.LAYERNORM, ("FLOAT16", "FLOAT16"), 0), (R.LAYERNORM, ("SAME", "SAME"), 2),
                                        (R.RMSNORM, ("FLOAT16", "FLOAT16"), 1), (R.RMSNORM, ("FLOAT16", "FLOAT16"), 0), (R.RMSNORM, ("SAME", "SAME"), 1)],
                         ids=["layernorm-f16-weight+bias", "layernorm-f16-weight", "layernorm-f16-plain", "layernorm-same-weight+bias",
                              "rmsnorm-f16-weight", "rmsnorm-f16-plain", "rmsnorm-same-weight"])
def test_norm_cast(abi, oracle, op, pair, wb, dtype, part):
    run_cases(abi, oracle, cases_of(op, dtype, cast_kind(dtype, pair, abi), part), pair=pair, wb=wb)


@pytest.mark.parametrize("part", range(NPART))
@pytest.mark.parametrize("dtype_kind", _kinds(R.LAYERNORM), ids=_kind_id)
@pytest.mark.parametrize("op", [R.LAYERNORM, R.RMSNORM], ids=["layernorm", "rmsnorm"])
def test_norm_cast_bfp(abi, oracle, op, dtype_kind, part):
    dtype, kind = dtype_kind
    assert _kinds(op) == _kinds(R.LAYERNORM)
    pair = PAIR_OF_KIND[kind]
    assert cast_kind(dtype, pair, abi) == kind
    run_cases(abi, oracle, cases_of(op, dtype, kind, part), pair=pair, wb=2 if op == R.LAYERNORM else 1, with_bfp=True)
    if dtype == R.F32 and not part:      # (float32 norms have one kind; the narrow output cast of a module rides along on the first slice)
        run_cases(abi, oracle, cases_of(op, dtype, kind, part)[::3], pair=("FLOAT16", "FLOAT16"), wb=2 if op == R.LAYERNORM else 1, with_bfp=True)


# ------------------------------------------------------------------------------------------------- many rows, large tensors
def _slabbed(abi, oracle, op, dtype, cols, rows, off=0, mixed=False, pair=None, expect=None, slab=37):
    """[rows, cols] made of one slab of `slab` planted-free random rows repeated: the whole result must repeat its first slab bit for bit,
    and that slab must meet the float64 truth -- so every row of the tensor does, the last and the grid-wrap rows included"""
    tdt = TORCH_DT[dtype]
    odt = TORCH_DT[OTHER[dtype]] if (mixed and op == R.SOFTMAX) else tdt
    S = (make("normal", (slab, cols), seed=cols + rows) * 2 + (0.0 if op == R.SOFTMAX else 0.5)).to(tdt)
    if op == R.SOFTMAX:
        S[1, : cols // 2] = float("-inf")
    w, b = params_of(op, dtype, cols, 2, mixed)
    truth, floor = truth_of(op, S, w, b, pair, float("-inf"), abi, oracle)
    wg, bg = (None if t is None else abi.view(t, off) for t in (w, b))
    pad = off // S.element_size()
    reps = -(-rows // slab)
    xbuf = torch.empty(rows * cols + 16, dtype=tdt, device=abi.dev)
    x = xbuf[pad: pad + rows * cols].view(rows, cols)
    x.copy_(S.to(abi.dev).repeat(reps, 1)[:rows])
    obuf = torch.zeros(rows * cols + 16, dtype=odt, device=abi.dev)
    opad = off // odt.itemsize
    out = obuf[opad: opad + rows * cols].view(rows, cols)
    cls = abi.query(op, x, out, wg, bg, cast_kind(dtype, pair, abi))
    what = (R.OP_NAMES[op], R.DT_NAMES[dtype], rows, cols, off, mixed, pair, cls)
    if expect is not None:
        expect(cls, what)
    assert abi.run(op, x, out, wg, bg, pair) == abi.lib.OK, what
    it = {4: torch.int32, 2: torch.int16}[odt.itemsize]
    first = out[:slab].contiguous().view(it)
    whole = rows // slab
    assert bool((out[: whole * slab].contiguous().view(it).view(whole, slab, cols) == first).all()), (what, "rows differ from their slab")
    if rows % slab:
        assert bool((out[whole * slab:].contiguous().view(it) == first[: rows % slab]).all()), (what, "last rows differ from their slab")
    check_truth(op, out[:slab], truth, floor, odt, pair, abi, oracle, what)
    return cls


def test_more_rows_than_one_round_of_the_grid(abi, oracle, cuda):
    """Once per kernel template, at its shortest rows: a persistent workgroup iterates at least three times, the last time ragged
    (8 workgroups per CU is the most a 256-thread kernel can keep resident; fewer resident means more iterations); the softmax wave
    kernel takes one pass per workgroup however many rows there are; the fallbacks run 4096 workgroups at the most."""
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count

    def rows_for(cls):
        if cls.grid == R.G_CAPPED:
            return 2 * 4096 + 5
        return cls.rows_per_iter * (2 * 8 * cus + cus) + 3

    def sized(op, dtype, cols, family, grid, **kw):
        probe = R.row_class(op, dtype, 1, cols, kw.get("off", 0), kw.get("mixed", False))
        assert probe.family == family and probe.grid == grid, probe
        def expect(cls, what):
            assert cls == probe, (what, probe)      # (not a 26-32 MiB tensor: the same class as one row)
        _slabbed(abi, oracle, op, dtype, cols, rows_for(probe), expect=expect, **kw)

    sized(R.SOFTMAX, R.BF16, 8, R.WAVE, R.G_ONE_PASS)                       # the softmax wave kernel, aligned ...
    sized(R.SOFTMAX, R.BF16, 9, R.WAVE, R.G_ONE_PASS)                       # ... and RAG
    sized(R.SOFTMAX, R.F32, 4, R.WAVE, R.G_ONE_PASS, off=4)
    sized(R.LAYERNORM, R.BF16, 8, R.WAVE, R.G_PERSISTENT)                   # the layernorm wave kernel
    sized(R.RMSNORM, R.F32, 4, R.WAVE, R.G_PERSISTENT)
    sized(R.LAYERNORM, R.BF16, 257 * 8, R.BLOCK, R.G_PERSISTENT)            # the workgroup-per-row kernel
    sized(R.RMSNORM, R.F32, 257 * 4, R.BLOCK, R.G_PERSISTENT)
    sized(R.SOFTMAX, R.BF16, 7, R.LDS_ROWS, R.G_CAPPED)                     # the fallbacks: rows staged in LDS ...
    sized(R.LAYERNORM, R.F16, 6, R.LDS_ROWS, R.G_CAPPED)
    sized(R.SOFTMAX, R.F16, 16, R.LDS_ROWS, R.G_CAPPED, mixed=True)         # (mixed dtypes: float16 in, float32 out)


def test_global_fallback_above_the_workgroup_cap(abi, oracle):
    """... and rows too long for LDS, read three times: the shortest such row is 16385 elements, so these two tensors are 256 MiB each"""
    for op in (R.SOFTMAX, R.LAYERNORM):
        probe = R.row_class(op, R.BF16, 1, 16385)
        assert probe.family == R.GLOBAL_ROWS
        assert _slabbed(abi, oracle, op, R.BF16, 16385, 2 * 4096 + 5, slab=5) == probe


@pytest.mark.parametrize("dtype", DTYPES, ids=[R.DT_NAMES[d] for d in DTYPES])
@pytest.mark.parametrize("op,fused", [(R.LAYERNORM, False), (R.RMSNORM, False), (R.RMSNORM, True)], ids=["layernorm", "rmsnorm", "rmsnorm_cast"])
def test_one_pass_variants_at_26_mib(abi, oracle, op, fused, dtype):
    """tensors of 26-32 MiB on the workgroup-per-row kernel: one shape per distinct (vectors per lane, rows per iteration) variant the
    table holds, each just over 26 MiB"""
    pair = ("FLOAT16", "FLOAT16") if fused else None
    cases = R.mid_cases(R.table(op, dtype, cast_kind(dtype, pair, abi)))
    if fused:
        assert len(cases) == (0 if dtype == R.F32 else 1)       # the RMSNorm module on 16-bit rows of 2049 .. 4096 elements
    else:
        assert [(c.cls.vpl, c.cls.rows_per_iter) for c in cases] == ([(2, 8), (3, 4), (4, 4)] + ([(5, 2), (6, 2), (8, 2)] if dtype != R.F32 else []))
    for c in cases:
        def expect(cls, what, c=c):
            assert cls == c.cls, (what, c.cls)
        _slabbed(abi, oracle, op, dtype, c.cols, c.rows, pair=pair, expect=expect)


@pytest.mark.parametrize("op", [R.LAYERNORM, R.RMSNORM], ids=["layernorm", "rmsnorm"])
def test_bfp_form_at_26_mib(abi, op):
    """a tensor of 26-32 MiB through the fused BFP form: no one-pass or four-row variant there -- the persistent workgroup kernel with
    the epilogue, bit for bit the two launches (bf16 rows of 4096, where the RMSNorm module alone would take its four-row form)"""
    dtype, cols, pair, B = R.BF16, 4096, ("FLOAT16", "FLOAT16"), 64
    rows = R.mid_rows(dtype, cols)
    alone = R.row_class(op, dtype, rows, cols, cast=R.CAST_RANGE)
    assert alone.grid == (R.G_MODULE_ROWS4 if op == R.RMSNORM else R.G_PERSISTENT)
    want = R.row_class(op, dtype, rows, cols, cast=R.CAST_RANGE, bfp=B)
    assert want == R.RowClass(R.BLOCK, 8, 2, R.THREADS, 0, 0, 0, 1, R.G_PERSISTENT, 2)
    S = (make("normal", (37, cols), seed=cols) * 2 + 0.5).to(TORCH_DT[dtype]).to(abi.dev)
    x = S.repeat(-(-rows // 37), 1)[:rows].contiguous()
    w, b = (None if t is None else t.to(abi.dev) for t in params_of(op, dtype, cols, 2, False))
    two, chain, fused = (torch.zeros_like(x) for _ in range(3))
    assert abi.query(op, x, two, w, b, R.CAST_RANGE) == alone
    assert abi.query(op, x, fused, w, b, R.CAST_RANGE, B) == want
    assert abi.run(op, x, two, w, b, pair) == abi.lib.OK and abi.bfp_qdq(two, chain, B) == abi.lib.OK
    assert abi.run(op, x, fused, w, b, pair, bfp=B) == abi.lib.OK
    assert bool((fused.view(torch.int16) == chain.view(torch.int16)).all())
