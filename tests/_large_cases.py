"""Case table of the tensors with more than 2^31 elements (tests/test_gpu_large_index.py) and the geometry that goes with it: how a
case is cut into chunks, which rows the oracle windows take, which periods its index decode has and how much device memory it needs.
Imported by tests/test_large_cases_host.py (host only: the table provably does what it is for) and by the GPU tests.  Nothing here
needs a GPU to be imported.

Most kernels of csrc/ carry two index forms, a 32-bit one (FastDiv31 numerators, uint32 tile arithmetic) below 2^31 elements and a
64-bit one from there on.  A case names ONE call on a tensor of n > 2^31 + 2^20 elements.  Its reference is the same call on chunks of
fewer than 2^31 elements each -- the 32-bit form, which the rest of the suite pins to the oracle -- cut along the leading axis at whole
rows, whole scale groups and whole blocks.  Every case has a twin just under the boundary (`under(case)`: the same tensor cut to the
largest whole-row size with n < 2^31), where the 32-bit forms run at their largest values.

The period rule.  A kernel that truncates an index to 32 bits, or drops its sign, reads element e - 2^32 or e - 2^31 in place of e.
Whatever the kernel derives from the index -- the column e % L, the channel (e / inner) % C, the scale group, the block along a
strided dimension -- has a period P, and when P divides 2^31 the wrapped index decodes to the SAME column, channel or group: scales,
masks and block boundaries all come out right and only the data differ.  So for every period P of a case 2^31 % P != 0 and
2^32 % P != 0, which rules out power-of-two row lengths and channel counts: L = 3072, 5120, 1536, 3075 and C = 96 with inner = 40
here, and row counts that are no multiple of 256.  A power-of-two BLOCK along a contiguous dimension divides 2^31 by necessity; what
counts there is the row it lies in, and the rule is applied to B * stride for strided blocks only.  The data themselves are random
without a period (never `repeat`), so a wrapped read returns other values in every case.

Not covered, on purpose:
  * bfp_cols ColsIdx.small == 0 (2^31 lane slots: tens of GiB), see tests/_strided_cases.py;
  * hist_observer.hip:98 narrow == false: needs 2^32 16-byte vectors, 64 GiB of bf16;
  * stream.hpp:452: the stream kernels' tile count beyond 32 bits, tens of GiB as well;
  * DMXQ_INPUT_HYPERNET_TILED: read once per process, so it would take a child process per case;
  * the REFUSING side of bfp.hip:387 (a member of bfp_qdq_multi with 2^30 tiles): a tile holds at least 2048 elements, so that is a
    tensor of 2^41 elements.  The case `multi_bfp` runs the accepting side with a member of more than 2^31 elements."""
from collections import namedtuple

TWO31 = 1 << 31
TWO32 = 1 << 32
MIN_N = TWO31 + (1 << 20)
GIB = 1 << 30
ITEM = {"bf16": 2, "f16": 2, "f32": 4, "i8": 1}

# name     : pytest id
# op       : key of OPS in tests/test_gpu_large_index.py
# shape    : [rows, L] or [outer, C, inner]; always cut along dim 0
# dtype    : of the big inputs; out: of the big outputs (None = dtype); extra: bytes per element of further big inputs (scores, second operand)
# p        : the format / call parameters
# unit     : chunk boundaries are multiples of `unit` indices of dim 0 (scale groups along the rows, 16-byte alignment of ragged rows)
# targets  : names from BRANCHES that the case runs
# twin     : also run just under 2^31
Case = namedtuple("Case", "name op shape dtype out extra p unit targets twin kind specials")


def case(name, op, shape, dtype="bf16", out=None, extra=0, p=None, unit=1, targets=(), twin=True, kind="heavy", specials=True):
    return Case(name, op, tuple(shape), dtype, out or dtype, extra, dict(p or {}), unit, tuple(targets), twin, kind, specials)


# every branch of csrc/ between a 32-bit and a 64-bit index form (file:line as of the commit that added this table), by the name the
# cases use
BRANCHES = (
    "elementwise.hip:make_channel_map", "stream.hpp:500 ChanIter::start", "elementwise.hip:323", "elementwise.hip:457",
    "hypernet.hip:406", "hypernet.hip:369", "hypernet.hip:459", "hypernet.hip:468", "hypernet_rows.hpp:77", "hypernet.hip:238",
    "hypernet_multi.hip:147", "bfp.hip:387", "fixed_multi.hip:62", "fixed_multi.hip:104", "fixed_multi.hip:152", "fixed_multi.hip:159",
    "bfp_urows.hip:72", "reduce.hip:486", "rope.hip:87", "topk.hip:315",
)
# kernels that index in int64_t throughout: no branch, but no index above 2^31 before these cases either
INT64_KERNELS = ("blockfmt.hip", "bfp_pack.hip", "nm_mask.hip", "dynamic_quant.hip", "hadamard.hip", "error_stats.hip", "approx.hip",
                 "lastdim.hpp", "lut16.hip", "elementwise.hip:binary", "elementwise.hip:relu", "act_cast.hip:unary", "reduce.hip:histc",
                 "reduce.hip:group_minmax", "common.hpp:rnd_unit")

A = (699405, 3072)        # 2,148,572,160 elements; 699405 = 15 * 46627 is odd
A5 = (419643, 5120)       # the same count with rows of 5120
N15 = (1398795, 1536)     # rows of 1536 (softmax / layernorm / rmsnorm)
U = (698717, 3075)        # rows that are not whole 16-byte vectors
O3 = (559600, 96, 40)     # [outer, C, inner]: channels along dim 1 with inner > 1
WIDE = (43, 3 << 24)      # 43 rows of 50,331,648: wider than the lastdim kernels' 32-bit lane offsets take
CHMAP = ("elementwise.hip:make_channel_map", "stream.hpp:500 ChanIter::start")

CASES = [
    # ---- affine integer casts and channel scaling (elementwise.hip: ChannelMap.small == 0, no run_align shortcut)
    case("fixed_lastdim_bf16", "fixed_qdq", A, p=dict(ch_axis=-1, gs=None), targets=CHMAP + ("elementwise.hip:323",)),
    case("fixed_lastdim_f32", "fixed_qdq", A, "f32", p=dict(ch_axis=-1, gs=None), targets=CHMAP + ("elementwise.hip:323",)),
    case("fixed_rowgroups_bf16", "fixed_qdq", A, p=dict(ch_axis=0, gs=15), unit=15, targets=CHMAP),
    case("fixed_axis1_bf16", "fixed_qdq", O3, p=dict(ch_axis=1, gs=None), targets=CHMAP),
    case("fixed_axis1_groups_bf16", "fixed_qdq", O3, p=dict(ch_axis=1, gs=8), targets=CHMAP),
    case("scale_mul_lastdim_bf16", "scale_channels", A5, p=dict(ch_axis=-1, divide=False), targets=CHMAP + ("elementwise.hip:457",)),
    case("scale_div_axis1_bf16", "scale_channels", O3, p=dict(ch_axis=1, divide=True), targets=CHMAP),
    case("scale_div_lastdim_f32out", "scale_channels", A, out="f32", p=dict(ch_axis=-1, divide=True), targets=CHMAP + ("elementwise.hip:457",)),
    # ---- the fused weight / input chains (hypernet.hip, hypernet_rows.hpp: HnArgs.small == 0)
    case("hypernet_dense_scale", "weight_hypernet", A, p=dict(B=64, M=0, K=0, scale=True), targets=("hypernet.hip:406",), kind="weight"),
    case("hypernet_24_scale", "weight_hypernet", A, extra=2, p=dict(B=64, M=4, K=2, scale=True, score="bf16"),
         targets=("hypernet.hip:406", "hypernet_rows.hpp:77"), kind="weight"),
    case("hypernet_24_f32score", "weight_hypernet", A, extra=4, p=dict(B=64, M=4, K=2, scale=False, score="f32"),
         targets=("hypernet.hip:406",), kind="weight"),
    case("nm_sparsify_typed", "nm_sparsify", A, extra=2, p=dict(M=4, K=2), targets=("hypernet.hip:369",)),
    case("nm_mask_28", "nm_mask", A5, p=dict(M=8, K=2), kind="uniform", specials=False),
    case("input_hypernet_lastdim", "input_hypernet", A, out="f32", p=dict(B=64)),
    case("input_hypernet_rows", "input_hypernet", A, out="f32", p=dict(B=512), targets=("hypernet.hip:468", "hypernet_rows.hpp:77")),
    case("input_hypernet_tiled", "input_hypernet", WIDE, out="f32", p=dict(B=64, col_window=64 * 64),
         targets=("hypernet.hip:459", "hypernet.hip:238"), specials=False),
    # ---- block formats
    case("sbfp_rows", "sbfp_qdq", A, p=dict(B=64)),
    case("mxfp_rows", "mxfp_qdq", A5, p=dict(B=32)),
    case("mxfp_rows_f32", "mxfp_qdq", A5, "f32", p=dict(B=32)),
    case("bfp_urows", "bfp_qdq", U, p=dict(B=64), unit=8, targets=("bfp_urows.hip:72",)),
    case("bfp_rows", "bfp_qdq", A, p=dict(B=16)),
    case("float_rows", "float_qdq", A),
    case("bfp_pack", "bfp_pack", A, out="i8", extra=2, p=dict(B=16)),
    case("dynamic_per_token", "dynamic_fixed_qdq", A, p=dict(granularity="per_token", gs=None)),
    case("dynamic_per_group", "dynamic_fixed_qdq", A, p=dict(granularity="per_group", gs=128)),
    case("hadamard_64", "hadamard_qdq", A, p=dict(H=64, B=64), kind="normal"),
    # ---- row functions and element functions
    case("softmax_1536", "softmax", N15, kind="normal"),
    case("layernorm_1536", "layernorm", N15, kind="normal", specials=False),
    case("rmsnorm_1536", "rmsnorm", N15, kind="normal", specials=False),
    case("unary_cast_gelu", "unary_cast", A, kind="normal"),
    case("unary_cast_gelu_f32", "unary_cast", A, "f32", kind="normal"),
    case("lut16_gelu", "lut16_apply", A, kind="normal"),
    case("binary_cast_add", "binary_cast", A, extra=2, kind="normal"),
    case("relu_cast", "relu_cast", A, kind="normal"),
]
BY_NAME = {c.name: c for c in CASES}

# cases with a harness of their own in tests/test_gpu_large_index.py: (name, shape, dtype, targets, peak GiB)
SPECIAL = [
    case("rope_refusal", "rope", (8, 32, 4099, 2048), targets=("rope.hip:87",), kind="normal", specials=False),
    case("topk_mask", "topk_mask", (3 * (1 << 30) + 12345,), targets=("topk.hip:315",), twin=False, kind="analytic", specials=False),
    case("channel_maxabs_plane", "channel_maxabs", A, out="f32", p=dict(ch_axis=0), targets=("reduce.hip:486",)),
    case("channel_maxabs_lastdim", "channel_maxabs", A5, out="f32", p=dict(ch_axis=-1)),
    case("channel_maxabs_axis1", "channel_maxabs", O3, out="f32", p=dict(ch_axis=1)),
    case("group_minmax_axis1", "group_minmax", O3, out="f32", p=dict(ch_axis=1, gs=8), specials=False),
    case("group_minmax_rows", "group_minmax", A, out="f32", p=dict(ch_axis=0, gs=15), unit=15, specials=False),
    case("histc", "histc", A, out="f32", p=dict(bins=2048), kind="normal", specials=False),
    case("error_stats", "error_stats", A, extra=2, kind="dyadic", specials=False),
    case("cast_error", "cast_error", A, kind="dyadic", specials=False),
    case("bernoulli_mask", "bernoulli_mask", A, kind="uniform", specials=False, twin=False),
    case("float_qdq_stochastic", "float_qdq_stochastic", A, kind="heavy", specials=False, twin=False),
    case("fixed_qdq_stochastic", "fixed_qdq_stochastic", A, kind="normal", specials=False, twin=False),
    case("multi_hypernet", "weight_hypernet_multi", A, targets=("hypernet_multi.hip:147",), kind="weight", twin=False),
    case("multi_bfp", "bfp_qdq_multi", A, targets=("bfp.hip:387",), twin=False),
    case("multi_fixed", "fixed_qdq_multi", A, p=dict(gs=15), unit=15, targets=("fixed_multi.hip:62",), twin=False),
    case("multi_float", "float_qdq_multi", A, targets=("fixed_multi.hip:104",), twin=False),
    case("multi_fixed_float", "fixed_float_qdq_multi", A, p=dict(gs=15), unit=15, targets=("fixed_multi.hip:152", "fixed_multi.hip:159"), twin=False),
]
SPECIAL_BY_NAME = {c.name: c for c in SPECIAL}
ALL = CASES + SPECIAL


def numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def row_len(c):
    """elements per index of dim 0"""
    return numel(c.shape[1:])


def under(c):
    """the twin just under the boundary: the same tensor cut to the largest whole-row (whole-group) size with n < 2^31"""
    rl = row_len(c)
    rows = (TWO31 - 1) // rl // c.unit * c.unit
    return c._replace(name=c.name + "_under", shape=(rows,) + c.shape[1:])


def chunks(c, limit=TWO31):
    """[(a, b)] along dim 0: as few chunks as keep every one below `limit` elements, boundaries at multiples of c.unit"""
    rows, rl = c.shape[0], row_len(c)
    k = 2
    while True:
        step = -(-rows // k)
        step = -(-step // c.unit) * c.unit
        if step * rl < limit:
            break
        k += 1
    return [(a, min(a + step, rows)) for a in range(0, rows, step)]


def windows(c, width=64):
    """the two oracle windows along dim 0: `width` rows straddling element 2^31 (the last `width` rows before the end for a twin under
    the boundary, shifted to whole groups) and the last `width` rows.  A case with p['col_window'] (rows too long for 64 of them) gets
    (row, first column, columns) triples: whole blocks of one row."""
    rows, rl = c.shape[0], row_len(c)
    if "col_window" in c.p:
        w, B = c.p["col_window"], c.p["B"]
        out = []
        for e in (min(TWO31, rows * rl - w // 2), rows * rl - w // 2):
            r, col = divmod(e, rl)
            c0 = max(0, min(col // B * B - w // 2, rl - w))
            out.append((r, c0, w))
        return out
    width = -(-width // c.unit) * c.unit
    mid = min(TWO31 // rl, rows - width // 2) - width // 2
    mid = max(0, mid // c.unit * c.unit)
    last = (rows - width) // c.unit * c.unit
    return [(mid, min(mid + width, rows)), (last, rows)]


def special_rows(c):
    """rows beyond the 2^31 boundary (the last rows of a twin) that get a NaN, an Inf, a denormal and an all-zero block: outside the
    straddling window, inside the last chunk"""
    rows, rl = c.shape[0], row_len(c)
    first = min(TWO31 // rl + 100, rows - 164)
    return [first + 7 * k for k in range(4)]


def periods(c):
    """every period of the case's index decode"""
    p, out = c.p, set()
    if len(c.shape) == 2:
        rows, L = c.shape
        out.add(L)
        if p.get("ch_axis") == 0:
            out.add((p.get("gs") or 1) * L)
    elif len(c.shape) == 3:
        outer, C, inner = c.shape
        out |= {C, C * inner, inner, (p.get("gs") or 1) * inner}
    elif len(c.shape) == 4:
        B, n1, n2, D = c.shape
        out |= {n2 * D, n1 * n2 * D, n2}
    if p.get("stride", 1) > 1:
        out.add(p["B"] * p["stride"])
    out.discard(1)
    return sorted(out)


def peak_bytes(c):
    """device memory a test of the case needs at once: the inputs, the full-size output, one chunk's output, and 1 GiB for the pieces in
    which inputs are generated and outputs compared"""
    n = numel(c.shape)
    big = n * (ITEM[c.dtype] + c.extra + ITEM[c.out])
    chunk = max(b - a for a, b in chunks(c)) * row_len(c)
    return big + chunk * ITEM[c.out] + GIB


# ------------------------------------------------------------------------------------------------ the harness (torch imported on use)
def torch_dtype(name):
    import torch
    return {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32, "i8": torch.int8}[name]


def device_input(kind, shape, dtype, seed, dev, piece=1 << 26):
    """a tensor WITHOUT a period, generated on the device in pieces from one seeded generator (never `repeat`):
    heavy   normal * exp(4 normal), the exponent spread of tests/_data.py make("heavy")
    weight  heavy / 10
    normal  2 * normal
    uniform U[0, 1): scores and probabilities
    dyadic  multiples of 2^-6 with magnitude below 4, which bf16 holds exactly"""
    import torch
    n = numel(shape)
    out = torch.empty(n, dtype=dtype, device=dev)
    g = torch.Generator(device=dev).manual_seed(seed)
    for s in range(0, n, piece):
        m = min(piece, n - s)
        if kind in ("heavy", "weight"):
            v = torch.randn(m, generator=g, device=dev)
            v *= torch.exp(4.0 * torch.randn(m, generator=g, device=dev))
            if kind == "weight":
                v *= 0.1
        elif kind == "normal":
            v = torch.randn(m, generator=g, device=dev) * 2.0
        elif kind == "uniform":
            v = torch.rand(m, generator=g, device=dev)
        elif kind == "dyadic":
            v = torch.randint(-255, 256, (m,), generator=g, device=dev).float() / 64.0
        else:
            raise ValueError(kind)
        out[s:s + m] = v
        del v
    return out.view(shape)


def plant_specials(x, c):
    """a NaN, an Inf, a denormal and an all-zero block, each in a row of its own beyond element 2^31 -- and, for the twins that are
    views of the same tensor, in the last rows under it (every chunk unit a case uses)"""
    x2 = x.view(x.shape[0], -1)
    sets = [special_rows(c)] + [special_rows(under(c._replace(unit=u))) for u in (1, 8, 15)]
    den = 1e-40 if x.dtype != torch_dtype("f16") else 6e-8
    for rows in sets:
        x2[rows[0], 5] = float("nan")
        x2[rows[1], 70] = float("inf")
        x2[rows[2], 128:256] = den
        x2[rows[3], 256:512] = 0.0


def mismatches_on_device(a, b, piece=1 << 27):
    """elements whose bit patterns differ, a NaN matching any NaN; compared where the tensors live, every element"""
    import torch
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    a, b = a.reshape(-1), b.reshape(-1)
    assert a.is_contiguous() and b.is_contiguous()
    it = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    if torch.equal(a.view(it), b.view(it)):
        return 0
    bad = 0
    for s in range(0, a.numel(), piece):
        x, y = a[s:s + piece], b[s:s + piece]
        d = x.view(it) != y.view(it)
        if x.is_floating_point():
            d &= ~(torch.isnan(x) & torch.isnan(y))
        bad += int(d.sum())
    return bad


def check_chunks(c, fn, xs, full, cut=None):
    """the whole-output check: `full` = fn(xs) was computed FIRST; every chunk of dim 0 is computed again on contiguous, 16-byte
    aligned views -- fewer than 2^31 elements, the 32-bit index form -- and compared with the same rows of `full`, bit for bit.
    fn(list of tensors, cut) -> tuple of tensors whose dim 0 is the inputs'; cut = (a, b)."""
    seen = 0
    for a, b in chunks(c):
        views = [t[a:b] for t in xs]
        assert all(v.is_contiguous() and v.data_ptr() % 16 == 0 and v.numel() < TWO31 for v in views), (c.name, a, b)
        part = fn(views, (a, b))
        assert len(part) == len(full)
        for k, (f, p) in enumerate(zip(full, part)):
            bad = mismatches_on_device(f[a:b], p)
            assert bad == 0, (c.name, "chunk", (a, b), "output", k, "mismatches", bad)
        seen += b - a
        del part, views
    assert seen == c.shape[0]
