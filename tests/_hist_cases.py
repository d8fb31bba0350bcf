"""The case table of the device HistogramObserver (csrc/hist_observer.hip), shared by oracle/gen_golden_hist.py (which runs the
reference's observer on it and writes tests/golden/hist_sequences.npz), tests/test_hist_cases_host.py and
tests/test_gpu_hist_cases.py.  It imports no reference and no GPU.

* CASES: sequences of batches.  No input is stored: a batch is a function of (case seed, batch index) through tests/_data.make --
  or a seeded torch.Generator for integer data -- and of operations that IEEE-754 rounds exactly (multiply, add, abs, clamp, where),
  so every machine regenerates the same bits; the fixture keeps their SHA-256.
* plan(): hist_plan restated from its comments and the reference's forward() in float32 torch scalars, and classify(): the classes a
  state belongs to.  REQUIRED is the list the table has to reach, no more and no less.
* sparse_rebin(): _combine_histograms walking only the non-zero fine cells, the running sum in float64, one rounding per new bin.
* HistRef64: tests/_hist_ref.py with the two order-free sums as the kernel takes them (float64, rounded once).
"""
import math
from collections import namedtuple

import numpy as np
import torch

from _data import make, sha256_bits
from _hist_ref import HistRef

BINS, UP = 2048, 128
MAX_CELLS = 4.0e18          # hist_plan refuses a fine grid of more cells (kernel: `q * (float)bins <= 4.0e18f`)
MAX_BINS = 8192             # kHistMaxBins
MAX_UP = 1 << 20            # the cap on upsample_rate
ERR_NAME = {0: "", 1: "OverflowError", 2: "ValueError"}    # kErrNone, kErrOverflow, kErrNan -> what int() raises on the host
ERR_CODE = {v: k for k, v in ERR_NAME.items()}

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DT_NAME = {F32: "f32", BF16: "bf16", F16: "f16"}

#: name, kind, batches, tensor dtype, shape (None: 4096 elements per tensor), ch_axis, group_size, format, symmetric qscheme, seed,
#: element offset of the device view from its allocation, every `keep`-th state stored, whether the module layer can express the case
Case = namedtuple("Case", "name kind nb dtype shape ch_axis group_size fmt sym seed offset keep module")


def _c(name, kind, nb=4, dtype=F32, shape=None, ch_axis=-1, group_size=None, fmt="XP[8,0](CSN)", sym=False, seed=0, offset=0, keep=1,
       module=False):
    return Case(name, kind, nb, dtype, shape, ch_axis, group_size, fmt, sym, seed, offset, keep, module)


ADDRUN_MAX_BATCHES = 40
#: batches of the "addrun" sequence: the generator lengthened it until add_run's first shortcut was met (tests/test_hist_cases_host.py
#: asserts that it is)
ADDRUN_BATCHES = 30

CASES = [
    _c("const_data", "const_data", seed=1, module=True),
    _c("below1", "below1", seed=2, module=True),
    _c("shrink", "shrink", seed=3, fmt="XP[4,0](CSN)", sym=True),
    _c("repeat", "repeat", seed=4, module=True),
    _c("negonly", "negonly", seed=5, sym=True, module=True),
    _c("ratio20", "ratio20", seed=6),
    _c("twovals", "twovals", seed=7),
    _c("single", "single", nb=5, seed=8),
    _c("tiny", "tiny", seed=9),
    _c("spike", "spike", seed=10, fmt="XP[4,0](CSN)"),
    _c("edges", "edges", seed=11, module=True),
    _c("posonly", "posonly", seed=12, fmt="XP[4,0](CSN)", sym=True),
    _c("sameint", "sameint", seed=13),
    _c("negfrac", "negfrac", seed=14),
    _c("ceil_over", "ceil_over", seed=15),
    _c("half", "half", seed=16),
    _c("negzero", "negzero", seed=23),
    _c("grow12", "grow", nb=12, seed=17, keep=3),
    _c("alt12", "alt", nb=12, seed=18, keep=3, sym=True),
    _c("grow24", "grow", nb=24, seed=19, keep=3, fmt="XP[4,0](CSN)"),
    _c("alt24", "alt", nb=24, seed=20, keep=3),
    _c("addrun", "addrun", nb=ADDRUN_BATCHES, seed=21, keep=3),
    _c("big63", "big63", nb=3, seed=22),
    # every precision with both qschemes
    _c("p2_aff", "widen", seed=30, fmt="XP[2,0](CSN)"),
    _c("p2_sym", "widen", seed=31, fmt="XP[2,0](CSN)", sym=True),
    _c("p4_aff", "widen", seed=32, fmt="XP[4,0](CSN)"),
    _c("p4_sym", "widen", seed=33, fmt="XP[4,0](CSN)", sym=True, module=True),
    _c("p8_aff", "widen", seed=34),
    _c("p8_sym", "widen", seed=35, sym=True),
    _c("p16_aff", "widen", seed=36, fmt="XP[16,0](CSN)"),
    _c("p16_sym", "widen", seed=37, fmt="XP[16,0](CSN)", sym=True),
    # 16-bit tensors: the device gets the 16-bit tensor, the reference the widened values
    _c("bf16_widen", "widen", seed=40, dtype=BF16, module=True),
    _c("f16_below1", "below1", seed=41, dtype=F16, fmt="XP[4,0](CSN)", sym=True),
    # groups: one launch, one reference observer per slab
    _c("g_last", "widen", seed=50, shape=(64, 64), ch_axis=-1, group_size=16, module=True),
    _c("g_first_inner", "widen", seed=51, shape=(64, 64), ch_axis=0, group_size=16, sym=True),
    _c("g_ragged_inner", "shrink", seed=52, shape=(8, 8, 64), ch_axis=1, group_size=3),
    _c("g_scalar_ragged", "widen", seed=53, shape=(64, 63), ch_axis=-1, group_size=16, fmt="XP[4,0](CSN)"),
    _c("g_offset", "widen", seed=54, shape=(64, 64), ch_axis=-1, group_size=16, offset=1),
    _c("g_bf16", "below1", seed=55, dtype=BF16, shape=(64, 64), ch_axis=-1, group_size=8),
    _c("g_bf16_offset", "widen", seed=56, dtype=BF16, shape=(64, 64), ch_axis=0, group_size=32, offset=1),
    # one launch whose four groups are in init, add, re-bin and skip at batch 2; group 3 is the one that errs
    _c("mixed_nan", "mixed_nan", nb=5, seed=60, shape=(4, 1024), ch_axis=0, group_size=1),
    _c("mixed_inf", "mixed_inf", nb=5, seed=61, shape=(4, 1024), ch_axis=0, group_size=1, sym=True),
    _c("mixed_ovf", "mixed_ovf", nb=5, seed=62, shape=(4, 1024), ch_axis=0, group_size=1),
]
BY_NAME = {c.name: c for c in CASES}
ERROR_CASES = {"mixed_nan": "ValueError", "mixed_inf": "OverflowError", "mixed_ovf": "OverflowError"}
BAD_GROUP, BAD_BATCH = 3, 2

#: what the table has to reach (classify() and case_classes())
REQUIRED = frozenset([
    "init_fresh", "init_single", "add", "rebin_down_eq_up", "rebin_down_over_ceil", "rebin_down_ge_2000",
    "start_zero", "start_pos", "start_half", "min_tie_signed_zero",
    "histc_same_int", "histc_same_int_const", "histc_neg_frac", "histc_neg_trunc",
    "err_nan", "err_inf", "err_ovf_end",
    "data_edges", "data_two_values", "data_one_element", "data_tiny", "data_spike", "data_pos", "data_neg",
    "grow12", "grow24", "alt12", "alt24",
    "p2_aff", "p2_sym", "p4_aff", "p4_sym", "p8_aff", "p8_sym", "p16_aff", "p16_sym",
    "t_bf16", "t_f16",
    "axis_first", "axis_last", "inner_gt_1", "ragged_group", "scalar_count", "misaligned_view",
    "mixed_launch", "addrun_shortcut_1",
])
KIND_CLASSES = {"edges": "data_edges", "twovals": "data_two_values", "single": "data_one_element", "tiny": "data_tiny",
                "spike": "data_spike", "posonly": "data_pos", "negonly": "data_neg"}


# ------------------------------------------------------------------------------------------------ inputs
def numel(case):
    if case.kind == "single":
        return 1
    return int(np.prod(case.shape)) if case.shape else 4096


def _plant(x, lo, hi):
    x = x.clamp(lo, hi)
    x[0], x[1] = lo, hi
    return x


def _batch32(case, b):
    """batch b of a case as a flat float32 tensor"""
    n, kind = numel(case), case.kind
    N = make("normal", (n,), seed=case.seed * 1000 + b)
    if kind == "widen":
        return N * (1, 3, 10, 40)[b]
    if kind == "shrink":
        return N * (40, 10, 3, 1)[b]
    if kind == "const_data":
        return torch.full((n,), 1.5) if b == 0 else N * (0, 3, 7, 2)[b]
    if kind == "below1":
        return N.clamp(-3, 3) * (0.1, 0.2, 0.15, 0.3)[b]
    if kind == "repeat":     # an old range of [-4, 4]: every quantity of the plan is exact, so the relaxed range is the old one
        return _plant(make("normal", (n,), seed=case.seed * 1000) * 3, -4.0, 4.0) if b < 3 else N
    if kind == "negonly":
        return -(N.abs() * (1, 2, 1.5, 3)[b] + 1.3)
    if kind == "posonly":
        return N.abs() * (5, 6, 4, 8)[b] + 0.25
    if kind == "ratio20":
        return N * (1, 20, 1, 25)[b]
    if kind == "twovals":
        hi, lo = ((3.5, -1.25), (7.25, -1.25), (0.5, 0.25), (3.5, -1.25))[b]
        return torch.where(N > 0, torch.tensor(hi), torch.tensor(lo))
    if kind == "single":
        return torch.tensor([(0.75, -2.5, 6.0, 6.0, 6.5)[b]])
    if kind == "tiny":
        return N * 1e-30 * (1, 3, 0.5, 8)[b]
    if kind == "spike":
        x = torch.zeros(n)
        x[::512] = N[::512] * (1, 3, 2, 9)[b]
        return x
    if kind == "edges":      # integers: the range is a whole number of bins per unit, every value sits on a bin edge
        g = torch.Generator().manual_seed(case.seed * 1000 + b)
        r = 8 * (1, 2, 2, 4)[b]
        return _plant(torch.randint(-r, r + 1, (n,), generator=g).float(), -float(r), float(r))
    if kind == "sameint":    # both ends of the range truncate to 2
        if b == 2:
            return torch.full((n,), 2.5)
        lo, hi = ((2.25, 2.875), (2.125, 2.9375), None, (2.25, 2.5))[b]
        return _plant(2.0 + N.abs() * 0.25, lo, hi)
    if kind == "negfrac":    # a lower end in (-1, 0): int() gives 0, truncf -0
        lo, hi = ((-0.5, 2.25), (-0.75, 3.5), (-0.25, 1.0), (-0.875, 5.0))[b]
        return _plant(N * (1, 2, 1, 3)[b], lo, hi)
    if kind == "ceil_over":
        hi = (4.0, float(np.nextafter(np.float32(4.0), np.float32(8.0))), 4.001, 4.0)[b]
        return _plant(N * 2, -4.0, hi)
    if kind == "half":       # old range [0, 1]: a fine cell is 2^-18; a new minimum of -(k + 0.5) cells, k = 4
        if b == 0:
            return _plant(N.abs() * 0.25, 0.0, 1.0)
        return _plant(N.abs() * 0.25, (-(4 + 0.5) / (BINS * UP), -0.001, -0.5)[b - 1], (1.0, 1.5, 1.0)[b - 1])
    if kind == "negzero":    # a minimum of +0 meets a running minimum of -0 and the other way round: torch.min keeps the new one
        x = N.abs() * (1, 2, 1, 3)[b] + 0.25
        x[0] = (0.0, -0.0, 0.0, -0.0)[b]
        return x
    if kind == "grow":
        return N * float(np.float32(1.3) ** b)
    if kind == "alt":
        return N * (3.0 if b % 2 else 1.0) + (0.5 * b if b % 4 == 1 else -0.25 * b if b % 4 == 3 else 0.0)
    if kind == "addrun":     # 4095 zeros and one maximum that widens the range by 5 / 128 per batch (down = 133): the earlier maxima's
        x = torch.zeros(n)   # counts are split again and again into ever smaller tail bins that follow the mass of bin 0
        x[1] = float(np.float32((1 + 5 / 128.0) ** (b - 1) * (1 + 4.5 / 128.0))) if b else 1.0
        return x
    if kind == "big63":      # |x| >= 2^63: the reference's torch.histc refuses int(extremum); this repository accepts it
        return N * (1e30, 3e30, 1e30)[b]
    if kind.startswith("mixed_"):
        x = N.reshape(4, 1024).clone()
        x[0] = torch.full((1024,), 1.5) if b < 2 else x[0] * 2                         # init at batch 2 (a single-valued range)
        x[1] = _plant(make("normal", (1024,), seed=case.seed * 1000 + 500) * 2, -4.0, 4.0) if b < 3 else x[1]   # add at batch 2
        x[2] = x[2] * (1, 2, 5, 3, 9)[b]                                                # re-bin at batch 2
        if kind == "mixed_ovf":   # old range [0, 3e38]; a maximum of 3.4e38 relaxes to an upper end past float32
            if b < BAD_BATCH:
                x[3] = _plant(x[3].abs() * 1e38, 0.0, 3.0e38)
            elif b == BAD_BATCH:
                x[3] = _plant(x[3].abs() * 1e38, 0.0, 3.4e38)
            else:
                x[3] = x[3].abs()
        elif b == BAD_BATCH:
            x[3, 70] = float("nan") if kind == "mixed_nan" else float("-inf")
        return x.reshape(-1)
    raise ValueError(kind)


def batch(case, b):
    """batch b in the case's dtype and shape (the reference gets `.float()` of it)"""
    x = _batch32(case, b)
    if case.dtype == F16:
        x = x.clamp(-65504.0, 65504.0)
    x = x.to(case.dtype)
    return x.reshape(case.shape) if case.shape and case.kind != "single" else x


def slabs(case, x):
    """the group slabs of a batch, in group order (per tensor: the tensor)"""
    return list(torch.split(x, case.group_size, dim=case.ch_axis)) if case.group_size else [x]


def n_groups(case):
    return -(-case.shape[case.ch_axis] // case.group_size) if case.group_size else 1


def stored_batches(case):
    """the batches whose states the fixture keeps: every `keep`-th and the last"""
    return [b for b in range(case.nb) if b % case.keep == case.keep - 1 or b == case.nb - 1]


def input_digest(case):
    import hashlib

    h = hashlib.sha256()
    for b in range(case.nb):
        h.update(sha256_bits(batch(case, b)).encode())
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------ the plan, restated
_f = lambda v: torch.tensor(float(v), dtype=torch.float32)


def plan(nmin, nmax, omin, omax, bins=BINS, up=UP):
    """hist_plan: mode ("skip" | "init" | "add" | "rebin"), err (an exception name or ""), the new running range (lo, hi), the histc
    range (hl, hh), down, start, and `quot` / `squot`, the float32 quotients that ceil and round were taken of"""
    nmin, nmax, omin, omax = _f(nmin), _f(nmax), _f(omin), _f(omax)
    p = dict(mode="skip", err="", lo=0.0, hi=0.0, hl=0.0, hh=0.0, down=1, start=0, quot=None, squot=None,
             fresh=bool(omin == math.inf and omax == -math.inf))
    if torch.isnan(nmin) or torch.isnan(nmax):
        return dict(p, err="ValueError")
    if torch.isinf(nmin) or torch.isinf(nmax):
        return dict(p, err="OverflowError")
    if p["fresh"] or bool(omin == omax):
        mode, lo, hi = "init", nmin, nmax
    else:
        lo, hi = torch.min(nmin, omin), torch.max(nmax, omax)
        p["tie_zero"] = bool(nmin == omin) and math.copysign(1.0, float(nmin)) != math.copysign(1.0, float(omin))
        fine = (omax - omin) / (bins * up)
        quot = (hi - lo) / (bins * fine)
        q = torch.ceil(quot)
        if torch.isnan(q):
            return dict(p, err="ValueError")
        if not (bool(q >= 1) and bool(q * _f(bins) <= _f(MAX_CELLS))):
            return dict(p, err="OverflowError")
        down = int(q.item())
        hi = hi + (down * (bins * fine) - (hi - lo))
        if torch.isinf(hi):
            return dict(p, err="OverflowError", quot=float(quot))
        squot = (omin - lo) / fine
        p.update(down=down, start=int(torch.round(squot).item()), quot=float(quot), squot=float(squot))
        mode = "add" if bool(lo == omin) and bool(hi == omax) else "rebin"
    hl, hh = float(int(lo)), float(int(hi))      # int(): toward zero, no negative zero
    same_int = hl == hh
    if same_int:
        hl, hh = float(nmin), float(nmax)
        if hl == hh:
            hl, hh = float(_f(hl - 1.0)), float(_f(hh + 1.0))
    p.update(mode=mode, lo=float(lo), hi=float(hi), hl=hl, hh=hh, same_int=same_int, const=bool(nmin == nmax))
    return p


def classify(p, up=UP):
    """the plan classes of one state"""
    if p["mode"] == "skip":
        return {"err_nan"} if p["err"] == "ValueError" else {"err_ovf_end"} if p["quot"] is not None else {"err_inf"}
    out = set()
    if p["mode"] == "init":
        out.add("init_fresh" if p["fresh"] else "init_single")
    else:
        if p["mode"] == "add":
            out.add("add")
        else:
            if p["down"] == up:
                out.add("rebin_down_eq_up")
            if p["down"] >= 2000:
                out.add("rebin_down_ge_2000")
            if 0.0 < p["quot"] - (p["down"] - 1) < 0.05:
                out.add("rebin_down_over_ceil")
        out.add("start_zero" if p["start"] == 0 else "start_pos")
        if p.get("tie_zero"):
            out.add("min_tie_signed_zero")
        if p["squot"] - math.floor(p["squot"]) == 0.5:
            out.add("start_half")
        if p["same_int"]:
            out.add("histc_same_int_const" if p["const"] else "histc_same_int")
    if not p["same_int"]:
        if -1.0 < p["lo"] < 0.0:
            out.add("histc_neg_frac")
        if p["lo"] <= -1.0 and p["lo"] != math.trunc(p["lo"]):
            out.add("histc_neg_trunc")
    return out


def case_classes(case):
    """the classes a case reaches by what it is, whatever its data"""
    out = set()
    if case.kind in KIND_CLASSES:
        out.add(KIND_CLASSES[case.kind])
    if case.kind in ("grow", "alt"):
        out.add(f"{case.kind}{case.nb}")
    if case.kind == "widen" and case.dtype == F32 and case.shape is None:
        out.add(case.name)
    if case.dtype != F32:
        out.add("t_" + DT_NAME[case.dtype])
    if case.group_size:
        nd = len(case.shape)
        axis = case.ch_axis % nd
        C, inner = case.shape[axis], int(np.prod(case.shape[axis + 1:]))
        out.add("axis_last" if case.ch_axis == -1 else "axis_first" if axis == 0 else "axis_mid")
        if inner > 1:
            out.add("inner_gt_1")
        if C % case.group_size:
            out.add("ragged_group")
        if (C * inner) % 8 or (case.group_size * inner) % 8:
            out.add("scalar_count")
        if case.offset % (16 // torch.empty(0, dtype=case.dtype).element_size()):
            out.add("misaligned_view")
    return out - {"axis_mid"}


# ------------------------------------------------------------------------------------------------ the re-bin, sparse and in float64
def sparse_rebin(old, bins, up, down, start):
    """_combine_histograms' interpolated histogram (float32 numpy, [bins]) without the dense grid: only the cells of non-zero old bins
    are walked, one float64 addition per cell as torch.cumsum(dtype=double) makes them, the running sum read at the end of every new
    bin and rounded once there.  Also returns whether some run of equal cells began with |v| < 2^(ilogb(S) - 54), S != 0: add_run's
    first shortcut."""
    old = np.asarray(old, dtype=np.float32)
    ncell = bins * down
    upto = np.zeros(bins, dtype=np.float64)
    S, j, short1 = 0.0, 0, False
    for i in np.flatnonzero(old):
        v = float(old[i])
        c = start + int(i) * up
        c1 = min(c + up, ncell)
        while c < c1:
            jj = c // down
            if jj > j:
                upto[j:jj] = S
                j = jj
            e = min((jj + 1) * down, c1)
            if S != 0.0 and abs(v) < math.ldexp(1.0, math.frexp(S)[1] - 1 - 54):
                short1 = True
            for _ in range(e - c):
                S += v
            c = e
    upto[j:] = S
    before = np.zeros(bins, dtype=np.float32)
    before[1:] = upto[:-1].astype(np.float32)
    return ((upto - before.astype(np.float64)) / float(up)).astype(np.float32), short1


# ------------------------------------------------------------------------------------------------ the host code's copy, fp64 sums
class HistRef64(HistRef):
    """tests/_hist_ref.py with torch.sum(hist) and err.sum() as the kernel takes them: float64, rounded once to float32.  A state on
    which this picks another (first, last) than HistRef is order-sensitive; the table holds none."""

    def _clip_error(self, hist, lo, hi, first, last):
        levels = 2 ** self.precision
        width = (hi - lo) / self.bins
        step = width * (last - first + 1) / levels
        if step == 0.0:
            return 0.0
        cube3 = lambda a, b: (b * b * b - a * a * a) / 3
        begin = (torch.arange(self.bins) - first) * width
        end = begin + width
        lvl_b = torch.clamp(torch.div(begin, step, rounding_mode="floor"), 0, levels - 1)
        lvl_e = torch.clamp(torch.div(end, step, rounding_mode="floor"), 0, levels - 1)
        density = hist / width
        err = torch.zeros(self.bins)
        err += density * cube3(begin - (lvl_b + 0.5) * step, torch.ones(self.bins) * (step / 2))
        err += (lvl_e - lvl_b - 1) * (density * cube3(torch.tensor(-step / 2), torch.tensor(step / 2)))
        err += density * cube3(torch.tensor(-step / 2), end - (lvl_e * step + step / 2))
        return err.double().sum().float().item()

    def search_range(self):
        hist, min_val, max_val = self.histogram, self.min_val, self.max_val
        width = (max_val - min_val) / self.bins
        total = hist.double().sum().float().item()
        csum = torch.cumsum(hist, dim=0)
        step, lo_q, hi_q = 1e-5, 0.0, 1.0
        first, last, best = 0, self.bins - 1, float("inf")
        while lo_q < hi_q:
            nlo, nhi = lo_q + step, hi_q - step
            l = min(last, max(first, int(torch.searchsorted(csum, torch.tensor(nlo * total, dtype=csum.dtype), right=False))))
            r = max(first, min(last, int(torch.searchsorted(csum, torch.tensor(nhi * total, dtype=csum.dtype), right=True)) - 1))
            nfirst, nlast = first, last
            if (l - first) > (last - r):
                nfirst, lo_q = l, nlo
            else:
                nlast, hi_q = r, nhi
            if nfirst == first and nlast == last:
                continue
            err = self._clip_error(hist, min_val.item(), max_val.item(), nfirst, nlast)
            if err > best:
                break
            best, first, last = err, nfirst, nlast
        return min_val + width * first, min_val + width * (last + 1), (first, last)


def new_ref(case, dmx_format, get_qmin_qmax, cls=HistRef):
    fmt = dmx_format.from_shorthand(case.fmt)
    qmin, qmax = get_qmin_qmax(fmt)
    return cls(precision=fmt.precision, qmin=qmin, qmax=qmax, symmetric=case.sym)
