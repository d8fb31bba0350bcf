"""The kernel classes of the row functions (softmax, LayerNorm, RMSNorm; csrc/approx.hip) restated in Python, and the case table the
tests run: for every class a call can reach, the smallest row length -- and the smallest base misalignment -- that selects it.

The restatement is written from the comments of csrc/approx.hip and csrc/row_class.hpp, NOT by asking the library:
tests/test_row_cases_host.py holds it against dmxq_row_class_of over every row length, and tests/test_gpu_row_classes.py asks the
library again with the real device pointers of every case.  No GPU is needed to import this module.

A class is the tuple RowClass(family, epl, vpl, lpr, rag, half_vec, fast32, bfpout, grid, rows_per_iter) of include/dmxq.h."""
import functools
from collections import namedtuple

F32, F16, BF16 = 0, 1, 2
SOFTMAX, LAYERNORM, RMSNORM = 0, 1, 2
OP_NAMES = {SOFTMAX: "softmax", LAYERNORM: "layernorm", RMSNORM: "rmsnorm"}
DT_NAMES = {F32: "f32", F16: "f16", BF16: "bf16"}
CAST_NONE, CAST_RANGE, CAST_GENERAL, CAST_MAN16 = 0, 1, 2, 3
UNSUPPORTED, WAVE, BLOCK, LDS_ROWS, GLOBAL_ROWS = 0, 1, 2, 3, 4
FAMILY_NAMES = {UNSUPPORTED: "unsupported", WAVE: "wave", BLOCK: "block", LDS_ROWS: "lds_rows", GLOBAL_ROWS: "global_rows"}
G_NONE, G_PERSISTENT, G_ONE_PASS, G_MID_ONE_PASS, G_MODULE_ONE_PASS, G_MODULE_ROWS4, G_CAPPED = range(7)

RowClass = namedtuple("RowClass", "family epl vpl lpr rag half_vec fast32 bfpout grid rows_per_iter")
REFUSED = RowClass(UNSUPPORTED, 0, 0, 0, 0, 0, 0, 0, G_NONE, 0)

THREADS = 256                 # a workgroup: four waves of 64
LDS_ROW_FLOATS = 16 * 1024    # the LDS fallback stages a row of up to 64 KiB of fp32
WAVE_SHAPES = [(64, v) for v in (1, 2, 3, 4, 5, 6, 8, 10, 12, 16)] + [(32, v) for v in (1, 3, 5)]   # (lanes per row, vectors per lane)
BLOCK_VPL = (2, 3, 4, 5, 6, 8)
MID_LO, MID_HI = 26 << 20, 32 << 20     # tensors of 26-32 MiB fit the chip in one round of workgroups


def full_epl(dtype):
    """elements of a 16-byte lane-vector"""
    return 4 if dtype == F32 else 8


def elem_bytes(dtype):
    return 4 if dtype == F32 else 2


def wave_shape(nv):
    """the instantiated (lanes per row, vectors per lane) with the fewest idle lane slots for a row of nv vectors; 64 lanes on a tie"""
    fits = [(lpr * vpl, -lpr, vpl) for lpr, vpl in WAVE_SHAPES if lpr * vpl >= nv]
    if not fits:
        return 64, 0
    _, neg_lpr, vpl = min(fits)
    return -neg_lpr, vpl


def rows_per_wave(vpl, epl):
    """row slots a wave handles together: about 32 fp32 values per lane, at most 4 rows"""
    q = 32 // (vpl * epl)
    return 4 if q >= 4 else (2 if q >= 2 else 1)


def wave_rows(vpl, epl, lpr):
    return (THREADS // 64) * rows_per_wave(vpl, epl) * (64 // lpr)


def bfp_lanes(block, epl, lpr):
    """lanes of one slot that hold a BFP block of `block` elements; 0 = the fused epilogue refuses the size"""
    if block < 1 or block > 512 or block % epl:
        return 0
    lpb = block // epl
    return lpb if lpb & (lpb - 1) == 0 and lpb <= lpr else 0


def _fallback(cols, cast):
    if cast:
        return REFUSED   # the fused-cast forms exist for register-resident rows only
    return RowClass(LDS_ROWS if cols <= LDS_ROW_FLOATS else GLOBAL_ROWS, 0, 0, 0, 0, 0, 0, 0, G_CAPPED, 1)


def row_class(op, dtype, rows, cols, off=0, mixed=False, cast=CAST_NONE, bfp=0):
    """The class of one call.  `off`: the bytes by which the least aligned of the call's base pointers (in, out, weight, bias) misses the
    16-byte grid; `mixed`: the output (or weight / bias) dtype differs from the input's."""
    full, eb = full_epl(dtype), elem_bytes(dtype)
    if op == SOFTMAX:
        nv = -(-cols // full)
        if mixed or off % eb or cols < full or nv > 1024:
            return _fallback(cols, cast)
        whole = cols % full == 0 and off % 16 == 0
        half = not whole and dtype != F32 and cols % 4 == 0 and cols // 4 <= 1024 and off % 8 == 0
        rag = not whole and not half
        epl = 4 if half else full
        lpr, vpl = wave_shape(cols // 4 if half else nv)
        if bfp and (not cast or rag or not bfp_lanes(bfp, epl, lpr)):
            return REFUSED
        fast32 = dtype == F32 and not rag and cast == CAST_MAN16
        return RowClass(WAVE, epl, vpl, lpr, int(rag), int(half), int(fast32), int(bool(bfp)), G_ONE_PASS, wave_rows(vpl, epl, lpr))
    if mixed:
        return _fallback(cols, cast)
    if cols % full == 0 and off % 16 == 0:
        epl = full
    elif dtype != F32 and cols % 4 == 0 and off % 8 == 0:
        epl = 4
    else:
        return _fallback(cols, cast)
    nv = cols // epl
    if epl == full and 256 < nv <= 8 * THREADS:      # long rows: a workgroup per row
        need = -(-nv // THREADS)
        vpl = need if need <= 6 else 8
        if bfp and (not cast or not bfp_lanes(bfp, epl, 64)):
            return REFUSED
        grid, rpi = G_PERSISTENT, (2 if vpl * epl <= 32 else 1)
        rpi_mid = 8 if 16 // vpl >= 8 else (4 if 16 // vpl >= 4 else 2)
        if MID_LO < rows * cols * eb <= MID_HI and not bfp:
            if cast and op == RMSNORM and vpl == 2 and epl == 8:
                grid, rpi = G_MODULE_ROWS4, 4       # the RMSNorm module on 16-bit rows of 4096
            elif not cast and rpi_mid != rpi:
                grid, rpi = G_MID_ONE_PASS, rpi_mid
        return RowClass(BLOCK, epl, vpl, THREADS, 0, 0, 0, int(bool(bfp)), grid, rpi)
    if nv <= 1024:
        lpr, vpl = wave_shape(nv)
        if bfp and (not cast or not bfp_lanes(bfp, epl, lpr)):
            return REFUSED
        grid = G_PERSISTENT
        if cast and op == LAYERNORM and not bfp and (epl, vpl, lpr) == (8, 3, 32):
            grid = G_MODULE_ONE_PASS                # the LayerNorm module on 16-bit rows of 768
        return RowClass(WAVE, epl, vpl, lpr, 0, int(epl != full), 0, int(bool(bfp)), grid, wave_rows(vpl, epl, lpr))
    return _fallback(cols, cast)


def mid_rows(dtype, cols):
    """the fewest rows that put a tensor just over 26 MiB"""
    return MID_LO // (cols * elem_bytes(dtype)) + 1


# ------------------------------------------------------------------------------------------------------------------- the sweep
SWEEP_COLS = tuple(range(1, 16513)) + (20000, 32768)


def offsets(dtype):
    """the alignment classes of a call: on the 16-byte grid, one element off (2 or 4 bytes), 4 bytes off, 8 bytes off"""
    return (0, 2, 4, 8) if dtype != F32 else (0, 4, 8)


def cast_kinds(op, dtype):
    """the fused-cast kinds that differ in class: 16-bit rows take range-only casts; float32 softmax has its FAST32 form"""
    if dtype != F32:
        return (CAST_RANGE,)
    return (CAST_GENERAL, CAST_MAN16) if op == SOFTMAX else (CAST_GENERAL,)


def forms():
    """every (op, dtype, cast kind) the table is kept for"""
    return [(op, dt, ck) for op in (SOFTMAX, LAYERNORM, RMSNORM) for dt in (F32, F16, BF16) for ck in (CAST_NONE,) + cast_kinds(op, dt)]


Case = namedtuple("Case", "op dtype cast cols off mixed rows cls")


def sweep(classify, op, dtype, cast):
    """First hit of every (class, alignment) under `classify(op, dtype, rows, cols, off, mixed, cast)` over SWEEP_COLS: a list of Case in
    the order found.  Calls of the workgroup-per-row family are asked a second time at 26 MiB (the one-pass variants)."""
    seen, out = set(), []

    def note(cols, off, mixed, rows):
        c = classify(op, dtype, rows, cols, off, mixed, cast)
        if (c, off, mixed) not in seen:
            seen.add((c, off, mixed))
            out.append(Case(op, dtype, cast, cols, off, mixed, rows, c))
        return c

    for cols in SWEEP_COLS:
        for off in offsets(dtype):
            if note(cols, off, False, 1).family == BLOCK:
                note(cols, off, False, mid_rows(dtype, cols))
        if cast == CAST_NONE:
            note(cols, 0, True, 1)
    return out


@functools.lru_cache(maxsize=None)
def table(op, dtype, cast):
    """the case table of one form: the restatement's own sweep"""
    return tuple(sweep(row_class, op, dtype, cast))


def launched(cases):
    """the cases that launch something at ordinary sizes (no refusals, no 26 MiB variants)"""
    return [c for c in cases if c.cls.family != UNSUPPORTED and c.cls.grid not in (G_MID_ONE_PASS, G_MODULE_ROWS4)]


def mid_cases(cases):
    """one case per distinct (vpl, rows per iteration) of the 26-32 MiB variants"""
    seen, out = set(), []
    for c in cases:
        if c.cls.grid in (G_MID_ONE_PASS, G_MODULE_ROWS4) and (c.cls.vpl, c.cls.rows_per_iter) not in seen:
            seen.add((c.cls.vpl, c.cls.rows_per_iter))
            out.append(c)
    return out


def row_counts(cls):
    """ragged row counts: one row, one short of a workgroup's share, two shares and three rows"""
    p = cls.rows_per_iter
    return sorted({n for n in (1, p - 1, 2 * p + 3) if n >= 1})


def bfp_blocks(cls):
    """(accepted, refused) BFP block sizes of a fused-cast class: one lane per block, 16, 64, a whole row segment (lpb == lanes per
    row; 64 lanes in the workgroup kernel); refused: twice that, and three lane-vectors (not a power of two)"""
    lanes = 64 if cls.family == BLOCK else cls.lpr
    ok = sorted({b for b in (cls.epl, 16, 64, cls.epl * lanes) if bfp_lanes(b, cls.epl, lanes)})
    return ok, [2 * cls.epl * lanes, 3 * cls.epl]


# ------------------------------------------------------------------------------------------------------ what is compiled
def instantiated(op, dtype):
    """the register-resident (epl, vpl, lpr, rag) kernel shapes csrc/approx.hip instantiates for one op and dtype (each once more per
    fused-cast / BFP form)"""
    full = full_epl(dtype)
    epls = (full,) if dtype == F32 else (full, 4)
    out = {(WAVE, e, v, l, 0) for e in epls for l, v in WAVE_SHAPES}
    if op == SOFTMAX:
        out |= {(WAVE, full, v, l, 1) for l, v in WAVE_SHAPES}
    else:
        out |= {(BLOCK, full, v, THREADS, 0) for v in BLOCK_VPL}
    return out


def shape_name(op, dtype, shape):
    fam, e, v, l, rag = shape
    return f"{OP_NAMES[op]}/{DT_NAMES[dtype]}/{FAMILY_NAMES[fam]}/E{e}/V{v}/L{l}" + ("/rag" if rag else "")


# the row lengths of the two older tests that claimed to cover every shape (tests/test_gpu_sparse_calib_approx.py
# test_softmax_layernorm_every_row_kernel_shape, tests/test_gpu_act_cast.py test_row_function_cast_contract): kept for the record of
# how many classes they reached (tests/test_row_cases_host.py prints the count)
OLD_PLAIN_COLS = (4, 8, 64, 252, 256, 264, 768, 1024, 1280, 1500, 1536, 2048, 2304, 2560, 3072, 4096, 5120, 6144, 7168, 8192, 12288, 16384,
                  777, 1501)
OLD_CAST_COLS = (8, 64, 256, 768, 1024, 1500, 1536, 2048, 4096, 197, 12 * 256, 16384)
