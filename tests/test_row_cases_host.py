"""No GPU: the Python restatement of the row-kernel selection (tests/_row_cases.py) against the library's own answer
(dmxq_row_class_of, the function softmax_dispatch / norm_dispatch decide with; a host function that launches nothing), over every
row length from 1 to 16512 and {20000, 32768}, the three dtypes, every op form and every alignment class; the case table against
the set of classes that sweep reaches; and the kernel shapes that are compiled but can never be selected, by name."""
import ctypes

import pytest

import _row_cases as R


def _asker(dmx):
    """classify(op, dtype, rows, cols, off, mixed, cast, bfp=0) through the library, with made-up base addresses (never dereferenced)"""
    L, lib = dmx._lib.lib(), dmx._lib
    cls = lib.RowClass()
    ref = ctypes.byref(cls)
    other = {R.F32: R.BF16, R.F16: R.F32, R.BF16: R.F16}

    def classify(op, dtype, rows, cols, off, mixed, cast, bfp=0):
        if op == R.SOFTMAX:   # the views of input and output start `off` bytes into their buffers
            args = (op, dtype, other[dtype] if mixed else dtype, dtype, rows, cols, 0x100000 + off, 0x500000 + off, None, None)
        elif mixed == "out":  # a norm whose OUTPUT dtype differs (parameters in the input's dtype, or none)
            args = (op, dtype, other[dtype], dtype, rows, cols, 0x100000 + off, 0x500000, 0x900000 if off else None, None)
        else:                 # weight and bias are views `off` bytes off the grid; mixed: parameters of another dtype
            args = (op, dtype, dtype, other[dtype] if mixed else dtype, rows, cols, 0x100000, 0x500000, 0x900000 + off,
                    0xA00000 + off if op == R.LAYERNORM else None)
        assert L.dmxq_row_class_of(*args, cast, bfp, ref) == lib.OK
        return R.RowClass(*cls.key())

    return classify


@pytest.fixture(scope="module")
def swept(dmx):
    """{form: cases} from ONE pass of the library over the sweep, every answer compared with the restatement on the way"""
    ask = _asker(dmx)

    def both(op, dtype, rows, cols, off, mixed, cast):
        got, want = ask(op, dtype, rows, cols, off, mixed, cast), R.row_class(op, dtype, rows, cols, off, mixed, cast)
        assert got == want, (R.OP_NAMES[op], R.DT_NAMES[dtype], rows, cols, off, mixed, cast, got, want)
        return got

    return {form: tuple(R.sweep(both, *form)) for form in R.forms()}


def test_restatement_equals_the_library_and_the_table_equals_the_reachable_classes(swept):
    for form, cases in swept.items():
        assert cases == R.table(*form), form      # same classes, same first row length and misalignment, same order
        assert R.launched(cases) or form[2] != R.CAST_NONE


def test_element_misaligned_bases_and_mixed_output_norms(dmx):
    """outside the table (no tensor can be made that way, or nothing new to launch): a base that is not even element aligned -- an odd
    byte offset, and 2 bytes on float32 -- sends softmax and the norms to the fallbacks, or refuses the fused forms; so does a norm whose
    output dtype differs from its input's.  Restatement against library on every row length of the sweep."""
    ask = _asker(dmx)
    n_fallback = 0
    for op, dtype, cast in R.forms():
        odd = (1, 3, 7, 9, 15) + ((2, 6) if dtype == R.F32 else ())
        for cols in R.SWEEP_COLS:
            for off in odd:
                got = ask(op, dtype, 1, cols, off, False, cast)
                assert got == R.row_class(op, dtype, 1, cols, off, False, cast), (op, dtype, cols, off, cast, got)
                assert got.family in ((R.UNSUPPORTED,) if cast else (R.LDS_ROWS, R.GLOBAL_ROWS)), (op, dtype, cols, off, cast, got)
                n_fallback += 1
            if op != R.SOFTMAX and cast == R.CAST_NONE:
                for off in (0, 8):
                    got = ask(op, dtype, 1, cols, off, "out", cast)
                    assert got == R.row_class(op, dtype, 1, cols, off, True, cast) and got.family in (R.LDS_ROWS, R.GLOBAL_ROWS), (op, dtype, cols, off, got)
    assert n_fallback > 100000


def test_enum_values_and_argument_checks(dmx):
    L, lib = dmx._lib.lib(), dmx._lib
    assert (lib.ROW_SOFTMAX, lib.ROW_LAYERNORM, lib.ROW_RMSNORM) == (R.SOFTMAX, R.LAYERNORM, R.RMSNORM)
    assert (lib.ROWCAST_NONE, lib.ROWCAST_RANGE, lib.ROWCAST_GENERAL, lib.ROWCAST_MAN16) == (R.CAST_NONE, R.CAST_RANGE, R.CAST_GENERAL, R.CAST_MAN16)
    assert (lib.ROWK_UNSUPPORTED, lib.ROWK_WAVE, lib.ROWK_BLOCK, lib.ROWK_LDS_ROWS, lib.ROWK_GLOBAL_ROWS) == (R.UNSUPPORTED, R.WAVE, R.BLOCK, R.LDS_ROWS, R.GLOBAL_ROWS)
    assert (lib.ROWGRID_NONE, lib.ROWGRID_PERSISTENT, lib.ROWGRID_ONE_PASS, lib.ROWGRID_MID_ONE_PASS, lib.ROWGRID_MODULE_ONE_PASS,
            lib.ROWGRID_MODULE_ROWS4, lib.ROWGRID_CAPPED) == (R.G_NONE, R.G_PERSISTENT, R.G_ONE_PASS, R.G_MID_ONE_PASS, R.G_MODULE_ONE_PASS,
                                                             R.G_MODULE_ROWS4, R.G_CAPPED)
    cls = lib.RowClass()
    ref, p = ctypes.byref(cls), 0x100000
    ok = (R.SOFTMAX, R.BF16, R.BF16, R.BF16, 4, 256, p, p, None, None, R.CAST_NONE, 0)
    assert L.dmxq_row_class_of(*ok, ref) == lib.OK and cls.family == R.WAVE      # in == out: an in-place call has the same class
    for pos, bad in ((0, 3), (0, -1), (1, 7), (2, 7), (4, 0), (5, 0), (10, 4), (10, -1), (11, -1), (11, 16)):   # (11, 16): BFP without a cast
        args = list(ok)
        args[pos] = bad
        assert L.dmxq_row_class_of(*args, ref) == lib.ERR_BAD_ARG, (pos, bad)
    assert L.dmxq_row_class_of(*ok, None) == lib.ERR_BAD_ARG
    assert L.dmxq_row_class_of(R.LAYERNORM, R.BF16, R.BF16, 9, 4, 256, p, p, p, None, R.CAST_NONE, 0, ref) == lib.ERR_BAD_ARG


def test_fused_bfp_block_sizes(dmx, swept):
    """the *_cast_bfp entries: which block sizes a class takes (a power-of-two number of lane-vectors inside one slot of a row's lanes),
    restatement against library for every fused-cast class of the table"""
    ask = _asker(dmx)
    n, fused32 = 0, set()
    for form, cases in swept.items():
        if form[2] == R.CAST_NONE:
            continue
        for c in cases:
            for B in (1, 2, 4, 8, 12, 16, 24, 32, 48, 64, 128, 256, 384, 512, 1024):
                got = ask(c.op, c.dtype, c.rows, c.cols, c.off, c.mixed, c.cast, B)
                assert got == R.row_class(c.op, c.dtype, c.rows, c.cols, c.off, c.mixed, c.cast, B), (c, B, got)
                if c.cls.family == R.UNSUPPORTED or c.cls.rag:
                    assert got == R.REFUSED, (c, B)
                n += got.bfpout
                if got.bfpout and (c.op, c.dtype) == (R.SOFTMAX, R.F32):
                    fused32.add((got.lpr, got.vpl, got.fast32))
            if c.cls.family != R.UNSUPPORTED and not c.cls.rag:
                ok, refused = R.bfp_blocks(c.cls)
                assert ok and all(ask(c.op, c.dtype, c.rows, c.cols, c.off, c.mixed, c.cast, B).bfpout == 1 for B in ok), c
                assert all(ask(c.op, c.dtype, c.rows, c.cols, c.off, c.mixed, c.cast, B) == R.REFUSED for B in refused), c
    assert n > 1000
    # float32 softmax has TWO fused-BFP instantiations per shape, with and without FAST32: the cast kinds of R.cast_kinds, over which
    # tests/test_gpu_row_classes.py runs its BFP forms, reach both for every shape
    assert fused32 == {(lpr, vpl, f) for lpr, vpl in R.WAVE_SHAPES for f in (0, 1)}


# Compiled, never selected: full-width (16-byte) lane-vectors with more than 256 vectors per row always take the workgroup-per-row
# kernel of the norms, so the wave kernel's 64-lane shapes with 5 and more vectors per lane are dead there (each exists once more per
# fused-cast and fused-BFP form).  A dispatch change that makes one reachable -- or strands another shape -- fails here.
UNREACHABLE = sorted(f"{op}/{dt}/wave/E{e}/V{v}/L64" for op in ("layernorm", "rmsnorm") for dt, e in (("f32", 4), ("f16", 8), ("bf16", 8))
                     for v in (5, 6, 8, 10, 12, 16))


def test_unreachable_instantiations_are_the_listed_ones(swept):
    dead = []
    for op in (R.SOFTMAX, R.LAYERNORM, R.RMSNORM):
        for dt in (R.F32, R.F16, R.BF16):
            reached = {(c.cls.family, c.cls.epl, c.cls.vpl, c.cls.lpr, c.cls.rag) for form, cases in swept.items() if form[:2] == (op, dt)
                       for c in cases if c.cls.family in (R.WAVE, R.BLOCK)}
            have = R.instantiated(op, dt)
            assert reached <= have, (op, dt, sorted(reached - have))     # the dispatch never names a shape that is not compiled
            dead += [R.shape_name(op, dt, s) for s in have - reached]
    assert sorted(dead) == UNREACHABLE


def _distinct(cases):
    return {(c.dtype, c.cls) for c in cases if c.cls.family != R.UNSUPPORTED}


def test_the_table_reaches_more_than_the_older_row_lengths(dmx, swept, capsys):
    """How many classes the row lengths of the two older "every kernel shape" tests reach (aligned, contiguous tensors of up to 130
    rows, as those tests make them), against the table -- printed for the record, and the table must hold every one of theirs."""
    ask = _asker(dmx)
    lines = []
    for op in (R.SOFTMAX, R.LAYERNORM, R.RMSNORM):
        for fused in (False, True):
            if op == R.RMSNORM and not fused:
                continue    # (the older tests run rms_norm only in its fused form)
            forms = [f for f in swept if f[0] == op and (f[2] != R.CAST_NONE) == fused]
            old = {(f[1], ask(op, f[1], 7, cols, 0, False, f[2])) for f in forms for cols in (R.OLD_CAST_COLS if fused else R.OLD_PLAIN_COLS)}
            old = {(dt, c) for dt, c in old if c.family != R.UNSUPPORTED}
            new = set().union(*(_distinct(swept[f]) for f in forms))
            assert old <= new and len(old) < len(new)
            lines.append(f"{R.OP_NAMES[op]}{', fused cast' if fused else ''}: reachable classes {len(new)}, reached by the older row lengths {len(old)}")
    with capsys.disabled():
        print("\n" + "\n".join(lines))
