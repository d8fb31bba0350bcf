"""The device HistogramObserver (csrc/hist_observer.hip) on every class of tests/_hist_cases.py, bit for bit against the states the
reference's own observer left after each batch (tests/golden/hist_sequences.npz; one reference observer per group slab), through both
bindings' hist_observe / hist_qparams.  Grouped cases are ONE launch for all groups.  The error sequences check the sticky status,
that the bad group's state is untouched while the other groups of that launch advance, and that the clean batches afterwards match a
reference observer that skipped the bad one.  Where the reference refuses what this repository accepts (an extremum of 2^63 and more,
DESIGN.md §8; flagged `own` in the fixture) the stored state is that of tests/_hist_ref.py.  A re-bin whose fine grid the reference
could not allocate (`down` up to 2^30) is compared with the sparse float64 re-bin of tests/_hist_cases.py."""
import functools
import os

import numpy as np
import pytest
import torch

import _hist_cases as HC
from _hist_ref import HistRef, histc as ref_histc
from test_gpu_hist_observer import BINDINGS, Kernel, _bits

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hist_sequences.npz")
NAMES = [c.name for c in HC.CASES]
MODULE_NAMES = [c.name for c in HC.CASES if c.module]


@functools.lru_cache(maxsize=None)
def gold():
    return np.load(GOLD, allow_pickle=False)


def on_device(case, x, dev):
    """the batch on the device, `case.offset` elements into its allocation (a view off the 16-byte grid when that is odd)"""
    buf = torch.empty(x.numel() + case.offset, dtype=x.dtype, device=dev)
    view = buf[case.offset:].view(x.shape)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + case.offset * x.element_size()
    return view


def qrange(dmx, case):
    fmt = dmx.Format.from_shorthand(case.fmt)
    return (fmt.precision,) + tuple(dmx.observer.get_qmin_qmax(fmt))


def assert_state(g, name, i, hist, mn, mx, scale, zp, where):
    """stored state i of a case == the device's, every group"""
    G = g[f"{name}_hist"].shape[1]
    assert np.array_equal(_bits(hist).reshape(G, -1), g[f"{name}_hist"][i]), where
    assert np.array_equal(_bits(torch.stack([mn.reshape(-1), mx.reshape(-1)], dim=1)), g[f"{name}_range"][i]), where
    assert np.array_equal(_bits(scale).reshape(-1), g[f"{name}_scale"][i]), where
    assert np.array_equal(zp.cpu().numpy().reshape(-1).astype(np.int64), g[f"{name}_zp"][i]), where


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("binding", BINDINGS)
def test_every_stored_state_bit_exact(dmx, cuda, binding, name):
    f, g, case = dmx.ops.front(binding), gold(), HC.BY_NAME[name]
    assert len(HC.CASES) == len(g["names"])
    precision, qmin, qmax = qrange(dmx, case)
    G = HC.n_groups(case)
    k = Kernel(f, cuda, G)
    stored = HC.stored_batches(case)
    exc = g[f"{name}_exc"]
    want_status = 0
    for b in range(case.nb):
        before = (k.hist.clone(), k.mn.clone(), k.mx.clone())
        k.observe(on_device(case, HC.batch(case, b), cuda), case.ch_axis, case.group_size)
        if name in HC.ERROR_CASES and b == HC.BAD_BATCH:
            want_status = HC.ERR_CODE[str(exc[b, HC.BAD_GROUP])]
            assert want_status == HC.ERR_CODE[HC.ERROR_CASES[name]]
            j = HC.BAD_GROUP     # the bad group's state is untouched ...
            assert torch.equal(k.hist[j].view(torch.int32), before[0][j].view(torch.int32))
            assert torch.equal(k.mn[j].view(torch.int32), before[1][j].view(torch.int32))
            assert torch.equal(k.mx[j].view(torch.int32), before[2][j].view(torch.int32))
            for j in range(HC.BAD_GROUP):   # ... and every other group of the launch advanced (to its reference's state: below)
                assert not torch.equal(k.hist[j], before[0][j])
        assert int(k.status[0]) == want_status, (b, "sticky status")
        if b in stored:
            scale, zp = k.qparams(precision, qmin, qmax, case.sym)
            assert_state(g, name, stored.index(b), k.hist, k.mn, k.mx, scale, zp, (name, b))


@pytest.mark.parametrize("binding", BINDINGS)
def test_beyond_int64_extrema_equal_the_host_code(dmx, cuda, binding):
    """|x| >= 2^63: the reference raises OverflowError at torch.histc(min=int(extremum)) (recorded); this repository's host code, and
    with it the kernels, accept the batch -- held here against tests/_hist_ref.py run live, batch by batch"""
    f, case = dmx.ops.front(binding), HC.BY_NAME["big63"]
    assert [str(e) for e in gold()["big63_exc"][:, 0]] == ["OverflowError"] * case.nb
    precision, qmin, qmax = qrange(dmx, case)
    ref = HC.new_ref(case, dmx.Format, dmx.observer.get_qmin_qmax)
    k = Kernel(f, cuda, 1)
    for b in range(case.nb):
        x = HC.batch(case, b)
        assert float(x.abs().max()) >= 2.0 ** 63
        k.observe(x.to(cuda))
        ref(x)
        scale, zp = k.qparams(precision, qmin, qmax, case.sym)
        rs, rz = ref.calculate_qparams()
        assert np.array_equal(_bits(k.hist[0]), _bits(ref.histogram)), b
        assert np.array_equal(_bits(torch.cat([k.mn, k.mx])), _bits(torch.stack([ref.min_val, ref.max_val]))), b
        assert np.array_equal(_bits(scale), _bits(rs)) and int(zp[0]) == int(rz.reshape(-1)[0]), b
    assert int(k.status[0]) == 0


@pytest.mark.parametrize("name", MODULE_NAMES)
def test_module_layer_reaches_the_same_states(dmx, cuda, name):
    """the cases the module layer can express (default bins and upsample rate, no view offset), through dmx.HistogramObserver and
    through CastTo.enable_calibration: the same stored states, and the cast's scale / zero point buffers"""
    g, case = gold(), HC.BY_NAME[name]
    assert len(MODULE_NAMES) == 8 and case.offset == 0
    qs = torch.per_tensor_symmetric if case.sym else torch.per_tensor_affine
    fmt = dmx.Format.from_shorthand(case.fmt)
    obs = dmx.HistogramObserver(dtype=fmt, qscheme=qs, ch_axis=case.ch_axis)
    cast = dmx.CastTo(format=case.fmt).to(cuda)
    cast.enable_calibration(True, dmx.HistogramObserver, qs, **(dict(group_size=case.group_size, ch_axis=case.ch_axis) if case.group_size else {}))
    stored = HC.stored_batches(case)
    for b in range(case.nb):
        x = HC.batch(case, b).to(cuda)
        obs(x, case.group_size)
        cast(x)
        if b in stored:
            i = stored.index(b)
            scale, zp = obs.calculate_qparams()
            assert_state(g, name, i, obs.histogram, obs.min_val, obs.max_val, scale, zp, (name, b, "observer"))
            co = cast.activation_post_process
            assert_state(g, name, i, co.histogram, co.min_val, co.max_val, cast.scale, cast.zero_point, (name, b, "CastTo"))
    obs.check_finite()
    cast.enable_calibration(False)


def _planted(n, seed, scale, lo, hi):
    from _data import make

    x = (make("normal", (n,), seed=seed).abs() * scale + lo).clamp(lo, hi)
    x[0], x[1] = lo, hi
    return x


#: (the narrow batch's range, the wide batch's range): `down` = 2^30 with start 0; 5.7 * 2^27 with start 2^39; 9.4 * 2^19 / 2.2 from a range
#: whose ends both truncate to 1
BEYOND_DENSE = [((0.0, 2.0 ** -20), (0.0, 8.0)), ((0.0, 2.0 ** -20), (-2.0, 3.7)), ((1.0, 1.0 + 2.0 ** -12), (-3.3, 6.1))]


@pytest.mark.parametrize("narrow,wide", BEYOND_DENSE)
@pytest.mark.parametrize("binding", BINDINGS)
def test_rebin_beyond_the_dense_grid_equals_the_sparse_walk(dmx, cuda, binding, narrow, wide):
    """four narrow batches (each a third wider than the one before: after three re-bins the old histogram holds rounded fractions and the
    running sum a float32 rounding residual, which every later new bin receives), then one wide batch: a fine grid of 2^31 to 2^41 cells, which neither the reference nor tests/_hist_ref.py can
    allocate; the merge kernel's re-bin against HC.sparse_rebin (held against the reference's dense grid on every re-bin of the table
    by oracle/gen_golden_hist.py), the counts against ATen's CPU torch.histc, the range against the restated plan"""
    f = dmx.ops.front(binding)
    x0 = _planted(4096, 901, (narrow[1] - narrow[0]) / 3, *narrow)
    x1 = _planted(4096, 902, (wide[1] - wide[0]) / 3, *wide)
    xs = [x0] + [_planted(4096, 903 + i, (narrow[1] - narrow[0]) / 3, narrow[0], narrow[0] + m * (narrow[1] - narrow[0]))
                 for i, m in enumerate((1.3, 1.7, 2.2))]
    ref = HistRef()
    for x in xs:
        ref(x)
    p = HC.plan(*torch.aminmax(x1), ref.min_val, ref.max_val)
    assert p["mode"] == "rebin" and HC.BINS * p["down"] >= 2 ** 31 and p["down"] <= 2 ** 30
    inc, _ = HC.sparse_rebin(ref.histogram.numpy(), HC.BINS, HC.UP, p["down"], p["start"])
    assert np.count_nonzero(inc) > HC.BINS // 2      # the residual of the float32 rounding, in every bin past the old mass
    want = ref_histc(x1, HC.BINS, int(p["lo"]), int(p["hi"])) + torch.from_numpy(inc)
    k = Kernel(f, cuda, 1)
    for x in xs:
        k.observe(x.to(cuda))
    assert np.array_equal(_bits(k.hist[0]), _bits(ref.histogram))
    k.observe(x1.to(cuda))
    assert np.array_equal(_bits(k.hist[0]), _bits(want))
    assert [float(k.mn[0]), float(k.mx[0])] == [p["lo"], p["hi"]] and int(k.status[0]) == 0
    assert float(want.sum()) > 4 * 4096   # all five batches are in the merged histogram
