"""The case table of the device HistogramObserver (tests/_hist_cases.py) against the reference's recorded states
(tests/golden/hist_sequences.npz, written by oracle/gen_golden_hist.py), without a GPU: the inputs regenerate to the recorded
digests, tests/_hist_ref.py reproduces every stored state bit for bit, the restated plan classifies every state and the classes
reached are exactly the list the table promises, the constants the restatement shares with the kernel are read back from the source
text, and the recorded exception names are what the restated plan's error codes stand for."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import _hist_cases as HC

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "hist_sequences.npz")
CSRC = os.path.join(os.path.dirname(HERE), "dmx-compressor_amd", "csrc")
NAMES = [c.name for c in HC.CASES]


def _bits(t):
    return t.detach().float().contiguous().reshape(-1).view(torch.int32).numpy().view(np.uint32)


@functools.lru_cache(maxsize=None)
def gold():
    return np.load(GOLD, allow_pickle=False)


@functools.lru_cache(maxsize=None)
def replay(name):
    """one run of tests/_hist_ref.py over a case, shared by the tests: per (batch, group) the restated plan and the exception raised,
    per stored batch the state and qparams, and whether a re-bin of the addrun sequence met add_run's first shortcut"""
    import dmx_compressor_amd as dmx

    case = HC.BY_NAME[name]
    G = HC.n_groups(case)
    refs = [HC.new_ref(case, dmx.Format, dmx.observer.get_qmin_qmax) for _ in range(G)]
    stored = HC.stored_batches(case)
    plans, raised, states, short1 = {}, {}, {}, False
    for b in range(case.nb):
        x = HC.batch(case, b)
        for g, slab in enumerate(HC.slabs(case, x)):
            xs = slab.float().contiguous()
            mn, mx = torch.aminmax(xs)
            r = refs[g]
            p = plans[b, g] = HC.plan(mn, mx, r.min_val, r.max_val)
            if case.kind == "addrun" and p["mode"] == "rebin":
                inc, s1 = HC.sparse_rebin(r.histogram.numpy(), HC.BINS, HC.UP, p["down"], p["start"])
                assert np.array_equal(_bits(r._rebin_onto(torch.zeros(HC.BINS), r.histogram, p["down"], p["start"])), inc.view(np.uint32))
                short1 = short1 or s1
            try:
                r(xs)
                raised[b, g] = ""
            except (ValueError, OverflowError) as e:
                raised[b, g] = type(e).__name__
            if b in stored:
                s, z = r.calculate_qparams()
                states[b, g] = (_bits(r.histogram).copy(), _bits(torch.stack([r.min_val, r.max_val])).copy(), _bits(s.reshape(1))[0],
                                int(z.reshape(-1)[0]))
    return dict(plans=plans, raised=raised, states=states, short1=short1)


def test_table_and_fixture_name_the_same_cases():
    assert list(gold()["names"]) == NAMES and len(set(NAMES)) == len(NAMES)
    for c in HC.CASES:
        assert c.nb <= 40 and HC.n_groups(c) <= 8 and HC.numel(c) <= 4096
        assert list(gold()[f"{c.name}_batches"]) == HC.stored_batches(c)
    assert os.path.getsize(GOLD) <= 865 * 1024


@pytest.mark.parametrize("name", NAMES)
def test_inputs_regenerate_to_the_recorded_digest(name):
    assert HC.input_digest(HC.BY_NAME[name]) == str(gold()[f"{name}_sha"])


@pytest.mark.parametrize("name", NAMES)
def test_hist_ref_reproduces_every_stored_state(dmx, name):
    g, case = gold(), HC.BY_NAME[name]
    states = replay(name)["states"]
    for i, b in enumerate(HC.stored_batches(case)):
        for j in range(HC.n_groups(case)):
            hist, rng, scale, zp = states[b, j]
            assert np.array_equal(hist, g[f"{name}_hist"][i, j]), (b, j)
            assert np.array_equal(rng, g[f"{name}_range"][i, j]), (b, j)
            assert scale == g[f"{name}_scale"][i, j] and zp == int(g[f"{name}_zp"][i, j]), (b, j)


@pytest.mark.parametrize("name", NAMES)
def test_recorded_exceptions_are_the_plans_error_codes(dmx, name):
    """the reference raised exactly where the restated plan skips, with the exception its error code stands for -- except from the
    first extremum of 2^63 and more on, which the reference's torch.histc refuses and this repository accepts: that
    group's later states are flagged `own` in the fixture"""
    g, case = gold(), HC.BY_NAME[name]
    rp = replay(name)
    exc, own = g[f"{name}_exc"], g[f"{name}_own"]
    stored = HC.stored_batches(case)
    for j in range(HC.n_groups(case)):
        diverged = False
        for b in range(case.nb):
            p = rp["plans"][b, j]
            assert rp["raised"][b, j] == p["err"] and HC.ERR_NAME[HC.ERR_CODE[p["err"]]] == p["err"]
            assert (p["mode"] == "skip") == bool(p["err"])
            if not diverged and str(exc[b, j]) != p["err"]:
                assert str(exc[b, j]) == "OverflowError" and max(abs(p["lo"]), abs(p["hi"])) >= 2.0 ** 63, (b, j)
                diverged = True
            if not diverged:
                assert str(exc[b, j]) == p["err"], (b, j)
            if b in stored:
                assert bool(own[stored.index(b), j]) == diverged, (b, j)
    if name in HC.ERROR_CASES:
        assert str(exc[HC.BAD_BATCH, HC.BAD_GROUP]) == HC.ERROR_CASES[name] == rp["plans"][HC.BAD_BATCH, HC.BAD_GROUP]["err"]
        assert all(rp["plans"][b, j]["err"] == "" for b in range(case.nb) for j in range(4) if (b, j) != (HC.BAD_BATCH, HC.BAD_GROUP))
    if name == "big63":
        assert str(exc[0, 0]) == "OverflowError" and bool(own.all())


def test_classes_reached_are_the_promised_list(dmx):
    reached = set()
    for c in HC.CASES:
        rp = replay(c.name)
        reached |= HC.case_classes(c)
        for b in range(c.nb):
            modes = set()
            for j in range(HC.n_groups(c)):
                p = rp["plans"][b, j]
                reached |= HC.classify(p)
                modes.add(p["mode"])
            if modes >= {"init", "add", "rebin", "skip"}:
                reached.add("mixed_launch")
        if rp["short1"]:
            reached.add("addrun_shortcut_1")
    assert reached == HC.REQUIRED, (sorted(HC.REQUIRED - reached), sorted(reached - HC.REQUIRED))
    assert int(gold()["addrun_hit"]) == 1 and HC.ADDRUN_BATCHES <= HC.ADDRUN_MAX_BATCHES


def test_half_integer_start_is_exact(dmx):
    p = replay("half")["plans"][1, 0]
    assert p["squot"] == 4.5 and p["start"] == 4 and p["mode"] == "rebin"     # torch.round: half to even


def test_shared_constants_are_the_kernels():
    src = open(os.path.join(CSRC, "hist_observer.hip")).read()
    common = open(os.path.join(CSRC, "reduce_common.hpp")).read()
    assert float(re.search(r"q \* \(float\)bins <= ([0-9.e]+)f\)", src).group(1)) == HC.MAX_CELLS
    assert int(re.search(r"constexpr int kHistMaxBins = (\d+);", common).group(1)) == HC.MAX_BINS
    assert 1 << int(re.search(r"bins > kHistMaxBins \|\| upsample_rate > \(1 << (\d+)\)", src).group(1)) == HC.MAX_UP
    codes = re.search(r"enum \{ kErrNone = (\d), kErrOverflow = (\d), kErrNan = (\d) \}", src)
    assert [HC.ERR_NAME[int(c)] for c in codes.groups()] == ["", "OverflowError", "ValueError"]
    assert HC.BINS <= HC.MAX_BINS and HC.UP <= HC.MAX_UP


@pytest.mark.parametrize("down,start", [(133, 0), (2560, 1234567), (1 << 14, 77)])
def test_sparse_rebin_equals_the_dense_grid(down, start):
    """sparse_rebin against _hist_ref's dense grid (the reference's _combine_histograms, statement by statement) on a full histogram"""
    from _data import make
    from _hist_ref import HistRef

    old = (make("normal", (HC.BINS,), seed=77 + down).abs() * 37.25).round() / 8
    start = min(start, HC.BINS * (down - HC.UP))
    dense = HistRef()._rebin_onto(torch.zeros(HC.BINS), old, down, start)
    inc, _ = HC.sparse_rebin(old.numpy(), HC.BINS, HC.UP, down, start)
    assert np.array_equal(_bits(dense), inc.view(np.uint32))
