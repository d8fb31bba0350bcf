#!/usr/bin/env python3
"""oracle/gen_golden_hist.py — BUILD-CONTAINER ONLY.  Runs the reference's HistogramObserver (numerical/observer.py:213-583, imported
through oracle/ref_shim.py) on the case table of tests/_hist_cases.py, one reference observer per group slab, and writes
tests/golden/hist_sequences.npz: after every stored batch the bits of the histogram, the running range, the scale, the zero point,
and for every batch the name of the exception the reference raised.  The fixture is DATA produced by running the reference; inputs
are not stored, only their SHA-256.

While generating, every state (stored or not) holds three restatements against the reference, bit for bit:
  * tests/_hist_ref.py (the copy of this repository's host code) -- histogram, range, scale, zero point;
  * tests/_hist_cases.py plan() -- the range it predicts, and the exception name of its error code;
  * tests/_hist_cases.py sparse_rebin() -- on every re-bin.
The search is rerun with its two order-free sums taken in float64 and rounded once (the kernel's way).  A state where that picks
another (first, last) is ORDER-SENSITIVE; the allowed number is zero: replace the input, do not exempt it.

A group whose reference raised where this repository does not (an extremum of 2^63 and more: DESIGN.md §8) is DIVERGED from there
on; its stored states are those of tests/_hist_ref.py and are flagged `own`.

    python oracle/gen_golden_hist.py            # writes the fixture
    python oracle/gen_golden_hist.py --check    # compares a fresh run with the committed file, array by array
    python oracle/gen_golden_hist.py --addrun   # how many batches the "addrun" sequence needs for add_run's first shortcut
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import ref_shim  # noqa: E402
import _hist_cases as HC  # noqa: E402
from _hist_ref import HistRef  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "hist_sequences.npz")
MAX_BYTES = 865 * 1024          # tests/golden/histogram.npz, the largest fixture so far
DENSE_MAX_CELLS = 1 << 26       # the reference's dense grid is compared with sparse_rebin up to this many cells

ref = ref_shim.load_reference()
from dmx.compressor.numerical.observer import HistogramObserver as RefHist  # noqa: E402
from dmx.compressor.numerical.observer import _get_qmin_qmax as ref_qmin_qmax  # noqa: E402

import dmx_compressor_amd as dmx  # noqa: E402


def bits(t):
    return t.detach().float().contiguous().reshape(-1).view(torch.int32).numpy().view(np.uint32).copy()


def run_case(case, nb=None, want_states=True):
    """-> the arrays of one case, and (states checked, order-sensitive states, whether add_run's first shortcut was met)"""
    nb = nb or case.nb
    G = HC.n_groups(case)
    rfmt = ref.numerical.Format.from_shorthand(case.fmt)
    qs = torch.per_tensor_symmetric if case.sym else torch.per_tensor_affine
    refs = [RefHist(dtype=rfmt, qscheme=qs) for _ in range(G)]
    own = [HC.new_ref(case, dmx.Format, dmx.observer.get_qmin_qmax) for _ in range(G)]
    assert ref_qmin_qmax(rfmt) == (own[0].qmin, own[0].qmax)
    diverged = [False] * G
    stored = [b for b in HC.stored_batches(case._replace(nb=nb))]
    H, R, S, Z, OWN = [], [], [], [], []
    exc_names = np.zeros((nb, G), dtype="U16")
    checked = sensitive = 0
    short1 = False
    for b in range(nb):
        x = HC.batch(case, b)
        row = dict(h=[], r=[], s=[], z=[], own=[])
        for g, slab in enumerate(HC.slabs(case, x)):
            xs = slab.float().contiguous()
            mn, mx = torch.aminmax(xs)
            o = own[g]
            p = HC.plan(mn, mx, o.min_val, o.max_val)
            old_hist = o.histogram.clone()
            keep = {k: v.clone() for k, v in refs[g].state_dict().items()}
            keep.update(min_val=refs[g].min_val.clone(), max_val=refs[g].max_val.clone())
            name = ""
            try:
                refs[g](xs)
            except (ValueError, OverflowError) as e:
                name = type(e).__name__
                # a reference observer that skipped this batch (its init branch copies the range before torch.histc raises)
                refs[g].histogram.copy_(keep["histogram"])
                refs[g].min_val, refs[g].max_val = keep["min_val"], keep["max_val"]
            own_name = ""
            try:
                o(xs)
            except (ValueError, OverflowError) as e:
                own_name = type(e).__name__
            exc_names[b, g] = name
            assert own_name == p["err"], (case.name, b, g, own_name, p["err"])
            if name != own_name:
                # the one divergence: int(extremum) does not fit torch.histc's int64 bounds
                assert name == "OverflowError" and own_name == "" and max(abs(p["lo"]), abs(p["hi"])) >= 2.0 ** 63, (case.name, b, g, name)
                diverged[g] = True
            if not own_name:
                assert (p["lo"], p["hi"]) == (float(o.min_val), float(o.max_val)), (case.name, b, g, "plan range")
            if case.kind == "half" and b == 1:
                assert p["squot"] == 4.5 and p["start"] == 4, p
                rq = (keep["min_val"] - torch.min(mn, keep["min_val"])) / ((keep["max_val"] - keep["min_val"]) / (HC.BINS * HC.UP))
                assert float(rq) == 4.5, "the reference's quotient is not the half-integer"
            if p["mode"] == "rebin":
                inc, s1 = HC.sparse_rebin(old_hist.numpy(), HC.BINS, HC.UP, p["down"], p["start"])
                short1 = short1 or (s1 and case.kind == "addrun")
                if HC.BINS * p["down"] <= DENSE_MAX_CELLS:
                    dense = o._rebin_onto(torch.zeros(HC.BINS), old_hist, p["down"], p["start"])
                    assert np.array_equal(bits(dense), inc.view(np.uint32)), (case.name, b, g, "sparse re-bin")
            if not diverged[g]:
                assert np.array_equal(bits(o.histogram), bits(refs[g].histogram)), (case.name, b, g, "histogram")
                assert np.array_equal(bits(torch.stack([o.min_val, o.max_val])), bits(torch.stack([refs[g].min_val, refs[g].max_val]))), \
                    (case.name, b, g, "range")
            if b in stored and want_states:
                os_, oz = o.calculate_qparams()
                first_last = o.search_range()[2] if not o._uninitialised() else None
                o64 = HC.new_ref(case, dmx.Format, dmx.observer.get_qmin_qmax, cls=HC.HistRef64)
                o64.histogram, o64.min_val, o64.max_val = o.histogram, o.min_val, o.max_val
                if first_last is not None and o64.search_range()[2] != first_last:
                    sensitive += 1
                    print(f"ORDER-SENSITIVE: {case.name} batch {b} group {g}")
                if not diverged[g]:
                    rs, rz = refs[g].calculate_qparams()
                    assert np.array_equal(bits(os_), bits(rs)) and int(oz.reshape(-1)[0]) == int(rz.reshape(-1)[0]), (case.name, b, g, "qparams")
                    src = refs[g]
                else:
                    rs, rz, src = os_, oz, o
                checked += 1
                row["h"].append(bits(src.histogram))
                row["r"].append(bits(torch.stack([src.min_val.reshape(()), src.max_val.reshape(())])))
                row["s"].append(bits(rs.reshape(1))[0])
                row["z"].append(int(rz.reshape(-1)[0]))
                row["own"].append(int(diverged[g]))
        if b in stored and want_states:
            H.append(np.stack(row["h"])); R.append(np.stack(row["r"])); S.append(np.array(row["s"], dtype=np.uint32))
            Z.append(np.array(row["z"], dtype=np.int64)); OWN.append(np.array(row["own"], dtype=np.uint8))
    out = {}
    if want_states:
        n = case.name
        out = {f"{n}_hist": np.stack(H), f"{n}_range": np.stack(R), f"{n}_scale": np.stack(S), f"{n}_zp": np.stack(Z),
               f"{n}_own": np.stack(OWN), f"{n}_batches": np.array(stored, dtype=np.int64), f"{n}_exc": exc_names,
               f"{n}_sha": np.array(HC.input_digest(case))}
    return out, (checked, sensitive, short1)


def addrun_search():
    case = HC.BY_NAME["addrun"]
    for nb in range(2, HC.ADDRUN_MAX_BATCHES + 1):
        try:
            _, (_, _, hit) = run_case(case, nb=nb, want_states=False)
        except Exception as e:   # the sequence left what the reference accepts
            print(f"addrun: {nb} batches: {type(e).__name__}: {e}")
            return
        if hit:
            print(f"addrun: add_run's first shortcut is met with {nb} batches")
            return
    print(f"addrun: not met within {HC.ADDRUN_MAX_BATCHES} batches")


def generate():
    store, checked, sensitive = {}, 0, 0
    for case in HC.CASES:
        arrays, (c, s, hit) = run_case(case)
        if case.kind == "addrun":
            assert hit, "the addrun sequence no longer meets add_run's first shortcut"
            store["addrun_hit"] = np.array(1)
        store.update(arrays)
        checked += c
        sensitive += s
        print(f"{case.name}: {c} states")
    store["names"] = np.array([c.name for c in HC.CASES])
    print(f"{checked} states stored; order-sensitive states: {sensitive}")
    assert sensitive == 0, "replace the order-sensitive inputs"
    return store


def main():
    store = generate()
    if "--check" in sys.argv:
        old = np.load(OUT, allow_pickle=False)
        assert sorted(old.files) == sorted(store), "the committed fixture holds other arrays"
        for k in sorted(store):
            assert old[k].dtype == np.asarray(store[k]).dtype and np.array_equal(old[k], store[k]), f"{k} differs from the committed fixture"
        print(f"--check: {len(store)} arrays equal {os.path.relpath(OUT, ROOT)}")
        return
    np.savez_compressed(OUT, **store)
    size = os.path.getsize(OUT)
    print(f"wrote {os.path.relpath(OUT, ROOT)}: {size} bytes")
    assert size <= MAX_BYTES, "thin the long sequences (Case.keep) before dropping classes"


if __name__ == "__main__":
    if "--addrun" in sys.argv:
        addrun_search()
    else:
        main()
