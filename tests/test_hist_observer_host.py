"""The device HistogramObserver without a GPU: the C ABI's argument checks of dmxq_hist_observe / dmxq_hist_qparams, the front end's
refusal of CPU tensors, and the CPU restatement of the host code (tests/_hist_ref.py) against the reference's own recorded observer
states (tests/golden/histogram.npz), which pins that copy for the GPU tests."""
import ctypes
import os

import numpy as np
import pytest
import torch

from _hist_ref import HistRef

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _bits(t):
    return t.detach().cpu().contiguous().float().view(torch.int32).numpy().view(np.uint32)


def _f32(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int32)).view(torch.float32)


def test_hist_entry_points_reject_bad_arguments_without_gpu(dmx):
    L = dmx._lib.lib()
    lib = dmx._lib
    null = ctypes.c_void_p(None)
    one = ctypes.c_void_p(16)
    big = 1 << 40

    def observe(in_=one, dt=lib.F32, outer=4, C=64, inner=1, gs=16, bins=2048, up=128, state=one, status=one, scratch=one, nbytes=big):
        return L.dmxq_hist_observe(in_, dt, outer, C, inner, gs, bins, up, state, state, state, status, scratch, nbytes, null)

    assert observe(in_=null, outer=0, state=null, status=null, scratch=null) == lib.OK     # an empty observation: nothing to do
    assert observe(dt=7) == lib.ERR_BAD_ARG
    assert observe(gs=0) == lib.ERR_BAD_ARG
    assert observe(bins=0) == lib.ERR_BAD_ARG
    assert observe(up=0) == lib.ERR_BAD_ARG
    assert observe(outer=-1) == lib.ERR_BAD_ARG
    assert observe(bins=8193) == lib.ERR_UNSUPPORTED                                         # more bins than the LDS counters hold
    assert observe(in_=null) == lib.ERR_BAD_ARG
    assert observe(state=null) == lib.ERR_BAD_ARG
    assert observe(status=null) == lib.ERR_BAD_ARG
    assert observe(scratch=null) == lib.ERR_BAD_ARG
    assert observe(nbytes=(2 + 2048) * 4 * 4 - 1) == lib.ERR_BAD_ARG                          # scratch below (2 + bins) * G words
    assert observe(C=65536 * 16 + 1) == lib.ERR_UNSUPPORTED                                   # > 65535 groups

    def search(hist=one, G=4, bins=2048, precision=8, qmin=-128, qmax=127, out=one):
        return L.dmxq_hist_qparams(hist, hist, hist, G, bins, precision, qmin, qmax, 0, out, out, null)

    assert search(hist=null, G=0, out=null) == lib.OK
    assert search(G=-1) == lib.ERR_BAD_ARG
    assert search(bins=0) == lib.ERR_BAD_ARG
    assert search(precision=0) == lib.ERR_BAD_ARG
    assert search(precision=25) == lib.ERR_BAD_ARG
    assert search(qmin=3, qmax=3) == lib.ERR_BAD_ARG
    assert search(bins=8193) == lib.ERR_UNSUPPORTED
    assert search(hist=null) == lib.ERR_BAD_ARG
    assert search(out=null) == lib.ERR_BAD_ARG


def test_hist_front_end_refuses_cpu_tensors(dmx):
    x = torch.zeros(16)
    with pytest.raises(dmx._lib.DmxqError):
        dmx.ops.hist_observe(x, 0, 1, 128, torch.zeros(2048), torch.zeros(()), torch.zeros(()), torch.zeros(1, dtype=torch.int32),
                             torch.zeros(4100, dtype=torch.int32))
    with pytest.raises(dmx._lib.DmxqError):
        dmx.ops.hist_qparams(torch.zeros(2048), torch.zeros(1), torch.zeros(1), 8, -128, 127, False)
    assert dmx.ops.hist_scratch_words(6, 2048) == 6 * 2050


def test_observer_keeps_the_host_code_for_what_the_kernels_do_not_take(dmx, monkeypatch):
    obs = dmx.HistogramObserver()
    assert not obs.device_path_ok(torch.zeros(4, 4))                          # a CPU tensor: never the device path
    assert not dmx.HistogramObserver(bins=8193).device_path_ok(torch.zeros(4, 4))
    monkeypatch.setenv("DMXQ_HIST_HOST", "1")
    assert dmx.observer.hist_host_forced()
    monkeypatch.setenv("DMXQ_HIST_HOST", "0")
    assert not dmx.observer.hist_host_forced()
    # nothing observed: the reference's defaults, and no flag to raise
    scale, zp = obs.calculate_qparams()
    assert float(scale) == 1.0 and int(zp) == 0
    obs.check_finite()


def test_hist_ref_reproduces_the_reference_sequences(dmx):
    """tests/_hist_ref.py, fed the recorded batches, ends every batch in the reference's recorded state (histogram, running range)
    and with its (scale, zero point): the copy of the host code is exact on the CPU it runs on."""
    g = np.load(os.path.join(GOLD, "histogram.npz"), allow_pickle=False)
    for s in range(int(g["n_seq"])):
        fmt = dmx.Format.from_shorthand(str(g[f"seq{s}_fmt"]))
        qmin, qmax = dmx.observer.get_qmin_qmax(fmt)
        ref = HistRef(precision=fmt.precision, qmin=qmin, qmax=qmax, symmetric=str(g[f"seq{s}_qs"]) == "symmetric")
        for b in range(int(g["n_batch"])):
            ref(_f32(g[f"seq{s}_x{b}"]))
            assert np.array_equal(_bits(ref.histogram), g[f"seq{s}_hist{b}"]), (s, b)
            assert np.array_equal(_bits(torch.stack([ref.min_val, ref.max_val])), g[f"seq{s}_range{b}"]), (s, b)
            scale, zp = ref.calculate_qparams()
            assert np.array_equal(_bits(scale.reshape(1)), g[f"seq{s}_scale{b}"]), (s, b)
            assert int(zp.reshape(-1)[0]) == int(g[f"seq{s}_zp{b}"][0]), (s, b)
