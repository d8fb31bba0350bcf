"""The device HistogramObserver (csrc/hist_observer.hip: dmxq_hist_observe, dmxq_hist_qparams) against the reference's recorded
observer states (tests/golden/histogram.npz) and against tests/_hist_ref.py, the CPU copy of the host code, bit for bit: histogram,
running range, scale, zero point, and the chosen (first, last) bins.  Kernel-level cases run through both bindings.  The capture test
is the evidence that an observation and its search make no host synchronisation."""
import os

import numpy as np
import pytest
import torch

from _data import normal as _normal
from _hist_ref import HistRef

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BINDINGS = ("torch", "ctypes")


def normal(n, seed, start=0):
    return torch.from_numpy(_normal(n, seed, start)).float()


def _f32(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int32)).view(torch.float32)


def _bits(t):
    return t.detach().float().cpu().contiguous().view(torch.int32).numpy().view(np.uint32)


class Kernel:
    """observer state driven straight through one binding's front end"""

    def __init__(self, f, dev, G, bins=2048, up=128):
        self.f, self.G, self.bins, self.up = f, G, bins, up
        self.hist = torch.zeros(G, bins, device=dev)
        self.mn = torch.full((G,), float("inf"), device=dev)
        self.mx = torch.full((G,), float("-inf"), device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.scratch = torch.empty(f.hist_scratch_words(G, bins), dtype=torch.int32, device=dev)

    def observe(self, x, ch_axis=0, group_size=None):
        if group_size is None:
            x, ch_axis, group_size = x.reshape(1, -1), 0, 1
        self.f.hist_observe(x, ch_axis, group_size, self.up, self.hist, self.mn, self.mx, self.status, self.scratch)

    def qparams(self, precision, qmin, qmax, sym):
        return self.f.hist_qparams(self.hist, self.mn, self.mx, precision, qmin, qmax, sym)


@pytest.mark.parametrize("binding", BINDINGS)
def test_reference_sequences_bit_exact(dmx, cuda, binding):
    f = dmx.ops.front(binding)
    g = np.load(os.path.join(GOLD, "histogram.npz"), allow_pickle=False)
    for s in range(int(g["n_seq"])):
        fmt = dmx.Format.from_shorthand(str(g[f"seq{s}_fmt"]))
        qmin, qmax = dmx.observer.get_qmin_qmax(fmt)
        k = Kernel(f, cuda, 1)
        for b in range(int(g["n_batch"])):
            k.observe(_f32(g[f"seq{s}_x{b}"]).to(cuda))
            scale, zp = k.qparams(fmt.precision, qmin, qmax, str(g[f"seq{s}_qs"]) == "symmetric")
            assert np.array_equal(_bits(k.hist[0]), g[f"seq{s}_hist{b}"]), (s, b)
            assert np.array_equal(_bits(torch.cat([k.mn, k.mx])), g[f"seq{s}_range{b}"]), (s, b)
            assert np.array_equal(_bits(scale), g[f"seq{s}_scale{b}"]), (s, b)
            assert int(zp[0]) == int(g[f"seq{s}_zp{b}"][0]), (s, b)
    assert int(k.status[0]) == 0


def _batches(kind, shape, dtype, seed):
    n = int(np.prod(shape))
    base = [normal(n, seed, start=b * n).reshape(shape) for b in range(4)]
    scale = {"widen": [1, 3, 10, 40], "shrink": [40, 10, 3, 1], "constant": [2, 2, 2, 2], "below1": [0.1, 0.2, 0.15, 0.3],
             "onesided": [5, 6, 4, 8]}[kind]
    out = []
    for b, (x, c) in enumerate(zip(base, scale)):
        x = x * c
        if kind == "onesided":
            x = x.abs() + 0.25
        if kind == "constant" and b == 3:
            x = torch.full(shape, 1.5)
        out.append(x.to(dtype))
    return out


CASES = [
    # (kind, shape, dtype, format, symmetric qscheme, group size, ch_axis)
    ("widen", (64, 256), torch.float32, "XP[8,0](CSN)", False, None, -1),
    ("shrink", (64, 256), torch.bfloat16, "XP[4,0](CSN)", True, None, -1),
    ("below1", (64, 256), torch.float16, "XP[8,0](CSN)", False, 64, -1),
    ("onesided", (64, 256), torch.float32, "XP[4,0](CSN)", False, 128, -1),
    ("constant", (64, 256), torch.bfloat16, "XP[8,0](CSN)", True, 16, -1),
    ("widen", (256, 48), torch.float32, "XP[4,0](CSN)", True, 16, 0),
    ("onesided", (100, 40), torch.float16, "XP[8,0](CSN)", True, 64, 0),
    ("widen", (33, 7), torch.float32, "XP[8,0](CSN)", False, None, -1),
    ("onesided", (30, 20), torch.bfloat16, "XP[4,0](CSN)", True, 16, -1),
    ("below1", (128, 96), torch.bfloat16, "XP[4,0](CSN)", False, 128, 0),
    ("shrink", (96, 128), torch.float32, "XP[8,0](CSN)", True, 64, -1),
    ("widen", (32, 4, 64), torch.bfloat16, "XP[8,0](CSN)", False, None, -1),
]


@pytest.mark.parametrize("binding", BINDINGS)
def test_battery_against_host_code(dmx, cuda, binding):
    """seeded sequences through the kernels and through the host code's CPU copy: identical state, (first, last) and qparams"""
    f = dmx.ops.front(binding)
    for i, (kind, shape, dtype, fname, sym, gs, axis) in enumerate(CASES):
        fmt = dmx.Format.from_shorthand(fname)
        qmin, qmax = dmx.observer.get_qmin_qmax(fmt)
        xs = _batches(kind, shape, dtype, 1000 + i)
        slabs = (lambda x: torch.split(x, gs, dim=axis)) if gs else (lambda x: [x])
        G = len(slabs(xs[0]))
        refs = [HistRef(precision=fmt.precision, qmin=qmin, qmax=qmax, symmetric=sym) for _ in range(G)]
        k = Kernel(f, cuda, G)
        for b, x in enumerate(xs):
            k.observe(x.to(cuda), axis, gs)
            scale, zp = k.qparams(fmt.precision, qmin, qmax, sym)
            for j, (r, slab) in enumerate(zip(refs, slabs(x))):
                r(slab.float())
                rs, rz = r.calculate_qparams()
                where = (i, kind, b, j)
                assert np.array_equal(_bits(k.hist[j]), _bits(r.histogram)), where
                assert np.array_equal(_bits(torch.stack([k.mn[j], k.mx[j]])), _bits(torch.stack([r.min_val, r.max_val]))), where
                assert np.array_equal(_bits(scale[j]), _bits(rs.reshape(()))), where
                assert int(zp[j]) == int(rz.reshape(-1)[0]), where


def _calibrate(dmx, cuda, group_size, xs, capture):
    c = dmx.CastTo(format="XP[8,0](CSN)").to(cuda)
    kw = dict(group_size=group_size, ch_axis=-1) if group_size else {}
    c.enable_calibration(True, dmx.HistogramObserver, torch.per_tensor_affine, **kw)
    c(xs[0])   # eager warm-up: the state and the scratch are allocated here
    if capture:
        static = xs[0].clone()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):   # recorded, not run
            c(static)
        for x in xs[1:]:
            static.copy_(x)
            graph.replay()
    else:
        for x in xs[1:]:
            c(x)
    torch.cuda.synchronize()
    obs = c.activation_post_process
    state = [obs.histogram.clone(), obs.min_val.clone(), obs.max_val.clone(), c.scale.clone(), c.zero_point.clone()]
    c.enable_calibration(False)
    return state + [c(xs[-1])]


@pytest.mark.parametrize("group_size", [None, 128])
def test_calibration_step_captures_into_a_graph(dmx, cuda, group_size):
    """one CastTo calibration step (observe every group + search + qparams) captured with torch.cuda.graph and replayed on three more
    batches equals the eager sequence bit for bit -- the host code's .cpu() reads cannot be captured at all"""
    xs = [(normal(512 * 768, 31 + b) * (1 + 2 * b)).reshape(512, 768).to(cuda) for b in range(4)]
    eager = _calibrate(dmx, cuda, group_size, xs, capture=False)
    graphed = _calibrate(dmx, cuda, group_size, xs, capture=True)
    for a, b in zip(eager, graphed):
        assert a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                  b.view(torch.int32) if b.dtype == torch.float32 else b)
    assert eager[0].shape == ((768 // 128, 2048) if group_size else (2048,))


def test_batched_equals_per_slab(dmx, cuda):
    x = (normal(256 * 384, 5) * 3).reshape(256, 384).to(cuda)
    batched = dmx.HistogramObserver()
    slabs = [dmx.HistogramObserver() for _ in range(3)]
    for b in range(3):
        xb = x * (1 + b)
        batched(xb, 128)
        for o, s in zip(slabs, torch.split(xb, 128, dim=-1)):
            o(s)
    sb, zb = batched.calculate_qparams()
    for j, o in enumerate(slabs):
        s, z = o.calculate_qparams()
        assert torch.equal(batched.histogram[j], o.histogram)
        assert torch.equal(batched.min_val[j], o.min_val) and torch.equal(batched.max_val[j], o.max_val)
        assert torch.equal(sb[j:j + 1], s) and torch.equal(zb[j:j + 1], z)


@pytest.mark.parametrize("bad,exc", [(float("nan"), ValueError), (float("inf"), OverflowError)])
def test_non_finite_input_raises_at_the_end_of_calibration(dmx, cuda, bad, exc):
    x = (normal(64 * 256, 9)).reshape(64, 256).to(cuda)
    for gs in (None, 64):
        c = dmx.CastTo(format="XP[8,0](CSN)").to(cuda)
        c.enable_calibration(True, dmx.HistogramObserver, torch.per_tensor_affine, **(dict(group_size=gs) if gs else {}))
        c(x)
        y = x.clone()
        y[3, 70] = bad
        c(y)          # no raise here: the device path cannot raise mid-stream
        c(x)
        with pytest.raises(exc):
            c.enable_calibration(False)
        c.enable_calibration(False)   # the flag was cleared by the raise


def test_direct_entry_points_equal_the_dispatcher_ops(dmx, cuda):
    """the dispatcher-free entry points (dmxq_torch.so's dmxq_fast module) and the torch.ops.dmxq ops: the same state and qparams"""
    from dmx_compressor_amd import _backend_torch as B
    if B.FAST is None:
        pytest.skip("the torch binding was built without its direct entry points")
    x = (normal(96 * 128, 17) * 4).reshape(96, 128).to(cuda)
    out = []
    for observe, search in ((torch.ops.dmxq.hist_observe, torch.ops.dmxq.hist_qparams), (B.FAST.hist_observe, B.FAST.hist_qparams)):
        k = Kernel(dmx.ops, cuda, 4)
        for b in range(3):
            observe(x * (1 + b), -1, 32, 128, k.hist, k.mn, k.mx, k.status, k.scratch)
        out.append([k.hist, k.mn, k.mx, *search(k.hist, k.mn, k.mx, 8, -127, 127, False)])
    for a, b in zip(*out):
        assert torch.equal(a, b)
