"""CPU-side tests (-m "not gpu") of the block-Hadamard rotation: the float32 restatement tests/_hadamard_ref.py (the checker of
tests/test_gpu_hadamard.py) against the dense Sylvester matrix in float64, and the host-side vocabulary -- the "hadamard" key of
CastTo.set_pre_transform, format_sweep's labels."""
import copy
import pickle

import pytest
import torch

import _hadamard_ref as R
from _data import make


@pytest.mark.parametrize("kind", ["normal", "heavy", "outlier"])
@pytest.mark.parametrize("H", R.SIZES)
def test_rotate_ref_against_the_dense_matrix(H, kind):
    """per block |ref - exact| <= (k + 2) 2^-24 sqrt(H) max|x| (_hadamard_ref.rotation_bound); applying it twice gives x back within
    twice that bound (R is its own inverse)"""
    x = make(kind, (37, 2 * H), seed=H, block=H)
    ref = R.rotate_ref(x, H)
    assert ref.dtype == torch.float32 and ref.shape == x.shape
    exact = (x.double().reshape(37, 2, H) @ R.sylvester(H)).reshape(37, 2 * H)
    bound = R.rotation_bound(x, H)
    err = (ref.double() - exact).abs().reshape(37, 2, H)
    worst = float((err / bound).max())
    print(H, kind, "worst error / bound", worst)
    assert bool((err <= bound).all()), worst
    back = R.rotate_ref(ref, H)
    err2 = (back.double() - x.double()).abs().reshape(37, 2, H)
    print(H, kind, "worst round-trip error / (2 x bound)", float((err2 / (2 * bound)).max()))
    assert bool((err2 <= 2 * bound).all())


def test_rotate_ref_is_the_stated_butterfly():
    """the vectorised form against the definition spelled as loops, bit for bit (H = 8 and 32)"""
    import numpy as np
    for H in (8, 32):
        x = make("heavy", (3, H), seed=5, block=H)
        want = x.numpy().astype(np.float32).copy()
        for row in want:
            s = 1
            while s < H:
                old = row.copy()
                for i in range(H):
                    if not i & s:
                        row[i] = np.float32(old[i] + old[i + s])
                        row[i + s] = np.float32(old[i] - old[i + s])
                s *= 2
            row *= R.scale_of(H)
        assert np.array_equal(R.rotate_ref(x, H).numpy().view(np.int32), want.view(np.int32))


def test_set_pre_transform_hadamard(dmx):
    c = dmx.CastTo(format="BFP[8|8]{16}(SN)")
    for bad in (48, 4, 512, 64.0, True, "64"):
        with pytest.raises(ValueError):
            c.set_pre_transform({"hadamard": bad})
        with pytest.raises(ValueError):
            c.set_pre_transform({"hadamard": {"size": bad}})
    with pytest.raises(ValueError):
        c.set_pre_transform({"hadamard": {"size": 64, "inverse": 1}})
    with pytest.raises(ValueError):
        c.set_pre_transform({"hadamard": {"size": 64, "transpose": True}})
    with pytest.raises(ValueError):
        c.set_pre_transform({"hadamard": {"inverse": False}})
    c.set_pre_transform({"hadamard": 64})
    assert c.pre_transform == {"hadamard": {"size": 64, "inverse": True}}
    c.set_pre_transform({"hadamard": {"size": 128, "inverse": False}, "format": "FP[1|5|2,15](FN)"})
    assert c.pre_transform["hadamard"] == {"size": 128, "inverse": False}
    assert isinstance(c.pre_transform["format"], dmx.Format)
    c.set_pre_transform({"hadamard": {"size": 32}})
    assert c.pre_transform == {"hadamard": {"size": 32, "inverse": True}}
    for clone in (copy.deepcopy(c), pickle.loads(pickle.dumps(c))):
        assert clone.pre_transform == {"hadamard": {"size": 32, "inverse": True}} and clone.pre_transform is not c.pre_transform
    # the seam DmxModule.configure uses
    m = dmx.nn.Linear(64, 8)
    m.configure({"weight_format": "MXFP4[E2M1]{32}", "pre_weight_transform": {"hadamard": 64}})
    assert m.weight_cast.pre_transform == {"hadamard": {"size": 64, "inverse": True}}
    with pytest.raises(ValueError):
        m.configure({"pre_weight_transform": {"hadamard": 48}})


def test_front_end_validation_without_gpu(dmx):
    x = torch.zeros(4, 96)
    for size in (48, 4, 512):
        with pytest.raises(ValueError):
            dmx.ops.hadamard(x, size)
        with pytest.raises(ValueError):
            dmx.ops.hadamard_qdq(x, size, "BFP[8|8]{16}(SN)")
    with pytest.raises(dmx.DmxqError):      # a CPU tensor, as everywhere else
        dmx.ops.hadamard(x, 32)
    with pytest.raises(dmx.DmxqError):
        dmx.ops.hadamard_qdq(x, 32, "BFP[8|8]{16}(SN)")
    assert dmx.ops.gptq_fields(dmx.Format.from_shorthand("MXFP4[E2M1]{32}")) is None   # GPTQ / cast_error routing is unchanged


def test_c_abi_argument_validation(dmx):
    """dmxq_hadamard_qdq's status codes, before anything is launched (no GPU needed)"""
    import ctypes
    lib = dmx._lib
    L = lib.lib()
    null, one = ctypes.c_void_p(None), ctypes.c_void_p(4096)

    def fmt(*v):
        return ctypes.byref(lib.GptqFormat(*v))

    bfp = (lib.GPTQ_BFP, 8, 16, 1, 0, 0, 0, 0, 0, 0, 0, 0)
    call = L.dmxq_hadamard_qdq
    assert call(null, null, lib.BF16, lib.BF16, 0, 64, 64, 0, None, null, null, null) == lib.OK             # nothing to do
    assert call(null, null, lib.BF16, lib.BF16, 4, 64, 64, 0, None, null, null, null) == lib.ERR_BAD_ARG    # null pointers
    assert call(one, one, 7, lib.BF16, 4, 64, 64, 0, None, null, null, null) == lib.ERR_BAD_ARG             # dtype
    assert call(one, one, lib.BF16, lib.BF16, -1, 64, 64, 0, None, null, null, null) == lib.ERR_BAD_ARG     # negative size
    assert call(one, one, lib.BF16, lib.BF16, 4, 64, 64, 1, None, null, null, null) == lib.ERR_BAD_ARG      # inverse without a format
    assert call(one, one, lib.BF16, lib.BF16, 4, 64, 64, 1, fmt(4, *bfp[1:]), null, null, null) == lib.ERR_BAD_ARG   # kind
    assert call(one, one, lib.BF16, lib.F32, 4, 64, 64, 1, fmt(*bfp), null, null, null) == lib.ERR_BAD_ARG  # in place across widths
    assert call(one, one, lib.BF16, lib.BF16, 4, 64, 64, 1, fmt(lib.GPTQ_FIXED, 8, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0), null, null, null) \
        == lib.ERR_BAD_ARG                                                                                  # fixed point without a scale
    for size in (48, 4, 512, 0):
        assert call(one, one, lib.BF16, lib.BF16, 4, 1536, size, 0, None, null, null, null) == lib.ERR_UNSUPPORTED
    assert call(one, one, lib.BF16, lib.BF16, 4, 96, 64, 0, None, null, null, null) == lib.ERR_UNSUPPORTED  # L % size
    for bad in ((lib.GPTQ_BFP, 8, 128, 1), (lib.GPTQ_BFP, 8, 24, 1), (lib.GPTQ_BFP, 8, 1, 1), (lib.GPTQ_BFP, 23, 16, 1), (lib.GPTQ_BFP, 1, 16, 1)):
        assert call(one, one, lib.BF16, lib.BF16, 4, 64, 64, 1, fmt(*bad, 0, 0, 0, 0, 0, 0, 0, 0), null, null, null) == lib.ERR_UNSUPPORTED
    assert call(one, one, lib.BF16, lib.BF16, 4, 64, 64, 1, fmt(lib.GPTQ_MXFP, 0, 48, 0, 1, 2, 0, 0, 0, 0, 0, 0), null, null, null) == lib.ERR_UNSUPPORTED
    assert call(one, one, lib.BF16, lib.BF16, 4, 64, 64, 1, fmt(lib.GPTQ_MXFP, 0, 32, 0, 23, 8, 0, 0, 0, 0, 0, 0), null, null, null) == lib.ERR_UNSUPPORTED
    assert call(one, one, lib.BF16, lib.BF16, 4, 64, 64, 1, fmt(lib.GPTQ_FLOAT, 0, 0, 0, 23, 8, 127, 0, 0, 0, 0, 0), null, null, null) == lib.ERR_UNSUPPORTED
    # the range checks every user of dmxq_gptq_format shares, each reached through this entry point
    sc = one
    for bad in ((lib.GPTQ_FIXED, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0), (lib.GPTQ_FIXED, 25, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0),
                (lib.GPTQ_FLOAT, 0, 0, 0, 3, 0, 7, 0, 0, 0, 0, 0), (lib.GPTQ_FLOAT, 0, 0, 0, 3, 9, 7, 0, 0, 0, 0, 0),
                (lib.GPTQ_FLOAT, 0, 0, 0, -1, 4, 7, 0, 0, 0, 0, 0),
                (lib.GPTQ_MXFP, 0, 32, 0, 1, 0, 0, 0, 0, 0, 0, 0), (lib.GPTQ_MXFP, 0, 32, 0, 1, 9, 0, 0, 0, 0, 0, 0),
                (lib.GPTQ_MXFP, 0, 32, 0, -1, 2, 0, 0, 0, 0, 0, 0)):
        assert call(one, one, lib.BF16, lib.BF16, 4, 64, 64, 1, fmt(*bad), sc, sc, null) == lib.ERR_UNSUPPORTED, bad
    # a shared range check and a rule of this entry point broken at once: the format is judged before the pointers and before "nothing to do"
    assert call(null, null, lib.BF16, lib.BF16, 4, 64, 64, 1, fmt(lib.GPTQ_FLOAT, 0, 0, 0, 23, 8, 127, 0, 0, 0, 0, 0), null, null, null) == lib.ERR_UNSUPPORTED
    assert call(one, one, lib.BF16, lib.BF16, 4, 64, 64, 1, fmt(lib.GPTQ_FIXED, 25, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0), null, null, null) == lib.ERR_UNSUPPORTED
    assert call(null, null, lib.BF16, lib.BF16, 0, 64, 64, 1, fmt(lib.GPTQ_BFP, 23, 16, 1, 0, 0, 0, 0, 0, 0, 0, 0), null, null, null) == lib.ERR_UNSUPPORTED
    # ... but after the block size of the rotation and the format's kind
    assert call(one, one, lib.BF16, lib.BF16, 4, 1536, 48, 1, fmt(4, 23, 16, 1, 0, 0, 0, 0, 0, 0, 0, 0), null, null, null) == lib.ERR_BAD_ARG
    # the other users of dmxq_gptq_format answer kind 3 as they answer any unknown kind
    assert L.dmxq_cast_error(one, lib.BF16, 4, 64, ctypes.cast(ctypes.pointer(lib.GptqFormat(lib.GPTQ_MXFP, 0, 32, 0, 1, 2, 0, 0, 0, 0, 0, 0)),
                                                                ctypes.c_void_p), 1, null, null, 0, one, one, 1 << 20, null) == lib.ERR_BAD_ARG


def test_format_sweep_labels(dmx):
    from dmx_compressor_amd import benchmark as B
    fmts = ["BFP[8|8]{16}(SN)", dmx.Format.from_shorthand("MXFP4[E2M1]{32}"), ("XP[8,0](CSN)", 0.05, 0)]
    plain = ["BFP[8|8]{16}(SN)", "MXFP4[E2M1]{32}", "XP[8,0](CSN)"]
    assert B._sweep_labels(fmts, None) == ([None], plain)
    assert B._sweep_labels(fmts, 64) == ([64], [f"{l} @H64" for l in plain])
    entries, labels = B._sweep_labels(fmts, [None, 64, 128])
    assert entries == [None, 64, 128]
    assert labels == plain + [f"{l} @H64" for l in plain] + [f"{l} @H128" for l in plain]
    for bad in (48, [None, 4], []):
        with pytest.raises(ValueError):
            dmx.format_sweep(torch.zeros(4, 64), fmts, hadamard=bad)
