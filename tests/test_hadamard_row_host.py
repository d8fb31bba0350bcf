"""CPU-side tests (-m "not gpu") of the full-row Hadamard rotation: the tables H_m, tests/_hadamard_row_ref.py against scalar
loops and the dense float64 matrix, the front end's validation, the C ABI's status codes and CastTo's "hadamard_row" pre_transform."""
import copy
import ctypes
import pickle

import numpy as np
import pytest
import torch

import _hadamard_ref as B
import _hadamard_row_ref as R
from _data import bits_equal, make


@pytest.mark.parametrize("m", [12, 20, 28])
def test_tables_are_hadamard(dmx, m):
    """H_m H_m^T = m I in integers, entries +-1: the library's table and the checker's own construction, which agree"""
    H = dmx.ops.hadamard_matrix(m)
    Hl = H.to(torch.int64)
    assert H.dtype == torch.int8 and bool((H.abs() == 1).all()) and torch.equal(Hl @ Hl.T, m * torch.eye(m, dtype=torch.int64))
    assert np.array_equal(H.numpy().astype(np.int64), R.matrix(m))
    assert (m in (12, 20)) == (not torch.equal(H, H.T))   # Paley I is not symmetric: R^T is a map of its own


@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("n", [768, 512])
def test_restatement_is_the_stated_loops(n, transpose):
    x = make("heavy", (2, n), seed=n, block=64)
    want = np.stack([R.rotate_loops(row, transpose) for row in x.numpy()])
    assert np.array_equal(R.rotate_ref(x, transpose).numpy().view(np.int32), want.view(np.int32))
    x = make("heavy", (5, 256), seed=9, block=64)   # n = 256 is the block rotation
    assert bits_equal(R.rotate_ref(x, transpose), B.rotate_ref(x, 256)) == 0


@pytest.mark.parametrize("kind", ["normal", "outlier"])
@pytest.mark.parametrize("n", [512, 768, 1280, 1792, 4096, 14336])
def test_restatement_against_the_dense_matrix(n, kind):
    """every element within (k + m + 2) 2^-24 1.01 sum|x| / sqrt(n) of the float64 product (_hadamard_row_ref.rotation_bound), for R and
    for R^T; R^T(R(x)) within twice that bound of x"""
    x = make(kind, (3, n), seed=n, block=64)
    M, bound = R.dense(n), R.rotation_bound(x)
    for transpose in (False, True):
        exact = x.double() @ (M if transpose else M.T)
        err = (R.rotate_ref(x, transpose).double() - exact).abs()
        assert bool((err <= bound).all())
    back = R.rotate_ref(R.rotate_ref(x), True)
    assert bool(((back.double() - x.double()).abs() <= 2 * bound).all())


def test_front_end_validation_without_gpu(dmx):
    ops = dmx.ops
    assert [ops.hadamard_row_check(n) for n in (512, 768, 5120, 14336, 16384, 24576)] == [(1, 9), (12, 6), (20, 8), (28, 9), (1, 14), (12, 11)]
    for bad in (0, 7, 36, 1536 * 3, 11 * 512, 9 * 1024, 512.0, True):
        with pytest.raises(ValueError):
            ops.hadamard_row_check(bad)
    with pytest.raises(ValueError):
        ops.hadamard_matrix(16)
    assert ops.hadamard_row_class(4096, torch.bfloat16) == "block" and ops.hadamard_row_class(2048, torch.bfloat16, 128) == "wave"
    assert ops.hadamard_row_class(2048, torch.float32) == "block" and ops.hadamard_row_class(14336, torch.float16, 14336) == "block"
    for n, seg in ((256, None), (24576, None), (4608, None), (768, 128), (4096, 8), (4096, 512), (4096, 48)):
        assert ops.hadamard_row_class(n, torch.bfloat16, seg) is None, (n, seg)
    x = torch.zeros(4, 768)
    for fmt, g, gs in (("BFP[8|8]{16}(SN)", "per_token", None), ("XP[8,2](CSN)", "per_token", None), ("XP[4,0](CSN)", "per_tensor", None),
                       ("XP[4,0](CSN)", "per_group", 128), ("XP[4,0](CSN)", "per_group", 8), ("XP[4,0](CSN)", "per_group", 48),
                       ("XP[4,0](CSN)", "per_group", None)):
        with pytest.raises(ValueError):
            ops.hadamard_row_dynamic_qdq(x, fmt, g, gs)
    for call in (lambda: ops.hadamard_row(torch.zeros(4, 100)), lambda: ops.hadamard_row(x, dim=2),
                 lambda: ops.hadamard_row_dynamic_qdq(torch.zeros(4, 100), "XP[4,0](CSN)")):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: ops.hadamard_row(x), lambda: ops.hadamard_row_dynamic_qdq(x, "XP[4,0](CSN)")):
        with pytest.raises(dmx.DmxqError):      # a CPU tensor, as everywhere else
            call()


def test_c_abi_argument_validation(dmx):
    """dmxq_hadamard_row_qdq's status codes, before anything is launched (no GPU needed)"""
    lib = dmx._lib
    null, one, odd, two = ctypes.c_void_p(None), ctypes.c_void_p(4096), ctypes.c_void_p(4104), ctypes.c_void_p(8192)
    call = lib.lib().dmxq_hadamard_row_qdq
    bf, f32 = lib.BF16, lib.F32
    assert call(null, null, bf, bf, 0, 4096, 0, 0, 0, 0, 0, null, null, null) == lib.OK                   # nothing to do
    assert call(null, null, bf, bf, 4, 4096, 0, 0, 0, 0, 0, null, null, null) == lib.ERR_BAD_ARG          # null pointers
    assert call(one, one, 7, bf, 4, 4096, 0, 0, 0, 0, 0, null, null, null) == lib.ERR_BAD_ARG             # dtype
    assert call(one, one, bf, bf, -1, 4096, 0, 0, 0, 0, 0, null, null, null) == lib.ERR_BAD_ARG           # negative size
    assert call(one, one, bf, bf, 4, 4096, 0, 1, 0, 0, 0, null, null, null) == lib.ERR_BAD_ARG            # inverse without a format
    assert call(one, one, bf, f32, 4, 4096, 0, 0, 0, 0, 0, null, null, null) == lib.ERR_BAD_ARG           # in place across widths
    for n in (256, 24576, 4608, 4100):                                                                    # rows the kernel refuses
        assert call(one, odd, bf, bf, 4, n, 0, 0, 0, 0, 0, null, null, null) == lib.ERR_UNSUPPORTED, n
    assert call(odd, one, bf, bf, 4, 4096, 0, 0, 0, 0, 0, null, null, null) == lib.ERR_UNSUPPORTED        # unaligned
    assert call(one, odd, f32, bf, 4, 4096, 0, 0, 0, 0, 0, null, null, null) == lib.ERR_UNSUPPORTED       # narrowing rotation
    assert call(one, two, bf, f32, 4, 4096, 0, 0, 4, 1, 4096, null, null, null) == lib.ERR_UNSUPPORTED    # a cast across dtypes
    for seg in (8, 48, 512, 0):                                                                           # groups
        assert call(one, two, bf, bf, 4, 4096, 0, 0, 4, 1, seg, null, null, null) == lib.ERR_UNSUPPORTED, seg
    assert call(one, two, bf, bf, 4, 768, 0, 0, 4, 1, 128, null, null, null) == lib.ERR_UNSUPPORTED       # 128 does not divide 2^6
    assert call(one, two, bf, bf, 4, 4096, 0, 0, 23, 1, 4096, null, null, null) == lib.ERR_UNSUPPORTED    # precision


def test_set_pre_transform_hadamard_row(dmx):
    c = dmx.CastTo(format="XP[4,0](CSN)")
    for bad in (False, 64, "yes", {"size": 64}, {"inverse": 1}):
        with pytest.raises(ValueError):
            c.set_pre_transform({"hadamard_row": bad})
    with pytest.raises(ValueError):
        c.set_pre_transform({"hadamard_row": True, "hadamard": 64})
    c.set_pre_transform({"hadamard_row": {"inverse": False}})
    assert c.pre_transform == {"hadamard_row": {"inverse": False}}
    c.set_pre_transform({"hadamard_row": True})
    for setter in (lambda: c.set_learnable("per_tensor"), lambda: c.set_codebook(dmx.ops.NF4),
                   lambda: c.set_vq({"codebook": torch.zeros(16, 2)})):
        with pytest.raises(ValueError, match="hadamard"):     # exclusive in this order ...
            setter()
    c.set_dynamic("per_token")
    for clone in (copy.deepcopy(c), pickle.loads(pickle.dumps(c))):
        assert clone.pre_transform == {"hadamard_row": {"inverse": True}} and clone.pre_transform is not c.pre_transform and clone.dynamic == "per_token"
    assert not any("hadamard" in k for k in c.state_dict())
    learn = dmx.CastTo(format="XP[4,0](CSN)")
    learn.set_learnable("per_tensor")
    with pytest.raises(ValueError):         # ... and in the other
        learn.set_pre_transform({"hadamard_row": True})
    m = dmx.nn.Linear(768, 8)               # the seam DmxModule.configure uses
    m.configure({"input_format": "XP[4,0](CSN)", "pre_input_transform": [{"hadamard_row": True}]})
    assert m.input_casts.input_cast.pre_transform == {"hadamard_row": {"inverse": True}}
