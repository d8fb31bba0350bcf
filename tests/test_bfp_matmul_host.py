"""ops.bfp_matmul without a GPU: the refusals of bfp_matmul_check, the Meta kernel's shape and dtype, and the two C-ABI symbols."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("fx,fw,xs,ws", [
    ("BFP[8|8]{64}(SN)", "BFP[8|8]{32}(SN)", (4, 128), (8, 128)),      # two block sizes
    ("BFP[12|8]{64}(SN)", None, (4, 128), (8, 128)),                    # codes wider than int8
    ("FP[1|5|10,15](FN)", None, (4, 128), (8, 128)),                    # not a BFP format
    ("BFP[8|8]{64}(SN)", "XP[8,0](CSN)", (4, 128), (8, 128)),
    ("BFP[8|8]{64}(SS)", None, (4, 128), (8, 128)),                     # stochastic rounding
    ("BFP[8|8]{64}(SN)", None, (4, 128), (8, 64)),                      # a wrong K
    ("BFP[8|8]{64}(SN)", None, (4, 128), (2, 8, 128)),                  # w is not [N, K]
])
def test_check_refuses_before_any_launch(dmx, fx, fw, xs, ws):
    with pytest.raises(dmx.DmxqError):
        dmx.ops.bfp_matmul_check(torch.zeros(xs), torch.zeros(ws), fx, fw)
    with pytest.raises(dmx.DmxqError):
        dmx.ops.bfp_matmul(torch.zeros(xs), torch.zeros(ws), fx, fw)


def test_check_accepts_objects_and_shorthands(dmx):
    fa, fw = dmx.ops.bfp_matmul_check(torch.zeros(2, 3, 128), torch.zeros(8, 128), "BFP[8|8]{64}(SN)", dmx.BlockFloatingPoint(4, 64, False))
    assert (fa.precision, fw.precision, fw.symmetric) == (8, 4, False) and dmx.ops.BFP_MATMUL_CHAIN_BY_DEFAULT == frozenset()
    with pytest.raises(TypeError):
        dmx.nn.ReLU().configure(dict(block_matmul=True))


@pytest.mark.parametrize("out_dtype", (torch.float32, torch.bfloat16, torch.float16))
def test_meta_kernel_shape_and_dtype(dmx, out_dtype):
    if dmx.ops.BINDING != "torch":
        pytest.skip("the ctypes binding has no Meta kernels")
    m = lambda *s, dt: torch.empty(s, dtype=dt, device="meta")
    y = torch.ops.dmxq.bfp_matmul(m(5, 192, dt=torch.int8), m(5, 3, dt=torch.uint8), m(7, 192, dt=torch.int8), m(7, 3, dt=torch.uint8), 8, 4, 64, out_dtype)
    assert y.shape == (5, 7) and y.dtype == out_dtype and y.device.type == "meta"
    with pytest.raises(RuntimeError):
        torch.ops.dmxq.bfp_matmul(m(5, 192, dt=torch.int8), m(5, 2, dt=torch.uint8), m(7, 192, dt=torch.int8), m(7, 3, dt=torch.uint8), 8, 4, 64, out_dtype)


def test_symbols_and_geometry_classes(dmx):
    lib, L = dmx._lib, dmx._lib.lib()
    header = open(os.path.join(ROOT, "include", "dmxq.h")).read()
    for name in ("dmxq_bfp_matmul", "dmxq_bfp_matmul_class"):
        assert re.search(rf"\bint {name}\(", header) and name in lib.SIGNATURES and hasattr(L, name)
    assert L.dmxq_abi_version() == 4
    assert [L.dmxq_bfp_matmul_class(130, 257, 5 * B, B) for B in (32, 64, 128)] == [1, 2, 3]
    assert [L.dmxq_bfp_matmul_class(4, 4, K, B) for K, B in ((64, 16), (96, 64), (0, 64), (256, 256))] == [0, 0, 0, 0]
    import ctypes
    null, one = ctypes.c_void_p(None), ctypes.c_void_p(16)
    assert L.dmxq_bfp_matmul(null, null, null, null, null, lib.F32, 0, 8, 64, 64, 8, 8, null) == lib.OK            # M == 0
    assert L.dmxq_bfp_matmul(null, one, one, one, one, lib.F32, 4, 8, 64, 64, 8, 8, null) == lib.ERR_BAD_ARG
    assert L.dmxq_bfp_matmul(one, one, one, one, one, lib.F32, 4, 8, 64, 64, 9, 8, null) == lib.ERR_UNSUPPORTED   # p > 8
    assert L.dmxq_bfp_matmul(one, one, one, one, one, lib.F32, 4, 8, 96, 64, 8, 8, null) == lib.ERR_UNSUPPORTED   # K % B
    assert L.dmxq_bfp_matmul(ctypes.c_void_p(8), one, one, one, one, lib.F32, 4, 8, 64, 64, 8, 8, null) == lib.ERR_UNSUPPORTED   # alignment
