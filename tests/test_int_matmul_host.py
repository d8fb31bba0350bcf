"""ops.int_matmul / ops.dynamic_int_pack without a GPU: the C-ABI symbols, the class table, argument errors before any launch, the
refusals of int_matmul_check and the Meta kernels' shapes and dtypes."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_classes_and_argument_errors(dmx):
    lib, L = dmx._lib, dmx._lib.lib()
    header = open(os.path.join(ROOT, "include", "dmxq.h")).read()
    for name in ("dmxq_dynamic_fixed_pack", "dmxq_dynamic_pack_class", "dmxq_int_matmul", "dmxq_int_matmul_class"):
        assert re.search(rf"\bint {name}\(", header) and name in lib.SIGNATURES and hasattr(L, name)
    assert L.dmxq_abi_version() == 4
    cls = L.dmxq_int_matmul_class
    assert [cls(130, 257, 96, 0, 0), cls(16, 16, 131072, 0, 0), cls(16, 16, 131088, 0, 0), cls(4, 4, 24, 0, 0), cls(4, 4, 8, 0, 0)] == [1, 1, 0, 0, 0]
    assert [cls(130, 257, 5 * G, ga, G) for G in (32, 64, 128) for ga in (0, G)] == [2] * 6
    assert [cls(4, 4, 512, 0, 16), cls(4, 4, 512, 0, 256), cls(4, 4, 96, 0, 64), cls(4, 4, 128, 32, 64), cls(4, 4, 128, 64, 0)] == [0] * 5
    assert [L.dmxq_dynamic_pack_class(lib.BF16, S, r) for S, r in ((16, 0), (256, 0), (48, 1), (4096, 1), (16384, 1), (48, 0), (24, 1), (16400, 1))] \
        == [1, 1, 2, 3, 4, 0, 0, 0]
    null, one = ctypes.c_void_p(None), ctypes.c_void_p(16)
    mm, pack = L.dmxq_int_matmul, L.dmxq_dynamic_fixed_pack
    assert mm(null, null, null, null, null, lib.F32, 0, 8, 64, 0, 0, null) == lib.OK                      # M == 0
    assert mm(null, one, one, one, one, lib.F32, 4, 8, 64, 0, 0, null) == lib.ERR_BAD_ARG
    assert mm(one, one, one, one, one, 77, 4, 8, 64, 0, 0, null) == lib.ERR_BAD_ARG                        # dtype
    assert mm(one, one, one, one, one, lib.F32, 4, 8, 72, 0, 0, null) == lib.ERR_UNSUPPORTED               # K % 16
    assert mm(ctypes.c_void_p(8), one, one, one, one, lib.F32, 4, 8, 64, 0, 0, null) == lib.ERR_UNSUPPORTED   # alignment
    assert pack(null, lib.F32, one, one, 4, 64, 1, 8, 1, -127, 127, null) == lib.ERR_BAD_ARG
    assert pack(one, 77, one, one, 4, 64, 1, 8, 1, -127, 127, null) == lib.ERR_BAD_ARG
    assert pack(one, lib.F32, one, one, 4, 64, 1, 0, 1, -127, 127, null) == lib.ERR_BAD_ARG                # precision < 1
    assert pack(one, lib.F32, one, one, 4, 64, 1, 9, 1, -255, 255, null) == lib.ERR_UNSUPPORTED            # codes wider than int8
    assert pack(one, lib.F32, one, one, 0, 64, 1, 8, 1, -127, 127, null) == lib.OK


@pytest.mark.parametrize("fx,fw,xs,ws", [
    ("BFP[8|8]{64}(SN)", None, (4, 128), (8, 128)),                     # a BFP format
    ("XP[8,0](CSN)", "BFP[8|8]{64}(SN)", (4, 128), (8, 128)),
    ("XP[12,0](CSN)", None, (4, 128), (8, 128)),                        # codes wider than int8
    ("XP[8,0](CSS)", None, (4, 128), (8, 128)),                         # stochastic rounding
    ("XP[8,0](CSN)", None, (4, 128), (8, 64)),                          # a wrong K
])
def test_check_refuses_before_any_launch(dmx, fx, fw, xs, ws):
    ops = dmx.ops
    with pytest.raises(dmx.DmxqError):
        ops.int_matmul_check(torch.zeros(xs), torch.zeros(ws), fx, fw)
    with pytest.raises(dmx.DmxqError):
        ops.int_matmul(torch.zeros(xs), torch.zeros(ws), fx, fw)
    fa, fb = ops.int_matmul_check(torch.zeros(2, 3, 128), torch.zeros(8, 128), "XP[8,0](CSN)", "XP[4,0](CSN)")
    assert (fa.precision, fb.precision) == (8, 4) and ops.INT_MATMUL_CHAIN_BY_DEFAULT == frozenset() and ops.INT_MATMUL_GROUP_SIZES == (32, 64, 128)
    with pytest.raises(dmx.DmxqError):   # bfp_matmul keeps refusing integer formats
        ops.bfp_matmul_check(torch.zeros(xs), torch.zeros(8, xs[1]), "XP[8,0](CSN)")


@pytest.mark.parametrize("out_dtype", (torch.float32, torch.bfloat16, torch.float16))
def test_meta_kernels_shape_and_dtype(dmx, out_dtype):
    if dmx.ops.BINDING != "torch":
        pytest.skip("the ctypes binding has no Meta kernels")
    m = lambda *s, dt: torch.empty(s, dtype=dt, device="meta")
    for sa, sw, G in (((5,), (7,), 0), ((5,), (7, 3), 64), ((5, 3), (7, 3), 64)):
        y = torch.ops.dmxq.int_matmul(m(5, 192, dt=torch.int8), m(*sa, dt=torch.float32), m(7, 192, dt=torch.int8), m(*sw, dt=torch.float32), G, out_dtype)
        assert y.shape == (5, 7) and y.dtype == out_dtype and y.device.type == "meta"
    with pytest.raises(RuntimeError):
        torch.ops.dmxq.int_matmul(m(5, 192, dt=torch.int8), m(5, dt=torch.float32), m(7, 192, dt=torch.int8), m(7, 2, dt=torch.float32), 64, out_dtype)
    c, s = torch.ops.dmxq.dynamic_fixed_pack(m(3, 5, 128, dt=out_dtype), 64, False, 8, True, -127, 127)
    assert (c.shape, c.dtype, s.shape, s.dtype) == ((3, 5, 128), torch.int8, (30,), torch.float32)
