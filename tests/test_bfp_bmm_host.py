"""ops.bfp_bmm / ops.bfp_pack(block_dim=-2) without a GPU: the refusals before any launch, the Meta kernels' shapes and dtypes, the
three C-ABI symbols, the geometry classes and the entry's argument validation."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = "BFP[8|8]{64}(SN)"


@pytest.mark.parametrize("fx,fw,xs,ws,layout", [
    (F, "BFP[8|8]{32}(SN)", (2, 4, 128), (2, 8, 128), "nk"),        # two block sizes
    ("BFP[12|8]{64}(SN)", None, (2, 4, 128), (2, 8, 128), "nk"),    # codes wider than int8
    ("FP[1|5|10,15](FN)", None, (2, 4, 128), (2, 8, 128), "nk"),    # not a BFP format
    ("BFP[8|8]{64}(SS)", None, (2, 4, 128), (2, 8, 128), "nk"),     # stochastic rounding
    (F, None, (2, 4, 128), (3, 8, 128), "nk"),                      # unequal leading dimensions
    (F, None, (2, 4, 128), (8, 128), "nk"),                         # ranks differ
    (F, None, (2, 4, 128), (2, 8, 128), "kn"),                      # a wrong K for the layout
    (F, None, (2, 4, 128), (2, 8, 128), "nn"),                      # a wrong w_layout
])
def test_bmm_refuses_before_any_launch(dmx, fx, fw, xs, ws, layout):
    with pytest.raises(dmx.DmxqError):
        dmx.ops.bfp_bmm(torch.zeros(xs), torch.zeros(ws), fx, fw, w_layout=layout)


def test_defaults_and_other_modules(dmx):
    assert dmx.ops.BFP_BMM_CHAIN_BY_DEFAULT == frozenset() and dmx.nn.ActActMatMul().block_matmul is False
    with pytest.raises(TypeError):
        dmx.nn.ReLU().configure(dict(block_matmul=True))
    with pytest.raises(dmx.DmxqError):
        dmx.ops.bfp_pack(torch.zeros(4, 64), 8, 32, block_dim=0)


@pytest.mark.parametrize("out_dtype", (torch.float32, torch.bfloat16))
def test_meta_kernels_shape_and_dtype(dmx, out_dtype):
    if dmx.ops.BINDING != "torch":
        pytest.skip("the ctypes binding has no Meta kernels")
    m = lambda *s, dt: torch.empty(s, dtype=dt, device="meta")
    i8, u8 = torch.int8, torch.uint8
    y = torch.ops.dmxq.bfp_bmm(m(3, 5, 192, dt=i8), m(3, 5, 3, dt=u8), m(3, 7, 192, dt=i8), m(3, 7, 3, dt=u8), 8, 4, 64, 0, out_dtype)
    assert y.shape == (3, 5, 7) and y.dtype == out_dtype and y.device.type == "meta"
    y = torch.ops.dmxq.bfp_bmm(m(3, 5, 192, dt=i8), m(3, 5, 3, dt=u8), m(3, 192, 8, dt=i8), m(3, 3, 8, dt=u8), 8, 4, 64, 1, out_dtype)
    assert y.shape == (3, 5, 8) and y.dtype == out_dtype
    with pytest.raises(RuntimeError):   # "kn" exponents in the "nk" shape
        torch.ops.dmxq.bfp_bmm(m(3, 5, 192, dt=i8), m(3, 5, 3, dt=u8), m(3, 192, 8, dt=i8), m(3, 8, 3, dt=u8), 8, 4, 64, 1, out_dtype)
    c, e = torch.ops.dmxq.bfp_pack_cols(m(2, 3, 128, 40, dt=out_dtype), 8, 64, True)
    assert c.shape == (2, 3, 128, 40) and c.dtype == i8 and e.shape == (2, 3, 2, 40) and e.dtype == u8 and e.device.type == "meta"


def test_symbols_classes_and_argument_validation(dmx):
    lib, L = dmx._lib, dmx._lib.lib()
    header = open(os.path.join(ROOT, "include", "dmxq.h")).read()
    for name in ("dmxq_bfp_bmm", "dmxq_bfp_bmm_class", "dmxq_bfp_pack_cols"):
        assert re.search(rf"\bint {name}\(", header) and name in lib.SIGNATURES and hasattr(L, name)
    assert L.dmxq_abi_version() == 4
    cls = lambda *a: L.dmxq_bfp_bmm_class(*a)   # (batch, M, N, K, B, layout) -> 1 + 2 (3 layout + block index) + (N <= 64)
    assert [cls(3, 130, 260, 5 * B, B, 0) for B in (32, 64, 128)] == [1, 3, 5]
    assert [cls(3, 130, 64, 5 * B, B, 0) for B in (32, 64, 128)] == [2, 4, 6]
    assert [cls(3, 130, 260, 5 * B, B, 1) for B in (32, 64, 128)] == [7, 9, 11]
    assert [cls(3, 130, 64, 5 * B, B, 1) for B in (32, 64, 128)] == [8, 10, 12]
    assert [cls(3, 4, 8, 96, 64, 0), cls(3, 4, 38, 128, 64, 1), cls(3, 4, 38, 128, 64, 0), cls(3, 4, 8, 64, 16, 0), cls(65536, 4, 8, 64, 64, 0),
            cls(3, 4, 8, 64, 64, 2)] == [0, 0, 4, 0, 0, 0]   # (N = 38: refused in "kn" only; "nk" takes it on the 64-wide tile)
    mant = torch.empty(2, 128, 72, dtype=torch.int8)
    assert dmx.ops.bfp_bmm_class(mant, torch.empty(2, 64, 72, dtype=torch.int8), 32, "kn") is None   # K mismatch is the caller's; 72 % 32
    assert dmx.ops.bfp_bmm_class(torch.empty(2, 9, 128, dtype=torch.int8), mant, 64, "kn") == "kn_b64_n128"
    assert dmx.ops.bfp_bmm_class(torch.empty(2, 9, 128, dtype=torch.int8), torch.empty(2, 128, 64, dtype=torch.int8), 64, "kn") == "kn_b64_n64"
    null, one, four = ctypes.c_void_p(None), ctypes.c_void_p(16), ctypes.c_void_p(20)
    bmm = L.dmxq_bfp_bmm
    assert bmm(null, null, null, null, null, lib.F32, 0, 4, 8, 64, 64, 8, 8, 0, null) == lib.OK              # batch == 0
    assert bmm(null, one, one, one, one, lib.F32, 2, 4, 8, 64, 64, 8, 8, 0, null) == lib.ERR_BAD_ARG
    assert bmm(one, one, one, one, one, lib.F32, 2, 4, 8, 64, 64, 8, 8, 2, null) == lib.ERR_BAD_ARG           # layout
    assert bmm(one, one, one, one, one, lib.F32, 2, 4, 8, 64, 64, 9, 8, 0, null) == lib.ERR_UNSUPPORTED       # p > 8
    assert bmm(one, one, one, one, one, lib.F32, 2, 4, 8, 96, 64, 8, 8, 0, null) == lib.ERR_UNSUPPORTED       # K % B
    assert bmm(one, one, one, one, one, lib.F32, 2, 4, 6, 64, 64, 8, 8, 1, null) == lib.ERR_UNSUPPORTED       # "kn": N % 4
    assert bmm(one, one, four, one, one, lib.F32, 2, 4, 8, 64, 64, 8, 8, 0, null) == lib.ERR_UNSUPPORTED      # "nk": 16-byte codes
    assert bmm(one, one, ctypes.c_void_p(18), one, one, lib.F32, 2, 4, 8, 64, 64, 8, 8, 1, null) == lib.ERR_UNSUPPORTED   # "kn": 4-byte codes
    assert bmm(ctypes.c_void_p(8), one, one, one, one, lib.F32, 2, 4, 8, 64, 64, 8, 8, 1, null) == lib.ERR_UNSUPPORTED
    pack = L.dmxq_bfp_pack_cols
    assert pack(null, lib.BF16, null, null, 0, 64, 8, 64, 8, 1, null) == lib.OK
    assert pack(null, lib.BF16, one, one, 1, 64, 8, 64, 8, 1, null) == lib.ERR_BAD_ARG
    assert [pack(one, lib.BF16, one, one, 1, K, N, B, 8, 1, null) for K, N, B in ((96, 8, 64), (64, 12, 64), (64, 8, 16))] == [lib.ERR_UNSUPPORTED] * 3
    assert pack(one, lib.BF16, four, one, 1, 64, 8, 64, 8, 1, null) == lib.ERR_UNSUPPORTED                    # codes not 8-byte aligned
