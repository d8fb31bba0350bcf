#!/usr/bin/env python3
"""oracle/gen_golden_seams.py — needs the reference's sources (through oracle/_ref).  Makes every call tests/test_gpu_seams.py compares the S1 seam with, on the
same inputs, through the REFERENCE's own compiled CPU extension (oracle/_ref/quant_cpu.so, built from its sources by
`make -C oracle ref`), and stores the results in

  tests/golden/seams.npz   keys: one seam_key(function, input, arguments) per call (tests/test_gpu_seams.py); y<i>: the result's
                           float32 bit patterns; m<i>: the uint8 mask of the *_mask functions.

so that the GPU test needs neither the reference nor anything compiled from it.  The stochastic calls are recorded once (the
reference's RNG is an unseeded global mt19937): the test only uses their statistics.

    PYTHONDONTWRITEBYTECODE=1 python oracle/gen_golden_seams.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "_ref"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import quant_cpu  # noqa: E402  (the reference's C++ extension)
from _data import make  # noqa: E402
from test_gpu_seams import GOLD, seam_key  # noqa: E402

keys, store = [], {}


def rec(name, x, *args):
    k = seam_key(name, x, args)
    if k in keys:
        return
    out = getattr(quant_cpu, name)(x, *args)
    y, m = out if isinstance(out, tuple) else (out, None)
    assert y.dtype == torch.float32 and y.shape == x.shape, (name, y.dtype, y.shape)
    i = len(keys)
    keys.append(k)
    store[f"y{i}"] = y.contiguous().view(torch.int32).numpy().view(np.uint32).reshape(-1).copy()
    if m is not None:
        assert m.dtype == torch.uint8 and m.shape == x.shape
        store[f"m{i}"] = m.contiguous().numpy().reshape(-1).copy()


# test_block_quantize_seam
for mode in ("nearest", "down", "up"):
    for shape, wl in (((4096, 16), 8), ((512, 64), 4), ((33, 40), 6), ((7, 3, 5), 16)):
        rec(f"block_quantize_{mode}", make("mixed", shape, seed=wl, block=shape[-1]), wl, 0, True)
x = make("heavy", (6, 10, 4), seed=3)
for dim in (-1, 1, 2):
    rec("block_quantize_nearest", x, 8, dim, True)

# test_float_and_fixed_seams
x = torch.cat([make("heavy", (20000,), seed=1), torch.tensor([0.0, -0.0, 65520.0, 3e38, 1e-40, float("inf"), float("nan")])])
for man, exp, bias, flush in ((10, 5, 15, True), (3, 4, 7, False), (2, 5, 15, False), (22, 8, 127, False)):
    rec("float_quantize_nearest", x, man, exp, bias, flush)
for mode in ("nearest", "up", "down"):
    for wl, fl, clamp, sym in ((8, 0, True, True), (8, 3, True, False), (12, -2, False, True)):
        rec(f"fixed_point_quantize_{mode}", x[:-2], wl, fl, clamp, sym)

# test_fixed_point_mask_seams
x = torch.cat([make("heavy", (20000,), seed=4), torch.tensor([0.0, -0.0, 127.0, 127.5, 128.0, -127.5, -128.0, -128.5, 1e30, -1e30,
                                                            float("inf"), float("-inf")])])
for wl, fl, sym in ((8, 0, True), (8, 0, False), (8, 3, False), (4, 0, True), (12, -2, True)):
    rec("fixed_point_quantize_nearest_mask", x, wl, fl, sym)

# test_python_wrappers_keep_the_reference_contract
x = make("normal", (64, 32), seed=2)
rec("block_quantize_nearest", x, 8, 0, True)
rec("float_quantize_nearest", x, 10, 5, 15, True)
rec("fixed_point_quantize_nearest", x, 8, 4, True, False)

# test_stochastic_rounding_is_unbiased_like_the_reference
rec("fixed_point_quantize_stochastic", torch.full((200000,), 0.3), 8, 0, True, True)
rec("block_quantize_stochastic", torch.rand(4096, 16, generator=torch.Generator().manual_seed(6)) * 2 - 1, 6, 0, True)

np.savez_compressed(GOLD, keys=np.array(keys), **store)
print(f"{GOLD}: {len(keys)} calls, {os.path.getsize(GOLD)} bytes")
