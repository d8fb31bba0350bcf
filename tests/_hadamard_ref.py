"""The block-Hadamard rotation of include/dmxq.h (dmxq_hadamard_qdq) restated in torch float32 on the CPU, and its
composition with a cast.  Imports neither the library nor the reference: the casts come in as callables (the oracle's, in the tests).

R_H on a block of H = 2^k consecutive elements of the last dimension, widened to float32:
    for s = 1, 2, 4, .., H/2 in that order: every pair (i, i + s) with bit s of i clear becomes (v[i] + v[i+s], v[i] - v[i+s]),
    each ONE float32 operation on the old values; then ONE float32 multiply by c = float32(1 / sqrt(H)) (computed in double).
R_H is symmetric and orthonormal: its own inverse."""
import math

import numpy as np
import torch

SIZES = (8, 16, 32, 64, 128, 256)


def scale_of(H: int) -> np.float32:
    return np.float32(1.0 / math.sqrt(H))


def rotate_ref(x: torch.Tensor, H: int) -> torch.Tensor:
    """R_H of every block of H consecutive elements along the last dimension; float32 result of x's shape"""
    assert H in SIZES and x.shape[-1] % H == 0, (H, tuple(x.shape))
    v = x.detach().cpu().to(torch.float32).contiguous()
    shape = v.shape
    s = 1
    while s < H:
        t = v.reshape(-1, H // (2 * s), 2, s)
        a, b = t[:, :, 0, :], t[:, :, 1, :]
        v = torch.stack((a + b, a - b), dim=2)
        s *= 2
    c = torch.tensor(scale_of(H), dtype=torch.float32)
    return (v.reshape(-1) * c).reshape(shape)


def rotated_cast_ref(x: torch.Tensor, H: int, cast, inverse: bool, dtype: torch.dtype) -> torch.Tensor:
    """round_to(dtype, R(Q(R(x)))) with `inverse`, round_to(dtype, Q(R(x))) without; cast: float32 tensor -> float32 tensor (the
    oracle's bfp_cast / mxfp_cast / floating_point_cast / fixed_point_affine_cast along the last dimension), or None for Q = identity"""
    r = rotate_ref(x, H)
    q = r if cast is None else cast(r).to(torch.float32)
    if inverse:
        q = rotate_ref(q, H)
    return q.to(dtype)


def sylvester(H: int) -> torch.Tensor:
    """the dense orthonormal Sylvester-Hadamard matrix in float64"""
    m = torch.ones(1, 1, dtype=torch.float64)
    while m.shape[0] < H:
        m = torch.cat((torch.cat((m, m), 1), torch.cat((m, -m), 1)), 0)
    return m / math.sqrt(H)


def rotation_bound(x: torch.Tensor, H: int) -> torch.Tensor:
    """per block of H: (k + 2) 2^-24 sqrt(H) max|x| -- one rounding per stage (relative 2^-24 of a value of at most 2^stage max|x|),
    amplified by the later stages to at most sqrt(H) max|x| 2^-24 each after the scale, plus the scale's own two roundings (the
    constant and the product); float64 [..., L / H, 1]"""
    k = H.bit_length() - 1
    blocks = x.detach().cpu().double().reshape(*x.shape[:-1], x.shape[-1] // H, H)
    return (k + 2) * 2.0 ** -24 * math.sqrt(H) * blocks.abs().amax(dim=-1, keepdim=True)
