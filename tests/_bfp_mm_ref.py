"""References of the BFP matmul (DESIGN.md §8 "BFP matmul" / "Batched BFP matmul") that depend on neither route of the library.

  exact_terms        the block terms t_j as exact rationals, from hand-built codes and exponent bytes
  round_f32          nearest-even rounding of a rational to fp32 (denormals kept, overflow to Inf), on integers
  kernel_semantics   §8's kernel form: x = round(P sa), acc = round(x sw + acc) -- ONE rounding per block
  chain_semantics    the chain's form: round(round(x sw) + acc) -- two roundings
  ref_and_bound_mm / ref_and_bound_bmm   the float64 product of the unpacked operands and the bound of nb - 1 ordered fp32 adds of
                     exact terms (the check of tests/test_gpu_bfp_matmul.py and tests/test_gpu_bfp_bmm.py, for anything larger)

The two *_semantics functions are for tiny operands (about 16 x 8 outputs, 4 blocks): they run Python rationals per element.  An fp32
value is carried as a Python float (every fp32 is a double), so signed zeros, infinities and NaN are the IEEE ones.  Operands are
[M, K] / [M, nb] and [N, K] / [N, nb] ("nk"); a "kn" operand is transposed by the caller."""
import math
from fractions import Fraction

import torch

from _data import ulp_of

NAN, INF = float("nan"), float("inf")


def code_range(p):
    """the int8 codes of precision p: [-2^(p-1), 2^(p-1) - 1] (the lower end is the asymmetric format's)"""
    return -(1 << (p - 1)), (1 << (p - 1)) - 1


def block_sums(ca, cw, B):
    """P[m, n, j] = sum over block j of ca[m, k] cw[n, k], int64 on the CPU"""
    a, w = ca.cpu().to(torch.int64), cw.cpu().to(torch.int64)
    nb = a.shape[1] // B
    assert a.shape[1] == nb * B == w.shape[1]
    return torch.stack([a[:, j * B:(j + 1) * B] @ w[:, j * B:(j + 1) * B].T for j in range(nb)], -1)


def scale_of(byte, p):
    """the fp32 block scale 2^(e - 127 - (p - 2)) as a Python float: byte 0 -> +0, 255 -> NaN; >= 2^-132, exact in fp32 (a denormal
    below 2^-126)"""
    byte = int(byte)
    if byte == 0:
        return 0.0
    if byte == 255:
        return NAN
    return math.ldexp(1.0, byte - 127 - (p - 2))


def exact_terms(ca, ea, cw, ew, pa, pw, B):
    """[M][N][nb] of fractions.Fraction: t_j = P_j 2^(ea - 127 - (pa - 2)) 2^(ew - 127 - (pw - 2)), nothing rounded.  A byte 0 on either
    side makes the term 0 (its scale is 0), a byte 255 makes it None (NaN)."""
    P = block_sums(ca, cw, B).tolist()
    ea, ew = ea.cpu().tolist(), ew.cpu().tolist()
    out = []
    for m, row in enumerate(P):
        out.append([])
        for n, blocks in enumerate(row):
            ts = []
            for j, p in enumerate(blocks):
                a, w = ea[m][j], ew[n][j]
                if a == 255 or w == 255:
                    ts.append(None)
                elif a == 0 or w == 0:
                    ts.append(Fraction(0))
                else:
                    ts.append(Fraction(p) * Fraction(2) ** (a - 127 - (pa - 2)) * Fraction(2) ** (w - 127 - (pw - 2)))
            out[-1].append(ts)
    return out


def round_f32(x):
    """a rational (Fraction or int) -> the nearest fp32, ties to even, as a Python float: multiples of 2^-149 below 2^-126, +-Inf from
    2^128 (1 - 2^-25) on, a zero result signed like x.  Integer arithmetic only."""
    x = Fraction(x)
    if x == 0:
        return 0.0
    sign = -1.0 if x < 0 else 1.0
    n, d = abs(x).numerator, abs(x).denominator
    e = n.bit_length() - d.bit_length()                  # floor(log2 |x|) is e or e - 1
    if (n << max(-e, 0)) < (d << max(e, 0)):
        e -= 1
    q = max(e, -126) - 23                                # the exponent of the last place
    m, r = divmod(n << max(-q, 0), d << max(q, 0))
    if 2 * r > (d << max(q, 0)) or (2 * r == (d << max(q, 0)) and m & 1):
        m += 1
    if m.bit_length() + q > 128:
        return sign * INF
    return sign * math.ldexp(float(m), q)                # m < 2^25: exact


def _sign(v):
    return math.copysign(1.0, v)


def mul_f32(x, y):
    """one IEEE fp32 multiply of two fp32 values"""
    if math.isnan(x) or math.isnan(y):
        return NAN
    if math.isinf(x) or math.isinf(y):
        return NAN if x == 0 or y == 0 else _sign(x) * _sign(y) * INF
    if x == 0 or y == 0:
        return _sign(x) * _sign(y) * 0.0
    return round_f32(Fraction(x) * Fraction(y))


def add_f32(x, y):
    """one IEEE fp32 add"""
    if math.isnan(x) or math.isnan(y):
        return NAN
    if math.isinf(x) or math.isinf(y):
        if math.isinf(x) and math.isinf(y):
            return x if x == y else NAN
        return x if math.isinf(x) else y
    if x == 0 and y == 0:
        return -0.0 if _sign(x) < 0 and _sign(y) < 0 else 0.0
    s = Fraction(x) + Fraction(y)
    return 0.0 if s == 0 else round_f32(s)               # an exact cancellation is +0 under round-to-nearest


def fma_f32(x, y, z):
    """round(x y + z) with ONE rounding"""
    if math.isnan(x) or math.isnan(y) or math.isnan(z):
        return NAN
    if math.isinf(x) or math.isinf(y):
        if x == 0 or y == 0:
            return NAN
        p = _sign(x) * _sign(y) * INF
        return NAN if math.isinf(z) and z != p else p
    if math.isinf(z):
        return z
    if x == 0 or y == 0:
        return add_f32(_sign(x) * _sign(y) * 0.0, z)
    s = Fraction(x) * Fraction(y) + Fraction(z)
    return 0.0 if s == 0 else round_f32(s)


def _semantics(ca, ea, cw, ew, pa, pw, B, out_dtype, step):
    P = block_sums(ca, cw, B).tolist()
    ea, ew = ea.cpu().tolist(), ew.cpu().tolist()
    rows = []
    for m, row in enumerate(P):
        rows.append([])
        for n, blocks in enumerate(row):
            acc = 0.0
            for j, p in enumerate(blocks):
                x = mul_f32(float(p), scale_of(ea[m][j], pa))      # |P| <= 2^21: float(p) is exact
                acc = step(x, scale_of(ew[n][j], pw), acc)
            rows[-1].append(acc)
    return torch.tensor(rows, dtype=torch.float64).to(torch.float32).to(out_dtype)   # (fp32 values: the first convert is exact)


def kernel_semantics(ca, ea, cw, ew, pa, pw, B, out_dtype=torch.float32):
    """§8's kernel form, element by element: x = round_f32(P_j sa), acc = round_f32(x sw + acc) in ONE rounding (the fma), Inf and NaN by
    IEEE rules, byte 0 a scale of 0, byte 255 NaN; then one convert to out_dtype by torch on the CPU"""
    return _semantics(ca, ea, cw, ew, pa, pw, B, out_dtype, fma_f32)


def chain_semantics(ca, ea, cw, ew, pa, pw, B, out_dtype=torch.float32):
    """the same with two roundings per block: round_f32(x sw), then the add"""
    return _semantics(ca, ea, cw, ew, pa, pw, B, out_dtype, lambda x, sw, acc: add_f32(acc, mul_f32(x, sw)))


# ------------------------------------------------------------------------------------------------ the float64 product and its bound
def ref_and_bound_mm(ops, A, W, pa, pw, B, out_dtype=torch.float32):
    """the float64 product of the unpacked operands (unpack to float32 is exact) and (nb - 1) 2^-24 sum_j |t_j| (1 + 2^-20), plus half
    an ulp of a 16-bit output: nb - 1 ordered fp32 additions of exact block terms"""
    a, w = ops.bfp_unpack(*A, pa, B, torch.float32).double(), ops.bfp_unpack(*W, pw, B, torch.float32).double()
    nb = -(-a.shape[1] // B)
    ref = (a @ w.T).cpu()
    a, w = (torch.nn.functional.pad(t, (0, nb * B - t.shape[1])).view(-1, nb, B) for t in (a, w))   # (a ragged last block: zeros)
    t_abs = torch.einsum("mjk,njk->mnj", a, w).abs().sum(-1).cpu()
    bound = (nb - 1) * 2.0 ** -24 * t_abs * (1 + 2.0 ** -20)
    return ref, bound if out_dtype == torch.float32 else bound + 0.5 * ulp_of(ref, out_dtype)


def ref_and_bound_bmm(ops, A, W, layout, pa, pw, B, out_dtype=torch.float32):
    """the float64 batched product of the unpacked operands (unpack to float32 is exact) and (nb - 1) 2^-24 sum_j |t_j| (1 + 2^-20), plus
    half an ulp of a 16-bit output"""
    a = ops.bfp_unpack(*A, pa, B, torch.float32).double()
    cw, ew = (t.transpose(-1, -2).contiguous() for t in W) if layout == "kn" else W
    w = ops.bfp_unpack(cw, ew, pw, B, torch.float32).double()                                           # [batch, N, K]
    nb = -(-a.shape[-1] // B)
    ref = (a @ w.transpose(-1, -2)).cpu()
    a, w = (torch.nn.functional.pad(t, (0, nb * B - t.shape[-1])).view(t.shape[0], -1, nb, B) for t in (a, w))
    t_abs = torch.einsum("bmjk,bnjk->bmnj", a, w).abs().sum(-1).cpu()
    bound = (nb - 1) * 2.0 ** -24 * t_abs * (1 + 2.0 ** -20)
    return ref, bound if out_dtype == torch.float32 else bound + 0.5 * ulp_of(ref, out_dtype)
