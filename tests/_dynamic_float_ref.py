"""The CPU checker of the dynamic scaled float cast (ops.dynamic_float_qdq): the definition itself, in torch on the CPU
with the oracle's floating_point_cast as float_q.  Per segment, in fp32: amax = max |x| (one NaN makes it NaN); s = amax / fmax, an
IEEE division; with pow2_scale s is rounded up to a power of two on its bits; s = 1 where it is not finite or below 2^-126;
y = float_q(x / s) * s, one rounding to the output dtype.  Every binary operation below runs on two tensors of one shape (torch
divides by a Python scalar as a multiplication by its reciprocal, which is no IEEE division)."""
import torch

FORMATS = {"e4m3": (3, 4, 7, False), "e4m3_flush": (3, 4, 7, True), "e5m2": (2, 5, 15, False), "e2m1": (1, 2, 1, False)}   # man, exp, bias, flush
SHORTHAND = {"e4m3": "FP[1|4|3,7](_N)", "e4m3_flush": "FP[1|4|3,7](FN)", "e5m2": "FP[1|5|2,15](_N)", "e2m1": "FP[1|2|1,1](_N)"}
FMAX = {"e4m3": 480.0, "e4m3_flush": 480.0, "e5m2": 114688.0, "e2m1": 6.0}


def fmax_of(man, exp):
    return float(2.0 ** (2 ** (exp - 1)) * (2.0 - 2.0 ** -man))


def to_segments(x, granularity, g=None):
    """-> (x as [n_segments, S], a function that puts such a matrix back into x's shape, the shape of the scales)"""
    if granularity == "per_tile":
        R, C = x.shape[-2:]
        B = x.numel() // (R * C)
        seg = x.reshape(B, R // g, g, C // g, g).permute(0, 1, 3, 2, 4).reshape(-1, g * g)
        back = lambda y: y.reshape(B, R // g, C // g, g, g).permute(0, 1, 3, 2, 4).reshape(x.shape)   # noqa: E731
        return seg, back, tuple(x.shape[:-2]) + (R // g, C // g)
    S = {"per_token": x.shape[-1], "per_group": g, "per_tensor": x.numel()}[granularity]
    seg = x.reshape(-1, S)
    return seg, (lambda y: y.reshape(x.shape)), (seg.shape[0],)


def scale_rule(amax, fmax, pow2_scale):
    """steps 2 - 4 of the definition on a float32 tensor of absolute maxima"""
    s = amax / torch.full_like(amax, fmax)
    if pow2_scale:
        b = s.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        b = ((b & 0x7F800000) + torch.where((b & 0x007FFFFF) != 0, 0x00800000, 0)) & 0xFFFFFFFF
        b = torch.where(b >= 0x80000000, b - (1 << 32), b).to(torch.int32)
        s = b.view(torch.float32)
    ok = torch.isfinite(s) & (s >= torch.full_like(s, 2.0 ** -126))
    return torch.where(ok, s, torch.ones_like(s))


def dynamic_float_ref(O, x, fmt, granularity, g=None, pow2_scale=False, out_dtype=None):
    """-> (y in out_dtype (default x.dtype) with x's shape, scale float32 in the op's shape); O: the oracle module; fmt: (man, exp,
    bias, flush)"""
    man, exp, bias, flush = fmt
    x = x.detach().cpu()
    seg, back, sc_shape = to_segments(x.float(), granularity, g)
    a = seg.abs()
    amax = a.amax(dim=1)
    amax = torch.where(torch.isnan(seg).any(dim=1), torch.full_like(amax, float("nan")), amax)
    s = scale_rule(amax, fmax_of(man, exp), pow2_scale)
    se = s[:, None].expand_as(seg).contiguous()
    q = O.floating_point_cast((seg / se).contiguous(), man, exp, bias, flush)
    y = (q * se).to(out_dtype or x.dtype)
    return back(y), s.reshape(sc_shape)
