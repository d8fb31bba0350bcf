"""The CPU checker of the two-level block-scaled float cast (ops.block_scaled_float_qdq): the definition itself, in torch
on the CPU with the oracle's floating_point_cast as float_q of both the element format E and the scale format Sf.  In fp32:
    t  = the tensor scale: given, 1 when absent, or (max |x| / fmax) / scale_max over the whole tensor (one NaN makes the maximum NaN);
         1 where it is not finite or below 2^-126
    a  = max |x| per group (one NaN makes it NaN);  c = (a / fmax) / t;  sq = min(float_q_Sf(c), scale_max);  s = sq * t
    s usable (finite, >= 2^-126):  y = float_q_E(x / s) * s, one rounding to the output dtype
    else:                          y = a zero with the sign bit of float_q_E(x), and the reported s is 0
Every binary operation below runs on two tensors of one shape (torch divides by a Python scalar as a multiplication by its reciprocal,
which is no IEEE division)."""
import torch

from _dynamic_float_ref import FMAX, FORMATS, SHORTHAND, fmax_of   # noqa: F401  (the element formats: man, exp, bias, flush)

SCALE_FORMATS = {"e4m3": (3, 4, 7, False), "e5m2": (2, 5, 15, False)}
SCALE_SHORTHAND = {"e4m3": "FP[1|4|3,7](_N)", "e5m2": "FP[1|5|2,15](_N)"}
TINY = 2.0 ** -126


def usable(s):
    return torch.isfinite(s) & (s >= torch.full_like(s, TINY))


def amax_nan(seg):
    """max |x| of every row of a float32 matrix, NaN where the row holds one"""
    amax = seg.abs().amax(dim=1)
    return torch.where(torch.isnan(seg).any(dim=1), torch.full_like(amax, float("nan")), amax)


def tensor_scale_ref(x, fmt, scale_max, tensor_scale="dynamic"):
    """step 1 -> float32 [1]"""
    man, exp, _, _ = fmt
    if tensor_scale is None:
        t = torch.ones(1)
    elif isinstance(tensor_scale, str):
        A = amax_nan(x.detach().cpu().float().reshape(1, -1))
        t = (A / torch.full_like(A, fmax_of(man, exp))) / torch.full_like(A, scale_max)
    else:
        t = torch.as_tensor(tensor_scale, dtype=torch.float32).detach().cpu().reshape(1).clone()
    return torch.where(usable(t), t, torch.ones_like(t))


def block_scaled_ref(O, x, fmt, g, scale_fmt, scale_max=None, tensor_scale="dynamic", out_dtype=None):
    """-> (y in out_dtype (default x.dtype) with x's shape, scale float32 [n_groups], scale_code_value float32 [n_groups], tensor_scale
    float32 [1]); O: the oracle module; fmt, scale_fmt: (man, exp, bias, flush)"""
    man, exp, bias, flush = fmt
    sman, sexp, sbias, sflush = scale_fmt
    scale_max = fmax_of(sman, sexp) if scale_max is None else float(scale_max)
    x = x.detach().cpu()
    t = tensor_scale_ref(x, fmt, scale_max, tensor_scale)
    seg = x.float().reshape(-1, g)
    a = amax_nan(seg)
    te = t.expand_as(a).contiguous()
    c = (a / torch.full_like(a, fmax_of(man, exp))) / te
    sq = torch.minimum(O.floating_point_cast(c.contiguous(), sman, sexp, sbias, sflush), torch.full_like(c, scale_max))
    s = sq * te
    ok = usable(s)
    se = torch.where(ok, s, torch.ones_like(s))[:, None].expand_as(seg).contiguous()
    y = O.floating_point_cast((seg / se).contiguous(), man, exp, bias, flush) * se
    z = O.floating_point_cast(seg.contiguous(), man, exp, bias, flush)
    y = torch.where(ok[:, None].expand_as(seg), y, torch.copysign(torch.zeros_like(z), z))
    return y.to(out_dtype or x.dtype).reshape(x.shape), torch.where(ok, s, torch.zeros_like(s)), sq, t
