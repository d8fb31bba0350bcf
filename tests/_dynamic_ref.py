"""The CPU checker of the dynamic integer cast (ops.dynamic_fixed_qdq): the three-step chain that DEFINES it, built from
the oracle's group_minmax, qparams and fixed_point_affine_cast on x.reshape(-1, S), followed by `.to(dtype)`.  Finite inputs only --
what a NaN or an Inf does to a segment's scale is pinned against the library's own chain on the GPU (tests/test_gpu_dynamic_quant.py).
torch_restatement() spells the reference's two formulas (numerical/observer.py:59-115, numerical/cast.py:278-296 with
sim_helper.cpp:14-21's rounding) in plain torch; tests/test_dynamic_quant_host.py holds the helper to it bit for bit."""
import torch


def qrange(precision, fmt_symmetric):
    """observer.get_qmin_qmax of XP[precision,0](C..): (qmin, qmax)"""
    return -(2 ** (precision - 1)) + (1 if fmt_symmetric else 0), 2 ** (precision - 1) - 1


def segment_of(x, granularity, group_size=None):
    return {"per_token": x.shape[-1], "per_group": group_size, "per_tensor": x.numel()}[granularity]


def dynamic_ref(O, x, precision, fmt_symmetric, S, qscheme_symmetric, out_dtype=None):
    """-> (y in out_dtype (default x.dtype) with x's shape, scale float32 [n], zero_point int64 [n]); O: the oracle module"""
    x = x.detach().cpu()
    x2 = x.reshape(-1, S)
    mn, mx = O.group_minmax(x2, 0, 1)
    sc, zp = O.qparams(mn, mx, precision, fmt_symmetric, qscheme_symmetric)
    y = O.fixed_point_affine_cast(x2, precision, 0, True, fmt_symmetric, sc, zp, ch_axis=0)
    return y.to(out_dtype or x.dtype).reshape(x.shape), sc, zp


def torch_restatement(x, precision, fmt_symmetric, S, qscheme_symmetric, out_dtype=None):
    """the same three steps in plain torch on the CPU, float32 arithmetic as the reference runs it"""
    x = x.detach().cpu()
    x2 = x.float().reshape(-1, S)
    qmin, qmax = qrange(precision, fmt_symmetric)
    mn, mx = x2.amin(dim=1), x2.amax(dim=1)
    eps = torch.tensor([torch.finfo(torch.float32).eps])
    min_neg, max_pos = torch.min(mn, torch.zeros_like(mn)), torch.max(mx, torch.zeros_like(mx))
    if qscheme_symmetric:
        sc = torch.max(torch.max(-min_neg, max_pos) / (float(qmax - qmin) / 2), eps)
        zp = torch.zeros(sc.shape, dtype=torch.int64)
    else:
        sc = torch.max((max_pos - min_neg) / float(qmax - qmin), eps)
        zp = torch.clamp(qmin - torch.round(min_neg / sc).to(torch.int), qmin, qmax).to(torch.int64)
    t = x2 / sc[:, None] + zp[:, None].float()
    a1 = t + 0.5                                             # sim_helper.cpp round(a, 0.5, 0): the float32 add first,
    v = torch.round(a1.double() - 0.5).float()               # then nearbyint of the exact double difference (half to even)
    v = torch.clamp(v, float(qmin), float(qmax))             # fixed_min_max of a clamped XP[p,0]: the integer range itself
    y = (v - zp[:, None].float()) * sc[:, None]
    return y.to(out_dtype or x.dtype).reshape(x.shape), sc, zp
