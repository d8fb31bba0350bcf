"""The CPU checker of the outlier-aware dynamic cast (ops.outlier_fixed_qdq; DESIGN.md §8 "Outlier-aware dynamic cast"): the three steps
that DEFINE it, restated in numpy / torch CPU without the library's front end.
  1. rank: the bit pattern of |x| as float32, read as an integer (a NaN above Inf above every finite value), descending, equal patterns
     to the lower index (a stable sort): the first k positions of a segment are its outliers;
  2. inliers: the segment with +0.0 in the outliers' places through tests/_dynamic_ref.py's chain (the oracle's group_minmax, qparams and
     fixed_point_affine_cast, one segment per row);
  3. outliers: O(x) in their places -- the input's own bits (through `.to(out_dtype)` when the dtypes differ), or the oracle's
     float_quantize for a per-element float format followed by `.to(out_dtype)`.
-> (y, scale float32 [n], zero_point int64 [n], idx int32 [n, k], val [n, k]): idx / val in rank order."""
import numpy as np
import torch

import _dynamic_ref as D

qrange = D.qrange


def rank(x2, k):
    """-> int64 [n, k]: the positions of the k outliers of every row of x2, in rank order"""
    key = x2.detach().cpu().float().abs().contiguous().numpy().view(np.int32).astype(np.int64)
    order = np.argsort(-key, axis=1, kind="stable")   # descending; equal keys keep their index order: the lower index first
    return torch.from_numpy(np.ascontiguousarray(order[:, :k]))


def outlier_of(O, v, outlier_format, out_dtype):
    """O(v): outlier_format None, or (man, exp, bias, flush_subnormal)"""
    if outlier_format is None:
        return v if out_dtype == v.dtype else v.to(out_dtype)
    man, exp, bias, flush = outlier_format
    return O.float_quantize(v.float(), man, exp, bias, flush).to(out_dtype)


def outlier_ref(O, x, precision, fmt_symmetric, S, k, qscheme_symmetric, outlier_format=None, out_dtype=None):
    x = x.detach().cpu()
    out_dtype = out_dtype or x.dtype
    x2 = x.reshape(-1, S)
    if k == 0:
        y, sc, zp = D.dynamic_ref(O, x2, precision, fmt_symmetric, S, qscheme_symmetric, out_dtype)
        return y.reshape(x.shape), sc, zp, torch.empty(x2.shape[0], 0, dtype=torch.int32), torch.empty(x2.shape[0], 0, dtype=out_dtype)
    idx = rank(x2, k)
    mask = torch.zeros(x2.shape, dtype=torch.bool).scatter_(1, idx, True)
    xin = torch.where(mask, torch.zeros((), dtype=x2.dtype), x2)
    y_in, sc, zp = D.dynamic_ref(O, xin, precision, fmt_symmetric, S, qscheme_symmetric, out_dtype)
    ox = outlier_of(O, x2, outlier_format, out_dtype)
    y = torch.where(mask, ox, y_in)
    return y.reshape(x.shape), sc, zp, idx.to(torch.int32), ox.gather(1, idx)


def rel_l2(x, y):
    """|| x - y ||_2 / || x ||_2 in float64"""
    x, y = x.detach().cpu().double(), y.detach().cpu().double()
    return float((x - y).norm() / x.norm())


def student_t3(shape, seed):
    """seeded Student-t with 3 degrees of freedom, float32: z / sqrt(chi2_3 / 3)"""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal(shape)
    c = rng.chisquare(3, shape)
    return torch.from_numpy((z / np.sqrt(c / 3.0)).astype(np.float32))
