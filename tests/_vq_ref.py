"""The CPU checker of the vector codebook casts (ops.vq_qdq, ops.vq_accumulate, ops.vq_fit; DESIGN.md §8 "Vector codebook casts"): the
definition itself, in torch on the CPU.  A table C float32 [K, d]; D_k(u) = (((t_0 t_0) + t_1 t_1) + ...) + t_{d-1} t_{d-1} with
t_j = u_j - c_kj; the zero row z = the lowest k minimising D_k(0); the default norm max |c_kj|.  Per segment, in fp32: amax = max |x|
(one NaN makes it NaN); s = amax / norm, an IEEE division; s = 1 where it is not finite or below 2^-126; u = x / s; per d-vector:
best = +Inf, idx = z, for k = 0 .. K-1: D_k(u) < best takes k; y_j = c[idx][j] * s, one rounding to the output dtype.
Every binary operation below runs on two tensors of one shape (torch divides by a Python scalar as a multiplication by its
reciprocal, which is no IEEE division), and the row loop is the definition's own loop: no argmin, no NaN replacement."""
import itertools

import torch

from _codebook_ref import rel_l2, scale_rule
from _dynamic_float_ref import to_segments

INF = float("inf")


def table(rows):
    """-> c float32 [K, d] on the CPU"""
    return torch.as_tensor(rows, dtype=torch.float32).detach().cpu().clone()


def grid(levels, d):
    """the product table of a scalar codebook, rows in lexicographic order"""
    return torch.tensor(list(itertools.product([float(v) for v in levels], repeat=d)), dtype=torch.float32)


def distance(uv, row):
    """D of the vectors uv [n, d] to one row [d] -> [n]: products first, added left to right"""
    acc = None
    for j in range(uv.shape[1]):
        t = uv[:, j] - row[j].expand(uv.shape[0]).contiguous()
        p = t * t
        acc = p if acc is None else acc + p
    return acc


def choose(uv, c, z):
    """the row choice of the definition for the vectors uv [n, d] -> idx int64 [n]"""
    best = torch.full((uv.shape[0],), INF)
    idx = torch.full((uv.shape[0],), z, dtype=torch.int64)
    for k in range(c.shape[0]):
        D = distance(uv, c[k])
        lt = D < best
        best = torch.where(lt, D, best)
        idx = torch.where(lt, torch.full_like(idx, k), idx)
    return idx


def zero_row(c):
    """the lowest index minimising D_k(0): the definition's loop started anywhere ends there unless every distance is +Inf, then 0"""
    D = torch.stack([distance(torch.zeros(1, c.shape[1]), c[k])[0] for k in range(c.shape[0])])
    return int(torch.argmin(D))   # (finite entries: no NaN; the first of equal minima)


def norm_of(c, norm=None):
    return c.abs().max().reshape(1) if norm is None else torch.full((1,), norm, dtype=torch.float32)


def parts(x, rows, granularity="per_group", g=64, norm=None):
    """-> (seg [n, S] float32, back, s [n], u [n, S], idx int64 [n, S / d], c)"""
    c = table(rows)
    d = c.shape[1]
    seg, back, _ = to_segments(x.detach().cpu().float(), granularity, g)
    assert seg.shape[1] % d == 0
    amax = seg.abs().amax(dim=1)
    amax = torch.where(torch.isnan(seg).any(dim=1), torch.full_like(amax, float("nan")), amax)
    s = scale_rule(amax, norm_of(c, norm))
    u = seg / s[:, None].expand_as(seg).contiguous()
    idx = choose(u.reshape(-1, d), c, zero_row(c)).reshape(seg.shape[0], -1)
    return seg, back, s, u, idx, c


def vq_ref(x, rows, granularity="per_group", g=64, norm=None, out_dtype=None):
    """-> (y in out_dtype (default x.dtype) with x's shape, scale float32 [n_segments], index uint8 x.shape[:-1] + (L / d,))"""
    seg, back, s, u, idx, c = parts(x, rows, granularity, g, norm)
    d = c.shape[1]
    y = (c[idx].reshape(seg.shape) * s[:, None].expand_as(seg).contiguous()).to(out_dtype or x.dtype)
    return back(y), s, idx.to(torch.uint8).reshape(tuple(x.shape[:-1]) + (x.shape[-1] // d,))


def accumulate_ref(x, rows, granularity="per_group", g=64, norm=None):
    """-> (A float64 [K, d + 2], mag float64 [K, d + 1]): the k-means statistics over the vectors whose d quotients are all finite, and
    per row the sums of |w u_j| (columns 0 .. d-1) and of w (column d): the magnitudes that bound the error of a float64 sum taken in
    another order"""
    seg, _, s, u, idx, c = parts(x, rows, granularity, g, norm)
    K, d = c.shape
    uv = u.reshape(-1, d)
    fin = torch.isfinite(uv).all(dim=1)
    w = (s.double() * s.double())[:, None].expand(-1, seg.shape[1] // d).reshape(-1)[fin]
    k, ud = idx.reshape(-1)[fin], uv[fin].double()
    terms = torch.cat([w[:, None] * ud, w[:, None], torch.ones_like(w)[:, None]], dim=1)
    A = torch.zeros(K, d + 2, dtype=torch.float64).index_add_(0, k, terms)
    mag = torch.zeros(K, d + 1, dtype=torch.float64).index_add_(0, k, terms[:, :d + 1].abs())
    return A, mag


def kmeans_step(rows, A):
    """c_k <- float(A[k, :d] / A[k, d]) where A[k, d + 1] > 0; an empty row keeps its value"""
    c = table(rows)
    d = c.shape[1]
    return torch.where(A[:, d + 1:d + 2] > 0, (A[:, :d] / A[:, d:d + 1]).float(), c)


def sample_init(x, K, d, granularity="per_group", g=64, norm=1.0):
    """row i = the quotient vector number floor((2 i + 1) n / (2 K)) of x, u under `norm`"""
    seg, _, _ = to_segments(x.detach().cpu().float(), granularity, g)
    amax = seg.abs().amax(dim=1)
    amax = torch.where(torch.isnan(seg).any(dim=1), torch.full_like(amax, float("nan")), amax)
    s = scale_rule(amax, torch.full((1,), norm, dtype=torch.float32))
    uv = (seg / s[:, None].expand_as(seg).contiguous()).reshape(-1, d)
    n = uv.shape[0]
    return uv[[(2 * i + 1) * n // (2 * K) for i in range(K)]].clone()


def fit_ref(x, rows, granularity="per_group", g=64, norm=None, iters=7):
    """-> (table, norm, history): norm resolved once from the initial table; the relative L2 error before every step and after the last"""
    c = table(rows)
    norm = float(norm_of(c, norm)[0])
    hist = []
    for _ in range(iters):
        hist.append(rel_l2(x, vq_ref(x, c, granularity, g, norm)[0]))
        c = kmeans_step(c, accumulate_ref(x, c, granularity, g, norm)[0])
    hist.append(rel_l2(x, vq_ref(x, c, granularity, g, norm)[0]))
    return c, norm, hist
