"""The CPU checker of the codebook casts (ops.codebook_qdq, ops.codebook_accumulate, ops.codebook_fit; DESIGN.md §8 "Codebook casts"):
the definition itself, in torch on the CPU.  A table of K non-decreasing float32 levels c; thresholds t_j = (c_j + c_{j+1}) * 0.5; the
zero level z = the lowest index of the level with the smallest |c|.  Per segment, in fp32: amax = max |x| (one NaN makes it NaN);
s = amax / norm, an IEEE division (norm None: max(|c_0|, |c_{K-1}|)); s = 1 where it is not finite or below 2^-126; u = x / s;
idx = #{j : u > t_j} = bucketize(u, t, right=False), a NaN u takes idx = z; y = c[idx] * s, one rounding to the output dtype.
Every binary operation below runs on two tensors of one shape (torch divides by a Python scalar as a multiplication by its
reciprocal, which is no IEEE division)."""
import torch

from _dynamic_float_ref import to_segments

NF4 = (-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453, -0.28444138169288635, -0.18477343022823334,
       -0.09105003625154495, 0.0, 0.07958029955625534, 0.16093020141124725, 0.24611230194568634, 0.33791524171829224,
       0.44070982933044434, 0.5626170039176941, 0.7229568362236023, 1.0)
FP4_E2M1 = (-6.0, -4.0, -3.0, -2.0, -1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
IRREGULAR5 = (-1.0, -0.25, -0.25, 0.125, 0.75)   # one duplicated level
TWO = (-0.5, 1.0)
TABLES = {"nf4": NF4, "fp4_e2m1": FP4_E2M1, "irregular5": IRREGULAR5, "two": TWO}


def table(levels):
    """-> (c float32 [K], t float32 [K - 1], z)"""
    c = torch.as_tensor(levels, dtype=torch.float32).detach().cpu().clone()
    t = (c[:-1] + c[1:]) * torch.full_like(c[:-1], 0.5)
    z = int(torch.argmin(c.abs()))   # (the first of equal minima)
    return c, t, z


def norm_of(c, norm=None):
    return torch.maximum(c[0].abs(), c[-1].abs()).reshape(1) if norm is None else torch.full((1,), norm, dtype=torch.float32)


def scale_rule(amax, norm):
    s = amax / norm.expand_as(amax).contiguous()
    ok = torch.isfinite(s) & (s >= torch.full_like(s, 2.0 ** -126))
    return torch.where(ok, s, torch.ones_like(s))


def parts(x, levels, granularity="per_group", g=64, norm=None):
    """-> (seg [n, S] float32, back, s [n], u [n, S], idx int64 [n, S], c)"""
    c, t, z = table(levels)
    seg, back, _ = to_segments(x.detach().cpu().float(), granularity, g)
    amax = seg.abs().amax(dim=1)
    amax = torch.where(torch.isnan(seg).any(dim=1), torch.full_like(amax, float("nan")), amax)
    s = scale_rule(amax, norm_of(c, norm))
    u = seg / s[:, None].expand_as(seg).contiguous()
    idx = torch.bucketize(u, t, right=False)
    idx = torch.where(torch.isnan(u), torch.full_like(idx, z), idx)   # (bucketize puts a NaN past the last threshold)
    return seg, back, s, u, idx, c


def codebook_ref(x, levels, granularity="per_group", g=64, norm=None, out_dtype=None):
    """-> (y in out_dtype (default x.dtype) with x's shape, scale float32 [n_segments], index uint8 with x's shape)"""
    seg, back, s, u, idx, c = parts(x, levels, granularity, g, norm)
    y = (c[idx] * s[:, None].expand_as(seg).contiguous()).to(out_dtype or x.dtype)
    return back(y), s, back(idx.to(torch.uint8))


def accumulate_ref(x, levels, granularity="per_group", g=64, norm=None):
    """-> (A float64 [K, 3], sum |w u| per level, sum w per level): the Lloyd statistics over the elements with a finite u, and the
    magnitudes that bound the error of a float64 sum taken in another order"""
    seg, _, s, u, idx, c = parts(x, levels, granularity, g, norm)
    fin = torch.isfinite(u)
    w = (s.double() * s.double())[:, None].expand_as(u)[fin]
    k, ud = idx[fin], u[fin].double()
    A = torch.zeros(c.shape[0], 3, dtype=torch.float64)
    A[:, 0].index_add_(0, k, w * ud)
    A[:, 1].index_add_(0, k, w)
    A[:, 2].index_add_(0, k, torch.ones_like(w))
    mag = torch.zeros(c.shape[0], dtype=torch.float64).index_add_(0, k, (w * ud).abs())
    return A, mag, A[:, 1].clone()


def lloyd_step(levels, A):
    c = torch.as_tensor(levels, dtype=torch.float32).cpu()
    return torch.where(A[:, 2] > 0, (A[:, 0] / A[:, 1]).float(), c)


def rel_l2(x, y):
    x, y = x.detach().cpu().double(), y.detach().cpu().double()
    return float(torch.sqrt(((x - y) ** 2).sum() / (x ** 2).sum()))


def fit_ref(x, levels, granularity="per_group", g=64, norm=None, iters=7):
    """-> (levels, norm, history): norm resolved once from the initial table; the relative L2 error before every step and after the last"""
    c = torch.as_tensor(levels, dtype=torch.float32).cpu().clone()
    norm = float(norm_of(c, norm)[0])
    hist = []
    for _ in range(iters):
        hist.append(rel_l2(x, codebook_ref(x, c, granularity, g, norm)[0]))
        c = lloyd_step(c, accumulate_ref(x, c, granularity, g, norm)[0])
    hist.append(rel_l2(x, codebook_ref(x, c, granularity, g, norm)[0]))
    return c, norm, hist
