"""The definition of the learned step size cast (DESIGN.md §8 "Learned step size") in CPU torch: the reference the host and GPU tests
of ops.lsq_backward / ops.lsq_fixed_qdq compare against.  float32 tensors in; every per-element operation is one float32 operation in
the order of the definition (eager CPU torch fuses nothing), the two sums per segment are float64."""
import torch


def rne_minus_half(a1):
    """csrc/fixedq.hpp rne_minus_half on a float32 tensor: nearbyint((double)a1 - 0.5), narrowed (the subtraction is exact in float64)"""
    return torch.round(a1.double() - 0.5).float()


def ulp32(v):
    """the spacing of float32 at |v| (float64 tensor in, float64 out): 2^(floor(log2 |v|) - 23), the subnormal spacing below 2^-126"""
    a = v.double().abs().clamp(min=2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


def lsq_ref(x, g, s, z, qmin, qmax, k=1.0, want_dz=True):
    """x, g: float32 [n_seg, S]; s, z: float32 [n_seg] -> (y, dx, ds, dz, abs_ts, abs_tz): y / dx float32 [n_seg, S], ds / dz float32
    [n_seg] (dz None without want_dz), abs_ts / abs_tz float64 [n_seg] = sum |ts|, sum |tz| (for the tolerance of a reordered sum)"""
    assert x.dtype == g.dtype == s.dtype == z.dtype == torch.float32 and x.dim() == 2 and x.shape == g.shape
    sc = s.reshape(-1, 1)
    zq = torch.clamp(torch.round(z), qmin, qmax).reshape(-1, 1)
    v = x / sc + zq
    r = rne_minus_half(v + 0.5)
    inside = (r >= qmin) & (r <= qmax)
    q = torch.clamp(r, qmin, qmax)
    y = (q - zq) * sc
    dx = torch.where(inside, g, torch.zeros_like(g))
    e = torch.where(inside, q - v, q - zq)
    ts = g * e
    tz = torch.where(inside, torch.zeros_like(g), -(g * sc))
    ds = (float(k) * ts.double().sum(dim=1)).float()
    dz = (float(k) * tz.double().sum(dim=1)).float() if want_dz else None
    return y, dx, ds, dz, ts.double().abs().sum(dim=1), tz.double().abs().sum(dim=1)


def sum_bound(ref, n, abs_t, k=1.0):
    """|got - ref| allowed for a float64 sum of n terms taken in another order and rounded once to float32: ulp32(ref) + n 2^-52 sum|t|
    (scaled by |k|)"""
    return ulp32(ref) + n * 2.0 ** -52 * abs(float(k)) * abs_t
