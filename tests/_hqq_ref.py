"""The CPU checker of HQQ (ops.hqq_qdq; DESIGN.md §8 "HQQ"): the definition itself, in float32 torch on the CPU, no product import.
Every binary operation runs on two float32 tensors (torch divides by a Python scalar as a multiplication by its reciprocal, which is
no IEEE division), the sums over a group are the adjacent-pair tree taken by slicing, and no operation here can be contracted into
an FMA (each is its own call).  The square root is numpy's, not torch's: torch's CPU sqrt goes through a vector math library that is
accurate to an ulp but NOT correctly rounded (about 0.8 % of random float32 values come out one ulp off), numpy's is the hardware
instruction, which is (the same values as the float64 root rounded once)."""
import numpy as np
import torch


def qrange(precision, symmetric):
    """observer.get_qmin_qmax of a clamped XP[precision,0]"""
    return -(2 ** (precision - 1)) + (1 if symmetric else 0), 2 ** (precision - 1) - 1


def tree_sum(v):
    """sum over the last dim as the adjacent-pair tree (an odd length carries its last value up unchanged)"""
    while v.shape[-1] > 1:
        n = v.shape[-1]
        h = v[..., 0:n - 1:2] + v[..., 1::2]
        v = torch.cat([h, v[..., -1:]], -1) if n % 2 else h
    return v[..., 0]


def _full(like, v):
    return torch.full_like(like, float(v))


def sqrt_rn(a):
    """the correctly rounded float32 square root (see the module's docstring)"""
    return torch.from_numpy(np.sqrt(a.contiguous().numpy()))


def extrema(W):
    """(mn, mx) [n, 1]: one NaN in a group makes both NaN"""
    mn, mx = W.amin(dim=1, keepdim=True), W.amax(dim=1, keepdim=True)
    nan = torch.isnan(W).any(dim=1, keepdim=True)
    return torch.where(nan, _full(mn, "nan"), mn), torch.where(nan, _full(mx, "nan"), mx)


def scale_of(mn, mx, qmin, qmax):
    s = (mx - mn) / _full(mn, qmax - qmin)
    ok = torch.isfinite(s) & (s >= _full(s, 2.0 ** -126))
    s = torch.where(ok, s, torch.ones_like(s))
    return s, torch.ones_like(s) / s


def quantise(W, rs, z, qmin, qmax):
    return torch.clamp(torch.round(W * rs + z), qmin, qmax)


def betas(beta, kappa, iters):
    b, k, out = np.float32(beta), np.float32(kappa), []
    for _ in range(iters):
        out.append(float(np.float32(1.0) / b))
        b = np.float32(b * k)
    return out


def hqq_ref(x, qmin, qmax, g=64, lp_norm=0.5, beta=10.0, kappa=1.01, iters=20, out_dtype=None, history=False):
    """-> (y in out_dtype (default x.dtype) with x's shape, scale float32 [n], zero float32 [n], codes uint8 with x's shape
    [, per-group kept L1 error after every k: float32 [iters + 1, n]])"""
    W = x.detach().cpu().float().reshape(-1, g)
    mn, mx = extrema(W)
    s, rs = scale_of(mn, mx, qmin, qmax)
    z = _full(mn, qmin) - mn * rs
    inv_g = _full(mn, float(np.float32(1.0 / g)))
    ibs = betas(beta, kappa, iters)
    zb = eb = None
    hist = []
    for k in range(iters + 1):
        q = quantise(W, rs, z, qmin, qmax)
        d = W - (q - z) * s
        a = d.abs()
        err = tree_sum(a)[:, None]
        if k == 0:
            zb, eb = z, err
        else:
            better = err < eb
            zb, eb = torch.where(better, z, zb), torch.where(better, err, eb)
        hist.append(eb[:, 0].clone())
        if k == iters:
            break
        ib = _full(a, ibs[k])
        if lp_norm == 1.0:
            t = ib
        elif lp_norm == 0.5:
            t = ib / sqrt_rn(a)
        else:
            t = ib * a.pow(lp_norm - 1.0)
        e = torch.copysign(torch.clamp(a - t, min=0), d)
        z = tree_sum(q - (W - e) * rs)[:, None] * inv_g
    q = quantise(W, rs, zb, qmin, qmax)
    y = ((q - zb) * s).to(out_dtype or x.dtype).reshape(x.shape)
    codes = torch.where(q == q, q - qmin, torch.zeros_like(q)).to(torch.uint8).reshape(x.shape)
    out = (y, s[:, 0].clone(), zb[:, 0].clone(), codes)
    return out + (torch.stack(hist),) if history else out


def rtn_closed_form(x, qmin, qmax, g):
    """round-to-nearest on the min/max grid with the float zero point of step 3, written without the loop"""
    W = x.detach().cpu().float().reshape(-1, g)
    mn, mx = extrema(W)
    s, rs = scale_of(mn, mx, qmin, qmax)
    z = _full(mn, qmin) - mn * rs
    q = quantise(W, rs, z, qmin, qmax)
    return ((q - z) * s).to(x.dtype).reshape(x.shape), s[:, 0], z[:, 0]


def group_l1(x, y, g):
    return tree_sum((x.detach().cpu().float().reshape(-1, g) - y.detach().cpu().float().reshape(-1, g)).abs())


# the special groups of DESIGN.md §8 "HQQ" (g elements each): name -> a function of (g) giving the float32 group
def special_groups(g):
    base = torch.linspace(-1.0, 2.0, g)
    nan = base.clone(); nan[g // 3] = float("nan")
    pinf = base.clone(); pinf[1] = float("inf")
    ninf = base.clone(); ninf[g - 2] = float("-inf")
    over = base.clone(); over[0] = -3.0e38; over[g - 1] = 3.0e38
    return {"zero": torch.zeros(g), "constant": torch.full((g,), 3.0), "nan": nan, "pinf": pinf, "ninf": ninf, "overflow": over}


def plant(x, g, where=("first", "middle", "last")):
    """x [rows, cols] with the special groups written over groups at the start, the middle and the end of the flat group list
    -> (x, {name: [group indices]})"""
    x = x.clone()
    flat = x.reshape(-1, g)
    n = flat.shape[0]
    sp = special_groups(g)
    spots, at = {k: [] for k in sp}, {"first": 0, "middle": max(n // 2 - len(sp) // 2, 0), "last": n - len(sp)}
    for w in where:
        for j, (name, v) in enumerate(sp.items()):
            i = min(at[w] + j, n - 1)
            flat[i] = v.to(x.dtype)
            spots[name] = [k for k in spots[name] if k != i] + [i]
            for other in spots:
                if other != name and i in spots[other]:
                    spots[other].remove(i)
    return x, spots
