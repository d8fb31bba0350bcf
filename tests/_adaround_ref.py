"""The definition of the AdaRound cast and its backward (DESIGN.md §8 "AdaRound") in CPU torch: the reference the host and GPU tests of
ops.adaround_qdq / ops.adaround_backward compare against, the error bounds that go with it and the inputs both test files use.

  truth(...)    f = floor of the FLOAT32 quotient w / s (floor is discontinuous: the one place where the kernel's own arithmetic is part of
                the definition), everything after it in float64, with the exact values of the float32 constants G, ZG, beta - 1, -2 beta
                and reg_weight;
  spelled(...)  the definition in float32, one torch operation per operation, in its order (eager CPU torch fuses nothing);
  bounds(...)   per element, how far a conforming float32 evaluation may lie from the truth: forward error analysis of the pinned
                spelling (DESIGN.md §8 "AdaRound" has the derivation), starting from the DOCUMENTED 1 ulp of the device's expf and powf (HIP
                math API) -- nothing here is taken from the code under test.
Nothing here needs a GPU."""
import math

import torch

U = 2.0 ** -24          # the unit roundoff of float32: one correctly rounded operation is off by at most U relative
EXP_ULPS = 1.0          # expf and powf of the device library: at most 1 ulp, i.e. a relative error of at most 2^-23
POW_ULPS = 1.0
TINY = 2.0 ** -126      # below the normal range a result (a flushed 1 / Inf, an underflowing power) is off by at most this, absolutely
SLACK = 1.001           # the products of two relative errors of at most 2^-20 each that the first-order sums below leave out
EDGE = 2.0 ** -20       # dV is not compared where the truth's hr lies this close to 0 or 1: the live decision may flip there

G = torch.tensor(-0.1, dtype=torch.float32).item()
ZG = (torch.tensor(1.1, dtype=torch.float32) - torch.tensor(-0.1, dtype=torch.float32)).item()
assert ZG == torch.tensor(1.2, dtype=torch.float32).item()

# V values every test tensor carries: 0, the hr boundaries (truth hr 4.3e-7 beyond 1 and below 0: more than any conforming h is off),
# saturation and expf overflow.  All but 0 are dead: dV is exactly 0 there.
PLANTED = (0.0, 2.3979, -2.3979, 20.0, -20.0, 100.0, -100.0)


def consts(beta, reg_weight):
    """(bm1, m2b, rw): beta - 1, -2 beta and reg_weight as the float32 values the definition uses (both differences are exact)"""
    b = torch.tensor(float(beta), dtype=torch.float32)
    return (b - 1.0).item(), (-2.0 * b).item(), torch.tensor(float(reg_weight), dtype=torch.float32).item()


def _check(w, V, g, s, zq):
    assert w.dtype == V.dtype == s.dtype == zq.dtype == torch.float32 and w.dim() == 2 and w.shape == V.shape
    assert g is None or (g.dtype == torch.float32 and g.shape == w.shape)
    assert s.shape == zq.shape == (w.shape[0],)


def truth(w, V, g, s, zq, qmin, qmax, beta=2.0, reg_weight=0.0, hard=False, V64=None):
    """w, V, g: float32 [n_seg, S] (g may be None: no backward); s, zq: float32 [n_seg] -> dict of float64 tensors: f, sg, hr, h, t, y,
    in01, cell, dh, rec, t2, a, phi (= sign(t2) a^(beta - 1)), r, dreg, dV, reg.  V64: a float64 leaf to differentiate through in place of V."""
    _check(w, V, g, s, zq)
    bm1, m2b, rw = consts(beta, reg_weight)
    sc, z = s.double()[:, None], zq.double()[:, None]
    f = torch.floor(w / s[:, None]).double()          # the float32 quotient
    Vd = V.double() if V64 is None else V64
    sg = 1.0 / (1.0 + torch.exp(-Vd))
    hr = sg * ZG + G
    h = (Vd >= 0).double() if hard else torch.clamp(hr, 0.0, 1.0)
    t = (f + h) + z
    y = (torch.clamp(t, qmin, qmax) - z) * sc
    out = dict(f=f, sg=sg, hr=hr, h=h, t=t, y=y)
    if g is None:
        return out
    in01 = (hr > 0) & (hr < 1)
    cell = (f + z >= qmin) & (f + z <= qmax - 1)
    dh = sg * (1.0 - sg) * ZG
    rec = torch.where(in01 & cell, g.double() * sc * dh, torch.zeros_like(dh))
    t2 = 2.0 * h - 1.0
    a = t2.abs()
    p1 = a.pow(bm1)
    phi = torch.sign(t2) * p1
    r = 1.0 - p1 * a
    dreg = torch.where(in01, rw * (m2b * phi * dh), torch.zeros_like(dh))
    out.update(in01=in01, cell=cell, dh=dh, rec=rec, t2=t2, a=a, phi=phi, r=r, dreg=dreg, dV=rec + dreg, reg=r.sum())
    return out


def spelled(w, V, g, s, zq, qmin, qmax, beta=2.0, reg_weight=0.0, hard=False, mistake=None):
    """the definition in float32 -> dict of float32 tensors y, h, dh, ab (= a^beta as spelled), dV and the float64 scalar reg.
    mistake: None, or one planted error for the test that the bounds notice it -- "no_factor_2" (d|2h - 1| without its 2),
    "beta_exponent" (a^beta in place of a^(beta - 1) in the gradient), "no_clamp" (h = hr)."""
    _check(w, V, g, s, zq)
    assert mistake in (None, "no_factor_2", "beta_exponent", "no_clamp")
    bm1, m2b, rw = consts(beta, reg_weight)
    sc, z = s[:, None], zq[:, None]
    f = torch.floor(w / sc)
    sg = 1.0 / (1.0 + torch.exp(-V))
    hr = sg * ZG + G
    if hard:
        h = (V >= 0).float()
    else:
        h = hr if mistake == "no_clamp" else torch.clamp(hr, 0.0, 1.0)
    q = torch.clamp((f + h) + z, qmin, qmax)
    out = dict(y=(q - z) * sc, h=h)
    if g is None:
        return out
    fz = f + z
    cell = (fz >= qmin) & (fz <= qmax - 1)
    in01 = (hr > 0) & (hr < 1)
    dh = (sg * (1.0 - sg)) * ZG
    zero = torch.zeros_like(dh)
    dV = torch.where(in01 & cell, (g * sc) * dh, zero)
    t2 = 2.0 * h - 1.0
    a = torch.abs(t2)
    p1 = torch.pow(a, bm1)
    ab = p1 * a
    if rw != 0.0:
        pg = torch.pow(a, float(beta)) if mistake == "beta_exponent" else p1
        c = m2b / 2.0 if mistake == "no_factor_2" else m2b
        dV = dV + torch.where(in01, rw * (((c * pg) * torch.sign(t2)) * dh), zero)
    out.update(dh=dh, ab=ab, dV=dV, reg=(1.0 - ab).sum(dtype=torch.float64))
    return out


def _phi(t, bm1):
    return torch.sign(t) * t.abs().pow(bm1)


def bounds(tr, g, s, qmin, qmax, beta=2.0, reg_weight=0.0):
    """tr: truth(...) with a gradient -> dict of float64 tensors, the allowed |float32 evaluation - truth| of h, dh, y (in float32, before
    any narrowing), ab (= a^beta), r, dV per element.  First-order forward error analysis; see DESIGN.md §8 "AdaRound"."""
    bm1, m2b, rw = consts(beta, reg_weight)
    e_exp, e_pow = EXP_ULPS * 2.0 ** -23, POW_ULPS * 2.0 ** -23
    sc = s.double()[:, None]
    sg, hr, h = tr["sg"], tr["hr"], tr["h"]
    dh = sg * (1.0 - sg) * ZG
    # E = expf(-V) within e_exp; 1 + E and the reciprocal one rounding each: E / (1 + E) = 1 - sg of E's error reaches sg
    sg_abs = sg * (e_exp * (1.0 - sg) + 2.0 * U) + TINY
    # hr = fl(fl(sg ZG) + G); the clamp does not stretch
    h_abs = ZG * sg_abs + U * (sg * ZG) + U * hr.abs()
    # dh = fl(fl(sg fl(1 - sg)) ZG)
    om_abs = sg_abs + U * (1.0 - sg)
    prod_abs = sg_abs * (1.0 - sg) + sg * om_abs + U * sg * (1.0 - sg)
    dh_abs = ZG * prod_abs + U * dh
    out = dict(h=SLACK * h_abs, dh=SLACK * dh_abs)
    # y = fl(fl(clamp(fl(fl(f + h) + zq)) - zq) s): where the truth's t is further outside the range than its own error the clamp is exact
    f, t = tr["f"], tr["t"]
    pre = h_abs + U * ((f + h).abs() + t.abs())
    q_abs = torch.where((t < qmin - pre) | (t > qmax + pre), torch.zeros_like(pre), pre)
    q = torch.clamp(t, qmin, qmax)
    z = t - (f + h)
    out["y"] = SLACK * (sc * (q_abs + U * (q - z).abs()) + U * tr["y"].abs())
    if "dV" not in tr:
        return out
    gs = (g.double() * sc).abs()
    rec_abs = torch.where(tr["in01"] & tr["cell"], gs * dh_abs + 2.0 * U * tr["rec"].abs(), torch.zeros_like(dh))
    # t2 = fl(2 h - 1); phi(t) = sign(t) |t|^(beta - 1) is monotone, so the error of t2 moves it at most to phi's value at the interval's ends
    t2, a, phi = tr["t2"], tr["a"], tr["phi"]
    t_abs = 2.0 * h_abs + U * a
    phi_hi, phi_lo = _phi(t2 + t_abs, bm1), _phi(t2 - t_abs, bm1)
    phi_abs = torch.maximum(phi_hi - phi, phi - phi_lo) + e_pow * torch.maximum(phi_hi.abs(), phi_lo.abs()) + TINY
    # ab = fl(p1 a), r = fl(1 - ab): absolute throughout, a = |2 h - 1| cancels near h = 0.5
    ab = phi.abs() * a
    ab_abs = phi_abs * (a + t_abs) + phi.abs() * t_abs + U * ab + TINY
    out["ab"] = SLACK * ab_abs
    out["r"] = SLACK * (ab_abs + U * tr["r"].abs())
    # dreg = fl(rw fl(fl(fl(m2b p1) sign) dh)): three roundings on top of the factors' errors
    dreg_abs = torch.where(tr["in01"], abs(rw * m2b) * (phi_abs * (dh + dh_abs) + phi.abs() * dh_abs) + 3.0 * U * tr["dreg"].abs(),
                           torch.zeros_like(dh))
    out["dV"] = SLACK * (rec_abs + dreg_abs + U * tr["dV"].abs())
    return out


def near_edge(tr):
    """elements whose truth hr lies within EDGE of 0 or 1"""
    hr = tr["hr"]
    return (hr.abs() <= EDGE) | ((hr - 1.0).abs() <= EDGE)


def edge_share(tr, planted):
    """the share of the elements outside `planted` (checked on their own) that near_edge leaves out of the dV comparison"""
    free = torch.ones(tr["hr"].numel(), dtype=torch.bool)
    free[planted] = False
    e = near_edge(tr).reshape(-1)[free]
    return e.float().mean().item() if e.numel() else 0.0


def half_ulp_out(y, y_abs, dtype):
    """half a unit in the last place of the 16-bit output dtype around |y| + y_abs (0 for float32: its rounding is in the bound already)"""
    if dtype == torch.float32:
        return torch.zeros_like(y)
    man, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    a = (y.abs() + y_abs).clamp(min=2.0 ** emin)
    return 0.5 * torch.exp2(torch.floor(torch.log2(a)) - man)


def round_half_up(w, s):
    """floor(v + 0.5) of the float32 quotient v = w / s, exactly (float64 holds v + 0.5)"""
    return torch.floor((w / s[:, None]).double() + 0.5)


# ------------------------------------------------------------------------------------------------ the inputs of the host and GPU tests
def make(n_seg, S, dtype, qmin, qmax, seed):
    """-> (w in `dtype`, V float32, g in `dtype`: [n_seg, S]; s, zq: float32 [n_seg]; planted: the flat indices that hold PLANTED).
    w ~ N(0, 1) against scales around 1 / qmax, so a good share of the elements clips on both sides; integer zero points inside the
    range, nonzero where the range is asymmetric; V uniform in [-4, 4] with PLANTED written over its first elements."""
    gen = torch.Generator().manual_seed(seed)
    w = torch.randn(n_seg, S, generator=gen).to(dtype)
    g = torch.randn(n_seg, S, generator=gen).to(dtype)
    V = torch.rand(n_seg, S, generator=gen) * 8.0 - 4.0
    s = (torch.rand(n_seg, generator=gen) + 0.5) * (1.0 / qmax)
    if qmin + qmax != 0:
        zq = torch.randint(qmin // 2, qmax // 2 + 1, (n_seg,), generator=gen).float()
    else:
        zq = torch.zeros(n_seg)
    k = min(len(PLANTED), V.numel())
    planted = torch.arange(k) * max(1, V.numel() // k)       # spread over the tensor: several segments, several workgroups
    V.view(-1)[planted] = torch.tensor(PLANTED[:k])
    return w, V, g, s, zq, planted


def correlated_tokens(n, c, seed):
    """n tokens of c correlated channels (the triage prototype's calibration data): a random mixing of unit normals with decaying gains"""
    gen = torch.Generator().manual_seed(seed)
    mix = torch.randn(c, c, generator=gen) / math.sqrt(c)
    gains = torch.exp(-torch.arange(c, dtype=torch.float32) / (c / 4.0)) * 3.0 + 0.1
    return (torch.randn(n, c, generator=gen) * gains) @ mix


# ------------------------------------------------------------------------------------------------ the cases of the host and GPU tests
#            format,        beta, reg_weight
SETTINGS = [("XP[4,0](C_N)", 2.0, 0.37), ("XP[8,0](CSN)", 3.7, 0.01), ("XP[2,0](CSN)", 10.3, 1.0), ("XP[4,0](CSN)", 20.0, 0.05)]


def vec(dtype):
    return 4 if dtype == torch.float32 else 8


def tensor_sizes(scratch_bytes, dtype):
    """one vector; just past one workgroup's share; several partial sums with a ragged last workgroup -- found from
    ops.adaround_scratch_bytes as tests/test_gpu_lsq.py _tensor_sizes does"""
    V, one = vec(dtype), scratch_bytes(vec(dtype))
    share = V
    while scratch_bytes(share * 2) == one:
        share *= 2
    assert scratch_bytes(share) == one and scratch_bytes(share + V) == 2 * one
    several = 3 * share + 5 * V
    assert scratch_bytes(several) == 4 * one
    return [V, share + V, several]


def geometries(scratch_bytes, dtype):
    """[(name, (n_seg, S), granularity, group_size, class)]: the smallest shapes at which the kernels can go wrong"""
    V = vec(dtype)
    one, past, several = tensor_sizes(scratch_bytes, dtype)
    return [("one_vector_groups", (15, V), "per_group", V, "shift"), ("group16", (128, 16), "per_group", 16, "shift"),
            ("group128", (16, 128), "per_group", 128, "shift"), ("rows768", (3, 768), "per_token", None, "divide"),
            ("rows768_ragged_grid", (41, 768), "per_token", None, "divide"), ("tensor_one_vector", (1, one), "per_tensor", None, "tensor"),
            ("tensor_past_one_share", (1, past), "per_tensor", None, "tensor"), ("tensor_ragged", (1, several), "per_tensor", None, "tensor")]


GEOMETRY_NAMES = ["one_vector_groups", "group16", "group128", "rows768", "rows768_ragged_grid", "tensor_one_vector", "tensor_past_one_share",
                  "tensor_ragged"]


def within(got, want, bound, mask=None):
    """(ok, worst error / bound) of |got - want| <= bound, elementwise in float64, outside `mask`; the bound may be 0 where nothing
    may differ"""
    err = (got.double() - want.double()).abs()
    ok = err <= bound
    if mask is not None:
        ok = ok | mask
        err = torch.where(mask, torch.zeros_like(err), err)
    worst = (err / bound.clamp(min=1e-300)).max().item() if err.numel() else 0.0
    return bool(ok.all()), worst
