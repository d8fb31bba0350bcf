"""The CPU definition of AWQ (DESIGN.md §8 "AWQ"; Lin et al., 2023) that the tests hold the library to: the per-group dynamic integer
cast is tests/_dynamic_ref.dynamic_ref (the oracle's group_minmax -> qparams -> fixed_point_affine_cast), around it one float32 multiply
and rounding to the weight's dtype, one float32 division and one float32 subtraction; the losses are float64.  Finite inputs only."""
import torch

from _dynamic_ref import dynamic_ref

SCALE_MIN = 1e-4


def error_ref(O, w, s, precision, fmt_symmetric, group, qscheme_symmetric):
    """-> (d float32 = Q(w s) / s - w, wq in w's dtype); O: the oracle module; w [out, in] on the CPU, s float32 [in]"""
    w = w.detach().cpu()
    s = s.detach().cpu().float()
    x = w.float()
    ws = (x * s).to(w.dtype)
    wq = dynamic_ref(O, ws, precision, fmt_symmetric, group, qscheme_symmetric)[0]
    return wq.float() / s - x, wq


def rtn_error_ref(O, w, precision, fmt_symmetric, group, qscheme_symmetric):
    """the plain round-to-nearest error: the cast of w itself, minus w, in float32"""
    w = w.detach().cpu()
    return dynamic_ref(O, w, precision, fmt_symmetric, group, qscheme_symmetric)[0].float() - w.float()


def sumabs_ref(batches):
    """float64 [C]: the per-channel sum of |x| over every batch, every term exact in a double"""
    C = batches[0].shape[-1]
    acc = torch.zeros(C, dtype=torch.float64)
    for b in batches:
        acc += b.detach().cpu().double().abs().reshape(-1, C).sum(0)
    return acc


def x_mean_ref(batches):
    n = sum(b.numel() // b.shape[-1] for b in batches)
    return (sumabs_ref(batches) / n).to(torch.float32)


def gram64(batches):
    """float64 [C, C]: the mean of x^T x over the tokens"""
    C = batches[0].shape[-1]
    x = torch.cat([b.detach().cpu().double().reshape(-1, C) for b in batches])
    return x.t() @ x / x.shape[0]


def candidate_scales_f64(x_mean, n_grid):
    """the formula evaluated in float64 on the float32 x_mean: [n_grid, C]"""
    xm = x_mean.detach().cpu().double()
    rows = []
    for k in range(n_grid):
        s = xm.pow(k / n_grid).clamp(min=SCALE_MIN)
        rows.append(s / (s.max() * s.min()).sqrt())
    return torch.stack(rows)


def candidate_scales_ref(x_mean, n_grid):
    """the definition as written: float32 torch arithmetic (here on the CPU)"""
    xm = x_mean.detach().cpu().float()
    rows = []
    for k in range(n_grid):
        s = xm.pow(k / n_grid).clamp(min=SCALE_MIN)
        rows.append(s / (s.max() * s.min()).sqrt())
    return torch.stack(rows)


def loss64(d, gram):
    """sum((D G) * D) / out in float64, on a float32 or float64 D and gram"""
    d, gram = d.detach().cpu().double(), gram.detach().cpu().double()
    return float(((d @ gram) * d).sum() / d.shape[0])


def loss_bound(d, gram):
    """2 (in + 2) 2^-24 tr(|D| |G| |D|^T) / out: the inner-product bound of a float32 GEMM of depth `in` plus one product rounding, doubled"""
    d, gram = d.detach().cpu().double().abs(), gram.detach().cpu().double().abs()
    return float(2 * (d.shape[1] + 2) * 2.0 ** -24 * ((d @ gram) * d).sum() / d.shape[0])


def search_ref(O, w, batches, n_grid, precision, fmt_symmetric, group, qscheme_symmetric):
    """-> (losses float64 [n_grid], best, scales float32 [n_grid, in]) of the whole definition with a float64 second moment"""
    scales = candidate_scales_ref(x_mean_ref(batches), n_grid)
    G = gram64(batches)
    losses = torch.tensor([loss64(error_ref(O, w, s, precision, fmt_symmetric, group, qscheme_symmetric)[0], G) for s in scales],
                          dtype=torch.float64)
    finite = torch.isfinite(losses)
    best = int(torch.where(finite, losses, torch.full_like(losses, float("inf"))).argmin()) if bool(finite.any()) else 0
    return losses, best, scales


# ------------------------------------------------------------------------------------------------ the improvement data set
IN, OUT, TOKENS, GROUP = 256, 48, 96, 128
SEEDS = (0, 1, 2, 3, 4)


def dataset(seed, dtype):
    """Linear(256, 48): weight 0.05 randn, 96 tokens of randn with 8 random channels multiplied by 30 -> (w, bias, x) in `dtype`"""
    g = torch.Generator().manual_seed(1000 + seed)
    w = 0.05 * torch.randn(OUT, IN, generator=g)
    b = 0.05 * torch.randn(OUT, generator=g)
    x = torch.randn(TOKENS, IN, generator=g)
    ch = torch.randperm(IN, generator=g)[:8]
    x[:, ch] *= 30.0
    return w.to(dtype), b.to(dtype), x.to(dtype)


def output_error64(x, w, w_eff):
    """mean((x w_eff^T - x w^T)^2) in float64"""
    x, w, w_eff = x.detach().cpu().double(), w.detach().cpu().double(), w_eff.detach().cpu().double()
    return float(((x @ (w_eff - w).t()) ** 2).mean())
