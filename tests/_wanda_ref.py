"""The definition of Wanda in CPU torch: the checker of tests/test_gpu_wanda.py and tests/test_wanda_host.py, never the
thing under test.

    sumsq[j]  = sum_t (double)X[t, j]^2, added over the batches           sumsq_ref
    act_norm  = sumsq.sqrt().to(float32)                                  act_norm_ref
    score     = W.float().abs() * act_norm                                score_ref
    mask      = the N:M rule on that score, y = W * mask                  nm_ref, wanda_ref
"""
import torch


def exact_values(shape, dtype, seed):
    """values with 2^-4 <= |x| < 2^4 that `dtype` holds exactly: random mantissas of the dtype's width (8 significant bits for bfloat16 and
    for float32 tensors, which then hold bf16-representable values; 11 for float16) times 2^e, e in -4 .. 3, random signs.  Their
    squares are multiples of 2^-22 (bf16) or 2^-28 (f16) below 2^8, so a float64 sum of up to 2^12 of them is exact in ANY order."""
    g = torch.Generator().manual_seed(seed)
    bits = 11 if dtype == torch.float16 else 8
    n = 1
    for s in shape:
        n *= s
    man = torch.randint(1 << (bits - 1), 1 << bits, (n,), generator=g).double() / float(1 << (bits - 1))   # [1, 2)
    e = torch.randint(-4, 4, (n,), generator=g).double()
    sign = torch.randint(0, 2, (n,), generator=g).double() * 2.0 - 1.0
    v = (sign * man * torch.exp2(e)).reshape(shape)
    t = v.to(dtype)
    assert torch.equal(t.double(), v)
    return t


def sumsq_ref(batches):
    """float64 [C]: x.double().pow(2).sum(0) over the flattened tokens of every batch, the batches added in order"""
    total = None
    for x in batches:
        s = x.detach().cpu().reshape(-1, x.shape[-1]).double().pow(2).sum(0)
        total = s if total is None else total + s
    return total


def act_norm_ref(sumsq):
    return sumsq.sqrt().to(torch.float32)


def score_ref(w, act_norm):
    return w.detach().cpu().float().abs() * act_norm.detach().cpu()


def nm_ref(score, K, M, oracle=None):
    """the 0 / 1 float32 mask of the N:M rule along the last dim: the K highest of every group of M kept; stable ascending rank, the
    lower index zeroed first among ties, NaN highest, -0 == +0.  The oracle's mask where one is given, else a stable argsort (which
    orders 0.0 / -0.0 / NaN as the rule wants)."""
    if oracle is not None:
        return oracle.nm_mask(score, K, M, -1)
    g = score.reshape(-1, M)
    order = torch.argsort(g, dim=1, stable=True)
    mask = torch.ones_like(g)
    mask.scatter_(1, order[:, :M - K], 0.0)
    return mask.reshape(score.shape)


def wanda_ref(w, act_norm, K, M, oracle=None):
    """-> (score, mask, y): y = W * mask in torch's promotion of (W.dtype, float32)"""
    score = score_ref(w, act_norm)
    mask = nm_ref(score, K, M, oracle)
    return score, mask, w.detach().cpu() * mask
