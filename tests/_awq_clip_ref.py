"""The CPU checker of AWQ weight clipping (ops.awq_clip; DESIGN.md §8 "AWQ clipping"): the definition itself in float32 torch on the CPU,
no product import.  The per-group dynamic integer cast is tests/_dynamic_ref.torch_restatement (the reference's two formulas in plain
torch, held to the oracle by tests/test_dynamic_quant_host.py); every other operation runs on two float32 tensors as its own call (no
contraction into an FMA), the inner sum over l runs in index order from the first product and the sum over j is the adjacent-pair
tree taken by slicing.  The cast's restatement is for finite inputs, so groups that are not ordinary are fed zeros and masked."""
import itertools

import torch

from _dynamic_ref import qrange, torch_restatement   # noqa: F401  (qrange: for the tests)

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32


def clip_ratios(n_grid=20, max_shrink=0.5):
    """1 - i / n_grid for i < int(max_shrink * n_grid): double arithmetic, one rounding to float32"""
    return torch.tensor([1.0 - i / n_grid for i in range(int(max_shrink * n_grid))], dtype=torch.float64).to(F32)


def tree_sum(v):
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def group_loss(d, blocks):
    """d float32 [rows, G, g], blocks float32 [G, g, g] -> float32 [rows, G]: tsum_j(d_j * sum_l blocks[k][j][l] * d_l)"""
    g = d.shape[-1]
    t = blocks[None, :, :, 0] * d[:, :, 0:1]
    for l in range(1, g):
        t = t + blocks[None, :, :, l] * d[:, :, l:l + 1]
    return tree_sum(d * t)


def clip_ref(w, blocks, ratios, precision, fmt_symmetric, g, qscheme_symmetric):
    """-> (y in w's dtype, best uint8 [rows, G], clip float32 [rows, G], losses float32 [rows, G, n], q: the cast of y, float32)"""
    w, blocks, ratios = w.detach().cpu(), blocks.detach().cpu().float(), ratios.detach().cpu().float()
    rows, L = w.shape
    G, n, T = L // g, ratios.numel(), w.dtype
    W = w.float().reshape(rows, G, g)
    a = W.abs().amax(dim=-1, keepdim=True)
    a = torch.where(torch.isnan(W).any(dim=-1, keepdim=True), torch.full_like(a, float("nan")), a)
    ordinary = torch.isfinite(a) & (a > 0)
    Wz, az = torch.where(ordinary, W, torch.zeros_like(W)), torch.where(ordinary, a, torch.ones_like(a))
    y, clip = w.reshape(rows, G, g).clone(), a.clone()
    best = torch.zeros(rows, G, 1, dtype=torch.uint8)
    best_loss = torch.full_like(a, float("inf"))
    q_best = torch.zeros_like(W)
    losses = torch.empty(rows, G, n)
    for i in range(n):
        c = (az * ratios[i]).to(T).float()
        v = torch.where(Wz > c, c, torch.where(Wz < -c, -c, Wz)).to(T)
        q = torch_restatement(v.reshape(-1, g), precision, fmt_symmetric, g, qscheme_symmetric)[0].float().reshape(rows, G, g)
        loss = group_loss(q - Wz, blocks)[..., None]
        loss = torch.where(ordinary, loss, torch.full_like(loss, float("nan")))
        losses[:, :, i:i + 1] = loss
        better = torch.isfinite(loss) & (loss < best_loss)
        best_loss = torch.where(better, loss, best_loss)
        y, clip, q_best = torch.where(better, v, y), torch.where(better, c, clip), torch.where(better, q, q_best)
        best = torch.where(better, torch.full_like(best, i), best)
    return y.reshape(rows, L), best.reshape(rows, G), clip.reshape(rows, G), losses, q_best.reshape(rows, L)


# ------------------------------------------------------------------------------------------------ data
def moment_blocks(x, g):
    """the float32 [G, g, g] diagonal blocks of the mean of x^T x over the tokens (x float32 [tokens, L])"""
    t, L = x.shape
    xg = x.reshape(t, L // g, g).transpose(0, 1)
    return (xg.transpose(1, 2) @ xg / t).contiguous()


def dataset(rows, L, g, seed, dtype, tokens=64):
    """Gaussian weights scaled by 0.05 and inputs randn * (1 + 3 rand) per channel -> (w in dtype, blocks float32 [L / g, g, g])"""
    gen = torch.Generator().manual_seed(7000 + seed)
    w = (0.05 * torch.randn(rows, L, generator=gen)).to(dtype)
    x = torch.randn(tokens, L, generator=gen) * (1.0 + 3.0 * torch.rand(L, generator=gen))
    return w, moment_blocks(x, g)


# ------------------------------------------------------------------------------------------------ the parity cases
# A case is (g, precision, symmetric, dtype); it runs on every shape of SHAPES(g).  Every (g, precision, symmetric) occurs, with the
# dtype going round, and every (g, dtype) -- each instantiation of the kernel -- occurs at XP[4,0] affine.
GROUPS, PRECISIONS, DTYPES = (16, 32, 64, 128), (2, 3, 4, 8), (BF16, F16, F32)


def shapes(g):
    return [(rows, L) for rows in (1, 3, 9) for L in (g, 3 * g)]


def _cases():
    out = []
    for (gi, g), (pi, p), (si, sym) in itertools.product(enumerate(GROUPS), enumerate(PRECISIONS), enumerate((False, True))):
        out.append((g, p, sym, DTYPES[(gi + pi + si) % 3]))
    for g, dt in itertools.product(GROUPS, DTYPES):
        if (g, 4, False, dt) not in out:
            out.append((g, 4, False, dt))
    return out


CASES = _cases()


def case_id(c):
    g, p, sym, dt = c
    return f"g{g}-p{p}-{'sym' if sym else 'affine'}-{str(dt).split('.')[-1]}"


_case_cache = {}


def case_data(c):
    """[(w, blocks, the checker's outputs)] over the case's shapes: computed once per process, never modified"""
    if c not in _case_cache:
        g, p, sym, dt = c
        ratios = clip_ratios()
        out = []
        for k, (rows, L) in enumerate(shapes(g)):
            w, blocks = dataset(rows, L, g, 100 * GROUPS.index(g) + 10 * p + k, dt)
            out.append((w, blocks, clip_ref(w, blocks, ratios, p, True, g, sym)))
        _case_cache[c] = out
    return _case_cache[c]


# ------------------------------------------------------------------------------------------------ planted groups
def special_groups(g):
    """name -> a float32 group that is not ordinary, or a constant one"""
    base = torch.linspace(-1.0, 2.0, g)
    nan = base.clone(); nan[g // 3] = float("nan")
    pinf = base.clone(); pinf[1] = float("inf")
    ninf = base.clone(); ninf[g - 2] = float("-inf")
    return {"zero": torch.zeros(g), "nan": nan, "pinf": pinf, "ninf": ninf, "constant": torch.full((g,), 0.75)}


def plant(w, g):
    """w with the special groups written over groups at the first, middle and last positions of the flat group list -> (w, {name: [i]})"""
    w = w.clone()
    flat = w.reshape(-1, g)
    n, sp = flat.shape[0], special_groups(g)
    assert n >= 3 * len(sp)
    spots = {name: [] for name in sp}
    for start in (0, n // 2 - len(sp) // 2, n - len(sp)):
        for j, (name, v) in enumerate(sp.items()):
            flat[start + j] = v.to(w.dtype)
            spots[name].append(start + j)
    return w, spots


def same(a, b):
    """bit for bit, a NaN matching any NaN"""
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.is_floating_point():
        return bool(torch.equal(a, b))
    na, nb = torch.isnan(a), torch.isnan(b)
    it = {4: torch.int32, 2: torch.int16}[a.element_size()]
    z = torch.zeros_like(a)
    return bool(torch.equal(na, nb)) and bool(torch.equal(torch.where(na, z, a).view(it), torch.where(nb, z, b).view(it)))
