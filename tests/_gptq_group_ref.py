"""CPU restatements of GPTQ with DYNAMIC per-group integer scales (dmxq_gptq_block_dynamic, csrc/gptq_dynamic.hip) --
checkers, never the thing under test, built from the oracle's group_minmax, qparams and fixed_point_affine_cast:
  * block_fp32_dynamic: tests/_gptq_ref.py block_fp32 (float32, the kernel's order) with the group step: at every column j with
                        j % g == 0 each row takes (scale, zp) = qparams(group_minmax(w[:, j:j + g])) of the block AS UPDATED so far and
                        casts the group's columns with it;
  * apply_ref_dynamic:  the whole apply() for a dynamic weight cast (per_group g, or g None with `whole` = "per_token" / "per_tensor":
                        the scale taken once from W), optional act_order, in float64 (the reference-shaped loop, float64 linear
                        algebra, casts of the float32-rounded slices) or float32 (block_fp32_dynamic inside the blocks)."""
import torch

from _gptq_ref import inv_diag


def group_qparams(O, seg, precision, fmt_symmetric, qscheme_symmetric):
    """(scale float32 [rows], zp int64 [rows]) of the rows of the [rows, g] float32 segment"""
    mn, mx = O.group_minmax(seg.contiguous(), 0, 1)
    return O.qparams(mn, mx, precision, fmt_symmetric, qscheme_symmetric)


def row_cast(O, x, precision, fmt_symmetric, sc, zp):
    """the [rows, m] slice cast with one (scale, zp) per row, as DMXQ_GPTQ_FIXED casts with a per-row scale"""
    return O.fixed_point_affine_cast(x.contiguous(), precision, 0, True, fmt_symmetric, sc, zp, ch_axis=0)


def block_fp32_dynamic(W, hinv, invd, mb, g, precision, fmt_symmetric, qscheme_symmetric, O):
    """(Q, E, scale [rows, count / g], zp [rows, count / g]) of one column block; g % mb == 0 and count % g == 0"""
    w = W.detach().to(torch.float32).clone()
    hinv = hinv.to(torch.float32)
    rows, count = w.shape
    assert count % g == 0 and g % mb == 0
    Q = torch.zeros_like(w)
    E = torch.zeros_like(w)
    scale = torch.zeros(rows, count // g, dtype=torch.float32)
    zp = torch.zeros(rows, count // g, dtype=torch.int64)
    sc = z = None
    for j1 in range(0, count, mb):
        if j1 % g == 0:
            sc, z = group_qparams(O, w[:, j1:j1 + g], precision, fmt_symmetric, qscheme_symmetric)
            scale[:, j1 // g], zp[:, j1 // g] = sc, z
        q = row_cast(O, w[:, j1:j1 + mb], precision, fmt_symmetric, sc, z)
        d = w[:, j1:j1 + mb] - q
        D = invd[j1:j1 + 1].reshape(1, 1) if mb == 1 else invd[j1 // mb]
        err = d[:, 0:1] * D[0, :mb]
        for i in range(1, mb):
            err = err + d[:, i:i + 1] * D[i, :mb]
        Q[:, j1:j1 + mb] = q
        E[:, j1:j1 + mb] = err
        if j1 + mb < count:
            acc = err[:, 0:1] * hinv[j1, j1 + mb:]
            for i in range(1, mb):
                acc = acc + err[:, i:i + 1] * hinv[j1 + i, j1 + mb:]
            w[:, j1 + mb:] = w[:, j1 + mb:] - acc
    return Q, E, scale, zp


def act_perm(H):
    """the processing order under act_order: stable argsort of diag(H), descending"""
    return torch.argsort(torch.diag(H), descending=True, stable=True)


def apply_ref_dynamic(W, H, mb, block, g, precision, fmt_symmetric, qscheme_symmetric, O, dtype, act_order=False, whole="per_token",
                      percdamp=0.01):
    """-> (Q [rows, ncols] in the ORIGINAL column order, scale [rows, G], zp [rows, G], perm or None); scale / zp in processing order"""
    W = W.detach().to(dtype).clone()
    H = H.detach().to(dtype).clone()
    rows, ncols = W.shape
    dead = torch.diag(H) == 0
    H[dead, dead] = 1
    W[:, dead] = 0
    perm = None
    if act_order:
        perm = act_perm(H)
        W = W[:, perm].contiguous()
        H = H[perm][:, perm].contiguous()
    idx = torch.arange(ncols)
    H[idx, idx] += percdamp * torch.mean(torch.diag(H))
    Hinv = torch.linalg.cholesky(torch.cholesky_inverse(torch.linalg.cholesky(H)), upper=True)
    Q = torch.zeros_like(W)
    if g is None:
        seg = W.float() if whole == "per_token" else W.float().reshape(1, -1)
        sc0, z0 = group_qparams(O, seg, precision, fmt_symmetric, qscheme_symmetric)
        sc0, z0 = sc0.reshape(-1, 1).expand(rows, 1).contiguous(), z0.reshape(-1, 1).expand(rows, 1).contiguous()
        scale, zp = sc0.clone(), z0.clone()
    else:
        assert ncols % g == 0 and block % g == 0
        scale = torch.zeros(rows, ncols // g, dtype=torch.float32)
        zp = torch.zeros(rows, ncols // g, dtype=torch.int64)
    for i1 in range(0, ncols, block):
        i2 = min(i1 + block, ncols)
        hb = Hinv[i1:i2, i1:i2]
        if dtype == torch.float32 and g is not None and g % mb == 0:
            Qb, Eb, sb, zb = block_fp32_dynamic(W[:, i1:i2], hb, inv_diag(hb, mb), mb, g, precision, fmt_symmetric, qscheme_symmetric, O)
            scale[:, i1 // g:i2 // g], zp[:, i1 // g:i2 // g] = sb, zb
        else:
            w = W[:, i1:i2].clone()
            Qb, Eb = torch.zeros_like(w), torch.zeros_like(w)
            for j1 in range(0, i2 - i1, mb):
                j2 = min(j1 + mb, i2 - i1)
                if g is None:
                    q = row_cast(O, w[:, j1:j2].float(), precision, fmt_symmetric, scale[:, 0], zp[:, 0])
                else:
                    for s in range(-(-j1 // g) * g, j2, g):   # the groups that start inside this microblock
                        k = (i1 + s) // g
                        scale[:, k], zp[:, k] = group_qparams(O, w[:, s:s + g].float(), precision, fmt_symmetric, qscheme_symmetric)
                    q = torch.empty(rows, j2 - j1, dtype=torch.float32)
                    for s in range(j1 // g * g, j2, g):
                        a, b, k = max(s, j1), min(s + g, j2), (i1 + s) // g
                        q[:, a - j1:b - j1] = row_cast(O, w[:, a:b].float(), precision, fmt_symmetric, scale[:, k].contiguous(),
                                                       zp[:, k].contiguous())
                q = q.to(dtype)
                err = (w[:, j1:j2] - q) @ torch.linalg.inv(hb[j1:j2, j1:j2])
                Qb[:, j1:j2], Eb[:, j1:j2] = q, err
                w[:, j2:] -= err @ hb[j1:j2, j2:]
        Q[:, i1:i2] = Qb
        W[:, i2:] -= Eb @ Hinv[i1:i2, i2:]
    if perm is not None:
        Qp, Q = Q, torch.empty_like(Q)
        Q[:, perm] = Qp
    return Q, scale, zp, perm
