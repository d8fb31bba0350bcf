"""The full-row Hadamard rotation of include/dmxq.h (dmxq_hadamard_row_qdq; DESIGN.md §8 "Full-row Hadamard rotation") restated in
torch float32 on the CPU, and its composition with the dynamic integer cast (tests/_dynamic_ref.py torch_restatement).  Imports neither
the library nor the reference; the tables H_m are built here from Legendre symbols, independently of the library's.  rotate_loops()
spells the three steps of the definition -- butterflies ascending, the m-point stage left to right, one multiply; R^T: the m-point
stage first, with H_m^T -- as scalar loops on one row; rotate_ref() is the vectorised form the GPU tests use."""
import math

import numpy as np
import torch

from _dynamic_ref import torch_restatement


def matrix(m: int) -> np.ndarray:
    """H_m as int64 [m, m]: Paley I (q = m - 1) for 12 and 20, Paley II (q = 13) for 28"""
    if m == 1:
        return np.ones((1, 1), dtype=np.int64)
    q = m - 1 if m in (12, 20) else 13
    chi = [0] + [1 if any(r * r % q == a for r in range(1, q)) else -1 for a in range(1, q)]   # the Legendre symbol mod q
    Q = np.array([[chi[(j - i) % q] for j in range(q)] for i in range(q)], dtype=np.int64)
    S = np.zeros((q + 1, q + 1), dtype=np.int64)
    S[0, 1:] = 1
    S[1:, 0] = -1 if m in (12, 20) else 1
    S[1:, 1:] = Q
    if m in (12, 20):
        return np.eye(m, dtype=np.int64) + S
    return np.kron(S, np.array([[1, 1], [1, -1]])) + np.kron(np.eye(14, dtype=np.int64), np.array([[1, -1], [-1, -1]]))


def split(n: int):   # -> (m, k) with n = m 2^k
    odd = n
    while odd % 2 == 0:
        odd //= 2
    m = 1 if odd == 1 else 4 * odd
    assert odd in (1, 3, 5, 7) and n % m == 0, n
    return m, (n // m).bit_length() - 1


def rotate_ref(x: torch.Tensor, transpose: bool = False) -> torch.Tensor:
    """R (R^T) of the last dimension; float32 result of x's shape"""
    n = x.shape[-1]
    m, k = split(n)
    P = 1 << k
    H = matrix(m).T if transpose else matrix(m)
    v = x.detach().cpu().to(torch.float32).contiguous().reshape(-1, n)

    def mstage(v):
        cols = v.reshape(-1, m, P)
        out = torch.empty_like(cols)
        for a in range(m):
            sign = H[a]
            acc = cols[:, 0] if sign[0] > 0 else -cols[:, 0]
            for b in range(1, m):
                acc = acc + cols[:, b] if sign[b] > 0 else acc - cols[:, b]
            out[:, a] = acc
        return out.reshape(-1, n)

    if transpose and m > 1:
        v = mstage(v)
    s = 1
    while s < P:
        t = v.reshape(-1, P // (2 * s), 2, s)
        a, b = t[:, :, 0, :], t[:, :, 1, :]
        v = torch.stack((a + b, a - b), dim=2).reshape(-1, n)
        s *= 2
    if not transpose and m > 1:
        v = mstage(v)
    return (v * torch.tensor(np.float32(1.0 / math.sqrt(n)))).reshape(x.shape)


def rotate_loops(row: np.ndarray, transpose: bool = False) -> np.ndarray:
    """the definition on ONE float32 row as scalar loops (the independent form the vectorised one is held to)"""
    n = row.shape[0]
    m, k = split(n)
    P = 1 << k
    H = matrix(m).T if transpose else matrix(m)
    v = row.astype(np.float32).copy()

    def mstage(v):
        w = v.copy()
        for b in range(P):
            for a in range(m):
                acc = v[b] if H[a, 0] > 0 else np.float32(-v[b])
                for c in range(1, m):
                    acc = np.float32(acc + v[c * P + b]) if H[a, c] > 0 else np.float32(acc - v[c * P + b])
                w[a * P + b] = acc
        return w

    if transpose and m > 1:
        v = mstage(v)
    s = 1
    while s < P:
        old = v.copy()
        for i in range(n):
            if not (i % P) & s:
                v[i] = np.float32(old[i] + old[i + s])
                v[i + s] = np.float32(old[i] - old[i + s])
        s *= 2
    if not transpose and m > 1:
        v = mstage(v)
    return (v * np.float32(1.0 / math.sqrt(n))).astype(np.float32)


def dense(n: int) -> torch.Tensor:
    """kron(H_m, H_2^k) / sqrt(n) in float64: y = M @ x"""
    m, k = split(n)
    S = np.ones((1, 1), dtype=np.int64)
    for _ in range(k):
        S = np.kron(np.array([[1, 1], [1, -1]]), S)
    return torch.from_numpy(np.kron(matrix(m), S).astype(np.float64)) / math.sqrt(n)


def rotation_bound(x: torch.Tensor) -> torch.Tensor:
    """per row (k + m + 2) 2^-24 1.01 sum|x| / sqrt(n): the summation bound over a tree of depth k + m - 1 (k butterfly levels, m - 1
    further adds), plus the scale's two roundings (the constant, the product); 1.01 covers the O(u^2) terms.  float64 [rows, 1]"""
    n = x.shape[-1]
    m, k = split(n)
    return (k + m + 2) * 2.0 ** -24 * 1.01 * x.detach().cpu().double().abs().sum(dim=-1, keepdim=True) / math.sqrt(n)
