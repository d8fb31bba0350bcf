"""CPU restatements of GPTQ with the oracle's casts (oracle/oracle.py) -- checkers, never the thing under test:
  * block_fp32: the in-block column loop (dmxq_gptq_block, csrc/gptq.hip) in float32 and in the kernel's order;
  * apply_ref:  the whole apply() (layer_reconstruction.py:266-327: dead columns, damping, Cholesky chain, blocks, trailing updates) in
                float64 (the reference's loop, linear algebra in float64) or in float32 (kernel order inside the blocks);
  * CASES / hessian64: the reference fixture's cases (tools/gen_golden_gptq.py, tests/golden/gptq.npz) and their Hessian in float64."""
import math

import torch


def slice_cast(oracle, fmt, scale=None, zero_point=None, per_row=False):
    """the module's weight cast of a [rows, m] float32 slice, by the oracle: BFP blocks along the columns, FloatingPoint per element,
    FixedPoint with the affine wrapper per row (per_row) or per tensor"""
    from dmx_compressor_amd.format import BlockFloatingPoint, FixedPoint, FloatingPoint

    if isinstance(fmt, BlockFloatingPoint):
        return lambda x: oracle.bfp_cast(x, fmt.precision, fmt.block_size, -1, fmt.symmetric)
    if isinstance(fmt, FloatingPoint):
        return lambda x: oracle.floating_point_cast(x, fmt.mantissa, fmt.exponent, fmt.bias, fmt.flush_subnormal, fmt.unsigned)
    from dmx_compressor_amd.format import ScaledBlockFloatingPoint
    if isinstance(fmt, ScaledBlockFloatingPoint):
        bf, sf = fmt.block_format, fmt.scaler_format
        return lambda x: oracle.sbfp_cast(x, bf.precision, fmt.block_size, sf.mantissa, sf.exponent, sf.bias, sf.flush_subnormal,
                                          bf.clamp, bf.symmetric, block_dim=-1)
    if isinstance(fmt, FixedPoint):
        return lambda x: oracle.fixed_point_affine_cast(x, fmt.precision, fmt.fraction, fmt.clamp, fmt.symmetric, scale, zero_point,
                                                        ch_axis=0 if per_row else None)
    raise TypeError(fmt)


def inv_diag(hinv, mb):
    """the host's inverses of the diagonal microblocks: [count] (mb 1) or [ceil(count / mb), mb, mb], a ragged last one padded with
    the identity"""
    count = hinv.shape[0]
    if mb == 1:
        return 1.0 / torch.diagonal(hinv).contiguous()
    nmb = -(-count // mb)
    blk = torch.eye(nmb * mb, dtype=hinv.dtype)
    blk[:count, :count] = hinv
    return torch.linalg.inv(torch.stack([blk[b * mb:(b + 1) * mb, b * mb:(b + 1) * mb] for b in range(nmb)])).contiguous()


def block_fp32(W, hinv, invd, mb, cast):
    """(Q, E) of one column block: float32, every product and difference rounded on its own, sums in index order from the first
    product (the order csrc/gptq.hip documents)"""
    w = W.detach().to(torch.float32).clone()
    hinv = hinv.to(torch.float32)
    rows, count = w.shape
    Q = torch.zeros_like(w)
    E = torch.zeros_like(w)
    for j1 in range(0, count, mb):
        m = min(mb, count - j1)
        q = cast(w[:, j1:j1 + m].contiguous())
        d = w[:, j1:j1 + m] - q
        D = invd[j1:j1 + 1].reshape(1, 1) if mb == 1 else invd[j1 // mb]
        err = d[:, 0:1] * D[0, :m]
        for i in range(1, m):
            err = err + d[:, i:i + 1] * D[i, :m]
        Q[:, j1:j1 + m] = q
        E[:, j1:j1 + m] = err
        if j1 + m < count:
            acc = err[:, 0:1] * hinv[j1, j1 + m:]
            for i in range(1, m):
                acc = acc + err[:, i:i + 1] * hinv[j1 + i, j1 + m:]
            w[:, j1 + m:] = w[:, j1 + m:] - acc
    return Q, E


def loss(W, Q, H):
    """tr((W - Q) H (W - Q)^T) in float64"""
    D = (W.double() - Q.double())
    return float(torch.einsum("ij,jk,ik->", D, H.double(), D))


# the reference fixture's cases: (module kind, in, out), weight format, microblock, block, calibration input shape, seed
CASES = {
    "a": dict(module=("linear", 256, 96), format="BFP[8|8]{64}(SN)", mb=64, block=128, input=(2, 8, 256), seed=100),
    "b": dict(module=("linear", 256, 96), format="MXINT4{64}", mb=64, block=128, input=(2, 8, 256), seed=100),
    "c": dict(module=("linear", 256, 96), format="FP[1|4|3,7](_N)", mb=1, block=128, input=(2, 8, 256), seed=100),
    "d": dict(module=("linear", 200, 96), format="XP[4,0](CSN)", mb=1, block=64, input=(2, 8, 200), seed=200, calib=True),
    "e": dict(module=("conv", 16, 32), format="BFP[8|8]{16}(SN)", mb=16, block=48, input=(2, 16, 10, 10), seed=300),
    "f": dict(module=("linear", 256, 96), format="SBFP<XP[4,0](CSN)><FP[0|4|4,7](FN)>{16}", mb=16, block=128, input=(2, 8, 256),
              seed=100),
}


def case_cast(oracle, case, scale=None, zero_point=None):
    from dmx_compressor_amd.format import Format
    return slice_cast(oracle, Format.from_shorthand(case["format"]), scale, zero_point, per_row=bool(case.get("calib")))


def hessian64(kind, xs, module):
    """measure_hessian (layer_reconstruction.py:240-264) over the batches, in float64: the batch is the sample count"""
    H, n = None, 0
    for inp in xs:
        if inp.dim() == 2:
            inp = inp.unsqueeze(0)
        tmp = inp.shape[0]
        if kind == "linear":
            inp = inp.reshape(-1, inp.shape[-1]).t()
        else:
            inp = torch.nn.functional.unfold(inp, module.kernel_size, dilation=module.dilation, padding=module.padding,
                                             stride=module.stride).permute([1, 0, 2]).flatten(1)
        inp = inp.double()
        if H is None:
            H = torch.zeros(inp.shape[0], inp.shape[0], dtype=torch.float64)
        H *= n / (n + tmp)
        n += tmp
        inp = math.sqrt(2 / n) * inp
        H = H + inp @ inp.t()
    return H


def apply_ref(W, H, mb, block, cast, dtype, percdamp=0.01):
    """Q of apply() on the CPU: float64 = the reference's loop with float64 linear algebra (casts of the float32-rounded slices);
    float32 = block_fp32 (kernel order) inside the blocks and float32 linear algebra around them"""
    W = W.detach().to(dtype).clone()
    H = H.detach().to(dtype).clone()
    ncols = W.shape[1]
    dead = torch.diag(H) == 0
    H[dead, dead] = 1
    W[:, dead] = 0
    idx = torch.arange(ncols)
    H[idx, idx] += percdamp * torch.mean(torch.diag(H))
    Hinv = torch.linalg.cholesky(torch.cholesky_inverse(torch.linalg.cholesky(H)), upper=True)
    Q = torch.zeros_like(W)
    for i1 in range(0, ncols, block):
        i2 = min(i1 + block, ncols)
        hb = Hinv[i1:i2, i1:i2]
        if dtype == torch.float32:
            Qb, Eb = block_fp32(W[:, i1:i2], hb, inv_diag(hb, mb), mb, cast)
        else:
            w = W[:, i1:i2].clone()
            Qb, Eb = torch.zeros_like(w), torch.zeros_like(w)
            for j1 in range(0, i2 - i1, mb):
                j2 = min(j1 + mb, i2 - i1)
                q = cast(w[:, j1:j2].float().contiguous()).to(dtype)
                err = (w[:, j1:j2] - q) @ torch.linalg.inv(hb[j1:j2, j1:j2])
                Qb[:, j1:j2], Eb[:, j1:j2] = q, err
                w[:, j2:] -= err @ hb[j1:j2, j2:]
        Q[:, i1:i2] = Qb
        W[:, i2:] -= Eb @ Hinv[i1:i2, i2:]
    return Q
