"""ops.bfp_matmul / bfp_matmul_packed (csrc/bfp_matmul.hip, DESIGN.md §8 "BFP matmul"): the int8-MFMA kernel against the float64
product of the unpacked operands under the textbook bound of nb - 1 ordered fp32 additions of exact terms, against the chain of torch
operations bit for bit (special blocks included), the front end's properties, and Linear's opt-in switch."""
import pytest
import torch

from _bfp_mm_ref import ref_and_bound_mm as _ref_and_bound
from _data import make, mismatches_nan_aware, ulp_of

pytestmark = pytest.mark.gpu
BLOCKS = (32, 64, 128)
PRECISIONS = ((8, 8), (8, 4), (4, 4))
SHAPES = (lambda B: (1, 16, B), lambda B: (17, 33, 3 * B), lambda B: (130, 257, 5 * B), lambda B: (256, 128, 16 * B))


def _packed(ops, dev, M, N, K, B, pa, pw, kind="heavy", sym_a=True):
    x, w = make(kind, (M, K), seed=M + K).to(dev), make("normal", (N, K), seed=N + K + 1).to(dev)
    return x, w, ops.bfp_pack(x, pa, B, sym_a), ops.bfp_pack(w, pw, B, True)


@pytest.mark.parametrize("shape", range(len(SHAPES)))
@pytest.mark.parametrize("pa,pw", PRECISIONS)
@pytest.mark.parametrize("B", BLOCKS)
def test_kernel_against_float64(dmx, cuda, B, pa, pw, shape):
    """also pins the MFMA result layout (which lane holds which (m, n)): a transposed or permuted tile misses the bound at once"""
    ops = dmx.ops
    M, N, K = SHAPES[shape](B)
    _, _, A, W = _packed(ops, cuda, M, N, K, B, pa, pw)
    assert ops.bfp_matmul_class(A[0], W[0], B) == f"mfma_b{B}"
    y = ops.bfp_matmul_packed(*A, *W, pa, pw, B, fused=True)
    ref, bound = _ref_and_bound(ops, A, W, pa, pw, B)
    err = (y.cpu().double() - ref).abs()
    print(f"B={B} p=({pa},{pw}) {M}x{N}x{K}: max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert y.shape == (M, N) and y.dtype == torch.float32 and bool((err <= bound).all())


@pytest.mark.parametrize("out_dtype", (torch.bfloat16, torch.float16))
@pytest.mark.parametrize("B", BLOCKS)
def test_kernel_sixteen_bit_outputs(dmx, cuda, B, out_dtype):
    ops = dmx.ops
    _, _, A, W = _packed(ops, cuda, 17, 33, 3 * B, B, 8, 8, kind="normal")     # (odd N: element stores) ...
    _, _, A2, W2 = _packed(ops, cuda, 130, 260, 5 * B, B, 8, 8, kind="normal")  # ... N % 4 == 0: 8-byte stores
    for a, w in ((A, W), (A2, W2)):
        y = ops.bfp_matmul_packed(*a, *w, 8, 8, B, out_dtype=out_dtype, fused=True)
        ref, bound = _ref_and_bound(ops, a, w, 8, 8, B, out_dtype)
        assert y.dtype == out_dtype and bool(((y.cpu().double() - ref).abs() <= bound).all())
        assert mismatches_nan_aware(y, ops.bfp_matmul_packed(*a, *w, 8, 8, B, out_dtype=out_dtype, fused=False)) == 0


@pytest.mark.parametrize("pa,pw", PRECISIONS)
@pytest.mark.parametrize("B", BLOCKS)
def test_kernel_against_chain_bit_for_bit_with_special_blocks(dmx, cuda, B, pa, pw):
    ops = dmx.ops
    M, N, K = 130, 257, 5 * B
    x, w = make("heavy", (M, K), seed=3).to(cuda), make("normal", (N, K), seed=4).to(cuda)
    x[3, :B] = 0.0                      # an all-zero block: exponent byte 0
    x[5, B:2 * B] = 1e-40               # a block whose maximum is a denormal: exponent byte 0 as well
    x[7, 2 * B + 1] = float("inf")      # exponent byte 255: row 7 of y is NaN
    w[11, 3 * B + 2] = float("nan")     # column 11 of y is NaN
    x[9, :B] = 0.25
    x[9, 0] = -1.999                    # rounds to -2^(p-1) quanta, a code only the asymmetric format has
    A, W = ops.bfp_pack(x, pa, B, False), ops.bfp_pack(w, pw, B, True)
    assert int(A[1][3, 0]) == 0 and int(A[1][5, 1]) == 0 and int(A[1][7, 2]) == 255 and int(W[1][11, 3]) == 255
    assert int(A[0][9, 0]) == -(1 << (pa - 1))
    y = ops.bfp_matmul_packed(*A, *W, pa, pw, B, fused=True)
    assert mismatches_nan_aware(y, ops.bfp_matmul_packed(*A, *W, pa, pw, B, fused=False)) == 0
    nan = torch.zeros(M, N, dtype=torch.bool, device=cuda)
    nan[7, :] = True
    nan[:, 11] = True
    assert torch.equal(torch.isnan(y), nan)
    # the zero blocks add +0: the same product without them (their codes and the partner's, block 0 of row 3 / block 1 of row 5)
    for r, j in ((3, 0), (5, 1)):
        keep = [k for k in range(K) if not j * B <= k < (j + 1) * B]
        ea = torch.cat([A[1][r:r + 1, :j], A[1][r:r + 1, j + 1:]], 1)
        ew = torch.cat([W[1][:, :j], W[1][:, j + 1:]], 1)
        rest = ops.bfp_matmul_packed(A[0][r:r + 1, keep].contiguous(), ea.contiguous(), W[0][:, keep].contiguous(), ew.contiguous(), pa, pw, B)
        assert mismatches_nan_aware(y[r:r + 1], rest) == 0


def test_front_end_properties(dmx, cuda):
    ops, f = dmx.ops, "BFP[8|8]{64}(SN)"
    x, w = make("heavy", (3, 20, 320), seed=1, dtype=torch.bfloat16).to(cuda), make("normal", (70, 320), seed=2, dtype=torch.bfloat16).to(cuda)
    y = ops.bfp_matmul(x, w, f)
    assert y.shape == (3, 20, 70) and y.dtype == torch.bfloat16
    assert mismatches_nan_aware(y, ops.bfp_matmul(ops.bfp_qdq(x, 8, 64), ops.bfp_qdq(w, 8, 64), f)) == 0     # pack of a cast tensor: the same codes
    assert mismatches_nan_aware(y, ops.bfp_matmul(x, w, f)) == 0                                             # reproducible
    assert mismatches_nan_aware(y, ops.bfp_matmul(x.reshape(60, 320), w, f).reshape(3, 20, 70)) == 0         # leading dimensions
    # what the kernel refuses runs the chain, within the same bound of the float64 reference
    x2, w2 = x.reshape(60, 320).float(), w.float()
    for B, K, view in ((16, 320, False), (64, 300, False), (64, 320, True)):
        xa, wa = x2[:, :K].contiguous(), w2[:, :K].contiguous()
        A, W = ops.bfp_pack(xa, 8, B), ops.bfp_pack(wa, 8, B)
        if view:   # contiguous codes at an odd byte offset
            A = (torch.empty(60 * K + 1, dtype=torch.int8, device=cuda)[1:].view(60, K).copy_(A[0]), A[1])
        assert ops.bfp_matmul_class(A[0], W[0], B) is None
        with pytest.raises(NotImplementedError):
            ops.bfp_matmul_packed(*A, *W, 8, 8, B, fused=True)
        got = ops.bfp_matmul_packed(*A, *W, 8, 8, B)
        ref, bound = _ref_and_bound(ops, A, W, 8, 8, B)
        assert bool(((got.cpu().double() - ref).abs() <= bound).all())
        assert mismatches_nan_aware(got, ops.bfp_matmul_packed(*A, *W, 8, 8, B, fused=False)) == 0


def test_linear_block_matmul_switch(dmx, cuda):
    import copy
    nn, ops = dmx.nn, dmx.ops
    torch.manual_seed(0)
    base = nn.Linear(320, 70).to(cuda)
    base.configure(dict(input_formats=["BFP[8|8]{64}(SN)"], weight_format="BFP[8|8]{64}(SN)"))
    x = make("normal", (2, 9, 320), seed=5).to(cuda)
    with torch.no_grad():
        want_off = copy.deepcopy(base)(x)
        m = copy.deepcopy(base)
        assert m.block_matmul is False and mismatches_nan_aware(m(x), want_off) == 0          # off: today's forward
        keys = set(m.state_dict())
        m.configure(dict(block_matmul=True))
        assert m.block_matmul is True and set(m.state_dict()) == keys
        y = m(x)
        want = m.accum_cast(ops.bfp_matmul(x, m.weight, "BFP[8|8]{64}(SN)", out_dtype=torch.float32)) + m.bias
        assert mismatches_nan_aware(y, want) == 0
        A, W = ops.bfp_pack(x.reshape(18, 320), 8, 64), ops.bfp_pack(m.weight, 8, 64)
        ref, bound = _ref_and_bound(ops, A, W, 8, 8, 64)
        err = ((y.reshape(18, 70) - m.bias).cpu().double() - ref).abs()
        assert bool((err <= bound + 0.5 * ulp_of(y.reshape(18, 70).cpu().double(), torch.float32)).all())   # (+ the rounding of the bias add)
        m.configure(dict(weight_format="FP[1|4|3,7](_N)"))                                       # a non-BFP weight format: today's forward
        other = copy.deepcopy(base)
        other.configure(dict(weight_format="FP[1|4|3,7](_N)"))
        assert mismatches_nan_aware(m(x), other(x)) == 0
    g = copy.deepcopy(base)
    g.set_block_matmul(True)
    xg = x.clone().requires_grad_(True)                                                          # a gradient required: today's forward
    yg = g(xg)
    assert yg.requires_grad and mismatches_nan_aware(yg, copy.deepcopy(base)(x)) == 0
