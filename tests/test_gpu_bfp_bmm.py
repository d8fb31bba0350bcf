"""ops.bfp_bmm / bfp_bmm_packed (csrc/bfp_bmm.hip, DESIGN.md §8 "Batched BFP matmul") and ops.bfp_pack(block_dim=-2): the batched
int8-MFMA kernel in both W layouts against the float64 product of the unpacked operands under the textbook bound of nb - 1 ordered fp32
additions of exact terms, against the chain bit for bit (special blocks included), the column-blocked pack against its transposing
definition, and the opt-in switch of ActActMatMul / ScaledDotProductAttention."""
import copy

import pytest
import torch

from _bfp_mm_ref import ref_and_bound_bmm as _ref_and_bound
from _data import make, mismatches_nan_aware

pytestmark = pytest.mark.gpu
BLOCKS = (32, 64, 128)
LAYOUTS = ("nk", "kn")
SHAPES = (lambda B: (3, 17, 36, 3 * B), lambda B: (2, 130, 260, 5 * B), lambda B: (3, 33, 64, 2 * B))   # (batch, M, N, K)


def _operands(dev, layout, batch, M, N, K, kind="heavy"):
    x = make(kind, (batch, M, K), seed=M + K).to(dev)
    w = make("normal", (batch, K, N) if layout == "kn" else (batch, N, K), seed=N + K + 1).to(dev)
    return x, w


def _pack(ops, x, w, layout, pa, pw, B, sym_a=True):
    return ops.bfp_pack(x, pa, B, sym_a), ops.bfp_pack(w, pw, B, True, block_dim=-2 if layout == "kn" else -1)


@pytest.mark.parametrize("shape", range(len(SHAPES)))
@pytest.mark.parametrize("pa,pw", ((8, 8), (8, 4)))
@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_kernel_against_float64(dmx, cuda, layout, B, pa, pw, shape):
    """pins the lane-to-(m, n) layout of both tile widths and the byte transpose of the "kn" staging"""
    ops = dmx.ops
    batch, M, N, K = SHAPES[shape](B)
    A, W = _pack(ops, *_operands(cuda, layout, batch, M, N, K), layout, pa, pw, B)
    assert ops.bfp_bmm_class(A[0], W[0], B, layout) == f"{layout}_b{B}_n{64 if N <= 64 else 128}"
    y = ops.bfp_bmm_packed(*A, *W, pa, pw, B, layout, fused=True)
    ref, bound = _ref_and_bound(ops, A, W, layout, pa, pw, B)
    err = (y.cpu().double() - ref).abs()
    print(f"{layout} B={B} p=({pa},{pw}) {batch}x{M}x{N}x{K}: max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert y.shape == (batch, M, N) and y.dtype == torch.float32 and bool((err <= bound).all())


@pytest.mark.parametrize("out_dtype", (torch.bfloat16, torch.float16, torch.float32))
@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_kernel_against_chain_bit_for_bit_with_special_blocks(dmx, cuda, layout, B, out_dtype):
    ops = dmx.ops
    batch, M, N, K = 2, 130, 132, 3 * B
    x, w = _operands(cuda, layout, batch, M, N, K)
    x[0, 3, :B] = 0.0                        # exponent byte 0 in A
    x[1, 7, 2 * B + 1] = float("inf")        # 255 in A: row 7 of batch 1 is NaN
    if layout == "kn":
        w[0, B:2 * B, 5] = 0.0               # byte 0 in W (block 1 of column 5)
        w[1, 3, 11] = float("nan")           # 255 in W: column 11 of batch 1 is NaN
    else:
        w[0, 5, B:2 * B] = 0.0
        w[1, 11, 3] = float("nan")
    A, W = _pack(ops, x, w, layout, 8, 4, B, sym_a=False)
    assert int(A[1][0, 3, 0]) == 0 and int(A[1][1, 7, 2]) == 255
    assert (int(W[1][0, 1, 5]), int(W[1][1, 0, 11])) == (0, 255) if layout == "kn" else (int(W[1][0, 5, 1]), int(W[1][1, 11, 0])) == (0, 255)
    y = ops.bfp_bmm_packed(*A, *W, 8, 4, B, layout, out_dtype=out_dtype, fused=True)
    assert y.dtype == out_dtype and mismatches_nan_aware(y, ops.bfp_bmm_packed(*A, *W, 8, 4, B, layout, out_dtype=out_dtype, fused=False)) == 0
    nan = torch.zeros(batch, M, N, dtype=torch.bool, device=cuda)
    nan[1, 7, :] = True
    nan[1, :, 11] = True
    assert torch.equal(torch.isnan(y), nan)
    if layout == "nk":
        for b in range(batch):
            two_d = ops.bfp_matmul_packed(A[0][b], A[1][b], W[0][b], W[1][b], 8, 4, B, out_dtype=out_dtype, fused=True)
            assert mismatches_nan_aware(y[b], two_d) == 0


@pytest.mark.parametrize("case", ("n_mod_4", "ragged_k", "unaligned"))
def test_refused_kn_inputs_run_the_chain(dmx, cuda, case):
    ops, B = dmx.ops, 64
    batch, M, N, K = 2, 9, (38 if case == "n_mod_4" else 40), (100 if case == "ragged_k" else 128)
    x, w = _operands(cuda, "kn", batch, M, N, K, kind="normal")
    A, W = _pack(ops, x, w, "kn", 8, 8, B)
    if case == "unaligned":   # contiguous codes at an odd byte offset
        W = (torch.empty(batch * K * N + 1, dtype=torch.int8, device=cuda)[1:].view(batch, K, N).copy_(W[0]), W[1])
    assert ops.bfp_bmm_class(A[0], W[0], B, "kn") is None
    with pytest.raises(NotImplementedError):
        ops.bfp_bmm_packed(*A, *W, 8, 8, B, "kn", fused=True)
    before = dict(dmx._front._bfp_bmm_routes)
    got = ops.bfp_bmm_packed(*A, *W, 8, 8, B, "kn")
    assert dmx._front._bfp_bmm_routes["chain"] == before["chain"] + 1
    ref, bound = _ref_and_bound(ops, A, W, "kn", 8, 8, B)
    assert bool(((got.cpu().double() - ref).abs() <= bound).all())


@pytest.mark.parametrize("symmetric", (True, False))
@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float32))
@pytest.mark.parametrize("B", BLOCKS)
def test_pack_block_dim_minus_2(dmx, cuda, B, dtype, symmetric):
    ops, routes = dmx.ops, dmx._front._bfp_pack_cols_routes
    for shape in ((3, 2 * B, 40), (130, 264)):   # whole blocks: the column kernel; 130 rows end in a ragged block: the transposing route
        x = make("heavy", shape, seed=B, dtype=dtype).to(cuda)
        x[..., :B, 3] = 0.0                   # an all-zero block
        x[..., 0, :] = 0.0                    # an all-zero row
        x[..., B + 1, 9] = float("nan")
        before = dict(routes)
        c, e = ops.bfp_pack(x, 8, B, symmetric, block_dim=-2)
        kernel = shape[-2] % B == 0
        assert (routes["fused"], routes["chain"]) == (before["fused"] + kernel, before["chain"] + (not kernel))
        wc, we = ops.bfp_pack(x.transpose(-1, -2).contiguous(), 8, B, symmetric)
        assert c.shape == x.shape and e.shape == shape[:-2] + (-(-shape[-2] // B), shape[-1]) and c.is_contiguous() and e.is_contiguous()
        assert torch.equal(c, wc.transpose(-1, -2)) and torch.equal(e, we.transpose(-1, -2))
        assert int(e[..., 0, 3].max()) == 0 and int(e[..., 1, 9].min()) == 255
    with pytest.raises(NotImplementedError):
        ops.bfp_pack(x, 8, B, symmetric, block_dim=-2, fused=True)


def test_attention_block_matmul_switch(dmx, cuda):
    nn, ops, f = dmx.nn, dmx.ops, "BFP[8|8]{32}(SN)"
    q, k, v = (make("normal", (2, 3, 33, 64), seed=s, dtype=torch.bfloat16).to(cuda) for s in (1, 2, 3))
    p = torch.softmax(make("normal", (2, 3, 33, 33), seed=4).to(cuda), -1).to(torch.bfloat16)
    kt = k.transpose(-2, -1)
    routes = dmx._front._bfp_bmm_routes
    bmm = lambda a, w, layout: ops.bfp_bmm_packed(*ops.bfp_pack(a, 8, 32), *ops.bfp_pack(w, 8, 32, block_dim=-2 if layout == "kn" else -1),
                                                  8, 8, 32, layout, out_dtype=torch.bfloat16)
    base = nn.ActActMatMul().to(cuda)
    base.configure(dict(input_formats=[f, f]))
    with torch.no_grad():
        on = copy.deepcopy(base)
        keys = set(on.state_dict())
        assert on.block_matmul is False and torch.equal(on(q, kt), copy.deepcopy(base)(q, kt))        # off: today's forward
        on.configure(dict(block_matmul=True))
        assert on.block_matmul is True and set(on.state_dict()) == keys
        before = dict(routes)
        y_qk, y_pv, y_pv32 = on(q, kt), on(p, v), on(p[..., :32].contiguous(), v[..., :32, :].contiguous())
        # Q K^T ("nk", K = 64) and P V over 32 keys ("kn") ran the kernel; P V over 33 keys has a ragged block: the chain
        assert (routes["fused"], routes["chain"]) == (before["fused"] + 2, before["chain"] + 1)
        assert mismatches_nan_aware(y_qk, bmm(q, k, "nk")) == 0 and mismatches_nan_aware(y_pv, bmm(p, v, "kn")) == 0
        assert mismatches_nan_aware(y_pv32, bmm(p[..., :32].contiguous(), v[..., :32, :].contiguous(), "kn")) == 0
        assert y_qk.shape == (2, 3, 33, 33) and y_pv.shape == (2, 3, 33, 64) and y_qk.dtype == torch.bfloat16
        mixed, mixed_on = copy.deepcopy(base), copy.deepcopy(base)                                   # two block sizes: today's forward
        for m in (mixed, mixed_on):
            m.configure(dict(input_formats=[f, "BFP[8|8]{64}(SN)"]))
        mixed_on.set_block_matmul(True)
        assert torch.equal(mixed_on(q, kt), mixed(q, kt))
        # the compound module needs only its actmatmul switched
        sdpa = nn.ScaledDotProductAttention().to(cuda)
        sdpa.actmatmul.configure(dict(input_formats=[f, f]))
        off = copy.deepcopy(sdpa)
        sdpa.actmatmul.set_block_matmul(True)
        before = dict(routes)
        out = sdpa(q, k, v)
        assert routes["fused"] + routes["chain"] == before["fused"] + before["chain"] + 2 and routes["fused"] > before["fused"]
        assert out.shape == (2, 3, 33, 64) and torch.equal(off(q, k, v), copy.deepcopy(off)(q, k, v))
