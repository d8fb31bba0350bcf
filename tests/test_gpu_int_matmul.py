"""ops.int_matmul_packed / ops.dynamic_int_pack (csrc/int_matmul.hip, csrc/dynamic_pack.hip; DESIGN.md §8 "Integer matmul"): the
int8-MFMA kernel against the float64 product under the one-rounding-per-operation bound, exact cases, the int32 range, the `row`
class against its chain bit for bit, the pack against ops.dynamic_fixed_qdq, and Linear's block_matmul route."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
MODES = ((None, False), (32, False), (32, True), (64, False), (64, True), (128, False), (128, True))   # (G, grouped activation scales)
SHAPES = (lambda G: (1, 1, 16), lambda G: (130, 257, 96), lambda G: (64, 132, 5 * G), lambda G: (129, 128, 3 * G))
# the (mode, shape) pairs that exist: K must be a multiple of G (the row class takes the G-shapes at G = 32)
CASES = [(G, ag, s(G or 32)) for G, ag in MODES for s in SHAPES if s(G or 32)[2] % (G or 16) == 0]
# dtype -> (half an ulp relative to |y|, half the smallest subnormal, the largest finite value)
OUT = {torch.float32: (2.0 ** -24, 2.0 ** -150, 3.4028234663852886e38), torch.bfloat16: (2.0 ** -8, 2.0 ** -134, 3.3895313892515355e38),
       torch.float16: (2.0 ** -11, 2.0 ** -25, 65504.0)}


def _operands(dev, M, N, K, G, ag, pa=8, pw=8, seed=0, pow2=False):
    g = torch.Generator().manual_seed(seed + M + 3 * N + 7 * K)
    codes = lambda r, p: torch.randint(-3 if pow2 else -(2 ** (p - 1) - 1), 4 if pow2 else 2 ** (p - 1), (r, K), generator=g, dtype=torch.int8)

    def scales(*shape):
        e = torch.randint(-2, 3, shape, generator=g).double() if pow2 else torch.rand(shape, generator=g, dtype=torch.float64) * 30 - 20
        return (2.0 ** e).float()

    sa = scales(M, K // G) if ag else scales(M)
    sw = scales(N, K // G) if G else scales(N)
    return [t.to(dev) for t in (codes(M, pa), sa, codes(N, pw), sw)]


def _ref64(ca, sa, cw, sw, G):
    """-> (y64, sum over groups of |t_g|) in float64 on the host"""
    ca, sa, cw, sw = (t.cpu().double() for t in (ca, sa, cw, sw))
    (M, K), N = ca.shape, cw.shape[0]
    G = G or K
    P = torch.einsum("mgk,ngk->mng", ca.view(M, K // G, G), cw.view(N, K // G, G))
    t = P * (sa[:, None, None] if sa.dim() == 1 else sa[:, None, :]) * (sw[None, :, None] if sw.dim() == 1 else sw[None, :, :])
    return t.sum(-1), t.abs().sum(-1)


def _within_bound(y, y64, T, n_groups, dtype):
    rel, sub, fmax = OUT[dtype]
    y = y.cpu().double()
    fits = y64.abs() <= fmax * (1 - 2 * rel)
    bound = (n_groups + 3) * 2.0 ** -24 * T + rel * y64.abs() + sub
    ok = ((y - y64).abs() <= bound) | (~fits & (y.abs() >= fmax) & (y.sign() == y64.sign()))   # (near or past fmax: also fmax or Inf)
    return bool(ok.all())


@pytest.mark.parametrize("pa,pw", ((8, 8), (8, 4), (4, 4)))
@pytest.mark.parametrize("G,ag,shape", CASES)
def test_kernel_against_float64(dmx, cuda, G, ag, shape, pa, pw):
    """|y - y64| <= (n_groups + 3) 2^-24 sum |t_g| + half an ulp of the output dtype: one rounding per convert, multiply and fma.  Also
    pins the MFMA result layout, the K tail of the row class (K = 16, 96) and both store forms (N = 132 against 1, 257, 128 + edges)."""
    ops = dmx.ops
    M, N, K = shape
    A = _operands(cuda, M, N, K, G, ag, pa, pw)
    assert ops.int_matmul_class(A[0], A[2], G if ag else 0, G or 0) == ("group" if G else "row")
    y64, T = _ref64(*A, G)
    for dtype in OUT:
        y = ops.int_matmul_packed(*A, G, out_dtype=dtype, fused=True)
        assert y.shape == (M, N) and y.dtype == dtype and _within_bound(y, y64, T, K // G if G else 1, dtype), dtype
        assert _within_bound(ops.int_matmul_packed(*A, G, out_dtype=dtype, fused=False), y64, T, K // G if G else 1, dtype), dtype   # the chain


@pytest.mark.parametrize("G,ag", MODES)
def test_exact_with_power_of_two_scales(dmx, cuda, G, ag):
    A = _operands(cuda, 130, 257, 384, G, ag, pow2=True)     # |t| <= 9 * 384 * 2^4, multiples of 2^-4: every fp32 step is exact
    y = dmx.ops.int_matmul_packed(*A, G, fused=True)
    assert torch.equal(y.cpu().double(), _ref64(*A, G)[0])


def test_row_class_full_int32_range(dmx, cuda):
    K = 131072
    ca = torch.full((16, K), 127, dtype=torch.int8, device=cuda)
    sign = torch.tensor([1, -1] * 8, dtype=torch.int8, device=cuda)
    cw = ca * sign[:, None]
    one = torch.ones(16, device=cuda)
    y = dmx.ops.int_matmul_packed(ca, one, cw, one, fused=True)
    assert torch.equal(y, (sign.float() * float(127 * 127 * K))[None, :].expand(16, 16))   # 16129 * 2^17: no int32 wrap


@pytest.mark.parametrize("out_dtype", tuple(OUT))
def test_row_kernel_equals_row_chain_and_routes(dmx, cuda, out_dtype):
    ops, routes = dmx.ops, dmx.ops._front._int_matmul_routes
    for M, N, K in ((130, 257, 96), (64, 132, 160)):
        A = _operands(cuda, M, N, K, None, False, 8, 4, seed=1)
        before = dict(routes)
        y = ops.int_matmul_packed(*A, out_dtype=out_dtype, fused=True)
        assert routes["fused"] == before["fused"] + 1 and routes["chain"] == before["chain"]
        assert torch.equal(y, ops.int_matmul_packed(*A, out_dtype=out_dtype, fused=False)) and routes["chain"] == before["chain"] + 1
    A = _operands(cuda, 4, 4, 24, None, False)               # K % 16 != 0: class 0
    with pytest.raises(NotImplementedError):
        ops.int_matmul_packed(*A, fused=True)
    before = routes["chain"]
    assert _within_bound(ops.int_matmul_packed(*A), *_ref64(*A, None), 1, torch.float32) and routes["chain"] == before + 1   # fused=None


@pytest.mark.parametrize("fmt", ("XP[8,0](CSN)", "XP[4,0](CSN)"))
@pytest.mark.parametrize("gran,G,L", (("per_token", None, 48), ("per_token", None, 768), ("per_token", None, 4096), ("per_token", None, 8208),
                                      ("per_group", 32, 256), ("per_group", 128, 256)))
def test_pack_is_the_dynamic_cast(dmx, cuda, fmt, gran, G, L):
    ops, routes = dmx.ops, dmx.ops._front._int_pack_routes
    x = torch.randn(37, L, generator=torch.Generator().manual_seed(L), dtype=torch.float32).to(cuda) * 3
    x[5] = 0.0                                               # an all-zero row: scale eps, codes 0
    want, want_sc, _ = ops.dynamic_fixed_qdq(x, fmt, gran, G, symmetric_qscheme=True, return_qparams=True)
    codes, sc = ops.dynamic_int_pack(x, fmt, gran, G, fused=True)
    S = G or L
    assert codes.dtype == torch.int8 and codes.shape == x.shape and torch.equal(sc.reshape(-1), want_sc)
    assert torch.equal((codes.float().view(-1, S) * sc.reshape(-1, 1)).view_as(x), want)
    assert not codes[5].any() and bool((sc.reshape(37, -1)[5] == torch.finfo(torch.float32).eps).all())
    for dt in (torch.bfloat16, torch.float16):
        xh = x.to(dt)
        ch, sh = ops.dynamic_int_pack(xh, fmt, gran, G, fused=True)
        cf, sf = ops.dynamic_int_pack(xh.float(), fmt, gran, G, fused=True)
        assert torch.equal(ch, cf) and torch.equal(sh, sf)
        assert torch.equal(sh.reshape(-1), ops.dynamic_fixed_qdq(xh, fmt, gran, G, symmetric_qscheme=True, return_qparams=True)[1])
    off = torch.empty(x.numel() + 1, device=cuda)[1:].view_as(x).copy_(x)   # a base one element off 16-byte alignment: the chain
    before = routes["chain"]
    co, so = ops.dynamic_int_pack(off, fmt, gran, G)
    assert routes["chain"] == before + 1 and torch.equal(co, codes) and torch.equal(so, sc)
    with pytest.raises(NotImplementedError):
        ops.dynamic_int_pack(off, fmt, gran, G, fused=True)


def test_linear_block_matmul_integer_route(dmx, cuda):
    nn, ops, fmt = dmx.nn, dmx.ops, "XP[8,0](CSN)"
    torch.manual_seed(0)
    base = nn.Linear(320, 72).to(cuda, torch.bfloat16)
    base.configure(dict(input_formats=[fmt], weight_format=fmt, input_dynamic="per_token", weight_dynamic={"per_group": 64},
                        output_formats=["FP[1|5|10,15](FN)"]))
    x = torch.randn(2, 9, 320, generator=torch.Generator().manual_seed(5)).to(cuda, torch.bfloat16)

    def module(symmetric, on):
        m = copy.deepcopy(base)
        for c in (m.input_casts.input_cast, m.weight_cast):
            c.qscheme = torch.per_tensor_symmetric if symmetric else torch.per_tensor_affine
        m.set_block_matmul(on)
        return m

    routes = ops._front._int_matmul_routes
    with torch.no_grad():
        m = module(True, True)
        keys, before = set(m.state_dict()), routes["fused"]
        y = m(x)
        assert routes["fused"] == before + 1 and set(m.state_dict()) == keys == set(base.state_dict())
        prod = ops.int_matmul(x, m.weight, fmt, fmt, "per_token", "per_group", 64)
        assert torch.equal(y, m.output_casts.output_cast(m.accum_cast(prod) + m.bias)) and y.dtype == torch.bfloat16
        assert not torch.equal(y, module(True, False)(x))            # the opt-in changes the product by design
        before = dict(routes)
        assert torch.equal(module(False, True)(x), module(False, False)(x)) and routes == before   # an affine qscheme: today's forward
    xg = x.clone().requires_grad_(True)                              # a gradient required: today's forward
    yg = module(True, True)(xg)
    assert yg.requires_grad and torch.equal(yg, module(True, False)(x)) and routes == before
