"""GPTQ with dynamic per-group integer scales and activation order on the GPU: the fused column kernel (csrc/gptq_dynamic.hip,
ops.gptq_block_dynamic) bit for bit against the CPU restatement in its own order (tests/_gptq_group_ref.py), and
`DmxModule.optimal_brain_compressing` end to end for dynamic weight casts (per_group / per_token / per_tensor) and `act_order`."""
import pytest
import torch
import torch.nn.functional as F

from _data import bits_equal, make
from _gptq_group_ref import apply_ref_dynamic, block_fp32_dynamic
from _gptq_ref import CASES, hessian64, inv_diag, loss

pytestmark = pytest.mark.gpu


def _hinv(count, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(4 * count, count, generator=g)
    H = 2.0 / X.shape[0] * (X.t() @ X)
    H += 0.01 * torch.mean(torch.diag(H)) * torch.eye(count)
    return torch.linalg.cholesky(torch.cholesky_inverse(torch.linalg.cholesky(H)), upper=True).contiguous()


def _qsym(dmx, m):
    from dmx_compressor_amd.observer import _SYMMETRIC
    return m.weight_cast.qscheme in _SYMMETRIC


# (format, microblock, group, rows, count, symmetric qscheme, special): microblock 1 .. 64 and == group, one to eight groups per block,
# row counts below / across / beyond the 64-row workgroup; "zeros": an all-zero first group in some rows and one all-zero row (scale =
# eps, the division route); "outlier": one large element in an otherwise small group
KERNEL_CASES = [
    ("XP[4,0](CSN)", 1, 128, 150, 128, True, None),
    ("XP[4,0](CSN)", 1, 32, 65, 64, True, None),
    ("XP[4,0](C_N)", 8, 16, 1, 48, False, None),
    ("XP[8,0](CSN)", 16, 64, 96, 128, True, None),
    ("XP[3,0](C_N)", 32, 32, 70, 96, False, None),
    ("XP[4,0](CSN)", 64, 64, 130, 128, True, None),
    ("XP[4,0](CSN)", 8, 32, 20, 96, True, "zeros"),
    ("XP[4,0](C_N)", 1, 16, 20, 64, False, "zeros"),
    ("XP[4,0](CSN)", 1, 64, 67, 128, False, "outlier"),
]


_CACHE = {}   # CPU references and GPU runs shared between tests: computed once, never modified


def _cached(key, make_value):
    if key not in _CACHE:
        _CACHE[key] = make_value()
    return _CACHE[key]


def _kernel_case(case, O):
    """the inputs and the CPU restatement's results, once for both bindings"""
    return _cached(("kernel", case), lambda: _make_kernel_case(case, O))


def _make_kernel_case(case, O):
    from dmx_compressor_amd.format import Format

    sh, mb, g, rows, count, qsym, special = case
    fmt = Format.from_shorthand(sh)
    gen = torch.Generator().manual_seed(rows * 1000 + count + g)
    W = torch.randn(rows, count, generator=gen) * 0.05
    if special == "zeros":
        W[2:6, :g] = 0.0
        W[0, :] = 0.0
    elif special == "outlier":
        W[3, g + 5] = 50.0
        W[rows - 1, 2] = -37.5
    hinv = _hinv(count, seed=count + mb)
    invd = inv_diag(hinv, mb)
    ref = block_fp32_dynamic(W, hinv, invd, mb, g, fmt.precision, bool(fmt.symmetric), qsym, O)
    return fmt, W, hinv, invd, ref


@pytest.mark.parametrize("binding", ["torch", "ctypes"])
@pytest.mark.parametrize("case", KERNEL_CASES, ids=[f"{c[0]}-mb{c[1]}-g{c[2]}-{c[3]}x{c[4]}-{'sym' if c[5] else 'affine'}{'-' + c[6] if c[6] else ''}"
                                                    for c in KERNEL_CASES])
def test_kernel_bits_vs_restatement(dmx, oracle, cuda, case, binding):
    from dmx_compressor_amd import _backend_ctypes as B
    from dmx_compressor_amd.observer import get_qmin_qmax

    sh, mb, g, rows, count, qsym, special = case
    fmt, W, hinv, invd, (Qr, Er, scr, zpr) = _kernel_case(case, oracle)
    if special == "zeros":
        assert (scr[0] == torch.finfo(torch.float32).eps).all() and (scr[2:6, 0] == torch.finfo(torch.float32).eps).all()
    ng = count // g
    # W as a column block of a wider matrix, Q with NaN around the target, the scales as a column block of wider tensors
    Wd = torch.zeros(rows, count + 40, device=cuda)
    Wd[:, 5:5 + count] = W.to(cuda)
    Qd = torch.full((rows, count + 40), float("nan"), device=cuda)
    Ed = torch.empty(rows, count, device=cuda)
    Sd = torch.full((rows, ng + 3), -1.0, device=cuda)
    Zd = torch.full((rows, ng + 3), 99, dtype=torch.int64, device=cuda)
    args = (Wd[:, 5:5 + count], hinv.to(cuda), invd.to(cuda))
    outs = (Qd[:, 5:5 + count], Ed, Sd[:, 1:1 + ng], Zd[:, 1:1 + ng])
    if binding == "torch":
        dmx.ops.gptq_block_dynamic(*args, *outs, mb, g, fmt, qsym)
    else:
        qmin, qmax = get_qmin_qmax(fmt)
        fields = [2, fmt.precision, 0, int(fmt.symmetric), 0, 0, 0, 0, 0, 0, 1, 1]
        B.gptq_block_dynamic(*args, mb, fields, dmx._lib.ROUND_NEAREST, g, qmin, qmax, qsym, *outs)
    torch.cuda.synchronize()
    assert bits_equal(Sd[:, 1:1 + ng], scr) == 0
    assert bits_equal(Zd[:, 1:1 + ng], zpr) == 0
    assert bits_equal(Qd[:, 5:5 + count], Qr) == 0
    assert bits_equal(Ed, Er) == 0
    assert torch.isnan(Qd[:, :5]).all() and torch.isnan(Qd[:, 5 + count:]).all()   # nothing outside the block written
    assert (Sd[:, 0] == -1).all() and (Sd[:, 1 + ng:] == -1).all() and (Zd[:, 0] == 99).all() and (Zd[:, 1 + ng:] == 99).all()


def test_kernel_refuses_what_it_does_not_cover(dmx, cuda):
    W = torch.randn(64, 96, device=cuda)
    hinv = torch.eye(96, device=cuda)
    q, e = torch.empty_like(W), torch.empty_like(W)
    fmt = dmx.Format.from_shorthand("XP[4,0](CSN)")

    def run(mb, g, f=fmt, invd=None):
        ng = 96 // g
        dmx.ops.gptq_block_dynamic(W, hinv, invd if invd is not None else torch.ones(-(-96 // mb) * mb * mb, device=cuda), q, e,
                                   torch.empty(64, ng, device=cuda), torch.empty(64, ng, dtype=torch.int64, device=cuda), mb, g, f)

    with pytest.raises(NotImplementedError):
        run(1, 48)                       # a group outside 16 / 32 / 64 / 128
    with pytest.raises(NotImplementedError):
        run(1, 64)                       # 96 columns are not whole groups of 64
    with pytest.raises(NotImplementedError):
        run(32, 16)                      # a microblock wider than a group: the host loop's
    with pytest.raises(NotImplementedError):
        run(1, 32, dmx.Format.from_shorthand("XP[4,0](CSS)"))   # stochastic rounding
    with pytest.raises(ValueError):
        run(1, 32, dmx.Format.from_shorthand("XP[4,2](CSN)"))   # no integer range: not a dynamic format at all
    with pytest.raises(ValueError):
        run(1, 32, dmx.Format.from_shorthand("FP[1|4|3,7](_N)"))


# ------------------------------------------------------------------------------------------------ optimal_brain_compressing
def _linear(dmx, cuda, fin, fout, dynamic, fmt="XP[4,0](CSN)", seed=0, weight=None, **config):
    torch.manual_seed(seed)
    m = dmx.nn.Linear(fin, fout).to(cuda)
    if weight is not None:
        with torch.no_grad():
            m.weight.copy_(weight)
    m.configure({"weight_format": fmt, "weight_dynamic": dynamic, **config})
    return m


def _compress(dmx, m, xs, **hp):
    """-> the Hessian as measured on the device"""
    with torch.no_grad(), m.optimal_brain_compressing(dmx.DmxModuleGPTQHyperparams(**hp)):
        for x in xs:
            m(x)
        return m.obc.H.clone()


@pytest.mark.parametrize("dynamic,mb,fuse,act_order", [({"per_group": 32}, 1, True, False), ({"per_group": 32}, 8, True, False),
                                                       ({"per_group": 32}, 1, False, False), ({"per_group": 16}, 32, True, False),
                                                       ({"per_group": 32}, 16, False, False), ({"per_group": 48}, 1, True, False),
                                                       ("per_token", 1, True, False), ("per_token", 1, True, True),
                                                       ("per_token", 8, False, False), ("per_token", 1, False, True),
                                                       ("per_tensor", 1, True, True), ({"per_group": 32}, 1, True, True)])
def test_diagonal_hessian_is_the_dynamic_cast(dmx, cuda, dynamic, mb, fuse, act_order):
    """inputs with orthogonal columns: H is diagonal, every update is zero -> Q is exactly ops.dynamic_fixed_qdq of W (of the permuted W,
    un-permuted, for groups under act_order: per-row and per-tensor scales do not depend on the order)"""
    m = _linear(dmx, cuda, 192, 40, dynamic)
    m.fuse_gptq = fuse
    W0 = m.weight.detach().clone()
    gran, g = ("per_group", dynamic["per_group"]) if isinstance(dynamic, dict) else (dynamic, None)
    x = torch.diag(torch.rand(192, device=cuda) + 0.5).unsqueeze(0)
    H = _compress(dmx, m, [x], microblock_size=mb, block_size=96, act_order=act_order)
    Q = m.weight.detach()
    perm = m.gptq_qparams["perm"]
    if act_order:
        assert torch.equal(perm, torch.argsort(torch.diag(H), descending=True, stable=True)) and not torch.equal(perm, torch.arange(192, device=cuda))
    else:
        assert perm is None
    Wp = W0[:, perm].contiguous() if (act_order and g) else W0
    want, sc, zp = dmx.ops.dynamic_fixed_qdq(Wp, m.weight_cast.format, gran, g, symmetric_qscheme=_qsym(dmx, m), return_qparams=True)
    got = Q[:, perm].contiguous() if (act_order and g) else Q
    assert bits_equal(got, want) == 0
    G = 192 // g if g else 1
    assert m.gptq_qparams["scale"].shape == (40, G) and m.gptq_qparams["zero_point"].shape == (40, G)
    if gran != "per_tensor":
        assert bits_equal(m.gptq_qparams["scale"].reshape(-1), sc) == 0 and torch.equal(m.gptq_qparams["zero_point"].reshape(-1), zp)
    else:
        assert (m.gptq_qparams["scale"] == sc).all() and (m.gptq_qparams["zero_point"] == zp).all()


# the calibration of fixture case "a" (tests/_gptq_ref.py CASES): Linear(256, 96), its seeded weight and three [2, 8, 256] inputs
def _case_a():
    c = CASES["a"]
    W = make("normal", (96, 256), seed=c["seed"]) * 0.05
    xs = [make("normal", c["input"], seed=c["seed"] + 1 + b) for b in range(3)]
    return W, xs


def _case_a_reference(g, mb, O):
    """the float64 restatement's loss on case "a" (CPU, once per (g, mb)) and the float64 Hessian"""
    def run():
        W, xs = _case_a()
        H = hessian64("linear", xs, None)
        Q64 = apply_ref_dynamic(W, H, mb, 128, g, 4, True, False, O, torch.float64)[0]
        return loss(W, Q64, H), H
    return _cached(("ref64", g, mb), run)


def _case_a_run(dmx, cuda, g, mb, fuse):
    """apply() on case "a" with XP[4,0](CSN) per_group g -> (W0, RTN, Q, H as measured on the device), all on the CPU; once per
    configuration for the tests below"""
    return _cached(("run", g, mb, fuse), lambda: _make_case_a_run(dmx, cuda, g, mb, fuse))


def _make_case_a_run(dmx, cuda, g, mb, fuse):
    W, xs = _case_a()
    m = _linear(dmx, cuda, 256, 96, {"per_group": g}, weight=W)
    m.fuse_gptq = fuse
    assert not _qsym(dmx, m)   # (the default qscheme is affine: what _case_a_reference restates)
    W0 = m.weight.detach().clone()
    with torch.no_grad():
        rtn = m.weight_cast(W0.clone())   # round-to-nearest: the module's own dynamic cast of the original weight
    H = _compress(dmx, m, [x.to(cuda) for x in xs], microblock_size=mb, block_size=128)
    return W0.cpu(), rtn.cpu(), m.weight.detach().cpu().clone(), H.cpu()


@pytest.mark.parametrize("mb", [1, 16])
@pytest.mark.parametrize("g", [32, 128])
def test_fused_matches_loop_and_beats_rtn(dmx, oracle, cuda, g, mb):
    """same calibration, fused kernel vs the torch loop: both below round-to-nearest's loss, fused within 2 % of the loop, at least 90 %
    of the elements equal (tests/test_gpu_gptq.py's conditions)"""
    W0, rtn, Qf, H = _case_a_run(dmx, cuda, g, mb, True)
    _, _, Ql, _ = _case_a_run(dmx, cuda, g, mb, False)
    lf, ll, lr = loss(W0, Qf, H), loss(W0, Ql, H), loss(W0, rtn, H)
    share = (Qf == Ql).float().mean().item()
    print(f"g={g} mb={mb}: fused {lf:.9e} loop {ll:.9e} rtn {lr:.9e} equal share {share:.6f}")
    assert lf < lr and ll < lr, (lf, ll, lr)
    assert lf <= 1.02 * ll, (lf, ll)
    assert share >= 0.9


# The float32 (kernel order) and float64 restatements of apply() (tests/_gptq_group_ref.py apply_ref_dynamic) on these four cases, on the
# CPU, both losses taken with the float64 Hessian: relative spreads |l32 - l64| / l64 of 7.63e-7 (g 32, mb 1), 2.8e-8 (g 32, mb 16),
# 2.5e-7 (g 128, mb 1), 2.4e-7 (g 128, mb 16); largest 7.63e-7.  The bound is twice that: the GPU's Cholesky chain differs from the CPU's
# float32 one by about as much again.  The bound is on the LOSS because the elements cannot carry one: the two restatements agree on only
# 30-63 % of the elements of Q -- a one-ulp difference in a group's scale moves every element of the group by an ulp, on the same integer
# code.
SPREAD_F32_F64 = 7.63e-7
EPS = 2 * SPREAD_F32_F64   # 1.526e-6


@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("mb", [1, 16])
@pytest.mark.parametrize("g", [32, 128])
def test_against_float64_restatement(dmx, oracle, cuda, g, mb, fuse):
    W0, _, Q, _ = _case_a_run(dmx, cuda, g, mb, fuse)
    l64, H64 = _case_a_reference(g, mb, oracle)
    lq = loss(W0, Q, H64)
    print(f"g={g} mb={mb} fuse={fuse}: loss {lq:.9e} float64 restatement {l64:.9e} ratio - 1 = {lq / l64 - 1:.3e} (eps {EPS:.3e})")
    assert lq <= (1 + EPS) * l64, (lq, l64, EPS)


@pytest.mark.parametrize("act_order", [False, True])
@pytest.mark.parametrize("g", [32, 128])
def test_after_apply(dmx, oracle, cuda, g, act_order):
    """the recorded scales, the switched-off cast, the forward on Q as written, and Q on the recorded grid (re-casting Q with the recorded
    scale and zero point of each group returns Q)"""
    W, xs = _case_a()
    m = _linear(dmx, cuda, 256, 96, {"per_group": g}, weight=W, input_formats=["BFP[8|8]{64}(SN)"])
    keys = set(m.state_dict())
    _compress(dmx, m, [x.to(cuda) for x in xs], microblock_size=1, block_size=128, act_order=act_order)
    qp = m.gptq_qparams
    G = 256 // g
    assert set(qp) == {"scale", "zero_point", "group_size", "perm"} and qp["group_size"] == g
    assert qp["scale"].shape == (96, G) and qp["scale"].dtype == torch.float32
    assert qp["zero_point"].shape == (96, G) and qp["zero_point"].dtype == torch.int64
    assert (qp["perm"] is None) if not act_order else (qp["perm"].dtype == torch.int64 and qp["perm"].shape == (256,))
    assert set(m.state_dict()) == keys                                     # a plain attribute: no state_dict key
    assert not m.weight_cast._flag("fake_quant_enabled") and m.input_casts.input_cast._flag("fake_quant_enabled")
    Q = m.weight.detach()
    x = xs[0].to(cuda)
    with torch.no_grad():
        y = m(x)
        want = F.linear(m.input_casts.input_cast(x), Q, m.bias)
    assert bits_equal(y, want) == 0
    perm = qp["perm"].cpu() if act_order else torch.arange(256)
    Qp = Q.cpu()[:, perm].contiguous()
    on_grid = oracle.fixed_point_affine_cast(Qp.reshape(-1, g), 4, 0, True, True, qp["scale"].cpu().reshape(-1), qp["zero_point"].cpu().reshape(-1),
                                             ch_axis=0)
    on_grid = on_grid.reshape(Qp.shape)
    # bit for bit, but for the sign of a zero: the cast rounds a small negative quotient to -0.0 (rintf keeps the sign, and with zero point 0
    # nothing removes it), while re-casting that -0.0 starts with -0.0 / scale + zp = +0.0.  The same value on the same grid point; every
    # other element must agree in every bit.  (Measured on case "a", g 32: 433 such zeros of 24576 elements, the only differing bits.)
    assert not torch.isnan(Qp).any() and torch.equal(on_grid, Qp)
    nz = Qp != 0
    assert bits_equal(on_grid[nz], Qp[nz]) == 0
    assert (on_grid[~nz] == 0).all()


def test_act_order_permutation_and_loss(dmx, oracle, cuda):
    """input channels whose scales differ by 100x: perm is the stable descending argsort of the measured diag(H), and the loss stays below
    round-to-nearest's"""
    gen = torch.Generator().manual_seed(21)
    W = torch.randn(32, 128, generator=gen) * 0.05
    sc = torch.logspace(0, 2, 128)[torch.randperm(128, generator=gen)]
    X = (torch.randn(4, 64, 128, generator=gen) * sc).to(cuda)
    m = _linear(dmx, cuda, 128, 32, {"per_group": 32}, weight=W)
    W0 = m.weight.detach().clone()
    with torch.no_grad():
        rtn = m.weight_cast(W0.clone())
    H = _compress(dmx, m, [X[i:i + 1] for i in range(4)], microblock_size=1, block_size=128, act_order=True)
    perm = m.gptq_qparams["perm"]
    assert torch.equal(perm, torch.argsort(torch.diag(H), descending=True, stable=True))
    d = torch.diag(H)[perm]
    assert (d[:-1] >= d[1:]).all() and d[0] > 1000 * d[-1]
    lq, lr = loss(W0, m.weight.detach(), H), loss(W0, rtn, H)
    print(f"act_order: loss {lq:.6e} rtn {lr:.6e}")
    assert lq < lr


@pytest.mark.parametrize("dynamic", ["per_token", "per_tensor"])
def test_per_token_and_per_tensor_equal_the_static_twin(dmx, cuda, dynamic):
    """the scale is taken once from W by group_minmax -> qparams; the static kernel does the rest: bit for bit apply() on a twin module
    whose static per-channel / per-tensor cast holds those scales"""
    from dmx_compressor_amd.observer import get_qmin_qmax

    W, xs = _case_a()
    xs = [x.to(cuda) for x in xs]
    m = _linear(dmx, cuda, 256, 96, dynamic, weight=W)
    twin = _linear(dmx, cuda, 256, 96, None, weight=W)
    per_row = dynamic == "per_token"
    Wd = twin.weight.detach().float()
    qmin, qmax = get_qmin_qmax(twin.weight_cast.format)
    mn, mx = dmx.ops.group_minmax(Wd if per_row else Wd.reshape(1, -1), 0, 1)
    sc, zp = dmx.ops.qparams(mn, mx, qmin, qmax, _qsym(dmx, m))
    wc = twin.weight_cast
    if per_row:
        wc.qscheme, wc.is_per_channel, wc.ch_axis = torch.per_channel_affine, True, 0
    wc.scale, wc.zero_point = sc.clone(), zp.clone()
    _compress(dmx, m, xs, microblock_size=1, block_size=128)
    _compress(dmx, twin, xs, microblock_size=1, block_size=128)
    assert bits_equal(m.weight.detach(), twin.weight.detach()) == 0
    assert not torch.equal(m.weight.detach().cpu(), W)
    qp = m.gptq_qparams
    assert qp["group_size"] is None and qp["perm"] is None and qp["scale"].shape == (96, 1) and qp["zero_point"].shape == (96, 1)
    assert bits_equal(qp["scale"].reshape(-1), sc.expand(96).contiguous()) == 0 and torch.equal(qp["zero_point"].reshape(-1), zp.expand(96))
    assert not m.weight_cast._flag("fake_quant_enabled") and twin.weight_cast._flag("fake_quant_enabled")
    assert not hasattr(twin, "gptq_qparams")                               # a static cast: as before


def test_refusals_leave_the_module_alone(dmx, cuda):
    def refused(m, x, exc, **hp):
        w0 = m.weight.detach().clone()
        with torch.no_grad():
            y0 = m(x)
        with pytest.raises(exc), torch.no_grad(), m.optimal_brain_compressing(dmx.DmxModuleGPTQHyperparams(**hp)):
            m(x)
        with torch.no_grad():
            assert m.obc is None and bits_equal(m.weight.detach(), w0) == 0 and bits_equal(m(x), y0) == 0
        assert not hasattr(m, "gptq_qparams")

    torch.manual_seed(9)
    c = dmx.nn.Conv2d(8, 16, 3).to(cuda)
    c.configure({"weight_format": "XP[4,0](CSN)", "weight_dynamic": "per_tensor"})
    refused(c, torch.randn(2, 8, 10, 10, device=cuda), dmx.DmxqError)
    m = dmx.nn.Linear(128, 32).to(cuda)
    m.configure({"weight_format": "BFP[8|8]{64}(SN)"})
    refused(m, torch.randn(2, 8, 128, device=cuda), dmx.DmxqError, microblock_size=64, act_order=True)
    m = _linear(dmx, cuda, 256, 32, {"per_group": 256})
    refused(m, torch.randn(2, 8, 256, device=cuda), ValueError, block_size=128)
