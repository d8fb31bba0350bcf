"""Host tests (no GPU) of HQQ (ops.hqq_qdq, DmxHQQHyperparams; DESIGN.md §8 "HQQ"): the properties of the CPU checker itself
(tests/_hqq_ref.py), which the GPU tests compare the kernel and the chain against, the outcomes of the special groups DESIGN.md lists,
and the argument checks that need no GPU."""
import math

import pytest
import torch

import _hqq_ref as R
from _data import make

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


@pytest.fixture(scope="module")
def heavy():
    return make("heavy", (64, 256), seed=11, dtype=F32)


# ------------------------------------------------------------------------------------------------ the checker's own invariants
@pytest.mark.parametrize("p,sym", [(2, False), (3, True), (4, False), (8, True)])
def test_iters0_is_round_to_nearest(heavy, p, sym):
    qmin, qmax = R.qrange(p, sym)
    for x in (heavy, heavy.to(BF16), make("normal", (8, 128), seed=3, dtype=F16)):
        y, s, z, codes = R.hqq_ref(x, qmin, qmax, 64, iters=0)
        y0, s0, z0 = R.rtn_closed_form(x, qmin, qmax, 64)
        assert torch.equal(_bits(y), _bits(y0)) and torch.equal(s, s0) and torch.equal(z, z0)
        assert int(codes.max()) <= qmax - qmin


@pytest.mark.parametrize("lp", [0.5, 1.0, 0.7])
@pytest.mark.parametrize("p", [2, 4])
def test_group_l1_never_rises(heavy, lp, p):
    qmin, qmax = R.qrange(p, False)
    x = torch.cat([heavy[:16], make("normal", (16, 256), seed=5, dtype=F32) * 4.0])
    base = R.group_l1(x, R.hqq_ref(x, qmin, qmax, 64, lp, iters=0)[0], 64)
    for iters in (1, 5, 20):
        y, *_, hist = R.hqq_ref(x, qmin, qmax, 64, lp, iters=iters, history=True)
        l1 = R.group_l1(x, y, 64)
        assert bool((l1 <= base).all())
        assert torch.equal(l1, hist[-1]) and torch.equal(base, hist[0])        # the kept error IS the output's error
        assert bool((hist[1:] <= hist[:-1]).all())                             # and it never rises from one k to the next


@pytest.mark.parametrize("dtype", [BF16, F16, F32])
@pytest.mark.parametrize("p,sym", [(2, True), (3, False), (4, True), (8, False)])
def test_y_reconstructs_from_codes(dtype, p, sym):
    qmin, qmax = R.qrange(p, sym)
    x = (make("normal", (12, 128), seed=p, dtype=F32) * 3.0).to(dtype)
    y, s, z, codes = R.hqq_ref(x, qmin, qmax, 32, iters=5)
    q = codes.reshape(-1, 32).float() + torch.full((1, 1), float(qmin))
    rec = ((q - z[:, None]) * s[:, None]).to(dtype).reshape(x.shape)
    assert torch.equal(_bits(rec), _bits(y))
    assert int(codes.max()) <= qmax - qmin


def test_special_groups_give_the_documented_outcomes():
    g, (qmin, qmax) = 64, R.qrange(4, False)
    sp = R.special_groups(g)
    x = torch.stack(list(sp.values()))
    names = list(sp)
    for iters in (0, 20):
        y, s, z, codes = R.hqq_ref(x, qmin, qmax, g, iters=iters)
        row = {n: (y[i], float(s[i]), float(z[i]), codes[i]) for i, n in enumerate(names)}
        # all-zero: scale 1, zero point qmin, y = +0 everywhere, codes 0
        y_, s_, z_, c_ = row["zero"]
        assert s_ == 1.0 and z_ == qmin and torch.equal(_bits(y_), _bits(torch.zeros(g))) and int(c_.max()) == 0
        # constant c: scale 1, zero point qmin - c, y = c exactly
        y_, s_, z_, c_ = row["constant"]
        assert s_ == 1.0 and z_ == qmin - 3.0 and torch.equal(y_, torch.full((g,), 3.0)) and int(c_.max()) == 0
        # one NaN: both extrema NaN -> scale 1, zero point NaN, the whole group NaN, codes 0
        y_, s_, z_, c_ = row["nan"]
        assert s_ == 1.0 and math.isnan(z_) and bool(torch.isnan(y_).all()) and int(c_.max()) == 0
        # +Inf: scale 1 (the spread is Inf), zero point z_0 = qmin - mn kept (every later error is NaN), the Inf lands on qmax: finite
        y_, s_, z_, c_ = row["pinf"]
        assert s_ == 1.0 and z_ == qmin + 1.0 and bool(torch.isfinite(y_).all()) and float(y_[1]) == qmax - z_ and int(c_[1]) == qmax - qmin
        # -Inf: scale 1, zero point +Inf: y = -Inf at the finite elements, NaN at the -Inf itself
        y_, s_, z_, c_ = row["ninf"]
        assert s_ == 1.0 and z_ == float("inf")
        assert math.isnan(float(y_[g - 2])) and bool((y_[torch.arange(g) != g - 2] == float("-inf")).all())
        # a spread that overflows float32: scale 1, zero point qmin - mn; finite, no NaN
        y_, s_, z_, c_ = row["overflow"]
        assert s_ == 1.0 and z_ == float(torch.tensor(float(qmin)) - torch.tensor(-3.0e38)) and bool(torch.isfinite(y_).all())


def test_special_groups_do_not_touch_their_neighbours():
    g, (qmin, qmax) = 32, R.qrange(3, True)
    x = make("normal", (6, 128), seed=2, dtype=F32)
    xp, spots = R.plant(x, g)
    y, s, z, _ = R.hqq_ref(x, qmin, qmax, g)
    yp, sp, zp, _ = R.hqq_ref(xp, qmin, qmax, g)
    planted = sorted(i for v in spots.values() for i in v)
    keep = torch.tensor([i for i in range(x.numel() // g) if i not in planted])
    assert len(planted) == 18 and len(keep) == 6
    assert torch.equal(y.reshape(-1, g)[keep], yp.reshape(-1, g)[keep]) and torch.equal(s[keep], sp[keep]) and torch.equal(z[keep], zp[keep])


@pytest.mark.parametrize("p", [2, 3])
def test_strictly_lower_l1_on_heavy_tails(p):
    """tests/_data.py's "heavy" kind (a normal times exp(4 normal)), g = 64: the summed L1 error after 20 iterations is strictly below
    round-to-nearest's (iters=0)"""
    qmin, qmax = R.qrange(p, False)
    x = make("heavy", (64, 512), seed=21, dtype=F32)
    l0 = R.group_l1(x, R.hqq_ref(x, qmin, qmax, 64, iters=0)[0], 64).double().sum()
    l20 = R.group_l1(x, R.hqq_ref(x, qmin, qmax, 64, iters=20)[0], 64).double().sum()
    print(f"XP[{p},0] heavy g=64: L1 {float(l0):.6g} -> {float(l20):.6g} (ratio {float(l20 / l0):.4f})")
    assert float(l20) < float(l0)


def test_tree_sum_is_the_adjacent_pair_tree():
    v = make("normal", (3, 8), seed=1, dtype=F32)
    want = ((v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3])) + ((v[:, 4] + v[:, 5]) + (v[:, 6] + v[:, 7]))
    assert torch.equal(R.tree_sum(v), want)
    w = v[:, :6]   # 6 -> 3 -> 2 -> 1: the odd level carries its last value up
    assert torch.equal(R.tree_sum(w), ((w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])) + (w[:, 4] + w[:, 5]))


# ------------------------------------------------------------------------------------------------ argument checks (no GPU)
def test_hqq_check_accepts_and_normalises(dmx):
    ops = dmx.ops
    fmt, g, lp, beta, kappa, iters = ops.hqq_check("XP[4,0](CSN)")
    assert repr(fmt) == "XP[4,0](CSN)" and (g, lp, beta, kappa, iters) == (64, 0.5, 10.0, 1.01, 20)
    assert ops.hqq_check("XP[3,0](C_N)", 48, 1, 2, 1, 0)[1:] == (48, 1.0, 2.0, 1.0, 0)
    assert ops.HQQ_CHAIN_BY_DEFAULT is not None and ops.HQQ_KERNEL_NORMS == (0.5, 1.0)


@pytest.mark.parametrize("bad", [
    dict(fmt="XP[4,1](CSN)"), dict(fmt="XP[4,0](_SN)"), dict(fmt="XP[4,0](CSS)"), dict(fmt="XP[4,0](CSU)"), dict(fmt="FP[1|4|3,7](FN)"),
    dict(fmt=4), dict(group_size=0), dict(group_size=64.0), dict(group_size=True), dict(group_size=None),
    dict(lp_norm=0.0), dict(lp_norm=1.5), dict(lp_norm=-0.5), dict(lp_norm=float("nan")), dict(lp_norm="0.5"),
    dict(beta=0.0), dict(beta=-1.0), dict(beta=float("inf")), dict(kappa=0.99), dict(kappa=float("nan")),
    dict(iters=-1), dict(iters=2.0), dict(iters=True),
])
def test_hqq_check_refuses(dmx, bad):
    with pytest.raises(ValueError):
        dmx.ops.hqq_check(**{"fmt": "XP[4,0](CSN)", **bad})


def test_front_end_errors_come_before_any_gpu_use(dmx):
    ops, x = dmx.ops, torch.zeros(4, 96, dtype=BF16)   # (a CPU tensor: a ValueError must come before the DmxqError of a non-GPU tensor)
    with pytest.raises(ValueError, match="multiple of the group size"):
        ops.hqq_qdq(x, "XP[4,0](CSN)", 64)
    with pytest.raises(ValueError, match="8 bits"):
        ops.hqq_qdq(x, "XP[12,0](CSN)", 32, return_codes=True)
    with pytest.raises(ValueError):
        ops.hqq_qdq(torch.zeros(()), "XP[4,0](CSN)")
    with pytest.raises(dmx.DmxqError):
        ops.hqq_qdq(x, "XP[4,0](CSN)", 32)


def test_hqq_class_names_the_kernels_groups(dmx):
    ops = dmx.ops
    for dt in (BF16, F16, F32):
        for g in (16, 32, 64, 128, 256):
            assert ops.hqq_class(g, dt) == "group"
        for g in (8, 48, 512, 1, 0):
            assert ops.hqq_class(g, dt) is None


def test_hyperparams_checks(dmx):
    H = dmx.DmxHQQHyperparams
    h = H()
    assert (h.group_size, h.lp_norm, h.beta, h.kappa, h.iters) == (None, 0.5, 10.0, 1.01, 20)
    assert H(group_size=128, lp_norm=1, iters=0).group_size == 128
    for bad in (dict(group_size=0), dict(group_size=1.5), dict(group_size=True), dict(lp_norm=0), dict(lp_norm=2), dict(lp_norm="a"),
                dict(beta=0), dict(beta=float("nan")), dict(kappa=0.5), dict(iters=-1), dict(iters=1.0)):
        with pytest.raises((ValueError, TypeError)):
            H(**bad)
