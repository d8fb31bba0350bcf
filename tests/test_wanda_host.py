"""-m "not gpu": the host side of Wanda -- the CPU definition's own properties, the class and workspace queries of the
library, the argument errors that need no GPU, the hyperparameters, the recipe's wiring, the refusals and the silent no-ops."""
import ctypes
import os
import re

import pytest
import torch

import _wanda_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
SPARSE = "BTOPK{2:4,-1}(U)"


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("dtype", [BF16, F16])
def test_float64_sum_of_the_exact_values_does_not_depend_on_the_order(dtype):
    x = R.exact_values((4096, 64), dtype, 1)
    a = x.double().abs()
    assert float(a.min()) >= 2.0 ** -4 and float(a.max()) < 2.0 ** 4
    unit = 2.0 ** (-22 if dtype == BF16 else -28)
    sq = x.double().pow(2)
    assert torch.equal(sq / unit, (sq / unit).round())   # every square is a multiple of the unit
    fwd = R.sumsq_ref([x])
    assert torch.equal(R.sumsq_ref([x.flip(0)]), fwd)
    assert torch.equal(R.sumsq_ref(list(x.split(100))), fwd)
    seq = torch.zeros(64, dtype=torch.float64)
    for r in sq:
        seq += r
    assert torch.equal(seq, fwd)
    # a float32 accumulation is not exact: a test that passes on these inputs has accumulated in float64
    f32 = torch.zeros(64)
    for r in x.float():
        f32 += r * r
    assert not torch.equal(f32.double(), fwd)


def test_reference_score_and_mask_rule(oracle):
    nan, inf = float("nan"), float("inf")
    w = torch.tensor([[1.0, -2.0, 0.5, -0.0, 3.0, nan, 1.0, 1.0]], dtype=BF16)
    an = torch.tensor([2.0, 1.0, 0.0, 4.0, inf, 1.0, 1.0, 1.0])
    s = R.score_ref(w, an)
    assert s.dtype == F32 and s[0, :5].tolist() == [2.0, 2.0, 0.0, 0.0, inf] and torch.isnan(s[0, 5])
    for K, M in [(2, 4), (1, 4), (4, 8), (2, 8)]:
        assert torch.equal(R.nm_ref(s, K, M), R.nm_ref(s, K, M, oracle)), (K, M)
    # ties go by index (the lower index is zeroed first), -0 == +0, NaN ranks highest
    assert R.nm_ref(s, 2, 4).tolist() == [[1.0, 1.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0]]
    assert R.nm_ref(torch.tensor([[0.0, -0.0, -0.0, 0.0]]), 2, 4).tolist() == [[0.0, 0.0, 1.0, 1.0]]
    score, mask, y = R.wanda_ref(w, an, 2, 4, oracle)
    assert y.dtype == F32 and torch.signbit(y[0, 3]) and y[0, 2] == 0 and not torch.signbit(y[0, 2])
    assert R.act_norm_ref(torch.tensor([4.0, 0.0, nan, 1e300], dtype=torch.float64)).tolist()[:2] == [2.0, 0.0]
    assert torch.isinf(R.act_norm_ref(torch.tensor([1e300], dtype=torch.float64)))[0]


# ------------------------------------------------------------------------------------------------ the library's host queries
def test_wanda_class_over_dtype_length_and_group(dmx):
    L = dmx._lib.lib()
    for dt in (dmx._lib.F32, dmx._lib.F16, dmx._lib.BF16):
        for length in (16, 32, 64, 1024, 4096, 14336):
            for M in (0, 4, 8, 16):
                assert L.dmxq_wanda_class(dt, length, M) == 1, (dt, length, M)
        for length in (8, 24, 40, 100, 4100, 0, -16):
            for M in (0, 4, 8, 16):
                assert L.dmxq_wanda_class(dt, length, M) == 0, (dt, length, M)
        for M in (1, 2, 3, 5, 32, 64, -4):
            assert L.dmxq_wanda_class(dt, 64, M) == 0, (dt, M)
    assert L.dmxq_wanda_class(7, 64, 4) == 0
    assert dmx.ops.wanda_class(BF16, 4096, 4) is True and dmx.ops.wanda_class(F32, 24, 8) is False
    assert dmx.ops.WANDA_CHAIN_BY_DEFAULT <= {0, 4, 8, 16}


def test_channel_sumsq_workspace_query(dmx):
    q = dmx.ops.channel_sumsq_workspace_bytes
    assert q(0, 64) == 0 and q(5, 0) == 0 and q(-1, 8) == 0
    assert q(1, 8) == 8 * 8                      # one slab
    assert q(32, 64) == 64 * 8 and q(33, 64) == 2 * 64 * 8
    assert q(8192, 4096) == 256 * 4096 * 8       # 256 slabs of 32 rows
    assert q(8192, 14336) == 73 * 14336 * 8      # 2048 / 28 column tiles = 73 slabs of 113 rows
    assert q(2048, 768) == 64 * 768 * 8
    for rows, C in [(4099, 768), (257, 1032), (5, 13), (1 << 20, 16)]:
        b = q(rows, C)
        assert b % (8 * C) == 0 and 1 <= b // (8 * C) <= 2048 and b // (8 * C) <= -(-rows // 32)


def test_c_abi_argument_errors_without_a_gpu(dmx):
    L, lib = dmx._lib.lib(), dmx._lib
    null, p = ctypes.c_void_p(None), ctypes.c_void_p(4096)
    odd = ctypes.c_void_p(4098)
    nm = L.dmxq_wanda_nm
    assert nm(null, lib.BF16, null, null, null, 0, p, lib.F32, 0, 64, 2, 4, null) == lib.OK                  # an empty weight
    assert nm(p, lib.BF16, p, null, null, 0, p, lib.F32, 4, 64, 5, 4, null) == lib.ERR_BAD_ARG               # K > M
    assert nm(p, lib.BF16, p, null, null, 0, p, lib.F32, 4, 64, 0, 4, null) == lib.ERR_BAD_ARG               # K < 1
    assert nm(p, lib.BF16, p, null, null, 0, p, lib.F32, 4, 40, 8, 16, null) == lib.ERR_BAD_ARG              # L % M
    assert nm(p, lib.BF16, p, null, null, 0, null, 0, 4, 64, 2, 4, null) == lib.ERR_BAD_ARG                  # all three outputs absent
    assert nm(p, 9, p, p, null, 0, null, 0, 4, 64, 2, 4, null) == lib.ERR_BAD_ARG                            # dtype
    assert nm(p, lib.BF16, p, null, p, 9, null, 0, 4, 64, 2, 4, null) == lib.ERR_BAD_ARG                     # mask dtype
    assert nm(p, lib.BF16, null, p, null, 0, null, 0, 4, 64, 2, 4, null) == lib.ERR_BAD_ARG                  # no act_norm
    assert nm(p, lib.BF16, p, null, p, lib.F32, null, 0, 4, 64, 0, 0, null) == lib.ERR_BAD_ARG               # K = M = 0 is the score alone
    assert nm(p, lib.BF16, p, p, null, 0, null, 0, 4, 24, 4, 8, null) == lib.ERR_UNSUPPORTED                 # class 0: the chain's
    assert nm(p, lib.BF16, p, p, null, 0, null, 0, 4, 64, 1, 2, null) == lib.ERR_UNSUPPORTED                 # M = 2
    assert nm(odd, lib.BF16, p, p, null, 0, null, 0, 4, 64, 2, 4, null) == lib.ERR_UNSUPPORTED               # alignment
    acc = L.dmxq_channel_sumsq_accumulate
    assert acc(null, lib.BF16, 0, 64, null, null, null) == lib.OK
    assert acc(null, lib.BF16, 4, 64, p, p, null) == lib.ERR_BAD_ARG
    assert acc(p, lib.BF16, 4, 64, p, null, null) == lib.ERR_BAD_ARG
    assert acc(p, 5, 4, 64, p, p, null) == lib.ERR_BAD_ARG
    assert acc(p, lib.BF16, -1, 64, p, p, null) == lib.ERR_BAD_ARG


def test_front_end_argument_errors_come_before_any_gpu_use(dmx):
    w, an = torch.zeros(4, 64, dtype=BF16), torch.ones(64)
    f = dmx.ops.wanda_nm_sparsify
    with pytest.raises(ValueError, match="do not fit"):
        f(w, an, 5, 4)
    with pytest.raises(ValueError, match="not a multiple"):
        f(torch.zeros(4, 40, dtype=BF16), torch.ones(40), 8, 16)
    with pytest.raises(ValueError, match="one entry per input channel"):
        f(w, torch.ones(32), 2, 4)
    with pytest.raises(TypeError, match="float32"):
        f(w, torch.ones(64, dtype=BF16), 2, 4)
    with pytest.raises(TypeError, match="float32"):
        dmx.ops.wanda_score(w, torch.ones(64, dtype=torch.float64))
    with pytest.raises(ValueError, match="nothing to compute"):
        f(w, an, 2, 4, return_y=False)
    with pytest.raises(ValueError, match="score alone"):
        f(w, an, 0, 0)
    with pytest.raises(ValueError, match="matrix"):
        f(torch.zeros(64, dtype=BF16), an, 2, 4)
    # valid arguments on CPU tensors: the library has no CPU path
    with pytest.raises(dmx.DmxqError):
        f(w, an, 2, 4)
    with pytest.raises(dmx.DmxqError):
        dmx.ops.channel_sumsq(torch.zeros(4, 8))


def test_signatures_cover_the_header(dmx):
    src = open(os.path.join(ROOT, "include", "dmxq.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    new = ["dmxq_channel_sumsq_workspace_bytes", "dmxq_channel_sumsq_accumulate", "dmxq_wanda_class", "dmxq_wanda_nm"]
    L = dmx._lib.lib()
    for name in new:
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src)
        assert m, name
        assert len(dmx._lib.SIGNATURES[name]) == len([a for a in m.group(1).split(",") if a.strip()]), name
        assert hasattr(L, name)
    assert L.dmxq_abi_version() == 4
    assert L.dmxq_channel_sumsq_workspace_bytes.restype is ctypes.c_int64


# ------------------------------------------------------------------------------------------------ hyperparameters, recipe, exports
def test_hyperparams_validation(dmx):
    hp = dmx.DmxWandaHyperparams()
    assert hp.reset is True and dmx.DmxWandaHyperparams(reset=False).reset is False
    assert dmx.nn.DmxWandaHyperparams is dmx.DmxWandaHyperparams and "DmxWandaHyperparams" in dmx.nn.__all__
    for bad in (1, 0, None, "yes"):
        with pytest.raises(TypeError):
            dmx.DmxWandaHyperparams(reset=bad)
    m = dmx.nn.Linear(64, 32)
    m.configure({"weight_sparseness": SPARSE})
    with pytest.raises(TypeError, match="DmxWandaHyperparams"):
        with m.wanda_pruning(dmx.DmxModuleGPTQHyperparams()):
            pass
    assert m.wanda is None


def test_recipe_wiring_and_exports(dmx):
    from dmx_compressor_amd import advanced_recipe
    assert "DmxWandaRecipe" in advanced_recipe.__all__ and dmx.DmxWandaRecipe is advanced_recipe.DmxWandaRecipe
    assert issubclass(dmx.DmxWandaRecipe, dmx.DmxBaseRecipe)
    r = dmx.DmxWandaRecipe(lambda mdl: {l: dmx.DmxWandaHyperparams() for l in mdl})
    assert r.recipe_context_manager is dmx.DmxModule.wanda_pruning
    for name in ("channel_sumsq", "wanda_score", "wanda_nm_sparsify", "wanda_class", "WANDA_CHAIN_BY_DEFAULT"):
        assert name in dmx.ops.__all__ and hasattr(dmx.ops, name)
    assert dmx.ops._front._wanda_routes.keys() == {"fused", "chain"}
    # entering and leaving over modules on which Wanda does nothing: every context opens and closes, nothing is set
    model = torch.nn.Sequential(dmx.nn.Linear(8, 8), dmx.nn.LayerNorm(8))
    with r.applied_to(model) as entered:
        assert len(entered) == 2 and all(l.wanda is None for l in model)


def test_the_two_refusals_come_before_any_state_is_touched(dmx):
    m = dmx.nn.Linear(64, 32)
    m.configure({"weight_sparseness": SPARSE})
    m.smoothquant.enable(True)
    with pytest.raises(dmx.DmxqError, match="SmoothQuant"):
        with m.wanda_pruning(dmx.DmxWandaHyperparams()):
            pass
    assert m.wanda is None and m.wanda_sumsq is None
    m.smoothquant.enable(False)
    m.configure({"weight_sparseness": "BTOPK{2:4,0}(U)"})
    with pytest.raises(dmx.DmxqError, match="block_dim"):
        with m.wanda_pruning(dmx.DmxWandaHyperparams()):
            pass
    assert m.wanda is None and m.wanda_sumsq is None
    m.configure({"weight_sparseness": "BTOPK{2:4,1}(U)"})   # dimension 1 IS the last of a 2-D weight
    with pytest.raises(RuntimeError, match="no calibration token"):
        with m.wanda_pruning(dmx.DmxWandaHyperparams()):
            assert m.wanda is not None
    assert m.wanda is None


def test_silent_no_op_on_other_modules(dmx):
    dense = dmx.nn.Linear(8, 8)
    conv = dmx.nn.Conv2d(4, 4, 3)
    conv.configure({"weight_sparseness": SPARSE})
    for m in (conv, dmx.nn.LayerNorm(8), dense):
        with m.wanda_pruning(dmx.DmxWandaHyperparams()) as ctx:
            assert ctx is m and m.wanda is None
        assert m.wanda is None and m.wanda_act_norm is None
    assert dense.weight_sparsifier.score.shape == torch.Size([0])
