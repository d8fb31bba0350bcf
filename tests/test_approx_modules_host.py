"""Host test (no GPU, no reference) of tests/golden/approx_modules_{f32,bf16,f16}.npz: the forward outputs of the REFERENCE's
activation / normalisation DmxModules on the case table of tests/_approx_cases.py, written by oracle/gen_golden_r7.py.

Checked here:
  * the inputs regenerated from the table hash to the stored digests (the GPU test runs this repo's modules on THESE inputs);
  * `raw` (the module's `_forward(input_cast(x))`) and `y` (its forward) are what the oracle's casts around torch's CPU function give:
    bit for bit where torch's CPU capability is the recorded one; on another CPU torch's vectorised exp / erf may differ in the last
    place, and there every element must lie in the cast bracket (tests/_data.outside_cast_bracket) of 1 ulp around the stored `raw`;
  * what the reference does with `GELU(approximate="tanh")`: its stored rows ARE the rows of `GELU()` -- the constructor argument never
    reaches `F.gelu` there.  This repo's `nn.GELU(approximate="tanh")` evaluates torch's tanh form (a documented
    divergence; tests/test_gpu_approx_modules.py pins it to the float64 tanh form)."""
import pytest
import torch

from _approx_cases import CASES, BY_NAME, CONFIGS, DTYPES, Fixture, case_input, case_params, cpu_cast, to_bits, torch_forward
from _data import outside_cast_bracket, sha256_bits


@pytest.fixture(scope="module", params=sorted(DTYPES))
def fx(request):
    return Fixture(request.param)


def _mismatches(a, b):
    both_nan = (torch.isnan(a.float()) & torch.isnan(b.float())).numpy()
    return int(((to_bits(a) != to_bits(b)) & ~both_nan).sum())


def test_every_case_of_the_table_is_in_the_fixture(fx):
    missing = [c.name for c in CASES if not fx.has(c)]
    assert not missing, missing
    for c in CASES:
        for config in CONFIGS:
            assert fx.y(c, config).dtype == fx.dtype and tuple(fx.raw(c, config).shape) == c.shape
            assert fx.d_ref(c.family, config) >= 0.0


def test_regenerated_inputs_hash_to_the_stored_digests(fx):
    for c in CASES:
        assert sha256_bits(case_input(c, fx.dtype)) == fx.sha256(c), c.name


def test_oracle_casts_around_torch_reproduce_the_reference_forward(fx, oracle):
    same_cpu = torch.backends.cpu.get_cpu_capability() == fx.cpu_capability
    total = 0
    for c in CASES:
        x = case_input(c, fx.dtype)
        w, b = case_params(c, fx.dtype)
        for config in CONFIGS:
            cast = cpu_cast(oracle, config)
            raw0 = torch_forward(c, cast(x), w, b, fx.eps(c, config))
            y0 = cast(raw0)
            raw, y = fx.raw(c, config), fx.y(c, config)
            assert raw0.dtype == fx.dtype and tuple(y0.shape) == c.shape
            if c.family == "softmax":
                assert fx.dim(c, config) == c.kwargs["dim"]
            n_raw, n_y = _mismatches(raw0, raw), _mismatches(y0, y)
            total += n_raw + n_y
            if same_cpu:
                assert n_raw == 0 and n_y == 0, (c.name, config, n_raw, n_y)
            else:
                # (the recorded NaN-for-+Inf elements are a property of the recording CPU's vectorised kernel: not compared)
                keep = ~fx.defect(c, config)
                assert outside_cast_bracket(raw0[keep], raw.double()[keep], lambda t: t.clone(), fx.dtype, 1.0) == 0, (c.name, config, n_raw)
                assert outside_cast_bracket(y0[keep], raw.double()[keep], cast, fx.dtype, 1.0) == 0, (c.name, config, n_y)
    print(f"{fx.dtype}: torch CPU capability {torch.backends.cpu.get_cpu_capability()} (recorded: {fx.cpu_capability}): "
          f"{total} elements differ from the stored bits")


def test_reference_gelu_ignores_approximate_tanh(fx):
    for config in CONFIGS:
        for part in (fx.raw, fx.y):
            assert _mismatches(part(BY_NAME["gelu_approximate_tanh"], config), part(BY_NAME["gelu"], config)) == 0, config
        assert fx.d_ref("gelu_tanh", config) == fx.d_ref("gelu", config)
    # ... and the erf form is NOT the tanh form on these inputs: the divergence is observable
    c = BY_NAME["gelu"]
    x = case_input(c, fx.dtype)
    tanh_form = torch.nn.functional.gelu(x, approximate="tanh")
    assert _mismatches(tanh_form, fx.y(c, "same")) > 0


def test_recorded_nan_for_inf_elements_are_erf_gelu_of_plus_infinity(fx, oracle):
    """the one place where the reference's CPU value and the float64 truth disagree on NaN / Inf: torch's vectorised
    CPU erf-GELU of +Inf.  The generator admits nothing else; here: every recorded element is a NaN whose cast input is +Inf, in a
    GELU case, and stands for +Inf."""
    seen = 0
    for c in CASES:
        for config in CONFIGS:
            d = fx.defect(c, config)
            if not bool(d.any()):
                continue
            seen += int(d.sum())
            assert c.family in ("gelu", "gelu_tanh"), c.name
            cin = cpu_cast(oracle, config)(case_input(c, fx.dtype))
            assert bool((cin[d] == float("inf")).all()) and bool(torch.isnan(fx.raw(c, config)[d]).all())
            assert bool((fx.centre(c, config)[d] == float("inf")).all())
            assert bool((torch.nn.functional.gelu(cin.double())[d] == float("inf")).all())
    assert seen > 0
