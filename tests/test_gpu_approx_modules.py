"""-m gpu: the activation / normalisation DmxModules (nn.Softmax, LayerNorm, RMSNorm, GELU, SiLU, QuickGELU, Exp, NewGELU, FastGELU) on
the HIP kernels of csrc/approx.hip, act_cast.hip and lut16.hip, pinned to the REFERENCE's own module forwards.

tests/golden/approx_modules_{f32,bf16,f16}.npz (oracle/gen_golden_r7.py) holds, for every case of tests/_approx_cases.py and the
configurations "basic" (config_rules.BASIC: FLOAT16 in, FLOAT16 out) and "same" (unconfigured), the reference module's
`raw = _forward(input_cast(x))` and `y = forward(x)` on its CPU path, and `d_ref`, how far `raw` itself sits from the float64 truth.
Here the SAME module is built from this repo's `dmx.nn` (same constructor arguments, weights, this repo's config_rules.BASIC) and run;
tests/test_gpu_act_cast.py checks the kernels against a truth its author assembled, this file checks that the modules MEAN what the
reference's mean (eps defaults, affine handling, dim, which function, the dtype weight and bias are applied in).

Contract: the existing one (tests/_data.outside_cast_bracket) re-centred on the reference's value,
    got == cast_out(v)  for some v within (N + d_ref) ulps of `raw`,
N the number tests/test_gpu_act_cast.py grants the kernel against the truth (imported, not restated), widened only by the reference's
own distance from that truth; exact at the FLOAT16 flush / saturation cliffs because the bracket is taken through the cast.  Over ALL
elements.  The count of elements whose bits differ from `y` and their largest distance are printed, not asserted: no cap exists that
does not come from this library's own output (profiles/r14_accuracy_vs_reference.txt keeps the measured ones).

Two places where the reference's CPU path is not the yardstick, both recorded in the fixture and checked from the
other side by tests/test_approx_modules_host.py:
  * `GELU(approximate="tanh")`: the reference evaluates erf (`test_reference_gelu_ignores_approximate_tanh`); this repo honours the
    argument, and that module is pinned to the float64 tanh form under the existing contract;
  * erf-GELU of +Inf: torch's vectorised CPU kernel returns NaN where float64 (and torch on a GPU) return +Inf; at those recorded
    elements the float64 value stands in for `raw`.
"""
import pytest
import torch

from _approx_cases import CASES, CONFIGS, DTYPES, Fixture, build_module, case_input, cpu_cast, distance_to
from _data import outside_cast_bracket, sha256_bits
from test_gpu_act_cast import UNARY, _basic, _ln_truth, _n_ulp, _row_n_ulp

pytestmark = pytest.mark.gpu

# NewGELU / FastGELU have no kernel of their own in this library: its casts around torch's GPU evaluation of transformers' formula
# 0.5 x (1 + tanh(z(x))), op by op in the tensor dtype.  No earlier contract names a number for them, so this one is derived.  With
# every operation correctly rounded (relative error eps / 2 each) the five operations that form z leave it with a relative error of
# 2.5 eps, which tanh turns into at most max |z sech^2 z| * 2.5 eps = 1.12 eps absolute; tanh's own rounding adds 0.25 eps and the
# rounding of 1 + tanh (a value below 2) 0.5 eps; the two remaining products add (1 + tanh) eps <= 2 eps relative to |x| / 2.  Total
# 3.9 eps |x| / 2, i.e. < 8 ulps of the floor |x| / 2 (an ulp is more than half of eps * magnitude).  A library tanh that is 4 ulps
# off instead of half an ulp adds 3.5 eps |x| / 2 < 7 more: 16 covers both.
N_COMPOSED_GELU = 16
UNFUSED = ("new_gelu", "fast_gelu")

_fixtures = {}


def fixture(dt_name):
    if dt_name not in _fixtures:
        _fixtures[dt_name] = Fixture(dt_name)
    return _fixtures[dt_name]


def must_be_fused(case, dtype):
    """where tests/test_gpu_act_cast.py requires the one-launch kernel to answer"""
    epl = 4 if dtype == torch.float32 else 8
    cols = case.shape[-1]
    if case.family in UNFUSED:
        return False
    if case.family == "softmax":           # the last dim only; rows of at most 1024 lane-vectors are register resident
        return case.kwargs["dim"] == -1 and cols <= 1024 * epl
    if case.family in ("layernorm", "rmsnorm"):
        return cols % 4 == 0 and cols <= 8 * 256 * epl
    return True


def run_case(dmx, oracle, device, fx, case, config):
    """this repo's module of `case` under `config` on the fixture's input: everything the test asserts and the report prints"""
    dtype = fx.dtype
    x = case_input(case, dtype)
    assert sha256_bits(x) == fx.sha256(case), "the regenerated input is not the one the reference ran on"
    m = build_module(dmx.nn, case, dtype, device)
    if config == "basic":
        _basic(dmx, m)
    fo = m.output_casts.output_cast.format if config == "basic" else None
    with torch.no_grad():
        got = m(x.to(device))
        fused = m._fused_forward(x.to(device)) is not None
    cast = cpu_cast(oracle, config)
    cin = cast(x)
    fam = case.family
    floor = None
    if fam == "softmax":
        n = _row_n_ulp("softmax", dtype, fo)
    elif fam in ("layernorm", "rmsnorm"):
        n = _row_n_ulp(fam, dtype, fo)
        if fam == "layernorm":
            floor = _ln_truth(cin, case.args[0], None if m.weight is None else m.weight.detach().cpu(), None if m.bias is None else m.bias.detach().cpu(), m.eps)[1]
    elif fam in UNFUSED:
        n, floor = N_COMPOSED_GELU, cin.double().abs() / 2
    else:
        _, floor_fn, tol = UNARY[fam]
        n, floor = _n_ulp(tol, dtype, fo), None if floor_fn is None else floor_fn(cin)
    return dict(m=m, got=got, fused=fused, cast=cast, cin=cin, n=n, floor=floor, d_ref=fx.d_ref(fam, config), y=fx.y(case, config),
                centre=fx.centre(case, config), defect=fx.defect(case, config))


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
@pytest.mark.parametrize("dt_name", sorted(DTYPES))
def test_module_forward_against_the_reference(dmx, cuda, oracle, dt_name, case, config):
    fx = fixture(dt_name)
    dtype = fx.dtype
    r = run_case(dmx, oracle, cuda, fx, case, config)
    m, got = r["m"], r["got"]
    assert r["fused"] == must_be_fused(case, dtype), ("fused path", r["fused"])
    assert got.dtype == r["y"].dtype and tuple(got.shape) == tuple(r["y"].shape)
    # the module's effective parameters are the reference's
    assert getattr(m, "eps", None) == fx.eps(case, config) and getattr(m, "dim", None) == fx.dim(case, config)
    differ, worst, above, below = distance_to(got, r["y"], dtype, r["floor"])
    print(f"{case.name} {dt_name} {config}: {differ} of {got.numel()} elements differ from the reference's forward, largest distance {worst:.2f} ulp "
          f"({above} above, {below} below); N = {r['n']}, d_ref = {r['d_ref']:.3f}")
    if case.family == "gelu_tanh":
        # the reference evaluates erf for this constructor (tests/test_approx_modules_host.py::test_reference_gelu_ignores_approximate_tanh
        # records it); this repo evaluates torch's tanh form: the float64 tanh form under the existing contract
        f64, _, _ = UNARY["gelu_tanh"]
        truth = f64(r["cin"], dtype)
        want_nan = torch.isnan(r["cast"](truth.to(dtype)))
        assert torch.equal(torch.isnan(got).cpu(), want_nan)
        assert outside_cast_bracket(got, truth, r["cast"], dtype, r["n"], r["floor"]) == 0
        return
    want_nan = torch.isnan(r["cast"](r["centre"].to(dtype)))
    assert torch.equal(want_nan[~r["defect"]], torch.isnan(r["y"])[~r["defect"]])
    assert torch.equal(torch.isnan(got).cpu(), want_nan), "NaN exactly where the reference's forward is NaN"
    bad = outside_cast_bracket(got, r["centre"], r["cast"], dtype, r["n"] + r["d_ref"], r["floor"])
    assert bad == 0, (case.name, dt_name, config, bad, r["n"], r["d_ref"])
