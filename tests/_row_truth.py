"""Float64 truths and tolerances of the row functions (softmax, layer_norm, rms_norm), shared by tests/test_gpu_sparse_calib_approx.py,
tests/test_gpu_act_cast.py and tests/test_gpu_row_classes.py.  The numbers are stated once, here."""
import torch

F = torch.nn.functional

# (tests/_data.py err_in_ulps; measured maxima for the kernels AND for torch's own CPU result, which is what the reference
# evaluates, are in profiles/r02_accuracy_table.txt):
#   16-bit outputs: 1 ulp everywhere ("within 1 ULP of the stated format");
#   fp32 outputs: gelu 2 (erf / tanh + 3 products), softmax 8 (expf <= 1, a row sum of up to 16k fp32 terms, one division;
#   the argument x - max is compensated -- torch's CPU softmax measures 7-24 on the same inputs), layer_norm 3 (two row
#   reductions, rsqrt, fma).  gelu and layer_norm are counted against the magnitude of their CANCELLING terms.
#   EXTENT of softmax's 8: it was measured on random rows, where the roundings of the row sum behave like a random walk.  A row of
#   thousands of EQUAL terms rounds the same way at every addition of a lane's serial partial sum, and the error grows with the count:
#   the planted rows of tests/test_gpu_row_classes.py under input_clamp = -1 (one spike, every other element lifted to -1) measured
#   9 ulps on rows of 2564 elements (wave kernel, 12 vectors per lane) and 12 ulps on rows of 16385 (global fallback, 64 terms per
#   thread).  The 8 is therefore no bound for nearly uniform long rows; 16-bit outputs stay within 1 ulp there as well.
TOL = {"gelu": {torch.float32: 2.0}, "softmax": {torch.float32: 8.0}, "layernorm": {torch.float32: 3.0}}


def tol(op, dtype):
    return TOL[op].get(dtype, 1.0)


# softmax / layer_norm / rms_norm between two casts: the float32 tolerances of the unfused functions; only softmax uses the v_exp / v_rcp
# forms, so only softmax is granted the 64 fp32 ulps behind a narrow output cast
ROW_TOL = {"softmax": {torch.float32: 8}, "layernorm": {torch.float32: 3}, "rmsnorm": {torch.float32: 4}}


def n_ulp(table, dtype, fo):
    n = table.get(dtype, 1)
    if dtype == torch.float32 and fo is not None and fo.mantissa <= 16:
        n = 64  # v_exp / v_rcp forms behind an output cast of <= 16 mantissa bits (csrc/act_cast.hip)
    return n


def row_n_ulp(kind, dtype, fo):
    return n_ulp(ROW_TOL[kind], dtype, fo if kind == "softmax" else None)


def ln_truth(x, cols, w, b, eps=1e-5):
    xd = x.double()
    truth = F.layer_norm(xd, (cols,), None if w is None else w.double(), None if b is None else b.double(), eps)
    # cancelling terms of y = (x - mean) rstd w + b: the row mean is a sum of terms of the row's magnitude, so its rounding
    # error -- and with it the error of every (x - mean) -- is relative to max|x| of the ROW, not to the element
    mu, rstd = xd.mean(-1, keepdim=True), (xd.var(-1, unbiased=False, keepdim=True) + eps).rsqrt()
    floor = (xd.abs().amax(-1, keepdim=True) + mu.abs()) * rstd * (1.0 if w is None else w.double().abs()) + (0.0 if b is None else b.double().abs())
    return truth, floor


def rms_truth(c, cols, w, eps):
    xd = c.double()
    y = xd * (xd.pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    return y if w is None else y * w.double()


def cpu_cast(oracle, f):
    """CastTo.forward on the CPU through the oracle: dtype -> same dtype"""
    if f is None:
        return lambda x: x.clone()
    return lambda x: oracle.floating_point_cast(x, f.mantissa, f.exponent, f.bias, f.flush_subnormal).to(x.dtype)


def cpu_cast_canonical_nan(oracle, f):
    """cpu_cast with every NaN cast as the canonical quiet NaN is.  torch's CPU conversion float16 -> float32 turns a NaN in the scalar
    tail of a tensor (numel % 8 elements) into the all-ones pattern 0x7FFFFFFF, which the reference's bit arithmetic -- and so the
    oracle -- rounds up through exponent and sign to -0.0, while the same NaN in the vectorised body (0x7FC00000) saturates to the
    format's largest value: what a NaN becomes would depend on where in the tensor it sits.  The kernels saturate every NaN."""
    cast = cpu_cast(oracle, f)
    if f is None:
        return cast

    def g(x):
        y, nan = cast(x), torch.isnan(x)
        if bool(nan.any()):
            y = torch.where(nan, cast(torch.full((16,), float("nan"), dtype=x.dtype))[0], y)
        return y

    return g
