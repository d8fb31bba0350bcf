"""GPU tests of the full-row Hadamard rotation (csrc/hadamard_row.hip, ops.hadamard_row, ops.hadamard_row_dynamic_qdq, the
"hadamard_row" key of CastTo.set_pre_transform): the fused kernel, bit for bit, scales and zero points included, against
tests/_hadamard_row_ref.py on the CPU (finite inputs) and against the library's own chain on the GPU (NaN / Inf / zero rows, refusals)."""
import pytest
import torch

import _hadamard_row_ref as R
from _data import bits_equal, make, mismatches_nan_aware

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
INT8, INT4 = "XP[8,0](CSN)", "XP[4,0](CSN)"
# 512: the smallest row, one wave; 2048 / 4096: the wave -> block boundary (16-bit / fp32) and the first strides through LDS; 16384: the
# largest, 64 KiB of LDS; 768 / 1280 / 1792: each factor at its smallest chunk (lanes past the row's end); 14336 = 28 * 512: the one that matters
ROWS_N = [512, 2048, 4096, 16384, 768, 1280, 1792, 14336]


def routes_of(ops):
    return getattr(ops, "_hadamard_row_routes", None) or ops._front._hadamard_row_routes


def fused(ops, fn, *a, **kw):   # fn(..., fused=True), and the host-side route counter says that the kernel ran
    before = dict(routes_of(ops))
    out = fn(*a, fused=True, **kw)
    assert routes_of(ops)["fused"] == before["fused"] + 1 and routes_of(ops)["chain"] == before["chain"]
    return out


@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=["bf16", "f16", "f32"])
@pytest.mark.parametrize("n", ROWS_N)
def test_kernel_against_the_restatement(dmx, cuda, n, dtype):
    """rows 1 and 5 (independent rows: the one-row call is held to the first row of the same reference) x transpose x {rotation only, to the
    input dtype and float32; INT4 / INT8 x symmetric / affine x per token / per group (16 and, where it divides 2^k, 128) x inverse}"""
    ops = dmx.ops
    P = 1 << R.split(n)[1]
    x = make("outlier" if n % 1024 else "normal", (5, n), seed=n, dtype=dtype, block=64)
    xd = x.to(cuda)
    for transpose in (False, True):
        r = R.rotate_ref(x, transpose)
        for rows in (5, 1):
            assert bits_equal(fused(ops, ops.hadamard_row, xd[:rows], transpose=transpose), r[:rows].to(dtype)) == 0
        assert bits_equal(fused(ops, ops.hadamard_row, xd, transpose=transpose, out_dtype=F32), r) == 0
        for fmt, p in ((INT4, 4), (INT8, 8)):
            for qsym in (False, True):
                for g in [None] + [g for g in (16, 128) if P % g == 0]:
                    q, wsc, wzp = R.torch_restatement(r, p, True, g or n, qsym, F32)
                    for inverse in (False, True):
                        want = (R.rotate_ref(q, not transpose) if inverse else q).to(dtype)
                        for rows in (5, 1):
                            y, sc, zp = fused(ops, ops.hadamard_row_dynamic_qdq, xd[:rows], fmt, "per_group" if g else "per_token", g,
                                              inverse=inverse, transpose=transpose, symmetric_qscheme=qsym, return_qparams=True)
                            k = rows * (n // (g or n))
                            assert bits_equal(sc.cpu(), wsc[:k]) == 0 and bits_equal(zp.cpu(), wzp[:k]) == 0, (fmt, qsym, g, inverse, rows)
                            assert bits_equal(y, want[:rows]) == 0, (fmt, qsym, g, inverse, rows, transpose)


def test_special_rows_against_the_chain(dmx, cuda):
    """rows holding a NaN, an Inf and only zeros, beside ordinary ones: the kernel and the chain agree (any NaN matches any NaN), scales
    and zero points included"""
    ops = dmx.ops
    for n, dtype in ((768, BF16), (4096, F32)):
        x = make("normal", (6, n), seed=3, dtype=dtype)
        x[1, 5], x[2, n - 3], x[3] = float("nan"), float("inf"), 0.0
        xd = x.to(cuda)
        assert mismatches_nan_aware(fused(ops, ops.hadamard_row, xd), ops.hadamard_row(xd, fused=False)) == 0
        for g, gs in (("per_token", None), ("per_group", 64)):
            for qsym in (False, True):
                got = fused(ops, ops.hadamard_row_dynamic_qdq, xd, INT4, g, gs, symmetric_qscheme=qsym, return_qparams=True)
                want = ops.hadamard_row_dynamic_qdq(xd, INT4, g, gs, symmetric_qscheme=qsym, return_qparams=True, fused=False)
                assert [mismatches_nan_aware(a, b) for a, b in zip(got, want)] == [0, 0, 0], (n, g, qsym)


def test_in_place_through_the_c_abi(dmx, cuda):
    lib = dmx._lib
    for n, dt, code in ((1792, BF16, lib.BF16), (4096, F32, lib.F32)):
        x = make("outlier", (5, n), seed=23, dtype=dt, block=64)
        want = R.rotate_ref(R.torch_restatement(R.rotate_ref(x), 4, True, n, False, F32)[0], True).to(dt)
        buf = x.to(cuda)
        rc = lib.lib().dmxq_hadamard_row_qdq(lib.ptr(buf), lib.ptr(buf), code, code, 5, n, 0, 1, 4, 2, n, None, None, lib.stream_of(buf))
        assert rc == lib.OK and bits_equal(buf, want) == 0


def test_refused_cases_take_the_chain(dmx, cuda):
    """an unaligned view and a row past the kernel's range: the chain's bits under fused=None, NotImplementedError under fused=True"""
    ops = dmx.ops
    base = make("normal", (2 + 3 * 768,), seed=7, dtype=BF16)
    big = make("normal", (2, 24576), seed=8, dtype=BF16)
    for x, xd in ((base[2:].reshape(3, 768), base.to(cuda)[2:].reshape(3, 768)), (big, big.to(cuda))):
        for call, ref in ((lambda **kw: ops.hadamard_row(xd, **kw), R.rotate_ref(x).to(BF16)),
                          (lambda **kw: ops.hadamard_row_dynamic_qdq(xd, INT8, **kw),
                           R.rotate_ref(R.torch_restatement(R.rotate_ref(x), 8, True, x.shape[-1], False, F32)[0], True).to(BF16))):
            before = dict(routes_of(ops))
            assert bits_equal(call(), ref) == 0
            assert routes_of(ops)["fused"] == before["fused"] and routes_of(ops)["chain"] == before["chain"] + 1
            with pytest.raises(NotImplementedError):
                call(fused=True)


def test_cast_to_with_the_pre_transform(dmx, cuda):
    """CastTo {"hadamard_row": True} + set_dynamic("per_token") is the one-launch op; a static format goes step by step; both survive
    a capture and one replay on new data"""
    ops = dmx.ops
    c = dmx.CastTo(format=INT4).to(cuda)
    c.set_pre_transform({"hadamard_row": True})
    c.set_dynamic("per_token")
    x0, x1 = (make("outlier", (5, 1280), seed=s, dtype=BF16, block=64).to(cuda) for s in (1, 2))
    before = dict(routes_of(ops))
    y = c(x0)
    assert routes_of(ops)["fused"] == before["fused"] + 1 and bits_equal(y, fused(ops, ops.hadamard_row_dynamic_qdq, x0, INT4)) == 0
    step = dmx.CastTo(format="BFP[8|8]{16}(SN)").to(cuda)
    step.set_pre_transform({"hadamard_row": {"inverse": False}})
    want = dmx.Format.from_shorthand("BFP[8|8]{16}(SN)").cast(ops.hadamard_row(x0, out_dtype=F32), -1, out_dtype=BF16)
    assert bits_equal(step(x0), want) == 0
    with pytest.raises(ValueError):
        c(torch.zeros(4, 100, dtype=BF16, device=cuda))
    buf = x0.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = c(buf)
    buf.copy_(x1)
    graph.replay()
    torch.cuda.synchronize()
    assert bits_equal(out, fused(ops, ops.hadamard_row_dynamic_qdq, x1, INT4)) == 0
