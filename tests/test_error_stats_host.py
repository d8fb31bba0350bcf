"""CPU-side tests of the error measurement (no GPU): argument validation of dmxq_error_stats / dmxq_cast_error before anything is
launched, benchmark.compute_error on CPU tensors and tests/_error_ref.py (the float64 restatement the GPU tests check the kernels
against) against tests/golden/error_stats.npz -- the reference's own compute_error on the seeded cases of _error_ref.py, written by
tools/gen_golden_error.py --, and DmxModule.monitoring."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import _error_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "error_stats.npz")


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLD, allow_pickle=False)
    assert json.loads(str(g["case_table"])) == json.loads(R.case_table_json()), "the fixture was generated from another case table"
    assert list(g["names"]) == list(R.CASES)
    return g


def test_fixture_is_small():
    assert os.path.getsize(GOLD) < 64 * 1024 < os.path.getsize(os.path.join(os.path.dirname(GOLD), "gptq.npz"))


def test_entry_points_validate_without_a_device(dmx):
    L, lib = dmx._lib.lib(), dmx._lib
    null, p = ctypes.c_void_p(None), ctypes.c_void_p(4096)
    big = 1 << 20
    assert L.dmxq_error_scratch_bytes(0, 1) == 32 and L.dmxq_error_scratch_bytes(4096 * 4096, 8) == 2048 * 8 * 32
    assert L.dmxq_error_scratch_bytes(1 << 40, 1) == 2048 * 32   # bounded: the grid is (8 workgroups per CU; without a device, or on an MI355X: 256 CUs)
    # dmxq_error_stats: null pointers and a negative n are unsupported, a dtype outside the enum is a bad argument
    for ref, test, stats, scratch in ((null, p, p, p), (p, null, p, p), (p, p, null, p), (p, p, p, null)):
        assert L.dmxq_error_stats(ref, lib.F32, test, lib.BF16, 64, 0, stats, scratch, big, null) == lib.ERR_UNSUPPORTED
    assert L.dmxq_error_stats(p, lib.F32, p, lib.F32, -1, 0, p, p, big, null) == lib.ERR_UNSUPPORTED
    assert L.dmxq_error_stats(p, 7, p, lib.F32, 64, 0, p, p, big, null) == lib.ERR_BAD_ARG
    assert L.dmxq_error_stats(p, lib.F32, p, 3, 64, 0, p, p, big, null) == lib.ERR_BAD_ARG
    assert L.dmxq_error_stats(p, lib.F32, p, lib.F32, 1 << 20, 0, p, p, 64, null) == lib.ERR_BAD_ARG       # scratch below the query
    assert L.dmxq_error_stats(null, lib.F32, null, lib.F32, 0, 1, p, null, 0, null) == lib.OK               # n == 0 merged into a row: no-op

    def fmts(*fields):
        arr = (lib.GptqFormat * len(fields))(*[lib.GptqFormat(*f) for f in fields])
        return arr, ctypes.cast(arr, ctypes.c_void_p)

    bfp = (lib.GPTQ_BFP, 8, 16, 1, 0, 0, 0, 0, 0, 0, 0, 0)
    fp8 = (lib.GPTQ_FLOAT, 0, 0, 0, 3, 4, 7, 0, 0, 0, 0, 0)
    int8 = (lib.GPTQ_FIXED, 8, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0)

    def call(f, n, in_=p, dtype=lib.BF16, rows=4, L_=128, scale=null, zp=null, stats=p, scratch=p, acc=0):
        return L.dmxq_cast_error(in_, dtype, rows, L_, f, n, scale, zp, acc, stats, scratch, big, null)

    keep, one = fmts(bfp)
    keep9, nine = fmts(*[bfp] * 9)
    assert call(nine, 9) == lib.ERR_UNSUPPORTED                                   # more than 8 formats
    assert call(one, 1, in_=null) == call(one, 1, stats=null) == call(one, 1, scratch=null) == call(null, 1) == lib.ERR_UNSUPPORTED
    assert call(one, 1, rows=-1) == call(one, 1, L_=-8) == lib.ERR_UNSUPPORTED
    assert call(one, 0) == lib.ERR_BAD_ARG and call(one, 1, dtype=5) == lib.ERR_BAD_ARG
    keepk, bad = fmts((7,) + bfp[1:])
    assert call(bad, 1) == lib.ERR_BAD_ARG                                        # a kind outside dmxq_gptq_kind
    keep2, two = fmts(fp8, (9,) + bfp[1:])
    assert call(two, 2) == lib.ERR_BAD_ARG
    # what the fused kernel does not take: nothing launched, the caller runs the cast and dmxq_error_stats
    assert call(one, 1, L_=1500) == lib.ERR_UNSUPPORTED                           # L % 8 != 0
    assert call(one, 1, L_=24) == lib.ERR_UNSUPPORTED                             # ragged blocks
    assert call(one, 1, in_=ctypes.c_void_p(4098)) == lib.ERR_UNSUPPORTED         # misaligned
    for f in ((lib.GPTQ_BFP, 8, 4, 1) + (0,) * 8, (lib.GPTQ_BFP, 8, 256, 1) + (0,) * 8, (lib.GPTQ_BFP, 23, 16, 1) + (0,) * 8,
              (lib.GPTQ_BFP, 1, 16, 1) + (0,) * 8, (lib.GPTQ_FLOAT, 0, 0, 0, 23, 8, 127, 0, 0, 0, 0, 0), int8[:11] + (1,)):
        k, ptr = fmts(f)
        assert call(ptr, 1, L_=256, scale=p, zp=p) == lib.ERR_UNSUPPORTED, f
    # the range checks every user of dmxq_gptq_format shares, each reached through this entry point
    for f in ((lib.GPTQ_FIXED, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0), (lib.GPTQ_FIXED, 25, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0),
              (lib.GPTQ_FLOAT, 0, 0, 0, 3, 0, 7, 0, 0, 0, 0, 0), (lib.GPTQ_FLOAT, 0, 0, 0, 3, 9, 7, 0, 0, 0, 0, 0),
              (lib.GPTQ_FLOAT, 0, 0, 0, -1, 4, 7, 0, 0, 0, 0, 0)):
        k, ptr = fmts(f)
        assert call(ptr, 1, L_=256, scale=p, zp=p) == lib.ERR_UNSUPPORTED, f
    k, ptr = fmts((lib.GPTQ_MXFP, 0, 32, 0, 1, 2, 0, 0, 0, 0, 0, 0))
    assert call(ptr, 1, L_=256) == lib.ERR_BAD_ARG                                # MXFP: refused like any unknown kind
    # a shared range check and a rule of this entry point broken at once: every format's kind is judged first, the format's ranges
    # before the input pointer and before the size of the scratch
    k, ptr = fmts((lib.GPTQ_FLOAT, 0, 0, 0, 23, 8, 127, 0, 0, 0, 0, 0), (9,) + bfp[1:])
    assert call(ptr, 2, L_=256) == lib.ERR_BAD_ARG
    k, ptr = fmts((lib.GPTQ_FLOAT, 0, 0, 0, 23, 8, 127, 0, 0, 0, 0, 0))
    assert L.dmxq_cast_error(p, lib.BF16, 4, 256, ptr, 1, null, null, 0, p, p, 8, null) == lib.ERR_UNSUPPORTED
    k, ptr = fmts(bfp)
    assert L.dmxq_cast_error(p, lib.BF16, 4, 256, ptr, 1, null, null, 0, p, p, 8, null) == lib.ERR_BAD_ARG
    k, ptr = fmts((lib.GPTQ_FIXED, 25, 0, 1, 0, 0, 0, 0, 0, 0, 1, 1))
    assert call(ptr, 1, L_=256, in_=null) == lib.ERR_UNSUPPORTED
    keepi, fixed = fmts(int8)
    assert call(fixed, 1) == lib.ERR_UNSUPPORTED                                  # a fixed point format without its scale / zero point
    assert call(one, 1, rows=0, acc=1) == lib.OK                                  # n == 0 merged into a row: no-op
    del keep, keep9, keepk, keep2, keepi


def test_front_end_refuses_what_it_must(dmx):
    x = torch.zeros(4, 16)
    with pytest.raises(dmx.DmxqError):
        dmx.ops.error_stats(x, x)                                                 # no CPU path
    with pytest.raises(dmx.DmxqError):
        dmx.ops.cast_error(x, ["BFP[8|8]{16}(SN)"])
    from dmx_compressor_amd import _front
    with pytest.raises(NotImplementedError):
        _front._cast_error_entry("BFP[8|8]{16}(SS)")                             # stochastic: not a property of the format alone
    with pytest.raises(NotImplementedError):
        _front._cast_error_entry(("XP[8,0](CSS)", 0.1, 0))
    with pytest.raises(ValueError):
        _front._cast_error_entry(("BFP[8|8]{16}(SN)", 0.1, 0))                    # only fixed point takes a triple
    fmt, scale, zp = _front._cast_error_entry(("XP[8,0](CSN)", 0.5, 3))
    assert repr(fmt) == "XP[8,0](CSN)" and (scale, zp) == (0.5, 3)


@pytest.mark.parametrize("name", list(R.CASES))
def test_compute_error_on_cpu_equals_the_reference(dmx, gold, name):
    """benchmark.compute_error on CPU tensors is the reference's expressions: maxdelta bit for bit; mse bit for bit on the torch build
    that wrote the fixture (ATen leaves the order of its float32 sum open), within the fp32 summation bound elsewhere"""
    a, b = R.build_case(name)
    e = dmx.compute_error(a, b)
    assert set(e) == {"mse", "maxdelta"}
    assert float(e["maxdelta"]) == float(gold[f"{name}_maxdelta"])
    ns = R.compute_error_ref(a, b)["n"]
    if torch.__version__ == str(gold["torch_version"]):
        assert float(e["mse"]) == float(gold[f"{name}_mse"])
    else:
        assert abs(float(e["mse"]) - float(gold[f"{name}_mse"])) <= max(ns + [1]) * 2.0 ** -24 * float(gold[f"{name}_mse"])
    ta, tb = dmx.gather_tensors(a), dmx.gather_tensors(b)
    assert len(ta) == len(tb) == len(ns)
    assert dmx.compute_mse_error(ta, tb) == e["mse"] and dmx.compute_maxdelta_error(ta, tb) == e["maxdelta"]


@pytest.mark.parametrize("name", list(R.CASES))
def test_float64_restatement_agrees_with_the_reference(gold, name):
    """_error_ref.py against the reference's numbers: maxdelta exactly; mse within (n - 1) 2^-24 relative per pair -- the worst case of
    an fp32 sum of n non-negative terms, whatever order ATen chose"""
    a, b = R.build_case(name)
    rows = [R.error_row_ref(x, y) for x, y in zip(R.gather(a), R.gather(b))]
    r = R.compute_error_ref(a, b)
    assert r["maxdelta"] == float(gold[f"{name}_maxdelta"])
    bound = sum((int(row[3]) - 1) * 2.0 ** -24 * float(row[0] / row[3]) for row in rows)
    print(name, "mse", r["mse"], "reference", float(gold[f"{name}_mse"]), "bound", bound)
    assert abs(r["mse"] - float(gold[f"{name}_mse"])) <= bound


def test_monitoring_records_and_removes_its_hook(dmx):
    m = dmx.nn.Linear(8, 4)
    x = torch.arange(16, dtype=torch.float32).reshape(2, 8) / 7
    records = []
    assert len(m._forward_hooks) == 0
    with m.monitoring(records) as mm:
        assert mm is m and len(m._forward_hooks) == 1
        y = m(x)   # (a freshly made module casts nothing: SAME formats, torch's own linear on the CPU)
    assert len(m._forward_hooks) == 0
    assert len(records) == 1 and set(records[0]) == {"input", "output"}
    args, kwargs = records[0]["input"]
    assert isinstance(args, tuple) and args[0] is x and kwargs == {} and records[0]["output"] is y
    m(x)
    assert len(records) == 1
    with pytest.raises(RuntimeError):
        with m.monitoring(records):
            raise RuntimeError("the hook goes with the context, also on an exception")
    assert len(m._forward_hooks) == 0
