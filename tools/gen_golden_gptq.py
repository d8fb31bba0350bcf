"""tests/golden/gptq.npz: the reference's own GPTQ (optimal_brain_compressing, layer_reconstruction.py:70-113, 233-327) on six cases.

Build container only: loads the reference read-only through oracle/ref_shim.py.  What had to be stubbed for its GPTQ to run on the
CPU: the `skopt` module (ref_shim's stand-in; GPTQ never calls it) and `torch.cuda.synchronize` (a no-op here: apply() calls it
unconditionally).  Nothing else of the reference is replaced.

Per case the weight and the three calibration batches are generated from seeds by tests/_data.py `make` (so the GPU test rebuilds the
same module without the reference), and the fixture keeps: the seeds, every 8th row of the reference's H (float32, as it computes it),
its diagonal, the reference's Q (float32), its loss tr((W - Q) H (W - Q)^T) and round-to-nearest's, in float64 with the reference's H,
and the CPU spread between this repo's float32 (kernel order) and float64 restatements of apply() (tests/_gptq_ref.py), from which the
tests derive their tolerances.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import oracle as O  # noqa: E402
import ref_shim  # noqa: E402
from _data import make  # noqa: E402
from _gptq_ref import CASES, apply_ref, case_cast, hessian64, loss  # noqa: E402

torch.cuda.synchronize = lambda *a, **k: None   # the reference's apply() synchronises unconditionally
ref_shim.load_reference()
from dmx.compressor.advanced_recipe import (DmxModuleGPTQHyperparams, DmxModuleQuantizerCalibrationHyperparams,  # noqa: E402
                                            DmxQuantizerCalibrationHyperparams)
from dmx.compressor.layer_reconstruction import OptimalBrainCompressor  # noqa: E402
from dmx.compressor.modeling import nn as rnn  # noqa: E402
from dmx.compressor.numerical.observer import MinMaxObserver  # noqa: E402

_captured = {}
_apply = OptimalBrainCompressor.apply


def _capturing_apply(self, *a, **k):
    _captured["H"] = self.H.detach().clone()
    return _apply(self, *a, **k)


OptimalBrainCompressor.apply = _capturing_apply


def main():
    O.build()
    out = {}
    spreads, shares = [], []
    for name, c in CASES.items():
        kind, fin, fout = c["module"]
        m = rnn.Linear(fin, fout) if kind == "linear" else rnn.Conv2d(fin, fout, 3)
        W0 = make("normal", tuple(m.weight.shape), seed=c["seed"]) * 0.05
        with torch.no_grad():
            m.weight.copy_(W0)
        m.transform({"weight_format": c["format"]})
        xs = [make("normal", c["input"], seed=c["seed"] + 1 + b) for b in range(3)]
        scale = zp = None
        if c.get("calib"):
            hp = DmxModuleQuantizerCalibrationHyperparams(weight=DmxQuantizerCalibrationHyperparams(
                observer_cls=MinMaxObserver, qscheme_to_overload=torch.per_channel_symmetric, ch_axis=0))
            with torch.no_grad(), m.calibrating_quantizers(hp):
                m(xs[0])
            scale, zp = m.weight_cast.scale.detach().clone(), m.weight_cast.zero_point.detach().clone()
        with torch.no_grad():
            rtn = m.weight_hypernet(m.weight.detach().clone()).reshape(W0.shape[0], -1)
        with torch.no_grad(), m.optimal_brain_compressing(DmxModuleGPTQHyperparams(microblock_size=c["mb"], block_size=c["block"])):
            for x in xs:
                m(x)
        H = _captured.pop("H").float()
        Q = m.weight.detach().reshape(W0.shape[0], -1).float()
        W2 = W0.reshape(W0.shape[0], -1)
        # this repo's CPU restatements of apply() on the same inputs: float64 and float32 (kernel order), their loss spread
        H64 = hessian64(kind, xs, m)
        cast = case_cast(O, c, scale, zp)
        Q64 = apply_ref(W2, H64, c["mb"], c["block"], cast, torch.float64)
        Q32 = apply_ref(W2, H, c["mb"], c["block"], cast, torch.float32)   # (float32 all through: the H a float32 pipeline accumulates)
        l64, l32 = loss(W2, Q64, H64), loss(W2, Q32, H64)
        spreads.append(abs(l32 - l64) / l64)
        shares.append(float((Q32 == Q64.float()).float().mean()))
        out[f"{name}_H_rows"] = H[::8].numpy()
        out[f"{name}_H_diag"] = torch.diagonal(H).numpy()
        out[f"{name}_Q"] = Q.numpy()
        out[f"{name}_loss_ref"] = np.float64(loss(W2, Q, H))
        out[f"{name}_loss_rtn"] = np.float64(loss(W2, rtn, H))
        out[f"{name}_seed"] = np.int64(c["seed"])
        if scale is not None:
            out[f"{name}_scale"] = scale.numpy()
            out[f"{name}_zero_point"] = zp.numpy()
        print(f"{name}: loss ref {out[f'{name}_loss_ref']:.6g} rtn {out[f'{name}_loss_rtn']:.6g} | restatement f64 {l64:.6g} f32 {l32:.6g} "
              f"spread {spreads[-1]:.3g} share(Q32 == Q64) {shares[-1]:.4f}", flush=True)
    out["spread_f32_f64"] = np.array(spreads)
    out["share_f32_f64"] = np.array(shares)
    path = os.path.join(ROOT, "tests", "golden", "gptq.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
