"""GPTQ (optimal brain compression) of one Linear / Conv2d DmxModule (reference: layer_reconstruction.py:233-327).

`measure_hessian` accumulates H = 2/n * X X^T on the device (fp32, `addmm_`), with the reference's sample count and running rescale.
`apply` factorises H (torch: cholesky -> cholesky_inverse -> upper cholesky), then walks the weight's columns in blocks: the in-block
column loop is ONE launch of csrc/gptq.hip per block when the weight cast is a format that kernel covers (ops.gptq_block), the
trailing update W[:, i2:] -= E @ Hinv[i1:i2, i2:] a GEMM; any other format runs the reference-shaped loop (the module's own
`weight_hypernet` on each slice, torch linear algebra) on the GPU.
"""
import math

import torch
import torch.nn.functional as F

from ._lib import DmxqError

__all__ = ["OptimalBrainCompressor"]


class OptimalBrainCompressor:
    H = None

    def __init__(self, module):
        self.module = module
        self.example_counter = 0

    def measure_hessian(self, inp):
        """layer_reconstruction.py:240-264, in fp32 on the input's device.  The sample count is the batch (inp.shape[0] after a 2-D
        input is unsqueezed), not the token count, as in the reference."""
        if inp.dim() == 2:
            inp = inp.unsqueeze(0)
        tmp = inp.shape[0]
        m = self.module
        if isinstance(m, torch.nn.Linear):
            if inp.dim() == 3:
                inp = inp.reshape((-1, inp.shape[-1]))
            inp = inp.t()
        if isinstance(m, torch.nn.Conv2d):
            inp = F.unfold(inp, m.kernel_size, dilation=m.dilation, padding=m.padding, stride=m.stride)
            inp = inp.permute([1, 0, 2]).flatten(1)
        inp = inp.float()
        if self.H is None:
            self.H = torch.zeros(inp.shape[0], inp.shape[0], dtype=torch.float32, device=inp.device)
        self.H *= self.example_counter / (self.example_counter + tmp)
        self.example_counter += tmp
        inp = math.sqrt(2 / self.example_counter) * inp
        self.H.addmm_(inp, inp.t())

    # ------------------------------------------------------------------------------------------------ apply
    def _check(self, microblock_size, block_size):
        m = self.module
        assert block_size % microblock_size == 0
        sp = m.weight_sparsifier
        if sp is not None and getattr(sp.sparseness, "blocked", False):
            assert microblock_size % sp.sparseness.block_size == 0
        if m.weight_cast.format.blocked:
            assert microblock_size % m.weight_cast.format.block_size == 0
        from .sparse import Dense
        if sp is not None and not isinstance(sp.sparseness, Dense):
            raise DmxqError("GPTQ with a weight sparsifier is not supported (the reference's slices do not broadcast against its mask)")
        sq = m.smoothquant
        if sq is not None and sq._flag("enabled") and not sq._flag("fused_to_weight"):
            raise DmxqError("GPTQ with SmoothQuant enabled and not fused to the weight is not supported (the reference's slices do not "
                            "broadcast against its scale)")

    def _fused_fields(self):
        """dmxq_gptq_format fields when the kernel reproduces this module's weight cast of a slice, else None"""
        from . import ops
        from .format import FixedPoint, Same
        m = self.module
        if not getattr(m, "fuse_gptq", True):
            return None
        wc, st = m.weight_cast, m.weight_storage_cast
        if st is not None and not (isinstance(st.format, Same) and not st.pre_transform):
            return None
        if wc.pre_transform or wc.dynamic is not None or not wc._flag("fake_quant_enabled") or wc._flag("observer_enabled"):
            return None   # (a dynamic cast: its scale buffers are not what it casts with)
        per_row = False
        if isinstance(wc.format, FixedPoint):
            if wc.group_size:
                return None
            if wc.is_per_channel:
                if wc.ch_axis % 2 != 0 or wc.scale.numel() != m.weight.shape[0]:   # (the slices are [rows, m]: channels are the rows)
                    return None
                per_row = True
            elif wc.scale.numel() != 1:
                return None
        elif wc.block_dim % 2 != 1:   # BFP blocks along the slice's columns
            return None
        return ops.gptq_fields(wc.format, per_row)

    def apply(self, microblock_size=1, block_size=128, percdamp=0.01):
        self._check(microblock_size, block_size)
        m = self.module
        weight = m.weight
        W = weight.data.clone()
        if isinstance(m, torch.nn.Conv2d):
            W = W.flatten(1)
        W = W.float()
        ncols = W.shape[1]
        H = self.H.to(weight.device)
        self.H = None
        dead = torch.diag(H) == 0
        H[dead, dead] = 1
        W[:, dead] = 0
        Q = torch.zeros_like(W)
        damp = percdamp * torch.mean(torch.diag(H))
        diag = torch.arange(ncols, device=H.device)
        H[diag, diag] += damp
        H = torch.linalg.cholesky(H)
        H = torch.cholesky_inverse(H)
        Hinv = torch.linalg.cholesky(H, upper=True).contiguous()   # (LAPACK hands back column-major strides; the kernel reads rows)

        fields = self._fused_fields() if block_size <= 128 else None
        if fields is not None:
            done = self._fused(W, Q, Hinv, microblock_size, block_size, fields)
            if not done:
                fields = None
        if fields is None:
            self._loop(W, Q, Hinv, microblock_size, block_size)
        with torch.no_grad():
            weight.copy_(Q.reshape(weight.shape).to(weight.dtype))

    @staticmethod
    def _inv_diag(Hinv, mb):
        """the inverses of ALL diagonal microblocks of Hinv, as one batched inverse once the factorisation is done: [ceil(ncols / mb),
        mb, mb], a ragged last microblock padded with the identity (microblock 1: 1 / diagonal, [ncols]).  block_size % mb == 0, so the
        microblocks of a column block are a contiguous run of these."""
        ncols = Hinv.shape[0]
        if mb == 1:
            return (1.0 / torch.diagonal(Hinv)).contiguous()
        nmb = -(-ncols // mb)
        pad = nmb * mb - ncols
        P = Hinv
        if pad:
            P = F.pad(Hinv, (0, pad, 0, pad))
            idx = torch.arange(ncols, ncols + pad, device=P.device)
            P[idx, idx] = 1.0
        blocks = P.view(nmb, mb, nmb, mb).diagonal(dim1=0, dim2=2).permute(2, 0, 1)   # [nmb, mb, mb]: the diagonal microblocks
        return torch.linalg.inv(blocks).contiguous()

    def _fused(self, W, Q, Hinv, mb, block_size, fields):
        from . import ops
        wc = self.module.weight_cast
        sc = zp = None
        if fields[0] == 2:
            sc = wc.scale.detach().float().contiguous()
            zp = wc.zero_point.detach().to(torch.int64).contiguous()
        ncols = W.shape[1]
        invd = self._inv_diag(Hinv, mb)
        E = torch.empty(W.shape[0], min(block_size, ncols), dtype=torch.float32, device=W.device)
        for i1 in range(0, ncols, block_size):
            i2 = min(i1 + block_size, ncols)
            count = i2 - i1
            e = E[:, :count]
            d = invd[i1:i2] if mb == 1 else invd[i1 // mb:-(-i2 // mb)]
            try:
                ops.gptq_block(W[:, i1:i2], Hinv[i1:i2, i1:i2], d, Q[:, i1:i2], e, mb, fields, sc, zp)
            except NotImplementedError:
                if i1 == 0:
                    return False   # (a microblock / format the kernel does not take: nothing done yet, the loop runs instead)
                raise
            if i2 < ncols:
                W[:, i2:].addmm_(e, Hinv[i1:i2, i2:], alpha=-1)
        return True

    def _loop(self, W, Q, Hinv, mb, block_size):
        """layer_reconstruction.py:296-318 as written, on the GPU"""
        hyper = self.module.weight_hypernet
        ncols = W.shape[1]
        for i1 in range(0, ncols, block_size):
            i2 = min(i1 + block_size, ncols)
            count = i2 - i1
            _W = W[:, i1:i2].clone()
            _Q = torch.zeros_like(_W)
            _E = torch.zeros_like(_W)
            _Hinv = Hinv[i1:i2, i1:i2]
            for j1 in range(0, count, mb):
                j2 = min(j1 + mb, count)
                w = _W[:, j1:j2]
                q = hyper(w)
                err = (w - q).matmul(torch.linalg.inv(_Hinv[j1:j2, j1:j2]))
                _Q[:, j1:j2] = q
                _W[:, j2:] -= err.matmul(_Hinv[j1:j2, j2:])
                _E[:, j1:j2] = err
            Q[:, i1:i2] = _Q
            W[:, i2:] -= _E.matmul(Hinv[i1:i2, i2:])
