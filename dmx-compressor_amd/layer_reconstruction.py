"""GPTQ (optimal brain compression) of one Linear / Conv2d DmxModule (reference: layer_reconstruction.py:233-327).

`measure_hessian` accumulates H = 2/n * X X^T on the device (fp32, `addmm_`), with the reference's sample count and running rescale.
`apply` factorises H (torch: cholesky -> cholesky_inverse -> upper cholesky), then walks the weight's columns in blocks: the in-block
column loop is ONE launch of csrc/gptq.hip per block when the weight cast is a format that kernel covers (ops.gptq_block), the
trailing update W[:, i2:] -= E @ Hinv[i1:i2, i2:] a GEMM; any other format runs the reference-shaped loop (the module's own
`weight_hypernet` on each slice, torch linear algebra) on the GPU.

Not in the reference ("GPTQ with dynamic scales and activation order"):
  * a DYNAMIC integer weight cast (`weight_dynamic`): per_group g takes the scale of every group of g input columns inside the column
    loop, from the row's current, already error-compensated values -- one csrc/gptq_dynamic.hip launch per block
    (ops.gptq_block_dynamic), or the torch loop `_loop_dynamic` with the same definition; per_token / per_tensor take their scale once
    from W and run the static kernel.  apply() then records the scales in `module.gptq_qparams` and switches the weight cast's
    fake quantisation off (see apply);
  * `act_order`: the columns are visited in order of decreasing diag(H).
"""
import math

import torch
import torch.nn.functional as F

from ._lib import DmxqError

__all__ = ["OptimalBrainCompressor", "WandaCalibrator", "AWQCalibrator", "AWQClipCalibrator", "hqq_apply", "AdaRoundCalibrator"]


def refuse_scaled_weight_cast(module):
    """GPTQ on a module whose weight cast is a scaled float cast (CastTo.set_scaling) is not supported: NotImplementedError"""
    wc = getattr(module, "weight_cast", None)
    if wc is not None and wc._scaling is not None:
        raise NotImplementedError(f"GPTQ with a scaled float weight cast (weight_scaling = {wc.scaling!r}) is not supported: a segment's "
                                  "scale would move with every compensated column; clear the setting (set_scaling(None)) or use a "
                                  "dynamic integer cast (weight_dynamic)")


def refuse_vq_weight_cast(module, what):
    """GPTQ, AWQ, the AWQ clip, Wanda, HQQ, AdaRound and folding on a module whose weight cast is a vector codebook cast (CastTo.set_vq):
    NotImplementedError"""
    wc = getattr(module, "weight_cast", None)
    if wc is not None and wc._vq is not None:
        raise NotImplementedError(f"{what} with a vector codebook weight cast (weight_vq = {wc._vq_repr()}) is not supported yet: these "
                                  "procedures assume the format's own scalar grid; clear the setting (set_vq(None)) first")


def refuse_codebook_weight_cast(module, what):
    """GPTQ, AWQ, Wanda and folding on a module whose weight cast is a codebook cast (CastTo.set_codebook): NotImplementedError"""
    wc = getattr(module, "weight_cast", None)
    if wc is not None and wc._codebook is not None:
        raise NotImplementedError(f"{what} with a codebook weight cast (weight_codebook = {wc._codebook_repr()}) is not supported yet: these "
                                  "procedures assume the format's own grid; clear the setting (set_codebook(None)) first")


def refuse_learnable_weight_cast(module, what):
    """GPTQ, AWQ, Wanda and folding on a module whose weight cast has learned scales (CastTo.set_learnable): NotImplementedError"""
    wc = getattr(module, "weight_cast", None)
    if wc is not None and wc._learnable is not None:
        raise NotImplementedError(f"{what} with a learnable weight cast (weight_learnable = {wc.learnable!r}) is not supported: the scales "
                                  "are parameters that training moves, not values a calibration may assume; clear the setting "
                                  "(set_learnable(None)) first")


def refuse_outlier_weight_cast(module, what):
    """GPTQ, AWQ and HQQ on a module whose dynamic weight cast keeps outliers (CastTo.set_dynamic with "outliers"): NotImplementedError"""
    wc = getattr(module, "weight_cast", None)
    if wc is not None and wc._outliers is not None:
        raise NotImplementedError(f"{what} with an outlier-aware weight cast (weight_dynamic = {wc.dynamic!r}) is not supported: it would "
                                  "reproduce the cast without its outliers; clear the outliers (set_dynamic without \"outliers\") first")


class OptimalBrainCompressor:
    H = None

    def __init__(self, module):
        refuse_learnable_weight_cast(module, "GPTQ")
        refuse_codebook_weight_cast(module, "GPTQ")
        refuse_vq_weight_cast(module, "GPTQ")
        refuse_outlier_weight_cast(module, "GPTQ")
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

    def _dynamic_plan(self, block_size):
        """None when the weight cast casts with stored scales (or not at all); (granularity, group_size) for a dynamic integer weight
        cast, after the checks of what GPTQ supports with one.  No GPU involved, nothing modified."""
        from .format import FixedPoint, Same
        m = self.module
        wc = m.weight_cast
        if wc is None or wc._dynamic is None or not isinstance(wc.format, FixedPoint):
            return None
        if not wc._flag("fake_quant_enabled") or wc._flag("observer_enabled"):
            return None   # (the cast does not run dynamically in this state: cast.py _quantize)
        gran, g = wc._dynamic
        if not isinstance(m, torch.nn.Linear) or m.weight.dim() != 2:
            raise DmxqError(f"GPTQ with a dynamic weight cast ({wc.dynamic!r}) supports Linear modules with a 2-D weight only: on a "
                            f"{type(m).__name__} weight of shape {tuple(m.weight.shape)} the segments of the cast are not runs of GPTQ's columns")
        if wc.pre_transform:
            raise DmxqError(f"GPTQ with a dynamic weight cast ({wc.dynamic!r}) and a pre_transform {sorted(wc.pre_transform)} is not supported")
        st = m.weight_storage_cast
        if st is not None and not (isinstance(st.format, Same) and not st.pre_transform):
            raise DmxqError(f"GPTQ with a dynamic weight cast ({wc.dynamic!r}) needs a weight_storage_cast of SAME")
        if wc.format.rounding != "nearest":
            raise DmxqError(f"GPTQ with a dynamic weight cast ({wc.dynamic!r}) needs nearest rounding, got {wc.format!r}")
        if gran == "per_group":
            ncols = m.weight.shape[1]
            if ncols % g != 0 or block_size % g != 0:
                raise ValueError(f"GPTQ with weight_dynamic per_group {g}: the group size must divide the {ncols} input columns and the "
                                 f"block size {block_size} (groups do not straddle column blocks)")
        return gran, g

    def _check_act_order(self, act_order):
        """activation order permutes the columns: allowed where the cast of a column depends on per-row or per-tensor parameters only"""
        from .format import FixedPoint
        if not isinstance(act_order, bool):
            raise TypeError(f"act_order must be a bool, got {act_order!r}")
        if not act_order:
            return
        wc = self.module.weight_cast
        if wc.pre_transform:
            raise DmxqError(f"GPTQ with act_order and a weight cast pre_transform {sorted(wc.pre_transform)} is not supported: a rotation or a "
                            "shaping of the slice mixes neighbouring input columns, which the permutation tears apart")
        if getattr(wc.format, "blocked", False):
            raise DmxqError(f"GPTQ with act_order and the blocked weight format {wc.format!r} is not supported: its blocks are runs of "
                            "neighbouring input columns, which the permutation tears apart")
        if isinstance(wc.format, FixedPoint) and (wc._dynamic is None or wc._flag("observer_enabled")):
            if wc.group_size:
                raise DmxqError("GPTQ with act_order and static group scales is not supported (the scales would have to follow the columns)")
            if wc.is_per_channel and wc.ch_axis % 2 != 0:
                raise DmxqError("GPTQ with act_order and per-input-channel scales is not supported (the scales would have to follow the columns)")

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
        if wc.pre_transform or wc._codebook is not None or wc._vq is not None or wc.dynamic is not None or wc._scaling is not None or wc._learnable is not None or not wc._flag("fake_quant_enabled") or wc._flag("observer_enabled"):
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

    def apply(self, microblock_size=1, block_size=128, percdamp=0.01, act_order=False):
        """GPTQ of the module's weight, in place.  act_order (not in the reference): after the dead-column fix and before damping the
        columns of W and the rows and columns of H are permuted by perm = argsort(diag(H), descending, stable), everything runs on the
        permuted problem and Q is un-permuted at the end; DmxqError for a blocked format (BFP, MXINT, MXFP, SBFP), for static group
        or per-input-channel scales, whose parameters belong to runs of neighbouring columns, and for a weight cast with a pre_transform.

        A DYNAMIC integer weight cast (weight_dynamic; Linear only, nearest rounding, no pre_transform, storage cast SAME -- DmxqError
        otherwise): per_group g (it divides the column count and block_size, ValueError otherwise) derives each group's scale inside
        the column loop from the row's current values (ops.gptq_block_dynamic per block where g is 16 / 32 / 64 / 128 and a multiple of
        the microblock, `_loop_dynamic` otherwise and with fuse_gptq = False); per_token / per_tensor take theirs once from W after
        the dead columns are zeroed.  SIDE EFFECT for such a cast, and the reason: a dynamic cast is not idempotent on Q -- a group's
        extrema move after its scale was fixed, so re-deriving the scale from Q on the next forward would put Q on ANOTHER grid.
        Therefore apply() (1) records
            module.gptq_qparams = {"scale": float32 [rows, G], "zero_point": int64 [rows, G], "group_size": g or None, "perm": perm or None}
        (G = columns / g groups in PROCESSING order, i.e. groups of permuted columns under act_order; G = 1 and group_size None for
        per_token / per_tensor; a plain attribute, no state_dict key), and (2) switches the weight cast's fake_quant_enabled flag OFF, so
        that forwards use Q as written.  Static casts behave as before: nothing recorded, no switch touched."""
        self._check(microblock_size, block_size)
        refuse_scaled_weight_cast(self.module)
        self._check_act_order(act_order)
        dyn = self._dynamic_plan(block_size)
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
        perm = None
        if act_order:
            perm = torch.argsort(torch.diag(H), descending=True, stable=True)
            W = W[:, perm].contiguous()
            H = H[perm][:, perm].contiguous()
        Q = torch.zeros_like(W)
        damp = percdamp * torch.mean(torch.diag(H))
        diag = torch.arange(ncols, device=H.device)
        H[diag, diag] += damp
        H = torch.linalg.cholesky(H)
        H = torch.cholesky_inverse(H)
        Hinv = torch.linalg.cholesky(H, upper=True).contiguous()   # (LAPACK hands back column-major strides; the kernel reads rows)

        qparams = None
        if dyn is not None:
            qparams = self._dynamic(W, Q, Hinv, microblock_size, block_size, *dyn)
        else:
            fields = self._fused_fields() if block_size <= 128 else None
            if fields is not None:
                done = self._fused(W, Q, Hinv, microblock_size, block_size, fields)
                if not done:
                    fields = None
            if fields is None:
                self._loop(W, Q, Hinv, microblock_size, block_size)
        if perm is not None:
            Qp, Q = Q, torch.empty_like(Q)
            Q[:, perm] = Qp
        with torch.no_grad():
            weight.copy_(Q.reshape(weight.shape).to(weight.dtype))
        if qparams is not None:
            m.gptq_qparams = {"scale": qparams[0], "zero_point": qparams[1], "group_size": dyn[1], "perm": perm}
            m.weight_cast.disable_fake_quant()

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

    def _fused(self, W, Q, Hinv, mb, block_size, fields, sc=None, zp=None):
        """sc / zp: the scales of a FIXED cast when they are not the weight cast's buffers (a dynamic per_token / per_tensor cast)"""
        from . import ops
        wc = self.module.weight_cast
        if fields[0] == 2 and sc is None:
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

    # ------------------------------------------------------------------------------------------------ dynamic integer weight casts
    @staticmethod
    def _segment_qparams(x2, qmin, qmax, sym):
        """(scale float32 [n], zero point int64 [n]) of the rows of the contiguous [n, S] tensor: ops.group_minmax -> ops.qparams, the two
        steps that define the dynamic cast (ops.dynamic_fixed_qdq), in pieces of what one group_minmax call takes"""
        from . import ops
        from ._front import DYNAMIC_CHAIN_PIECE as piece
        out = []
        for i in range(0, x2.shape[0], piece):
            mn, mx = ops.group_minmax(x2[i:i + piece], 0, 1)
            out.append(ops.qparams(mn, mx, qmin, qmax, sym))
        if len(out) == 1:
            return out[0]
        return torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out])

    def _dynamic(self, W, Q, Hinv, mb, block_size, gran, g):
        """the column loop for a dynamic integer weight cast -> (scale [rows, G], zero_point [rows, G]) in processing order"""
        from . import ops
        from .observer import _SYMMETRIC, get_qmin_qmax
        m = self.module
        wc = m.weight_cast
        fmt = wc.format
        qmin, qmax = get_qmin_qmax(fmt)
        sym = wc.qscheme in _SYMMETRIC
        rows, ncols = W.shape
        fuse = getattr(m, "fuse_gptq", True) and block_size <= 128
        if gran != "per_group":
            # one scale per output channel (a weight row is a "token") or for the tensor, taken ONCE from W as GPTQ sees it; the static
            # kernel does the rest
            per_row = gran == "per_token"
            sc, zp = self._segment_qparams(W if per_row else W.reshape(1, -1), qmin, qmax, sym)
            done = False
            if fuse:
                fields = ops.gptq_fields(fmt, per_row)
                done = fields is not None and self._fused(W, Q, Hinv, mb, block_size, fields, sc, zp)
            if not done:
                self._loop_dynamic(W, Q, Hinv, mb, block_size, None, sc, zp, per_row, qmin, qmax, sym)
            return sc.reshape(-1, 1).expand(rows, 1).contiguous(), zp.reshape(-1, 1).expand(rows, 1).contiguous()
        scale = torch.empty(rows, ncols // g, dtype=torch.float32, device=W.device)
        zp = torch.empty(rows, ncols // g, dtype=torch.int64, device=W.device)
        done = False
        if fuse and g % mb == 0 and g in (16, 32, 64, 128):
            done = self._fused_dynamic(W, Q, Hinv, mb, block_size, g, scale, zp, sym)
        if not done:
            self._loop_dynamic(W, Q, Hinv, mb, block_size, g, scale, zp, True, qmin, qmax, sym)
        return scale, zp

    def _fused_dynamic(self, W, Q, Hinv, mb, block_size, g, scale, zp, sym):
        """one ops.gptq_block_dynamic launch per column block; the trailing GEMM as in _fused"""
        from . import ops
        fmt = self.module.weight_cast.format
        ncols = W.shape[1]
        invd = self._inv_diag(Hinv, mb)
        E = torch.empty(W.shape[0], min(block_size, ncols), dtype=torch.float32, device=W.device)
        for i1 in range(0, ncols, block_size):
            i2 = min(i1 + block_size, ncols)
            e = E[:, :i2 - i1]
            d = invd[i1:i2] if mb == 1 else invd[i1 // mb:-(-i2 // mb)]
            try:
                ops.gptq_block_dynamic(W[:, i1:i2], Hinv[i1:i2, i1:i2], d, Q[:, i1:i2], e, scale[:, i1 // g:i2 // g], zp[:, i1 // g:i2 // g],
                                       mb, g, fmt, sym)
            except NotImplementedError:
                if i1 == 0:
                    return False   # (a microblock / format the kernel does not take: nothing done yet, the loop runs instead)
                raise
            if i2 < ncols:
                W[:, i2:].addmm_(e, Hinv[i1:i2, i2:], alpha=-1)
        return True

    def _loop_dynamic(self, W, Q, Hinv, mb, block_size, g, scale, zp, per_row, qmin, qmax, sym):
        """The column loop for a dynamic integer weight cast in torch: the A/B partner of the fused kernels and the route for what they
        do not take.  Same definition AND same arithmetic order as the kernels (csrc/gptq.hip: every product and difference its own
        elementwise op, sums in index order from the first product; the diagonal microblocks inverted by `_inv_diag`; the trailing
        update the same addmm_), so that the two routes derive the same group scales: a scale follows its group's extremum to the last
        bit, and one bit of it moves every element of the group.
        g None: `scale` / `zp` are given ([rows] when per_row, else [1]) and every slice is cast with them.  g: at the start of each
        microblock, every group of g columns that STARTS inside it takes (scale, zp) = qparams(group_minmax(W[:, j:j + g])) of the
        current values, written to scale[:, j // g] / zp[:, j // g]; a column is cast with its group's pair (a microblock wider than a
        group is cast group by group, all with scales from the microblock's start)."""
        from . import ops
        fmt = self.module.weight_cast.format
        ncols = W.shape[1]
        invd = self._inv_diag(Hinv, mb)

        def cast(w, sc, z):
            return ops.fixed_qdq(w.contiguous(), fmt.precision, fmt.fraction, fmt.clamp, fmt.symmetric, fmt.rounding, scale=sc, zero_point=z,
                                 ch_axis=0 if per_row else None)

        for i1 in range(0, ncols, block_size):
            i2 = min(i1 + block_size, ncols)
            count = i2 - i1
            _W = W[:, i1:i2].clone()
            _E = torch.empty_like(_W)
            _Hinv = Hinv[i1:i2, i1:i2]
            for j1 in range(0, count, mb):
                j2 = min(j1 + mb, count)
                n = j2 - j1
                w = _W[:, j1:j2]
                if g is None:
                    q = cast(w, scale, zp)
                else:   # (block_size % g == 0: a group never straddles a block, and i1 is a group start)
                    for s in range(-(-j1 // g) * g, j2, g):
                        sc, z = self._segment_qparams(_W[:, s:s + g].contiguous(), qmin, qmax, sym)
                        scale[:, (i1 + s) // g], zp[:, (i1 + s) // g] = sc, z
                    q = torch.empty_like(w)
                    for s in range(j1 // g * g, j2, g):   # the pieces of the microblock, one per group it touches
                        a, b = max(s, j1), min(s + g, j2)
                        k = (i1 + s) // g
                        q[:, a - j1:b - j1] = cast(_W[:, a:b], scale[:, k].contiguous(), zp[:, k].contiguous())
                d = w - q
                D = invd[i1 + j1].reshape(1, 1) if mb == 1 else invd[(i1 + j1) // mb]
                err = d[:, 0:1] * D[0, :n]
                for i in range(1, n):
                    err = err + d[:, i:i + 1] * D[i, :n]
                Q[:, i1 + j1:i1 + j2] = q
                _E[:, j1:j2] = err
                if j2 < count:
                    acc = err[:, 0:1] * _Hinv[j1, j2:]
                    for i in range(1, n):
                        acc = acc + err[:, i:i + 1] * _Hinv[j1 + i, j2:]
                    _W[:, j2:] -= acc
            if i2 < ncols:
                W[:, i2:].addmm_(_E, Hinv[i1:i2, i2:], alpha=-1)


# ---------------------------------------------------------------------------------------------------- Wanda
def wanda_applies(module) -> bool:
    """Wanda acts on a Linear with a 2-D weight and a weight sparseness other than DENSE; on anything else nothing happens"""
    from .sparse import Dense
    sp = getattr(module, "weight_sparsifier", None)
    return (isinstance(module, torch.nn.Linear) and getattr(module, "weight", None) is not None and module.weight.dim() == 2
            and sp is not None and not isinstance(sp.sparseness, Dense))


def refuse_wanda(module):
    """the configurations Wanda does not support, as a DmxqError before any state is touched"""
    from .sparse import BlockTopK
    sq = module.smoothquant
    if sq is not None and sq._flag("enabled") and not sq._flag("fused_to_weight"):
        raise DmxqError("Wanda with SmoothQuant enabled and not fused to the weight is not supported: the sparsifier sees W, but the GEMM "
                        "sees W * s and x / s; fuse the scale to the weight first (fuse_to_weight) or disable SmoothQuant")
    sp = module.weight_sparsifier.sparseness
    if isinstance(sp, BlockTopK) and sp.block_dim not in (-1, module.weight.dim() - 1):
        raise DmxqError(f"Wanda ranks the groups of {sp!r} along the input channels, the weight's last dimension; block_dim = "
                        f"{sp.block_dim} is not supported")


class WandaCalibrator:
    """Wanda (Sun et al., 2023): while DmxModule.wanda_pruning is active, `observe` adds the per-input-channel sum of
    squares of every forward's input into a float64 [in_features] device vector (one ops.channel_sumsq call, nothing read back) and
    counts the tokens on the host; `apply` turns it into the fp32 norm vector, scores the weight with it and writes the score (and, for
    an N:M sparseness, the mask) into the module's weight sparsifier.  The weight itself is never modified."""

    def __init__(self, module, sumsq=None, n_tokens: int = 0):
        refuse_learnable_weight_cast(module, "Wanda")
        refuse_codebook_weight_cast(module, "Wanda")
        refuse_vq_weight_cast(module, "Wanda")
        self.module = module
        self.sumsq = sumsq
        self.n_tokens = int(n_tokens)

    def observe(self, inp):
        from . import ops
        C = inp.shape[-1]
        if self.sumsq is None or self.sumsq.device != inp.device:
            prev = self.sumsq
            self.sumsq = torch.zeros(C, dtype=torch.float64, device=inp.device)
            if prev is not None:
                self.sumsq += prev.to(inp.device)
        ops.channel_sumsq(inp, out=self.sumsq)
        self.n_tokens += inp.numel() // C if C else 0

    def apply(self):
        from . import ops
        from .sparse import BlockTopK
        m = self.module
        if self.n_tokens == 0:
            raise RuntimeError("Wanda: no calibration token was observed inside wanda_pruning (run at least one forward of the module); "
                               "the score is left as it was")
        sp = m.weight_sparsifier
        w = m.weight.detach()
        act_norm = self.sumsq.to(w.device).sqrt().to(torch.float32)
        if isinstance(sp.sparseness, BlockTopK):
            mask, score = ops.wanda_nm_sparsify(w, act_norm, sp.sparseness.K, sp.sparseness.block_size, return_mask=True, return_score=True,
                                                return_y=False)
        else:   # (global TopK, Bernoulli: the score only; the sparseness' own rule then compares per layer)
            mask, score = None, ops.wanda_score(w, act_norm)
        if sp.score.shape == score.shape and sp.score.device == score.device and sp.score.dtype == score.dtype:
            sp.score.data = score
        else:   # (the lazy sparsifier has not seen the weight yet: allocated as _LazySparsify.forward does)
            sp.score = torch.nn.Parameter(score, requires_grad=True)
        if mask is not None:
            sp.mask = mask
        else:
            sp._mask, sp._mask_pending = None, True   # (read again from the new score)
        m.__dict__.pop("_live_weight", None)   # (a LiveWeightBatch result computed with the old score)
        m.wanda_act_norm, m.wanda_sumsq, m.wanda_n_tokens = act_norm, self.sumsq, self.n_tokens


# ---------------------------------------------------------------------------------------------------- AWQ
def awq_applies(module) -> bool:
    """AWQ acts on a Linear with a 2-D weight, a smoothquant member and a weight cast other than SAME; on anything else nothing happens"""
    from .format import Same
    wc = getattr(module, "weight_cast", None)
    return (isinstance(module, torch.nn.Linear) and getattr(module, "weight", None) is not None and module.weight.dim() == 2
            and getattr(module, "smoothquant", None) is not None and wc is not None and not isinstance(wc.format, Same))


def refuse_awq(module):
    """the configurations AWQ does not support, as a DmxqError before any state is touched"""
    sq = module.smoothquant
    if sq._flag("fused_to_weight"):
        raise DmxqError("AWQ on a module whose SmoothQuant scale has been fused to the weight already is not supported: the search would "
                        "scale an already scaled weight; start from the unfused weight (a fresh module or its original state_dict)")
    if sq._flag("enabled"):
        raise DmxqError("AWQ with SmoothQuant enabled is not supported: the search writes the scale SmoothQuant already holds; disable it "
                        "first (smoothquant.disable()), AWQ enables it again with its own scale")
    if sq._flag("dynamic"):
        raise DmxqError("AWQ with a dynamic SmoothQuant is not supported: every forward would overwrite the searched scale; switch it off "
                        "first (smoothquant.set_dynamic(False))")
    if sq.calibrating:
        raise DmxqError("AWQ inside a SmoothQuant calibration is not supported: both write smoothquant.scale; leave calibrating_smoothquant "
                        "first")
    if sq.process_group is not None:
        raise DmxqError("AWQ on a sharded module (smoothquant.set_process_group) is not supported: the candidates' losses would need an "
                        "all-reduce; run the search on the whole weight, or clear the group (set_process_group(None))")


class AWQCalibrator:
    """AWQ (Lin et al., 2023): while DmxModule.awq_scaling is active, `observe` adds every forward's per-input-channel
    sum of |x| into a float64 [in] device vector (one ops.channel_sumabs call) and folds x^T x into a float32 [in, in] running mean over
    the tokens (one addmm_), counting the tokens on the host -- nothing is read back; `apply` forms the candidate scales from the mean
    magnitudes, measures each candidate's output error with the module's own weight cast (ops.awq_search), and hands the best one to
    the module's SmoothQuant, which carries it from there on.  The weight itself is not modified (unless fuse_to_weight asks for it)."""

    def __init__(self, module, hyperparams, sumabs=None, gram=None, n_tokens: int = 0):
        refuse_learnable_weight_cast(module, "AWQ")
        refuse_codebook_weight_cast(module, "AWQ")
        refuse_vq_weight_cast(module, "AWQ")
        refuse_outlier_weight_cast(module, "AWQ")   # (neither ops.awq_scaled_error nor its chain selects outliers)
        # the clip that follows the fuse: its refusals now, before any state is touched (SmoothQuant's own state is refuse_awq's matter)
        self.clip_plan = refuse_awq_clip(module, after_awq_scaling=True) if hyperparams.clip is not None else None
        self.module = module
        self.hyperparams = hyperparams
        self.sumabs, self.gram = sumabs, gram
        self.n_tokens = int(n_tokens)

    def observe(self, inp):
        from . import ops
        C = inp.shape[-1]
        t = inp.numel() // C if C else 0
        if t == 0:
            return
        if self.sumabs is None or self.sumabs.device != inp.device:
            prev, prev_g = self.sumabs, self.gram
            self.sumabs = torch.zeros(C, dtype=torch.float64, device=inp.device)
            self.gram = torch.zeros(C, C, dtype=torch.float32, device=inp.device)
            if prev is not None:
                self.sumabs += prev.to(inp.device)
                self.gram += prev_g.to(inp.device)
        with torch.no_grad():
            x = inp.detach()
            ops.channel_sumabs(x, out=self.sumabs)
            n = self.n_tokens
            x = x.reshape(-1, C).float() * (1.0 / math.sqrt(n + t))
            self.gram *= n / (n + t)
            with ops._front._full_fp32_matmul():
                self.gram.addmm_(x.t(), x)
        self.n_tokens = n + t

    def _kernel_plan(self):
        """(format, group size, symmetric_qscheme) when a candidate's error is ops.awq_scaled_error by definition of the module's stages --
        a nearest-rounding dynamic per_group integer weight cast that runs as such, without pre_transform, behind a SAME storage cast --
        else None: the stages themselves run"""
        from .cast import _SYMMETRIC
        from .format import FixedPoint, Same
        m = self.module
        wc, st = m.weight_cast, m.weight_storage_cast
        if wc._dynamic is None or wc._dynamic[0] != "per_group" or not isinstance(wc.format, FixedPoint) or wc.format.rounding != "nearest":
            return None
        if not wc._flag("fake_quant_enabled") or wc._flag("observer_enabled") or wc.pre_transform:
            return None
        if st is not None and not (isinstance(st.format, Same) and not st.pre_transform):
            return None
        return wc.format, wc._dynamic[1], wc.qscheme in _SYMMETRIC

    def apply(self):
        from . import ops
        m = self.module
        sq = m.smoothquant
        if self.n_tokens == 0:
            raise RuntimeError("AWQ: no calibration token was observed inside awq_scaling (run at least one forward of the module); "
                               "the scale is left as it was")
        with torch.no_grad():
            E = m.effective_weight.detach()
            E = E if E.is_contiguous() else E.contiguous()
            x_mean = (self.sumabs.to(E.device) / self.n_tokens).to(torch.float32)
            scales = ops.awq_candidate_scales(x_mean, self.hyperparams.n_grid, sq.scale_cast)
            plan = self._kernel_plan()
            if plan is not None and (E.dtype not in (torch.float32, torch.float16, torch.bfloat16) or E.shape[1] % plan[1]):
                plan = None
            if plan is not None:
                fmt, g, sym = plan
                error_fn = lambda k, s: ops.awq_scaled_error(E, s, fmt, g, symmetric_qscheme=sym)
            else:
                E32 = E.float()

                def error_fn(k, s):   # the module's own stages, as weight_hypernet runs them behind the sparsifier
                    wq = ops.scale_channels(E, s, sq.win_ch_axis, False, E.dtype)
                    if m.weight_storage_cast is not None:
                        wq = m.weight_storage_cast(wq)
                    wq = m.weight_cast(wq)
                    return ops.scale_channels(wq, s, sq.win_ch_axis, True, torch.float32) - E32

            losses, best = ops.awq_search(E, self.gram.to(E.device), scales, error_fn)
            sq.scale = scales.index_select(0, best.reshape(1))[0].clone()
        sq.enable(True)
        if self.hyperparams.fuse_to_weight:
            sq.fuse_to_weight(m.weight)
        if self.clip_plan is not None:   # (fuse_to_weight holds: DmxAWQHyperparams): the GEMM now sees x / s, whose second moment is
            with torch.no_grad():        # gram / s / s^T -- two float32 divisions in this order
                s = sq.scale.detach().to(self.gram.device, torch.float32)
                g = self.clip_plan[1]
                blocks = ops.awq_gram_blocks(self.gram / s[:, None] / s[None, :], g)
            awq_clip_apply(m, self.clip_plan, self.hyperparams.clip, blocks, self.n_tokens)
        m.__dict__.pop("_live_weight", None)   # (a LiveWeightBatch result computed without the scale)
        m.awq_losses, m.awq_best, m.awq_x_mean, m.awq_n_tokens = losses, best, x_mean, self.n_tokens
        m.awq_sumabs, m.awq_gram = self.sumabs, self.gram


# ---------------------------------------------------------------------------------------------------- AWQ clipping
def awq_clip_applies(module) -> bool:
    """AWQ clipping acts on a Linear with a 2-D weight; on anything else nothing happens"""
    return isinstance(module, torch.nn.Linear) and getattr(module, "weight", None) is not None and module.weight.dim() == 2


def refuse_awq_clip(module, after_awq_scaling: bool = False):
    """-> (format, group size, symmetric_qscheme) of a module DmxModule.awq_clipping takes, or the refusal as a DmxqError before any state
    is touched.  after_awq_scaling: asked by an awq_scaling context that will fuse its scale and then clip -- SmoothQuant's state and the
    active AWQ context are that context's own"""
    from .cast import _SYMMETRIC
    from .format import FixedPoint, Same
    from .sparse import Dense
    wc, st = module.weight_cast, module.weight_storage_cast
    if wc is None:
        raise DmxqError("AWQ clipping needs a weight cast: the module has none")
    refuse_vq_weight_cast(module, "AWQ clipping")
    for what, setting in (("an outlier-aware", wc._outliers), ("a codebook", wc._codebook), ("a learnable", wc._learnable), ("a scaled float", wc._scaling)):
        if setting is not None:
            raise DmxqError(f"AWQ clipping with {what} weight cast is not supported: the search reproduces the plain per-group dynamic "
                            "integer cast; clear the setting first")
    if wc.pre_transform:
        raise DmxqError(f"AWQ clipping with a weight cast pre_transform {sorted(wc.pre_transform)} is not supported: the clamp would act on "
                        "the weight, the cast on its rotation")
    if st is not None and not (isinstance(st.format, Same) and not st.pre_transform):
        raise DmxqError("AWQ clipping needs a weight_storage_cast of SAME: the clamped weight must reach the weight cast as it is")
    if (wc._dynamic is None or wc._dynamic[0] != "per_group" or not isinstance(wc.format, FixedPoint) or wc.format.rounding != "nearest"
            or not wc._flag("fake_quant_enabled") or wc._flag("observer_enabled")):
        raise DmxqError(f"AWQ clipping needs a weight cast that is a nearest-rounding dynamic per-group integer cast (weight_dynamic = "
                        f"{{'per_group': g}} on XP[p,0](C.N)) and runs as such (fake quantisation on, no observer), got {wc.format!r} with "
                        f"weight_dynamic = {wc.dynamic!r}")
    sp = module.weight_sparsifier
    if sp is not None and not isinstance(sp.sparseness, Dense):
        raise DmxqError(f"AWQ clipping with a weight sparseness {sp.sparseness!r} is not supported: the search casts the dense weight")
    if module.weight.dtype not in (torch.float32, torch.float16, torch.bfloat16) or module.weight.shape[1] % wc._dynamic[1]:
        raise DmxqError(f"AWQ clipping needs a float32, float16 or bfloat16 weight whose {module.weight.shape[1]} columns are a multiple of "
                        f"the group size {wc._dynamic[1]}")
    if module.obc is not None:
        raise DmxqError("AWQ clipping inside optimal_brain_compressing on the same module is not supported: both rewrite the weight")
    if not after_awq_scaling:
        sq = module.smoothquant
        if sq is not None and (sq._flag("enabled") and not sq._flag("fused_to_weight") or sq._flag("dynamic") or sq.calibrating):
            raise DmxqError("AWQ clipping with SmoothQuant enabled and not fused to the weight, dynamic or calibrating is not supported: the "
                            "weight cast sees W * s, not the weight that would be clamped; fuse the scale to the weight or disable it")
        if module.awq is not None:
            raise DmxqError("AWQ clipping inside awq_scaling on the same module is not supported: the scale search would see a moving "
                            "weight; ask for the clip through DmxAWQHyperparams(clip=...) instead")
    return wc.format, wc._dynamic[1], wc.qscheme in _SYMMETRIC


def awq_clip_apply(module, plan, hp, blocks, n_tokens):
    """clip the module's weight in place with ops.awq_clip and record the outcome as plain attributes (no buffer, no state_dict key)"""
    from . import ops
    fmt, g, sym = plan
    ratios = ops.awq_clip_ratios(hp.n_grid, hp.max_shrink)
    w = module.weight.detach()
    y, best, clip = ops.awq_clip(w, blocks.to(w.device), fmt, g, ratios, symmetric_qscheme=sym, return_best=True, return_clip=True)
    with torch.no_grad():
        module.weight.copy_(y)
    module.awq_clip = {"clip": clip, "best": best, "group_size": g, "ratios": ratios}
    module.awq_clip_blocks, module.awq_clip_n_tokens = blocks, n_tokens
    module.__dict__.pop("_live_weight", None)   # (a LiveWeightBatch result computed from the unclipped weight)


class AWQClipCalibrator:
    """AWQ weight clipping (AutoAWQ's clip search; DESIGN.md §8 "AWQ clipping"): while DmxModule.awq_clipping is active, `observe` folds
    the inputs that reach the GEMM into a float32 [G, g, g] running mean over the tokens of the DIAGONAL BLOCKS of x^T x (one baddbmm_,
    AWQCalibrator's formula per block: a 14336-column layer keeps 7 MB at g = 128 instead of the 822 MB of the whole matrix), counting the
    tokens on the host -- nothing is read back; `apply` clips the weight in place with ops.awq_clip.  The weight cast stays dynamic: it
    re-derives its scale from the clamped weight, which is the scale the search used."""

    def __init__(self, module, hyperparams, blocks=None, n_tokens: int = 0):
        self.plan = refuse_awq_clip(module)
        self.module = module
        self.hyperparams = hyperparams
        self.blocks = blocks
        self.n_tokens = int(n_tokens)

    def observe(self, inp):
        from . import ops
        C, g = inp.shape[-1], self.plan[1]
        t = inp.numel() // C if C else 0
        if t == 0:
            return
        if self.blocks is None or self.blocks.device != inp.device:
            prev = self.blocks
            self.blocks = torch.zeros(C // g, g, g, dtype=torch.float32, device=inp.device)
            if prev is not None:
                self.blocks += prev.to(inp.device)
        with torch.no_grad():
            n = self.n_tokens
            x = inp.detach().reshape(-1, C).float() * (1.0 / math.sqrt(n + t))
            x = x.reshape(t, C // g, g).transpose(0, 1)   # [G, tokens, g]
            self.blocks *= n / (n + t)
            with ops._front._full_fp32_matmul():
                self.blocks.baddbmm_(x.transpose(1, 2), x)
        self.n_tokens = n + t

    def apply(self):
        if self.n_tokens == 0:
            raise RuntimeError("AWQ clipping: no calibration token was observed inside awq_clipping (run at least one forward of the "
                               "module); the weight is left as it was")
        awq_clip_apply(self.module, self.plan, self.hyperparams, self.blocks, self.n_tokens)


# ---------------------------------------------------------------------------------------------------- HQQ
def refuse_hqq(module):
    """-> (format, the weight cast's own per-group size or None) of a module DmxModule.hqq_quantize takes, or the refusal"""
    from .format import FixedPoint, Same
    from .observer import get_qmin_qmax
    wc, st = module.weight_cast, module.weight_storage_cast
    if wc is None:
        raise DmxqError("HQQ needs a weight cast: the module has none")
    refuse_scaled_weight_cast_for(module, "HQQ")
    refuse_learnable_weight_cast(module, "HQQ")
    refuse_codebook_weight_cast(module, "HQQ")
    refuse_vq_weight_cast(module, "HQQ")
    refuse_outlier_weight_cast(module, "HQQ")
    if wc.pre_transform:
        raise DmxqError(f"HQQ with a weight cast pre_transform {sorted(wc.pre_transform)} is not supported: the zero points would be solved "
                        "for the rotated weight")
    if st is not None and not (isinstance(st.format, Same) and not st.pre_transform):
        raise DmxqError("HQQ needs a weight_storage_cast of SAME: the written weight must reach the GEMM as it is")
    if wc._flag("observer_enabled"):
        raise DmxqError("HQQ while the weight cast's observer is calibrating is not supported: leave calibrating_quantizers first")
    fmt = wc.format
    if not isinstance(fmt, FixedPoint) or get_qmin_qmax(fmt) == (None, None) or fmt.rounding != "nearest":
        raise DmxqError(f"HQQ needs a weight format that is a clamped XP[p,0] with nearest rounding, got {fmt!r}")
    own = wc._dynamic[1] if wc._dynamic is not None and wc._dynamic[0] == "per_group" else None
    return fmt, own


def refuse_scaled_weight_cast_for(module, what):
    wc = getattr(module, "weight_cast", None)
    if wc is not None and wc._scaling is not None:
        raise NotImplementedError(f"{what} with a scaled float weight cast (weight_scaling = {wc.scaling!r}) is not supported: clear the "
                                  "setting (set_scaling(None)) first")


def hqq_apply(module, hp):
    """DmxModule.hqq_quantize's work on a Linear / Conv2d: see there"""
    from . import ops
    fmt, own = refuse_hqq(module)   # (before anything is touched)
    weight = module.weight
    w2 = weight.data.reshape(weight.shape[0], -1)
    g = hp.group_size if hp.group_size is not None else (own if own is not None else 64)
    if w2.shape[1] % g:
        raise ValueError(f"HQQ: the group size {g} must divide the {w2.shape[1]} input columns of the weight")
    y, sc, zero = ops.hqq_qdq(w2, fmt, g, hp.lp_norm, hp.beta, hp.kappa, hp.iters, return_qparams=True)
    with torch.no_grad():
        weight.copy_(y.reshape(weight.shape))
    G = w2.shape[1] // g
    module.hqq_qparams = {"scale": sc.reshape(-1, G), "zero": zero.reshape(-1, G), "group_size": g}
    module.weight_cast.disable_fake_quant()


# ---------------------------------------------------------------------------------------------------- AdaRound
def adaround_applies(module) -> bool:
    """AdaRound acts on a Linear with a 2-D weight; on anything else nothing happens"""
    return isinstance(module, torch.nn.Linear) and getattr(module, "weight", None) is not None and module.weight.dim() == 2


def refuse_adaround(module):
    """-> (format, granularity, group size, dynamic, symmetric_qscheme) of a module DmxModule.adaround_reconstructing takes, or the
    refusal as a DmxqError before any state is touched"""
    from .cast import _SYMMETRIC
    from .format import FixedPoint, Same
    from .observer import get_qmin_qmax
    from .sparse import Dense
    wc, st = module.weight_cast, module.weight_storage_cast
    if wc is None:
        raise DmxqError("AdaRound needs a weight cast: the module has none")
    refuse_vq_weight_cast(module, "AdaRound")
    for what, setting in (("an outlier-aware", wc._outliers), ("a codebook", wc._codebook), ("a learnable", wc._learnable), ("a scaled float", wc._scaling)):
        if setting is not None:
            raise DmxqError(f"AdaRound with {what} weight cast is not supported: it rounds on the grid of a plain integer cast; clear the "
                            "setting first")
    if wc.pre_transform:
        raise DmxqError(f"AdaRound with a weight cast pre_transform {sorted(wc.pre_transform)} is not supported: the grid would be the "
                        "rotated weight's")
    if st is not None and not (isinstance(st.format, Same) and not st.pre_transform):
        raise DmxqError("AdaRound needs a weight_storage_cast of SAME: the written weight must reach the weight cast as it is")
    sp = module.weight_sparsifier
    if sp is not None and not isinstance(sp.sparseness, Dense):
        raise DmxqError(f"AdaRound with a weight sparseness {sp.sparseness!r} is not supported: it rounds the dense weight")
    sq = module.smoothquant
    if sq is not None and sq._flag("enabled") and not sq._flag("fused_to_weight"):
        raise DmxqError("AdaRound with SmoothQuant enabled and not fused to the weight is not supported: the weight cast sees W * s, not "
                        "the weight that would be rounded; fuse the scale to the weight or disable it")
    for name, ctx in (("optimal_brain_compressing", module.obc), ("awq_scaling", module.awq), ("awq_clipping", module.awq_clipper)):
        if ctx is not None:
            raise DmxqError(f"AdaRound inside {name} on the same module is not supported: both rewrite what the weight cast sees")
    if wc._flag("observer_enabled"):
        raise DmxqError("AdaRound while the weight cast's observer is calibrating is not supported: leave calibrating_quantizers first")
    fmt = wc.format
    if not isinstance(fmt, FixedPoint) or get_qmin_qmax(fmt) == (None, None) or fmt.rounding != "nearest":
        raise DmxqError(f"AdaRound needs a weight format that is a clamped XP[p,0] with nearest rounding, got {fmt!r}")
    if not wc._flag("fake_quant_enabled"):
        raise DmxqError("AdaRound needs a weight cast that runs: its fake quantisation is switched off")
    w = module.weight
    if w.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise DmxqError(f"AdaRound needs a float32, float16 or bfloat16 weight, got {w.dtype}")
    sym = wc.qscheme in _SYMMETRIC
    if wc._dynamic is not None:
        gran, g = wc._dynamic
        if gran == "per_group" and w.shape[1] % g:
            raise DmxqError(f"AdaRound: the group size {g} of weight_dynamic does not divide the weight's {w.shape[1]} columns")
        return fmt, gran, g, True, sym
    if wc.group_size:
        raise DmxqError(f"AdaRound with a static group_size ({wc.group_size}) weight cast is not supported: take weight_dynamic per group, "
                        "or a static per-tensor or per-output-channel cast")
    if wc.is_per_channel:
        if wc.ch_axis % 2 != 0 or wc.scale.numel() != w.shape[0] or wc.zero_point.numel() != w.shape[0]:
            raise DmxqError(f"AdaRound with a static per-channel weight cast needs one calibrated scale per OUTPUT channel (ch_axis 0, "
                            f"{w.shape[0]} entries), got ch_axis {wc.ch_axis} with {wc.scale.numel()} entries")
        return fmt, "per_token", None, False, sym
    if wc.scale.numel() != 1 or wc.zero_point.numel() != 1:
        raise DmxqError(f"AdaRound with a static per-tensor weight cast needs ONE scale, got {wc.scale.numel()}")
    return fmt, "per_tensor", None, False, sym


def adaround_schedule(hp, step: int):
    """(reg_weight, beta) of Adam step `step` of hp.iters: no regulariser during the first int(warmup * iters) steps, then hp.reg_weight
    with beta going from beta[0] to beta[1] by a cosine over the remaining steps"""
    warm = int(hp.warmup * hp.iters)
    if step < warm:
        return 0.0, hp.beta[0]
    rel = (step - warm) / max(1, hp.iters - warm)
    return hp.reg_weight, hp.beta[1] + 0.5 * (hp.beta[0] - hp.beta[1]) * (1.0 + math.cos(math.pi * rel))


class AdaRoundCalibrator:
    """AdaRound (Nagel et al., 2020; DESIGN.md §8 "AdaRound"): while DmxModule.adaround_reconstructing is active, `observe` folds the
    inputs that reach the GEMM into the float32 [in, in] running mean over the tokens of x^T x (AWQCalibrator's formula, one addmm_),
    counting the tokens on the host -- nothing is read back; `apply` learns the rounding of every weight element on the weight cast's own
    grid against that moment and writes the hard-rounded weight in place.  The loop has no sampling: the same calibration gives the same
    bits twice."""

    def __init__(self, module, hyperparams):
        self.plan = refuse_adaround(module)
        self.module = module
        self.hyperparams = hyperparams
        self.gram = None
        self.n_tokens = 0

    def observe(self, inp):
        from . import ops
        C = inp.shape[-1]
        t = inp.numel() // C if C else 0
        if t == 0:
            return
        if self.gram is None or self.gram.device != inp.device:
            prev = self.gram
            self.gram = torch.zeros(C, C, dtype=torch.float32, device=inp.device)
            if prev is not None:
                self.gram += prev.to(inp.device)
        with torch.no_grad():
            n = self.n_tokens
            x = inp.detach().reshape(-1, C).float() * (1.0 / math.sqrt(n + t))
            self.gram *= n / (n + t)
            with ops._front._full_fp32_matmul():
                self.gram.addmm_(x.t(), x)
        self.n_tokens = n + t

    def qparams(self, W):
        """(scale float32 [n_seg], zero point int64 [n_seg]) of the weight cast for the contiguous weight W: a dynamic cast's own two
        steps (group_minmax -> qparams), a static cast's buffers"""
        from .observer import get_qmin_qmax
        fmt, gran, g, dynamic, sym = self.plan
        wc = self.module.weight_cast
        if not dynamic:
            return wc.scale.detach().to(W.device, torch.float32).reshape(-1).contiguous(), wc.zero_point.detach().to(W.device, torch.int64).reshape(-1).contiguous()
        qmin, qmax = get_qmin_qmax(fmt)
        S = {"per_token": W.shape[1], "per_group": g, "per_tensor": W.numel()}[gran]
        sc, zp = OptimalBrainCompressor._segment_qparams(W.reshape(-1, S), qmin, qmax, sym)
        return sc.reshape(-1).float().contiguous(), zp.reshape(-1).to(torch.int64).contiguous()

    def apply(self):
        from . import ops
        m, hp = self.module, self.hyperparams
        if self.n_tokens == 0:
            raise RuntimeError("AdaRound: no calibration token was observed inside adaround_reconstructing (run at least one forward of "
                               "the module); the weight is left as it was")
        fmt, gran, g, dynamic, _ = self.plan
        with torch.no_grad():
            W = m.weight.detach()
            W = W if W.is_contiguous() else W.contiguous()
            out = W.shape[0]
            G = self.gram.to(W.device)
            W32 = W.float()
            sc, zp = self.qparams(W)
            zf = zp.to(torch.float32)

            def loss_of(Wq):
                D = Wq.float() - W32
                with ops._front._full_fp32_matmul():
                    return ((D @ G) * D).sum(dtype=torch.float64) / out

            W_rtn = m.weight_cast(W).to(W.dtype)   # the module's own round-to-nearest cast
            V = ops.adaround_init(W, sc, zp, fmt, gran, g)
            opt = torch.optim.Adam([V], lr=hp.lr)
            for step in range(hp.iters):
                rw, beta = adaround_schedule(hp, step)
                D = ops.adaround_qdq(W, V, sc, zf, fmt, gran, g, out_dtype=torch.float32) - W32
                with ops._front._full_fp32_matmul():
                    gD = (D @ G) * (2.0 / out)   # (the gradient of sum((D G) * D) / out in D: G is symmetric)
                V.grad, _ = ops.adaround_backward(W, V, gD, sc, zf, fmt, gran, g, beta=beta, reg_weight=rw, want_reg=False)
                opt.step()
            W_hard = ops.adaround_qdq(W, V, sc, zf, fmt, gran, g, hard=True)
            loss_rtn, loss_hard = loss_of(W_rtn), loss_of(W_hard)
            if hp.keep_best:
                kept = loss_hard < loss_rtn   # (ties go to round-to-nearest; decided on the device)
                W_new = torch.where(kept, W_hard, W_rtn)
                loss = torch.where(kept, loss_hard, loss_rtn)
            else:
                kept, W_new, loss = torch.ones((), dtype=torch.bool, device=W.device), W_hard, loss_hard
            flipped = (W_new != W_rtn).sum()
            m.weight.copy_(W_new)
        m.adaround = {"loss_rtn": loss_rtn, "loss_hard": loss_hard, "loss": loss, "kept": kept, "flipped": flipped, "scale": sc, "zero_point": zp,
                      "group_size": g if gran == "per_group" else None, "granularity": gran}
        if dynamic:
            m.weight_cast.disable_fake_quant()
        m.__dict__.pop("_live_weight", None)   # (a LiveWeightBatch result computed from the weight before rounding)
