"""CPU restatement of HistogramObserver's host code (dmx-compressor_amd/observer.py: forward, _rebin_onto, _clip_error,
_search_range, calculate_qparams) -- the reference for the device path's tests, as tests/_gptq_ref.py is for GPTQ.

Copied statement by statement; only the two device calls change: `ops.group_minmax` becomes torch.aminmax and `ops.histc` (with
_front.histc's "lo == hi: the data's own range" rule) becomes ATen's CPU torch.histc, which dmxq_histc reproduces bit for bit
(tests/test_golden.py).  Everything runs on float32 CPU tensors.
"""
import torch


def histc(x, bins, lo, hi):
    """_front.histc on the CPU"""
    lo, hi = float(lo), float(hi)
    if lo == hi:
        lo, hi = float(x.min()), float(x.max())
        if lo == hi:
            lo, hi = lo - 1.0, hi + 1.0
    lo, hi = torch.tensor(lo, dtype=torch.float32), torch.tensor(hi, dtype=torch.float32)
    # a range wider than FLT_MAX / bins (far past the 2^63 where the reference's torch.histc refuses the range: DESIGN.md §8): the
    # numerator (x - lo) * bins overflows, ATen's bin is then an out-of-range float -> int64 conversion (undefined; bin 0 on x86-64),
    # dmxq_histc's a saturating one clamped to the last bin -- restated here, so that the copy stays defined
    over = (x >= lo) & (x <= hi) & torch.isinf((x.float() - lo) * float(bins))
    if bool(over.any()):
        h = torch.histc(x[~over], bins, min=lo.item(), max=hi.item())
        h[-1] += over.sum()
        return h
    return torch.histc(x, bins, min=lo.item(), max=hi.item())


def qparams(mn, mx, qmin, qmax, symmetric):
    """observer.py:59-115 _calculate_qparams in fp32 (dmxq_qparams)"""
    mn, mx = torch.as_tensor(mn, dtype=torch.float32).reshape(1), torch.as_tensor(mx, dtype=torch.float32).reshape(1)
    eps = torch.tensor(torch.finfo(torch.float32).eps)
    min_neg, max_pos = torch.minimum(mn, torch.zeros(1)), torch.maximum(mx, torch.zeros(1))
    if symmetric:
        m = torch.maximum(-min_neg, max_pos)
        return torch.maximum(m / (torch.tensor(float(qmax - qmin)) / 2), eps), torch.zeros(1, dtype=torch.int64)
    s = torch.maximum((max_pos - min_neg) / float(qmax - qmin), eps)
    z = torch.clamp(qmin - torch.round(min_neg / s), qmin, qmax)
    return s, z.to(torch.int64)


class HistRef:
    def __init__(self, bins=2048, upsample_rate=128, precision=8, qmin=-128, qmax=127, symmetric=False):
        self.bins, self.upsample_rate, self.precision = bins, upsample_rate, precision
        self.qmin, self.qmax, self.symmetric = qmin, qmax, symmetric
        self.histogram = torch.zeros(bins)
        self.min_val = torch.tensor(float("inf"))
        self.max_val = torch.tensor(float("-inf"))

    def _uninitialised(self):
        return float(self.min_val) == float("inf") and float(self.max_val) == float("-inf")

    def forward(self, x):
        if x.numel() == 0:
            return x
        xd = x.detach().float().cpu()
        new_min, new_max = torch.aminmax(xd)
        old_min, old_max = self.min_val, self.max_val
        if self._uninitialised() or float(old_min) == float(old_max):
            hist = histc(xd, self.bins, int(new_min), int(new_max))
            lo, hi = new_min, new_max
        else:
            lo, hi = torch.min(new_min, old_min), torch.max(new_max, old_max)
            fine = (old_max - old_min) / (self.bins * self.upsample_rate)
            down = int(torch.ceil((hi - lo) / (self.bins * fine)).item())
            hi = hi + (down * (self.bins * fine) - (hi - lo))
            start = int(torch.round((old_min - lo) / fine).item())
            hist = histc(xd, self.bins, int(lo), int(hi))
            old_hist = self.histogram
            if lo == old_min and hi == old_max:
                hist = hist + old_hist
            else:
                hist = self._rebin_onto(hist, old_hist, down, start)
        self.histogram = hist
        self.min_val, self.max_val = lo.clone(), hi.clone()
        return x

    __call__ = forward

    def _rebin_onto(self, hist, old_hist, down, start):
        n, up = self.bins, self.upsample_rate
        cells = torch.zeros(n * down)
        cells[start:n * up + start] = old_hist.repeat_interleave(up)
        upto = torch.cumsum(cells, 0, dtype=torch.double)[down - 1::down]
        before = torch.zeros(n)
        before[1:n] = upto[0:-1]
        return hist + ((upto - before) / up).to(torch.float)

    def _clip_error(self, hist, lo: float, hi: float, first: int, last: int) -> float:
        levels = 2 ** self.precision
        width = (hi - lo) / self.bins
        step = width * (last - first + 1) / levels
        if step == 0.0:
            return 0.0
        cube3 = lambda a, b: (b * b * b - a * a * a) / 3
        begin = (torch.arange(self.bins) - first) * width
        end = begin + width
        lvl_b = torch.clamp(torch.div(begin, step, rounding_mode="floor"), 0, levels - 1)
        lvl_e = torch.clamp(torch.div(end, step, rounding_mode="floor"), 0, levels - 1)
        density = hist / width
        err = torch.zeros(self.bins)
        err += density * cube3(begin - (lvl_b + 0.5) * step, torch.ones(self.bins) * (step / 2))
        err += (lvl_e - lvl_b - 1) * (density * cube3(torch.tensor(-step / 2), torch.tensor(step / 2)))
        err += density * cube3(torch.tensor(-step / 2), end - (lvl_e * step + step / 2))
        return err.sum().item()

    def search_range(self):
        """_search_range; also returns the chosen (first, last)"""
        hist, min_val, max_val = self.histogram, self.min_val, self.max_val
        width = (max_val - min_val) / self.bins
        total = torch.sum(hist).item()
        csum = torch.cumsum(hist, dim=0)
        step, lo_q, hi_q = 1e-5, 0.0, 1.0
        first, last, best = 0, self.bins - 1, float("inf")
        while lo_q < hi_q:
            nlo, nhi = lo_q + step, hi_q - step
            l = int(torch.searchsorted(csum, torch.tensor(nlo * total, dtype=csum.dtype), right=False))
            l = min(last, max(first, l))
            r = int(torch.searchsorted(csum, torch.tensor(nhi * total, dtype=csum.dtype), right=True)) - 1
            r = max(first, min(last, r))
            nfirst, nlast = first, last
            if (l - first) > (last - r):
                nfirst, lo_q = l, nlo
            else:
                nlast, hi_q = r, nhi
            if nfirst == first and nlast == last:
                continue
            err = self._clip_error(hist, min_val.item(), max_val.item(), nfirst, nlast)
            if err > best:
                break
            best, first, last = err, nfirst, nlast
        return min_val + width * first, min_val + width * (last + 1), (first, last)

    def calculate_qparams(self):
        if self._uninitialised():
            return torch.tensor([1.0]), torch.tensor([0])
        lo, hi, _ = self.search_range()
        return qparams(lo, hi, self.qmin, self.qmax, self.symmetric)
