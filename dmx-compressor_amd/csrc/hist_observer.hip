// csrc/hist_observer.hip — the HistogramObserver on the device (numerical/observer.py:213-583, and its twin in
// dmx-compressor_amd/observer.py, whose host code is the specification):
//   * dmxq_hist_observe   one observation of G groups: the groups' min / max (dmxq_group_minmax), a zeroing of the count scratch,
//                         ONE grouped histc launch and ONE plan-and-merge launch -- four launches whatever G is (five while a stream
//                         is captured: the min / max reduction then initialises with a fill launch of its own);
//   * dmxq_hist_qparams   the L2 range search of every group and its (scale, zero_point), ONE launch.
// Nothing is read back to the host and nothing is allocated: the state (histogram, running range, a sticky non-finite flag) and the
// scratch are the caller's, so both entry points can be captured into a graph and replayed.
//
// Bit-exactness with the host code, piece by piece:
//   plan     the branch (re-initialise / add / re-bin), the relaxed upper end, `down` and `start` are the host's fp32 tensor
//            expressions, evaluated op by op (the library is built with -ffp-contract=off); the histc range is the extremum
//            truncated toward zero (Python's int()), or the data's own range when both ends truncate to the same integer;
//   histc    dmxq_histc's bin rule (reduce_common.hpp hist_add), counts per group in LDS, one global atomic per non-empty bin;
//   re-bin   the fp64 running sum of torch.cumsum over the fine cells, in index order, on one lane -- only the bins * upsample_rate
//            non-zero cells are visited, so `down` costs nothing; a run of equal cells is added in one step when every partial sum
//            of the run is exactly representable (then the result cannot differ from the sequential one);
//   search   the quantile walk of _search_range with its l / r pointers moving one way; cumsum as torch's CPU cumsum computes it (a
//            double running sum, each prefix rounded to fp32); every move's error evaluated over the workgroup with the host's fp32
//            per-bin terms.  The two sums the host leaves to ATen's vectorised reductions -- torch.sum(hist) and err.sum() -- have no
//            defined order there; here both are fp64 sums rounded once to fp32 (total: in index order; err: per-thread strided,
//            then a fixed butterfly and the waves in order).
#include <math.h>

#include "common.hpp"
#include "reduce_common.hpp"

namespace dmxq {
namespace {

constexpr int kMergeThreads = 256;
constexpr int kSearchThreads = 256;

enum { kModeSkip = 0, kModeInit = 1, kModeAdd = 2, kModeRebin = 3 };
enum { kErrNone = 0, kErrOverflow = 1, kErrNan = 2 };   // what int() raises on the host: OverflowError (inf), ValueError (nan)

struct HistPlan {
  int mode, err;
  float lo, hi;        // the new running range
  float hl, hh;        // the histc range
  int64_t down, start;
};

// observer.py HistogramObserver.forward, the scalar part: nmin / nmax this observation's extrema, omin / omax the running range
__device__ HistPlan hist_plan(float nmin, float nmax, float omin, float omax, int64_t bins, int64_t up) {
  HistPlan p{kModeSkip, kErrNone, 0.0f, 0.0f, 0.0f, 0.0f, 1, 0};
  if (isnan(nmin) || isnan(nmax)) { p.err = kErrNan; return p; }
  if (isinf(nmin) || isinf(nmax)) { p.err = kErrOverflow; return p; }
  float lo, hi;
  if ((omin == INFINITY && omax == -INFINITY) || omin == omax) {
    p.mode = kModeInit;
    lo = nmin;
    hi = nmax;
  } else {
    lo = omin < nmin ? omin : nmin;   // torch.min(new_min, old_min): the first operand when equal
    hi = nmax < omax ? omax : nmax;   // torch.max(new_max, old_max)
    const float fine = (omax - omin) / (float)(bins * up);
    const float bf = (float)bins * fine;
    const float q = ceilf((hi - lo) / bf);
    // int(ceil(...)): nan / inf raise on the host; a ratio whose fine grid has more than 2^62 cells could not be allocated there
    if (isnan(q)) { p.err = kErrNan; return p; }
    if (!(q >= 1.0f && q * (float)bins <= 4.0e18f)) { p.err = kErrOverflow; return p; }   // (q >= up whenever the range is finite)
    p.down = (int64_t)q;
    hi = hi + (q * bf - (hi - lo));
    if (isinf(hi)) { p.err = kErrOverflow; return p; }
    p.start = (int64_t)rintf((omin - lo) / fine);   // torch.round: half to even
    p.mode = (lo == omin && hi == omax) ? kModeAdd : kModeRebin;
  }
  p.lo = lo;
  p.hi = hi;
  // ops.histc(x, bins, int(lo), int(hi)) and _front.histc's "lo == hi: the data's own range, widened by one if constant"
  float hl = truncf(lo) + 0.0f, hh = truncf(hi) + 0.0f;   // (+ 0: int() has no negative zero)
  if (hl == hh) {
    hl = nmin;
    hh = nmax;
    if (hl == hh) { hl = (float)((double)nmin - 1.0); hh = (float)((double)nmax + 1.0); }
  }
  p.hl = hl;
  p.hh = hh;
  return p;
}

// ------------------------------------------------------------------------------------------------ grouped histc
// grid = G * splits workgroups; workgroup b counts split b % splits of group b / splits into LDS and flushes with one atomic per
// non-empty bin.  Group g is `outer` runs of len = min(gs, C - g*gs) * inner elements at (o*C + g*gs) * inner (dmxq_group_minmax's
// view).  VEC: every run starts 16-byte aligned and is a whole number of 8-element vectors.
template <int DT, bool VEC, bool FAST>
__device__ __forceinline__ void hist_count_body(const void* __restrict__ in, int64_t outer, int64_t C, int64_t inner, int64_t c0,
                                                int64_t len, uint32_t* s_hist, float lo, float hi, int bins, uint32_t splits,
                                                uint32_t sp) {
  const float fb = (float)bins;
  const Recip width = make_recip(hi - lo);
  const int64_t stride = (int64_t)splits * kHistThreads;
  const int64_t t0 = (int64_t)sp * kHistThreads + threadIdx.x;
  if (VEC) {
    constexpr int U = 4;  // 16-byte loads in flight per lane
    const int64_t vl = len / 8, nv = outer * vl;
    const bool narrow = nv < (1ll << 32);
    auto at = [&](int64_t t) -> int64_t {
      if (outer == 1) return c0 * inner + t * 8;
      const int64_t o = narrow ? (int64_t)((uint32_t)t / (uint32_t)vl) : t / vl;
      return (o * C + c0) * inner + (t - o * vl) * 8;
    };
    for (int64_t t = t0; t < nv; t += U * stride) {
      Raw8<DT> raw[U];
#pragma unroll
      for (int u = 0; u < U; u++) raw[u] = load8_raw<DT>(in, at(t + u * stride < nv ? t + u * stride : t));
#pragma unroll
      for (int u = 0; u < U; u++) {
        if (u == 0 || t + u * stride < nv) {
          float a[8];
          widen8<DT>(raw[u], a);
#pragma unroll
          for (int k = 0; k < 8; k++) hist_add<FAST>(s_hist, a[k], lo, hi, fb, width, bins);
        }
      }
    }
  } else {
    const int64_t n = outer * len;
    for (int64_t e = t0; e < n; e += stride) {
      const int64_t o = e / len;
      hist_add<FAST>(s_hist, load_rt(in, DT, (o * C + c0) * inner + (e - o * len)), lo, hi, fb, width, bins);
    }
  }
}

template <int DT, bool VEC>
__global__ __launch_bounds__(kHistThreads) void hist_count_kernel(const void* __restrict__ in, int64_t outer, int64_t C, int64_t inner,
                                                                  int64_t gs, int64_t G, int bins, int64_t up, const float* __restrict__ mm,
                                                                  const float* __restrict__ min_val, const float* __restrict__ max_val,
                                                                  uint32_t* __restrict__ counts, uint32_t splits) {
  extern __shared__ uint32_t s_hist[];
  __shared__ float s_lo, s_hi;
  __shared__ int s_on;
  const int64_t g = blockIdx.x / splits;
  const uint32_t sp = blockIdx.x - (uint32_t)g * splits;
  if (threadIdx.x == 0) {
    const HistPlan p = hist_plan(mm[g], mm[G + g], min_val[g], max_val[g], bins, up);
    s_lo = p.hl;
    s_hi = p.hh;
    s_on = p.mode != kModeSkip && p.hl < p.hh && !isinf(p.hl) && !isinf(p.hh);
  }
  for (int b = threadIdx.x; b < bins; b += kHistThreads) s_hist[b] = 0;
  __syncthreads();
  if (!s_on) return;   // (block-uniform)
  const float lo = s_lo, hi = s_hi;
  const int64_t c0 = g * gs, len = ((C - c0 < gs) ? (C - c0) : gs) * inner;
  if (recip_ok(hi - lo)) hist_count_body<DT, VEC, true>(in, outer, C, inner, c0, len, s_hist, lo, hi, bins, splits, sp);
  else hist_count_body<DT, VEC, false>(in, outer, C, inner, c0, len, s_hist, lo, hi, bins, splits, sp);
  __syncthreads();
  uint32_t* out = counts + g * bins;
  for (int b = threadIdx.x; b < bins; b += kHistThreads) {
    const uint32_t c = s_hist[b];
    if (c) atomicAdd(&out[b], c);
  }
}

// ------------------------------------------------------------------------------------------------ plan and merge
// exponent of the lowest set bit of a finite non-zero double
__device__ __forceinline__ int lsb_exp(double x) {
  const uint64_t b = (uint64_t)__double_as_longlong(x);
  const int ef = (int)((b >> 52) & 0x7FF);
  uint64_t m = b & 0xFFFFFFFFFFFFFull;
  if (ef) m |= 1ull << 52;
  return (ef ? ef : 1) - 1075 + __builtin_ctzll(m);
}
// S + v + v + ... (k times), each sum rounded to double, as torch.cumsum(dtype=torch.double) adds the k equal cells of one old bin.
// Two cases take one step: |v| below a quarter of S's ulp (no sum changes S: the small tail bins of a wide histogram), and S, v
// multiples of 2^e with |S| + k|v| < 2^53 * 2^e (every partial sum is exact: one multiply-add).  Anything else adds k times.
__device__ __forceinline__ double add_run(double S, double v, int64_t k) {
  if (v == 0.0 || k <= 0) return S;
  if (S != 0.0 && fabs(v) < ldexp(1.0, ilogb(S) - 54)) return S;
  int e = lsb_exp(v);
  if (S != 0.0) e = min(e, lsb_exp(S));
  if (fabs(ldexp(S, -e)) + (double)k * fabs(ldexp(v, -e)) < 0x1p53) return S + (double)k * v;
  for (int64_t t = 0; t < k; t++) S += v;
  return S;
}

// observer.py _rebin_onto on one lane: old bin i covers the fine cells [start + i*up, + up), new bin j the cells [j*down, + down);
// inc[j] = fp32((upto[j] - fp32(upto[j-1])) / up) with upto[j] the fp64 running sum up to the end of new bin j.  Cells past
// bins * down are dropped (the host's slice assignment fails there instead).
__device__ void rebin_walk(const float* old, float* inc, int bins, int64_t up, int64_t down, int64_t start) {
  const int64_t ncell = (int64_t)bins * down;
  const double dup = (double)up;
  double S = 0.0;
  float prev = 0.0f;
  int64_t j = 0, nb = down;   // the next new bin and the cell where it ends
  auto emit = [&]() {
    inc[j] = (float)((S - (double)prev) / dup);
    prev = (float)S;
    j++;
    nb += down;
  };
  for (int i = 0; i < bins; i++) {
    int64_t c = start + (int64_t)i * up;
    if (c >= ncell) break;
    const int64_t c1 = c + up < ncell ? c + up : ncell;
    while (nb <= c) emit();
    const double v = (double)old[i];
    while (c < c1) {
      const int64_t e = nb < c1 ? nb : c1;
      S = add_run(S, v, e - c);
      c = e;
      if (e == nb) emit();
    }
  }
  while (j < bins) emit();
}

// one workgroup per group: the plan, then re-initialise (hist = counts), add (counts + hist) or re-bin (counts + the old histogram
// spread onto the new grid), and the new running range; a non-finite observation leaves the group's state alone and raises the
// observer's sticky flag (the largest code wins: nan over inf)
__global__ __launch_bounds__(kMergeThreads) void hist_merge_kernel(const float* __restrict__ mm, int64_t G, int bins, int64_t up,
                                                                   const uint32_t* __restrict__ counts, float* __restrict__ hist,
                                                                   float* __restrict__ min_val, float* __restrict__ max_val, int* status) {
  extern __shared__ float s_old[];
  __shared__ HistPlan s_p;
  const int64_t g = blockIdx.x;
  if (threadIdx.x == 0) s_p = hist_plan(mm[g], mm[G + g], min_val[g], max_val[g], bins, up);
  __syncthreads();
  const HistPlan p = s_p;
  if (p.mode == kModeSkip) {
    if (threadIdx.x == 0) atomicMax(status, p.err);
    return;
  }
  float* h = hist + g * bins;
  const uint32_t* cnt = counts + g * bins;
  if (p.mode == kModeInit) {
    for (int b = threadIdx.x; b < bins; b += kMergeThreads) h[b] = (float)cnt[b];
  } else if (p.mode == kModeAdd) {
    for (int b = threadIdx.x; b < bins; b += kMergeThreads) h[b] = (float)cnt[b] + h[b];
  } else {
    for (int b = threadIdx.x; b < bins; b += kMergeThreads) s_old[b] = h[b];
    __syncthreads();
    if (threadIdx.x == 0) rebin_walk(s_old, h, bins, up, p.down, p.start);   // the increments, over the old values (now in LDS)
    __syncthreads();
    for (int b = threadIdx.x; b < bins; b += kMergeThreads) h[b] = (float)cnt[b] + h[b];
  }
  if (threadIdx.x == 0) {
    min_val[g] = p.lo;
    max_val[g] = p.hi;
  }
}

// ------------------------------------------------------------------------------------------------ range search
// c10::div_floor_floating: torch.div(a, b, rounding_mode="floor") on the CPU
__device__ __forceinline__ float div_floor(float a, float b) {
  if (b == 0.0f) return a / b;
  const float mod = fmodf(a, b);
  float div = (a - mod) / b;
  if (mod != 0.0f && ((b < 0.0f) != (mod < 0.0f))) div -= 1.0f;
  if (div == 0.0f) return copysignf(0.0f, a / b);
  float fl = floorf(div);
  if (div - fl > 0.5f) fl += 1.0f;
  return fl;
}
__device__ __forceinline__ float clamp_level(float v, float top) { return fminf(fmaxf(v, 0.0f), top); }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// one workgroup per group; every thread runs the same walk (same values, same branches), each move's error is summed over the
// workgroup.  hist: the state in global memory (read by the error passes through the cache); csum in LDS.
__global__ __launch_bounds__(kSearchThreads) void hist_search_kernel(const float* __restrict__ hist, const float* __restrict__ min_val,
                                                                     const float* __restrict__ max_val, int bins, int levels, int qmin, int qmax,
                                                                     int sym, float* __restrict__ scale, int64_t* __restrict__ zp) {
  extern __shared__ float s_cs[];
  __shared__ double s_part[2][kSearchThreads / kWave];
  __shared__ double s_total;
  const int64_t g = blockIdx.x;
  const float mn = min_val[g], mx = max_val[g];
  if (mn == INFINITY && mx == -INFINITY) {   // nothing observed (observer.py:66-69); block-uniform
    if (threadIdx.x == 0) { scale[g] = 1.0f; zp[g] = 0; }
    return;
  }
  const float* h = hist + g * bins;
  for (int b = threadIdx.x; b < bins; b += kSearchThreads) s_cs[b] = h[b];
  __syncthreads();
  if (threadIdx.x == 0) {   // torch.cumsum on the CPU: a double running sum, each prefix stored as fp32
    double acc = 0.0;
#pragma unroll 8
    for (int b = 0; b < bins; b++) {
      acc += (double)s_cs[b];
      s_cs[b] = (float)acc;
    }
    s_total = (double)(float)acc;   // torch.sum(hist).item(): fp64 in index order, rounded once
  }
  __syncthreads();
  const double total = s_total;
  const double lo_d = (double)mn, hi_d = (double)mx;
  const double width = (hi_d - lo_d) / (double)bins;
  const float top = (float)(levels - 1);
  const int w = threadIdx.x / kWave;
  int parity = 0;
  // _clip_error(hist, min_val, max_val, first, last) (observer.py:277-329): fp32 per-bin terms, the scalars width and step as doubles
  auto clip_error = [&](int first, int last) -> double {
    const double step = width * (double)(last - first + 1) / (double)levels;
    if (step == 0.0) return 0.0;
    const float wf = (float)width, sf = (float)step, s2 = (float)(step / 2), ns2 = (float)(-step / 2);
    const float b3 = (s2 * s2) * s2, na3 = (ns2 * ns2) * ns2;
    const float mid = (b3 - na3) / 3.0f;
    double acc = 0.0;
    for (int i = threadIdx.x; i < bins; i += kSearchThreads) {
      const float begin = (float)(i - first) * wf;
      const float end = begin + wf;
      const float lb = clamp_level(div_floor(begin, sf), top), le = clamp_level(div_floor(end, sf), top);
      const float density = h[i] / wf;
      const float a = begin - (lb + 0.5f) * sf;
      const float b = end - (le * sf + s2);
      float e = 0.0f;
      e += density * ((b3 - (a * a) * a) / 3.0f);
      e += ((le - lb) - 1.0f) * (density * mid);
      e += density * (((b * b) * b - na3) / 3.0f);
      acc += (double)e;
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & (kWave - 1)) == 0) s_part[parity][w] = acc;
    __syncthreads();
    double sum = 0.0;
#pragma unroll
    for (int k = 0; k < kSearchThreads / kWave; k++) sum += s_part[parity][k];
    parity ^= 1;   // (two buffers: the next write cannot overtake a read of this one, a barrier lies between)
    return (double)(float)sum;
  };
  // _search_range (observer.py:331-397)
  const double qstep = 1e-5;
  double lo_q = 0.0, hi_q = 1.0, best = INFINITY;
  int first = 0, last = bins - 1;
  int pl = 0, pr = bins;                       // searchsorted(left) of the lower threshold, searchsorted(right) of the upper
  float cl = s_cs[0], cr = s_cs[bins - 1];     // s_cs[pl], s_cs[pr - 1]
  while (lo_q < hi_q) {
    const double nlo = lo_q + qstep, nhi = hi_q - qstep;
    const float tl = (float)(nlo * total), tr = (float)(nhi * total);
    while (pl < bins && cl < tl) { pl++; cl = pl < bins ? s_cs[pl] : 0.0f; }
    while (pr > 0 && cr > tr) { pr--; cr = pr > 0 ? s_cs[pr - 1] : 0.0f; }
    const int l = min(last, max(first, pl));
    const int r = max(first, min(last, pr - 1));
    int nfirst = first, nlast = last;
    if ((l - first) > (last - r)) { nfirst = l; lo_q = nlo; }
    else { nlast = r; hi_q = nhi; }
    if (nfirst == first && nlast == last) continue;
    const double err = clip_error(nfirst, nlast);
    if (err > best) break;
    best = err;
    first = nfirst;
    last = nlast;
  }
  if (threadIdx.x == 0) {
    const float wd = (mx - mn) / (float)bins;
    qparams_one(mn + wd * (float)first, mn + wd * (float)(last + 1), qmin, qmax, sym, scale[g], zp[g]);
  }
}

}  // namespace
}  // namespace dmxq

using namespace dmxq;

extern "C" int dmxq_hist_observe(const void* in, int dtype_in, int64_t outer, int64_t C, int64_t inner, int64_t group_size, int64_t bins,
                                 int64_t upsample_rate, float* hist, float* min_val, float* max_val, int* status, void* scratch,
                                 int64_t scratch_bytes, void* stream) {
  if (!valid_dtype(dtype_in) || outer < 0 || C < 0 || inner < 0 || group_size < 1 || bins < 1 || upsample_rate < 1 || scratch_bytes < 0)
    return DMXQ_ERR_BAD_ARG;
  if (bins > kHistMaxBins || upsample_rate > (1 << 20)) return DMXQ_ERR_UNSUPPORTED;
  if (outer == 0 || C == 0 || inner == 0) return DMXQ_OK;   // an empty observation changes nothing (observer.py:461-462)
  if (!in || !hist || !min_val || !max_val || !status || !scratch) return DMXQ_ERR_BAD_ARG;
  const int64_t G = (C + group_size - 1) / group_size;
  if (G > 65535) return DMXQ_ERR_UNSUPPORTED;
  if (scratch_bytes < (2 * G + G * bins) * 4) return DMXQ_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  uint32_t* counts = (uint32_t*)scratch;            // [G, bins] (first: its zeroing starts where the caller's allocation is aligned)
  float* mm = (float*)(counts + G * bins);          // [2, G]: this observation's minima, maxima
  const int rc = dmxq_group_minmax(in, dtype_in, outer, C, inner, group_size, mm, mm + G, stream);
  if (rc != DMXQ_OK) return rc;
  launch_pre();
  if (hipMemsetAsync(counts, 0, (size_t)(G * bins) * sizeof(uint32_t), s) != hipSuccess) {
    (void)launch_status();
    return DMXQ_ERR_LAUNCH;
  }
  // ~256 workgroups of 16 waves over all groups, ~32 elements per lane (dmxq_histc's geometry for one group)
  const int64_t per_group = outer * group_size * inner;
  int64_t splits = (per_group + kHistThreads * 32 - 1) / (kHistThreads * 32);
  const int64_t cap = (256 + G - 1) / G;
  if (splits > cap) splits = cap;
  if (splits < 1) splits = 1;
  const bool vec = aligned16(in) && (group_size * inner) % 8 == 0 && (C * inner) % 8 == 0;
  const size_t lds = (size_t)bins * sizeof(uint32_t);
#define DMXQ_HO(D_, V_) DMXQ_LAUNCH((hist_count_kernel<D_, V_>), dim3((unsigned)(G * splits)), dim3(kHistThreads), lds, s, in, outer, C, inner, group_size, G, (int)bins, upsample_rate, (const float*)mm, (const float*)min_val, (const float*)max_val, counts, (uint32_t)splits)
#define DMXQ_HOD(D_) do { if (vec) DMXQ_HO(D_, true); else DMXQ_HO(D_, false); } while (0)
  if (dtype_in == DMXQ_F32) DMXQ_HOD(DMXQ_F32); else if (dtype_in == DMXQ_F16) DMXQ_HOD(DMXQ_F16); else DMXQ_HOD(DMXQ_BF16);
#undef DMXQ_HOD
#undef DMXQ_HO
  DMXQ_LAUNCH(hist_merge_kernel, dim3((unsigned)G), dim3(kMergeThreads), (size_t)bins * sizeof(float), s, (const float*)mm, G, (int)bins,
              upsample_rate, (const uint32_t*)counts, hist, min_val, max_val, status);
  return launch_status();
}

extern "C" int dmxq_hist_qparams(const float* hist, const float* min_val, const float* max_val, int64_t n_groups, int64_t bins, int precision,
                                 int qmin, int qmax, int symmetric_qscheme, float* scale, int64_t* zero_point, void* stream) {
  if (n_groups < 0 || bins < 1 || precision < 1 || precision > 24 || qmax <= qmin) return DMXQ_ERR_BAD_ARG;
  if (bins > kHistMaxBins) return DMXQ_ERR_UNSUPPORTED;
  if (n_groups == 0) return DMXQ_OK;
  if (!hist || !min_val || !max_val || !scale || !zero_point) return DMXQ_ERR_BAD_ARG;
  if (n_groups > 0x7FFFFFFF) return DMXQ_ERR_UNSUPPORTED;
  DMXQ_LAUNCH(hist_search_kernel, dim3((unsigned)n_groups), dim3(kSearchThreads), (size_t)bins * sizeof(float), (hipStream_t)stream, hist,
              min_val, max_val, (int)bins, 1 << precision, qmin, qmax, symmetric_qscheme, scale, zero_point);
  return launch_status();
}
