// csrc/adaround.hip — the soft cast of learned weight rounding (AdaRound, Nagel et al. 2020) and its backward pass, each in ONE pass over
// memory (include/dmxq.h dmxq_adaround_forward / dmxq_adaround_backward; DESIGN.md §8 "AdaRound").  Not in the reference.  The weight
// stays on the grid of an integer cast with one (scale s, integer zero point zq) per segment; a float32 variable V per element decides
// between rounding down and rounding up.
//
// Definition, per element, every operation ONE fp32 operation in this order (G = -0.1f, ZG = 1.1f - (-0.1f)):
//   v  = w / s                     IEEE division
//   f  = floorf(v)
//   sg = 1 / (1 + expf(-V));   hr = sg * ZG + G
//   h  = hr < 0 ? 0 : (hr > 1 ? 1 : hr)            soft;      h = V >= 0 ? 1 : 0     hard (no transcendental)
//   t  = (f + h) + zq;   q = t < qmin ? qmin : (t > qmax ? qmax : t)
//   y  = (q - zq) * s              rounded once more to dtype_out
// and backward (the gradient of V alone; the weight is frozen), with bm1 = beta - 1 and m2b = -2 * beta formed once in fp32:
//   in01 = 0 < hr && hr < 1;   cell = qmin <= f + zq && f + zq <= qmax - 1
//   dh   = (sg * (1 - sg)) * ZG
//   rec  = (in01 && cell) ? (g * s) * dh : 0
//   t2   = 2 * h - 1;   a = |t2|;   p1 = powf(a, bm1);   r = 1 - p1 * a
//   dreg = in01 ? reg_weight * (((m2b * p1) * sign(t2)) * dh) : 0          (sign(0) = 0)
//   dV   = rec + dreg;   reg = sum (double)r
// p1, r and dreg are formed only where they are used (reg_weight != 0 or reg_out given): with reg_weight == 0, dV = rec.
// NaN / Inf follow from the comparisons, nothing is special-cased: V = +-Inf and any |V| large enough saturate (h = 1 or 0, dh = 0,
// expf overflowing to +Inf gives sg = 0); a NaN V gives a NaN y in soft mode, h = 0 in hard mode, dV = 0 and a NaN reg; a NaN w gives a
// NaN y and rec = 0; an infinite w clamps to qmin / qmax and is no live cell.
// Repeatability: lsq.hip's rule.  No floating-point atomics; a lane adds its own r in index order in fp64, lanes fold by a fixed xor
// butterfly, waves in wave order, the workgroups' partial sums (the caller's scratch) by a second small launch in a fixed order.  The
// grid depends on the shape alone, so the same call twice gives the same bits.
//
// Geometry: both kernels only stream.  A lane's unit is one 16-byte vector of the weight (8 sixteen-bit or 4 fp32 elements) with the
// 16 or 32 bytes of V that go with it; a unit lies inside one segment (S is a whole number of units), so a lane needs one scale and one
// zero point per unit.  The unit's segment is u >> log2(S / unit) where S / unit is a power of two (and for ONE segment, where the shift
// is 63), otherwise u / (S / unit): a 32-bit division below 2^31 elements and a 64-bit one from there on.  Everything else is int64.
#include <math.h>

#include "common.hpp"

namespace dmxq {
namespace {

constexpr int kArThreads = kThreads;
constexpr int kArWaves = kArThreads / kWave;
constexpr int kArBatch = 2;                  // units in flight per lane
constexpr int kArWgPerCu = 8;                // the largest grid: 8 workgroups on every CU (common.hpp plan_cus)
constexpr int64_t kArShare = 8192;           // elements of a workgroup's share before the grid is capped
constexpr float kArG = -0.1f;
constexpr float kArZG = 1.1f - (-0.1f);

// how a unit finds its segment: kShift u >> l2; kDiv32 / kDiv64 u / nv
enum { kArShift = 0, kArDiv32 = 1, kArDiv64 = 2 };

struct ArSeg {
  int64_t nv;   // units per segment
  int l2, how;
  __device__ __forceinline__ int64_t of(int64_t u) const {
    if (how == kArShift) return u >> l2;
    if (how == kArDiv32) return (int64_t)((uint32_t)u / (uint32_t)nv);
    return u / nv;
  }
};

struct ArFmt { float qmin, qmax; };

__device__ __forceinline__ float ar_clampq(float t, const ArFmt& f) { return t < f.qmin ? f.qmin : (t > f.qmax ? f.qmax : t); }

// 16 bytes of the weight dtype, or (W32: float32 beside a 16-bit weight) 32 bytes, as N floats
template <int DT, bool W32, int N>
__device__ __forceinline__ void ar_load(const void* p, int64_t u, float (&x)[N]) {
  if constexpr (DT == DMXQ_F32 || !W32) {
    const u32x4 r = load_raw16<true>(p, u * 16);
    widen<DT, N>(r, x);
  } else {
    const u32x4 r0 = load_raw16<true>(p, u * 32), r1 = load_raw16<true>(p, u * 32 + 16);
#pragma unroll
    for (int j = 0; j < 4; j++) { x[j] = u2f(r0[j]); x[4 + j] = u2f(r1[j]); }
  }
}

template <int DT, bool W32, int N>
__device__ __forceinline__ void ar_store(void* p, int64_t u, const float (&y)[N]) {
  if constexpr (DT == DMXQ_F32 || W32) store_vec<DMXQ_F32, N>(p, u * N, y);
  else store_vec<DT, N>(p, u * N, y);
}

// ------------------------------------------------------------------------------------------------ forward
template <int DT, bool O32>
__global__ __launch_bounds__(kArThreads) void adaround_forward_kernel(const void* __restrict__ win, const float* __restrict__ Vin, void* __restrict__ yo,
                                                                     int64_t nunits, const ArSeg sg, const ArFmt f,
                                                                     const float* __restrict__ scale, const float* __restrict__ zp, int hard) {
  constexpr int N = 16 / Elem<DT>::bytes;
  const int64_t stride = (int64_t)gridDim.x * kArThreads;
  const int64_t u0 = (int64_t)blockIdx.x * kArThreads + threadIdx.x;
  for (int64_t u = u0; u < nunits; u += kArBatch * stride) {
    float w[kArBatch][N], V[kArBatch][N];
#pragma unroll
    for (int b = 0; b < kArBatch; b++) {
      const int64_t uu = u + b * stride < nunits ? u + b * stride : u;   // (a slot past the end re-reads the lane's first unit and stores nothing)
      ar_load<DT, false, N>(win, uu, w[b]);
      ar_load<DT, true, N>(Vin, uu, V[b]);
    }
#pragma unroll
    for (int b = 0; b < kArBatch; b++) {
      if (b == 0 || u + b * stride < nunits) {
        const int64_t uu = u + b * stride;
        const int64_t seg = sg.of(uu);
        const float s = scale[seg], zq = zp[seg];
        float y[N];
#pragma unroll
        for (int j = 0; j < N; j++) {
          const float v = w[b][j] / s;
          const float fl = floorf(v);
          float h;
          if (hard) {
            h = V[b][j] >= 0.0f ? 1.0f : 0.0f;
          } else {
            const float sig = 1.0f / (1.0f + expf(-V[b][j]));
            const float hr = sig * kArZG + kArG;
            h = hr < 0.0f ? 0.0f : (hr > 1.0f ? 1.0f : hr);
          }
          const float q = ar_clampq((fl + h) + zq, f);
          y[j] = (q - zq) * s;
        }
        ar_store<DT, O32, N>(yo, uu, y);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ backward
// the workgroup's sum -> out[0]: butterfly inside a wave, waves in wave order
__device__ __forceinline__ void ar_block_store(double a, double* out, double* sh) {
  for (int o = 1; o < kWave; o <<= 1) a += __shfl_xor(a, o);
  const int w = threadIdx.x / kWave;
  if ((threadIdx.x & (kWave - 1)) == 0) sh[w] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    double p = sh[0];
#pragma unroll
    for (int k = 1; k < kArWaves; k++) p += sh[k];
    out[0] = p;
  }
}

struct ArReg { float bm1, m2b, rw; int on; };   // on: reg_weight != 0 or the sum is wanted

template <int DT, bool G32>
__global__ __launch_bounds__(kArThreads) void adaround_backward_kernel(const void* __restrict__ win, const float* __restrict__ Vin, const void* __restrict__ gin,
                                                                      float* __restrict__ dVo, int64_t nunits, const ArSeg sg, const ArFmt f,
                                                                      const float* __restrict__ scale, const float* __restrict__ zp, const ArReg rg,
                                                                      double* __restrict__ part) {
  constexpr int N = 16 / Elem<DT>::bytes;
  __shared__ double s_red[kArWaves];
  const float qmax1 = f.qmax - 1.0f;
  double acc = 0.0;
  const int64_t stride = (int64_t)gridDim.x * kArThreads;
  const int64_t u0 = (int64_t)blockIdx.x * kArThreads + threadIdx.x;
  for (int64_t u = u0; u < nunits; u += kArBatch * stride) {
    float w[kArBatch][N], V[kArBatch][N], g[kArBatch][N];
#pragma unroll
    for (int b = 0; b < kArBatch; b++) {
      const int64_t uu = u + b * stride < nunits ? u + b * stride : u;
      ar_load<DT, false, N>(win, uu, w[b]);
      ar_load<DT, true, N>(Vin, uu, V[b]);
      ar_load<DT, G32, N>(gin, uu, g[b]);
    }
#pragma unroll
    for (int b = 0; b < kArBatch; b++) {
      if (b == 0 || u + b * stride < nunits) {
        const int64_t uu = u + b * stride;
        const int64_t seg = sg.of(uu);
        const float s = scale[seg], zq = zp[seg];
        float d[N];
#pragma unroll
        for (int j = 0; j < N; j++) {
          const float v = w[b][j] / s;
          const float fz = floorf(v) + zq;
          const bool cell = (f.qmin <= fz) && (fz <= qmax1);
          const float sig = 1.0f / (1.0f + expf(-V[b][j]));
          const float hr = sig * kArZG + kArG;
          const bool in01 = (0.0f < hr) && (hr < 1.0f);
          const float h = hr < 0.0f ? 0.0f : (hr > 1.0f ? 1.0f : hr);
          const float dh = (sig * (1.0f - sig)) * kArZG;
          float dv = (in01 && cell) ? (g[b][j] * s) * dh : 0.0f;
          if (rg.on) {
            const float t2 = 2.0f * h - 1.0f;
            const float a = fabsf(t2);
            const float p1 = powf(a, rg.bm1);
            const float r = 1.0f - p1 * a;
            const float sgn = t2 > 0.0f ? 1.0f : (t2 < 0.0f ? -1.0f : 0.0f);
            const float dreg = in01 ? rg.rw * (((rg.m2b * p1) * sgn) * dh) : 0.0f;
            if (rg.rw != 0.0f) dv = dv + dreg;
            acc += (double)r;
          }
          d[j] = dv;
        }
        store_vec<DMXQ_F32, N>(dVo, uu * N, d);
      }
    }
  }
  if (part) ar_block_store(acc, part + blockIdx.x, s_red);
}

// one workgroup: thread t folds the partial sums t, t + 256, ... in order, then butterfly and waves in order
__global__ __launch_bounds__(kArThreads) void adaround_final_kernel(const double* __restrict__ part, int nwg, double* __restrict__ reg_out) {
  __shared__ double s_red[kArWaves];
  double a = 0.0;
  for (int i = threadIdx.x; i < nwg; i += kArThreads) a += part[i];
  ar_block_store(a, reg_out, s_red);
}

inline int ar_grid(int64_t n) {
  const int64_t g = (n + kArShare - 1) / kArShare;
  const int64_t max_wg = (int64_t)kArWgPerCu * plan_cus();
  return (int)(g < 1 ? 1 : (g > max_wg ? max_wg : g));
}

inline int ar_class(int dtype, int64_t S) {
  const int V = dtype == DMXQ_F32 ? 4 : 8;
  if (S < V || S % V != 0) return DMXQ_ADAROUND_NONE;
  const int64_t nv = S / V;
  return (nv & (nv - 1)) == 0 ? DMXQ_ADAROUND_SHIFT : DMXQ_ADAROUND_DIVIDE;
}

inline ArSeg ar_seg(int dtype, int64_t n_segments, int64_t S) {
  const int64_t nv = S / (dtype == DMXQ_F32 ? 4 : 8);
  if (n_segments == 1) return ArSeg{nv, 63, kArShift};   // (u >> 63 == 0: no lookup arithmetic for the per-tensor cast)
  if ((nv & (nv - 1)) == 0) {
    int l2 = 0;
    while (((int64_t)1 << l2) < nv) l2++;
    return ArSeg{nv, l2, kArShift};
  }
  return ArSeg{nv, 0, n_segments * S < ((int64_t)1 << 31) ? kArDiv32 : kArDiv64};
}

// the checks both entries share (g's dtype takes the place of the output's in the backward) -> DMXQ_OK to go on
inline int ar_check(int dtype_w, int dtype_o, int64_t n_segments, int64_t segment, int qmin, int qmax) {
  if (!valid_dtype(dtype_w) || !valid_dtype(dtype_o)) return DMXQ_ERR_BAD_ARG;
  if (n_segments < 0 || segment < 0 || qmax <= qmin) return DMXQ_ERR_BAD_ARG;
  if (dtype_o != dtype_w && dtype_o != DMXQ_F32) return DMXQ_ERR_UNSUPPORTED;
  if (segment > 0 && ar_class(dtype_w, segment) == DMXQ_ADAROUND_NONE) return DMXQ_ERR_UNSUPPORTED;
  if (segment > 0 && n_segments > INT64_MAX / (segment * 4)) return DMXQ_ERR_UNSUPPORTED;
  return DMXQ_OK;
}

}  // namespace
}  // namespace dmxq

using namespace dmxq;

extern "C" int dmxq_adaround_class(int dtype, int64_t segment) {
  if (!valid_dtype(dtype)) return DMXQ_ADAROUND_NONE;
  return ar_class(dtype, segment);
}

extern "C" int64_t dmxq_adaround_scratch_bytes(int64_t n) {
  if (n < 0) return 0;
  return (int64_t)ar_grid(n) * (int64_t)sizeof(double);
}

extern "C" int dmxq_adaround_forward(const void* w, const float* V, void* y, int dtype_w, int dtype_out, int64_t n_segments, int64_t segment,
                                     int qmin, int qmax, const float* scale, const float* zero_point, int hard, void* stream) {
  const int st = ar_check(dtype_w, dtype_out, n_segments, segment, qmin, qmax);
  if (st != DMXQ_OK) return st;
  if (n_segments > 0 && segment > 0 && (!w || !V || !y || !scale || !zero_point)) return DMXQ_ERR_BAD_ARG;
  if (n_segments == 0 || segment == 0) return DMXQ_OK;
  if (!aligned16(w) || !aligned16(V) || !aligned16(y)) return DMXQ_ERR_UNSUPPORTED;
  const int64_t n = n_segments * segment;
  const int64_t nunits = n / (dtype_w == DMXQ_F32 ? 4 : 8);
  const ArSeg sg = ar_seg(dtype_w, n_segments, segment);
  const ArFmt f{(float)qmin, (float)qmax};
  const int grid = ar_grid(n);
  hipStream_t s = (hipStream_t)stream;
#define DMXQ_AR_FWD(D_, O_) DMXQ_LAUNCH((adaround_forward_kernel<D_, O_>), dim3(grid), dim3(kArThreads), 0, s, w, V, y, nunits, sg, f, scale, zero_point, hard ? 1 : 0)
  const bool o32 = dtype_out == DMXQ_F32;
  if (dtype_w == DMXQ_BF16) { if (o32) DMXQ_AR_FWD(DMXQ_BF16, true); else DMXQ_AR_FWD(DMXQ_BF16, false); }
  else if (dtype_w == DMXQ_F16) { if (o32) DMXQ_AR_FWD(DMXQ_F16, true); else DMXQ_AR_FWD(DMXQ_F16, false); }
  else DMXQ_AR_FWD(DMXQ_F32, true);
#undef DMXQ_AR_FWD
  return launch_status();
}

extern "C" int dmxq_adaround_backward(const void* w, const float* V, const void* g, float* dV, int dtype_w, int dtype_g, int64_t n_segments,
                                      int64_t segment, int qmin, int qmax, const float* scale, const float* zero_point, float beta,
                                      float reg_weight, double* reg_out, void* scratch, int64_t scratch_bytes, void* stream) {
  const int st = ar_check(dtype_w, dtype_g, n_segments, segment, qmin, qmax);
  if (st != DMXQ_OK) return st;
  if (scratch_bytes < 0) return DMXQ_ERR_BAD_ARG;
  if (n_segments > 0 && segment > 0 && (!w || !V || !g || !dV || !scale || !zero_point)) return DMXQ_ERR_BAD_ARG;
  const int64_t n = n_segments * segment;
  if (reg_out && n > 0) {
    if (!scratch || scratch_bytes < dmxq_adaround_scratch_bytes(n)) return DMXQ_ERR_BAD_ARG;
    if ((reinterpret_cast<uintptr_t>(scratch) & 7u) || (reinterpret_cast<uintptr_t>(reg_out) & 7u)) return DMXQ_ERR_UNSUPPORTED;
  }
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    if (reg_out) {   // the empty sum
      DMXQ_LAUNCH(adaround_final_kernel, dim3(1), dim3(kArThreads), 0, s, (const double*)nullptr, 0, reg_out);
      return launch_status();
    }
    return DMXQ_OK;
  }
  if (!aligned16(w) || !aligned16(V) || !aligned16(g) || !aligned16(dV)) return DMXQ_ERR_UNSUPPORTED;
  const int64_t nunits = n / (dtype_w == DMXQ_F32 ? 4 : 8);
  const ArSeg sg = ar_seg(dtype_w, n_segments, segment);
  const ArFmt f{(float)qmin, (float)qmax};
  const ArReg rg{beta - 1.0f, -2.0f * beta, reg_weight, (reg_weight != 0.0f || reg_out) ? 1 : 0};
  const int grid = ar_grid(n);
  double* part = reg_out ? (double*)scratch : nullptr;
#define DMXQ_AR_BWD(D_, G_) DMXQ_LAUNCH((adaround_backward_kernel<D_, G_>), dim3(grid), dim3(kArThreads), 0, s, w, V, g, dV, nunits, sg, f, scale, zero_point, rg, part)
  const bool g32 = dtype_g == DMXQ_F32;
  if (dtype_w == DMXQ_BF16) { if (g32) DMXQ_AR_BWD(DMXQ_BF16, true); else DMXQ_AR_BWD(DMXQ_BF16, false); }
  else if (dtype_w == DMXQ_F16) { if (g32) DMXQ_AR_BWD(DMXQ_F16, true); else DMXQ_AR_BWD(DMXQ_F16, false); }
  else DMXQ_AR_BWD(DMXQ_F32, true);
#undef DMXQ_AR_BWD
  if (reg_out) DMXQ_LAUNCH(adaround_final_kernel, dim3(1), dim3(kArThreads), 0, s, (const double*)part, grid, reg_out);
  return launch_status();
}
