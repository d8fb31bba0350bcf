// csrc/lsq.hip — the backward pass of a learned step size integer cast (LSQ, Esser et al. 2020; LSQ+, Bhalgat et al. 2020) in ONE pass
// over memory (include/dmxq.h dmxq_lsq_backward; DESIGN.md §8 "Learned step size").  Not in the reference, whose casts are identity
// straight-through estimators.  The forward of such a cast is dmxq_fixed_qdq with one (scale, zero point) per segment, unchanged; this
// file turns the incoming gradient g into dx (the CLIPPED straight-through estimator) and the two sums per segment that are the
// gradients of the scale s and of the float zero point z.
//
// Definition, per element, every operation fp32 and in this order (zq = clamp(rint(z), qmin, qmax), the offset the forward uses):
//   v  = x / s + zq                      IEEE division, then the add: fixedq.hpp fixed_affine_q1's own operand
//   r  = rne_minus_half(v + 0.5f)        fixedq.hpp: the forward's rounding, shared
//   in = qmin <= r && r <= qmax;   q = clamp(r, qmin, qmax)   (a NaN r is not `in` and stays NaN through the clamp)
//   dx = in ? g : 0
//   e  = in ? q - v : q - zq             ONE fp32 subtraction
//   ts = g * e;   tz = in ? 0 : -(g * s)
// and per segment ds = (float)(k * sum (double)ts), dz = (float)(k * sum (double)tz), k the gradient factor (a double argument).
// NaN: a NaN x makes r NaN: the element is not `in`, dx = 0, and q - zq is NaN: ds of its segment is NaN.  A NaN g makes ts NaN (ds NaN)
// and is passed on as dx where the element is `in`.  Nothing is special-cased: it all follows from the comparisons.
// Repeatability: error_stats.hip's rule.  No floating-point atomics; a lane sums its own elements in index order in fp64, lanes are
// folded by a fixed xor butterfly, waves in wave order, partial rows of the "tensor" class by a second small launch in a fixed order
// (no ticket: error_stats.hip says why).  The order depends on the shape alone: the same call twice gives the same bits.
//
// Geometry: dynamic_geom.hpp's segment classes, one 16-byte load of x and of g and one 16-byte store of dx per vector.  dx does not
// depend on the sums, so nothing waits for a reduction: a vector is loaded, cast, stored and folded into the lane's two accumulators.
//   * group (S = 16 .. 256, a power of two): S / V adjacent lanes per segment, a wave takes U x 64 consecutive vectors;
//   * short_row / wave_row: a wave per row, four rows per workgroup; block_row: a 256-thread workgroup per row; a lane walks its row in
//     batches of four vectors in flight;
//   * tensor (ONE segment of any whole number of vectors): a grid-stride stream; every workgroup writes one partial row [sum ts, sum tz]
//     into the caller's scratch, lsq_final_kernel folds the rows.
#include <math.h>

#include "dynamic_geom.hpp"
#include "fixedq.hpp"

namespace dmxq {
namespace {

constexpr int kLsqThreads = kDynThreads;
constexpr int kLsqWaves = kLsqThreads / kWave;
constexpr int kLsqBatch = 4;                 // 16-byte loads in flight per lane and operand
constexpr int kLsqWgPerCu = 8;               // the largest "tensor" grid: 8 workgroups on every CU (common.hpp plan_cus)
constexpr int64_t kLsqShare = 8192;          // elements of a "tensor" workgroup's share: 256 lanes x 4 vectors of 8 sixteen-bit elements

struct LsqFmt { float qmin, qmax; };

__device__ __forceinline__ float lsq_zq(float z, const LsqFmt& f) {
  const float r = rintf(z);
  return r < f.qmin ? f.qmin : (r > f.qmax ? f.qmax : r);
}

// one segment's constants and a lane's two fp64 accumulators
template <bool DZ>
struct LsqLane {
  float s, zq;
  double ts, tz;
  __device__ __forceinline__ void setup(float scale, float z, const LsqFmt& f) { s = scale; zq = lsq_zq(z, f); ts = 0.0; tz = 0.0; }
  // V elements of x and g -> dx, and the lane's sums (elements in index order)
  template <int V>
  __device__ __forceinline__ void add(const float (&x)[V], const float (&g)[V], float (&dx)[V], const LsqFmt& f) {
#pragma unroll
    for (int j = 0; j < V; j++) {
      const float v = x[j] / s + zq;
      const float r = rne_minus_half(v + 0.5f);
      const bool in = (f.qmin <= r) && (r <= f.qmax);
      const float q = r < f.qmin ? f.qmin : (r > f.qmax ? f.qmax : r);
      dx[j] = in ? g[j] : 0.0f;
      const float e = in ? (q - v) : (q - zq);
      ts += (double)(g[j] * e);
      if (DZ) tz += (double)(in ? 0.0f : -(g[j] * s));
    }
  }
};

// the sums of `lanes` adjacent lanes (a power of two up to 64) by an xor butterfly: every lane of the group ends with the same bits
template <bool DZ>
__device__ __forceinline__ void lsq_fold(double& a, double& b, int lanes) {
  for (int o = 1; o < lanes; o <<= 1) {
    a += __shfl_xor(a, o);
    if (DZ) b += __shfl_xor(b, o);
  }
}

// the workgroup's (a, b) -> out[0 .. 1]: butterfly inside a wave, waves in wave order
template <bool DZ>
__device__ __forceinline__ void lsq_block_store(double a, double b, double* out, double (*sh)[2]) {
  lsq_fold<DZ>(a, b, kWave);
  const int w = threadIdx.x / kWave;
  if ((threadIdx.x & (kWave - 1)) == 0) { sh[w][0] = a; sh[w][1] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double p = sh[0][0], q = sh[0][1];
#pragma unroll
    for (int k = 1; k < kLsqWaves; k++) { p += sh[k][0]; q += sh[k][1]; }
    out[0] = p;
    out[1] = DZ ? q : 0.0;
  }
}

// ------------------------------------------------------------------------------------------------ group
// segments of `lanes` adjacent lanes; nvec = n_segments * lanes vectors in all; wave w takes vectors [w U 64, (w + 1) U 64).  Lanes past
// the end re-read the last vector, meet only each other (the tensor ends on a segment boundary) and store nothing.
template <int DT, int U, bool DZ>
__global__ __launch_bounds__(kLsqThreads) void lsq_group_kernel(const void* __restrict__ xin, const void* __restrict__ gin, void* __restrict__ dxo,
                                                               int64_t nvec, int lanes, int lanes_log2, const LsqFmt f,
                                                               const float* __restrict__ scale, const float* __restrict__ zp, double k,
                                                               float* __restrict__ ds, float* __restrict__ dz) {
  constexpr int V = 16 / Elem<DT>::bytes;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = (int64_t)blockIdx.x * kLsqWaves + threadIdx.x / kWave;
  const int64_t base = wave * (U * kWave) + lane;
  u32x4 rx[U], rg[U];
#pragma unroll
  for (int u = 0; u < U; u++) {
    const int64_t i = base + (int64_t)u * kWave;
    const int64_t ic = i < nvec ? i : nvec - 1;
    rx[u] = load_raw16<true>(xin, ic * 16);
    rg[u] = load_raw16<true>(gin, ic * 16);
  }
#pragma unroll
  for (int u = 0; u < U; u++) {
    const int64_t i = base + (int64_t)u * kWave;
    const int64_t seg = (i < nvec ? i : nvec - 1) >> lanes_log2;
    LsqLane<DZ> a;
    a.setup(scale[seg], zp[seg], f);
    float x[V], g[V], d[V];
    widen<DT, V>(rx[u], x);
    widen<DT, V>(rg[u], g);
    a.template add<V>(x, g, d, f);
    lsq_fold<DZ>(a.ts, a.tz, lanes);
    if (i < nvec) {
      if (dxo) store_vec<DT, V>(dxo, i * V, d);
      if ((lane & (lanes - 1)) == 0) {
        ds[seg] = (float)(k * a.ts);
        if (DZ) dz[seg] = (float)(k * a.tz);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ rows
// rows of nv vectors; WAVES = 1: a wave per row, four rows per workgroup; WAVES = 4: the workgroup's row.  Lane t takes the vectors
// t, t + T, t + 2 T, ... of its row, kLsqBatch of them in flight.
template <int DT, int WAVES, bool DZ>
__global__ __launch_bounds__(kLsqThreads) void lsq_rows_kernel(const void* __restrict__ xin, const void* __restrict__ gin, void* __restrict__ dxo,
                                                              int64_t rows, int nv, const LsqFmt f, const float* __restrict__ scale,
                                                              const float* __restrict__ zp, double k, float* __restrict__ ds,
                                                              float* __restrict__ dz) {
  constexpr int V = 16 / Elem<DT>::bytes;
  constexpr int T = kWave * WAVES;                       // lanes per row
  constexpr int RPB = kLsqThreads / T;                   // rows per workgroup
  __shared__ double s_red[kLsqWaves][2];
  __shared__ double s_out[2];
  const int t = threadIdx.x & (T - 1);
  const int64_t row = (int64_t)blockIdx.x * RPB + threadIdx.x / T;
  if (row >= rows) return;                               // (wave-uniform, and only where WAVES == 1: no barrier is skipped)
  const int64_t v0 = row * nv;
  LsqLane<DZ> a;
  a.setup(scale[row], zp[row], f);
  for (int v = t; v < nv; v += kLsqBatch * T) {
    u32x4 rx[kLsqBatch], rg[kLsqBatch];
#pragma unroll
    for (int u = 0; u < kLsqBatch; u++) {
      const int vv = v + u * T < nv ? v + u * T : v;     // (a slot past the row re-reads the lane's first vector and adds nothing)
      rx[u] = load_raw16<true>(xin, (v0 + vv) * 16);
      rg[u] = load_raw16<true>(gin, (v0 + vv) * 16);
    }
    __builtin_amdgcn_sched_barrier(0);   // all 2 * kLsqBatch loads are issued before the first is waited for
#pragma unroll
    for (int u = 0; u < kLsqBatch; u++) {
      if (u == 0 || v + u * T < nv) {
        float x[V], g[V], d[V];
        widen<DT, V>(rx[u], x);
        widen<DT, V>(rg[u], g);
        a.template add<V>(x, g, d, f);
        if (dxo) store_vec<DT, V>(dxo, (v0 + v + u * T) * V, d);
      }
    }
  }
  if constexpr (WAVES == 1) {
    lsq_fold<DZ>(a.ts, a.tz, kWave);
    if (t == 0) {
      ds[row] = (float)(k * a.ts);
      if (DZ) dz[row] = (float)(k * a.tz);
    }
  } else {
    lsq_block_store<DZ>(a.ts, a.tz, s_out, s_red);
    if (threadIdx.x == 0) {
      ds[row] = (float)(k * s_out[0]);
      if (DZ) dz[row] = (float)(k * s_out[1]);
    }
  }
}

// ------------------------------------------------------------------------------------------------ tensor
// ONE segment of nvec vectors over the grid; workgroup b writes its partial row part[2 b .. 2 b + 1]
template <int DT, bool DZ>
__global__ __launch_bounds__(kLsqThreads) void lsq_tensor_kernel(const void* __restrict__ xin, const void* __restrict__ gin, void* __restrict__ dxo,
                                                                int64_t nvec, const LsqFmt f, const float* __restrict__ scale,
                                                                const float* __restrict__ zp, double* __restrict__ part) {
  constexpr int V = 16 / Elem<DT>::bytes;
  __shared__ double s_red[kLsqWaves][2];
  LsqLane<DZ> a;
  a.setup(scale[0], zp[0], f);
  const int64_t stride = (int64_t)gridDim.x * kLsqThreads;
  const int64_t t0 = (int64_t)blockIdx.x * kLsqThreads + threadIdx.x;
  for (int64_t t = t0; t < nvec; t += kLsqBatch * stride) {
    u32x4 rx[kLsqBatch], rg[kLsqBatch];
#pragma unroll
    for (int u = 0; u < kLsqBatch; u++) {
      const int64_t vv = t + u * stride < nvec ? t + u * stride : t;
      rx[u] = load_raw16<true>(xin, vv * 16);
      rg[u] = load_raw16<true>(gin, vv * 16);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < kLsqBatch; u++) {
      if (u == 0 || t + u * stride < nvec) {
        float x[V], g[V], d[V];
        widen<DT, V>(rx[u], x);
        widen<DT, V>(rg[u], g);
        a.template add<V>(x, g, d, f);
        if (dxo) store_vec<DT, V>(dxo, (t + u * stride) * V, d);
      }
    }
  }
  lsq_block_store<DZ>(a.ts, a.tz, part + (int64_t)blockIdx.x * 2, s_red);
}

// one workgroup: thread t folds the partial rows t, t + 256, ... in order, then butterfly and waves in order
__global__ __launch_bounds__(kLsqThreads) void lsq_final_kernel(const double* __restrict__ part, int nwg, double k, int want_dz,
                                                               float* __restrict__ ds, float* __restrict__ dz) {
  __shared__ double s_red[kLsqWaves][2];
  __shared__ double s_out[2];
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < nwg; i += kLsqThreads) {
    a += part[(int64_t)i * 2];
    b += part[(int64_t)i * 2 + 1];
  }
  lsq_block_store<true>(a, b, s_out, s_red);
  if (threadIdx.x == 0) {
    ds[0] = (float)(k * s_out[0]);
    if (want_dz) dz[0] = (float)(k * s_out[1]);
  }
}

inline int lsq_grid(int64_t n) {
  const int64_t g = (n + kLsqShare - 1) / kLsqShare;
  const int64_t max_wg = (int64_t)kLsqWgPerCu * plan_cus();
  return (int)(g < 1 ? 1 : (g > max_wg ? max_wg : g));
}

// mode: 0 groups inside rows, 1 whole rows, 2 the whole tensor as one segment
inline int lsq_class(int64_t S, int V, int mode) {
  if (mode == 2) return (S >= 1 && S % V == 0) ? DMXQ_LSQ_TENSOR : DMXQ_DYN_NONE;
  return dyn_class(S, V, mode != 0);
}

struct LsqArgs {
  const void *x, *g;
  void* dx;
  int64_t n_segments, S;
  int mode;
  LsqFmt f;
  const float *scale, *zp;
  double k;
  float *ds, *dz;
  double* part;
  hipStream_t s;
};

template <int DT, bool DZ>
int lsq_launch(const LsqArgs& a) {
  constexpr int V = 16 / Elem<DT>::bytes;
  const int64_t nv = a.S / V;   // vectors per segment
  const int cls = lsq_class(a.S, V, a.mode);
  if (cls == DMXQ_DYN_NONE) return DMXQ_ERR_UNSUPPORTED;
  if (cls == DMXQ_LSQ_TENSOR) {
    const int grid = lsq_grid(a.S);
    DMXQ_LAUNCH((lsq_tensor_kernel<DT, DZ>), dim3(grid), dim3(kLsqThreads), 0, a.s, a.x, a.g, a.dx, nv, a.f, a.scale, a.zp, a.part);
    DMXQ_LAUNCH(lsq_final_kernel, dim3(1), dim3(kLsqThreads), 0, a.s, (const double*)a.part, grid, a.k, DZ ? 1 : 0, a.ds, a.dz);
    return launch_status();
  }
  if (cls == DMXQ_DYN_GROUP) {
    const int lanes = (int)nv;   // 2 .. 64
    int l2 = 0;
    while ((1 << l2) < lanes) l2++;
    const int64_t nvec = a.n_segments * nv;
    // dynamic_quant.hip's rule: one vector per lane while that already fills the device, four independent loads per lane and operand beyond
    const bool deep = plan_norm(nvec) > ((int64_t)1 << 19);
    const int64_t per_wg = (int64_t)kLsqThreads * (deep ? 4 : 1);
    const int64_t grid = (nvec + per_wg - 1) / per_wg;
    if (grid > 0x7FFFFFFF) return DMXQ_ERR_UNSUPPORTED;
    if (deep) DMXQ_LAUNCH((lsq_group_kernel<DT, 4, DZ>), dim3((unsigned)grid), dim3(kLsqThreads), 0, a.s, a.x, a.g, a.dx, nvec, lanes, l2, a.f, a.scale, a.zp, a.k, a.ds, a.dz);
    else DMXQ_LAUNCH((lsq_group_kernel<DT, 1, DZ>), dim3((unsigned)grid), dim3(kLsqThreads), 0, a.s, a.x, a.g, a.dx, nvec, lanes, l2, a.f, a.scale, a.zp, a.k, a.ds, a.dz);
    return launch_status();
  }
  const bool wave_row = cls != DMXQ_DYN_BLOCK_ROW;
  const int64_t rpb = wave_row ? kLsqWaves : 1;
  const int64_t grid = (a.n_segments + rpb - 1) / rpb;
  if (grid > 0x7FFFFFFF) return DMXQ_ERR_UNSUPPORTED;
  if (wave_row) DMXQ_LAUNCH((lsq_rows_kernel<DT, 1, DZ>), dim3((unsigned)grid), dim3(kLsqThreads), 0, a.s, a.x, a.g, a.dx, a.n_segments, (int)nv, a.f, a.scale, a.zp, a.k, a.ds, a.dz);
  else DMXQ_LAUNCH((lsq_rows_kernel<DT, 4, DZ>), dim3((unsigned)grid), dim3(kLsqThreads), 0, a.s, a.x, a.g, a.dx, a.n_segments, (int)nv, a.f, a.scale, a.zp, a.k, a.ds, a.dz);
  return launch_status();
}

}  // namespace
}  // namespace dmxq

using namespace dmxq;

extern "C" int dmxq_lsq_class(int dtype, int64_t segment, int whole_rows) {
  if (!valid_dtype(dtype) || whole_rows < 0 || whole_rows > 2) return DMXQ_DYN_NONE;
  return lsq_class(segment, dtype == DMXQ_F32 ? 4 : 8, whole_rows);
}

extern "C" int64_t dmxq_lsq_scratch_bytes(int64_t n) {
  if (n < 0) return 0;
  return (int64_t)lsq_grid(n) * 2 * (int64_t)sizeof(double);
}

extern "C" int dmxq_lsq_backward(const void* x, const void* g, void* dx, int dtype_x, int dtype_g, int dtype_dx, int64_t n_segments,
                                 int64_t segment, int whole_rows, int precision, int rounding, int qmin, int qmax, const float* scale,
                                 const float* zero_point, double grad_factor, int want_dz, float* ds, float* dz, void* scratch,
                                 int64_t scratch_bytes, void* stream) {
  if (!valid_dtype(dtype_x) || !valid_dtype(dtype_g) || !valid_dtype(dtype_dx) || !valid_rounding(rounding)) return DMXQ_ERR_BAD_ARG;
  if (n_segments < 0 || segment < 0 || precision < 1 || qmax <= qmin || whole_rows < 0 || whole_rows > 2) return DMXQ_ERR_BAD_ARG;
  if (whole_rows == 2 && n_segments > 1) return DMXQ_ERR_BAD_ARG;
  if (n_segments > 0 && segment > 0 && (!x || !g || !scale || !zero_point || !ds || (want_dz && !dz))) return DMXQ_ERR_BAD_ARG;
  // what the kernels take; everything else is the caller's chain (nothing launched)
  if (dtype_x != dtype_g || dtype_x != dtype_dx || rounding != DMXQ_ROUND_NEAREST || precision > 22) return DMXQ_ERR_UNSUPPORTED;
  const int V = dtype_x == DMXQ_F32 ? 4 : 8;
  if (segment % V != 0) return DMXQ_ERR_UNSUPPORTED;
  if (n_segments == 0 || segment == 0) return DMXQ_OK;
  const int cls = lsq_class(segment, V, whole_rows);
  if (cls == DMXQ_DYN_NONE) return DMXQ_ERR_UNSUPPORTED;
  if (!aligned16(x) || !aligned16(g) || (dx && !aligned16(dx))) return DMXQ_ERR_UNSUPPORTED;
  if (n_segments > INT64_MAX / (segment * 4)) return DMXQ_ERR_UNSUPPORTED;
  if (cls == DMXQ_LSQ_TENSOR) {
    if (!scratch || (reinterpret_cast<uintptr_t>(scratch) & 7u)) return DMXQ_ERR_UNSUPPORTED;
    if (scratch_bytes < dmxq_lsq_scratch_bytes(segment)) return DMXQ_ERR_BAD_ARG;
  }
  const LsqArgs a{x, g, dx, n_segments, segment, whole_rows, LsqFmt{(float)qmin, (float)qmax}, scale, zero_point, grad_factor, ds, dz,
                  (double*)scratch, (hipStream_t)stream};
#define DMXQ_LSQ(D_) (want_dz ? lsq_launch<D_, true>(a) : lsq_launch<D_, false>(a))
  if (dtype_x == DMXQ_BF16) return DMXQ_LSQ(DMXQ_BF16);
  if (dtype_x == DMXQ_F16) return DMXQ_LSQ(DMXQ_F16);
  return DMXQ_LSQ(DMXQ_F32);
#undef DMXQ_LSQ
}
