// csrc/error_stats.hip — quantization-error statistics on the device (include/dmxq.h "error statistics"):
//   * dmxq_error_stats   [sum (r - t)^2, sum r^2, max |r - t|, n] of a reference and a test tensor, one read of each;
//   * dmxq_cast_error    the same row for each of up to 8 formats between a [rows, L] tensor and its cast to that format, from ONE read
//                        of the tensor: the casts are evaluated in registers and nothing is written but the statistics.
// Replaces utils/benchmark.py:349-389 (per tensor pair one mse_loss, one abs().max() and two .item() synchronisations) and, for a
// sweep over K formats, K casts (read + write each) followed by 2 K torch reductions over temporaries.
//
// Definitions (one for both kernels), r / t widened to fp32 (exact):
//   d = r - t                 ONE fp32 subtraction
//   sum_sq_err += d * d       formed in fp64 -- exact, d has 24 significant bits -- and accumulated in fp64 (a fused multiply-add of an
//                             exact product is the separately rounded sum: -ffp-contract=off changes nothing here)
//   sum_sq_ref += r * r       likewise
//   max_abs_err               torch's (r - t).float().abs().max(): the difference rounded to the promoted dtype of the pair, widened.
//                             Rounding to nearest is monotone and odd, so max |round(d)| = round(max |d|): the lanes keep the fp32
//                             maximum and the final kernel rounds it once.
// NaN: a NaN difference makes sum_sq_err NaN by itself; the maximum is taken on the BIT PATTERNS of |d| as unsigned integers, where
// every NaN pattern lies above +inf -- a NaN wins every comparison and stays (fmaxf would drop it).
// Repeatability: no floating-point atomics.  Every lane sums its own elements in index order, a wave is folded by a fixed xor
// butterfly, the waves of a workgroup in wave order into one partial row in `scratch`, and the final kernel folds the partial rows in
// a fixed order (a second small launch: reduce.hip measured a returning atomic ticket slower than a separate launch on this chip,
// profiles/r04_tune_reduce_tickets.txt, and a fixed order needs no ticket at all).  The same input twice gives the same bits.
//
// dmxq_cast_error, geometry: the tensor is flat -- L is a multiple of every block size, so the blocks of the flat index ARE the row
// blocks.  A lane holds 8 consecutive elements (16 bytes of a 16-bit tensor), a wave 512: blocks of 8 .. 128 elements are 1 .. 16
// neighbouring lanes, whose maxima (on the bit patterns of |x|, what the BFP kernels compare) are one lane-local maximum and up to
// four xor shuffles per vector and format.  The casts are the literal per-element leaves (bfp_math.hpp bfp_block_params /
// bfp_q1_nearest_rt, floatq.hpp float_q1, fixedq.hpp fixed_affine_q1 with its IEEE division): bit for bit the library's casts, then rounded to the tensor's
// dtype as CastTo.forward returns them.  The format loop runs over descriptors held in the kernel arguments and is NOT unrolled (one
// copy of the three cast bodies whatever K is; no spills at K = 8): a batch of vectors stays in registers across the loop, every
// format folds the batch into a register pair and then into its lane's slot in LDS (K * 12 bytes per lane).
#include <math.h>

#include "bfp_math.hpp"
#include "format_desc.hpp"
#include "reduce_common.hpp"

namespace dmxq {
namespace {

constexpr int kErrThreads = 256;
constexpr int kErrWaves = kErrThreads / kWave;
constexpr int kErrWgPerCu = 8;      // the largest grid: 8 workgroups of 4 waves on every CU of the device (common.hpp plan_cus: 2048 on 256 CUs)
constexpr int kErrMaxFormats = 8;
constexpr int kErrBatch = 4;        // 16-byte loads in flight per lane and operand
constexpr int kErrRow = 4;          // doubles per partial row: sum_sq_err, sum_sq_ref, bits of max |d|, unused

struct ErrAcc {
  double sse, ssr;
  uint32_t mb;   // bit pattern of max |d| (a NaN pattern once any d was NaN)
  __device__ __forceinline__ void add(float r, float t) {
    const float d = r - t;
    sse = fma((double)d, (double)d, sse);
    ssr = fma((double)r, (double)r, ssr);
    mb = umax(mb, f2u(d) & 0x7FFFFFFFu);
  }
};

// the workgroup's (sse, ssr, mb) -> row[0 .. 2]: xor butterfly inside a wave (every lane ends with the same bits), waves in order
__device__ __forceinline__ void err_block_store(double sse, double ssr, uint32_t mb, double* row, double (*s)[3]) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    sse += __shfl_xor(sse, o);
    ssr += __shfl_xor(ssr, o);
    mb = umax(mb, (uint32_t)__shfl_xor((int)mb, o));
  }
  const int w = threadIdx.x / kWave;
  if ((threadIdx.x & (kWave - 1)) == 0) {
    s[w][0] = sse;
    s[w][1] = ssr;
    s[w][2] = __longlong_as_double((long long)mb);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = s[0][0], b = s[0][1];
    uint32_t m = (uint32_t)__double_as_longlong(s[0][2]);
#pragma unroll
    for (int k = 1; k < kErrWaves; k++) {
      a += s[k][0];
      b += s[k][1];
      m = umax(m, (uint32_t)__double_as_longlong(s[k][2]));
    }
    row[0] = a;
    row[1] = b;
    row[2] = __longlong_as_double((long long)m);
  }
  __syncthreads();
}

// ------------------------------------------------------------------------------------------------ error_stats
// VEC: both pointers 16-byte aligned: n / 8 vectors over the grid, the n % 8 last elements on the first lanes of workgroup 0.
template <int DR, int DT, bool VEC>
__global__ __launch_bounds__(kErrThreads) void error_stats_kernel(const void* __restrict__ ref, const void* __restrict__ test, int64_t n,
                                                                  double* __restrict__ part) {
  __shared__ double s_red[kErrWaves][3];
  ErrAcc acc{0.0, 0.0, 0u};
  const int64_t stride = (int64_t)gridDim.x * kErrThreads;
  const int64_t t0 = (int64_t)blockIdx.x * kErrThreads + threadIdx.x;
  if (VEC) {
    const int64_t nv = n / 8;
    for (int64_t t = t0; t < nv; t += kErrBatch * stride) {
      Raw8<DR> a[kErrBatch];
      Raw8<DT> b[kErrBatch];
#pragma unroll
      for (int u = 0; u < kErrBatch; u++) {
        const int64_t v = t + u * stride < nv ? t + u * stride : t;
        a[u] = load8_raw<DR>(ref, v * 8);
        b[u] = load8_raw<DT>(test, v * 8);
      }
      __builtin_amdgcn_sched_barrier(0);   // all 2 * kErrBatch loads are issued before the first is waited for
#pragma unroll
      for (int u = 0; u < kErrBatch; u++) {
        if (u == 0 || t + u * stride < nv) {
          float r[8], q[8];
          widen8<DR>(a[u], r);
          widen8<DT>(b[u], q);
#pragma unroll
          for (int j = 0; j < 8; j++) acc.add(r[j], q[j]);
        }
      }
    }
    const int64_t e = nv * 8 + t0;
    if (e < n) acc.add(load1<DR>(ref, e), load1<DT>(test, e));
  } else {
    for (int64_t e = t0; e < n; e += stride) acc.add(load1<DR>(ref, e), load1<DT>(test, e));
  }
  err_block_store(acc.sse, acc.ssr, acc.mb, part + (int64_t)blockIdx.x * kErrRow, s_red);
}

// ------------------------------------------------------------------------------------------------ cast_error
// The formats as the kernel takes them: 6 dwords each, field by field in 8-wide vectors (48 scalar registers' worth of kernel
// arguments).  The loop over formats is not unrolled; format k's fields are element k of each vector -- a register-indexed read.  (An
// array of structs indexed by k, and even a chain of selects over its entries, made the compiler keep the argument block in scratch.)
typedef int i32x8 __attribute__((ext_vector_type(8)));
struct ErrFmt {
  int kind;           // dmxq_gptq_kind
  int a, b, c, d, e;  // BFP: precision, log2(block_size / 8), "(_N)";  FLOAT: man, exp_bits, bias, flush, unsigned_abs;
                      // FIXED: sigma, clamp, bits of t_min, bits of t_max
};
struct ErrFmts {
  i32x8 kind, a, b, c, d, e;
  int n;         // formats in use
};
__device__ __forceinline__ ErrFmt err_fmt_at(const ErrFmts& fm, int k) {
  return ErrFmt{fm.kind[k], fm.a[k], fm.b[k], fm.c[k], fm.d[k], fm.e[k]};
}

template <int DT>
__device__ __forceinline__ float round_to(float v) {   // `.to(dtype)` and back: what CastTo.forward returns, widened
  if (DT == DMXQ_BF16) return (float)(__bf16)v;
  if (DT == DMXQ_F16) return (float)(_Float16)opaque(v);
  return v;
}

// the cast of one lane's 8 elements to format f; bm: bit pattern of the maximum |x| over these 8 elements.  Called by whole waves.
template <int DT>
__device__ __forceinline__ void err_cast8(const float (&x)[8], uint32_t bm, const ErrFmt& f, float sc, float z, float (&q)[8]) {
  if (f.kind == DMXQ_GPTQ_BFP) {
    const int wl = f.a;
    // blocks are aligned groups of 1 << f.b lanes, and the tensor ends on a block boundary: lanes past the end only meet each other
#pragma unroll
    for (int i = 0; i < 4; i++)
      if (i < f.b) bm = umax(bm, (uint32_t)__shfl_xor((int)bm, 1 << i));   // (wave-uniform: every lane of the wave takes part)
    const BfpBlockParams p = bfp_block_params<true, false>(bm, wl);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      q[j] = round_to<DT>(bfp_q1_nearest_rt(x[j], p, wl, f.c != 0));
    }
  } else if (f.kind == DMXQ_GPTQ_FLOAT) {
    const FloatFmt ff{f.a, f.b, f.c, f.d, f.e, DMXQ_ROUND_NEAREST, 0ull};
#pragma unroll
    for (int j = 0; j < 8; j++) q[j] = round_to<DT>(float_q1<DMXQ_ROUND_NEAREST>(x[j], ff, 0u));
  } else {
    const FixedFmt fx{f.a, f.b, DMXQ_ROUND_NEAREST, u2f((uint32_t)f.c), u2f((uint32_t)f.d), 0ull};
#pragma unroll
    for (int j = 0; j < 8; j++) q[j] = round_to<DT>(fixed_affine_q1(x[j], sc, z, fx));
  }
}

// nvec vectors of 8 elements; a wave takes chunks of 64 consecutive vectors (512 elements: whole blocks), kErrBatch chunks per round
template <int DT>
__global__ __launch_bounds__(kErrThreads) void cast_error_kernel(const void* __restrict__ in, int64_t nvec, const ErrFmts fm,
                                                                 const float* __restrict__ scale, const int64_t* __restrict__ zp,
                                                                 double* __restrict__ part) {
  extern __shared__ double s_dyn[];                 // [K][kErrThreads] sums, then [K][kErrThreads] maxima (uint32_t)
  __shared__ double s_red[kErrWaves][3];
  const int K = fm.n;
  double* const s_sse = s_dyn;
  uint32_t* const s_mb = (uint32_t*)(s_dyn + K * kErrThreads);
  for (int k = 0; k < K; k++) {
    s_sse[k * kErrThreads + threadIdx.x] = 0.0;
    s_mb[k * kErrThreads + threadIdx.x] = 0u;
  }
  double ssr = 0.0;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t nchunk = (nvec + kWave - 1) / kWave;
  const int64_t cstride = (int64_t)gridDim.x * kErrWaves;
  const int64_t c0 = (int64_t)blockIdx.x * kErrWaves + threadIdx.x / kWave;
  for (int64_t c = c0; c < nchunk; c += kErrBatch * cstride) {
    Raw8<DT> raw[kErrBatch];
#pragma unroll
    for (int u = 0; u < kErrBatch; u++) {
      const int64_t cc = c + u * cstride < nchunk ? c + u * cstride : c;
      const int64_t v = cc * kWave + lane;
      raw[u] = load8_raw<DT>(in, (v < nvec ? v : nvec - 1) * 8);   // (a lane past the end re-reads the last vector and adds nothing)
    }
    __builtin_amdgcn_sched_barrier(0);   // all kErrBatch loads are issued before the first is waited for
    float x[kErrBatch][8];
    uint32_t bmax[kErrBatch];
    bool act[kErrBatch];
#pragma unroll
    for (int u = 0; u < kErrBatch; u++) {
      act[u] = (u == 0 || c + u * cstride < nchunk) && (c + u * cstride) * kWave + lane < nvec;
      widen8<DT>(raw[u], x[u]);
      uint32_t m = 0u;
#pragma unroll
      for (int j = 0; j < 8; j++) m = umax(m, f2u(x[u][j]) & 0x7FFFFFFFu);
      bmax[u] = m;
      if (act[u]) {
#pragma unroll
        for (int j = 0; j < 8; j++) ssr = fma((double)x[u][j], (double)x[u][j], ssr);
      }
    }
    for (int k = 0; k < K; k++) {
      const ErrFmt f = err_fmt_at(fm, k);
      float sc = 1.0f, z = 0.0f;
      if (f.kind == DMXQ_GPTQ_FIXED) {
        sc = scale[k];
        z = (float)zp[k];
      }
      double sse = 0.0;
      uint32_t mb = 0u;
#pragma unroll
      for (int u = 0; u < kErrBatch; u++) {
        float q[8];
        err_cast8<DT>(x[u], bmax[u], f, sc, z, q);
        if (act[u]) {
#pragma unroll
          for (int j = 0; j < 8; j++) {
            const float d = x[u][j] - q[j];
            sse = fma((double)d, (double)d, sse);
            mb = umax(mb, f2u(d) & 0x7FFFFFFFu);
          }
        }
      }
      s_sse[k * kErrThreads + threadIdx.x] += sse;   // (the lane's own slot: no barrier)
      s_mb[k * kErrThreads + threadIdx.x] = umax(s_mb[k * kErrThreads + threadIdx.x], mb);
    }
  }
  for (int k = 0; k < K; k++)
    err_block_store(s_sse[k * kErrThreads + threadIdx.x], ssr, s_mb[k * kErrThreads + threadIdx.x],
                    part + ((int64_t)blockIdx.x * K + k) * kErrRow, s_red);
}

// ------------------------------------------------------------------------------------------------ final reduction
// one workgroup per format: thread t folds the partial rows t, t + 256, ... in order, then butterfly and waves in order; the maximum is
// rounded to MAXDT, the promoted dtype of the pair.  accumulate: sums add, max takes the max (a NaN stays), count adds.
__global__ __launch_bounds__(kErrThreads) void error_final_kernel(const double* __restrict__ part, int nwg, int K, int maxdt, double count,
                                                                  int accumulate, double* __restrict__ stats) {
  __shared__ double s_red[kErrWaves][3];
  __shared__ double s_row[kErrRow];
  const int k = blockIdx.x;
  double sse = 0.0, ssr = 0.0;
  uint32_t mb = 0u;
  for (int i = threadIdx.x; i < nwg; i += kErrThreads) {
    const double* row = part + ((int64_t)i * K + k) * kErrRow;
    sse += row[0];
    ssr += row[1];
    mb = umax(mb, (uint32_t)__double_as_longlong(row[2]));
  }
  err_block_store(sse, ssr, mb, s_row, s_red);
  if (threadIdx.x == 0) {
    const uint32_t m = (uint32_t)__double_as_longlong(s_row[2]);
    float mx = u2f(m);   // (a NaN pattern stays a NaN through the roundings below)
    if (maxdt == DMXQ_BF16) mx = round_to<DMXQ_BF16>(mx);
    else if (maxdt == DMXQ_F16) mx = round_to<DMXQ_F16>(mx);
    double o0 = s_row[0], o1 = s_row[1], o2 = (double)mx, o3 = count;
    double* out = stats + (int64_t)k * 4;
    if (accumulate) {
      const double old = out[2];
      o0 += out[0];
      o1 += out[1];
      o2 = (old != old || o2 != o2) ? (double)NAN : (old > o2 ? old : o2);
      o3 += out[3];
    }
    out[0] = o0;
    out[1] = o1;
    out[2] = o2;
    out[3] = o3;
  }
}

inline int err_grid(int64_t n) {
  const int64_t per_wg = (int64_t)kErrThreads * kErrBatch * 8;
  const int64_t g = (n + per_wg - 1) / per_wg;
  const int64_t max_wg = (int64_t)kErrWgPerCu * plan_cus();
  return (int)(g < 1 ? 1 : (g > max_wg ? max_wg : g));
}

}  // namespace
}  // namespace dmxq

using namespace dmxq;

extern "C" int64_t dmxq_error_scratch_bytes(int64_t n, int n_formats) {
  if (n < 0 || n_formats < 1) return 0;
  return (int64_t)err_grid(n) * n_formats * kErrRow * (int64_t)sizeof(double);
}

extern "C" int dmxq_error_stats(const void* ref, int dtype_ref, const void* test, int dtype_test, int64_t n, int accumulate, double* stats,
                                void* scratch, int64_t scratch_bytes, void* stream) {
  if (!valid_dtype(dtype_ref) || !valid_dtype(dtype_test)) return DMXQ_ERR_BAD_ARG;
  if (n < 0 || !stats) return DMXQ_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const int maxdt = dtype_ref == dtype_test ? dtype_ref : DMXQ_F32;   // torch's promotion of two floating dtypes
  if (n == 0) {
    if (!accumulate)
      DMXQ_LAUNCH(error_final_kernel, dim3(1), dim3(kErrThreads), 0, s, (const double*)nullptr, 0, 1, maxdt, 0.0, 0, stats);
    return accumulate ? DMXQ_OK : launch_status();
  }
  if (!ref || !test || !scratch) return DMXQ_ERR_UNSUPPORTED;
  if (reinterpret_cast<uintptr_t>(scratch) & 7u) return DMXQ_ERR_UNSUPPORTED;
  if (scratch_bytes < dmxq_error_scratch_bytes(n, 1)) return DMXQ_ERR_BAD_ARG;
  const int grid = err_grid(n);
  const bool vec = aligned16(ref) && aligned16(test);
  double* part = (double*)scratch;
#define DMXQ_ES(R_, T_) do { if (vec) DMXQ_LAUNCH((error_stats_kernel<R_, T_, true>), dim3(grid), dim3(kErrThreads), 0, s, ref, test, n, part); \
                             else DMXQ_LAUNCH((error_stats_kernel<R_, T_, false>), dim3(grid), dim3(kErrThreads), 0, s, ref, test, n, part); } while (0)
#define DMXQ_EST(R_) do { if (dtype_test == DMXQ_F32) DMXQ_ES(R_, DMXQ_F32); else if (dtype_test == DMXQ_F16) DMXQ_ES(R_, DMXQ_F16); \
                          else DMXQ_ES(R_, DMXQ_BF16); } while (0)
  if (dtype_ref == DMXQ_F32) DMXQ_EST(DMXQ_F32); else if (dtype_ref == DMXQ_F16) DMXQ_EST(DMXQ_F16); else DMXQ_EST(DMXQ_BF16);
#undef DMXQ_EST
#undef DMXQ_ES
  DMXQ_LAUNCH(error_final_kernel, dim3(1), dim3(kErrThreads), 0, s, (const double*)part, grid, 1, maxdt, (double)n, accumulate ? 1 : 0,
              stats);
  return launch_status();
}

extern "C" int dmxq_cast_error(const void* in, int dtype, int64_t rows, int64_t L, const dmxq_gptq_format* formats, int n_formats,
                               const float* scale, const int64_t* zero_point, int accumulate, double* stats, void* scratch,
                               int64_t scratch_bytes, void* stream) {
  if (!valid_dtype(dtype) || n_formats < 1) return DMXQ_ERR_BAD_ARG;
  if (n_formats > kErrMaxFormats || !formats) return DMXQ_ERR_UNSUPPORTED;
  for (int k = 0; k < n_formats; k++)
    if (formats[k].kind != DMXQ_GPTQ_BFP && formats[k].kind != DMXQ_GPTQ_FLOAT && formats[k].kind != DMXQ_GPTQ_FIXED) return DMXQ_ERR_BAD_ARG;
  if (rows < 0 || L < 0 || !stats) return DMXQ_ERR_UNSUPPORTED;
  ErrFmts fm{};
  fm.n = n_formats;
  for (int k = 0; k < n_formats; k++) {
    const dmxq_gptq_format& g = formats[k];
    ErrFmt e{g.kind, 0, 0, 0, 0, 0};
    FormatDesc d;
    if (g.per_row || format_desc(g, &d) != DMXQ_OK) return DMXQ_ERR_UNSUPPORTED;
    if (g.kind == DMXQ_GPTQ_BFP) {
      const int B = g.block_size;
      if (!(B == 8 || B == 16 || B == 32 || B == 64 || B == 128) || L % B != 0) return DMXQ_ERR_UNSUPPORTED;
      e.a = d.wl;
      e.b = B == 8 ? 0 : B == 16 ? 1 : B == 32 ? 2 : B == 64 ? 3 : 4;
      e.c = d.asym;
    } else if (g.kind == DMXQ_GPTQ_FLOAT) {
      e.a = d.f.man; e.b = d.f.exp_bits; e.c = d.f.bias; e.d = d.f.flush; e.e = d.f.unsigned_abs;
    } else {
      if (!scale || !zero_point) return DMXQ_ERR_UNSUPPORTED;
      e.a = d.x.sigma; e.b = d.x.clamp;
      memcpy(&e.c, &d.x.t_min, 4);
      memcpy(&e.d, &d.x.t_max, 4);
    }
    fm.kind[k] = e.kind; fm.a[k] = e.a; fm.b[k] = e.b; fm.c[k] = e.c; fm.d[k] = e.d; fm.e[k] = e.e;
  }
  if (L % 8 != 0) return DMXQ_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = rows * L;
  if (n == 0) {
    if (!accumulate)
      DMXQ_LAUNCH(error_final_kernel, dim3(n_formats), dim3(kErrThreads), 0, s, (const double*)nullptr, 0, n_formats, dtype, 0.0, 0, stats);
    return accumulate ? DMXQ_OK : launch_status();
  }
  if (!in || !scratch || !aligned16(in) || (reinterpret_cast<uintptr_t>(scratch) & 7u)) return DMXQ_ERR_UNSUPPORTED;
  if (scratch_bytes < dmxq_error_scratch_bytes(n, n_formats)) return DMXQ_ERR_BAD_ARG;
  const int grid = err_grid(n);
  const size_t lds = (size_t)n_formats * kErrThreads * (sizeof(double) + sizeof(uint32_t));
  double* part = (double*)scratch;
#define DMXQ_CE(D_) DMXQ_LAUNCH((cast_error_kernel<D_>), dim3(grid), dim3(kErrThreads), lds, s, in, n / 8, fm, scale, zero_point, part)
  if (dtype == DMXQ_F32) DMXQ_CE(DMXQ_F32); else if (dtype == DMXQ_F16) DMXQ_CE(DMXQ_F16); else DMXQ_CE(DMXQ_BF16);
#undef DMXQ_CE
  DMXQ_LAUNCH(error_final_kernel, dim3(n_formats), dim3(kErrThreads), 0, s, (const double*)part, grid, n_formats, dtype, (double)n,
              accumulate ? 1 : 0, stats);
  return launch_status();
}
