// csrc/codebook.hip — codebook casts (NF4, Lloyd-Max / k-means tables) in ONE launch, and the weighted Lloyd statistics that fit a table
// to a tensor on the device (include/dmxq.h dmxq_codebook_qdq, dmxq_codebook_accumulate; DESIGN.md §8 "Codebook casts").  Not in the
// reference, whose level sets are all fixed by a few bit-field widths: here a small table of ARBITRARY levels sits under a per-segment
// absolute-maximum scale.
//
// The definition (fp32 throughout).  The table: K levels c_0 <= ... <= c_{K-1}, 2 <= K <= 16 here; thresholds t_j = (c_j + c_{j+1}) * 0.5f
// (one add, one multiply), j < K - 1; the zero level z = the lowest index of the level with the smallest |c|.  Per segment:
//   amax = max |x|, ONE NaN anywhere makes it NaN (the maximum runs on the magnitude BITS, as dynamic_float.hip does)
//   s    = amax / norm, an IEEE division; norm <= 0: the table's own max(|c_0|, |c_{K-1}|); s = 1 when s is not finite or below 2^-126
//   u    = x / s, the IEEE quotient (dynamic_float.hpp df_quotient_vec: div_by_recip with its wave-uniform `/` redo)
//   idx  = #{ j : u > t_j }: a tie goes to the lower level, +Inf gives K - 1, -Inf gives 0, and a NaN u takes idx = z
//   y    = c[idx] * s: ONE fp32 multiply, one rounding to the output dtype.
// The table arrives as a DEVICE pointer and every derived value -- thresholds, z, the default norm -- is formed in the kernel as a
// wave-uniform value, so that a fit loop (accumulate, update the K levels with torch, cast) runs without a host round trip: capturable.
// A table shorter than 16 is padded in the kernel: missing levels repeat the last one, missing thresholds are +Inf (never exceeded), so
// ONE compiled body serves K = 2 .. 16.  Search and lookup are compare / select chains over levels held in scalar registers: the
// thresholds are non-decreasing, so { j : u > t_j } is a prefix and "the level after the last threshold exceeded" is c[idx]; no array
// is indexed at run time.
//
// The weighted Lloyd step (the true-MSE form: an element's error is s^2 (u - c)^2): over the elements whose u is finite, for the level
// k = idx, in float64, A[k,0] += w u, A[k,1] += w, A[k,2] += 1 with w = (double)s * (double)s.  Scale, u and idx are formed by the SAME
// device functions as the cast.  A lane keeps 16 x 3 accumulators in registers (select chains again), a wave folds them by a fixed xor
// butterfly, a workgroup adds its waves in wave order and writes one partial row; a second small launch folds the rows in a fixed order.
// No floating-point atomics: the same input gives the same bits.
//
// Geometry: dynamic_float.hip's, without tiles -- segments inside a wave (16 .. 256, a power of two), a wave per row (short_row /
// wave_row), a 256-thread workgroup per row (block_row); dynamic_float.hpp dynf_class, the same split of the rows.  A lane's 16-byte
// vectors stay RAW in registers between the maximum pass and the cast; a segment is read completely before any of it is written; lanes
// past the end re-read the last vector / row and store (and add) nothing.  Indices leave as one 8-byte (sixteen-bit dtypes) or 4-byte
// (fp32) store per lane vector, scales as plain stores from one lane per segment.
#include <math.h>

#include "dynamic_float.hpp"

namespace dmxq {
namespace {

constexpr int kCbMax = 16;                    // levels the kernels hold in registers
constexpr int kCbWaves = kDynThreads / kWave;
constexpr int kCbStats = kCbMax * 3;          // a partial row: [16][3] float64
constexpr int kCbWgPerCu = 4;                 // the largest accumulate grid: 4 workgroups on every CU (common.hpp plan_cus)

__device__ __forceinline__ float cb_uniform(float v) { return u2f((uint32_t)__builtin_amdgcn_readfirstlane((int)f2u(v))); }

// the table and what is derived from it, every member wave-uniform (scalar registers after unrolling: all indices are compile-time)
struct CbTable {
  float c[kCbMax], t[kCbMax - 1];
  float cz, norm;
  uint32_t z;
  __device__ __forceinline__ void load(const float* __restrict__ levels, int K, float norm_arg) {
#pragma unroll
    for (int j = 0; j < kCbMax; j++) c[j] = load_uniform_const(levels + (j < K ? j : K - 1));
#pragma unroll
    for (int j = 0; j < kCbMax - 1; j++) {
      const float m = (c[j] + c[j + 1]) * 0.5f;
      t[j] = cb_uniform(j < K - 1 ? m : INFINITY);
    }
    float best = __builtin_fabsf(c[0]);
    cz = c[0];
    z = 0u;
#pragma unroll
    for (int j = 1; j < kCbMax; j++) {
      const bool lower = j < K && __builtin_fabsf(c[j]) < best;
      best = lower ? __builtin_fabsf(c[j]) : best;
      cz = lower ? c[j] : cz;
      z = lower ? (uint32_t)j : z;
    }
    cz = cb_uniform(cz);
    z = (uint32_t)__builtin_amdgcn_readfirstlane((int)z);
    const float a = __builtin_fabsf(c[0]), b = __builtin_fabsf(c[kCbMax - 1]);
    norm = cb_uniform(norm_arg > 0.0f ? norm_arg : (a > b ? a : b));
  }
  // the nearest level of u and its index
  __device__ __forceinline__ void search(float u, float& lvl, uint32_t& idx) const {
    lvl = c[0];
    idx = 0u;
#pragma unroll
    for (int j = 0; j < kCbMax - 1; j++) {
      const bool g = u > t[j];
      lvl = g ? c[j + 1] : lvl;
      idx += g ? 1u : 0u;
    }
    const bool nan = u != u;
    lvl = nan ? cz : lvl;
    idx = nan ? z : idx;
  }
};

// ------------------------------------------------------------------------------------------------ the two uses of a vector
// A sink receives every lane vector of a tile once its segment's scale is known: vector index i (`live`: inside the tensor; a lane past
// the end holds a repeated vector), the quotients u, the scale.  seg(): once per segment, from every lane that holds its first vector.
template <int DT, bool IDX>
struct CbCastSink {
  static constexpr int V = 16 / Elem<DT>::bytes;
  void* out;
  uint8_t* index;
  float* scale_out;
  __device__ __forceinline__ void vec(int64_t i, bool live, const float (&u)[V], float s, const CbTable& tb) {
    float y[V];
    uint32_t id[V];
#pragma unroll
    for (int k = 0; k < V; k++) {
      float lvl;
      tb.search(u[k], lvl, id[k]);
      y[k] = lvl * s;
    }
    if (live) {
      store_vec<DT, V>(out, i * V, y);
      if constexpr (IDX) {
        const uint32_t w0 = id[0] | (id[1] << 8) | (id[2] << 16) | (id[3] << 24);
        if constexpr (V == 8) {
          const u32x2 w = {w0, id[4] | (id[5] << 8) | (id[6] << 16) | (id[7] << 24)};
          *(u32x2*)(index + i * 8) = w;
        } else {
          *(uint32_t*)(index + i * 4) = w0;
        }
      }
    }
  }
  __device__ __forceinline__ void seg(int64_t segment, float s) {
    if (scale_out) scale_out[segment] = s;
  }
};

template <int DT>
struct CbAccSink {
  static constexpr int V = 16 / Elem<DT>::bytes;
  double wu[kCbMax], w[kCbMax];
  uint32_t n[kCbMax];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int k = 0; k < kCbMax; k++) { wu[k] = 0.0; w[k] = 0.0; n[k] = 0u; }
  }
  __device__ __forceinline__ void vec(int64_t, bool live, const float (&u)[V], float s, const CbTable& tb) {
    const double ws = (double)s * (double)s;
#pragma unroll
    for (int e = 0; e < V; e++) {
      float lvl;
      uint32_t id;
      tb.search(u[e], lvl, id);
      const bool use = live && __builtin_fabsf(u[e]) < INFINITY;   // (a NaN compares false)
      id = use ? id : (uint32_t)kCbMax;
      const double p = ws * (double)u[e];
#pragma unroll
      for (int k = 0; k < kCbMax; k++) {
        const bool hit = id == (uint32_t)k;
        wu[k] += hit ? p : 0.0;
        w[k] += hit ? ws : 0.0;
        n[k] += hit ? 1u : 0u;
      }
    }
  }
  __device__ __forceinline__ void seg(int64_t, float) {}
};

// ------------------------------------------------------------------------------------------------ tiles
// segments of `lanes` adjacent lanes; nvec = n_segments * lanes vectors in all; wave `wave` takes vectors [wave U 64, (wave + 1) U 64)
template <int DT, int U, class SINK>
__device__ __forceinline__ void cb_group_tile(const void* __restrict__ in, int64_t nvec, int lanes, int lanes_log2, int64_t wave,
                                              const CbTable& tb, SINK& sink) {
  constexpr int V = 16 / Elem<DT>::bytes;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t base = wave * (U * kWave) + lane;
  u32x4 raw[U];
#pragma unroll
  for (int u = 0; u < U; u++) {
    const int64_t i = base + (int64_t)u * kWave;
    raw[u] = load_raw16<true>(in, (i < nvec ? i : nvec - 1) * 16);
  }
#pragma unroll
  for (int u = 0; u < U; u++) {
    const int64_t i = base + (int64_t)u * kWave;
    DfSeg sg;
    sg.setup(group_max_u32(absmax_bits<DT>(raw[u]), lanes), tb.norm, 0);
    const bool fast = __builtin_amdgcn_ballot_w64(!recip_ok(sg.s)) == 0ull;
    float x[V], q[V];
    widen<DT, V>(raw[u], x);
    df_quotient_vec<V>(x, q, sg, fast);
    const bool live = i < nvec;
    sink.vec(i, live, q, sg.s, tb);
    if (live && (lane & (lanes - 1)) == 0) sink.seg(i >> lanes_log2, sg.s);
  }
}

// row `row` of nv vectors; WAVES = 1: a wave's row; WAVES = 4: the workgroup's row (one barrier).  U x 64 x WAVES >= nv.
template <int DT, int U, int WAVES, class SINK>
__device__ __forceinline__ void cb_row_tile(const void* __restrict__ in, int64_t rows, int nv, int64_t row, const CbTable& tb, SINK& sink) {
  constexpr int V = 16 / Elem<DT>::bytes;
  constexpr int T = kWave * WAVES;                       // lanes per row
  const int t = threadIdx.x & (T - 1);
  const bool row_ok = row < rows;                        // (wave-uniform; a wave past the last row re-reads it and stores nothing)
  row = row_ok ? row : rows - 1;
  const int64_t v0 = row * nv;
  u32x4 raw[U];
#pragma unroll
  for (int u = 0; u < U; u++) {
    const int v = t + u * T;
    raw[u] = load_raw16<true>(in, (v0 + (v < nv ? v : nv - 1)) * 16);   // clamped: a repeated vector cannot change a maximum
  }
  uint32_t m = 0u;
#pragma unroll
  for (int u = 0; u < U; u++) m = max(m, absmax_bits<DT>(raw[u]));
  m = df_block_max<WAVES>(group_max_u32(m, kWave));
  DfSeg sg;
  sg.setup(m, tb.norm, 0);
  const bool fast = __builtin_amdgcn_ballot_w64(!recip_ok(sg.s)) == 0ull;   // (one segment per wave)
  if (t == 0 && row_ok) sink.seg(row, sg.s);
#pragma unroll
  for (int u = 0; u < U; u++) {
    const int v = t + u * T;
    float x[V], q[V];
    widen<DT, V>(raw[u], x);
    df_quotient_vec<V>(x, q, sg, fast);
    sink.vec(v0 + v, v < nv && row_ok, q, sg.s, tb);
  }
}

// ------------------------------------------------------------------------------------------------ the cast
template <int DT, int U, bool IDX>
__global__ __launch_bounds__(kDynThreads) void cb_group_kernel(const void* __restrict__ in, void* __restrict__ out, int64_t nvec, int lanes,
                                                              int lanes_log2, const float* __restrict__ levels, int K, float norm,
                                                              float* __restrict__ scale_out, uint8_t* __restrict__ index) {
  CbTable tb;
  tb.load(levels, K, norm);
  CbCastSink<DT, IDX> sink{out, index, scale_out};
  cb_group_tile<DT, U>(in, nvec, lanes, lanes_log2, (int64_t)blockIdx.x * kCbWaves + threadIdx.x / kWave, tb, sink);
}

// WAVES = 1: a wave per row, four rows per workgroup; WAVES = 4: the workgroup's row
template <int DT, int U, int WAVES, bool IDX>
__global__ __launch_bounds__(kDynThreads) void cb_rows_kernel(const void* __restrict__ in, void* __restrict__ out, int64_t rows, int nv,
                                                             const float* __restrict__ levels, int K, float norm,
                                                             float* __restrict__ scale_out, uint8_t* __restrict__ index) {
  constexpr int RPB = kCbWaves / WAVES;                  // rows per workgroup
  CbTable tb;
  tb.load(levels, K, norm);
  CbCastSink<DT, IDX> sink{out, index, scale_out};
  cb_row_tile<DT, U, WAVES>(in, rows, nv, (int64_t)blockIdx.x * RPB + threadIdx.x / (kWave * WAVES), tb, sink);
}

// ------------------------------------------------------------------------------------------------ the Lloyd statistics
// the workgroup's accumulators -> part[0 .. 47]: an xor butterfly inside a wave (every lane ends with the same bits), waves in wave order
template <int DT>
__device__ __forceinline__ void cb_block_store(CbAccSink<DT>& a, double* __restrict__ part) {
  __shared__ double s_red[kCbWaves][kCbStats];
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
#pragma unroll
  for (int k = 0; k < kCbMax; k++) {
    double c = (double)a.n[k];   // (a lane sees fewer than 2^32 elements: exact)
    for (int o = 1; o < kWave; o <<= 1) {
      a.wu[k] += __shfl_xor(a.wu[k], o);
      a.w[k] += __shfl_xor(a.w[k], o);
      c += __shfl_xor(c, o);
    }
    if (lane == 0) { s_red[w][k * 3] = a.wu[k]; s_red[w][k * 3 + 1] = a.w[k]; s_red[w][k * 3 + 2] = c; }
  }
  __syncthreads();
  if (threadIdx.x < kCbStats) {
    double p = s_red[0][threadIdx.x];
#pragma unroll
    for (int i = 1; i < kCbWaves; i++) p += s_red[i][threadIdx.x];
    part[threadIdx.x] = p;
  }
}

// workgroup b takes the wave tiles 4 b .. 4 b + 3, then those of workgroup b + grid, ...: the same count of rounds for its four waves
template <int DT, int U>
__global__ __launch_bounds__(kDynThreads) void cb_acc_group_kernel(const void* __restrict__ in, int64_t nvec, int lanes, int lanes_log2,
                                                                  int64_t n_wg_tiles, const float* __restrict__ levels, int K, float norm,
                                                                  double* __restrict__ part) {
  CbTable tb;
  tb.load(levels, K, norm);
  CbAccSink<DT> sink;
  sink.clear();
  for (int64_t b = blockIdx.x; b < n_wg_tiles; b += gridDim.x) cb_group_tile<DT, U>(in, nvec, lanes, lanes_log2, b * kCbWaves + threadIdx.x / kWave, tb, sink);
  cb_block_store<DT>(sink, part + (int64_t)blockIdx.x * kCbStats);
}

template <int DT, int U, int WAVES>
__global__ __launch_bounds__(kDynThreads) void cb_acc_rows_kernel(const void* __restrict__ in, int64_t rows, int nv, int64_t n_wg_tiles,
                                                                 const float* __restrict__ levels, int K, float norm,
                                                                 double* __restrict__ part) {
  constexpr int RPB = kCbWaves / WAVES;
  CbTable tb;
  tb.load(levels, K, norm);
  CbAccSink<DT> sink;
  sink.clear();
  for (int64_t b = blockIdx.x; b < n_wg_tiles; b += gridDim.x) {
    cb_row_tile<DT, U, WAVES>(in, rows, nv, b * RPB + threadIdx.x / (kWave * WAVES), tb, sink);
    if constexpr (WAVES > 1) __syncthreads();            // (df_block_max's LDS words are read before the next row overwrites them)
  }
  cb_block_store<DT>(sink, part + (int64_t)blockIdx.x * kCbStats);
}

// A[k, j] (+)= the partial rows' entries (k, j), k < K: ONE workgroup; the rows are cut into 5 runs of consecutive rows, thread (run, e)
// adds its run in row order, then thread e adds the 5 run sums in run order -- an order that depends on the number of rows alone
constexpr int kCbFoldRuns = 5;
__global__ __launch_bounds__(kDynThreads) void cb_fold_kernel(const double* __restrict__ part, int n_rows, int K, int accumulate,
                                                             double* __restrict__ A) {
  __shared__ double s_run[kCbFoldRuns][kCbStats];
  const int e = threadIdx.x % kCbStats, run = threadIdx.x / kCbStats;
  if (run < kCbFoldRuns) {
    const int q = (n_rows + kCbFoldRuns - 1) / kCbFoldRuns;
    const int r0 = run * q, r1 = r0 + q < n_rows ? r0 + q : n_rows;
    double sum = 0.0;
    for (int r = r0; r < r1; r++) sum += part[(int64_t)r * kCbStats + e];
    s_run[run][e] = sum;
  }
  __syncthreads();
  if (threadIdx.x < K * 3) {
    double total = s_run[0][threadIdx.x];
#pragma unroll
    for (int g = 1; g < kCbFoldRuns; g++) total += s_run[g][threadIdx.x];
    A[threadIdx.x] = accumulate ? A[threadIdx.x] + total : total;
  }
}

// ------------------------------------------------------------------------------------------------ launch plans
struct CbPlan {
  int cls;
  int64_t nv, nvec, wg_tiles;   // vectors per segment, vectors in all (group), workgroup tiles
  int lanes, lanes_log2, U;
  bool deep;
};

// the geometry of (n_segments, S): dynf_launch_segments' rules
inline CbPlan cb_plan(int64_t n_segments, int64_t S, int V, bool whole_rows) {
  CbPlan p{};
  p.cls = dynf_class(S, V, whole_rows);
  if (p.cls == DMXQ_DYN_NONE) return p;
  p.nv = S / V;
  if (p.cls == DMXQ_DYN_GROUP) {
    p.lanes = (int)p.nv;   // 2 .. 64
    while ((1 << p.lanes_log2) < p.lanes) p.lanes_log2++;
    p.nvec = n_segments * p.nv;
    // one vector per lane while that already fills the device, four independent loads per lane beyond (dynamic_quant.hip's rule)
    p.deep = plan_norm(p.nvec) > ((int64_t)1 << 19);
    p.U = p.deep ? 4 : 1;
    const int64_t per_wg = (int64_t)kDynThreads * p.U;
    p.wg_tiles = (p.nvec + per_wg - 1) / per_wg;
    return p;
  }
  const bool wave_row = p.cls != DMXQ_DYN_BLOCK_ROW;
  const int64_t rpb = wave_row ? kCbWaves : 1;
  p.wg_tiles = (n_segments + rpb - 1) / rpb;
  const int64_t T = wave_row ? kWave : kDynThreads;
  const int64_t per_lane = (p.nv + T - 1) / T;
  p.U = per_lane <= 1 ? 1 : per_lane <= 2 ? 2 : per_lane <= 4 ? 4 : per_lane <= 8 ? 8 : 16;
  if (!wave_row && p.U < 8) p.U = 8;
  if (p.U == 16 && V != 4) p.cls = DMXQ_DYN_NONE;   // (not reached: dynf_class sends such sixteen-bit rows to the workgroup form)
  return p;
}

inline int cb_acc_grid(const CbPlan& p) {
  const int64_t most = (int64_t)kCbWgPerCu * plan_cus();
  return (int)(p.wg_tiles < most ? p.wg_tiles : most);
}

template <int DT, bool IDX>
int cb_launch_cast(const CbPlan& p, const void* in, void* out, int64_t n_segments, const float* levels, int K, float norm, float* scale_out,
                   uint8_t* index, hipStream_t s) {
  constexpr int V = 16 / Elem<DT>::bytes;
  const dim3 grid((unsigned)p.wg_tiles), block(kDynThreads);
  if (p.cls == DMXQ_DYN_GROUP) {
    if (p.deep) DMXQ_LAUNCH((cb_group_kernel<DT, 4, IDX>), grid, block, 0, s, in, out, p.nvec, p.lanes, p.lanes_log2, levels, K, norm, scale_out, index);
    else DMXQ_LAUNCH((cb_group_kernel<DT, 1, IDX>), grid, block, 0, s, in, out, p.nvec, p.lanes, p.lanes_log2, levels, K, norm, scale_out, index);
    return launch_status();
  }
#define DMXQ_CB_ROWS(U_, W_) DMXQ_LAUNCH((cb_rows_kernel<DT, U_, W_, IDX>), grid, block, 0, s, in, out, n_segments, (int)p.nv, levels, K, norm, scale_out, index)
  if (p.cls != DMXQ_DYN_BLOCK_ROW) {
    if (p.U == 1) DMXQ_CB_ROWS(1, 1);
    else if (p.U == 2) DMXQ_CB_ROWS(2, 1);
    else if (p.U == 4) DMXQ_CB_ROWS(4, 1);
    else if (p.U == 8) DMXQ_CB_ROWS(8, 1);
    else if constexpr (V == 4) DMXQ_CB_ROWS(16, 1);
    else return DMXQ_ERR_UNSUPPORTED;
  } else {
    if (p.U == 8) DMXQ_CB_ROWS(8, 4);
    else if constexpr (V == 4) DMXQ_CB_ROWS(16, 4);
    else return DMXQ_ERR_UNSUPPORTED;
  }
#undef DMXQ_CB_ROWS
  return launch_status();
}

template <int DT>
int cb_launch_acc(const CbPlan& p, const void* in, int64_t n_segments, const float* levels, int K, float norm, double* A, int accumulate,
                  double* part, hipStream_t s) {
  constexpr int V = 16 / Elem<DT>::bytes;
  const int g = cb_acc_grid(p);
  const dim3 grid((unsigned)g), block(kDynThreads);
  if (p.cls == DMXQ_DYN_GROUP) {
    if (p.deep) DMXQ_LAUNCH((cb_acc_group_kernel<DT, 4>), grid, block, 0, s, in, p.nvec, p.lanes, p.lanes_log2, p.wg_tiles, levels, K, norm, part);
    else DMXQ_LAUNCH((cb_acc_group_kernel<DT, 1>), grid, block, 0, s, in, p.nvec, p.lanes, p.lanes_log2, p.wg_tiles, levels, K, norm, part);
  } else {
#define DMXQ_CB_ACC(U_, W_) DMXQ_LAUNCH((cb_acc_rows_kernel<DT, U_, W_>), grid, block, 0, s, in, n_segments, (int)p.nv, p.wg_tiles, levels, K, norm, part)
    if (p.cls != DMXQ_DYN_BLOCK_ROW) {
      if (p.U == 1) DMXQ_CB_ACC(1, 1);
      else if (p.U == 2) DMXQ_CB_ACC(2, 1);
      else if (p.U == 4) DMXQ_CB_ACC(4, 1);
      else if (p.U == 8) DMXQ_CB_ACC(8, 1);
      else if constexpr (V == 4) DMXQ_CB_ACC(16, 1);
      else return DMXQ_ERR_UNSUPPORTED;
    } else {
      if (p.U == 8) DMXQ_CB_ACC(8, 4);
      else if constexpr (V == 4) DMXQ_CB_ACC(16, 4);
      else return DMXQ_ERR_UNSUPPORTED;
    }
#undef DMXQ_CB_ACC
  }
  DMXQ_LAUNCH(cb_fold_kernel, dim3(1), block, 0, s, (const double*)part, g, K, accumulate, A);
  return launch_status();
}

// the checks the two entries share -> DMXQ_OK when a launch is due; *done: nothing to do (an empty tensor)
inline int cb_check(const void* in, int dtype_in, int mode, int64_t n_segments, int64_t segment, const float* levels, int K, float norm,
                    CbPlan* p, bool* done) {
  *done = false;
  if (!valid_dtype(dtype_in)) return DMXQ_ERR_BAD_ARG;
  if (mode != DMXQ_DYNF_GROUP && mode != DMXQ_DYNF_ROWS) return DMXQ_ERR_BAD_ARG;
  if (n_segments < 0 || segment < 0 || K < 2 || K > 256 || !(norm < INFINITY)) return DMXQ_ERR_BAD_ARG;
  if (n_segments > 0 && segment > 0 && (!in || !levels)) return DMXQ_ERR_BAD_ARG;
  // what the kernels take; everything else is the caller's chain (nothing launched)
  if (K > kCbMax) return DMXQ_ERR_UNSUPPORTED;
  if (n_segments == 0 || segment == 0) { *done = true; return DMXQ_OK; }
  const int V = dtype_in == DMXQ_F32 ? 4 : 8;
  *p = cb_plan(n_segments, segment, V, mode == DMXQ_DYNF_ROWS);
  if (p->cls == DMXQ_DYN_NONE) return DMXQ_ERR_UNSUPPORTED;
  if (!aligned16(in) || (reinterpret_cast<uintptr_t>(levels) & 3u)) return DMXQ_ERR_UNSUPPORTED;
  if (n_segments > INT64_MAX / (segment * 4) || p->wg_tiles > 0x7FFFFFFF) return DMXQ_ERR_UNSUPPORTED;
  return DMXQ_OK;
}

}  // namespace
}  // namespace dmxq

using namespace dmxq;

extern "C" int dmxq_codebook_class(int dtype, int mode, int64_t segment) {
  if (!valid_dtype(dtype) || (mode != DMXQ_DYNF_GROUP && mode != DMXQ_DYNF_ROWS)) return DMXQ_DYN_NONE;
  return dynf_class(segment, dtype == DMXQ_F32 ? 4 : 8, mode == DMXQ_DYNF_ROWS);
}

extern "C" int dmxq_codebook_qdq(const void* in, void* out, int dtype_in, int dtype_out, int mode, int64_t n_segments, int64_t segment,
                                 const float* levels, int K, float norm, float* scale_out, uint8_t* index_out, void* stream) {
  if (!valid_dtype(dtype_out)) return DMXQ_ERR_BAD_ARG;
  CbPlan p{};
  bool done = false;
  const int st = cb_check(in, dtype_in, mode, n_segments, segment, levels, K, norm, &p, &done);
  if (st != DMXQ_OK) return st;
  if (!done && !out) return DMXQ_ERR_BAD_ARG;
  if (dtype_in != dtype_out) return DMXQ_ERR_UNSUPPORTED;
  if (done) return DMXQ_OK;
  if (!aligned16(out) || (index_out && !aligned16(index_out))) return DMXQ_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
#define DMXQ_CB_GO(DT_)                                                                                                    \
  return index_out ? cb_launch_cast<DT_, true>(p, in, out, n_segments, levels, K, norm, scale_out, index_out, s)            \
                   : cb_launch_cast<DT_, false>(p, in, out, n_segments, levels, K, norm, scale_out, nullptr, s)
  if (dtype_in == DMXQ_BF16) DMXQ_CB_GO(DMXQ_BF16);
  if (dtype_in == DMXQ_F16) DMXQ_CB_GO(DMXQ_F16);
  DMXQ_CB_GO(DMXQ_F32);
#undef DMXQ_CB_GO
}

extern "C" int64_t dmxq_codebook_workspace_bytes(int dtype, int mode, int64_t n_segments, int64_t segment) {
  if (!valid_dtype(dtype) || n_segments <= 0 || segment <= 0 || (mode != DMXQ_DYNF_GROUP && mode != DMXQ_DYNF_ROWS)) return 0;
  const CbPlan p = cb_plan(n_segments, segment, dtype == DMXQ_F32 ? 4 : 8, mode == DMXQ_DYNF_ROWS);
  if (p.cls == DMXQ_DYN_NONE || p.wg_tiles > 0x7FFFFFFF) return 0;
  return (int64_t)cb_acc_grid(p) * kCbStats * (int64_t)sizeof(double);
}

extern "C" int dmxq_codebook_accumulate(const void* in, int dtype_in, int mode, int64_t n_segments, int64_t segment, const float* levels,
                                        int K, float norm, double* acc, int accumulate, void* workspace, void* stream) {
  CbPlan p{};
  bool done = false;
  const int st = cb_check(in, dtype_in, mode, n_segments, segment, levels, K, norm, &p, &done);
  if (st != DMXQ_OK) return st;
  if (!acc) return DMXQ_ERR_BAD_ARG;
  if (done) return DMXQ_OK;   // (an empty tensor: nothing launched, acc untouched -- the caller zeroes a fresh acc itself)
  if (!workspace) return DMXQ_ERR_BAD_ARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 7u) || (reinterpret_cast<uintptr_t>(acc) & 7u)) return DMXQ_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (dtype_in == DMXQ_BF16) return cb_launch_acc<DMXQ_BF16>(p, in, n_segments, levels, K, norm, acc, accumulate, (double*)workspace, s);
  if (dtype_in == DMXQ_F16) return cb_launch_acc<DMXQ_F16>(p, in, n_segments, levels, K, norm, acc, accumulate, (double*)workspace, s);
  return cb_launch_acc<DMXQ_F32>(p, in, n_segments, levels, K, norm, acc, accumulate, (double*)workspace, s);
}
