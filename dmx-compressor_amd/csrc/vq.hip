// csrc/vq.hip — vector codebook casts (VQ: GPTVQ / AQLM / QuIP#-style d-dimensional tables) in ONE launch, and the weighted k-means
// statistics that fit a table to a tensor on the device (include/dmxq.h dmxq_vq_qdq, dmxq_vq_accumulate; DESIGN.md §8 "Vector codebook
// casts").  Not in the reference.  d consecutive elements are replaced TOGETHER by one row of a [K, d] table under a per-segment
// absolute-maximum scale: d = 2, K = 256 is 4 bits per weight, d = 4 is 2 bits, d = 8 is 1 bit.
//
// The definition (fp32 throughout, every operation rounded on its own: the build has no fma contraction).  The table: C float32 [K, d],
// finite, 2 <= K <= 256, d in {2, 4, 8}, no order, duplicates allowed.
//   D_k(u) = (((t_0 t_0) + t_1 t_1) + ...) + t_{d-1} t_{d-1},  t_j = u_j - c_kj      (products first, added left to right)
//   z      = the lowest k that minimises D_k(0);   the default norm = max_{k,j} |c_kj|
// Per segment (csrc/codebook.hip's segments; a d-vector never straddles one):
//   amax = max |x|, ONE NaN anywhere makes it NaN;  s = amax / norm (IEEE), s = 1 when s is not finite or below 2^-126   (DfSeg)
//   u    = x / s, the IEEE quotient                                                                          (df_quotient_vec)
//   idx  : best = +Inf, idx = z; for k = 0 .. K-1: if D_k(u) < best then best = D_k, idx = k   -- a tie keeps the lower index; a vector
//          whose distances are all NaN or +Inf (a NaN / Inf component, overflowing squares) takes z
//   y_j  = c[idx][j] * s: ONE fp32 multiply, one rounding to the output dtype.
// The table arrives as a DEVICE pointer; z and the default norm are formed in the kernel, so that a fit loop runs without a host round
// trip: capturable.
//
// The table in the kernel: ONE copy per workgroup in LDS (K d 4 <= 8 KiB), rows padded to a multiple of four with +Inf entries -- a
// padded row's distance is +Inf or NaN, never below `best`, so the search runs four rows per trip for every K.  z and the norm come from
// the workgroup's first wave (a lane per row, a lexicographic (distance, index) butterfly; the maximum on the magnitude bits).  The search
// reads row k with the SAME address in every lane (an LDS broadcast read: no bank conflict) and holds the running (best, idx) of a
// lane's d-vectors in registers; the row loop is the outer one, so that one row read serves a whole batch of a lane's raw vectors (up to
// four 16-byte vectors: up to 16 d-vectors).  The lookup reads the winning row from LDS by index.
//
// Geometry: dynamic_float.hpp's, as csrc/codebook.hip -- segments inside a wave (16 .. 256, a power of two), a wave per row (short_row /
// wave_row), a 256-thread workgroup per row (block_row, up to 16384 elements).  A lane's 16-byte vectors stay RAW in registers between
// the maximum pass and the search; a 16-byte vector holds 16 / (elem d) whole d-vectors, which is why float32 takes d = 2 and 4 only;
// lanes past the end re-read the last vector / row and store (and add) nothing.  Indices leave as ONE 1-, 2- or 4-byte store per lane
// vector.
//
// The k-means statistics (the true-MSE form: a vector's error is s^2 |u - c|^2): float64 A[K][d + 2]; over the d-vectors whose d
// quotients are all finite, A[idx][j] += w u_j, A[idx][d] += w, A[idx][d + 1] += 1 with w = (double)s * (double)s.  s, u and idx come
// from the SAME device functions as the cast.  NO floating-point atomics, and a FIXED order:
//   * thread t of a workgroup owns table row r = 4 (t mod 64) + t / 64 (wave r mod 4, lane r / 4: a small table still spreads over the
//     four waves) and keeps that row's d + 2 sums in registers;
//   * the workgroup takes its tiles in the order b = blockIdx, blockIdx + grid, ...; within a tile the batches of raw vectors in order;
//     a batch is staged in LDS as (idx, s, u) in slots  n 256 + thread  (n: the d-vector's number inside the lane's batch);
//   * every wave walks the slots in ascending order, 64 at a time, and the owner of a slot's row adds it: row r receives its vectors in
//     slot order;
//   * the workgroup writes one partial [K][d + 2] block; a second small launch adds the blocks in workgroup order 0, 1, 2, ...
// The grid is a function of the geometry and the device's CU count alone, so the same input gives the same bits.
#include <math.h>

#include "dynamic_float.hpp"

namespace dmxq {
namespace {

constexpr int kVqMaxK = 256;
constexpr int kVqMaxWords = 2048;             // K4 d floats: 8 KiB
constexpr int kVqWaves = kDynThreads / kWave;
constexpr int kVqBatch = 4;                   // raw vectors of a lane that share one walk over the table (the cast)
constexpr int kVqWgPerCu = 2;                 // the largest accumulate grid: 2 workgroups on every CU (common.hpp plan_cus)
constexpr uint32_t kVqSkip = 0xFFFFFFFFu;     // a staged slot that adds nothing

struct VqTable {
  float c[kVqMaxWords];
  float norm;
  uint32_t z;
};

// the workgroup's copy of the table, z and the norm (two barriers; every thread of the workgroup calls it once) -> wave-uniform norm, z
template <int D>
__device__ __forceinline__ void vq_table_load(VqTable& tb, const float* __restrict__ table, int K, float norm_arg, float& norm, uint32_t& z) {
  const int K4 = (K + 3) & ~3;
  for (int e = threadIdx.x; e < K4 * D; e += kDynThreads) tb.c[e] = e < K * D ? table[e] : INFINITY;
  __syncthreads();
  if (threadIdx.x < kWave) {   // (the first wave, whole)
    const int lane = threadIdx.x;
    uint32_t m = 0u;
    for (int e = lane; e < K * D; e += kWave) m = max(m, f2u(tb.c[e]) & 0x7FFFFFFFu);
    m = group_max_u32(m, kWave);
    float best = INFINITY;
    uint32_t bi = 0x7FFFFFFFu;
    for (int k = lane; k < K; k += kWave) {
      float acc = 0.0f;
#pragma unroll
      for (int j = 0; j < D; j++) {
        const float t = 0.0f - tb.c[k * D + j];
        const float p = t * t;
        acc = j == 0 ? p : acc + p;
      }
      const bool lt = acc < best || (acc == best && (uint32_t)k < bi);
      best = lt ? acc : best;
      bi = lt ? (uint32_t)k : bi;
    }
    for (int o = 1; o < kWave; o <<= 1) {
      const float ob = __shfl_xor(best, o);
      const uint32_t oi = (uint32_t)__shfl_xor((int)bi, o);
      const bool lt = ob < best || (ob == best && oi < bi);
      best = lt ? ob : best;
      bi = lt ? oi : bi;
    }
    if (lane == 0) {
      tb.norm = norm_arg > 0.0f ? norm_arg : u2f(m);
      tb.z = bi;
    }
  }
  __syncthreads();
  norm = u2f((uint32_t)__builtin_amdgcn_readfirstlane((int)f2u(tb.norm)));
  z = (uint32_t)__builtin_amdgcn_readfirstlane((int)tb.z);
}

// the row choice for the B x V / D d-vectors of a batch: the rows are the outer loop, four per trip (padded rows never win)
template <int D, int B, int V>
__device__ __forceinline__ void vq_search(const VqTable& tb, int K, uint32_t z, const float (&u)[B][V], uint32_t (&idx)[B][V / D]) {
  constexpr int P = V / D;
  float best[B][P];
#pragma unroll
  for (int b = 0; b < B; b++) {
#pragma unroll
    for (int n = 0; n < P; n++) { best[b][n] = INFINITY; idx[b][n] = z; }
  }
  const int K4 = (K + 3) & ~3;
  for (int k = 0; k < K4; k += 4) {
#pragma unroll
    for (int kk = 0; kk < 4; kk++) {
      float c[D];
#pragma unroll
      for (int j = 0; j < D; j++) c[j] = tb.c[(k + kk) * D + j];
#pragma unroll
      for (int b = 0; b < B; b++) {
#pragma unroll
        for (int n = 0; n < P; n++) {
          float acc = 0.0f;
#pragma unroll
          for (int j = 0; j < D; j++) {
            const float t = u[b][n * D + j] - c[j];
            const float p = t * t;
            acc = j == 0 ? p : acc + p;
          }
          const bool lt = acc < best[b][n];
          best[b][n] = lt ? acc : best[b][n];
          idx[b][n] = lt ? (uint32_t)(k + kk) : idx[b][n];
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ the two uses of a batch
// A sink receives every batch of B lane vectors once their scales are known: vector indices i (`live`: inside the tensor; a lane past the
// end holds a repeated vector), the quotients u, the scales.  seg(): once per segment, from one lane that holds its first vector.  Every
// thread of the workgroup calls batch() the same number of times (the statistics sink has barriers inside).
template <int DT, int D>
struct VqCastSink {
  static constexpr int V = 16 / Elem<DT>::bytes, P = V / D;
  void* out;
  uint8_t* index;
  float* scale_out;
  template <int B>
  __device__ __forceinline__ void batch(const int64_t (&i)[B], const bool (&live)[B], const float (&u)[B][V], const float (&s)[B],
                                        const VqTable& tb, int K, uint32_t z) {
    uint32_t id[B][P];
    vq_search<D, B, V>(tb, K, z, u, id);
#pragma unroll
    for (int b = 0; b < B; b++) {
      float y[V];
#pragma unroll
      for (int n = 0; n < P; n++) {
#pragma unroll
        for (int j = 0; j < D; j++) y[n * D + j] = tb.c[id[b][n] * D + j] * s[b];
      }
      if (live[b]) {
        store_vec<DT, V>(out, i[b] * V, y);
        if (index) {
          if constexpr (P == 4) *(uint32_t*)(index + i[b] * 4) = id[b][0] | (id[b][1] << 8) | (id[b][2] << 16) | (id[b][3] << 24);
          else if constexpr (P == 2) *(uint16_t*)(index + i[b] * 2) = (uint16_t)(id[b][0] | (id[b][1] << 8));
          else index[i[b]] = (uint8_t)id[b][0];
        }
      }
    }
  }
  __device__ __forceinline__ void seg(int64_t segment, float s) {
    if (scale_out) scale_out[segment] = s;
  }
};

// the staged batch of the statistics: slot n 256 + thread
template <int D, int N>
struct VqStage {
  uint32_t idx[N * kDynThreads];
  float s[N * kDynThreads];
  float u[D][N * kDynThreads];
};

template <int DT, int D, int BA>
struct VqAccSink {
  static constexpr int V = 16 / Elem<DT>::bytes, P = V / D, N = BA * P;
  VqStage<D, N>* st;
  double a[D + 1];
  uint32_t n;
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int j = 0; j <= D; j++) a[j] = 0.0;
    n = 0u;
  }
  template <int B>
  __device__ __forceinline__ void batch(const int64_t (&)[B], const bool (&live)[B], const float (&u)[B][V], const float (&s)[B],
                                        const VqTable& tb, int K, uint32_t z) {
    static_assert(B == BA, "the stage is sized for the batch");
    uint32_t id[B][P];
    vq_search<D, B, V>(tb, K, z, u, id);
#pragma unroll
    for (int b = 0; b < B; b++) {
#pragma unroll
      for (int p = 0; p < P; p++) {
        bool use = live[b];
#pragma unroll
        for (int j = 0; j < D; j++) use = use && __builtin_fabsf(u[b][p * D + j]) < INFINITY;   // (a NaN compares false)
        const int slot = (b * P + p) * kDynThreads + threadIdx.x;
        st->idx[slot] = use ? id[b][p] : kVqSkip;
        st->s[slot] = s[b];
#pragma unroll
        for (int j = 0; j < D; j++) st->u[j][slot] = u[b][p * D + j];
      }
    }
    __syncthreads();
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = threadIdx.x / kWave;
    for (int base = 0; base < N * kDynThreads; base += kWave) {
      const uint32_t mine = st->idx[base + lane];
      uint64_t mask = __builtin_amdgcn_ballot_w64(mine != kVqSkip && (mine & 3u) == wave);
      while (mask) {   // (wave-uniform: the slots of this wave's rows, ascending)
        const int bit = __builtin_ctzll(mask);
        mask &= mask - 1;
        const uint32_t row = (uint32_t)__builtin_amdgcn_readlane((int)mine, bit);
        const bool hit = (uint32_t)lane == (row >> 2);
        const float sf = st->s[base + bit];
        const double w = (double)sf * (double)sf;
#pragma unroll
        for (int j = 0; j < D; j++) {
          const double t = w * (double)st->u[j][base + bit];
          a[j] += hit ? t : 0.0;
        }
        a[D] += hit ? w : 0.0;
        n += hit ? 1u : 0u;
      }
    }
    __syncthreads();   // (the stage is read completely before the next batch overwrites it)
  }
  __device__ __forceinline__ void seg(int64_t, float) {}
  // the thread's row -> the workgroup's partial block [K][D + 2]
  __device__ __forceinline__ void store(double* __restrict__ part, int K) const {
    const int row = 4 * (int)(threadIdx.x & (kWave - 1)) + (int)(threadIdx.x / kWave);
    if (row < K) {
      double* p = part + (int64_t)row * (D + 2);
#pragma unroll
      for (int j = 0; j <= D; j++) p[j] = a[j];
      p[D + 1] = (double)n;   // (a thread sees fewer than 2^32 vectors: exact)
    }
  }
};

// ------------------------------------------------------------------------------------------------ tiles
// segments of `lanes` adjacent lanes; nvec = n_segments * lanes vectors in all; wave `wave` takes vectors [wave U 64, (wave + 1) U 64)
template <int DT, int U, int B, class SINK>
__device__ __forceinline__ void vq_group_tile(const void* __restrict__ in, int64_t nvec, int lanes, int lanes_log2, int64_t wave,
                                              const VqTable& tb, int K, float norm, uint32_t z, SINK& sink) {
  constexpr int V = 16 / Elem<DT>::bytes;
  static_assert(U % B == 0, "whole batches");
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t base = wave * (U * kWave) + lane;
  u32x4 raw[U];
#pragma unroll
  for (int u = 0; u < U; u++) {
    const int64_t i = base + (int64_t)u * kWave;
    raw[u] = load_raw16<true>(in, (i < nvec ? i : nvec - 1) * 16);
  }
#pragma unroll
  for (int u0 = 0; u0 < U; u0 += B) {
    float q[B][V], s[B];
    int64_t ii[B];
    bool live[B];
#pragma unroll
    for (int b = 0; b < B; b++) {
      ii[b] = base + (int64_t)(u0 + b) * kWave;
      DfSeg sg;
      sg.setup(group_max_u32(absmax_bits<DT>(raw[u0 + b]), lanes), norm, 0);
      const bool fast = __builtin_amdgcn_ballot_w64(!recip_ok(sg.s)) == 0ull;
      float x[V];
      widen<DT, V>(raw[u0 + b], x);
      df_quotient_vec<V>(x, q[b], sg, fast);
      s[b] = sg.s;
      live[b] = ii[b] < nvec;
      if (live[b] && (lane & (lanes - 1)) == 0) sink.seg(ii[b] >> lanes_log2, sg.s);
    }
    sink.batch(ii, live, q, s, tb, K, z);
  }
}

// row `row` of nv vectors; WAVES = 1: a wave's row; WAVES = 4: the workgroup's row (one barrier).  U x 64 x WAVES >= nv.
template <int DT, int U, int B, int WAVES, class SINK>
__device__ __forceinline__ void vq_row_tile(const void* __restrict__ in, int64_t rows, int nv, int64_t row, const VqTable& tb, int K,
                                            float norm, uint32_t z, SINK& sink) {
  constexpr int V = 16 / Elem<DT>::bytes;
  constexpr int T = kWave * WAVES;                       // lanes per row
  static_assert(U % B == 0, "whole batches");
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
  sg.setup(m, norm, 0);
  const bool fast = __builtin_amdgcn_ballot_w64(!recip_ok(sg.s)) == 0ull;   // (one segment per wave)
  if (t == 0 && row_ok) sink.seg(row, sg.s);
#pragma unroll
  for (int u0 = 0; u0 < U; u0 += B) {
    float q[B][V], s[B];
    int64_t ii[B];
    bool live[B];
#pragma unroll
    for (int b = 0; b < B; b++) {
      const int v = t + (u0 + b) * T;
      float x[V];
      widen<DT, V>(raw[u0 + b], x);
      df_quotient_vec<V>(x, q[b], sg, fast);
      s[b] = sg.s;
      ii[b] = v0 + v;
      live[b] = v < nv && row_ok;
    }
    sink.batch(ii, live, q, s, tb, K, z);
  }
}

constexpr int vq_cast_batch(int U) { return U < kVqBatch ? U : kVqBatch; }
// the statistics stage at most four d-vectors per thread and batch, two at d = 8 (four kept 250 registers live): 12 .. 24 KiB of LDS
constexpr int vq_acc_batch(int U, int P, int D) {
  const int cap = D == 8 ? 2 : 4, b = cap / P < 1 ? 1 : cap / P;
  return b < U ? b : U;
}

// ------------------------------------------------------------------------------------------------ the cast
template <int DT, int D, int U>
__global__ __launch_bounds__(kDynThreads) void vq_group_kernel(const void* __restrict__ in, void* __restrict__ out, int64_t nvec, int lanes,
                                                              int lanes_log2, const float* __restrict__ table, int K, float norm_arg,
                                                              float* __restrict__ scale_out, uint8_t* __restrict__ index) {
  __shared__ VqTable tb;
  float norm;
  uint32_t z;
  vq_table_load<D>(tb, table, K, norm_arg, norm, z);
  VqCastSink<DT, D> sink{out, index, scale_out};
  vq_group_tile<DT, U, vq_cast_batch(U)>(in, nvec, lanes, lanes_log2, (int64_t)blockIdx.x * kVqWaves + threadIdx.x / kWave, tb, K, norm, z, sink);
}

// WAVES = 1: a wave per row, four rows per workgroup; WAVES = 4: the workgroup's row
template <int DT, int D, int U, int WAVES>
__global__ __launch_bounds__(kDynThreads) void vq_rows_kernel(const void* __restrict__ in, void* __restrict__ out, int64_t rows, int nv,
                                                             const float* __restrict__ table, int K, float norm_arg,
                                                             float* __restrict__ scale_out, uint8_t* __restrict__ index) {
  constexpr int RPB = kVqWaves / WAVES;                  // rows per workgroup
  __shared__ VqTable tb;
  float norm;
  uint32_t z;
  vq_table_load<D>(tb, table, K, norm_arg, norm, z);
  VqCastSink<DT, D> sink{out, index, scale_out};
  vq_row_tile<DT, U, vq_cast_batch(U), WAVES>(in, rows, nv, (int64_t)blockIdx.x * RPB + threadIdx.x / (kWave * WAVES), tb, K, norm, z, sink);
}

// ------------------------------------------------------------------------------------------------ the k-means statistics
// workgroup b takes the wave tiles 4 b .. 4 b + 3, then those of workgroup b + grid, ...: the same count of rounds for its four waves
template <int DT, int D, int U>
__global__ __launch_bounds__(kDynThreads) void vq_acc_group_kernel(const void* __restrict__ in, int64_t nvec, int lanes, int lanes_log2,
                                                                  int64_t n_wg_tiles, const float* __restrict__ table, int K, float norm_arg,
                                                                  double* __restrict__ part) {
  constexpr int BA = vq_acc_batch(U, 16 / Elem<DT>::bytes / D, D);
  __shared__ VqTable tb;
  __shared__ VqStage<D, VqAccSink<DT, D, BA>::N> stage;
  float norm;
  uint32_t z;
  vq_table_load<D>(tb, table, K, norm_arg, norm, z);
  VqAccSink<DT, D, BA> sink;
  sink.st = &stage;
  sink.clear();
  for (int64_t b = blockIdx.x; b < n_wg_tiles; b += gridDim.x)
    vq_group_tile<DT, U, BA>(in, nvec, lanes, lanes_log2, b * kVqWaves + threadIdx.x / kWave, tb, K, norm, z, sink);
  sink.store(part + (int64_t)blockIdx.x * K * (D + 2), K);
}

template <int DT, int D, int U, int WAVES>
__global__ __launch_bounds__(kDynThreads) void vq_acc_rows_kernel(const void* __restrict__ in, int64_t rows, int nv, int64_t n_wg_tiles,
                                                                 const float* __restrict__ table, int K, float norm_arg,
                                                                 double* __restrict__ part) {
  constexpr int RPB = kVqWaves / WAVES;
  constexpr int BA = vq_acc_batch(U, 16 / Elem<DT>::bytes / D, D);
  __shared__ VqTable tb;
  __shared__ VqStage<D, VqAccSink<DT, D, BA>::N> stage;
  float norm;
  uint32_t z;
  vq_table_load<D>(tb, table, K, norm_arg, norm, z);
  VqAccSink<DT, D, BA> sink;
  sink.st = &stage;
  sink.clear();
  for (int64_t b = blockIdx.x; b < n_wg_tiles; b += gridDim.x)   // (the batches' barriers also keep df_block_max's LDS words apart)
    vq_row_tile<DT, U, BA, WAVES>(in, rows, nv, b * RPB + threadIdx.x / (kWave * WAVES), tb, K, norm, z, sink);
  sink.store(part + (int64_t)blockIdx.x * K * (D + 2), K);
}

// A[e] (+)= the partial blocks' entries e, e < K (d + 2): a thread per entry adds the blocks in workgroup order 0, 1, 2, ...
__global__ __launch_bounds__(kDynThreads) void vq_fold_kernel(const double* __restrict__ part, int n_blocks, int entries, int accumulate,
                                                             double* __restrict__ A) {
  const int e = blockIdx.x * kDynThreads + threadIdx.x;
  if (e >= entries) return;
  double total = 0.0;
  for (int b = 0; b < n_blocks; b++) total += part[(int64_t)b * entries + e];
  A[e] = accumulate ? A[e] + total : total;
}

// ------------------------------------------------------------------------------------------------ launch plans
struct VqPlan {
  int cls;
  int64_t nv, nvec, wg_tiles;   // vectors per segment, vectors in all (group), workgroup tiles
  int lanes, lanes_log2, U;
  bool deep;
};

inline int vq_geometry(int64_t S, int V, int dim, int K, bool whole_rows) {
  if ((dim != 2 && dim != 4 && dim != 8) || V % dim != 0 || K < 2 || K > kVqMaxK) return DMXQ_DYN_NONE;
  return dynf_class(S, V, whole_rows);
}

// the geometry of (n_segments, S): csrc/codebook.hip's rules
inline VqPlan vq_plan(int64_t n_segments, int64_t S, int V, int dim, int K, bool whole_rows) {
  VqPlan p{};
  p.cls = vq_geometry(S, V, dim, K, whole_rows);
  if (p.cls == DMXQ_DYN_NONE) return p;
  p.nv = S / V;
  if (p.cls == DMXQ_DYN_GROUP) {
    p.lanes = (int)p.nv;   // 2 .. 64
    while ((1 << p.lanes_log2) < p.lanes) p.lanes_log2++;
    p.nvec = n_segments * p.nv;
    // one vector per lane while that already fills the device, four per lane beyond: one walk over the table then serves four vectors
    p.deep = plan_norm(p.nvec) > ((int64_t)1 << 18);
    p.U = p.deep ? 4 : 1;
    const int64_t per_wg = (int64_t)kDynThreads * p.U;
    p.wg_tiles = (p.nvec + per_wg - 1) / per_wg;
    return p;
  }
  const bool wave_row = p.cls != DMXQ_DYN_BLOCK_ROW;
  const int64_t rpb = wave_row ? kVqWaves : 1;
  p.wg_tiles = (n_segments + rpb - 1) / rpb;
  const int64_t T = wave_row ? kWave : kDynThreads;
  const int64_t per_lane = (p.nv + T - 1) / T;
  p.U = per_lane <= 1 ? 1 : per_lane <= 2 ? 2 : per_lane <= 4 ? 4 : per_lane <= 8 ? 8 : 16;
  if (!wave_row && p.U < 8) p.U = 8;
  if (p.U == 16 && V != 4) p.cls = DMXQ_DYN_NONE;   // (not reached: dynf_class sends such sixteen-bit rows to the workgroup form)
  return p;
}

inline int vq_acc_grid(const VqPlan& p) {
  const int64_t most = (int64_t)kVqWgPerCu * plan_cus();
  return (int)(p.wg_tiles < most ? p.wg_tiles : most);
}

template <int DT, int D>
int vq_launch_cast(const VqPlan& p, const void* in, void* out, int64_t n_segments, const float* table, int K, float norm, float* scale_out,
                   uint8_t* index, hipStream_t s) {
  constexpr int V = 16 / Elem<DT>::bytes;
  const dim3 grid((unsigned)p.wg_tiles), block(kDynThreads);
  if (p.cls == DMXQ_DYN_GROUP) {
    if (p.deep) DMXQ_LAUNCH((vq_group_kernel<DT, D, 4>), grid, block, 0, s, in, out, p.nvec, p.lanes, p.lanes_log2, table, K, norm, scale_out, index);
    else DMXQ_LAUNCH((vq_group_kernel<DT, D, 1>), grid, block, 0, s, in, out, p.nvec, p.lanes, p.lanes_log2, table, K, norm, scale_out, index);
    return launch_status();
  }
#define DMXQ_VQ_ROWS(U_, W_) DMXQ_LAUNCH((vq_rows_kernel<DT, D, U_, W_>), grid, block, 0, s, in, out, n_segments, (int)p.nv, table, K, norm, scale_out, index)
  if (p.cls != DMXQ_DYN_BLOCK_ROW) {
    if (p.U == 1) DMXQ_VQ_ROWS(1, 1);
    else if (p.U == 2) DMXQ_VQ_ROWS(2, 1);
    else if (p.U == 4) DMXQ_VQ_ROWS(4, 1);
    else if (p.U == 8) DMXQ_VQ_ROWS(8, 1);
    else if constexpr (V == 4) DMXQ_VQ_ROWS(16, 1);
    else return DMXQ_ERR_UNSUPPORTED;
  } else {
    if (p.U == 8) DMXQ_VQ_ROWS(8, 4);
    else if constexpr (V == 4) DMXQ_VQ_ROWS(16, 4);
    else return DMXQ_ERR_UNSUPPORTED;
  }
#undef DMXQ_VQ_ROWS
  return launch_status();
}

template <int DT, int D>
int vq_launch_acc(const VqPlan& p, const void* in, int64_t n_segments, const float* table, int K, float norm, double* A, int accumulate,
                  double* part, hipStream_t s) {
  constexpr int V = 16 / Elem<DT>::bytes;
  const int g = vq_acc_grid(p);
  const dim3 grid((unsigned)g), block(kDynThreads);
  if (p.cls == DMXQ_DYN_GROUP) {
    if (p.deep) DMXQ_LAUNCH((vq_acc_group_kernel<DT, D, 4>), grid, block, 0, s, in, p.nvec, p.lanes, p.lanes_log2, p.wg_tiles, table, K, norm, part);
    else DMXQ_LAUNCH((vq_acc_group_kernel<DT, D, 1>), grid, block, 0, s, in, p.nvec, p.lanes, p.lanes_log2, p.wg_tiles, table, K, norm, part);
  } else {
#define DMXQ_VQ_ACC(U_, W_) DMXQ_LAUNCH((vq_acc_rows_kernel<DT, D, U_, W_>), grid, block, 0, s, in, n_segments, (int)p.nv, p.wg_tiles, table, K, norm, part)
    if (p.cls != DMXQ_DYN_BLOCK_ROW) {
      if (p.U == 1) DMXQ_VQ_ACC(1, 1);
      else if (p.U == 2) DMXQ_VQ_ACC(2, 1);
      else if (p.U == 4) DMXQ_VQ_ACC(4, 1);
      else if (p.U == 8) DMXQ_VQ_ACC(8, 1);
      else if constexpr (V == 4) DMXQ_VQ_ACC(16, 1);
      else return DMXQ_ERR_UNSUPPORTED;
    } else {
      if (p.U == 8) DMXQ_VQ_ACC(8, 4);
      else if constexpr (V == 4) DMXQ_VQ_ACC(16, 4);
      else return DMXQ_ERR_UNSUPPORTED;
    }
#undef DMXQ_VQ_ACC
  }
  const int entries = K * (D + 2);
  DMXQ_LAUNCH(vq_fold_kernel, dim3((unsigned)((entries + kDynThreads - 1) / kDynThreads)), block, 0, s, (const double*)part, g, entries, accumulate, A);
  return launch_status();
}

// the checks the two entries share -> DMXQ_OK when a launch is due; *done: nothing to do (an empty tensor)
inline int vq_check(const void* in, int dtype_in, int mode, int64_t n_segments, int64_t segment, const float* table, int dim, int K,
                    float norm, VqPlan* p, bool* done) {
  *done = false;
  if (!valid_dtype(dtype_in)) return DMXQ_ERR_BAD_ARG;
  if (mode != DMXQ_DYNF_GROUP && mode != DMXQ_DYNF_ROWS) return DMXQ_ERR_BAD_ARG;
  if (dim != 2 && dim != 4 && dim != 8) return DMXQ_ERR_BAD_ARG;
  if (n_segments < 0 || segment < 0 || segment % dim != 0 || K < 2 || K > kVqMaxK || !(norm < INFINITY)) return DMXQ_ERR_BAD_ARG;
  if (n_segments > 0 && segment > 0 && (!in || !table)) return DMXQ_ERR_BAD_ARG;
  if (n_segments == 0 || segment == 0) { *done = true; return DMXQ_OK; }
  // what the kernels take; everything else is the caller's chain (nothing launched)
  const int V = dtype_in == DMXQ_F32 ? 4 : 8;
  *p = vq_plan(n_segments, segment, V, dim, K, mode == DMXQ_DYNF_ROWS);
  if (p->cls == DMXQ_DYN_NONE) return DMXQ_ERR_UNSUPPORTED;
  if (!aligned16(in) || (reinterpret_cast<uintptr_t>(table) & 3u)) return DMXQ_ERR_UNSUPPORTED;
  if (n_segments > INT64_MAX / (segment * 4) || p->wg_tiles > 0x7FFFFFFF) return DMXQ_ERR_UNSUPPORTED;
  return DMXQ_OK;
}

}  // namespace
}  // namespace dmxq

using namespace dmxq;

extern "C" int dmxq_vq_class(int dtype, int mode, int64_t segment, int dim, int K) {
  if (!valid_dtype(dtype) || (mode != DMXQ_DYNF_GROUP && mode != DMXQ_DYNF_ROWS)) return DMXQ_DYN_NONE;
  return vq_geometry(segment, dtype == DMXQ_F32 ? 4 : 8, dim, K, mode == DMXQ_DYNF_ROWS);
}

// (the float32 kernels exist for d = 2 and 4: vq_plan refuses d = 8 before a launch is chosen)
#define DMXQ_VQ_DISPATCH(FN_, ...)                                                                                    \
  do {                                                                                                                 \
    if (dtype_in == DMXQ_BF16) {                                                                                       \
      if (dim == 2) return FN_<DMXQ_BF16, 2>(__VA_ARGS__);                                                             \
      if (dim == 4) return FN_<DMXQ_BF16, 4>(__VA_ARGS__);                                                             \
      return FN_<DMXQ_BF16, 8>(__VA_ARGS__);                                                                           \
    }                                                                                                                  \
    if (dtype_in == DMXQ_F16) {                                                                                        \
      if (dim == 2) return FN_<DMXQ_F16, 2>(__VA_ARGS__);                                                              \
      if (dim == 4) return FN_<DMXQ_F16, 4>(__VA_ARGS__);                                                              \
      return FN_<DMXQ_F16, 8>(__VA_ARGS__);                                                                            \
    }                                                                                                                  \
    if (dim == 2) return FN_<DMXQ_F32, 2>(__VA_ARGS__);                                                                \
    if (dim == 4) return FN_<DMXQ_F32, 4>(__VA_ARGS__);                                                                \
    return DMXQ_ERR_UNSUPPORTED;                                                                                       \
  } while (0)

extern "C" int dmxq_vq_qdq(const void* in, void* out, int dtype_in, int dtype_out, int mode, int64_t n_segments, int64_t segment,
                           const float* table, int dim, int K, float norm, float* scale_out, uint8_t* index_out, void* stream) {
  if (!valid_dtype(dtype_out)) return DMXQ_ERR_BAD_ARG;
  VqPlan p{};
  bool done = false;
  const int st = vq_check(in, dtype_in, mode, n_segments, segment, table, dim, K, norm, &p, &done);
  if (st != DMXQ_OK) return st;
  if (!done && !out) return DMXQ_ERR_BAD_ARG;
  if (dtype_in != dtype_out) return DMXQ_ERR_UNSUPPORTED;
  if (done) return DMXQ_OK;
  if (!aligned16(out) || (index_out && !aligned16(index_out))) return DMXQ_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  DMXQ_VQ_DISPATCH(vq_launch_cast, p, in, out, n_segments, table, K, norm, scale_out, index_out, s);
}

extern "C" int64_t dmxq_vq_workspace_bytes(int dtype, int mode, int64_t n_segments, int64_t segment, int dim, int K) {
  if (!valid_dtype(dtype) || n_segments <= 0 || segment <= 0 || (mode != DMXQ_DYNF_GROUP && mode != DMXQ_DYNF_ROWS)) return 0;
  const VqPlan p = vq_plan(n_segments, segment, dtype == DMXQ_F32 ? 4 : 8, dim, K, mode == DMXQ_DYNF_ROWS);
  if (p.cls == DMXQ_DYN_NONE || p.wg_tiles > 0x7FFFFFFF) return 0;
  return (int64_t)vq_acc_grid(p) * K * (dim + 2) * (int64_t)sizeof(double);
}

extern "C" int dmxq_vq_accumulate(const void* in, int dtype_in, int mode, int64_t n_segments, int64_t segment, const float* table, int dim,
                                  int K, float norm, double* acc, int accumulate, void* workspace, void* stream) {
  VqPlan p{};
  bool done = false;
  const int st = vq_check(in, dtype_in, mode, n_segments, segment, table, dim, K, norm, &p, &done);
  if (st != DMXQ_OK) return st;
  if (!acc) return DMXQ_ERR_BAD_ARG;
  if (done) return DMXQ_OK;   // (an empty tensor: nothing launched, acc untouched -- the caller zeroes a fresh acc itself)
  if (!workspace) return DMXQ_ERR_BAD_ARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 7u) || (reinterpret_cast<uintptr_t>(acc) & 7u)) return DMXQ_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  double* part = (double*)workspace;
  DMXQ_VQ_DISPATCH(vq_launch_acc, p, in, n_segments, table, K, norm, acc, accumulate, part, s);
}
