// csrc/wanda.hip — Wanda (Sun et al., 2023): activation-aware N:M pruning calibrated on the device, for gfx950.
//
// Definition (DESIGN.md §8 "Wanda"; not in the reference).  For a Linear weight W[rows, L] and calibration inputs X[n_tokens, L]:
//   sumsq[j]  = sum_t (double)X[t, j]^2       float64, over every observed batch       -> dmxq_channel_sumsq_accumulate
//   act_norm  = (float)sqrt(sumsq)            one rounding to fp32; a [L] vector, formed by the caller
//   score     = |(float)W| * act_norm         ONE fp32 multiply per element             -> dmxq_wanda_nm
//   mask, y   = the N:M rule of csrc/nm_mask.hip on that score, y = W * mask (a real multiply)
// The score never has to exist in memory: dmxq_wanda_nm forms it in registers from the weight and the L2-resident norm vector and
// ranks it with the key / rank code of nm_rank.hpp (the same code nm_mask.hip runs on a stored score).
//
// The sums use no floating-point atomics and a fixed order (the rule of csrc/error_stats.hip): a channel's rows are added in index
// order inside a slab of rows, the slabs in slab order, and the slab partition is a function of (rows, C) alone -- the same batches
// in the same order give the same bits, whatever the dtype, the alignment or the form (vector / scalar loads) of the launch.  (The slabs
// are folded as 8 runs of consecutive slabs, each in slab order, and the runs in run order: see channel_sumsq_fold_kernel.)
#include "nm_rank.hpp"

namespace dmxq {

// ---------------------------------------------------------------------------------------------------------
// The slab partition of [rows, C]: a function of the shape ALONE (neither the dtype, nor the device, nor the alignment), because it
// IS the order of the sum.  At least 32 rows per slab (the partials then cost at most 1/8 of the bytes of a 16-bit input, written
// once and read once), and about 2048 waves of 512 channels over the launch (two per SIMD on 256 compute units, each with 16 rows of
// 16-byte loads in flight): [8192, 4096] -> 256 slabs of 32 rows, [8192, 14336] -> 73 slabs of 113, [2048, 768] -> 64 slabs of 32.
struct SumsqPlan { int64_t rows_per_slab, n_slabs; };
constexpr int kSumsqMinRows = 32, kSumsqWaves = 2048, kSumsqTileChannels = 512;
inline SumsqPlan sumsq_plan(int64_t rows, int64_t C) {
  if (rows <= 0 || C <= 0) return SumsqPlan{1, 0};
  const int64_t tiles = (C + kSumsqTileChannels - 1) / kSumsqTileChannels;
  int64_t slabs = kSumsqWaves / tiles;
  if (slabs < 1) slabs = 1;
  const int64_t most = (rows + kSumsqMinRows - 1) / kSumsqMinRows;
  if (slabs > most) slabs = most;
  const int64_t rps = (rows + slabs - 1) / slabs;
  return SumsqPlan{rps, (rows + rps - 1) / rps};
}

constexpr int kSumsqRowsInFlight = 16;

// A wave owns 64 lane-columns of one slab; a lane owns VEC consecutive channels (one 16-byte vector: 8 sixteen-bit or 4 fp32
// elements; VEC == 1: the generic form, one channel and scalar loads) and walks the rows of its slab in index order with one fp64
// fma accumulator per channel: fma((double)x, (double)x, acc) adds the EXACT square (a product of two fp32 values fits a double) with
// one rounding, which is what x.double().pow(2) summed row by row does.  16 rows are loaded before the first is used (raw vectors:
// four registers a row; widened when they are added).  Consecutive waves take neighbouring column tiles of the same slab, so a
// workgroup reads four contiguous kilobytes of every row.
//
// TERM: what a row adds to its channel -- the one kernel body serves dmxq_channel_sumsq_accumulate (the square: Wanda) and
// dmxq_channel_sumabs_accumulate (|x|, exact in a double as well: AWQ, csrc/awq.hip), with the same partition, order and lane forms.
constexpr int kTermSquare = 0, kTermAbs = 1;
template <int TERM>
__device__ __forceinline__ double channel_term_add(float x, double acc) {
  const double d = (double)x;
  if constexpr (TERM == kTermAbs) return acc + __builtin_fabs(d);
  else return __builtin_fma(d, d, acc);
}

template <int DT, int VEC, int TERM>
__global__ __launch_bounds__(kThreads) void channel_sumsq_slab_kernel(const void* __restrict__ in, int64_t rows, int64_t C, int64_t n_cols /* lane-columns */,
                                                                      int64_t n_tiles, int64_t rows_per_slab, int64_t n_slabs,
                                                                      double* __restrict__ partial) {
  const int64_t wave = (int64_t)blockIdx.x * (kThreads / kWave) + (threadIdx.x / kWave);
  const int64_t slab = wave / n_tiles, tile = wave - slab * n_tiles;
  if (slab >= n_slabs) return;
  const int64_t col = tile * kWave + (threadIdx.x % kWave);
  if (col >= n_cols) return;
  const int64_t r0 = slab * rows_per_slab;
  const int64_t r1 = r0 + rows_per_slab < rows ? r0 + rows_per_slab : rows;
  const int64_t c0 = col * VEC;
  double acc[VEC];
#pragma unroll
  for (int k = 0; k < VEC; k++) acc[k] = 0.0;
  for (int64_t r = r0; r < r1; r += kSumsqRowsInFlight) {
    if constexpr (VEC == 1) {
      float x[kSumsqRowsInFlight];
#pragma unroll
      for (int u = 0; u < kSumsqRowsInFlight; u++)
        if (r + u < r1) x[u] = load1<DT>(in, (r + u) * C + c0);   // (wave-uniform condition)
#pragma unroll
      for (int u = 0; u < kSumsqRowsInFlight; u++)
        if (r + u < r1) acc[0] = channel_term_add<TERM>(x[u], acc[0]);
    } else {
      u32x4 raw[kSumsqRowsInFlight];
#pragma unroll
      for (int u = 0; u < kSumsqRowsInFlight; u++)
        if (r + u < r1) raw[u] = load_raw16<false>(in, ((r + u) * C + c0) * (int64_t)Elem<DT>::bytes);
#pragma unroll
      for (int u = 0; u < kSumsqRowsInFlight; u++)
        if (r + u < r1) {
          float x[VEC];
          widen<DT, VEC>(raw[u], x);
#pragma unroll
          for (int k = 0; k < VEC; k++) acc[k] = channel_term_add<TERM>(x[k], acc[k]);
        }
    }
  }
#pragma unroll
  for (int k = 0; k < VEC; k++) partial[slab * C + c0 + k] = acc[k];
}

// acc[c] += the slabs' partials of channel c.  A workgroup covers 32 channels; its 8 lane-groups each add one run of consecutive slabs
// in slab order (run g: slabs [g q, (g + 1) q), q = ceil(n_slabs / 8)), and the first group then adds the 8 run sums in run order
// and the result into acc: a fixed order that depends on n_slabs alone, 8 times fewer dependent loads per lane than one run.
constexpr int kFoldChannels = 32, kFoldRuns = kThreads / kFoldChannels;
__global__ __launch_bounds__(kThreads) void channel_sumsq_fold_kernel(const double* __restrict__ partial, int64_t C, int64_t n_slabs, double* __restrict__ acc) {
  __shared__ double run_sum[kFoldRuns][kFoldChannels];
  const int lane = threadIdx.x % kFoldChannels, run = threadIdx.x / kFoldChannels;
  const int64_t c = (int64_t)blockIdx.x * kFoldChannels + lane;
  const int64_t q = (n_slabs + kFoldRuns - 1) / kFoldRuns;
  const int64_t s0 = run * q, s1 = s0 + q < n_slabs ? s0 + q : n_slabs;
  double sum = 0.0;
  if (c < C) {
    int64_t s = s0;
    for (; s + 8 <= s1; s += 8) {
      double p[8];
#pragma unroll
      for (int u = 0; u < 8; u++) p[u] = partial[(s + u) * C + c];
#pragma unroll
      for (int u = 0; u < 8; u++) sum += p[u];
    }
    for (; s < s1; s++) sum += partial[s * C + c];
  }
  run_sum[run][lane] = sum;
  __syncthreads();
  if (run == 0 && c < C) {
    double total = run_sum[0][lane];
#pragma unroll
    for (int g = 1; g < kFoldRuns; g++) total += run_sum[g][lane];
    acc[c] += total;
  }
}

// ---------------------------------------------------------------------------------------------------------
// One pass over W: a lane loads its unit of U consecutive weights (the unit geometry of nm_mask_vec_kernel: 8 for M <= 8, 16 for
// M = 16) and the matching U norms (aligned 16-byte loads of a vector that stays in L2), forms the scores, ranks each M-group and
// writes what was asked for: the fp32 score, the mask, W * mask.  M == 0: the score only.  A unit never straddles a row (L % U == 0),
// so its first column is (unit index) mod (units per row): taken once per lane by a 32-bit remainder and then advanced by the
// strides' remainders, which the host passes -- no 64-bit division in the loop.
struct WandaArgs {
  const void* w; const float* act_norm; float* score; void* mask; void* y;
  int dtw, dtm, dty;
  int K;
};

template <int M, int UNROLL>
__global__ __launch_bounds__(kThreads) void wanda_nm_kernel(WandaArgs a, int64_t n_units, uint32_t units_per_row, uint32_t step_mod /* kThreads % units_per_row */,
                                                            uint32_t stride_mod /* (grid * kThreads * UNROLL) % units_per_row */) {
  constexpr int U = M == 16 ? 16 : 8;
  const int64_t stride = (int64_t)gridDim.x * kThreads * UNROLL;
  const uint32_t first = blockIdx.x * (uint32_t)(UNROLL * kThreads) + threadIdx.x;   // (the grid is capped: below 2^31)
  uint32_t cu = first % units_per_row;
  for (int64_t u0 = first; u0 < n_units; u0 += stride) {
    float w[UNROLL][U], an[UNROLL][U];
    uint32_t c = cu;
#pragma unroll
    for (int r = 0; r < UNROLL; r++) {
      const int64_t u = u0 + (int64_t)r * kThreads;
      if (u < n_units) {
        load_elems<U>(a.w, a.dtw, u * U, w[r]);
        load_elems<U>(a.act_norm, DMXQ_F32, (int64_t)c * U, an[r]);
      }
      c += step_mod;
      c = c >= units_per_row ? c - units_per_row : c;
    }
#pragma unroll
    for (int r = 0; r < UNROLL; r++) {
      const int64_t u = u0 + (int64_t)r * kThreads;
      if (u >= n_units) continue;
      float s[U];
#pragma unroll
      for (int i = 0; i < U; i++) s[i] = __builtin_fabsf(w[r][i]) * an[r][i];
      if (a.score) store_elems<U>(a.score, DMXQ_F32, u * U, s);
      if constexpr (M != 0) {
        float mk[U];
        nm_unit_mask<M, U>(s, a.K, mk);
        if (a.mask) store_elems<U>(a.mask, a.dtm, u * U, mk);
        if (a.y) {
          float y[U];
#pragma unroll
          for (int i = 0; i < U; i++) y[i] = w[r][i] * mk[i];
          store_elems<U>(a.y, a.dty, u * U, y);
        }
      }
    }
    cu += stride_mod;
    cu = cu >= units_per_row ? cu - units_per_row : cu;
  }
}

template <int M>
static void launch_wanda(const WandaArgs& a, int64_t n, int64_t L, hipStream_t s) {
  constexpr int U = M == 16 ? 16 : 8, UNROLL = 2;
  const int64_t n_units = n / U;
  const int grid = grid_for((n_units + UNROLL - 1) / UNROLL);
  const uint32_t upr = (uint32_t)(L / U);
  DMXQ_LAUNCH((wanda_nm_kernel<M, UNROLL>), dim3(grid), dim3(kThreads), 0, s, a, n_units, upr, (uint32_t)(kThreads % upr),
              (uint32_t)(((int64_t)grid * kThreads * UNROLL) % upr));
}

}  // namespace dmxq

using namespace dmxq;

extern "C" int64_t dmxq_channel_sumsq_workspace_bytes(int64_t rows, int64_t C) {
  if (rows <= 0 || C <= 0) return 0;
  return sumsq_plan(rows, C).n_slabs * C * (int64_t)sizeof(double);
}

template <int TERM>
static int channel_sum_accumulate(const void* in, int dtype_in, int64_t rows, int64_t C, double* acc, void* workspace, void* stream) {
  if (!valid_dtype(dtype_in) || rows < 0 || C < 0) return DMXQ_ERR_BAD_ARG;
  if (rows == 0 || C == 0) return DMXQ_OK;
  if (!in || !acc || !workspace) return DMXQ_ERR_BAD_ARG;
  const SumsqPlan p = sumsq_plan(rows, C);
  hipStream_t s = (hipStream_t)stream;
  double* partial = (double*)workspace;
  const int vec = dtype_in == DMXQ_F32 ? 4 : 8;
  const bool vec_ok = C % vec == 0 && aligned16(in);   // (every row then starts on a 16-byte boundary)
  const int64_t n_cols = vec_ok ? C / vec : C;
  const int64_t n_tiles = (n_cols + kWave - 1) / kWave;
  const int64_t blocks = (n_tiles * p.n_slabs + kThreads / kWave - 1) / (kThreads / kWave);
  const int64_t fold_blocks = (C + kFoldChannels - 1) / kFoldChannels;
  if (blocks > 0x7FFFFFFF || fold_blocks > 0x7FFFFFFF) return DMXQ_ERR_UNSUPPORTED;
#define DMXQ_SUMSQ(D_, V_) DMXQ_LAUNCH((channel_sumsq_slab_kernel<D_, V_, TERM>), dim3((unsigned)blocks), dim3(kThreads), 0, s, in, rows, C, n_cols, n_tiles, p.rows_per_slab, p.n_slabs, partial)
  if (vec_ok) {
    if (dtype_in == DMXQ_F32) DMXQ_SUMSQ(DMXQ_F32, 4);
    else if (dtype_in == DMXQ_F16) DMXQ_SUMSQ(DMXQ_F16, 8);
    else DMXQ_SUMSQ(DMXQ_BF16, 8);
  } else {
    if (dtype_in == DMXQ_F32) DMXQ_SUMSQ(DMXQ_F32, 1);
    else if (dtype_in == DMXQ_F16) DMXQ_SUMSQ(DMXQ_F16, 1);
    else DMXQ_SUMSQ(DMXQ_BF16, 1);
  }
#undef DMXQ_SUMSQ
  DMXQ_LAUNCH(channel_sumsq_fold_kernel, dim3((unsigned)fold_blocks), dim3(kThreads), 0, s, partial, C, p.n_slabs, acc);
  return launch_status();
}

extern "C" int dmxq_channel_sumsq_accumulate(const void* in, int dtype_in, int64_t rows, int64_t C, double* acc, void* workspace, void* stream) {
  return channel_sum_accumulate<kTermSquare>(in, dtype_in, rows, C, acc, workspace, stream);
}

// the |x| twin (AWQ's per-channel mean magnitude): dmxq_channel_sumsq_workspace_bytes(rows, C) is its workspace query too
extern "C" int dmxq_channel_sumabs_accumulate(const void* in, int dtype_in, int64_t rows, int64_t C, double* acc, void* workspace, void* stream) {
  return channel_sum_accumulate<kTermAbs>(in, dtype_in, rows, C, acc, workspace, stream);
}

// 1: dmxq_wanda_nm takes (dtype_w, L, M) in its one-pass kernel (given 16-byte aligned pointers), 0: it refuses them.  One rule
// for the three group sizes: rows of whole 16-element spans, the granularity of nm_mask.hip's vector path.
extern "C" int dmxq_wanda_class(int dtype_w, int64_t L, int M) {
  if (!valid_dtype(dtype_w) || L <= 0) return 0;
  if (M != 0 && M != 4 && M != 8 && M != 16) return 0;
  if (L % 16 != 0 || L / 8 > 0x7FFFFFFF) return 0;
  return 1;
}

extern "C" int dmxq_wanda_nm(const void* w, int dtype_w, const float* act_norm, float* score_out, void* mask_out, int dtype_mask, void* y_out,
                             int dtype_y, int64_t rows, int64_t L, int K, int M, void* stream) {
  if (!valid_dtype(dtype_w) || rows < 0 || L < 0) return DMXQ_ERR_BAD_ARG;
  if (M == 0) {   // the score only
    if (K != 0 || mask_out || y_out || !score_out) return DMXQ_ERR_BAD_ARG;
  } else {
    if (M < 1 || M > 64 || K < 1 || K > M || L % M != 0) return DMXQ_ERR_BAD_ARG;
    if (!score_out && !mask_out && !y_out) return DMXQ_ERR_BAD_ARG;
    if ((mask_out && !valid_dtype(dtype_mask)) || (y_out && !valid_dtype(dtype_y))) return DMXQ_ERR_BAD_ARG;
  }
  const int64_t n = rows * L;
  if (n == 0) return DMXQ_OK;
  if (!w || !act_norm) return DMXQ_ERR_BAD_ARG;
  if (!dmxq_wanda_class(dtype_w, L, M) || !aligned16(w) || !aligned16(act_norm) || (score_out && !aligned16(score_out)) ||
      (mask_out && !aligned16(mask_out)) || (y_out && !aligned16(y_out)))
    return DMXQ_ERR_UNSUPPORTED;
  WandaArgs a{w, act_norm, score_out, mask_out, y_out, dtype_w, dtype_mask, dtype_y, K};
  hipStream_t s = (hipStream_t)stream;
  switch (M) {
    case 0: launch_wanda<0>(a, n, L, s); break;
    case 4: launch_wanda<4>(a, n, L, s); break;
    case 8: launch_wanda<8>(a, n, L, s); break;
    default: launch_wanda<16>(a, n, L, s); break;
  }
  return launch_status();
}
