// csrc/dynamic_cols.hip — the dynamic integer cast and the dynamic scaled float cast with segments along a NON-LAST dimension, each in
// ONE launch (include/dmxq.h dmxq_dynamic_fixed_qdq_cols, dmxq_dynamic_float_qdq_cols; DESIGN.md §8 "Dynamic casts along a non-last
// dimension").  KIVI's keys [B, H, T, D] grouped along T, per-channel activations, [in, out] (HF Conv1D) and conv weights grouped along
// input channels: until now movedim(d, -1).contiguous() -> the last-dim kernel -> movedim(-1, d).contiguous(), three launches and 12 B
// per bf16 element instead of 4.
//
// The contract is the last-dim entry on the tensor with the segment dimension moved last, moved back, bit for bit, qparams included:
// the per-element arithmetic IS that entry's (dynamic_quant.hpp qparams through DynSeg, dyn_q_exact and the reciprocal form under
// recip_ok; dynamic_float.hpp DfSeg and the quotient; floatq.hpp castg_vec) in its per-element-segment forms.
//
// Geometry.  The contiguous tensor is [outer, C, inner]; a segment is S consecutive indices along C at one (outer, inner) position.  A
// lane's 16-byte vector (V = 8 sixteen-bit or 4 fp32 elements) lies along `inner`, so its V elements belong to V DIFFERENT segments and
// the reduction runs down rows, not across lanes:
//   * a tile is one segment's S rows x 64 vectors; tiles are enumerated over the flat index p = (outer, segment, inner vector) --
//     adjacent lanes take adjacent p, so a row access of a wave is a run of whole vectors (1 KiB where inner allows), a small inner
//     fills the 64 lanes with several (outer, segment) positions and a large one spreads over several workgroups;
//   * the workgroup's WAVES waves split the S rows, R = S / WAVES consecutive rows per wave, a lane's R raw vectors held in registers
//     (R = 8 up to S = 64, 16 above; (R, WAVES) are template arguments).  S = 256 is sixteen waves of 16 rows, which leaves a lane 128
//     registers: the fp32 bodies fit them, the sixteen-bit ones with V = 8 columns do not, so a sixteen-bit lane takes HALF a vector
//     there (V = 4, 8-byte accesses, a tile of 256 rows x 64 half vectors: 512-byte runs per wave and row);
//   * a lane folds its rows' extrema per column lane-locally (no cross-lane step at all), the waves exchange the per-column keys
//     (integer cast: order-preserving (lo, hi) keys, reduce_common.hpp; float cast: the |x| bit patterns) through LDS
//     ONCE, with one barrier; every wave then forms the V per-column qparams itself and casts its own rows from the registers;
//   * lanes past the end re-read the last valid position and store nothing.
// One read and one write per element, no workspace, no atomics, no synchronisation with the host: capturable.  in == out is NOT offered:
// a tile is read completely before it is written, but tiles of one row range interleave in memory with their neighbours', and the entry
// refuses aliasing instead of reasoning about it.  Registers / LDS per (S, dtype): DESIGN.md §8.
#include <math.h>

#include "dynamic_float.hpp"   // DfSeg, df_quotient_cols (dynamic_geom.hpp: dync_class)
#include "dynamic_quant.hpp"   // DynFmt, DynExt, DynSeg, dyn_ext_add_cols, dyn_cast_cols
#include "floatq.hpp"

namespace dmxq {
namespace {

struct DcFloatFmt {
  CastG c;
  float fmax;
  int pow2;
};

// a lane's place: p = blockIdx.x * 64 + lane over (outer, segment, inner vector); -> the lane's first vector and whether it stores.
// The 64-bit division runs once per workgroup on uniform values; a lane adds its offset with a 32-bit division (iv0 + lane < innerV + 64).
struct DcPlace {
  int64_t v0;   // vector index of row 0 of the lane's column
  int64_t p;    // flat position: the qparams of the lane's V columns are entries p V .. p V + V - 1 of [outer, C / S, inner]
  bool ok;
};
__device__ __forceinline__ DcPlace dc_place(int64_t ncol, int64_t innerV, int S, int lane) {
  const int64_t p0 = (int64_t)blockIdx.x * kWave;
  const int64_t t0 = uniform_i64(p0 / innerV);
  const int64_t iv0 = p0 - t0 * innerV;
  DcPlace pl;
  pl.ok = p0 + lane < ncol;
  const int lc = pl.ok ? lane : (int)(ncol - 1 - p0);   // (p0 < ncol: the grid is ceil(ncol / 64))
  pl.p = p0 + lc;
  const int64_t a = iv0 + lc;
  const int64_t q = innerV <= 0x7FFFFFFF ? (int64_t)((uint32_t)a / (uint32_t)innerV) : (int64_t)(a >= innerV);
  // (outer, segment) = t0 + q: the segment's first row is row (t0 + q) S of the [outer C, inner] matrix
  pl.v0 = (t0 + q) * S * innerV + (a - q * innerV);
  return pl;
}

// the place again, as a value the compiler cannot trace back: the stores' row offsets are then formed where they are used, not kept
// beside the loads' from the top of the kernel (2 registers per row, which the 16-row tiles do not have)
__device__ __forceinline__ DcPlace dc_place_again(DcPlace pl) {
  uint32_t lo = (uint32_t)pl.v0, hi = (uint32_t)((uint64_t)pl.v0 >> 32);
  asm volatile("" : "+v"(lo), "+v"(hi));
  pl.v0 = (int64_t)(((uint64_t)hi << 32) | lo);
  return pl;
}

// a lane's vector of V elements: 16 bytes, or 8 (sixteen-bit, V = 4: the lower half of the raw vector, the upper half unused)
template <int DT, int V, int R>
__device__ __forceinline__ void dc_load(const void* in, const DcPlace& pl, int64_t innerV, int w, u32x4 (&raw)[R]) {
#pragma unroll
  for (int j = 0; j < R; j++) {
    const int64_t v = pl.v0 + (int64_t)(w * R + j) * innerV;
    if constexpr (V * Elem<DT>::bytes == 16) raw[j] = load_raw16<true>(in, v * 16);
    else {
      const u32x2 h = __builtin_nontemporal_load((const u32x2*)((const char*)in + v * 8));
      raw[j] = u32x4{h.x, h.y, 0u, 0u};
    }
  }
}
template <int DT, int V>
__device__ __forceinline__ void dc_widen(const u32x4& raw, float (&x)[V]) {
  if constexpr (V * Elem<DT>::bytes == 16) widen<DT, V>(raw, x);
  else {
    float t[2 * V];
    widen<DT, 2 * V>(raw, t);
#pragma unroll
    for (int k = 0; k < V; k++) x[k] = t[k];
  }
}

// ---------------------------------------------------------------------------------------------------- the integer cast
// the cast of rows J0 .. J0 + 7 of a lane.  Eight rows per call, 16 rows as two calls: a loop over 16 rows with the casts' cold redo paths
// is more than the compiler unrolls, and a rolled loop would index the raw vectors at run time (scratch)
template <int DT, int R, int J0, int V>
__device__ __forceinline__ void dync_fixed_rows(const u32x4 (&raw)[R], const DynSeg (&s)[V], bool all_fast, bool all_zp0, const DynFmt& f,
                                                void* __restrict__ out, const DcPlace& pl, int64_t innerV, int w) {
#pragma unroll
  for (int j = J0; j < J0 + 8; j++) {
    float x[V], y[V];
    dc_widen<DT, V>(raw[j], x);
    dyn_cast_cols<V>(x, y, s, all_fast, all_zp0, f);
    if (pl.ok) store_vec<DT, V>(out, (pl.v0 + (int64_t)(w * R + j) * innerV) * V, y);
    __builtin_amdgcn_sched_barrier(0);   // (a row at a time: rows cast side by side would need more registers than a 16-wave workgroup has)
  }
}

template <int DT, int R, int WAVES, int V = 16 / Elem<DT>::bytes>
__global__ __launch_bounds__(kWave * WAVES) void dync_fixed_kernel(const void* __restrict__ in, void* __restrict__ out, int64_t ncol,
                                                                  int64_t innerV, const DynFmt f, float* __restrict__ scale_out,
                                                                  int64_t* __restrict__ zp_out) {
  constexpr int S = R * WAVES;
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  const DcPlace pl = dc_place(ncol, innerV, S, lane);
  u32x4 raw[R];
  dc_load<DT, V, R>(in, pl, innerV, w, raw);
  DynExt e[V];
#pragma unroll
  for (int k = 0; k < V; k++) e[k].init();
#pragma unroll
  for (int j = 0; j < R; j++) {
    float x[V];
    dc_widen<DT, V>(raw[j], x);
    dyn_ext_add_cols<V>(e, x);
    __builtin_amdgcn_sched_barrier(0);   // (a row at a time, as it arrives: widened side by side the rows would not fit the registers)
  }
  uint32_t klo[V], khi[V];
#pragma unroll
  for (int k = 0; k < V; k++) e[k].keys(klo[k], khi[k]);
  // the waves' per-column keys: [wave][quarter of the vector][lane], 16 bytes per lane and access (no bank conflict)
  __shared__ u32x4 s_lo[WAVES][V / 4][kWave], s_hi[WAVES][V / 4][kWave];
#pragma unroll
  for (int c = 0; c < V / 4; c++) {
    s_lo[w][c][lane] = u32x4{klo[4 * c], klo[4 * c + 1], klo[4 * c + 2], klo[4 * c + 3]};
    s_hi[w][c][lane] = u32x4{khi[4 * c], khi[4 * c + 1], khi[4 * c + 2], khi[4 * c + 3]};
  }
  __syncthreads();
#pragma unroll 1   // (rolled: LDS is indexed, no register array is; unrolled, the WAVES x V / 4 x 2 reads in flight cost more registers than the tile)
  for (int i = 0; i < WAVES; i++) {
#pragma unroll
    for (int c = 0; c < V / 4; c++) {
      const u32x4 a = s_lo[i][c][lane], b = s_hi[i][c][lane];
#pragma unroll
      for (int q = 0; q < 4; q++) { klo[4 * c + q] = min(klo[4 * c + q], a[q]); khi[4 * c + q] = max(khi[4 * c + q], b[q]); }
    }
  }
  DynSeg s[V];
  bool slow = false, nz = false;
#pragma unroll
  for (int k = 0; k < V; k++) {
    s[k].setup(klo[k], khi[k], f);
    slow = slow || !recip_ok(s[k].sc);
    nz = nz || s[k].z != 0.0f;
  }
  // the recipe is chosen per wave (fast and exact columns may share a lane: the result does not depend on it)
  const bool all_fast = __builtin_amdgcn_ballot_w64(slow) == 0ull;
  const bool all_zp0 = __builtin_amdgcn_ballot_w64(nz) == 0ull;
  if (w == 0 && pl.ok) {
#pragma unroll
    for (int k = 0; k < V; k++) {
      if (scale_out) scale_out[pl.p * V + k] = s[k].sc;
      if (zp_out) zp_out[pl.p * V + k] = s[k].zp;
    }
  }
  const DcPlace ps = dc_place_again(pl);
  dync_fixed_rows<DT, R, 0>(raw, s, all_fast, all_zp0, f, out, ps, innerV, w);
  if constexpr (R == 16) dync_fixed_rows<DT, R, 8>(raw, s, all_fast, all_zp0, f, out, ps, innerV, w);
}

// ---------------------------------------------------------------------------------------------------- the scaled float cast
// per-column max |x| of a lane's rows as fp32 magnitude bits (exact: widening is monotone; a NaN pattern is the largest of all)
template <int DT, int V>
__device__ __forceinline__ void dc_absmax_cols(uint32_t (&m)[V], const u32x4& raw) {
  float x[V];
  dc_widen<DT, V>(raw, x);
#pragma unroll
  for (int k = 0; k < V; k++) m[k] = max(m[k], f2u(x[k]) & 0x7FFFFFFFu);
}

// rows J0 .. J0 + 7 of a lane (dync_fixed_rows' reason)
template <int DT, int R, int J0, int V>
__device__ __forceinline__ void dync_float_rows(const u32x4 (&raw)[R], const DfSeg (&sg)[V], bool fast, const DcFloatFmt& f,
                                                void* __restrict__ out, const DcPlace& pl, int64_t innerV, int w) {
#pragma unroll
  for (int j = J0; j < J0 + 8; j++) {
    float x[V], q[V];
    dc_widen<DT, V>(raw[j], x);
    df_quotient_cols<V>(x, q, sg, fast);
    castg_vec<DMXQ_F32, V>(q, f.c);
#pragma unroll
    for (int k = 0; k < V; k++) q[k] = q[k] * sg[k].s;
    if (pl.ok) store_vec<DT, V>(out, (pl.v0 + (int64_t)(w * R + j) * innerV) * V, q);
    __builtin_amdgcn_sched_barrier(0);   // (dync_fixed_rows' reason)
  }
}

template <int DT, int R, int WAVES, int V = 16 / Elem<DT>::bytes>
__global__ __launch_bounds__(kWave * WAVES) void dync_float_kernel(const void* __restrict__ in, void* __restrict__ out, int64_t ncol,
                                                                  int64_t innerV, const DcFloatFmt f, float* __restrict__ scale_out) {
  constexpr int S = R * WAVES;
  const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
  const DcPlace pl = dc_place(ncol, innerV, S, lane);
  u32x4 raw[R];
  dc_load<DT, V, R>(in, pl, innerV, w, raw);
  uint32_t m[V];
#pragma unroll
  for (int k = 0; k < V; k++) m[k] = 0u;
#pragma unroll
  for (int j = 0; j < R; j++) dc_absmax_cols<DT, V>(m, raw[j]);
  __shared__ u32x4 s_m[WAVES][V / 4][kWave];   // (dync_fixed_kernel's layout)
#pragma unroll
  for (int c = 0; c < V / 4; c++) s_m[w][c][lane] = u32x4{m[4 * c], m[4 * c + 1], m[4 * c + 2], m[4 * c + 3]};
  __syncthreads();
#pragma unroll 1
  for (int i = 0; i < WAVES; i++) {
#pragma unroll
    for (int c = 0; c < V / 4; c++) {
      const u32x4 a = s_m[i][c][lane];
#pragma unroll
      for (int q = 0; q < 4; q++) m[4 * c + q] = max(m[4 * c + q], a[q]);
    }
  }
  DfSeg sg[V];
  bool slow = false;
#pragma unroll
  for (int k = 0; k < V; k++) {
    sg[k].setup(m[k], f.fmax, f.pow2);
    slow = slow || !recip_ok(sg[k].s);
  }
  const bool fast = __builtin_amdgcn_ballot_w64(slow) == 0ull;
  if (w == 0 && pl.ok && scale_out) {
#pragma unroll
    for (int k = 0; k < V; k++) scale_out[pl.p * V + k] = sg[k].s;
  }
  const DcPlace ps = dc_place_again(pl);
  dync_float_rows<DT, R, 0>(raw, sg, fast, f, out, ps, innerV, w);
  if constexpr (R == 16) dync_float_rows<DT, R, 8>(raw, sg, fast, f, out, ps, innerV, w);
}

// ---------------------------------------------------------------------------------------------------- launch
// K: a macro naming the kernel template; the (R, WAVES) instance of a segment length (dynamic_geom.hpp dync_class)
#define DMXQ_DYNC_DISPATCH(KERNEL, DT_, ...)                                                                              \
  switch (S) {                                                                                                            \
    case 16: DMXQ_LAUNCH((KERNEL<DT_, 8, 2>), dim3((unsigned)grid), dim3(kWave * 2), 0, s, __VA_ARGS__); break;           \
    case 32: DMXQ_LAUNCH((KERNEL<DT_, 8, 4>), dim3((unsigned)grid), dim3(kWave * 4), 0, s, __VA_ARGS__); break;           \
    case 64: DMXQ_LAUNCH((KERNEL<DT_, 8, 8>), dim3((unsigned)grid), dim3(kWave * 8), 0, s, __VA_ARGS__); break;           \
    case 128: DMXQ_LAUNCH((KERNEL<DT_, 16, 8>), dim3((unsigned)grid), dim3(kWave * 8), 0, s, __VA_ARGS__); break;         \
    case 256: DMXQ_LAUNCH((KERNEL<DT_, 16, 16, 4>), dim3((unsigned)grid), dim3(kWave * 16), 0, s, __VA_ARGS__); break;    \
    default: return DMXQ_ERR_UNSUPPORTED;                                                                                 \
  }

// elements of a lane's vector: a 16-byte vector, except sixteen-bit segments of 256 (half vectors: the header comment)
inline int dync_lane_elems(int dtype, int64_t S) { return (dtype == DMXQ_F32 || S == 256) ? 4 : 8; }

// what both entries check alike; DMXQ_OK with *grid == 0: nothing to do
int dync_plan(const void* in, const void* out, int dtype_in, int dtype_out, int64_t outer, int64_t C, int64_t inner, int64_t S, int rounding,
              int64_t* ncol, int64_t* innerV, int64_t* grid) {
  *grid = 0;
  if (!valid_dtype(dtype_in) || !valid_dtype(dtype_out) || !valid_rounding(rounding)) return DMXQ_ERR_BAD_ARG;
  if (outer < 0 || C < 0 || inner < 0 || S < 1 || C % S != 0) return DMXQ_ERR_BAD_ARG;
  const bool empty = outer == 0 || C == 0 || inner == 0;
  if (!empty && (!in || !out || in == out)) return DMXQ_ERR_BAD_ARG;
  if (dtype_in != dtype_out || rounding != DMXQ_ROUND_NEAREST) return DMXQ_ERR_UNSUPPORTED;
  if (empty) return DMXQ_OK;
  const int V = dtype_in == DMXQ_F32 ? 4 : 8;
  if (dync_class(S, V, inner) == DMXQ_DYN_NONE) return DMXQ_ERR_UNSUPPORTED;
  if (!aligned16(in) || !aligned16(out)) return DMXQ_ERR_UNSUPPORTED;
  if (outer > INT64_MAX / 4 / C || outer * C > INT64_MAX / 4 / inner) return DMXQ_ERR_UNSUPPORTED;   // (byte offsets stay inside int64)
  *innerV = inner / dync_lane_elems(dtype_in, S);
  *ncol = outer * (C / S) * *innerV;
  const int64_t g = (*ncol + kWave - 1) / kWave;
  if (g > 0x7FFFFFFF) return DMXQ_ERR_UNSUPPORTED;
  *grid = g;
  return DMXQ_OK;
}

}  // namespace
}  // namespace dmxq

using namespace dmxq;

extern "C" int dmxq_dynamic_cols_class(int dtype, int64_t segment, int64_t inner) {
  if (!valid_dtype(dtype)) return DMXQ_DYN_NONE;
  return dync_class(segment, dtype == DMXQ_F32 ? 4 : 8, inner);
}

extern "C" int dmxq_dynamic_fixed_qdq_cols(const void* in, void* out, int dtype_in, int dtype_out, int64_t outer, int64_t C, int64_t inner,
                                           int64_t segment, int precision, int fraction, int clamp, int symmetric, int rounding, int qmin,
                                           int qmax, int symmetric_qscheme, float* scale_out, int64_t* zp_out, void* stream) {
  if (precision < 1 || qmax <= qmin) return DMXQ_ERR_BAD_ARG;
  int64_t ncol, innerV, grid;
  const int st = dync_plan(in, out, dtype_in, dtype_out, outer, C, inner, segment, rounding, &ncol, &innerV, &grid);
  if (st != DMXQ_OK) return st;
  if (fraction != 0 || !clamp || precision > 22) return DMXQ_ERR_UNSUPPORTED;
  if (grid == 0) return DMXQ_OK;
  const FixedFmt x = make_fixed_fmt(precision, 0, 1, symmetric, DMXQ_ROUND_NEAREST, 0ull);
  const DynFmt f{x.t_min, x.t_max, qmin, qmax, symmetric_qscheme ? 1 : 0};
  hipStream_t s = (hipStream_t)stream;
  const int S = (int)segment;
  if (dtype_in == DMXQ_BF16) { DMXQ_DYNC_DISPATCH(dync_fixed_kernel, DMXQ_BF16, in, out, ncol, innerV, f, scale_out, zp_out) }
  else if (dtype_in == DMXQ_F16) { DMXQ_DYNC_DISPATCH(dync_fixed_kernel, DMXQ_F16, in, out, ncol, innerV, f, scale_out, zp_out) }
  else { DMXQ_DYNC_DISPATCH(dync_fixed_kernel, DMXQ_F32, in, out, ncol, innerV, f, scale_out, zp_out) }
  return launch_status();
}

extern "C" int dmxq_dynamic_float_qdq_cols(const void* in, void* out, int dtype_in, int dtype_out, int64_t outer, int64_t C, int64_t inner,
                                           int64_t segment, int man_bits, int exp_bits, int exp_bias, int flush_subnormal, int rounding,
                                           int pow2_scale, float* scale_out, void* stream) {
  if (exp_bits < 1 || exp_bits >= 8 || man_bits < 0) return DMXQ_ERR_BAD_ARG;   // (8 exponent bits: no finite maximum to scale to)
  int64_t ncol, innerV, grid;
  const int st = dync_plan(in, out, dtype_in, dtype_out, outer, C, inner, segment, rounding, &ncol, &innerV, &grid);
  if (st != DMXQ_OK) return st;
  const dmxq_float_fmt ff{man_bits, exp_bits, exp_bias, flush_subnormal};
  DcFloatFmt f{};
  if (!castg_of(&ff, &f.c)) return DMXQ_ERR_UNSUPPORTED;
  if (grid == 0) return DMXQ_OK;
  f.fmax = f.c.k.max_val;
  f.pow2 = pow2_scale ? 1 : 0;
  hipStream_t s = (hipStream_t)stream;
  const int S = (int)segment;
  if (dtype_in == DMXQ_BF16) { DMXQ_DYNC_DISPATCH(dync_float_kernel, DMXQ_BF16, in, out, ncol, innerV, f, scale_out) }
  else if (dtype_in == DMXQ_F16) { DMXQ_DYNC_DISPATCH(dync_float_kernel, DMXQ_F16, in, out, ncol, innerV, f, scale_out) }
  else { DMXQ_DYNC_DISPATCH(dync_float_kernel, DMXQ_F32, in, out, ncol, innerV, f, scale_out) }
  return launch_status();
}
