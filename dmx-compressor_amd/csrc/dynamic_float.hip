// csrc/dynamic_float.hip — dynamic SCALED low-bit float cast in ONE launch (include/dmxq.h dmxq_dynamic_float_qdq).
// Not in the reference, whose float formats are cast unscaled (FP[1|4|3,7] saturates at +-480 and loses everything far below 1) and whose
// only scaled float cast is MXFP's power-of-two block of 32: here a segment -- a row, a group of a row, a g x g tile of the last two
// dims -- is scaled by its own absolute maximum on every call, the FP8 recipe's per-token activations and per-tile weights.
//
// The definition (fp32 throughout; the reference's float_quantize arithmetic, floatq.hpp, per element):
//   amax = max |x| over the segment, ONE NaN anywhere makes it NaN (the maximum runs on the magnitude BITS, where a NaN pattern is largest)
//   s    = amax / fmax, an IEEE division; fmax = 2^(2^(e-1)) (2 - 2^-m), the format's largest output
//   pow2_scale: s is rounded UP to a power of two on its bits, b = (b & 0x7F800000) + ((b & 0x007FFFFF) ? 0x00800000 : 0)
//   s    = 1 when s is not finite or below 2^-126 (an all-zero, a NaN or an Inf segment; a NaN's bits become -0 in the step above)
//   y    = float_q(x / s) * s: an IEEE quotient, the format's nearest cast with its flush flag and its saturation of NaN / Inf, ONE fp32
//          multiply, one rounding to the output dtype.
// The quotient: a wave whose scales all lie inside [2^-20, 2^20] (recip_ok) takes common.hpp div_by_recip, proven bit-equal to the
// division for x = +-0 or 2^-100 <= |x| <= 2^100 (div_by_recip_ok); lanes holding anything else, and every lane of a wave with a scale
// outside that range, redo their vector with `/` behind one cold wave-uniform branch.  A power-of-two scale takes the same route (its
// exact reciprocal would allow one multiply; the three operations of the reciprocal form are not what bounds the kernel).  The cast is
// floatq.hpp castg_vec with its own wave-uniform fallbacks (its float32 form: the rounding to the output dtype comes after the multiply).
//
// Geometry (dynamic_geom.hpp, as dynamic_quant.hip).  A lane moves 16-byte vectors (V = 8 sixteen-bit or 4 fp32 elements) held RAW in
// registers between the maximum pass and the cast: one read and one write per element, every segment read completely before any of it
// is written.
//   * segments inside a wave (16 .. 256, a power of two): flat, S / V adjacent lanes, the maximum by DPP / xor shuffles (group_max_u32);
//   * whole rows up to 16384: a wave per row up to 8 vectors per lane (16 for fp32), a 256-thread workgroup per row above (maxima
//     through LDS);
//   * g x g tiles, g = 32 / 64 / 128, of a [rows, cols] matrix (leading dims folded into rows: g divides both): a tile's g * g / V
//     vectors belong to ONE wave while they fit four per lane (four tiles per workgroup) and to a 256-thread workgroup otherwise
//     (2 .. 16 per lane: 8 at g = 128 sixteen-bit, 16 at g = 128 fp32).  Vector j of a tile is its row j / (g / V), column vector
//     j % (g / V): consecutive lanes read the g contiguous elements of a tile row, then the next row.
// Lanes past the end re-read the last vector / row / tile (a repeated vector cannot change a maximum) and store nothing.  No workspace,
// no synchronisation with the host: capturable.  The scales go out as plain stores from one lane per segment.
#include <math.h>

#include "dynamic_float.hpp"   // DfSeg, df_quotient_vec, df_block_max, dynf_class: shared with csrc/codebook.hip
#include "floatq.hpp"

namespace dmxq {
namespace {

struct DfFmt {
  CastG c;
  float fmax;
  int pow2;
};

// called by whole waves; `fast`: every scale of the wave lies inside the reciprocal's range (wave-uniform)
template <int V>
__device__ __forceinline__ void df_cast_vec(const float (&x)[V], float (&y)[V], const DfSeg& sg, bool fast, const DfFmt& f) {
  float q[V];
  df_quotient_vec<V>(x, q, sg, fast);
  castg_vec<DMXQ_F32, V>(q, f.c);
#pragma unroll
  for (int k = 0; k < V; k++) y[k] = q[k] * sg.s;
}

// segments of `lanes` adjacent lanes; nvec = n_segments * lanes vectors in all; wave w takes vectors [w U 64, (w + 1) U 64)
template <int DT, int U>
__global__ __launch_bounds__(kDynThreads) void dynf_group_kernel(const void* __restrict__ in, void* __restrict__ out, int64_t nvec, int lanes,
                                                                int lanes_log2, const DfFmt f, float* __restrict__ scale_out) {
  constexpr int V = 16 / Elem<DT>::bytes;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = (int64_t)blockIdx.x * (kDynThreads / kWave) + threadIdx.x / kWave;
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
    sg.setup(group_max_u32(absmax_bits<DT>(raw[u]), lanes), f.fmax, f.pow2);
    const bool fast = __builtin_amdgcn_ballot_w64(!recip_ok(sg.s)) == 0ull;
    float x[V], y[V];
    widen<DT, V>(raw[u], x);
    df_cast_vec<V>(x, y, sg, fast, f);
    if (i < nvec) {
      store_vec<DT, V>(out, i * V, y);
      if (scale_out && (lane & (lanes - 1)) == 0) scale_out[i >> lanes_log2] = sg.s;
    }
  }
}

// rows of nv vectors; WAVES = 1: a wave per row, four rows per workgroup; WAVES = 4: the workgroup's row.  U x 64 x WAVES >= nv.
template <int DT, int U, int WAVES>
__global__ __launch_bounds__(kDynThreads) void dynf_rows_kernel(const void* __restrict__ in, void* __restrict__ out, int64_t rows, int nv,
                                                               const DfFmt f, float* __restrict__ scale_out) {
  constexpr int V = 16 / Elem<DT>::bytes;
  constexpr int T = kWave * WAVES;                       // lanes per row
  constexpr int RPB = kDynThreads / T;                   // rows per workgroup
  const int t = threadIdx.x & (T - 1);
  int64_t row = (int64_t)blockIdx.x * RPB + threadIdx.x / T;
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
  sg.setup(m, f.fmax, f.pow2);
  const bool fast = __builtin_amdgcn_ballot_w64(!recip_ok(sg.s)) == 0ull;   // (one segment per wave)
  if (t == 0 && row_ok && scale_out) scale_out[row] = sg.s;
#pragma unroll
  for (int u = 0; u < U; u++) {
    const int v = t + u * T;
    float x[V], y[V];
    widen<DT, V>(raw[u], x);
    df_cast_vec<V>(x, y, sg, fast, f);
    if (v < nv && row_ok) store_vec<DT, V>(out, (v0 + v) * V, y);
  }
}

// g x g tiles of a [rows, cols] matrix; tile id = (rows / g index) * ntc + (cols / g index), the order of scale_out.  A tile is
// U x 64 x WAVES vectors exactly; gv = g / V vectors per tile row (a power of two, gv_log2), cv = cols / V vectors per matrix row.
template <int DT, int U, int WAVES>
__global__ __launch_bounds__(kDynThreads) void dynf_tile_kernel(const void* __restrict__ in, void* __restrict__ out, int64_t tiles, int64_t ntc,
                                                               int64_t cv, int g, int gv_log2, const DfFmt f, float* __restrict__ scale_out) {
  constexpr int V = 16 / Elem<DT>::bytes;
  constexpr int T = kWave * WAVES;                       // lanes per tile
  constexpr int TPB = kDynThreads / T;                   // tiles per workgroup
  const int t = threadIdx.x & (T - 1);
  int64_t tile = (int64_t)blockIdx.x * TPB + threadIdx.x / T;
  const bool tile_ok = tile < tiles;                     // (wave-uniform; a wave past the last tile re-reads it and stores nothing)
  tile = tile_ok ? tile : tiles - 1;
  const int64_t tr = tile / ntc, tc = tile - tr * ntc;
  const int64_t v0 = tr * g * cv + (tc << gv_log2);      // the tile's first vector
  const int gv_mask = (1 << gv_log2) - 1;
  u32x4 raw[U];
#pragma unroll
  for (int u = 0; u < U; u++) {
    const int j = t + u * T;
    raw[u] = load_raw16<true>(in, (v0 + (int64_t)(j >> gv_log2) * cv + (j & gv_mask)) * 16);
  }
  uint32_t m = 0u;
#pragma unroll
  for (int u = 0; u < U; u++) m = max(m, absmax_bits<DT>(raw[u]));
  m = df_block_max<WAVES>(group_max_u32(m, kWave));
  DfSeg sg;
  sg.setup(m, f.fmax, f.pow2);
  const bool fast = __builtin_amdgcn_ballot_w64(!recip_ok(sg.s)) == 0ull;   // (one segment per wave)
  if (t == 0 && tile_ok && scale_out) scale_out[tile] = sg.s;
#pragma unroll
  for (int u = 0; u < U; u++) {
    const int j = t + u * T;
    float x[V], y[V];
    widen<DT, V>(raw[u], x);
    df_cast_vec<V>(x, y, sg, fast, f);
    if (tile_ok) store_vec<DT, V>(out, (v0 + (int64_t)(j >> gv_log2) * cv + (j & gv_mask)) * V, y);
  }
}

template <int DT>
int dynf_launch_segments(const void* in, void* out, int64_t n_segments, int64_t S, bool whole_rows, const DfFmt& f, float* scale_out,
                         hipStream_t s) {
  constexpr int V = 16 / Elem<DT>::bytes;
  const int64_t nv = S / V;   // vectors per segment
  const int cls = dynf_class(S, V, whole_rows);
  if (cls == DMXQ_DYN_NONE) return DMXQ_ERR_UNSUPPORTED;
  if (cls == DMXQ_DYN_GROUP) {
    const int lanes = (int)nv;   // 2 .. 64
    int l2 = 0;
    while ((1 << l2) < lanes) l2++;
    const int64_t nvec = n_segments * nv;
    // one vector per lane while that already fills the device, four independent loads per lane beyond (dynamic_quant.hip's rule)
    const bool deep = plan_norm(nvec) > ((int64_t)1 << 19);
    const int64_t per_wg = (int64_t)kDynThreads * (deep ? 4 : 1);
    const int64_t grid = (nvec + per_wg - 1) / per_wg;
    if (grid > 0x7FFFFFFF) return DMXQ_ERR_UNSUPPORTED;
    if (deep) DMXQ_LAUNCH((dynf_group_kernel<DT, 4>), dim3((unsigned)grid), dim3(kDynThreads), 0, s, in, out, nvec, lanes, l2, f, scale_out);
    else DMXQ_LAUNCH((dynf_group_kernel<DT, 1>), dim3((unsigned)grid), dim3(kDynThreads), 0, s, in, out, nvec, lanes, l2, f, scale_out);
    return launch_status();
  }
  const bool wave_row = cls != DMXQ_DYN_BLOCK_ROW;
  const int64_t rpb = wave_row ? kDynThreads / kWave : 1;
  const int64_t grid = (n_segments + rpb - 1) / rpb;
  if (grid > 0x7FFFFFFF) return DMXQ_ERR_UNSUPPORTED;
  const int64_t per_lane = (nv + (wave_row ? kWave : kDynThreads) - 1) / (wave_row ? kWave : kDynThreads);
#define DMXQ_DYNF_ROWS(U_, W_) \
  DMXQ_LAUNCH((dynf_rows_kernel<DT, U_, W_>), dim3((unsigned)grid), dim3(kDynThreads), 0, s, in, out, n_segments, (int)nv, f, scale_out)
  if (wave_row) {
    if (per_lane <= 1) DMXQ_DYNF_ROWS(1, 1);
    else if (per_lane <= 2) DMXQ_DYNF_ROWS(2, 1);
    else if (per_lane <= 4) DMXQ_DYNF_ROWS(4, 1);
    else if (per_lane <= 8) DMXQ_DYNF_ROWS(8, 1);
    else if constexpr (V == 4) DMXQ_DYNF_ROWS(16, 1);
    else return DMXQ_ERR_UNSUPPORTED;   // (not reached: dynf_class sends such sixteen-bit rows to the workgroup form)
  } else {
    if (per_lane <= 8) DMXQ_DYNF_ROWS(8, 4);
    else if constexpr (V == 4) DMXQ_DYNF_ROWS(16, 4);
    else return DMXQ_ERR_UNSUPPORTED;   // (not reached: 16384 sixteen-bit elements are 2048 vectors)
  }
#undef DMXQ_DYNF_ROWS
  return launch_status();
}

template <int DT>
int dynf_launch_tiles(const void* in, void* out, int64_t rows, int64_t cols, int64_t g, const DfFmt& f, float* scale_out, hipStream_t s) {
  constexpr int V = 16 / Elem<DT>::bytes;
  if (dyn_tile_class(g) == DMXQ_DYN_NONE) return DMXQ_ERR_UNSUPPORTED;
  const int64_t ntc = cols / g, tiles = (rows / g) * ntc, cv = cols / V;
  int gv_log2 = 0;
  while ((1 << gv_log2) < g / V) gv_log2++;
  const int64_t tile_vecs = g * (g / V);                 // 128 .. 4096
  const bool wave_tile = tile_vecs <= 4 * kWave;
  const int64_t tpb = wave_tile ? kDynThreads / kWave : 1;
  const int64_t grid = (tiles + tpb - 1) / tpb;
  if (grid > 0x7FFFFFFF) return DMXQ_ERR_UNSUPPORTED;
  const int64_t per_lane = tile_vecs / (wave_tile ? kWave : kDynThreads);
#define DMXQ_DYNF_TILE(U_, W_) \
  DMXQ_LAUNCH((dynf_tile_kernel<DT, U_, W_>), dim3((unsigned)grid), dim3(kDynThreads), 0, s, in, out, tiles, ntc, cv, (int)g, gv_log2, f, scale_out)
  if (wave_tile) {
    if (per_lane == 2) DMXQ_DYNF_TILE(2, 1);
    else if (per_lane == 4) DMXQ_DYNF_TILE(4, 1);
    else return DMXQ_ERR_UNSUPPORTED;
  } else {
    if (per_lane == 2) DMXQ_DYNF_TILE(2, 4);
    else if (per_lane == 4) DMXQ_DYNF_TILE(4, 4);
    else if (per_lane == 8) DMXQ_DYNF_TILE(8, 4);
    else if constexpr (V == 4) {
      if (per_lane == 16) DMXQ_DYNF_TILE(16, 4);
      else return DMXQ_ERR_UNSUPPORTED;
    } else return DMXQ_ERR_UNSUPPORTED;
  }
#undef DMXQ_DYNF_TILE
  return launch_status();
}

}  // namespace
}  // namespace dmxq

using namespace dmxq;

extern "C" int dmxq_dynamic_float_class(int dtype, int mode, int64_t segment) {
  if (!valid_dtype(dtype)) return DMXQ_DYN_NONE;
  const int V = dtype == DMXQ_F32 ? 4 : 8;
  if (mode == DMXQ_DYNF_TILE) return dyn_tile_class(segment);
  if (mode == DMXQ_DYNF_GROUP || mode == DMXQ_DYNF_ROWS) return dynf_class(segment, V, mode == DMXQ_DYNF_ROWS);
  return DMXQ_DYN_NONE;
}

extern "C" int dmxq_dynamic_float_qdq(const void* in, void* out, int dtype_in, int dtype_out, int mode, int64_t n_segments, int64_t segment,
                                      int64_t rows, int64_t cols, int man_bits, int exp_bits, int exp_bias, int flush_subnormal, int rounding,
                                      int pow2_scale, float* scale_out, void* stream) {
  if (!valid_dtype(dtype_in) || !valid_dtype(dtype_out) || !valid_rounding(rounding)) return DMXQ_ERR_BAD_ARG;
  if (mode != DMXQ_DYNF_GROUP && mode != DMXQ_DYNF_ROWS && mode != DMXQ_DYNF_TILE) return DMXQ_ERR_BAD_ARG;
  if (n_segments < 0 || segment < 0 || rows < 0 || cols < 0) return DMXQ_ERR_BAD_ARG;
  if (exp_bits < 1 || exp_bits >= 8 || man_bits < 0) return DMXQ_ERR_BAD_ARG;   // (8 exponent bits: fp32's range, no finite maximum to scale to)
  const bool tile = mode == DMXQ_DYNF_TILE;
  if (tile && segment > 0 && (rows % segment != 0 || cols % segment != 0 || n_segments != (rows / segment) * (cols / segment)))
    return DMXQ_ERR_BAD_ARG;
  if (n_segments > 0 && segment > 0 && (!in || !out)) return DMXQ_ERR_BAD_ARG;
  // what the kernels take; everything else is the caller's chain (nothing launched)
  if (dtype_in != dtype_out || rounding != DMXQ_ROUND_NEAREST) return DMXQ_ERR_UNSUPPORTED;
  const dmxq_float_fmt ff{man_bits, exp_bits, exp_bias, flush_subnormal};
  DfFmt f{};
  if (!castg_of(&ff, &f.c)) return DMXQ_ERR_UNSUPPORTED;
  f.fmax = f.c.k.max_val;
  f.pow2 = pow2_scale ? 1 : 0;
  const int V = dtype_in == DMXQ_F32 ? 4 : 8;
  if (tile ? dyn_tile_class(segment) == DMXQ_DYN_NONE : dynf_class(segment, V, mode == DMXQ_DYNF_ROWS) == DMXQ_DYN_NONE)
    return segment == 0 ? DMXQ_OK : DMXQ_ERR_UNSUPPORTED;
  if (n_segments == 0) return DMXQ_OK;
  if (!aligned16(in) || !aligned16(out)) return DMXQ_ERR_UNSUPPORTED;
  const int64_t seg_elems = tile ? segment * segment : segment;
  if (n_segments > INT64_MAX / (seg_elems * 4)) return DMXQ_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
#define DMXQ_DYNF_GO(DT_)                                                                                    \
  return tile ? dynf_launch_tiles<DT_>(in, out, rows, cols, segment, f, scale_out, s)                         \
              : dynf_launch_segments<DT_>(in, out, n_segments, segment, mode == DMXQ_DYNF_ROWS, f, scale_out, s)
  if (dtype_in == DMXQ_BF16) DMXQ_DYNF_GO(DMXQ_BF16);
  if (dtype_in == DMXQ_F16) DMXQ_DYNF_GO(DMXQ_F16);
  DMXQ_DYNF_GO(DMXQ_F32);
#undef DMXQ_DYNF_GO
}
