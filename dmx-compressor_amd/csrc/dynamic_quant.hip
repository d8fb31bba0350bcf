// csrc/dynamic_quant.hip — dynamic per-token / per-group integer cast in ONE launch (include/dmxq.h dmxq_dynamic_fixed_qdq).
// Not in the reference, whose integer casts read scales that a calibration run left behind: here every segment of S consecutive
// elements derives its (scale, zero point) from its own extrema on every call -- the W8A8 recipe's per-token activations -- with the
// reference's two formulas (numerical/observer.py:59-115 -> reduce_common.hpp qparams_one; numerical/cast.py:278-296 -> FixedOp).
//
// The contract is the library's own three-launch chain on x.reshape(-1, S), bit for bit, scale and zero point included:
//   dmxq_group_minmax (one group per segment) -> dmxq_qparams -> dmxq_fixed_qdq (one scale per segment), that is:
//   * (mn, mx) = the segment's minimum and maximum as VALUES (the sign of a zero extremum cannot reach the result: qparams_one takes
//     fminf(mn, 0) / fmaxf(mx, 0), whose zero ends up in a sum, a quotient that rounds to 0, or below eps); ONE NaN anywhere in the
//     segment makes BOTH extrema NaN (torch.amin / amax propagate it; reduce.hip nan_to_both), which qparams_one's fminf / fmaxf then
//     DROP: min_neg = max_pos = 0, scale = eps, zero point = qmin under an affine scheme.  +-Inf is an ordinary extremum (scale Inf).
//   * (scale, zp) = qparams_one(mn, mx, qmin, qmax, symmetric_qscheme);
//   * y = (clamp(rne(x / scale + zp)) - zp) * scale in fp32 with an IEEE division, rne(t) = rintf((t + 0.5f) - 0.5f) (the clamped
//     integer formats' form of sim_helper.cpp round: elementwise.hip FixedOp<.., SIMPLE>), one rounding to the output dtype.  The
//     quotient comes from the reciprocal form (common.hpp affine_int_pairs, without its + zp / - zp steps when every zero point of the
//     wave is 0) when recip_ok(scale) holds for every segment of the wave, from the division otherwise (an all-zero segment: scale =
//     eps = 2^-23 < 2^-20); lanes with an Inf / NaN quotient redo their vector with the division.
//
// Geometry.  A lane moves 16-byte vectors (V = 8 sixteen-bit or 4 fp32 elements), held RAW in registers between the extrema pass and
// the cast: one read and one write per element.
//   * segments inside a wave (S = 16 .. 256, a power of two): flat, S / V adjacent lanes per segment, extrema by DPP / xor shuffles
//     over those lanes on order-preserving keys (reduce_common.hpp fkey); a wave takes U x 64 consecutive vectors, the grid does not
//     loop.  Lanes past the end re-read the last vector, meet only each other (the tensor ends on a segment boundary) and store nothing.
//   * whole rows (any S % V == 0 up to 16384): a wave per row while the row fits 16 vectors per lane (S <= 1024 V), four rows per
//     workgroup; a 256-thread workgroup per row above that, the four waves' extrema exchanged through LDS.  The vector count per lane
//     is a template argument (1, 2, 4, 8, 16): a lane whose slot lies past the row re-reads the row's last vector and stores nothing.
// Every segment is read completely before any of it is written.  No workspace, no synchronisation with the host: capturable.
#include <math.h>

#include "dynamic_geom.hpp"
#include "dynamic_quant.hpp"   // DynFmt, DynExt, dyn_group_minmax, DynSeg, dyn_q_exact, dyn_cast_vec: shared with csrc/awq.hip

namespace dmxq {
namespace {

// segments of `lanes` adjacent lanes; nvec = n_segments * lanes vectors in all; wave w takes vectors [w U 64, (w + 1) U 64)
template <int DT, int U>
__global__ __launch_bounds__(kDynThreads) void dyn_group_kernel(const void* __restrict__ in, void* __restrict__ out, int64_t nvec, int lanes,
                                                               int lanes_log2, const DynFmt f, float* __restrict__ scale_out,
                                                               int64_t* __restrict__ zp_out) {
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
    DynExt e;
    e.init();
    e.add<DT, V>(raw[u]);
    uint32_t klo, khi;
    e.keys(klo, khi);
    dyn_group_minmax(klo, khi, lanes);
    DynSeg s;
    s.setup(klo, khi, f);
    const bool all_fast = __builtin_amdgcn_ballot_w64(!recip_ok(s.sc)) == 0ull;
    const bool all_zp0 = __builtin_amdgcn_ballot_w64(s.z != 0.0f) == 0ull;
    float x[V], y[V];
    widen<DT, V>(raw[u], x);
    dyn_cast_vec<V>(x, y, s, all_fast, all_zp0, f);
    if (i < nvec) {
      store_vec<DT, V>(out, i * V, y);
      if ((lane & (lanes - 1)) == 0) {
        const int64_t g = i >> lanes_log2;
        if (scale_out) scale_out[g] = s.sc;
        if (zp_out) zp_out[g] = s.zp;
      }
    }
  }
}

// rows of nv vectors; WAVES = 1: a wave per row, four rows per workgroup; WAVES = 4: the workgroup's row.  U x 64 x WAVES >= nv.
template <int DT, int U, int WAVES>
__global__ __launch_bounds__(kDynThreads) void dyn_rows_kernel(const void* __restrict__ in, void* __restrict__ out, int64_t rows, int nv,
                                                              const DynFmt f, float* __restrict__ scale_out, int64_t* __restrict__ zp_out) {
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
    raw[u] = load_raw16<true>(in, (v0 + (v < nv ? v : nv - 1)) * 16);   // clamped: a repeated vector cannot change a min / max
  }
  DynExt e;
  e.init();
#pragma unroll
  for (int u = 0; u < U; u++) e.add<DT, V>(raw[u]);
  uint32_t klo, khi;
  e.keys(klo, khi);
  dyn_group_minmax(klo, khi, kWave);
  if constexpr (WAVES > 1) {
    __shared__ uint32_t s_lo[WAVES], s_hi[WAVES];
    const int w = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) { s_lo[w] = klo; s_hi[w] = khi; }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < WAVES; i++) { klo = min(klo, s_lo[i]); khi = max(khi, s_hi[i]); }
  }
  DynSeg s;
  s.setup(klo, khi, f);
  // one segment per wave: the recipe is wave-uniform
  const bool all_fast = __builtin_amdgcn_ballot_w64(!recip_ok(s.sc)) == 0ull;
  const bool all_zp0 = __builtin_amdgcn_ballot_w64(s.z != 0.0f) == 0ull;
  if (t == 0 && row_ok) {
    if (scale_out) scale_out[row] = s.sc;
    if (zp_out) zp_out[row] = s.zp;
  }
#pragma unroll
  for (int u = 0; u < U; u++) {
    const int v = t + u * T;
    float x[V], y[V];
    widen<DT, V>(raw[u], x);
    dyn_cast_vec<V>(x, y, s, all_fast, all_zp0, f);
    if (v < nv && row_ok) store_vec<DT, V>(out, (v0 + v) * V, y);
  }
}

template <int DT>
int dyn_launch(const void* in, void* out, int64_t n_segments, int64_t S, bool whole_rows, const DynFmt& f, float* scale_out, int64_t* zp_out,
               hipStream_t s) {
  constexpr int V = 16 / Elem<DT>::bytes;
  const int64_t nv = S / V;   // vectors per segment
  const int cls = dyn_class(S, V, whole_rows);
  if (cls == DMXQ_DYN_NONE) return DMXQ_ERR_UNSUPPORTED;
  if (cls == DMXQ_DYN_GROUP) {
    const int lanes = (int)nv;   // 2 .. 64
    int l2 = 0;
    while ((1 << l2) < lanes) l2++;
    const int64_t nvec = n_segments * nv;
    // one vector per lane while that already fills the device (about 8 waves per SIMD of 256 CUs), four independent loads per lane beyond
    const bool deep = plan_norm(nvec) > ((int64_t)1 << 19);
    const int64_t per_wg = (int64_t)kDynThreads * (deep ? 4 : 1);
    const int64_t grid = (nvec + per_wg - 1) / per_wg;
    if (grid > 0x7FFFFFFF) return DMXQ_ERR_UNSUPPORTED;
    if (deep) DMXQ_LAUNCH((dyn_group_kernel<DT, 4>), dim3((unsigned)grid), dim3(kDynThreads), 0, s, in, out, nvec, lanes, l2, f, scale_out, zp_out);
    else DMXQ_LAUNCH((dyn_group_kernel<DT, 1>), dim3((unsigned)grid), dim3(kDynThreads), 0, s, in, out, nvec, lanes, l2, f, scale_out, zp_out);
    return launch_status();
  }
  const bool wave_row = cls != DMXQ_DYN_BLOCK_ROW;
  const int64_t rpb = wave_row ? kDynThreads / kWave : 1;
  const int64_t grid = (n_segments + rpb - 1) / rpb;
  if (grid > 0x7FFFFFFF) return DMXQ_ERR_UNSUPPORTED;
  const int64_t per_lane = (nv + (wave_row ? kWave : kDynThreads) - 1) / (wave_row ? kWave : kDynThreads);
#define DMXQ_DYN_ROWS(U_, W_) \
  DMXQ_LAUNCH((dyn_rows_kernel<DT, U_, W_>), dim3((unsigned)grid), dim3(kDynThreads), 0, s, in, out, n_segments, (int)nv, f, scale_out, zp_out)
  if (wave_row) {
    if (per_lane <= 1) DMXQ_DYN_ROWS(1, 1);
    else if (per_lane <= 2) DMXQ_DYN_ROWS(2, 1);
    else if (per_lane <= 4) DMXQ_DYN_ROWS(4, 1);
    else if (per_lane <= 8) DMXQ_DYN_ROWS(8, 1);
    else DMXQ_DYN_ROWS(16, 1);
  } else {
    if (per_lane <= 8) DMXQ_DYN_ROWS(8, 4);
    else DMXQ_DYN_ROWS(16, 4);
  }
#undef DMXQ_DYN_ROWS
  return launch_status();
}

}  // namespace
}  // namespace dmxq

using namespace dmxq;

extern "C" int dmxq_dynamic_class(int dtype, int64_t segment, int whole_rows) {
  if (!valid_dtype(dtype)) return DMXQ_DYN_NONE;
  return dyn_class(segment, dtype == DMXQ_F32 ? 4 : 8, whole_rows != 0);
}

extern "C" int dmxq_dynamic_fixed_qdq(const void* in, void* out, int dtype_in, int dtype_out, int64_t n_segments, int64_t segment,
                                      int whole_rows, int precision, int fraction, int clamp, int symmetric, int rounding, int qmin, int qmax,
                                      int symmetric_qscheme, float* scale_out, int64_t* zp_out, void* stream) {
  if (!valid_dtype(dtype_in) || !valid_dtype(dtype_out) || !valid_rounding(rounding)) return DMXQ_ERR_BAD_ARG;
  if (n_segments < 0 || segment < 0 || precision < 1 || qmax <= qmin) return DMXQ_ERR_BAD_ARG;
  if (n_segments > 0 && segment > 0 && (!in || !out)) return DMXQ_ERR_BAD_ARG;
  // what the kernels take; everything else is the caller's chain (nothing launched)
  if (dtype_in != dtype_out || rounding != DMXQ_ROUND_NEAREST || fraction != 0 || !clamp || precision > 22) return DMXQ_ERR_UNSUPPORTED;
  const int V = dtype_in == DMXQ_F32 ? 4 : 8;
  if (segment % V != 0 || segment > kDynMaxRow) return DMXQ_ERR_UNSUPPORTED;
  if (n_segments == 0 || segment == 0) return DMXQ_OK;
  if (!aligned16(in) || !aligned16(out)) return DMXQ_ERR_UNSUPPORTED;
  if (n_segments > INT64_MAX / (segment * 4)) return DMXQ_ERR_UNSUPPORTED;
  const FixedFmt x = make_fixed_fmt(precision, 0, 1, symmetric, DMXQ_ROUND_NEAREST, 0ull);
  const DynFmt f{x.t_min, x.t_max, qmin, qmax, symmetric_qscheme ? 1 : 0};
  hipStream_t s = (hipStream_t)stream;
  if (dtype_in == DMXQ_BF16) return dyn_launch<DMXQ_BF16>(in, out, n_segments, segment, whole_rows != 0, f, scale_out, zp_out, s);
  if (dtype_in == DMXQ_F16) return dyn_launch<DMXQ_F16>(in, out, n_segments, segment, whole_rows != 0, f, scale_out, zp_out, s);
  return dyn_launch<DMXQ_F32>(in, out, n_segments, segment, whole_rows != 0, f, scale_out, zp_out, s);
}
