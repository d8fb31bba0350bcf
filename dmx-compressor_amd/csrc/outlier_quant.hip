// csrc/outlier_quant.hip — outlier-aware dynamic integer cast in ONE launch (include/dmxq.h dmxq_outlier_fixed_qdq; DESIGN.md §8
// "Outlier-aware dynamic cast"; SpQR, Dettmers et al. 2023; SqueezeLLM, Kim et al. 2023).  Not in the reference.  Every group of g
// consecutive elements keeps its k largest magnitudes EXACT (or in a per-element float format) and casts the rest with the dynamic
// cast's (scale, zero point) of the group WITHOUT them.  The contract is DESIGN.md §8's text: rank by the bit pattern of |x| as float32
// (a NaN above Inf above every finite value), equal patterns to the LOWER index; the k winners are replaced by +0.0 and the group goes
// through dmxq_dynamic_fixed_qdq's arithmetic (qparams_one takes min(mn, 0) / max(mx, 0), so a zero in a winner's place gives the
// qparams of the other elements alone); the winners come back as O(x).
//
// Geometry: dyn_class's DMXQ_DYN_GROUP only -- g a power of two from 16 to 256, g / V adjacent lanes of a wave per group, a lane
// holding ONE 16-byte vector (V = 8 sixteen-bit or 4 fp32 elements).  A wave takes 64 consecutive vectors per round of a grid-stride
// loop (csrc/hqq.hip's form).  Lanes past the tensor's end hold zeros, take part in every stage (the tensor ends on a group boundary,
// so they meet only each other) and store nothing.
//
// Selection: k rounds on registers (k is wave-uniform: one scalar loop).  An element's key is 0 once it is marked.
//   * 16-bit inputs: key = 1 << 23 | (the 15 magnitude bits of the element) << 8 | (255 - position in the group).  Widening bf16 /
//     fp16 to float32 is strictly monotone on magnitude patterns, so the 15 bits order as the float32 patterns do, and the inverted
//     position makes the key unique in its group: ONE integer maximum over the group's lanes (common.hpp group_max_u32) names the winner.
//   * float32 inputs: key = 1 << 31 | the 31 magnitude bits; a second maximum, of 256 - position over the holders of the first, picks
//     the lowest index among equal patterns.
//   The winner marks itself by a select (no array is indexed at run time: no scratch, build.py NO_SCRATCH) and, where the caller asked
//   for them, stores its position and O(x) with ordinary vector-memory stores.
// Cast: the marked elements are zeroed in the RAW vector, then DynExt, dyn_group_minmax, DynSeg::setup and dyn_cast_vec of
// csrc/dynamic_quant.hpp run unchanged: the dynamic kernel's bits by construction.  O(x) is the raw input pattern, or floatq.hpp's
// castg_vec of the lane's vector (called by whole waves: it ballots), selected into the packed output words.
// No LDS, no atomics, no workspace, no host synchronisation: capturable.
#include <math.h>

#include "dynamic_geom.hpp"
#include "dynamic_quant.hpp"   // DynFmt, DynExt, dyn_group_minmax, DynSeg, dyn_cast_vec: the dynamic cast's own, ONE copy
#include "floatq.hpp"          // CastG, castg_vec: the per-element float cast of the outliers

namespace dmxq {
namespace {

constexpr int kOutlierBlocksPerCu = 6;   // the grid's cap: 6 workgroups of 4 waves per CU (75-78 VGPRs: 6 waves per SIMD), the rest by the grid-stride loop
constexpr int kOutlierMaxK = 8;

template <int DT>
__global__ __launch_bounds__(kDynThreads) void outlier_group_kernel(const void* __restrict__ in, void* __restrict__ out, int64_t nvec, int lanes,
                                                                   int lanes_log2, int k, const DynFmt f, const CastG c,
                                                                   float* __restrict__ scale_out, int64_t* __restrict__ zp_out,
                                                                   int32_t* __restrict__ idx_out, void* __restrict__ val_out) {
  constexpr int V = 16 / Elem<DT>::bytes;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = (int64_t)blockIdx.x * (kDynThreads / kWave) + threadIdx.x / kWave;
  const int64_t stride = (int64_t)gridDim.x * kDynThreads;   // vectors per round of the grid
  const int pos0 = (lane & (lanes - 1)) * V;                 // the position in the group of the lane's first element
  for (int64_t i0 = wave * kWave; i0 < nvec; i0 += stride) {   // (wave-uniform: whole waves loop)
    const int64_t i = i0 + lane;
    const bool ok = i < nvec;
    u32x4 raw = {0u, 0u, 0u, 0u};
    if (ok) raw = load_raw16<true>(in, i * 16);
    // O(x) of the lane's vector as packed words of the tensor's dtype
    u32x4 rep = raw;
    if (c.active) {   // (wave-uniform)
      float o[V];
      widen<DT, V>(raw, o);
      castg_vec<DT, V>(o, c);
      const OutVec<DT, V> p = pack_vec<DT, V>(o);
#pragma unroll
      for (int j = 0; j < 4; j++) rep[j] = p.w[j];
    }
    // the keys
    uint32_t key[V];
#pragma unroll
    for (int j = 0; j < V; j++) {
      if constexpr (V == 8) {
        const uint32_t mag = (raw[j / 2] >> (16 * (j & 1))) & 0x7FFFu;
        key[j] = 0x00800000u | (mag << 8) | (uint32_t)(255 - (pos0 + j));
      } else {
        key[j] = 0x80000000u | (raw[j] & 0x7FFFFFFFu);
      }
    }
    const int64_t g = i >> lanes_log2;
    for (int r = 0; r < k; r++) {   // (k is a kernel argument: a scalar loop)
      uint32_t cand = key[0];
#pragma unroll
      for (int j = 1; j < V; j++) cand = max(cand, key[j]);
      const uint32_t top = group_max_u32(cand, lanes);
      bool win[V];
      if constexpr (V == 8) {
#pragma unroll
        for (int j = 0; j < V; j++) win[j] = key[j] == top;
      } else {
        uint32_t inv = 0u;   // 256 - position of the lane's first holder of the largest pattern (0: it holds none)
#pragma unroll
        for (int j = V - 1; j >= 0; j--) inv = key[j] == top ? (uint32_t)(256 - (pos0 + j)) : inv;
        const uint32_t first = group_max_u32(inv, lanes);
#pragma unroll
        for (int j = 0; j < V; j++) win[j] = key[j] == top && (uint32_t)(256 - (pos0 + j)) == first;
      }
      if (idx_out) {   // (wave-uniform)
        bool won = false;
        int pos = 0;
        uint32_t bits = 0u;
#pragma unroll
        for (int j = 0; j < V; j++) {
          const uint32_t b = V == 8 ? (rep[j / 2] >> (16 * (j & 1))) & 0xFFFFu : rep[j % 4];
          won = won || win[j];
          pos = win[j] ? pos0 + j : pos;
          bits = win[j] ? b : bits;
        }
        if (won && ok) {
          const int64_t slot = g * k + r;
          idx_out[slot] = pos;
          if constexpr (V == 8) ((uint16_t*)val_out)[slot] = (uint16_t)bits;
          else ((uint32_t*)val_out)[slot] = bits;
        }
      }
#pragma unroll
      for (int j = 0; j < V; j++) key[j] = win[j] ? 0u : key[j];
    }
    // the marks as masks over the packed words; the inliers: the raw vector with +0.0 in the marked places
    u32x4 mask, rawz;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if constexpr (V == 8) mask[j] = (key[2 * j] == 0u ? 0x0000FFFFu : 0u) | (key[2 * j + 1] == 0u ? 0xFFFF0000u : 0u);
      else mask[j] = key[j] == 0u ? 0xFFFFFFFFu : 0u;
      rawz[j] = raw[j] & ~mask[j];
    }
    // the dynamic cast of the inliers (csrc/dynamic_quant.hip dyn_group_kernel's steps)
    DynExt e;
    e.init();
    e.add<DT, V>(rawz);
    uint32_t klo, khi;
    e.keys(klo, khi);
    dyn_group_minmax(klo, khi, lanes);
    DynSeg s;
    s.setup(klo, khi, f);
    const bool all_fast = __builtin_amdgcn_ballot_w64(!recip_ok(s.sc)) == 0ull;
    const bool all_zp0 = __builtin_amdgcn_ballot_w64(s.z != 0.0f) == 0ull;
    float x[V], y[V];
    widen<DT, V>(rawz, x);
    dyn_cast_vec<V>(x, y, s, all_fast, all_zp0, f);
    if (ok) {
      const OutVec<DT, V> p = pack_vec<DT, V>(y);
      u32x4 w;
#pragma unroll
      for (int j = 0; j < 4; j++) w[j] = (p.w[j] & ~mask[j]) | (rep[j] & mask[j]);
      *(u32x4*)((char*)out + i * 16) = w;
      if ((lane & (lanes - 1)) == 0) {
        if (scale_out) scale_out[g] = s.sc;
        if (zp_out) zp_out[g] = s.zp;
      }
    }
  }
}

template <int DT>
int outlier_launch(const void* in, void* out, int64_t n_segments, int64_t S, int k, const DynFmt& f, const CastG& c, float* scale_out,
                   int64_t* zp_out, int32_t* idx_out, void* val_out, hipStream_t s) {
  constexpr int V = 16 / Elem<DT>::bytes;
  if (dyn_class(S, V, false) != DMXQ_DYN_GROUP) return DMXQ_ERR_UNSUPPORTED;
  const int lanes = (int)(S / V);   // 2 .. 64
  int l2 = 0;
  while ((1 << l2) < lanes) l2++;
  const int64_t nvec = n_segments * lanes;
  const int64_t want = (nvec + kDynThreads - 1) / kDynThreads;
  const int64_t cap = (int64_t)plan_cus() * kOutlierBlocksPerCu;
  const unsigned grid = (unsigned)(want < cap ? want : cap);
  DMXQ_LAUNCH((outlier_group_kernel<DT>), dim3(grid), dim3(kDynThreads), 0, s, in, out, nvec, lanes, l2, k, f, c, scale_out, zp_out, idx_out, val_out);
  return launch_status();
}

}  // namespace
}  // namespace dmxq

using namespace dmxq;

extern "C" int dmxq_outlier_class(int dtype, int64_t segment) {
  if (!valid_dtype(dtype)) return DMXQ_DYN_NONE;
  return dyn_class(segment, dtype == DMXQ_F32 ? 4 : 8, false);
}

extern "C" int dmxq_outlier_fixed_qdq(const void* in, void* out, int dtype_in, int dtype_out, int64_t n_segments, int64_t segment, int k,
                                      int precision, int fraction, int clamp, int symmetric, int rounding, int qmin, int qmax,
                                      int symmetric_qscheme, const dmxq_float_fmt* outlier_format, float* scale_out, int64_t* zp_out,
                                      int32_t* idx_out, void* val_out, void* stream) {
  if (!valid_dtype(dtype_in) || !valid_dtype(dtype_out) || !valid_rounding(rounding)) return DMXQ_ERR_BAD_ARG;
  if (n_segments < 0 || segment < 0 || precision < 1 || qmax <= qmin || k < 0) return DMXQ_ERR_BAD_ARG;
  if (segment > 0 && k >= segment) return DMXQ_ERR_BAD_ARG;
  if ((idx_out == nullptr) != (val_out == nullptr)) return DMXQ_ERR_BAD_ARG;
  if (n_segments > 0 && segment > 0 && (!in || !out)) return DMXQ_ERR_BAD_ARG;
  // what the kernel takes; everything else is the caller's chain (nothing launched)
  if (dtype_in != dtype_out || rounding != DMXQ_ROUND_NEAREST || fraction != 0 || !clamp || precision > 22) return DMXQ_ERR_UNSUPPORTED;
  if (k < 1 || k > kOutlierMaxK) return DMXQ_ERR_UNSUPPORTED;
  if (dmxq_outlier_class(dtype_in, segment) != DMXQ_DYN_GROUP) return DMXQ_ERR_UNSUPPORTED;
  CastG c;
  if (!castg_of(outlier_format, &c)) return DMXQ_ERR_UNSUPPORTED;
  if (n_segments == 0) return DMXQ_OK;
  if (!aligned16(in) || !aligned16(out)) return DMXQ_ERR_UNSUPPORTED;
  if (idx_out && ((reinterpret_cast<uintptr_t>(idx_out) & 3u) || (reinterpret_cast<uintptr_t>(val_out) & 3u))) return DMXQ_ERR_UNSUPPORTED;
  if (n_segments > INT64_MAX / (segment * 4)) return DMXQ_ERR_UNSUPPORTED;
  const FixedFmt x = make_fixed_fmt(precision, 0, 1, symmetric, DMXQ_ROUND_NEAREST, 0ull);
  const DynFmt f{x.t_min, x.t_max, qmin, qmax, symmetric_qscheme ? 1 : 0};
  hipStream_t s = (hipStream_t)stream;
  if (dtype_in == DMXQ_BF16) return outlier_launch<DMXQ_BF16>(in, out, n_segments, segment, k, f, c, scale_out, zp_out, idx_out, val_out, s);
  if (dtype_in == DMXQ_F16) return outlier_launch<DMXQ_F16>(in, out, n_segments, segment, k, f, c, scale_out, zp_out, idx_out, val_out, s);
  return outlier_launch<DMXQ_F32>(in, out, n_segments, segment, k, f, c, scale_out, zp_out, idx_out, val_out, s);
}
