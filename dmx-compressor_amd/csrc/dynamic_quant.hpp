// csrc/dynamic_quant.hpp — the device pieces of the dynamic per-segment integer cast (include/dmxq.h dmxq_dynamic_fixed_qdq),
// shared by csrc/dynamic_quant.hip (the cast itself) and csrc/awq.hip (the same cast on a weight scaled in registers): a segment's
// extrema with dmxq_group_minmax's NaN rule, their combine over the segment's adjacent lanes, (scale, zero point) by qparams_one, and the
// cast of a lane's vector with the reciprocal / division rule of csrc/dynamic_quant.hip's header comment.  ONE copy: what the two
// kernels compute from the same values is the same bits by construction.
#pragma once
#include <math.h>

#include "fixedq.hpp"
#include "reduce_common.hpp"

namespace dmxq {

struct DynFmt {
  float t_min, t_max;
  int qmin, qmax, sym;
};

struct DynExt : FloatExtrema {   // (reduce_common.hpp: the float accumulation and the NaN rule, shared with GPTQ's group scan)
  template <int DT, int V>
  __device__ __forceinline__ void add(const u32x4& raw) {
    float x[V];
    widen<DT, V>(raw, x);
#pragma unroll
    for (int k = 0; k < V; k++) FloatExtrema::add(x[k]);
  }
  // -> keys; a NaN anywhere: (-NaN, +NaN), which win every min / max of the combine
  __device__ __forceinline__ void keys(uint32_t& klo, uint32_t& khi) const {
    klo = fkey(mn());
    khi = fkey(mx());
  }
};

// min / max over aligned groups of `lanes` adjacent lanes (a wave-uniform power of two): the DPP stages run unconditionally and are kept
// or dropped by a select on a scalar condition (common.hpp group_max_u32)
__device__ __forceinline__ void dyn_group_minmax(uint32_t& lo, uint32_t& hi, int lanes) {
#define DMXQ_DYN_DPP(ctrl, n)                                                                                          \
  {                                                                                                                    \
    const uint32_t a = min(lo, (uint32_t)__builtin_amdgcn_update_dpp((int)lo, (int)lo, ctrl, 0xF, 0xF, false));       \
    const uint32_t b = max(hi, (uint32_t)__builtin_amdgcn_update_dpp((int)hi, (int)hi, ctrl, 0xF, 0xF, false));       \
    lo = lanes >= n ? a : lo;                                                                                          \
    hi = lanes >= n ? b : hi;                                                                                          \
  }
  DMXQ_DYN_DPP(0xB1, 2)    // quad_perm 1,0,3,2
  DMXQ_DYN_DPP(0x4E, 4)    // quad_perm 2,3,0,1
  DMXQ_DYN_DPP(0x141, 8)   // row_half_mirror
  DMXQ_DYN_DPP(0x140, 16)  // row_mirror
#undef DMXQ_DYN_DPP
  if (lanes >= 32) { lo = min(lo, (uint32_t)__shfl_xor((int)lo, 16)); hi = max(hi, (uint32_t)__shfl_xor((int)hi, 16)); }
  if (lanes >= 64) { lo = min(lo, (uint32_t)__shfl_xor((int)lo, 32)); hi = max(hi, (uint32_t)__shfl_xor((int)hi, 32)); }
}

// the cast of a segment, as its lanes hold it
struct DynSeg {
  float sc, rs, z;
  int64_t zp;
  __device__ __forceinline__ void setup(uint32_t klo, uint32_t khi, const DynFmt& f) {
    qparams_one(fkey_inv(klo), fkey_inv(khi), f.qmin, f.qmax, f.sym, sc, zp);
    z = (float)zp;
    rs = 1.0f / sc;
  }
};

// FixedOp<.., SIMPLE>::q with the IEEE division
__device__ __forceinline__ float dyn_q_exact(float x, float sc, float z, const DynFmt& f) {
  const float t = x / sc + z;
  float v = rintf((t + 0.5f) - 0.5f);
  v = v > f.t_max ? f.t_max : (v < f.t_min ? f.t_min : v);
  return (v - z) * sc;
}

// called by whole waves; the recipe is chosen per wave (every segment of the wave inside the reciprocal's range; every zero point 0)
template <int V>
__device__ __forceinline__ void dyn_cast_vec(const float (&x)[V], float (&y)[V], const DynSeg& s, bool all_fast, bool all_zp0, const DynFmt& f) {
  if (all_fast) {
    const bool special = all_zp0 ? affine_int_pairs<V, true>(x, y, s.sc, s.rs, 0.0f, f.t_min, f.t_max)
                                 : affine_int_pairs<V, false>(x, y, s.sc, s.rs, s.z, f.t_min, f.t_max);
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(special) != 0ull, 0)) {
      if (special) {
#pragma unroll
        for (int k = 0; k < V; k++) y[k] = dyn_q_exact(x[k], s.sc, s.z, f);
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < V; k++) y[k] = dyn_q_exact(x[k], s.sc, s.z, f);
  }
}

// THE ADJACENT-PAIR TREE SUM of DESIGN.md §8 (HQQ, AWQ clipping), shared by csrc/hqq.hip and csrc/awq_clip.hip:
// the sum over aligned groups of `lanes` adjacent lanes, every lane of a group ending with the same bits: the stages run
// unconditionally and are kept or dropped by a select on a scalar condition (dyn_group_minmax's form)
__device__ __forceinline__ float hqq_group_sum(float v, int lanes) {
#define DMXQ_HQQ_DPP(ctrl, n)                                                                                   \
  {                                                                                                              \
    const float o = u2f((uint32_t)__builtin_amdgcn_update_dpp((int)f2u(v), (int)f2u(v), ctrl, 0xF, 0xF, false)); \
    const float a = v + o;                                                                                       \
    v = lanes >= n ? a : v;                                                                                      \
  }
  DMXQ_HQQ_DPP(0xB1, 2)    // quad_perm 1,0,3,2
  DMXQ_HQQ_DPP(0x4E, 4)    // quad_perm 2,3,0,1
  DMXQ_HQQ_DPP(0x141, 8)   // row_half_mirror
  DMXQ_HQQ_DPP(0x140, 16)  // row_mirror
#undef DMXQ_HQQ_DPP
  if (lanes >= 32) v = v + __shfl_xor(v, 16);
  if (lanes >= 64) v = v + __shfl_xor(v, 32);
  return v;
}

// the adjacent-pair tree inside a lane's vector
template <int V>
__device__ __forceinline__ float hqq_vec_sum(float (&t)[V]) {
#pragma unroll
  for (int w = V / 2; w >= 1; w /= 2) {
#pragma unroll
    for (int k = 0; k < w; k++) t[k] = t[2 * k] + t[2 * k + 1];
  }
  return t[0];
}

}  // namespace dmxq
