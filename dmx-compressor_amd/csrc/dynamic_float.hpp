// csrc/dynamic_float.hpp — the device pieces that the casts scaled by a segment's absolute maximum share: the scale rule
// and the IEEE quotient of csrc/dynamic_float.hip (include/dmxq.h dmxq_dynamic_float_qdq), used as well by csrc/codebook.hip (the
// codebook cast, dmxq_codebook_qdq), and the row-class split of the two.  ONE copy: what the kernels compute from the same values is the
// same bits by construction.
#pragma once
#include <math.h>

#include "dynamic_geom.hpp"

namespace dmxq {

// a segment's scale and its reciprocal, from the bits of its absolute maximum: s = amax / fmax (an IEEE division), rounded UP to a power
// of two on its bits under pow2, and 1 when it is not finite or below 2^-126 (an all-zero, a NaN or an Inf segment, an fmax of 0)
struct DfSeg {
  float s, rs;
  __device__ __forceinline__ void setup(uint32_t amax_bits, float fmax, int pow2) {
    float t = u2f(amax_bits) / fmax;
    if (pow2) {
      const uint32_t b = f2u(t);
      t = u2f((b & 0x7F800000u) + ((b & 0x007FFFFFu) ? 0x00800000u : 0u));
    }
    s = (t >= 0x1p-126f && t < INFINITY) ? t : 1.0f;
    rs = 1.0f / s;
  }
};

// q = x / s, the IEEE quotient, called by whole waves; `fast`: every scale of the wave lies inside the reciprocal's range (wave-uniform).
// common.hpp div_by_recip where it is proven bit-equal to the division; lanes holding anything else, and every lane of a wave with a
// scale outside that range, redo their vector with `/` behind one cold wave-uniform branch.
template <int V>
__device__ __forceinline__ void df_quotient_vec(const float (&x)[V], float (&q)[V], const DfSeg& sg, bool fast) {
  bool ok = fast;
#pragma unroll
  for (int k = 0; k < V; k++) { q[k] = div_by_recip(x[k], sg.s, sg.rs); ok = ok && div_by_recip_ok(x[k]); }
  if (__builtin_expect(__builtin_amdgcn_ballot_w64(!ok) != 0ull, 0)) {
    if (!ok) {
#pragma unroll
      for (int k = 0; k < V; k++) q[k] = x[k] / sg.s;
    }
  }
}

// the maximum of a workgroup's waves (WAVES > 1): through LDS
template <int WAVES>
__device__ __forceinline__ uint32_t df_block_max(uint32_t m) {
  if constexpr (WAVES > 1) {
    __shared__ uint32_t s_max[WAVES];
    if ((threadIdx.x & (kWave - 1)) == 0) s_max[threadIdx.x / kWave] = m;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < WAVES; i++) m = max(m, s_max[i]);
  }
  return m;
}

// dynamic_geom.hpp's rule, except that a wave keeps a row only up to 8 sixteen-bit vectors per lane (16 for fp32): 16 sixteen-bit
// vectors with their 128 widened elements and the casts' fallbacks no longer unroll (the raw vectors would go to scratch), and a
// workgroup holds such a row with 8 per lane
inline int dynf_class(int64_t S, int V, bool whole_rows) {
  const int cls = dyn_class(S, V, whole_rows);
  return (cls == DMXQ_DYN_WAVE_ROW && V == 8 && S / V > 8 * kWave) ? DMXQ_DYN_BLOCK_ROW : cls;
}

}  // namespace dmxq
