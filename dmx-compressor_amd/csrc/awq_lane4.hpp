// csrc/awq_lane4.hpp — a lane's FOUR consecutive weight elements, whatever the dtype: the load, widening, rounding and store shared by
// csrc/awq.hip (one candidate scale's error) and csrc/awq_clip.hip (the clip search).  ONE copy of each.
#pragma once
#include "common.hpp"

namespace dmxq {

constexpr int kAwqV = 4;   // elements per lane

// four consecutive elements of dtype DT, raw: 16 bytes (fp32) or 8 (16-bit); plain loads -- a search reads the same weight once per candidate
template <int DT>
__device__ __forceinline__ u32x4 awq_load4(const void* p, int64_t vec) {
  if (DT == DMXQ_F32) return *(const u32x4*)((const char*)p + vec * 16);
  const u32x2 v = *(const u32x2*)((const char*)p + vec * 8);
  return u32x4{v.x, v.y, 0u, 0u};
}
template <int DT>
__device__ __forceinline__ void awq_widen4(const u32x4& v, float (&x)[kAwqV]) {
  if (DT == DMXQ_F32) {
#pragma unroll
    for (int j = 0; j < 4; j++) x[j] = u2f(v[j]);
  } else {
#pragma unroll
    for (int j = 0; j < 2; j++) {
      if (DT == DMXQ_BF16) { x[2 * j] = u2f(v[j] << 16); x[2 * j + 1] = u2f(v[j] & 0xFFFF0000u); }
      else { x[2 * j] = half_lo(v[j]); x[2 * j + 1] = half_hi(v[j]); }
    }
  }
}
// fp32 -> DT (one rounding, the store's) -> fp32: the value the next launch of the chain would read back; the packed words are kept
template <int DT>
__device__ __forceinline__ u32x4 awq_round4(float (&x)[kAwqV]) {
  u32x4 r;
  if (DT == DMXQ_F32) {
    r = u32x4{f2u(x[0]), f2u(x[1]), f2u(x[2]), f2u(x[3])};
  } else {
    r = u32x4{pack2<DT>(x[0], x[1]), pack2<DT>(x[2], x[3]), 0u, 0u};
    awq_widen4<DT>(r, x);
  }
  return r;
}
template <int DT>
__device__ __forceinline__ void awq_store4(void* p, int64_t vec, const u32x4& r) {
  if (DT == DMXQ_F32) *(u32x4*)((char*)p + vec * 16) = r;
  else *(u32x2*)((char*)p + vec * 8) = u32x2{r.x, r.y};
}

}  // namespace dmxq
