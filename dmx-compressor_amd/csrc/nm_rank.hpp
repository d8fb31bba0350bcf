// csrc/nm_rank.hpp — the N:M rank rule and the unit I/O of the vectorised mask kernels, shared by csrc/nm_mask.hip (a stored score)
// and csrc/wanda.hip (a score formed in registers from the weight and the activation norms).
//
// Rank rule (pinned by tests/golden/nm_mask_*.npz against the reference): ascending STABLE order, NaN last:
//   before(j, i) = s_j < s_i  or  (s_j == s_i or both NaN) and j < i   [NaN is "greater" than any number]
//   rank_i = #{j : before(j, i)} ;  mask_i = (rank_i >= M - K) ? 1 : 0
#pragma once
#include "common.hpp"

namespace dmxq {

// key that orders like the reference's sort: monotone map of the float to a signed-comparable integer,
// -0.0 == +0.0, every NaN maps to the same top key.
__device__ __forceinline__ int32_t sort_key(float s) {
  if (s != s) return 0x7FFFFFFF;
  if (s == 0.0f) return 0;
  const int32_t b = (int32_t)f2u(s);
  return b >= 0 ? b : (int32_t)(0x80000000u - (uint32_t)b);
}

// rank of every key of one group: M(M-1)/2 comparisons in registers, no sort, no indices
template <int M>
__device__ __forceinline__ void nm_rank(const int32_t (&key)[M], int (&rank)[M]) {
#pragma unroll
  for (int i = 0; i < M; i++) rank[i] = 0;
#pragma unroll
  for (int i = 0; i < M; i++)
#pragma unroll
    for (int jj = 0; jj < i; jj++) {
      // jj < i: on equal keys the lower index jj sorts first
      const bool jj_first = key[jj] <= key[i];
      rank[i] += jj_first ? 1 : 0;
      rank[jj] += jj_first ? 0 : 1;
    }
}

// the 0 / 1 mask of the U / M whole groups a lane's unit of U scores holds
template <int M, int U>
__device__ __forceinline__ void nm_unit_mask(const float (&s)[U], int K, float (&mk)[U]) {
  static_assert(U % M == 0, "whole groups");
#pragma unroll
  for (int g = 0; g < U; g += M) {
    int32_t key[M];
    int rank[M];
#pragma unroll
    for (int i = 0; i < M; i++) key[i] = sort_key(s[g + i]);
    nm_rank<M>(key, rank);
#pragma unroll
    for (int i = 0; i < M; i++) mk[g + i] = rank[i] >= M - K ? 1.0f : 0.0f;
  }
}

// A lane's unit of U = 8 or 16 consecutive elements, moved with 16-byte accesses (one per 8 sixteen-bit elements, one per 4 fp32
// elements); the dtype is a wave-uniform run-time value.
template <int U>
__device__ __forceinline__ void load_elems(const void* p, int dt, int64_t e0, float (&v)[U]) {
  if (dt == DMXQ_F32) {
#pragma unroll
    for (int k = 0; k < U; k += 4) {
      const f32x4 t = *(const f32x4*)((const float*)p + e0 + k);
      v[k] = t.x; v[k + 1] = t.y; v[k + 2] = t.z; v[k + 3] = t.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < U; k += 8) {
      const u32x4 t = *(const u32x4*)((const uint16_t*)p + e0 + k);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        if (dt == DMXQ_BF16) {
          v[k + 2 * j] = u2f(t[j] << 16);
          v[k + 2 * j + 1] = u2f(t[j] & 0xFFFF0000u);
        } else {
          v[k + 2 * j] = half_lo(t[j]);
          v[k + 2 * j + 1] = half_hi(t[j]);
        }
      }
    }
  }
}

template <int U>
__device__ __forceinline__ void store_elems(void* p, int dt, int64_t e0, const float (&v)[U]) {
  if (dt == DMXQ_F32) {
#pragma unroll
    for (int k = 0; k < U; k += 4) *(f32x4*)((float*)p + e0 + k) = f32x4{v[k], v[k + 1], v[k + 2], v[k + 3]};
  } else {
#pragma unroll
    for (int k = 0; k < U; k += 8) {
      u32x4 t;
#pragma unroll
      for (int j = 0; j < 4; j++)
        t[j] = dt == DMXQ_BF16 ? pack2<DMXQ_BF16>(v[k + 2 * j], v[k + 2 * j + 1]) : pack2<DMXQ_F16>(v[k + 2 * j], v[k + 2 * j + 1]);
      *(u32x4*)((uint16_t*)p + e0 + k) = t;
    }
  }
}

}  // namespace dmxq
