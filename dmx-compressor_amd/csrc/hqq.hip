// csrc/hqq.hip — Half-Quadratic Quantization in ONE launch (include/dmxq.h dmxq_hqq_qdq; DESIGN.md §8 "HQQ"; Badri and Shaji 2023).
// Not in the reference.  A calibration-free integer cast of a weight: every group of g consecutive elements keeps the min/max scale of
// the dynamic cast and re-solves its float ZERO POINT with `iters` proximal steps under an l_p norm (p <= 1), keeping per group the
// zero point whose L1 error was smallest.  The contract is DESIGN.md §8's text, which tests/_hqq_ref.py spells in CPU float32 and
// ops.hqq_qdq's chain in torch operations on the device: all three give the same bits.  Every operation below is a float32 one in the
// order of that text (build.py: -ffp-contract=off, IEEE division and square root).
//
// Geometry: dyn_class's DMXQ_DYN_GROUP only -- g a power of two from 16 to 256, g / V adjacent lanes of a wave per group, a lane
// holding ONE 16-byte vector (V = 8 sixteen-bit or 4 fp32 elements) widened once.  The loop runs on registers: load, iterate, store.
//   * extrema: DynExt + dyn_group_minmax (csrc/dynamic_quant.hpp), the dynamic cast's own;
//   * the two sums of an iteration (the error, the new zero point) in the ADJACENT-PAIR TREE order of the text: pairs inside the lane's
//     vector, then the lanes at distance 1, 2, 4, 8 (DPP), 16, 32 (shuffles).  Float addition commutes, so a + b in one lane and b + a
//     in its partner are the same bits; after the two quad stages a quad is uniform, so row_half_mirror (lane 7 - i) hands over the
//     value of the other quad exactly as an xor 4 would, and row_mirror the other half row's after that;
//   * z, z_best, err_best per group (uniform over the group's lanes), beta_k and 1 / beta_k uniform over the wave: one multiplication
//     and one division per iteration and lane, not per element (gfx950 has no scalar float unit to keep them in).
// A wave takes 64 consecutive vectors per round of a grid-stride loop.  Lanes past the tensor's end hold zeros, take part in every
// stage (the tensor ends on a group boundary, so they meet only each other) and store nothing.  No workspace, no host
// synchronisation: capturable.
#include <math.h>

#include "dynamic_geom.hpp"
#include "dynamic_quant.hpp"   // DynExt, dyn_group_minmax: the segment's extrema with dmxq_group_minmax's NaN rule, ONE copy

namespace dmxq {
namespace {

constexpr int kHqqBlocksPerCu = 4;   // the grid's cap: 4 workgroups of 4 waves per CU, the rest of the tensor by the grid-stride loop

struct HqqArgs {
  float qmin, qmax, range;   // range = qmax - qmin (exact: below 2^22)
  float beta, kappa, inv_g;
  int iters, code_bias;      // codes = q - qmin
};

// clamp(rint(x * rs + z), qmin, qmax): a NaN stays a NaN (torch.clamp's rule)
__device__ __forceinline__ float hqq_q(float x, float rs, float z, const HqqArgs& a) {
  const float v = rintf(x * rs + z);
  return v > a.qmax ? a.qmax : (v < a.qmin ? a.qmin : v);
}

// HALF: p = 0.5 (the shrink's threshold is (1 / beta) / sqrt(|d|)); else p = 1 (1 / beta)
template <int DT, bool HALF>
__global__ __launch_bounds__(kDynThreads) void hqq_group_kernel(const void* __restrict__ in, void* __restrict__ out, int64_t nvec, int lanes,
                                                               int lanes_log2, const HqqArgs a, float* __restrict__ scale_out,
                                                               float* __restrict__ zero_out, uint8_t* __restrict__ codes_out) {
  constexpr int V = 16 / Elem<DT>::bytes;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = (int64_t)blockIdx.x * (kDynThreads / kWave) + threadIdx.x / kWave;
  const int64_t stride = (int64_t)gridDim.x * kDynThreads;   // vectors per round of the grid
  for (int64_t i0 = wave * kWave; i0 < nvec; i0 += stride) {   // (wave-uniform: whole waves loop)
    const int64_t i = i0 + lane;
    const bool ok = i < nvec;
    u32x4 raw = {0u, 0u, 0u, 0u};
    if (ok) raw = load_raw16<true>(in, i * 16);
    // step 1
    DynExt e;
    e.init();
    e.add<DT, V>(raw);
    uint32_t klo, khi;
    e.keys(klo, khi);
    dyn_group_minmax(klo, khi, lanes);
    const float mn = fkey_inv(klo), mx = fkey_inv(khi);
    // step 2
    float s = (mx - mn) / a.range;
    s = (fabsf(s) < INFINITY && s >= 0x1p-126f) ? s : 1.0f;
    const float rs = 1.0f / s;
    // step 3
    float z = a.qmin - mn * rs;
    float b = a.beta;
    float x[V], q[V];
    widen<DT, V>(raw, x);
    // step 4
    float zb = z, eb = 0.0f;
    for (int k = 0;; k++) {
      float d[V], t[V];
#pragma unroll
      for (int j = 0; j < V; j++) {
        q[j] = hqq_q(x[j], rs, z, a);
        d[j] = x[j] - (q[j] - z) * s;
        t[j] = fabsf(d[j]);
      }
      const float err = hqq_group_sum(hqq_vec_sum<V>(t), lanes);
      const bool better = k == 0 || err < eb;   // (ordered: a NaN error never replaces the start)
      zb = better ? z : zb;
      eb = better ? err : eb;
      if (k == a.iters) break;
      const float ib = 1.0f / b;
#pragma unroll
      for (int j = 0; j < V; j++) {
        const float ad = fabsf(d[j]);
        const float th = HALF ? ib / sqrtf(ad) : ib;
        float m = ad - th;
        m = m < 0.0f ? 0.0f : m;   // (max(., 0) that keeps a NaN)
        const float sh = copysignf(m, d[j]);
        t[j] = q[j] - (x[j] - sh) * rs;
      }
      z = hqq_group_sum(hqq_vec_sum<V>(t), lanes) * a.inv_g;
      b = b * a.kappa;
    }
    // step 5
    float y[V];
#pragma unroll
    for (int j = 0; j < V; j++) {
      q[j] = hqq_q(x[j], rs, zb, a);
      y[j] = (q[j] - zb) * s;
    }
    if (ok) {
      store_vec<DT, V>(out, i * V, y);
      if (codes_out) {
        uint32_t w[V / 4];
#pragma unroll
        for (int j = 0; j < V / 4; j++) {
          w[j] = 0u;
#pragma unroll
          for (int c = 0; c < 4; c++) {
            const float qq = q[4 * j + c];
            const uint32_t code = qq == qq ? (uint32_t)((int)qq - a.code_bias) & 0xFFu : 0u;   // (a NaN code is stored as 0)
            w[j] |= code << (8 * c);
          }
        }
        if constexpr (V == 8) {
          const u32x2 cv = {w[0], w[1]};
          *(u32x2*)(codes_out + i * V) = cv;
        } else {
          *(uint32_t*)(codes_out + i * V) = w[0];
        }
      }
      if ((lane & (lanes - 1)) == 0) {
        const int64_t g = i >> lanes_log2;
        if (scale_out) scale_out[g] = s;
        if (zero_out) zero_out[g] = zb;
      }
    }
  }
}

template <int DT>
int hqq_launch(const void* in, void* out, int64_t n_segments, int64_t S, bool half, const HqqArgs& a, float* scale_out, float* zero_out,
               uint8_t* codes_out, hipStream_t s) {
  constexpr int V = 16 / Elem<DT>::bytes;
  if (dyn_class(S, V, false) != DMXQ_DYN_GROUP) return DMXQ_ERR_UNSUPPORTED;
  const int lanes = (int)(S / V);   // 2 .. 64
  int l2 = 0;
  while ((1 << l2) < lanes) l2++;
  const int64_t nvec = n_segments * lanes;
  const int64_t want = (nvec + kDynThreads - 1) / kDynThreads;
  const int64_t cap = (int64_t)plan_cus() * kHqqBlocksPerCu;
  const unsigned grid = (unsigned)(want < cap ? want : cap);
  if (half) DMXQ_LAUNCH((hqq_group_kernel<DT, true>), dim3(grid), dim3(kDynThreads), 0, s, in, out, nvec, lanes, l2, a, scale_out, zero_out, codes_out);
  else DMXQ_LAUNCH((hqq_group_kernel<DT, false>), dim3(grid), dim3(kDynThreads), 0, s, in, out, nvec, lanes, l2, a, scale_out, zero_out, codes_out);
  return launch_status();
}

}  // namespace
}  // namespace dmxq

using namespace dmxq;

extern "C" int dmxq_hqq_class(int dtype, int64_t group) {
  if (!valid_dtype(dtype)) return DMXQ_DYN_NONE;
  return dyn_class(group, dtype == DMXQ_F32 ? 4 : 8, false);
}

extern "C" int dmxq_hqq_qdq(const void* in, void* out, int dtype_in, int dtype_out, int64_t n_segments, int64_t segment, int rounding, int qmin,
                            int qmax, float lp_norm, float beta, float kappa, int iters, float* scale_out, float* zero_out, uint8_t* codes_out,
                            void* stream) {
  if (!valid_dtype(dtype_in) || !valid_dtype(dtype_out) || !valid_rounding(rounding)) return DMXQ_ERR_BAD_ARG;
  if (n_segments < 0 || segment < 0 || qmax <= qmin || iters < 0) return DMXQ_ERR_BAD_ARG;
  if (!(lp_norm > 0.0f && lp_norm <= 1.0f) || !(beta > 0.0f && beta < INFINITY) || !(kappa >= 1.0f && kappa < INFINITY)) return DMXQ_ERR_BAD_ARG;
  if (codes_out && (int64_t)qmax - qmin > 255) return DMXQ_ERR_BAD_ARG;
  if (n_segments > 0 && segment > 0 && (!in || !out)) return DMXQ_ERR_BAD_ARG;
  // what the kernel takes; everything else is the caller's chain (nothing launched)
  if (dtype_in != dtype_out || rounding != DMXQ_ROUND_NEAREST || (int64_t)qmax - qmin >= (1 << 22) || qmin < -(1 << 22) || qmax > (1 << 22))
    return DMXQ_ERR_UNSUPPORTED;
  if (lp_norm != 0.5f && lp_norm != 1.0f) return DMXQ_ERR_UNSUPPORTED;
  if (dmxq_hqq_class(dtype_in, segment) != DMXQ_DYN_GROUP) return DMXQ_ERR_UNSUPPORTED;
  if (n_segments == 0) return DMXQ_OK;
  if (!aligned16(in) || !aligned16(out) || (codes_out && (reinterpret_cast<uintptr_t>(codes_out) & 7u))) return DMXQ_ERR_UNSUPPORTED;
  if (n_segments > INT64_MAX / (segment * 4)) return DMXQ_ERR_UNSUPPORTED;
  const HqqArgs a{(float)qmin, (float)qmax, (float)(qmax - qmin), beta, kappa, 1.0f / (float)segment, iters, qmin};
  const bool half = lp_norm == 0.5f;
  hipStream_t s = (hipStream_t)stream;
  if (dtype_in == DMXQ_BF16) return hqq_launch<DMXQ_BF16>(in, out, n_segments, segment, half, a, scale_out, zero_out, codes_out, s);
  if (dtype_in == DMXQ_F16) return hqq_launch<DMXQ_F16>(in, out, n_segments, segment, half, a, scale_out, zero_out, codes_out, s);
  return hqq_launch<DMXQ_F32>(in, out, n_segments, segment, half, a, scale_out, zero_out, codes_out, s);
}
