// csrc/block_scaled_float.hip — two-level block-scaled low-bit float cast in ONE launch (include/dmxq.h dmxq_block_scaled_float_qdq;
// DESIGN.md §8 "Block-scaled float cast").  Not in the reference.  dynamic_float.hip keeps a group's scale as a full float32 number (or a
// power of two); a STORED block-scaled format keeps it in 8 bits -- E2M1 elements in blocks of 16 with an E4M3 block scale and one float32
// scale per tensor ("NVFP4"), E4M3 elements with quantised group scales -- and the quantisation of the scale is part of the error.
//
// The definition (fp32 throughout).  E: the element format with largest output fmax; Sf: the scale format with largest output sfmax;
// 0 < scale_max <= sfmax; t: the tensor scale, a DEVICE float (NULL: 1), replaced by 1 where it is not finite or below 2^-126.  Per group:
//   a  = max |x| over the group, ONE NaN anywhere makes it NaN (the maximum runs on the magnitude BITS, where a NaN pattern is largest)
//   c  = (a / fmax) / t, two IEEE divisions
//   sq = min(float_q_Sf(c), scale_max): the scale format's nearest cast with its flush flag, NaN / Inf saturating to sfmax (never NaN)
//   s  = sq * t, ONE fp32 multiply; USABLE when finite and >= 2^-126
//   usable:  y = float_q_E(x / s) * s -- an IEEE quotient, the format's nearest cast (NaN / Inf saturate), one multiply, one rounding
//   else:    y = a zero with the sign bit of float_q_E(x), and the reported s is 0 (an all-zero group; a group so far below the tensor's
//            maximum that its scale code is 0: a stored format holds zeros there)
// The quotient and the element cast are dynamic_float.hip's: common.hpp div_by_recip for a wave whose scales all lie inside [2^-20, 2^20]
// (recip_ok) and whose elements are +-0 or inside [2^-100, 2^100] (div_by_recip_ok), `/` behind one cold wave-uniform branch otherwise;
// floatq.hpp castg_vec for both casts (the scale's on one value).  An unusable group takes a second cold wave-uniform branch.
//
// Geometry: dynf_group_kernel's.  A lane moves one 16-byte vector (V = 8 sixteen-bit or 4 fp32 elements) held RAW in registers between
// the maximum and the cast; a group is g / V adjacent lanes (g a power of two from 16 to 256), its maximum by DPP / xor shuffles; four
// vectors per lane above 2^19 vectors.  Lanes past the end re-read the last vector and store nothing.  No workspace, no synchronisation
// with the host: capturable.  The scales go out as plain stores from one lane per group.  The dynamic tensor scale has a small reduction
// of its own below (dmxq_block_scaled_tensor_scale).
#include <math.h>

#include "dynamic_geom.hpp"
#include "floatq.hpp"

namespace dmxq {
namespace {

struct BsFmt {
  CastG e, sf;
  float fmax, scale_max;
};

// a group's scale code, scale and reciprocal, from the bits of its absolute maximum and the tensor scale
struct BsSeg {
  float s, rs, sq;
  bool usable;
  __device__ __forceinline__ void setup(uint32_t amax_bits, float t, const BsFmt& f) {   // (called by whole waves: castg_vec ballots)
    float c[1] = {(u2f(amax_bits) / f.fmax) / t};
    castg_vec<DMXQ_F32, 1>(c, f.sf);
    sq = fminf(c[0], f.scale_max);
    const float sv = sq * t;
    usable = sv >= 0x1p-126f && sv < INFINITY;
    s = usable ? sv : 1.0f;
    rs = 1.0f / s;
  }
};

// called by whole waves; `fast`: every scale of the wave lies inside the reciprocal's range (wave-uniform)
template <int V>
__device__ __forceinline__ void bs_cast_vec(const float (&x)[V], float (&y)[V], const BsSeg& sg, bool fast, const BsFmt& f) {
  float q[V];
  bool ok = fast;
#pragma unroll
  for (int k = 0; k < V; k++) { q[k] = div_by_recip(x[k], sg.s, sg.rs); ok = ok && div_by_recip_ok(x[k]); }
  if (__builtin_expect(__builtin_amdgcn_ballot_w64(!ok) != 0ull, 0)) {
    if (!ok) {
#pragma unroll
      for (int k = 0; k < V; k++) q[k] = x[k] / sg.s;
    }
  }
  castg_vec<DMXQ_F32, V>(q, f.e);
#pragma unroll
  for (int k = 0; k < V; k++) y[k] = q[k] * sg.s;
  if (__builtin_expect(__builtin_amdgcn_ballot_w64(!sg.usable) != 0ull, 0)) {   // (cold: a wave that holds an unusable group)
    float z[V];
#pragma unroll
    for (int k = 0; k < V; k++) z[k] = x[k];
    castg_vec<DMXQ_F32, V>(z, f.e);
#pragma unroll
    for (int k = 0; k < V; k++) y[k] = sg.usable ? y[k] : u2f(f2u(z[k]) & 0x80000000u);
  }
}

// groups of `lanes` adjacent lanes; nvec = n_groups * lanes vectors in all; wave w takes vectors [w U 64, (w + 1) U 64)
template <int DT, int U>
__global__ __launch_bounds__(kDynThreads) void bsf_group_kernel(const void* __restrict__ in, void* __restrict__ out, int64_t nvec, int lanes,
                                                               int lanes_log2, const BsFmt f, const float* __restrict__ tensor_scale,
                                                               float* __restrict__ scale_out, float* __restrict__ scale_q_out) {
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
  float t = tensor_scale ? *tensor_scale : 1.0f;   // (one address for the whole launch: a uniform load, once per wave)
  t = (t >= 0x1p-126f && t < INFINITY) ? t : 1.0f;
#pragma unroll
  for (int u = 0; u < U; u++) {
    const int64_t i = base + (int64_t)u * kWave;
    BsSeg sg;
    sg.setup(group_max_u32(absmax_bits<DT>(raw[u]), lanes), t, f);
    const bool fast = __builtin_amdgcn_ballot_w64(!recip_ok(sg.s)) == 0ull;
    float x[V], y[V];
    widen<DT, V>(raw[u], x);
    bs_cast_vec<V>(x, y, sg, fast, f);
    if (i < nvec) {
      store_vec<DT, V>(out, i * V, y);
      if ((lane & (lanes - 1)) == 0) {
        if (scale_out) scale_out[i >> lanes_log2] = sg.usable ? sg.s : 0.0f;
        if (scale_q_out) scale_q_out[i >> lanes_log2] = sg.sq;
      }
    }
  }
}

template <int DT>
int bsf_launch(const void* in, void* out, int64_t n_groups, int64_t g, const BsFmt& f, const float* tensor_scale, float* scale_out,
               float* scale_q_out, hipStream_t s) {
  constexpr int V = 16 / Elem<DT>::bytes;
  const int lanes = (int)(g / V);   // 2 .. 64
  int l2 = 0;
  while ((1 << l2) < lanes) l2++;
  const int64_t nvec = n_groups * lanes;
  // one vector per lane while that already fills the device, four independent loads per lane beyond (dynamic_float.hip's rule)
  const bool deep = plan_norm(nvec) > ((int64_t)1 << 19);
  const int64_t per_wg = (int64_t)kDynThreads * (deep ? 4 : 1);
  const int64_t grid = (nvec + per_wg - 1) / per_wg;
  if (grid > 0x7FFFFFFF) return DMXQ_ERR_UNSUPPORTED;
  if (deep) DMXQ_LAUNCH((bsf_group_kernel<DT, 4>), dim3((unsigned)grid), dim3(kDynThreads), 0, s, in, out, nvec, lanes, l2, f, tensor_scale,
                        scale_out, scale_q_out);
  else DMXQ_LAUNCH((bsf_group_kernel<DT, 1>), dim3((unsigned)grid), dim3(kDynThreads), 0, s, in, out, nvec, lanes, l2, f, tensor_scale,
                   scale_out, scale_q_out);
  return launch_status();
}

// ---------------------------------------------------------------------------------------------------------------------------
// The dynamic tensor scale: t = (max |x| / fmax) / scale_max over the WHOLE tensor, in three small launches on one float of the caller
// -- the word is zeroed, every workgroup folds its maximum of the magnitude bits into it with one integer atomic (exact in any order; a
// NaN pattern is the largest), and one thread turns the bits into t in place (two IEEE divisions; 1 where not finite or below 2^-126).
constexpr int kBsRedU = 4;          // 16-byte loads in flight per lane
constexpr int kBsRedMaxGrid = 1024;

__global__ void bsf_zero_kernel(uint32_t* word) { *word = 0u; }

template <int DT>
__global__ __launch_bounds__(kDynThreads) void bsf_absmax_kernel(const void* __restrict__ in, int64_t nvec, uint32_t* __restrict__ amax_bits) {
  __shared__ uint32_t s_max[kDynThreads / kWave];
  const int64_t stride = (int64_t)gridDim.x * (kDynThreads * kBsRedU);
  uint32_t m = 0u;
  for (int64_t i0 = (int64_t)blockIdx.x * (kDynThreads * kBsRedU) + threadIdx.x; i0 < nvec; i0 += stride) {
    u32x4 raw[kBsRedU];
#pragma unroll
    for (int u = 0; u < kBsRedU; u++) {
      const int64_t i = i0 + (int64_t)u * kDynThreads;
      raw[u] = load_raw16<false>(in, (i < nvec ? i : nvec - 1) * 16);   // clamped: a repeated vector cannot change a maximum; cached: the cast reads it next
    }
#pragma unroll
    for (int u = 0; u < kBsRedU; u++) m = max(m, absmax_bits<DT>(raw[u]));
  }
  m = group_max_u32(m, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0) s_max[threadIdx.x / kWave] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kDynThreads / kWave; w++) m = max(m, s_max[w]);
    if (m != 0u) atomicMax(amax_bits, m);
  }
}

__global__ void bsf_tensor_scale_kernel(float* word, float fmax, float scale_max) {
  const float t = (u2f(*reinterpret_cast<const uint32_t*>(word)) / fmax) / scale_max;
  *word = (t >= 0x1p-126f && t < INFINITY) ? t : 1.0f;
}

inline int bsf_class(int dtype, int64_t g) {
  if (!valid_dtype(dtype)) return DMXQ_DYN_NONE;
  return dyn_class(g, dtype == DMXQ_F32 ? 4 : 8, false) == DMXQ_DYN_GROUP ? DMXQ_DYN_GROUP : DMXQ_DYN_NONE;
}

}  // namespace
}  // namespace dmxq

using namespace dmxq;

extern "C" int dmxq_block_scaled_float_class(int dtype, int64_t group) { return bsf_class(dtype, group); }

extern "C" int dmxq_block_scaled_float_qdq(const void* in, void* out, int dtype_in, int dtype_out, int64_t n_groups, int64_t group, int man_bits,
                                           int exp_bits, int exp_bias, int flush_subnormal, int rounding, int scale_man_bits,
                                           int scale_exp_bits, int scale_exp_bias, int scale_flush_subnormal, int scale_rounding,
                                           float scale_max, const float* tensor_scale, float* scale_out, float* scale_q_out, void* stream) {
  if (!valid_dtype(dtype_in) || !valid_dtype(dtype_out) || !valid_rounding(rounding) || !valid_rounding(scale_rounding)) return DMXQ_ERR_BAD_ARG;
  if (n_groups < 0 || group < 0) return DMXQ_ERR_BAD_ARG;
  if (exp_bits < 1 || exp_bits >= 8 || man_bits < 0) return DMXQ_ERR_BAD_ARG;   // (8 exponent bits: no finite maximum to scale to)
  if (scale_exp_bits < 1 || scale_exp_bits >= 8 || scale_man_bits < 0) return DMXQ_ERR_BAD_ARG;
  if (n_groups > 0 && group > 0 && (!in || !out)) return DMXQ_ERR_BAD_ARG;
  // what the kernel takes (decided before scale_max is held against sfmax, which needs a format castg_of accepts)
  const bool formats_ok = man_bits <= 22 && scale_man_bits <= 22;
  const dmxq_float_fmt fe{man_bits, exp_bits, exp_bias, flush_subnormal}, fs{scale_man_bits, scale_exp_bits, scale_exp_bias, scale_flush_subnormal};
  BsFmt f{};
  if (formats_ok && (!castg_of(&fe, &f.e) || !castg_of(&fs, &f.sf))) return DMXQ_ERR_UNSUPPORTED;
  if (formats_ok) {
    const float sfmax = f.sf.k.max_val;
    if (!(scale_max > 0.0f && scale_max <= sfmax)) return DMXQ_ERR_BAD_ARG;
  } else if (!(scale_max > 0.0f)) {
    return DMXQ_ERR_BAD_ARG;
  }
  // everything else is the caller's chain (nothing launched)
  if (!formats_ok || dtype_in != dtype_out || rounding != DMXQ_ROUND_NEAREST || scale_rounding != DMXQ_ROUND_NEAREST) return DMXQ_ERR_UNSUPPORTED;
  f.fmax = f.e.k.max_val;
  f.scale_max = scale_max;
  if (bsf_class(dtype_in, group) == DMXQ_DYN_NONE) return group == 0 ? DMXQ_OK : DMXQ_ERR_UNSUPPORTED;
  if (n_groups == 0) return DMXQ_OK;
  if (!aligned16(in) || !aligned16(out)) return DMXQ_ERR_UNSUPPORTED;
  if (n_groups > INT64_MAX / (group * 4)) return DMXQ_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (dtype_in == DMXQ_BF16) return bsf_launch<DMXQ_BF16>(in, out, n_groups, group, f, tensor_scale, scale_out, scale_q_out, s);
  if (dtype_in == DMXQ_F16) return bsf_launch<DMXQ_F16>(in, out, n_groups, group, f, tensor_scale, scale_out, scale_q_out, s);
  return bsf_launch<DMXQ_F32>(in, out, n_groups, group, f, tensor_scale, scale_out, scale_q_out, s);
}

extern "C" int dmxq_block_scaled_tensor_scale(const void* in, int dtype_in, int64_t n, float fmax, float scale_max, float* t_out, void* stream) {
  if (!valid_dtype(dtype_in) || n < 0 || !t_out || (n > 0 && !in)) return DMXQ_ERR_BAD_ARG;
  if (!(fmax > 0.0f && fmax < INFINITY) || !(scale_max > 0.0f && scale_max < INFINITY)) return DMXQ_ERR_BAD_ARG;
  const int V = dtype_in == DMXQ_F32 ? 4 : 8;
  if (n % V != 0 || !aligned16(in)) return DMXQ_ERR_UNSUPPORTED;   // (whole aligned 16-byte vectors only: the caller's existing reduction)
  const int64_t nvec = n / V, per_wg = (int64_t)kDynThreads * kBsRedU;
  const int64_t tiles = (nvec + per_wg - 1) / per_wg;
  const unsigned grid = (unsigned)(tiles < kBsRedMaxGrid ? tiles : kBsRedMaxGrid);
  hipStream_t s = (hipStream_t)stream;
  uint32_t* word = reinterpret_cast<uint32_t*>(t_out);
  DMXQ_LAUNCH(bsf_zero_kernel, dim3(1), dim3(1), 0, s, word);
  if (nvec > 0) {
    if (dtype_in == DMXQ_BF16) DMXQ_LAUNCH((bsf_absmax_kernel<DMXQ_BF16>), dim3(grid), dim3(kDynThreads), 0, s, in, nvec, word);
    else if (dtype_in == DMXQ_F16) DMXQ_LAUNCH((bsf_absmax_kernel<DMXQ_F16>), dim3(grid), dim3(kDynThreads), 0, s, in, nvec, word);
    else DMXQ_LAUNCH((bsf_absmax_kernel<DMXQ_F32>), dim3(grid), dim3(kDynThreads), 0, s, in, nvec, word);
  }
  DMXQ_LAUNCH(bsf_tensor_scale_kernel, dim3(1), dim3(1), 0, s, t_out, fmax, scale_max);
  return launch_status();
}
