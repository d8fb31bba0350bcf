// csrc/hadamard.hip — orthonormal block-Hadamard rotation fused into a quantize-dequantize cast (include/dmxq.h dmxq_hadamard_qdq;
// DESIGN.md §8).  Not in the reference: the rotate -> quantize -> rotate back recipe of QuaRot / SpinQuant and of the MXFP4 training
// recipes, as ONE read and ONE write per element instead of a dense [H, H] matmul and two more passes around the cast.
//
// Arithmetic (the contract; tests/_hadamard_ref.py restates it in torch on the CPU), for a block of H = 2^k consecutive elements
// along the rows, widened to fp32 (exact):
//   for s = 1, 2, 4, .., H/2, in that order: for every i with bit s clear   v[i], v[i+s] = v[i] + v[i+s], v[i] - v[i+s]
//   (old values on the right; every add and subtract ONE fp32 operation, lower index minus upper index), then ONE fp32 multiply by
//   c = (float)(1 / sqrt((double)H)).  R_H is symmetric and orthonormal: the inverse rotation is R_H itself, scale included.
//   y = round_to(dtype_out, R_H(Q(R_H(x))))   with `inverse`,   round_to(dtype_out, Q(R_H(x)))   without,   round_to(dtype_out, R_H(x))
//   without a format; Q = the library's cast of the rotated fp32 tensor, fp32 in and out; one rounding to dtype_out at the very end.
//   NaN / Inf simply propagate through the adds.  No FMA anywhere (-ffp-contract=off).
//
// Geometry: the tensor is flat -- L % H == 0, so the blocks of the flat index ARE the row blocks.  A lane holds one 16-byte vector of
// the input (V = 8 sixteen-bit or 4 fp32 elements), a block is H / V neighbouring lanes of ONE wave (<= 64: a 256-wide fp32 block is a
// whole wave; a wave's 64 vectors are a whole number of blocks for every H).  The stages with s < V run in registers, the others
// across lanes with __shfl_xor: the lane whose bit is clear computes own + partner, the lane whose bit is set partner - own.  The
// number of cross-lane stages is a run-time loop (one kernel per dtype pair, whatever H and the format are).  One vector per lane, one
// tile per workgroup: the grid does not loop.  Lanes past the end re-read the last vector, meet only each other in the shuffles (the
// tensor ends on a block boundary) and store nothing.  Every block is fully read before any of it is written (the stores depend on
// the shuffles, which depend on every load of the block): in == out is fine when both dtypes have one width.
// A pointer that is not 16-byte aligned takes the same kernel with element-wise loads and stores (a wave-uniform flag).
//
// Casts: the literal per-element leaves of bfp_math.hpp / floatq.hpp / fixedq.hpp (nearest rounding) and the general path of the MXFP
// block (mxfp_math.hpp: blockfmt.hip's fast paths are bit-identical to it by construction), with float32 input rules (the rotated
// tensor is float32: the floor(log2 max) rule near powers of two applies).  Block maxima are taken on the bit patterns of |x| over the
// cast's own block: inside the lane's vector when the block is smaller than a vector (one pass of the cast body per sub-block, selected
// element by element: a rare shape, kept simple), with DPP / shuffles across block_size / V lanes otherwise.
#include <math.h>

#include "bfp_math.hpp"
#include "format_desc.hpp"

namespace dmxq {
namespace {

constexpr int kHadThreads = 256;
constexpr int kHadRotateOnly = -1;   // HadCast::kind without a format

struct HadCast {
  int kind;      // dmxq_gptq_kind, or kHadRotateOnly
  int inverse;   // rotate back after the cast
  int blog;      // BFP / MXFP: log2(block_size)
  int per_row;   // FIXED: scale / zero point indexed by row
  FormatDesc d;  // the format as the leaves take it (format_desc.hpp)
};

// R_H of the block this lane's vector belongs to: `lanes` = H / V lanes per block (a power of two, wave-uniform)
template <int V>
__device__ __forceinline__ void had_rotate(float (&v)[V], int lanes, int lane, float c) {
#pragma unroll
  for (int s = 1; s < V; s <<= 1) {
#pragma unroll
    for (int i = 0; i < V; i++) {
      if (!(i & s)) {
        const float a = v[i], b = v[i + s];
        v[i] = a + b;
        v[i + s] = a - b;
      }
    }
  }
  for (int m = 1; m < lanes; m <<= 1) {   // (every lane of the wave takes part: `lanes` is uniform)
    const bool upper = (lane & m) != 0;
#pragma unroll
    for (int i = 0; i < V; i++) {
      const float p = __shfl_xor(v[i], m);
      v[i] = upper ? p - v[i] : v[i] + p;
    }
  }
#pragma unroll
  for (int i = 0; i < V; i++) v[i] = v[i] * c;
}

// q = Q(x) for this lane's V elements of the rotated tensor.  Called by whole waves (the block maxima cross lanes).
template <int V>
__device__ __forceinline__ void had_cast(const float (&x)[V], float (&q)[V], const HadCast& c, float sc, float z) {
  if (c.kind == DMXQ_GPTQ_FLOAT) {
#pragma unroll
    for (int j = 0; j < V; j++) q[j] = float_q1<DMXQ_ROUND_NEAREST>(x[j], c.d.f, 0u);
  } else if (c.kind == DMXQ_GPTQ_FIXED) {
#pragma unroll
    for (int j = 0; j < V; j++) q[j] = fixed_affine_q1(x[j], sc, z, c.d.x);
  } else {
    // a block of >= V elements: ONE pass, the maximum over block_size / V lanes; a block smaller than the vector: one pass per sub-block,
    // each keeping its own elements
    const int B = 1 << c.blog;
    const int passes = B >= V ? 1 : V >> c.blog;
#pragma unroll
    for (int j = 0; j < V; j++) q[j] = 0.0f;
#pragma unroll 1
    for (int g = 0; g < passes; g++) {
      uint32_t bm = 0u;
#pragma unroll
      for (int j = 0; j < V; j++)
        if (passes == 1 || (j >> c.blog) == g) bm = umax(bm, f2u(x[j]) & 0x7FFFFFFFu);
      if (B > V) bm = group_max_u32(bm, B / V);   // (wave-uniform: blocks are aligned groups of B / V lanes)
      if (c.kind == DMXQ_GPTQ_BFP) {
        const BfpBlockParams p = bfp_block_params<true, false>(bm, c.d.wl);
#pragma unroll
        for (int j = 0; j < V; j++) {
          const float v = bfp_q1_nearest_rt(x[j], p, c.d.wl, c.d.asym != 0);
          q[j] = (passes == 1 || (j >> c.blog) == g) ? v : q[j];
        }
      } else {
        const float bs = mxfp_block_scale(bm, c.d.k.big_log2, c.d.k.big, 0);
        const bool zero = u2f(bm) == 0.0f;
#pragma unroll
        for (int j = 0; j < V; j++) {
          const float v = mxfp_q1(x[j], bs, zero, c.d.man, c.d.exp_bits, c.d.k.bias);
          q[j] = (passes == 1 || (j >> c.blog) == g) ? v : q[j];
        }
      }
    }
  }
}

// nvec vectors of V elements; thread t of the grid takes vector t.  vec: both pointers 16-byte aligned.
template <int DTI, int DTO>
__global__ __launch_bounds__(kHadThreads) void hadamard_qdq_kernel(const void* in, void* out, int64_t nvec, int64_t L, int lanes, int vec,
                                                                  float c, const float* __restrict__ scale,
                                                                  const int64_t* __restrict__ zp, const HadCast cst) {
  constexpr int V = 16 / Elem<DTI>::bytes;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t t = (int64_t)blockIdx.x * kHadThreads + threadIdx.x;
  const bool act = t < nvec;
  const int64_t e0 = (act ? t : nvec - 1) * V;   // (a lane past the end re-reads the last vector and stores nothing)
  float x[V];
  if (vec) {
    load_vec<DTI, V>(in, e0, x);
  } else {
#pragma unroll
    for (int j = 0; j < V; j++) x[j] = load1<DTI>(in, e0 + j);
  }
  had_rotate<V>(x, lanes, lane, c);
  if (cst.kind != kHadRotateOnly) {
    float sc = 1.0f, z = 0.0f;
    if (cst.kind == DMXQ_GPTQ_FIXED) {
      const int64_t g = cst.per_row ? e0 / L : 0;
      sc = scale[g];
      z = (float)zp[g];
    }
    float q[V];
    had_cast<V>(x, q, cst, sc, z);
#pragma unroll
    for (int j = 0; j < V; j++) x[j] = q[j];
    if (cst.inverse) had_rotate<V>(x, lanes, lane, c);
  }
  if (act) {
    if (vec) {
      store_vec<DTO, V>(out, e0, x);
    } else {
#pragma unroll
      for (int j = 0; j < V; j++) store1<DTO>(out, e0 + j, x[j]);
    }
  }
}

inline bool pow2(int64_t v) { return v >= 1 && (v & (v - 1)) == 0; }
inline int log2i(int64_t v) { int l = 0; while (((int64_t)1 << l) < v) l++; return l; }

}  // namespace
}  // namespace dmxq

using namespace dmxq;

extern "C" int dmxq_hadamard_qdq(const void* in, void* out, int dtype_in, int dtype_out, int64_t rows, int64_t L, int64_t size,
                                 int inverse, const dmxq_gptq_format* fmt, const float* scale, const int64_t* zero_point, void* stream) {
  if (!valid_dtype(dtype_in) || !valid_dtype(dtype_out) || rows < 0 || L < 0 || size < 0) return DMXQ_ERR_BAD_ARG;
  if (fmt && fmt->kind != DMXQ_GPTQ_BFP && fmt->kind != DMXQ_GPTQ_FLOAT && fmt->kind != DMXQ_GPTQ_FIXED && fmt->kind != DMXQ_GPTQ_MXFP)
    return DMXQ_ERR_BAD_ARG;
  if (!fmt && inverse) return DMXQ_ERR_BAD_ARG;
  if (!(size == 8 || size == 16 || size == 32 || size == 64 || size == 128 || size == 256) || L % size != 0) return DMXQ_ERR_UNSUPPORTED;
  HadCast c{};
  c.kind = kHadRotateOnly;
  c.inverse = inverse ? 1 : 0;
  if (fmt) {
    if (format_desc(*fmt, &c.d) != DMXQ_OK) return DMXQ_ERR_UNSUPPORTED;
    c.kind = fmt->kind;
    if (fmt->kind == DMXQ_GPTQ_BFP || fmt->kind == DMXQ_GPTQ_MXFP) {   // blocks: a power of two dividing the rotation's (BFP: >= 2)
      const int B = fmt->block_size;
      if (B < (fmt->kind == DMXQ_GPTQ_BFP ? 2 : 1) || !pow2(B) || size % B != 0) return DMXQ_ERR_UNSUPPORTED;
      c.blog = log2i(B);
    }
    c.per_row = fmt->kind == DMXQ_GPTQ_FIXED && fmt->per_row ? 1 : 0;
  }
  if (rows == 0 || L == 0) return DMXQ_OK;
  if (!in || !out) return DMXQ_ERR_BAD_ARG;
  if (fmt && fmt->kind == DMXQ_GPTQ_FIXED && (!scale || !zero_point)) return DMXQ_ERR_BAD_ARG;
  const int bi = dtype_in == DMXQ_F32 ? 4 : 2, bo = dtype_out == DMXQ_F32 ? 4 : 2;
  if (in == (const void*)out && bi != bo) return DMXQ_ERR_BAD_ARG;   // in place: equal widths only
  if (rows > INT64_MAX / L) return DMXQ_ERR_BAD_ARG;
  const int V = 16 / bi;
  const int64_t nvec = rows * L / V;   // (size >= 8 >= V divides L)
  const int64_t grid = (nvec + kHadThreads - 1) / kHadThreads;
  if (grid > 0x7FFFFFFF) return DMXQ_ERR_BAD_ARG;
  const int lanes = (int)(size / V);   // 1 .. 64
  const int vec = aligned16(in) && aligned16(out) ? 1 : 0;
  const float cs = (float)(1.0 / sqrt((double)size));
  hipStream_t s = (hipStream_t)stream;
#define DMXQ_HAD(I_, O_) \
  if (dtype_in == I_ && dtype_out == O_) \
    DMXQ_LAUNCH((hadamard_qdq_kernel<I_, O_>), dim3((unsigned)grid), dim3(kHadThreads), 0, s, in, out, nvec, L, lanes, vec, cs, scale, zero_point, c);
  DMXQ_HAD(DMXQ_BF16, DMXQ_BF16)
  DMXQ_HAD(DMXQ_F16, DMXQ_F16)
  DMXQ_HAD(DMXQ_F32, DMXQ_F32)
  DMXQ_HAD(DMXQ_BF16, DMXQ_F32)
  DMXQ_HAD(DMXQ_F16, DMXQ_F32)
  DMXQ_HAD(DMXQ_F32, DMXQ_BF16)
  DMXQ_HAD(DMXQ_F32, DMXQ_F16)
  DMXQ_HAD(DMXQ_BF16, DMXQ_F16)
  DMXQ_HAD(DMXQ_F16, DMXQ_BF16)
#undef DMXQ_HAD
  return launch_status();
}
