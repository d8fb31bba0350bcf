// csrc/int_matmul.hip — the dynamic-scale integer matmul (W8A8 / W4A8) on the int8 matrix cores (DESIGN.md §8 "Integer matmul"):
// y = A W^T on the packed operands dmxq_dynamic_fixed_pack writes (int8 codes + fp32 scales), the integer dot product a W8A8
// deployment forms -- not "dequantise to bf16, then let a BLAS multiply".
//
//   class ROW    (one scale per row on both sides)
//     P[m, n] = sum over ALL of K of ca[m, k] * cw[n, k]        ONE int32, exact: |P| <= 127 * 127 * 131072 < 2^31 (codes of a
//                                                                symmetric format; with -128 codes the guarantee ends at K = 131056)
//     y[m, n] = (float(P) * sa[m]) * sw[n]                      one nearest-even int -> fp32 convert, two fp32 multiplies in that
//                                                                order, one nearest-even convert to the output dtype
//   class GROUP  (weight scales per group of G = 32 / 64 / 128 codes along K; activation scales per row, or per the same G)
//     P_g     = sum over group g of ca * cw                      from a ZERO accumulator; |P_g| <= 128 * 2^14 = 2^21: exact in fp32
//     per-row A:  acc = fma(float(P_g), sw[n, g], acc) in ascending g from +0, y = acc * sa[m]
//     grouped A:  acc = fma(float(P_g) * sa[m, g], sw[n, g], acc) in ascending g from +0, y = acc
// No split-K, no atomics: the same operands give the same bits on every call.
//
// Geometry (csrc/bfp_matmul.hip's, which it shares line by line where the two agree).  A workgroup of 256 lanes owns a 128 x 128
// output tile, its 4 waves 2 x 2 with 64 x 64 each = 4 x 4 MFMA tiles of 16 x 16.  Both operand tiles come in with 16-byte global
// loads (rows past M / N clamped to the last row, nothing stored for them) and go through LDS, double-buffered along K, one barrier
// per step; LDS rows are padded to step + 16 bytes, so the 16 lanes of an MFMA operand (16 rows at one k offset, stride 144 / 80 /
// 48 bytes = 9 / 5 / 3 sixteen-byte bank groups: odd, hence 16 disjoint groups) do not collide.  The MFMA's row operand is W, its
// column operand A: a lane holds D for ONE m (lane % 16) and FOUR consecutive n, so a row scale is one register and the result
// leaves as one 16 (8)-byte store per tile where N % 4 == 0 and the base is aligned (scalar stores otherwise).
//
// ROW.  The 64 int32 accumulators of a lane live across the WHOLE K loop; nothing but MFMA, LDS reads and staging is inside it.
//   * MFMA shape.  v_mfma_i32_16x16x64_i8 (8 passes, 16 x 16 x 64 MACs) against v_mfma_i32_32x32x32_i8 (16 passes, 32 x 32 x 32):
//     per MFMA the 32 x 32 shape reads half the operand bytes per MAC, but the wave's tile is 64 x 64 in registers either way, and
//     per 64 bytes of K a lane then reads (4 + 4) x 16 B with 4 x 4 tiles of 16 x 16 and (2 + 2) x 2 x 16 B with 2 x 2 tiles of
//     32 x 32 x 2 k-halves: 8 ds_read_b128 in both; matrix-core time is 16 x 8 = 8 x 16 = 128 passes in both.  The counts tie; the
//     32 x 32 shape only halves the MFMA ISSUE count (8 against 16), which is not the limit (an issue slot is 4 cycles of the 32 an
//     MFMA occupies the pipe), and would split this file's epilogue in two lane layouts.  16x16x64 it is, shared with GROUP.
//   * K step 128 bytes per buffer (two chained 16x16x64 per tile): a barrier covers 32 MFMA = 1024 matrix-core cycles per wave.
//     2 x 2 x 128 x 144 B = 72 KiB of LDS: two workgroups per CU in gfx950's 160 KiB.
//   * K tail.  K is a multiple of 16, not of 128: a staged 16-byte vector that starts at or past K is not loaded but set to zero
//     (zero codes add nothing to an integer sum).
//   * Scales are read ONCE, in the epilogue, straight from global memory (clamped indices); they never touch LDS.
//   Issue counts of the K loop's block per step, from the ISA (hipcc -S, counted as tools/isa_count.py counts, fp32 kernel): 32 MFMA
//   (32 x 32 = 1024 matrix-core cycles) against 6 VALU operations (24 cycles: address and predicate arithmetic), 16 ds_read_b128,
//   8 ds_write_b128 and 17 SALU; the step's 8 global loads sit behind the K-tail predicate in a block of their own.  No convert,
//   multiply or fma inside the loop: MFMA : VALU issue is 43 : 1 where bfp_matmul's B = 64 loop is 1 : 1.5.
// GROUP.  One K step is one group; G = 128 is two chained MFMA, G = 32 one 16x16x32.  The weight scales travel beside the tile as
// floats in LDS (lane 128 + r loads the scale of W row r for the step's group), grouped activation scales likewise (lane r); a
// per-row activation scale is applied once at the end.  Epilogue per 16 x 16 tile and group: 4 v_cvt_f32_i32 + 4 v_fma_f32 with
// per-row A (against bfp_matmul's 12), + 4 v_mul_f32 with grouped A.  176 - 200 VGPRs (G = 128: 254), two waves per SIMD, 26 / 42 /
// 74 KiB of LDS (G = 32 / 64 / 128).
// Built without the packed fp32 instructions (build.py EXTRA_FLAGS); no scratch (build.py NO_SCRATCH).
#include "common.hpp"

namespace dmxq {

typedef int i32x4 __attribute__((ext_vector_type(4)));
constexpr int kImThreads = 256, kImTile = 128;
constexpr int64_t kImMaxRowK = 131072;   // 127 * 127 * 131072 < 2^31

// G: 0 = class ROW, else the group size; AG: grouped activation scales (G > 0 only)
template <int DTO, int G, bool AG>
__global__ __launch_bounds__(kImThreads, 2) void int_matmul_kernel(const int8_t* __restrict__ ca, const float* __restrict__ sa,
                                                                   const int8_t* __restrict__ cw, const float* __restrict__ sw,
                                                                   void* __restrict__ out, int M, int N, int64_t K, int vec_ok) {
  constexpr bool ROW = G == 0;
  constexpr int KS = ROW ? 128 : G;                      // bytes of a row per K step
  constexpr int MK = KS == 32 ? 32 : 64, CHAIN = KS / MK;   // the MFMA's K; MFMA per tile and step
  constexpr int VPR = KS / 16, LOADS = kImTile * VPR / kImThreads, STRIDE = KS + 16, OPB = kImTile * STRIDE;
  __shared__ __attribute__((aligned(16))) uint8_t lds[2][2 * OPB];            // [buffer][A tile | W tile]
  __shared__ __attribute__((aligned(16))) float lsc[ROW ? 1 : 2][ROW ? 4 : 2 * kImTile];   // GROUP: [buffer][A row scales | W row scales]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave >> 1, wn = wave & 1;
  const int l16 = lane & 15, q = lane >> 4;
  const int m0 = blockIdx.y * kImTile, n0 = blockIdx.x * kImTile;
  const int64_t steps = (K + KS - 1) / KS, ng = ROW ? 1 : K / KS;

  // staging: vector v = t + i * 256 of a tile is (row v / VPR, 16-byte chunk v % VPR); rows past the edge read the last row
  const int8_t* src_a[LOADS];
  const int8_t* src_w[LOADS];
  int dst[LOADS], koff[LOADS];
#pragma unroll
  for (int i = 0; i < LOADS; i++) {
    const int v = t + i * kImThreads, row = v / VPR, chunk = v % VPR;
    const int ra = m0 + row < M ? m0 + row : M - 1, rw = n0 + row < N ? n0 + row : N - 1;
    koff[i] = chunk * 16;
    src_a[i] = ca + (int64_t)ra * K + koff[i];
    src_w[i] = cw + (int64_t)rw * K + koff[i];
    dst[i] = row * STRIDE + koff[i];
  }
  // GROUP: lane t < 128 stages the (grouped) scale of A row t, lane 128 + r that of W row r
  const bool is_w = t >= kImTile;
  const int er = is_w ? (n0 + t - kImTile < N ? n0 + t - kImTile : N - 1) : (m0 + t < M ? m0 + t : M - 1);
  const float* src_s = (is_w ? sw : sa) + (int64_t)er * ng;
  const bool stage_s = !ROW && (is_w || AG);

  u32x4 ga[LOADS], gw[LOADS];
  float gs = 0.0f;
  auto gload = [&](int64_t s) {   // step s: bytes [s * KS, s * KS + KS) of every row (ROW: zero from K on), the scales of group s
#pragma unroll
    for (int i = 0; i < LOADS; i++) {
      if (!ROW || s * KS + koff[i] < K) {
        ga[i] = *(const u32x4*)(src_a[i] + s * KS);
        gw[i] = *(const u32x4*)(src_w[i] + s * KS);
      } else {
        ga[i] = u32x4{0u, 0u, 0u, 0u};
        gw[i] = u32x4{0u, 0u, 0u, 0u};
      }
    }
    if (stage_s) gs = src_s[s];
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < LOADS; i++) {
      *(u32x4*)(lds[buf] + dst[i]) = ga[i];
      *(u32x4*)(lds[buf] + OPB + dst[i]) = gw[i];
    }
    if (stage_s) lsc[ROW ? 0 : buf][t] = gs;
  };

  // a lane's operand of MFMA c of a step: row l16 of a 16-row tile, quarter q of that MFMA's MK bytes (the same quarter of A and W)
  const int off_a = (wm * 64 + l16) * STRIDE + q * (MK / 4);
  const int off_w = OPB + (wn * 64 + l16) * STRIDE + q * (MK / 4);

  i32x4 P[4][4];
  float acc[4][4][4];
#pragma unroll
  for (int mt = 0; mt < 4; mt++)
#pragma unroll
    for (int nt = 0; nt < 4; nt++) {
      P[mt][nt] = i32x4{0, 0, 0, 0};
#pragma unroll
      for (int i = 0; i < 4; i++) acc[mt][nt][i] = 0.0f;
    }

  gload(0);
  lstore(0);
  __syncthreads();
  for (int64_t s = 0; s < steps; s++) {
    const int buf = (int)(s & 1);
    if (s + 1 < steps) gload(s + 1);
#pragma unroll
    for (int c = 0; c < CHAIN; c++) {
      if constexpr (MK == 64) {
        i32x4 fa[4], fw[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
          fa[k] = *(const i32x4*)(lds[buf] + off_a + c * MK + k * 16 * STRIDE);
          fw[k] = *(const i32x4*)(lds[buf] + off_w + c * MK + k * 16 * STRIDE);
        }
#pragma unroll
        for (int mt = 0; mt < 4; mt++)
#pragma unroll
          for (int nt = 0; nt < 4; nt++)   // D[n][m]: rows from W, columns from A; GROUP starts every group from the constant 0
            P[mt][nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fw[nt], fa[mt], (!ROW && c == 0) ? i32x4{0, 0, 0, 0} : P[mt][nt], 0, 0, 0);
      } else {
        long fa[4], fw[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
          fa[k] = *(const long*)(lds[buf] + off_a + k * 16 * STRIDE);
          fw[k] = *(const long*)(lds[buf] + off_w + k * 16 * STRIDE);
        }
#pragma unroll
        for (int mt = 0; mt < 4; mt++)
#pragma unroll
          for (int nt = 0; nt < 4; nt++)
            P[mt][nt] = __builtin_amdgcn_mfma_i32_16x16x32_i8(fw[nt], fa[mt], i32x4{0, 0, 0, 0}, 0, 0, 0);
      }
    }
    if constexpr (!ROW) {
      float ra[4];
      f32x4 rw[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        if constexpr (AG) ra[k] = lsc[buf][wm * 64 + k * 16 + l16];
        rw[k] = *(const f32x4*)(&lsc[buf][kImTile + wn * 64 + k * 16 + 4 * q]);
      }
#pragma unroll
      for (int mt = 0; mt < 4; mt++)
#pragma unroll
        for (int nt = 0; nt < 4; nt++)
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const float p = AG ? (float)P[mt][nt][i] * ra[mt] : (float)P[mt][nt][i];
            acc[mt][nt][i] = __builtin_fmaf(p, rw[nt][i], acc[mt][nt][i]);
          }
    }
    if (s + 1 < steps) lstore(buf ^ 1);   // (its last readers passed the barrier that ended step s - 1)
    __syncthreads();
  }

  // lane: row m = .. + l16, columns n .. n + 3 with n = .. + 4 * q; the per-row scales straight from global memory
#pragma unroll
  for (int mt = 0; mt < 4; mt++) {
    const int m = m0 + wm * 64 + mt * 16 + l16;
    if (m >= M) continue;
    const float row_a = AG ? 1.0f : sa[m];
#pragma unroll
    for (int nt = 0; nt < 4; nt++) {
      const int n = n0 + wn * 64 + nt * 16 + 4 * q;
      float y[4];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        if constexpr (ROW) y[i] = ((float)P[mt][nt][i] * row_a) * sw[n + i < N ? n + i : N - 1];
        else y[i] = AG ? acc[mt][nt][i] : acc[mt][nt][i] * row_a;
      }
      const int64_t e0 = (int64_t)m * N + n;
      if (vec_ok) {   // N % 4 == 0 and an aligned base: the four columns are inside or outside together
        if (n < N) store_vec<DTO, 4, false>(out, e0, y);
      } else {
#pragma unroll
        for (int i = 0; i < 4; i++)
          if (n + i < N) store1<DTO>(out, e0 + i, y[i]);
      }
    }
  }
}

}  // namespace dmxq

using namespace dmxq;

extern "C" int dmxq_int_matmul_class(int64_t M, int64_t N, int64_t K, int64_t group_a, int64_t group_w) {
  if (M < 1 || N < 1 || K < 1) return DMXQ_INTMM_NONE;
  if (M > (int64_t)65535 * kImTile || N > 0x7FFFFF00) return DMXQ_INTMM_NONE;   // grid.y; 32-bit row / column indices
  if (group_w == 0) return (group_a == 0 && K >= 16 && K <= kImMaxRowK && K % 16 == 0) ? DMXQ_INTMM_ROW : DMXQ_INTMM_NONE;
  if (group_w != 32 && group_w != 64 && group_w != 128) return DMXQ_INTMM_NONE;
  if (K % group_w != 0 || (group_a != 0 && group_a != group_w)) return DMXQ_INTMM_NONE;
  return DMXQ_INTMM_GROUP;
}

extern "C" int dmxq_int_matmul(const int8_t* codes_a, const float* scale_a, const int8_t* codes_w, const float* scale_w, void* out,
                               int dtype_out, int64_t M, int64_t N, int64_t K, int64_t group_a, int64_t group_w, void* stream) {
  if (!valid_dtype(dtype_out) || M < 0 || N < 0 || K < 0 || group_a < 0 || group_w < 0) return DMXQ_ERR_BAD_ARG;
  if (M * N == 0) return DMXQ_OK;
  if (!codes_a || !scale_a || !codes_w || !scale_w || !out) return DMXQ_ERR_BAD_ARG;
  const int cls = dmxq_int_matmul_class(M, N, K, group_a, group_w);
  if (cls == DMXQ_INTMM_NONE || !aligned16(codes_a) || !aligned16(codes_w)) return DMXQ_ERR_UNSUPPORTED;   // (K % 16 == 0: every row aligned)
  if ((reinterpret_cast<uintptr_t>(scale_a) | reinterpret_cast<uintptr_t>(scale_w)) & 3u) return DMXQ_ERR_UNSUPPORTED;
  const int ob = dtype_out == DMXQ_F32 ? 4 : 2;
  const int vec_ok = N % 4 == 0 && (reinterpret_cast<uintptr_t>(out) % (4 * ob)) == 0;
  const dim3 grid((unsigned)((N + kImTile - 1) / kImTile), (unsigned)((M + kImTile - 1) / kImTile));
  hipStream_t s = (hipStream_t)stream;
#define DMXQ_IM(DT_, G_, AG_) DMXQ_LAUNCH((int_matmul_kernel<DT_, G_, AG_>), grid, dim3(kImThreads), 0, s, codes_a, scale_a, codes_w, scale_w, out, (int)M, (int)N, K, vec_ok)
#define DMXQ_IMA(DT_, G_) do { if (group_a) DMXQ_IM(DT_, G_, true); else DMXQ_IM(DT_, G_, false); } while (0)
#define DMXQ_IMG(DT_) do { if (group_w == 0) DMXQ_IM(DT_, 0, false); else if (group_w == 32) DMXQ_IMA(DT_, 32); else if (group_w == 64) DMXQ_IMA(DT_, 64); else DMXQ_IMA(DT_, 128); } while (0)
  if (dtype_out == DMXQ_F32) DMXQ_IMG(DMXQ_F32);
  else if (dtype_out == DMXQ_F16) DMXQ_IMG(DMXQ_F16);
  else DMXQ_IMG(DMXQ_BF16);
#undef DMXQ_IM
#undef DMXQ_IMA
#undef DMXQ_IMG
  return launch_status();
}
