// csrc/bfp_matmul.hip — the block-floating-point matmul on the int8 matrix cores (DESIGN.md §8 "BFP matmul"): the product an
// accelerator with a BFP datapath computes, on the packed operands dmxq_bfp_pack writes -- not "dequantise, then let a BLAS multiply".
//
//   y[m, n] = ((t_0 + t_1) + t_2) + ...   in fp32, ascending block order, one nearest-even convert to the output dtype
//   t_j     = (float(P_j) * 2^(ea[m, j] - 127 - (pa - 2))) * 2^(ew[n, j] - 127 - (pw - 2))
//   P_j     = sum over block j of ca[m, k] * cw[n, k]        an exact integer, |P_j| <= B * 2^7 * 2^7 = 2^21 for B <= 128
// Exponent byte 0 (pack's zero / denormal block): scale 0, the block adds +-0 and leaves the sum as it is; 255: scale NaN, y[m, n] NaN.
//
// Geometry.  A workgroup of 256 lanes owns a 128 x 128 output tile; its 4 waves sit 2 x 2 and own 64 x 64 each = 4 x 4 MFMA tiles of
// 16 x 16, whose 64 fp32 accumulators per lane stay in registers for the whole K loop (no split-K: the K loop IS the pinned order).
// One K step is one block of B codes (B = 128: half a block, the second MFMA chained on the first one's integer accumulator):
//   B = 32   one v_mfma_i32_16x16x32_i8 per tile and block (8-byte operands)
//   B = 64   one v_mfma_i32_16x16x64_i8                    (16-byte operands)
//   B = 128  two v_mfma_i32_16x16x64_i8, C of the second = D of the first
// every block starting from a ZERO integer accumulator (the inline constant 0 as the MFMA's C operand), so P_j is per block.
// Both operand tiles (128 rows x step bytes each) come in with 16-byte global loads, rows past M / N clamped to the last row (loads
// stay in bounds, nothing is stored for them), and go through LDS, double-buffered along K: the loads of step s + 1 are in flight
// while step s computes, one barrier per step.  LDS rows are padded to step + 16 bytes: the 16 lanes of one MFMA operand read
// 16 rows at one k offset, and at a stride of 80 (48) bytes those 16 (8)-byte reads fall into 16 disjoint bank groups.  The tile's
// 128 + 128 exponent bytes of a block travel with it: lane t loads ONE byte, turns it into the fp32 power of two ONCE
// (u2f(e << 23) * 2^-(p-2): exact, denormal results kept; 255 -> NaN) and stores the float beside the tile.
// The MFMA's "row" operand is the W tile and its "column" operand the A tile: a lane then holds D for ONE m (lane % 16) and FOUR
// consecutive n (4 * (lane / 16) + i), so the A scale is one register per tile row, the W scales one 16-byte LDS read per tile
// column, and the result leaves as one 16 (8)-byte store per tile.  The k order inside a block differs between the lanes' operand
// quarters but is the SAME for A and W, and integer sums do not care.
// Epilogue per 16 x 16 tile and block (the hot VALU part): 4 v_cvt_f32_i32, 4 v_mul_f32 by the row's scale (always exact: P * 2^e,
// e >= -132, is a multiple of 2^-149 -- or overflows to Inf), 4 v_fma_f32 with the column's scale into the accumulator.  Outside
// under/overflow the second product is exact too, so the fma has the bits of multiply-then-add.
// Issue cost from the ISA (tools/isa_count.py on the B = 64 fp32 kernel's K loop): 16 MFMA (8 passes = 32 cycles each on the matrix
// core) against 192 VALU operations of 4 cycles for the 16 tiles: 48 VALU cycles per 32 MFMA cycles, 1.5 : 1 at B = 64 (B = 128:
// 0.75 : 1, B = 32: 3 : 1) -- B = 64 and B = 32 are bound by the epilogue, which two workgroups per CU overlap with the other's MFMA.
// Built without the packed fp32 instructions (build.py EXTRA_FLAGS); no scratch (build.py NO_SCRATCH).
#include "common.hpp"

namespace dmxq {

typedef int i32x4 __attribute__((ext_vector_type(4)));
constexpr int kMmThreads = 256, kMmTile = 128;

template <int KS> struct MmFrag;
template <> struct MmFrag<64> {
  typedef i32x4 T;
  static __device__ __forceinline__ i32x4 mfma(T a, T b, i32x4 c) { return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0); }
};
template <> struct MmFrag<32> {
  typedef long T;
  static __device__ __forceinline__ i32x4 mfma(T a, T b, i32x4 c) { return __builtin_amdgcn_mfma_i32_16x16x32_i8(a, b, c, 0, 0, 0); }
};

template <int DTO, int B>
__global__ __launch_bounds__(kMmThreads, 2) void bfp_matmul_kernel(const int8_t* __restrict__ ca, const uint8_t* __restrict__ ea,
                                                                   const int8_t* __restrict__ cw, const uint8_t* __restrict__ ew,
                                                                   void* __restrict__ out, int M, int N, int64_t K, int64_t nb,
                                                                   float down_a, float down_w, int vec_ok) {
  constexpr int KS = B == 128 ? 64 : B, HALVES = B / KS;       // bytes of a row per K step; steps per block
  constexpr int VPR = KS / 16, LOADS = kMmTile * VPR / kMmThreads, STRIDE = KS + 16, OPB = kMmTile * STRIDE;
  typedef typename MmFrag<KS>::T Frag;
  __shared__ __attribute__((aligned(16))) uint8_t lds[2][2 * OPB];       // [buffer][A tile | W tile]
  __shared__ __attribute__((aligned(16))) float lsc[2][2 * kMmTile];     // [buffer][A row scales | W row scales]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave >> 1, wn = wave & 1;
  const int l16 = lane & 15, q = lane >> 4;
  const int m0 = blockIdx.y * kMmTile, n0 = blockIdx.x * kMmTile;

  // staging: vector v = t + i * 256 of a tile is (row v / VPR, 16-byte chunk v % VPR); rows past the edge read the last row
  const int8_t* src_a[LOADS];
  const int8_t* src_w[LOADS];
  int dst[LOADS];
#pragma unroll
  for (int i = 0; i < LOADS; i++) {
    const int v = t + i * kMmThreads, row = v / VPR, chunk = v % VPR;
    const int ra = m0 + row < M ? m0 + row : M - 1, rw = n0 + row < N ? n0 + row : N - 1;
    src_a[i] = ca + (int64_t)ra * K + chunk * 16;
    src_w[i] = cw + (int64_t)rw * K + chunk * 16;
    dst[i] = row * STRIDE + chunk * 16;
  }
  const bool is_w = t >= kMmTile;
  const int er = is_w ? (n0 + t - kMmTile < N ? n0 + t - kMmTile : N - 1) : (m0 + t < M ? m0 + t : M - 1);
  const uint8_t* src_e = (is_w ? ew : ea) + (int64_t)er * nb;
  const float down = is_w ? down_w : down_a;

  u32x4 ga[LOADS], gw[LOADS];
  uint32_t ge;
  auto gload = [&](int64_t s) {   // step s: bytes [s * KS, s * KS + KS) of every row, the exponents of block s / HALVES
#pragma unroll
    for (int i = 0; i < LOADS; i++) {
      ga[i] = *(const u32x4*)(src_a[i] + s * KS);
      gw[i] = *(const u32x4*)(src_w[i] + s * KS);
    }
    ge = src_e[s / HALVES];
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < LOADS; i++) {
      *(u32x4*)(lds[buf] + dst[i]) = ga[i];
      *(u32x4*)(lds[buf] + OPB + dst[i]) = gw[i];
    }
    lsc[buf][t] = ge == 255u ? u2f(0x7FC00000u) : u2f(ge << 23) * down;   // 2^(e - 127 - (p - 2)); e = 0: 0
  };

  // a lane's operand: row l16 of a 16-row tile, quarter q of the step's bytes (the same quarter of A and of W)
  const int off_a = (wm * 64 + l16) * STRIDE + q * (KS / 4);
  const int off_w = OPB + (wn * 64 + l16) * STRIDE + q * (KS / 4);

  float acc[4][4][4];
#pragma unroll
  for (int mt = 0; mt < 4; mt++)
#pragma unroll
    for (int nt = 0; nt < 4; nt++)
#pragma unroll
      for (int i = 0; i < 4; i++) acc[mt][nt][i] = 0.0f;

  gload(0);
  lstore(0);
  __syncthreads();
  const int64_t steps = nb * HALVES;
  i32x4 P[4][4];
  for (int64_t j = 0; j < nb; j++) {
#pragma unroll
    for (int h = 0; h < HALVES; h++) {
      const int64_t s = j * HALVES + h;
      const int buf = (int)(s & 1);
      if (s + 1 < steps) gload(s + 1);
      Frag fa[4], fw[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        fa[k] = *(const Frag*)(lds[buf] + off_a + k * 16 * STRIDE);
        fw[k] = *(const Frag*)(lds[buf] + off_w + k * 16 * STRIDE);
      }
#pragma unroll
      for (int mt = 0; mt < 4; mt++)
#pragma unroll
        for (int nt = 0; nt < 4; nt++)
          P[mt][nt] = MmFrag<KS>::mfma(fw[nt], fa[mt], h == 0 ? i32x4{0, 0, 0, 0} : P[mt][nt]);   // D[n][m]: rows from W, columns from A
      if (h == HALVES - 1) {
        float sa[4];
        f32x4 sw[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
          sa[k] = lsc[buf][wm * 64 + k * 16 + l16];
          sw[k] = *(const f32x4*)(&lsc[buf][kMmTile + wn * 64 + k * 16 + 4 * q]);
        }
#pragma unroll
        for (int mt = 0; mt < 4; mt++)
#pragma unroll
          for (int nt = 0; nt < 4; nt++)
#pragma unroll
            for (int i = 0; i < 4; i++)
              acc[mt][nt][i] = __builtin_fmaf((float)P[mt][nt][i] * sa[mt], sw[nt][i], acc[mt][nt][i]);
      }
      if (s + 1 < steps) lstore(buf ^ 1);   // (its last readers passed the barrier that ended step s - 1)
      __syncthreads();
    }
  }

  // lane: row m = .. + l16, columns n .. n + 3 with n = .. + 4 * q
#pragma unroll
  for (int mt = 0; mt < 4; mt++) {
    const int m = m0 + wm * 64 + mt * 16 + l16;
    if (m >= M) continue;
#pragma unroll
    for (int nt = 0; nt < 4; nt++) {
      const int n = n0 + wn * 64 + nt * 16 + 4 * q;
      const int64_t e0 = (int64_t)m * N + n;
      if (vec_ok) {   // N % 4 == 0 and an aligned base: the four columns are inside or outside together
        if (n < N) store_vec<DTO, 4, false>(out, e0, acc[mt][nt]);
      } else {
#pragma unroll
        for (int i = 0; i < 4; i++)
          if (n + i < N) store1<DTO>(out, e0 + i, acc[mt][nt][i]);
      }
    }
  }
}

}  // namespace dmxq

using namespace dmxq;

extern "C" int dmxq_bfp_matmul_class(int64_t M, int64_t N, int64_t K, int64_t block_size) {
  if (M < 1 || N < 1 || K < 1) return DMXQ_BFPMM_NONE;
  if (block_size != 32 && block_size != 64 && block_size != 128) return DMXQ_BFPMM_NONE;
  if (K % block_size != 0) return DMXQ_BFPMM_NONE;
  if (M > (int64_t)65535 * kMmTile || N > 0x7FFFFF00) return DMXQ_BFPMM_NONE;   // grid.y; 32-bit row / column indices
  return block_size == 32 ? DMXQ_BFPMM_B32 : (block_size == 64 ? DMXQ_BFPMM_B64 : DMXQ_BFPMM_B128);
}

extern "C" int dmxq_bfp_matmul(const int8_t* mant_a, const uint8_t* exps_a, const int8_t* mant_w, const uint8_t* exps_w, void* out,
                               int dtype_out, int64_t M, int64_t N, int64_t K, int64_t block_size, int prec_a, int prec_w, void* stream) {
  if (!valid_dtype(dtype_out) || M < 0 || N < 0 || K < 0 || block_size < 1) return DMXQ_ERR_BAD_ARG;
  if (prec_a < 2 || prec_a > 8 || prec_w < 2 || prec_w > 8) return DMXQ_ERR_UNSUPPORTED;
  if (M * N == 0) return DMXQ_OK;
  if (!mant_a || !exps_a || !mant_w || !exps_w || !out) return DMXQ_ERR_BAD_ARG;
  const int cls = dmxq_bfp_matmul_class(M, N, K, block_size);
  if (cls == DMXQ_BFPMM_NONE || !aligned16(mant_a) || !aligned16(mant_w)) return DMXQ_ERR_UNSUPPORTED;   // (K % 32 == 0: every row 16-byte aligned)
  const int ob = dtype_out == DMXQ_F32 ? 4 : 2;
  const int vec_ok = N % 4 == 0 && (reinterpret_cast<uintptr_t>(out) % (4 * ob)) == 0;
  const float down_a = 1.0f / (float)(1 << (prec_a - 2)), down_w = 1.0f / (float)(1 << (prec_w - 2));   // 2^-(p - 2), exact
  const dim3 grid((unsigned)((N + kMmTile - 1) / kMmTile), (unsigned)((M + kMmTile - 1) / kMmTile));
  hipStream_t s = (hipStream_t)stream;
#define DMXQ_MM(DT_, B_) DMXQ_LAUNCH((bfp_matmul_kernel<DT_, B_>), grid, dim3(kMmThreads), 0, s, mant_a, exps_a, mant_w, exps_w, out, (int)M, (int)N, K, K / block_size, down_a, down_w, vec_ok)
#define DMXQ_MMB(DT_) do { if (cls == DMXQ_BFPMM_B32) DMXQ_MM(DT_, 32); else if (cls == DMXQ_BFPMM_B64) DMXQ_MM(DT_, 64); else DMXQ_MM(DT_, 128); } while (0)
  if (dtype_out == DMXQ_F32) DMXQ_MMB(DMXQ_F32);
  else if (dtype_out == DMXQ_F16) DMXQ_MMB(DMXQ_F16);
  else DMXQ_MMB(DMXQ_BF16);
#undef DMXQ_MM
#undef DMXQ_MMB
  return launch_status();
}
