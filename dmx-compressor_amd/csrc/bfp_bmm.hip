// csrc/bfp_bmm.hip — the BATCHED block-floating-point matmul, second operand in either layout (DESIGN.md §8 "Batched BFP matmul"): the two
// products of an attention layer on the packed operands of dmxq_bfp_pack / dmxq_bfp_pack_cols.  Per batch element exactly the definition
// of csrc/bfp_matmul.hip (exact integer P_j per block, two power-of-two multiplies, fp32 adds in ascending block order from +0, one
// nearest-even convert; exponent byte 0 adds +-0, 255 makes the element NaN):
//   A codes [batch, M, K] + exps [batch, M, K / B]
//   "nk": W codes [batch, N, K] + exps [batch, N, K / B]     Q K^T: the multiplier is a transposed view of K[.., S, D]
//   "kn": W codes [batch, K, N] + exps [batch, K / B, N]     P V:   the multiplier V[.., S, D] is blocked along its NON-contiguous S
//   out [batch, M, N]
//
// Geometry.  grid = (N tiles, M tiles, batch); every batch offset is 64-bit.  A workgroup of 256 lanes owns 128 rows of A and
//   TN = 128 columns: waves 2 x 2, 64 x 64 each = 4 x 4 MFMA tiles of 16 x 16 (the 2-D kernel's geometry), or
//   TN = 64  columns (picked for N <= 64: head_dim 64 in P V): waves 4 x 1, 32 x 64 each = 2 x 4 tiles -- no MFMA work on columns that
//            do not exist, half the accumulators, the same 128 rows of A per workgroup.
// One K step is KS = min(B, 64) codes; B = 32: one v_mfma_i32_16x16x32_i8 per tile and block, B = 64: one 16x16x64, B = 128: two chained,
// each block from a zero integer accumulator.  The MFMA's row operand is the W tile and its column operand the A tile: a lane holds D
// for one m (lane % 16) and four consecutive n (4 * (lane / 16) + i); the epilogue per block is 4 cvt, 4 mul by the row's scale, 4 fma
// with the column's scale, as in the 2-D kernel.  No split-K; accumulators (64 or 32 per lane) stay in registers; no scratch.
//
// Staging.  Both tiles go through LDS as [row][k] with rows padded to KS + 16 bytes (the compute loop's 16 (8)-byte reads of 16 rows at
// one k offset fall into disjoint bank groups), double-buffered along K, one barrier per step; the 128 + TN exponent bytes of a block
// travel as fp32 powers of two beside the tile (lane t turns ONE byte into 2^(e - 127 - (p - 2)) once; 255 -> NaN, 0 -> 0).
//   A, and W in "nk": 16-byte global loads of a row's KS bytes into the padded row (rows past M / N clamped, nothing stored for them).
//   W in "kn": a K step arrives as KS rows of TN bytes; the MFMA operand wants consecutive k bytes for one n.  A lane loads FOUR dwords:
//     4 consecutive k rows (4 * kg + r) at the same 4 columns (4 * cg ..), i.e. a 4 x 4 byte tile, transposes it in registers with
//     v_perm_b32 (two byte-gathers and a shift-or per column: [d0.c, d1.c, 0, 0] | [d2.c, d3.c, 0, 0] << 16) and stores FOUR dwords, one per
//     column, at [4 * cg + c][4 * kg] of the same padded layout.  No byte-wide LDS access.  LDS position = global k: A needs no
//     permutation to match.  Column groups past N are clamped to the last group for the loads; their results are never stored.
//     A wave takes 16 column groups x 4 k groups: each of its load instructions reads 64 contiguous bytes of 4 rows.  (A tile row is
//     128 or 64 bytes: there is no 256-byte run to read.  The wider choice, 32 column groups x 2 k groups, was rejected on the count
//     below.)
//     Bank check of the four dword stores against the padded stride (64 banks of 4 bytes; dword index of lane (cg, kg), column c:
//     (4 cg + c) * S + kg with S = 20 (KS = 64) or 12 (KS = 32) dwords): cg contributes 16 cg (48 cg) mod 64 -- four classes only, so
//     with every lane storing column c in the same instruction 16 cg x 4 kg is a 4-way conflict and 32 cg x 2 kg 8-way.  Therefore
//     lane (cg, kg) stores column c = (i + cg / 4) % 4 in store instruction i (the perm selectors are per-lane registers, no select
//     chain): the bank is then (16 (cg % 4) + 20 c + kg) mod 64, resp. (48 (cg % 4) + 12 c + kg) mod 64, and over cg % 4, c, kg in
//     0 .. 3 these are 64 DISTINCT banks -- conflict-free (on 32 banks: two lanes per bank, the floor for 64 dwords).  Counted by
//     hand, not measured.
//   W exponents in "kn": one row of exps[K / B, N] -- TN contiguous bytes.
// Built without the packed fp32 instructions (build.py EXTRA_FLAGS, as bfp_matmul.hip); no scratch (build.py NO_SCRATCH).
#include "common.hpp"

namespace dmxq {

typedef int bm_i32x4 __attribute__((ext_vector_type(4)));
constexpr int kBmThreads = 256, kBmTileM = 128;

template <int KS> struct BmFrag;
template <> struct BmFrag<64> {
  typedef bm_i32x4 T;
  static __device__ __forceinline__ bm_i32x4 mfma(T a, T b, bm_i32x4 c) { return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0); }
};
template <> struct BmFrag<32> {
  typedef long T;
  static __device__ __forceinline__ bm_i32x4 mfma(T a, T b, bm_i32x4 c) { return __builtin_amdgcn_mfma_i32_16x16x32_i8(a, b, c, 0, 0, 0); }
};

// (two workgroups per CU everywhere but "kn" at B = 128 on the 128-wide tile: two chained halves in flight, 64 + 64 accumulators and the
//  transposing stage need a few registers more than 256, and scratch is not an option; that one class runs one workgroup per CU)
template <int DTO, int B, int TN, bool KN>
__global__ __launch_bounds__(kBmThreads, (KN && B == 128 && TN == 128) ? 1 : 2) void bfp_bmm_kernel(const int8_t* __restrict__ ca, const uint8_t* __restrict__ ea,
                                                                const int8_t* __restrict__ cw, const uint8_t* __restrict__ ew,
                                                                void* __restrict__ out, int M, int N, int64_t K, int64_t nb,
                                                                float down_a, float down_w, int vec_ok) {
  constexpr int KS = B == 128 ? 64 : B, HALVES = B / KS;       // bytes of a row per K step; steps per block
  constexpr int VPR = KS / 16, STRIDE = KS + 16, OPA = kBmTileM * STRIDE, OPW = TN * STRIDE;
  constexpr int LA = kBmTileM * VPR / kBmThreads;               // 16-byte vectors of the A tile per lane
  constexpr int WV = TN * VPR, LW = (WV + kBmThreads - 1) / kBmThreads;   // "nk": vectors of the W tile, per lane
  constexpr int WU = (TN / 64) * (KS / 16), LU = (WU + 3) / 4;  // "kn": units of 16 column groups x 4 k groups, per wave
  constexpr int MT = TN == 128 ? 4 : 2;                         // MFMA tile rows per wave
  typedef typename BmFrag<KS>::T Frag;
  __shared__ __attribute__((aligned(16))) uint8_t lds[2][OPA + OPW];          // [buffer][A tile | W tile]
  __shared__ __attribute__((aligned(16))) float lsc[2][kBmTileM + TN];        // [buffer][A row scales | W column scales]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = TN == 128 ? wave >> 1 : wave, wn = TN == 128 ? wave & 1 : 0;
  const int l16 = lane & 15, q = lane >> 4;
  const int m0 = blockIdx.y * kBmTileM, n0 = blockIdx.x * TN;
  const int64_t bz = blockIdx.z;
  ca += bz * M * K;
  ea += bz * M * nb;
  cw += bz * N * K;
  ew += bz * N * nb;
  const int64_t out0 = bz * M * N;

  // A (and W in "nk"): vector v = t + i * 256 of a tile is (row v / VPR, 16-byte chunk v % VPR); rows past the edge read the last row
  const int8_t* src_a[LA];
  int dst_a[LA];
#pragma unroll
  for (int i = 0; i < LA; i++) {
    const int v = t + i * kBmThreads, row = v / VPR, chunk = v % VPR;
    const int ra = m0 + row < M ? m0 + row : M - 1;
    src_a[i] = ca + (int64_t)ra * K + chunk * 16;
    dst_a[i] = row * STRIDE + chunk * 16;
  }
  // "kn": unit u of wave w is column groups 16 (w % CG) + l16, k groups 4 (w / CG + u * (4 / CG)) + q: unit u + 1 lies UK bytes along k
  // behind unit u, in LDS and (times N) in memory, so one source and four destinations serve every unit
  constexpr int CG = TN / 64, UK = 16 * (4 / CG);
  const int8_t* src_w[KN ? 1 : LW];
  int dst_w[KN ? 4 : LW];
  uint32_t sel[4];   // "kn": store instruction i takes column (i + cg / 4) % 4: [lo.c, hi.c, 0, 0]
  if constexpr (KN) {
    const int rot = (lane >> 2) & 3, cg = (wave % CG) * 16 + l16, kg = (wave / CG) * 4 + q;
    const int col = n0 + 4 * cg < N ? n0 + 4 * cg : N - 4;   // (N % 4 == 0, N >= 4)
    src_w[0] = cw + (int64_t)(4 * kg) * N + col;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int c = (i + rot) & 3;
      sel[i] = 0x0c0c0400u + (uint32_t)c * 0x00000101u;
      dst_w[i] = (4 * cg + c) * STRIDE + 4 * kg;
    }
  } else {
#pragma unroll
    for (int i = 0; i < LW; i++) {
      const int v = (t + i * kBmThreads) % WV, row = v / VPR, chunk = v % VPR;   // (% WV: the idle lanes of a 128-vector tile stay in range)
      const int rw = n0 + row < N ? n0 + row : N - 1;
      src_w[i] = cw + (int64_t)rw * K + chunk * 16;
      dst_w[i] = row * STRIDE + chunk * 16;
    }
  }
  const bool w_lane = WV % kBmThreads == 0 || t < WV;          // "nk": this lane has a vector of the W tile
  const bool w_wave = WU % 4 == 0 || wave < WU;                // "kn": this wave has a unit of the W tile (KS = 32, TN = 64: two waves)
  const bool is_w = t >= kBmTileM, has_e = t < kBmTileM + TN;
  const int er = is_w ? (n0 + t - kBmTileM < N ? n0 + t - kBmTileM : N - 1) : (m0 + t < M ? m0 + t : M - 1);
  const uint8_t* src_e = is_w ? (KN ? ew + er : ew + (int64_t)er * nb) : ea + (int64_t)er * nb;
  const int e_step = (KN && is_w) ? N : 1;
  const float down = is_w ? down_w : down_a;

  u32x4 ga[LA], gw[KN ? 1 : LW];
  uint32_t gk[KN ? LU : 1][4];
  uint32_t ge = 0u;
  auto gload = [&](int64_t s) {   // step s: bytes [s * KS, s * KS + KS) along K, the exponents of block s / HALVES
#pragma unroll
    for (int i = 0; i < LA; i++) ga[i] = *(const u32x4*)(src_a[i] + s * KS);
    if constexpr (KN) {
      if (w_wave) {
#pragma unroll
        for (int u = 0; u < LU; u++)
#pragma unroll
          for (int r = 0; r < 4; r++) gk[u][r] = *(const uint32_t*)(src_w[0] + (s * KS + u * UK + r) * N);
      }
    } else {
      if (w_lane) {
#pragma unroll
        for (int i = 0; i < LW; i++) gw[i] = *(const u32x4*)(src_w[i] + s * KS);
      }
    }
    if (has_e) ge = src_e[(s / HALVES) * (int64_t)e_step];
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < LA; i++) *(u32x4*)(lds[buf] + dst_a[i]) = ga[i];
    if constexpr (KN) {
      if (w_wave) {
#pragma unroll
        for (int u = 0; u < LU; u++)
#pragma unroll
          for (int i = 0; i < 4; i++)
            *(uint32_t*)(lds[buf] + OPA + dst_w[i] + u * UK) =   // [d0.c, d1.c, 0, 0] | [d2.c, d3.c, 0, 0] << 16
                __builtin_amdgcn_perm(gk[u][1], gk[u][0], sel[i]) | (__builtin_amdgcn_perm(gk[u][3], gk[u][2], sel[i]) << 16);
      }
    } else {
      if (w_lane) {
#pragma unroll
        for (int i = 0; i < LW; i++) *(u32x4*)(lds[buf] + OPA + dst_w[i]) = gw[i];
      }
    }
    if (has_e) lsc[buf][t] = ge == 255u ? u2f(0x7FC00000u) : u2f(ge << 23) * down;   // 2^(e - 127 - (p - 2)); e = 0: 0
  };

  // a lane's operand: row l16 of a 16-row tile, quarter q of the step's bytes (the same quarter of A and of W)
  const int off_a = (wm * MT * 16 + l16) * STRIDE + q * (KS / 4);
  const int off_w = OPA + (wn * 64 + l16) * STRIDE + q * (KS / 4);

  float acc[MT][4][4];
#pragma unroll
  for (int mt = 0; mt < MT; mt++)
#pragma unroll
    for (int nt = 0; nt < 4; nt++)
#pragma unroll
      for (int i = 0; i < 4; i++) acc[mt][nt][i] = 0.0f;

  gload(0);
  lstore(0);
  __syncthreads();
  const int64_t steps = nb * HALVES;
  bm_i32x4 P[MT][4];
  for (int64_t j = 0; j < nb; j++) {
#pragma unroll
    for (int h = 0; h < HALVES; h++) {
      const int64_t s = j * HALVES + h;
      const int buf = (int)(s & 1);
      if (s + 1 < steps) gload(s + 1);
      Frag fa[MT], fw[4];
#pragma unroll
      for (int k = 0; k < MT; k++) fa[k] = *(const Frag*)(lds[buf] + off_a + k * 16 * STRIDE);
#pragma unroll
      for (int k = 0; k < 4; k++) fw[k] = *(const Frag*)(lds[buf] + off_w + k * 16 * STRIDE);
#pragma unroll
      for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int nt = 0; nt < 4; nt++)
          P[mt][nt] = BmFrag<KS>::mfma(fw[nt], fa[mt], h == 0 ? bm_i32x4{0, 0, 0, 0} : P[mt][nt]);   // D[n][m]: rows from W, columns from A
      if (h == HALVES - 1) {
        float sa[MT];
        f32x4 sw[4];
#pragma unroll
        for (int k = 0; k < MT; k++) sa[k] = lsc[buf][wm * MT * 16 + k * 16 + l16];
#pragma unroll
        for (int k = 0; k < 4; k++) sw[k] = *(const f32x4*)(&lsc[buf][kBmTileM + wn * 64 + k * 16 + 4 * q]);
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
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
  for (int mt = 0; mt < MT; mt++) {
    const int m = m0 + wm * MT * 16 + mt * 16 + l16;
    if (m >= M) continue;
#pragma unroll
    for (int nt = 0; nt < 4; nt++) {
      const int n = n0 + wn * 64 + nt * 16 + 4 * q;
      const int64_t e0 = out0 + (int64_t)m * N + n;
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

// class value: 1 + 2 * (3 * w_layout + block index) + (TN == 64)
extern "C" int dmxq_bfp_bmm_class(int64_t batch, int64_t M, int64_t N, int64_t K, int64_t block_size, int w_layout) {
  if (batch < 1 || batch > 65535 || M < 1 || N < 1 || K < 1) return DMXQ_BFPBMM_NONE;   // grid.z: the caller splits larger batches
  if (w_layout != DMXQ_BFPBMM_NK && w_layout != DMXQ_BFPBMM_KN) return DMXQ_BFPBMM_NONE;
  if (block_size != 32 && block_size != 64 && block_size != 128) return DMXQ_BFPBMM_NONE;
  if (K % block_size != 0) return DMXQ_BFPBMM_NONE;
  if (w_layout == DMXQ_BFPBMM_KN && N % 4 != 0) return DMXQ_BFPBMM_NONE;
  if (M > (int64_t)65535 * kBmTileM || N > 0x7FFFFF00) return DMXQ_BFPBMM_NONE;   // grid.y; 32-bit row / column indices
  const int bi = block_size == 32 ? 0 : (block_size == 64 ? 1 : 2);
  return 1 + 2 * (3 * w_layout + bi) + (N <= 64 ? 1 : 0);
}

extern "C" int dmxq_bfp_bmm(const int8_t* mant_a, const uint8_t* exps_a, const int8_t* mant_w, const uint8_t* exps_w, void* out,
                            int dtype_out, int64_t batch, int64_t M, int64_t N, int64_t K, int64_t block_size, int prec_a, int prec_w,
                            int w_layout, void* stream) {
  if (!valid_dtype(dtype_out) || batch < 0 || M < 0 || N < 0 || K < 0 || block_size < 1) return DMXQ_ERR_BAD_ARG;
  if (w_layout != DMXQ_BFPBMM_NK && w_layout != DMXQ_BFPBMM_KN) return DMXQ_ERR_BAD_ARG;
  if (prec_a < 2 || prec_a > 8 || prec_w < 2 || prec_w > 8) return DMXQ_ERR_UNSUPPORTED;
  if (batch * M * N == 0) return DMXQ_OK;
  if (!mant_a || !exps_a || !mant_w || !exps_w || !out) return DMXQ_ERR_BAD_ARG;
  const int cls = dmxq_bfp_bmm_class(batch, M, N, K, block_size, w_layout);
  if (cls == DMXQ_BFPBMM_NONE || !aligned16(mant_a)) return DMXQ_ERR_UNSUPPORTED;   // (K % 32 == 0: every row and batch element 16-byte aligned)
  if (w_layout == DMXQ_BFPBMM_KN ? (reinterpret_cast<uintptr_t>(mant_w) & 3u) != 0 : !aligned16(mant_w)) return DMXQ_ERR_UNSUPPORTED;
  const int ob = dtype_out == DMXQ_F32 ? 4 : 2;
  const int vec_ok = N % 4 == 0 && (reinterpret_cast<uintptr_t>(out) % (4 * ob)) == 0;
  const float down_a = 1.0f / (float)(1 << (prec_a - 2)), down_w = 1.0f / (float)(1 << (prec_w - 2));   // 2^-(p - 2), exact
  const int tn = N <= 64 ? 64 : 128;
  const dim3 grid((unsigned)((N + tn - 1) / tn), (unsigned)((M + kBmTileM - 1) / kBmTileM), (unsigned)batch);
  hipStream_t s = (hipStream_t)stream;
#define DMXQ_BM(DT_, B_, TN_, KN_) DMXQ_LAUNCH((bfp_bmm_kernel<DT_, B_, TN_, KN_>), grid, dim3(kBmThreads), 0, s, mant_a, exps_a, mant_w, exps_w, out, (int)M, (int)N, K, K / block_size, down_a, down_w, vec_ok)
#define DMXQ_BML(DT_, B_, TN_) do { if (w_layout == DMXQ_BFPBMM_KN) DMXQ_BM(DT_, B_, TN_, true); else DMXQ_BM(DT_, B_, TN_, false); } while (0)
#define DMXQ_BMT(DT_, B_) do { if (tn == 64) DMXQ_BML(DT_, B_, 64); else DMXQ_BML(DT_, B_, 128); } while (0)
#define DMXQ_BMB(DT_) do { if (block_size == 32) DMXQ_BMT(DT_, 32); else if (block_size == 64) DMXQ_BMT(DT_, 64); else DMXQ_BMT(DT_, 128); } while (0)
  if (dtype_out == DMXQ_F32) DMXQ_BMB(DMXQ_F32);
  else if (dtype_out == DMXQ_F16) DMXQ_BMB(DMXQ_F16);
  else DMXQ_BMB(DMXQ_BF16);
#undef DMXQ_BM
#undef DMXQ_BML
#undef DMXQ_BMT
#undef DMXQ_BMB
  return launch_status();
}
