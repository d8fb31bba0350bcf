// csrc/gptq.hip — GPTQ's in-block column loop (layer_reconstruction.py:300-318) for ONE column block of <= 128 columns in one launch.
//
// The reference runs that loop in Python: per microblock of columns, weight_hypernet on the [rows, m] slice, torch.linalg.inv of the
// microblock's diagonal block of Hinv, two matmuls and slice copies -- at least 5 launches per column at microblock 1.  Here the host
// keeps what is GEMM-shaped (Hessian, Cholesky factorisations, the batched inverse of the diagonal microblocks, the trailing update
// W[:, i2:] -= E @ Hinv[i1:i2, i2:]) on torch's libraries, and this kernel does everything in between.
//
// Geometry: rows are independent given Hinv, so one LANE per weight row, one 64-lane wave per workgroup.  The workgroup's [64, count]
// block of W is read along the rows into LDS (column-major, a lane's four columns in one 16-byte slot: the update reads and writes
// them as one ds_read_b128 / ds_write_b128, conflict-free), next to the Hinv block (zero outside the upper triangle of
// [count, count], read as wave-uniform broadcasts) and E; inv_d is read with wave-uniform loads; the current microblock (<= 64
// columns) and its errors live in VGPRs.  Q overwrites W's columns as they become final, and Q and E leave along the rows at the
// end.  No cross-lane traffic; 128 KiB of LDS per workgroup.  (A first form kept the whole row in VGPRs with the column loops
// unrolled: at 128 columns the unroller gives up and the array goes to scratch.)
//
// Arithmetic order (every product and difference separately rounded: the library is built with -ffp-contract=off), with w the row's
// block as it is updated, H = Hinv block, D = inv_d of the current microblock, m = min(MB, count - j1) the microblock's width:
//   for each microblock j1 = 0, MB, 2 MB, ...:
//     q_i   = cast(w[j1 .. j1 + m))_i                                  (the module's weight cast of the [rows, m] slice, bit for bit)
//     d_i   = w_{j1+i} - q_i
//     err_c = d_0 * D[0][c];  err_c = err_c + d_i * D[i][c]   for i = 1 .. m-1 in order
//     for every later column k of the block:
//       acc = err_0 * H[j1][k];  acc = acc + err_i * H[j1+i][k]   for i = 1 .. m-1 in order;  w_k = w_k - acc
// At MB = 1 this is the reference's own order: q = cast(w_j), e = (w_j - q) * (1 / H[j][j]), w_k = w_k - e * H[j][k].
// Formats (casts from bfp_math.hpp / floatq.hpp / fixedq.hpp, the literal reference forms; the per-column cast is a small share of
// the O(count^2) update, so no fast forms are needed here):
//   BFP    nearest rounding, symmetric or "(_N)"; blocks of `block_size` along the slice's columns from its first column (a ragged
//          last microblock closes its last block early, torch.split semantics); block maxima are lane-local (one row per lane)
//   FLOAT  nearest rounding
//   FIXED  nearest rounding, affine x / sc + zp -> cast -> (x - zp) * sc with IEEE division (numerical/cast.py:278-296), the scale and
//          zero point of the row (per-output-channel) or of the whole tensor
//
// The loop itself lives in gptq_cols.hpp (gptq_block_body), which csrc/gptq_dynamic.hip shares: there the FIXED cast's scale and zero
// point are derived per group of columns inside the loop instead of being read here before it.
#include "gptq_cols.hpp"

namespace dmxq {

template <int KIND, int MB, bool ASYM>
__global__ __launch_bounds__(kGptqRows) void gptq_block_kernel(const float* __restrict__ wsrc, int64_t ldw, float* __restrict__ qdst,
                                                             int64_t ldq, float* __restrict__ edst, int64_t lde, int64_t rows, int count,
                                                             const float* __restrict__ hinv, int64_t ldh, const float* __restrict__ inv_d,
                                                             const float* __restrict__ scale, const int64_t* __restrict__ zp, GptqCast c) {
  gptq_block_body<KIND, MB, ASYM>(wsrc, ldw, qdst, ldq, edst, lde, rows, count, hinv, ldh, inv_d, scale, zp, c, GptqStoredScales{});
}

}  // namespace dmxq

using namespace dmxq;

extern "C" int dmxq_gptq_block(const float* w, int64_t ldw, float* q, int64_t ldq, float* err, int64_t lde, int64_t rows, int64_t count,
                               const float* hinv, int64_t ldh, const float* inv_d, int64_t microblock, const dmxq_gptq_format* fmt,
                               const float* scale, const int64_t* zero_point, void* stream) {
  if (!fmt || rows < 0 || count < 0 || microblock < 1) return DMXQ_ERR_BAD_ARG;
  if (fmt->kind != DMXQ_GPTQ_BFP && fmt->kind != DMXQ_GPTQ_FLOAT && fmt->kind != DMXQ_GPTQ_FIXED) return DMXQ_ERR_BAD_ARG;
  if (rows == 0 || count == 0) return DMXQ_OK;
  if (!w || !q || !err || !hinv || !inv_d || ldw < count || ldq < count || lde < count || ldh < count) return DMXQ_ERR_BAD_ARG;
  if (rows >= ((int64_t)1 << 37)) return DMXQ_ERR_BAD_ARG;  // (grid of rows / 64 workgroups)
  const int mb = (int)microblock;
  if (count > kGptqCols || !(mb == 1 || mb == 8 || mb == 16 || mb == 32 || mb == 64)) return DMXQ_ERR_UNSUPPORTED;
  if (fmt->kind == DMXQ_GPTQ_FIXED && (!scale || !zero_point)) return DMXQ_ERR_BAD_ARG;
  FormatDesc d;
  if (format_desc(*fmt, &d) != DMXQ_OK) return DMXQ_ERR_UNSUPPORTED;
  GptqCast c{};
  c.wl = d.wl;
  c.f = d.f;
  c.x = d.x;
  c.per_row = fmt->kind == DMXQ_GPTQ_FIXED && fmt->per_row ? 1 : 0;
  const bool asym = d.asym != 0;
  if (fmt->kind == DMXQ_GPTQ_BFP) {
    const int B = fmt->block_size;
    if (B < 2 || mb % B != 0) return DMXQ_ERR_UNSUPPORTED;
    for (int i = 0; i < mb; i++)
      if ((i + 1) % B == 0) c.ends |= 1ull << i;
  }
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((rows + kGptqRows - 1) / kGptqRows));
#define DMXQ_GPTQ(K_, M_, A_) DMXQ_LAUNCH((gptq_block_kernel<K_, M_, A_>), grid, dim3(kGptqRows), 0, s, w, ldw, q, ldq, err, lde, rows, \
                                          (int)count, hinv, ldh, inv_d, scale, zero_point, c)
#define DMXQ_GPTQ_MB(K_, A_)                  \
  switch (mb) {                               \
    case 1: DMXQ_GPTQ(K_, 1, A_); break;      \
    case 8: DMXQ_GPTQ(K_, 8, A_); break;      \
    case 16: DMXQ_GPTQ(K_, 16, A_); break;    \
    case 32: DMXQ_GPTQ(K_, 32, A_); break;    \
    default: DMXQ_GPTQ(K_, 64, A_); break;    \
  }
  if (fmt->kind == DMXQ_GPTQ_FLOAT) {
    DMXQ_GPTQ_MB(DMXQ_GPTQ_FLOAT, false);
  } else if (fmt->kind == DMXQ_GPTQ_FIXED) {
    DMXQ_GPTQ_MB(DMXQ_GPTQ_FIXED, false);
  } else {
    switch (mb) {  // (BFP blocks have >= 2 elements: no microblock of 1)
      case 8: if (asym) DMXQ_GPTQ(DMXQ_GPTQ_BFP, 8, true); else DMXQ_GPTQ(DMXQ_GPTQ_BFP, 8, false); break;
      case 16: if (asym) DMXQ_GPTQ(DMXQ_GPTQ_BFP, 16, true); else DMXQ_GPTQ(DMXQ_GPTQ_BFP, 16, false); break;
      case 32: if (asym) DMXQ_GPTQ(DMXQ_GPTQ_BFP, 32, true); else DMXQ_GPTQ(DMXQ_GPTQ_BFP, 32, false); break;
      default: if (asym) DMXQ_GPTQ(DMXQ_GPTQ_BFP, 64, true); else DMXQ_GPTQ(DMXQ_GPTQ_BFP, 64, false); break;
    }
  }
#undef DMXQ_GPTQ_MB
#undef DMXQ_GPTQ
  return launch_status();
}
