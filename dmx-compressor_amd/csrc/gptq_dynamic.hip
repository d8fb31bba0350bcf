// csrc/gptq_dynamic.hip — GPTQ's in-block column loop with DYNAMIC per-group integer scales (include/dmxq.h dmxq_gptq_block_dynamic;
// DESIGN.md §8): the W4 g128 recipe.  The loop, its geometry and its arithmetic order are csrc/gptq.hip's, shared through
// gptq_cols.hpp (gptq_block_body); what is added is the group step, per row, with w the row's block as the loop updates it:
//   at every column j with j % group == 0, before the microblock that starts there is cast:
//     (mn, mx) = dmxq_group_minmax of the float32 values w[j .. j + group) AS THEY STAND -- the updates of every earlier microblock of
//                this block and, through the caller's trailing GEMMs, of every earlier block are in them (one NaN makes both NaN);
//     (sc, zp) = dmxq_qparams(mn, mx, qmin, qmax, symmetric_qscheme) -- reduce_common.hpp qparams_one, the function csrc/reduce.hip and
//                csrc/dynamic_quant.hip call; written to scale_out / zp_out [row][j / group];
//   every column of the group is cast with that (sc, zp) exactly as DMXQ_GPTQ_FIXED casts with a per-row scale:
//     (fixed_q1(w / sc + zp) - zp) * sc, IEEE division, nearest rounding.
// A lane owns a row and the row's block sits in LDS, so the extrema are a lane-local scan of group / 4 sixteen-byte LDS slots at each
// group start: O(count) per row next to the O(count^2) update.  No LDS beyond the shared loop's 128 KiB; scale_out / zp_out are written
// straight from the lanes (count / group <= 8 entries per row).  Nothing is allocated and nothing waits for the host: capturable.
#include "gptq_cols.hpp"

namespace dmxq {

template <int MB>
__global__ __launch_bounds__(kGptqRows) void gptq_block_dynamic_kernel(const float* __restrict__ wsrc, int64_t ldw, float* __restrict__ qdst,
                                                                     int64_t ldq, float* __restrict__ edst, int64_t lde, int64_t rows,
                                                                     int count, const float* __restrict__ hinv, int64_t ldh,
                                                                     const float* __restrict__ inv_d, GptqCast c, GptqGroupScales dyn) {
  gptq_block_body<DMXQ_GPTQ_FIXED, MB, false>(wsrc, ldw, qdst, ldq, edst, lde, rows, count, hinv, ldh, inv_d, nullptr, nullptr, c, dyn);
}

}  // namespace dmxq

using namespace dmxq;

extern "C" int dmxq_gptq_block_dynamic(const float* w, int64_t ldw, float* q, int64_t ldq, float* err, int64_t lde, int64_t rows,
                                       int64_t count, const float* hinv, int64_t ldh, const float* inv_d, int64_t microblock,
                                       const dmxq_gptq_format* fmt, int rounding, int64_t group, int qmin, int qmax, int symmetric_qscheme,
                                       float* scale_out, int64_t lds, int64_t* zp_out, int64_t ldz, void* stream) {
  if (!fmt || rows < 0 || count < 0 || microblock < 1 || group < 1) return DMXQ_ERR_BAD_ARG;
  if (fmt->kind != DMXQ_GPTQ_FIXED || !valid_rounding(rounding) || qmax <= qmin) return DMXQ_ERR_BAD_ARG;
  if (rows == 0 || count == 0) return DMXQ_OK;
  if (!w || !q || !err || !hinv || !inv_d || ldw < count || ldq < count || lde < count || ldh < count) return DMXQ_ERR_BAD_ARG;
  if (!scale_out || !zp_out) return DMXQ_ERR_BAD_ARG;
  if (rows >= ((int64_t)1 << 37)) return DMXQ_ERR_BAD_ARG;  // (grid of rows / 64 workgroups)
  // what the kernel takes; everything else is the caller's loop (nothing launched)
  const int mb = (int)microblock;
  if (count > kGptqCols || !(mb == 1 || mb == 8 || mb == 16 || mb == 32 || mb == 64)) return DMXQ_ERR_UNSUPPORTED;
  if (!(group == 16 || group == 32 || group == 64 || group == 128) || count % group != 0 || group % mb != 0) return DMXQ_ERR_UNSUPPORTED;
  FormatDesc d;
  if (format_desc(*fmt, &d) != DMXQ_OK) return DMXQ_ERR_UNSUPPORTED;
  if (rounding != DMXQ_ROUND_NEAREST || fmt->fraction != 0 || !fmt->clamp || fmt->precision > 22) return DMXQ_ERR_UNSUPPORTED;
  if (lds < count / group || ldz < count / group) return DMXQ_ERR_BAD_ARG;
  GptqCast c{};
  c.x = d.x;
  c.per_row = 1;
  int l2 = 4;
  while (((int64_t)1 << l2) < group) l2++;
  const GptqGroupScales dyn{(int)group, l2, qmin, qmax, symmetric_qscheme ? 1 : 0, scale_out, zp_out, lds, ldz};
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((rows + kGptqRows - 1) / kGptqRows));
#define DMXQ_GPTQ_DYN(M_) DMXQ_LAUNCH((gptq_block_dynamic_kernel<M_>), grid, dim3(kGptqRows), 0, s, w, ldw, q, ldq, err, lde, rows, (int)count, \
                                      hinv, ldh, inv_d, c, dyn)
  switch (mb) {
    case 1: DMXQ_GPTQ_DYN(1); break;
    case 8: DMXQ_GPTQ_DYN(8); break;
    case 16: DMXQ_GPTQ_DYN(16); break;
    case 32: DMXQ_GPTQ_DYN(32); break;
    default: DMXQ_GPTQ_DYN(64); break;
  }
#undef DMXQ_GPTQ_DYN
  return launch_status();
}
