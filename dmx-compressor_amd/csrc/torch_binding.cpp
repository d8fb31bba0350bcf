// csrc/torch_binding.cpp — the thin torch extension over the C ABI of libdmxq.so (include/dmxq.h).
//
// Replaces the reference's pybind seam (quant/quant_cuda/quant_cuda.cpp:116-139: allocate with zeros_like, launch,
// return a new tensor) for the whole hot path: `torch.ops.dmxq.*`.  This file contains NO arithmetic: every op
//   1. checks / makes its tensors contiguous and factors the shape as [outer, L, inner] around the blocked dim,
//   2. allocates the outputs (torch's caching allocator: the ownership contract of the reference's native functions),
//   3. makes the tensor's device current (device guard) and passes torch's CURRENT HIP stream of that device,
//   4. calls ONE extern "C" entry point of include/dmxq.h.
// Meta kernels (shape / dtype propagation only) make the ops traceable by torch.compile / torch.export with fake
// tensors (the reference's `export=True` path, fx/transform.py:133-178); the straight-through-estimator backward is
// registered from Python (torch.library.register_autograd, dmx-compressor_amd/_torch_ops.py).
// Host-only C++: compiled with g++ against the torch headers, linked to libdmxq.so; no device code here.
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/library.h>

#include <tuple>
#include <vector>

#include "../../include/dmxq.h"

namespace {

using at::Tensor;
using OptDtype = c10::optional<at::ScalarType>;
using OptTensor = c10::optional<Tensor>;

inline int dt_code(at::ScalarType t) {
  switch (t) {
    case at::kFloat: return DMXQ_F32;
    case at::kHalf: return DMXQ_F16;
    case at::kBFloat16: return DMXQ_BF16;
    default: TORCH_CHECK_TYPE(false, "dmxq kernels take float32/float16/bfloat16 tensors, got ", t);
  }
  return -1;
}

inline void check(int rc, const char* what) {
  if (rc == DMXQ_OK) return;
  if (rc == DMXQ_ERR_UNSUPPORTED) TORCH_CHECK_NOT_IMPLEMENTED(false, what, ": ", dmxq_status_string(rc));
  TORCH_CHECK(false, what, ": ", dmxq_status_string(rc), " (status ", rc, ")");
}

struct Split3 { int64_t outer, L, inner; };
inline Split3 split3(const Tensor& x, int64_t dim) {
  const int64_t nd = x.dim();
  if (nd == 0) return {1, 1, 1};
  const int64_t d = ((dim % nd) + nd) % nd;
  Split3 s{1, x.size(d), 1};
  for (int64_t i = 0; i < d; i++) s.outer *= x.size(i);
  for (int64_t i = d + 1; i < nd; i++) s.inner *= x.size(i);
  return s;
}

inline Tensor prep(const Tensor& x, const char* what) {
  TORCH_CHECK(x.is_cuda(), what, ": tensor is on ", x.device(),
              "; dmx_compressor_amd runs on MI355X (HIP) tensors only and has no CPU fallback");
  dt_code(x.scalar_type());
  return x.contiguous();
}

// device guard + torch's current stream on the tensor's device (never the null stream)
struct Launch {
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard;
  void* stream;
  explicit Launch(const Tensor& x) : guard(x.device()) {
    stream = (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(x.device().index()).stream();
  }
};

inline Tensor empty_like_shape(const Tensor& x, OptDtype dt) {
  return at::empty(x.sizes(), x.options().dtype(dt.value_or(x.scalar_type())).memory_format(at::MemoryFormat::Contiguous));
}

inline const void* cptr(const OptTensor& t) { return t.has_value() && t->defined() ? t->data_ptr() : nullptr; }

// ------------------------------------------------------------------------------------------------ block formats
Tensor bfp_qdq(const Tensor& x, int64_t precision, int64_t block_size, int64_t block_dim, bool symmetric, int64_t rounding,
               OptDtype out_dtype, int64_t seed) {
  const Tensor xc = prep(x, "bfp_qdq");
  Tensor out = empty_like_shape(xc, out_dtype);
  const Split3 s = split3(xc, block_dim);
  Launch l(xc);
  check(dmxq_bfp_qdq(xc.data_ptr(), out.data_ptr(), dt_code(xc.scalar_type()), dt_code(out.scalar_type()), s.outer, s.L, s.inner,
                     block_size, (int)precision, (int)rounding, symmetric, (uint64_t)seed, l.stream), "dmxq_bfp_qdq");
  return out;
}
Tensor bfp_qdq_meta(const Tensor& x, int64_t, int64_t, int64_t, bool, int64_t, OptDtype out_dtype, int64_t) {
  return empty_like_shape(x, out_dtype);
}

// the pybind seam block_quantize_<rounding>(a, wl, dim, symmetric) on a [rows, L] float32 view, one block per row;
// symmetric = false selects the NATIVE asymmetric branch (quant_cpu.cpp:247-253), not the "(_N)" format post-pass
Tensor block_quantize(const Tensor& a, int64_t wl, bool symmetric, int64_t rounding, int64_t seed) {
  const Tensor xc = prep(a, "block_quantize");
  TORCH_CHECK(xc.dim() == 2, "block_quantize: expects a [rows, L] view");
  Tensor out = at::empty_like(xc);
  Launch l(xc);
  check(dmxq_bfp_qdq(xc.data_ptr(), out.data_ptr(), dt_code(xc.scalar_type()), dt_code(out.scalar_type()), xc.size(0), xc.size(1), 1,
                     std::max<int64_t>(xc.size(1), 2), (int)wl, (int)rounding, symmetric ? 1 : DMXQ_BFP_ASYM_NATIVE, (uint64_t)seed,
                     l.stream), "dmxq_bfp_qdq");
  return out;
}
Tensor block_quantize_meta(const Tensor& a, int64_t, bool, int64_t, int64_t) { return at::empty_like(a); }

std::vector<Tensor> bfp_qdq_multi(at::TensorList xs, int64_t precision, int64_t block_size, int64_t block_dim, bool symmetric,
                                  int64_t rounding, OptDtype out_dtype, int64_t seed) {
  std::vector<Tensor> outs, ins;
  if (xs.empty()) return outs;
  std::vector<dmxq_tensor_desc> d(xs.size());
  for (size_t i = 0; i < xs.size(); i++) {
    ins.push_back(prep(xs[i], "bfp_qdq_multi"));
    TORCH_CHECK(ins[i].scalar_type() == ins[0].scalar_type() && ins[i].device() == ins[0].device(),
                "bfp_qdq_multi: all tensors must share one dtype and one device");
    outs.push_back(empty_like_shape(ins[i], out_dtype));
    const Split3 s = split3(ins[i], block_dim);
    d[i] = dmxq_tensor_desc{ins[i].data_ptr(), outs[i].data_ptr(), s.outer, s.L, s.inner};
  }
  Launch l(ins[0]);
  check(dmxq_bfp_qdq_multi(d.data(), (int64_t)d.size(), dt_code(ins[0].scalar_type()), dt_code(outs[0].scalar_type()), block_size,
                           (int)precision, (int)rounding, symmetric, (uint64_t)seed, l.stream), "dmxq_bfp_qdq_multi");
  return outs;
}
std::vector<Tensor> bfp_qdq_multi_meta(at::TensorList xs, int64_t, int64_t, int64_t, bool, int64_t, OptDtype out_dtype, int64_t) {
  std::vector<Tensor> outs;
  for (const Tensor& x : xs) outs.push_back(empty_like_shape(x, out_dtype));
  return outs;
}

std::vector<int64_t> exps_shape(const Tensor& x, int64_t block_size) {
  std::vector<int64_t> sh(x.sizes().begin(), x.sizes().end());
  const int64_t L = sh.empty() ? 1 : sh.back();
  if (sh.empty()) sh.push_back(0);
  sh.back() = (L + block_size - 1) / block_size;
  return sh;
}
std::tuple<Tensor, Tensor> bfp_pack(const Tensor& x, int64_t precision, int64_t block_size, bool symmetric) {
  const Tensor xc = prep(x, "bfp_pack");
  TORCH_CHECK(block_size >= 1, "bfp_pack: block_size must be positive");
  const int64_t L = xc.dim() ? xc.size(-1) : 1;
  const int64_t rows = L ? xc.numel() / L : 0;
  Tensor mant = at::empty(xc.sizes(), xc.options().dtype(at::kChar));
  Tensor exps = at::empty(exps_shape(xc, block_size), xc.options().dtype(at::kByte));
  Launch l(xc);
  check(dmxq_bfp_pack(xc.data_ptr(), dt_code(xc.scalar_type()), (int8_t*)mant.data_ptr(), (uint8_t*)exps.data_ptr(), rows, L,
                      block_size, (int)precision, symmetric, l.stream), "dmxq_bfp_pack");
  return {mant, exps};
}
std::tuple<Tensor, Tensor> bfp_pack_meta(const Tensor& x, int64_t, int64_t block_size, bool) {
  return {at::empty(x.sizes(), x.options().dtype(at::kChar)), at::empty(exps_shape(x, block_size < 1 ? 1 : block_size), x.options().dtype(at::kByte))};
}

Tensor bfp_unpack(const Tensor& mant, const Tensor& exps, int64_t precision, int64_t block_size, at::ScalarType out_dtype) {
  TORCH_CHECK(mant.is_cuda() && exps.is_cuda(), "bfp_unpack: tensors must be on the GPU (no CPU fallback)");
  const Tensor m = mant.contiguous(), e = exps.contiguous();
  const int64_t L = m.dim() ? m.size(-1) : 1;
  const int64_t rows = L ? m.numel() / L : 0;
  Tensor out = at::empty(m.sizes(), m.options().dtype(out_dtype));
  Launch l(m);
  check(dmxq_bfp_unpack((const int8_t*)m.data_ptr(), (const uint8_t*)e.data_ptr(), out.data_ptr(), dt_code(out_dtype), rows, L,
                        block_size, (int)precision, l.stream), "dmxq_bfp_unpack");
  return out;
}
Tensor bfp_unpack_meta(const Tensor& mant, const Tensor&, int64_t, int64_t, at::ScalarType out_dtype) {
  return at::empty(mant.sizes(), mant.options().dtype(out_dtype));
}

at::ScalarType hypernet_dtype(const Tensor& w, const OptTensor& score, int64_t M, OptDtype out_dtype) {
  const bool masked = score.has_value() && score->defined() && M != 0;
  return out_dtype.value_or(masked ? at::promote_types(w.scalar_type(), score->scalar_type()) : w.scalar_type());
}
Tensor weight_hypernet(const Tensor& w, int64_t precision, int64_t block_size, bool symmetric, const OptTensor& score, int64_t K,
                       int64_t M, const OptTensor& sq_scale, OptDtype out_dtype, int64_t block_dim) {
  const Tensor wc = prep(w, "weight_hypernet");
  const bool masked = score.has_value() && score->defined() && M != 0;
  Tensor sc, sq;
  if (masked) {
    sc = prep(*score, "weight_hypernet");
    TORCH_CHECK_NOT_IMPLEMENTED(sc.sizes() == wc.sizes(), "weight_hypernet: score and weight shapes differ");
  }
  const Split3 s3 = split3(wc, wc.dim() ? block_dim : -1);
  const int64_t L = s3.L;
  const int64_t rows = L ? wc.numel() / L : 0;
  if (sq_scale.has_value() && sq_scale->defined()) {
    sq = sq_scale->detach().to(wc.device(), at::kFloat).contiguous();
    TORCH_CHECK_NOT_IMPLEMENTED(sq.numel() == L, "weight_hypernet: scale length differs from the channel count");
  }
  Tensor out = empty_like_shape(wc, hypernet_dtype(wc, score, M, out_dtype));
  Launch l(wc);
  if (s3.inner != 1) {  // blocks / groups / channels along a non-contiguous dim (conv weights): the strided form
    check(dmxq_weight_hypernet_strided(wc.data_ptr(), dt_code(wc.scalar_type()), masked ? sc.data_ptr() : nullptr,
                                       masked ? dt_code(sc.scalar_type()) : 0, (int)K, masked ? (int)M : 0,
                                       sq.defined() ? (const float*)sq.data_ptr() : nullptr, out.data_ptr(), dt_code(out.scalar_type()),
                                       s3.outer, L, s3.inner, block_size, (int)precision, symmetric, l.stream), "dmxq_weight_hypernet_strided");
    return out;
  }
  check(dmxq_weight_hypernet(wc.data_ptr(), dt_code(wc.scalar_type()), masked ? sc.data_ptr() : nullptr,
                             masked ? dt_code(sc.scalar_type()) : 0, (int)K, masked ? (int)M : 0,
                             sq.defined() ? (const float*)sq.data_ptr() : nullptr, out.data_ptr(), dt_code(out.scalar_type()), rows, L,
                             block_size, (int)precision, symmetric, l.stream), "dmxq_weight_hypernet");
  return out;
}
Tensor weight_hypernet_meta(const Tensor& w, int64_t, int64_t, bool, const OptTensor& score, int64_t, int64_t M, const OptTensor&,
                            OptDtype out_dtype, int64_t) {
  return empty_like_shape(w, hypernet_dtype(w, score, M, out_dtype));
}

// the Linear weights of a layer in one launch (dmxq_weight_hypernet_multi); scores / sq_scales: empty, or one per weight
std::vector<Tensor> weight_hypernet_multi(at::TensorList ws, int64_t precision, int64_t block_size, bool symmetric, at::TensorList scores,
                                          int64_t K, int64_t M, at::TensorList sq_scales, OptDtype out_dtype) {
  std::vector<Tensor> outs, wcs, scs, sqs;
  if (ws.empty()) return outs;
  const bool masked = !scores.empty() && M != 0;
  TORCH_CHECK(!masked || scores.size() == ws.size(), "weight_hypernet_multi: one score per weight");
  TORCH_CHECK(sq_scales.empty() || sq_scales.size() == ws.size(), "weight_hypernet_multi: one scale per weight, or none");
  std::vector<dmxq_hypernet_desc> d(ws.size());
  for (size_t i = 0; i < ws.size(); i++) {
    wcs.push_back(prep(ws[i], "weight_hypernet_multi"));
    TORCH_CHECK(wcs[i].scalar_type() == wcs[0].scalar_type() && wcs[i].device() == wcs[0].device(),
                "weight_hypernet_multi: all weights must share one dtype and one device");
    const int64_t L = wcs[i].dim() ? wcs[i].size(-1) : 1;
    const int64_t rows = L ? wcs[i].numel() / L : 0;
    if (masked) {
      scs.push_back(prep(scores[i], "weight_hypernet_multi"));
      TORCH_CHECK(scs[i].scalar_type() == scs[0].scalar_type(), "weight_hypernet_multi: all scores must share one dtype");
      TORCH_CHECK_NOT_IMPLEMENTED(scs[i].sizes() == wcs[i].sizes(), "weight_hypernet_multi: score and weight shapes differ");
    }
    if (!sq_scales.empty()) {
      sqs.push_back(sq_scales[i].detach().to(wcs[i].device(), at::kFloat).contiguous());
      TORCH_CHECK_NOT_IMPLEMENTED(sqs[i].numel() == L, "weight_hypernet_multi: scale length differs from the channel count");
    }
    const at::ScalarType od = out_dtype.value_or(masked ? at::promote_types(wcs[i].scalar_type(), scs[i].scalar_type()) : wcs[i].scalar_type());
    outs.push_back(empty_like_shape(wcs[i], od));
    d[i] = dmxq_hypernet_desc{wcs[i].data_ptr(), masked ? scs[i].data_ptr() : nullptr,
                              sqs.empty() ? nullptr : (const float*)sqs[i].data_ptr(), outs[i].data_ptr(), rows, L};
  }
  Launch l(wcs[0]);
  check(dmxq_weight_hypernet_multi(d.data(), (int64_t)d.size(), dt_code(wcs[0].scalar_type()), masked ? dt_code(scs[0].scalar_type()) : 0,
                                   (int)K, masked ? (int)M : 0, dt_code(outs[0].scalar_type()), block_size, (int)precision, symmetric,
                                   l.stream), "dmxq_weight_hypernet_multi");
  return outs;
}
std::vector<Tensor> weight_hypernet_multi_meta(at::TensorList ws, int64_t, int64_t, bool, at::TensorList scores, int64_t, int64_t M,
                                               at::TensorList, OptDtype out_dtype) {
  std::vector<Tensor> outs;
  const bool masked = !scores.empty() && M != 0;
  for (size_t i = 0; i < ws.size(); i++)
    outs.push_back(empty_like_shape(ws[i], out_dtype.value_or(masked ? at::promote_types(ws[i].scalar_type(), scores[i].scalar_type()) : ws[i].scalar_type())));
  return outs;
}

Tensor input_hypernet(const Tensor& x, const Tensor& sq_scale, int64_t precision, int64_t block_size, bool symmetric) {
  const Tensor xc = prep(x, "input_hypernet");
  const int64_t L = xc.dim() ? xc.size(-1) : 1;
  const int64_t rows = L ? xc.numel() / L : 0;
  const Tensor sq = sq_scale.detach().to(xc.device(), at::kFloat).contiguous();
  TORCH_CHECK_NOT_IMPLEMENTED(sq.numel() == L, "input_hypernet: scale length differs from the channel count");
  Tensor out = empty_like_shape(xc, at::kFloat);
  Launch l(xc);
  check(dmxq_input_hypernet(xc.data_ptr(), dt_code(xc.scalar_type()), (const float*)sq.data_ptr(), out.data_ptr(), dt_code(at::kFloat), rows,
                            L, block_size, (int)precision, symmetric, l.stream), "dmxq_input_hypernet");
  return out;
}
Tensor input_hypernet_meta(const Tensor& x, const Tensor&, int64_t, int64_t, bool) { return empty_like_shape(x, at::kFloat); }

// a cast as [man_bits, exp_bits, exp_bias, flush_subnormal]; empty = SAME
static const dmxq_float_fmt* fmt_of(at::IntArrayRef v, dmxq_float_fmt* slot) {
  if (v.empty()) return nullptr;
  TORCH_CHECK(v.size() == 4, "binary_cast: a cast is [man_bits, exp_bits, exp_bias, flush_subnormal]");
  *slot = dmxq_float_fmt{(int)v[0], (int)v[1], (int)v[2], (int)v[3]};
  return slot;
}
// bfp_block > 0: dmxq_binary_cast_bfp / dmxq_relu_cast_bfp (the consumer's BFP input cast along the last dim in the same launch)
Tensor binary_cast(const Tensor& a, const Tensor& b, int64_t op, at::IntArrayRef cast_a, at::IntArrayRef cast_b, at::IntArrayRef cast_out,
                   int64_t bfp_block, int64_t bfp_precision) {
  const Tensor ac = prep(a, "binary_cast"), bc = prep(b, "binary_cast");
  TORCH_CHECK_NOT_IMPLEMENTED(ac.sizes() == bc.sizes() && ac.scalar_type() == bc.scalar_type() && ac.device() == bc.device(),
                              "binary_cast: operands must share shape, dtype and device (no broadcasting)");
  Tensor out = empty_like_shape(ac, ac.scalar_type());
  dmxq_float_fmt fa, fb, fo;
  Launch l(ac);
  if (bfp_block > 0) {
    TORCH_CHECK_NOT_IMPLEMENTED(ac.dim() >= 1 && ac.numel() > 0, "binary_cast: the BFP cast needs a last dim");
    check(dmxq_binary_cast_bfp(ac.data_ptr(), bc.data_ptr(), out.data_ptr(), dt_code(ac.scalar_type()), ac.numel(), (int)op, fmt_of(cast_a, &fa),
                               fmt_of(cast_b, &fb), fmt_of(cast_out, &fo), ac.size(-1), bfp_block, (int)bfp_precision, l.stream), "dmxq_binary_cast_bfp");
    return out;
  }
  check(dmxq_binary_cast(ac.data_ptr(), bc.data_ptr(), out.data_ptr(), dt_code(ac.scalar_type()), ac.numel(), (int)op, fmt_of(cast_a, &fa),
                         fmt_of(cast_b, &fb), fmt_of(cast_out, &fo), l.stream), "dmxq_binary_cast");
  return out;
}
Tensor binary_cast_meta(const Tensor& a, const Tensor&, int64_t, at::IntArrayRef, at::IntArrayRef, at::IntArrayRef, int64_t, int64_t) {
  return empty_like_shape(a, a.scalar_type());
}

Tensor relu_cast(const Tensor& x, at::IntArrayRef cast_in, at::IntArrayRef cast_out, int64_t bfp_block, int64_t bfp_precision) {
  const Tensor xc = prep(x, "relu_cast");
  Tensor out = empty_like_shape(xc, xc.scalar_type());
  dmxq_float_fmt fi, fo;
  Launch l(xc);
  if (bfp_block > 0) {
    TORCH_CHECK_NOT_IMPLEMENTED(xc.dim() >= 1 && xc.numel() > 0, "relu_cast: the BFP cast needs a last dim");
    check(dmxq_relu_cast_bfp(xc.data_ptr(), out.data_ptr(), dt_code(xc.scalar_type()), xc.numel(), fmt_of(cast_in, &fi), fmt_of(cast_out, &fo),
                             xc.size(-1), bfp_block, (int)bfp_precision, l.stream), "dmxq_relu_cast_bfp");
    return out;
  }
  check(dmxq_relu_cast(xc.data_ptr(), out.data_ptr(), dt_code(xc.scalar_type()), xc.numel(), fmt_of(cast_in, &fi), fmt_of(cast_out, &fo), l.stream),
        "dmxq_relu_cast");
  return out;
}
Tensor relu_cast_meta(const Tensor& x, at::IntArrayRef, at::IntArrayRef, int64_t, int64_t) { return empty_like_shape(x, x.scalar_type()); }

Tensor sbfp_qdq(const Tensor& x, int64_t precision, int64_t block_size, int64_t sman, int64_t sexp, int64_t sbias, bool sflush,
                bool clamp, bool symmetric, int64_t block_dim, OptDtype out_dtype) {
  const Tensor xc = prep(x, "sbfp_qdq");
  Tensor out = empty_like_shape(xc, out_dtype);
  const Split3 s = split3(xc, block_dim);
  Launch l(xc);
  check(dmxq_sbfp_qdq(xc.data_ptr(), out.data_ptr(), dt_code(xc.scalar_type()), dt_code(out.scalar_type()), s.outer, s.L, s.inner,
                      block_size, (int)precision, clamp, symmetric, (int)sman, (int)sexp, (int)sbias, sflush, l.stream), "dmxq_sbfp_qdq");
  return out;
}
Tensor sbfp_qdq_meta(const Tensor& x, int64_t, int64_t, int64_t, int64_t, int64_t, bool, bool, bool, int64_t, OptDtype out_dtype) {
  return empty_like_shape(x, out_dtype);
}

Tensor mxfp_qdq(const Tensor& x, int64_t man, int64_t exp, int64_t block_size, int64_t block_dim, OptDtype out_dtype) {
  const Tensor xc = prep(x, "mxfp_qdq");
  Tensor out = empty_like_shape(xc, out_dtype);
  const Split3 s = split3(xc, block_dim);
  Launch l(xc);
  check(dmxq_mxfp_qdq(xc.data_ptr(), out.data_ptr(), dt_code(xc.scalar_type()), dt_code(out.scalar_type()), s.outer, s.L, s.inner,
                      block_size, (int)man, (int)exp, l.stream), "dmxq_mxfp_qdq");
  return out;
}
Tensor mxfp_qdq_meta(const Tensor& x, int64_t, int64_t, int64_t, int64_t, OptDtype out_dtype) { return empty_like_shape(x, out_dtype); }

// ------------------------------------------------------------------------------------------------ element formats
Tensor float_qdq(const Tensor& x, int64_t man, int64_t exp, int64_t bias, bool flush, bool unsigned_abs, int64_t rounding,
                 OptDtype out_dtype, int64_t seed) {
  const Tensor xc = prep(x, "float_qdq");
  Tensor out = empty_like_shape(xc, out_dtype);
  Launch l(xc);
  check(dmxq_float_qdq(xc.data_ptr(), out.data_ptr(), dt_code(xc.scalar_type()), dt_code(out.scalar_type()), xc.numel(), (int)man,
                       (int)exp, (int)bias, flush, unsigned_abs, (int)rounding, (uint64_t)seed, l.stream), "dmxq_float_qdq");
  return out;
}
Tensor float_qdq_meta(const Tensor& x, int64_t, int64_t, int64_t, bool, bool, int64_t, OptDtype out_dtype, int64_t) {
  return empty_like_shape(x, out_dtype);
}

std::vector<Tensor> float_qdq_multi(at::TensorList xs, int64_t man, int64_t exp, int64_t bias, bool flush, bool unsigned_abs, int64_t rounding,
                                    OptDtype out_dtype, int64_t seed) {
  std::vector<Tensor> outs, ins;
  if (xs.empty()) return outs;
  std::vector<dmxq_tensor_desc> d(xs.size());
  for (size_t i = 0; i < xs.size(); i++) {
    ins.push_back(prep(xs[i], "float_qdq_multi"));
    TORCH_CHECK(ins[i].scalar_type() == ins[0].scalar_type() && ins[i].device() == ins[0].device(),
                "float_qdq_multi: all tensors must share one dtype and one device");
    outs.push_back(empty_like_shape(ins[i], out_dtype));
    d[i] = dmxq_tensor_desc{ins[i].data_ptr(), outs[i].data_ptr(), 1, ins[i].numel(), 1};
  }
  Launch l(ins[0]);
  check(dmxq_float_qdq_multi(d.data(), (int64_t)d.size(), dt_code(ins[0].scalar_type()), dt_code(outs[0].scalar_type()), (int)man, (int)exp,
                             (int)bias, flush, unsigned_abs, (int)rounding, (uint64_t)seed, l.stream), "dmxq_float_qdq_multi");
  return outs;
}
std::vector<Tensor> float_qdq_multi_meta(at::TensorList xs, int64_t, int64_t, int64_t, bool, bool, int64_t, OptDtype out_dtype, int64_t) {
  std::vector<Tensor> outs;
  for (const Tensor& x : xs) outs.push_back(empty_like_shape(x, out_dtype));
  return outs;
}

std::tuple<std::vector<Tensor>, std::vector<Tensor>> fixed_float_qdq_multi(at::TensorList xs, int64_t precision, int64_t fraction, bool clamp, bool symmetric,
                                                                           int64_t rounding, at::TensorList scales, at::TensorList zero_points, int64_t group_size,
                                                                           at::TensorList fs, int64_t man, int64_t exp, int64_t bias, bool flush, bool unsigned_abs,
                                                                           int64_t rounding_float, int64_t seed) {
  std::vector<Tensor> outs, ins, scs, zps, fouts, fins;
  TORCH_CHECK(!xs.empty() && !fs.empty(), "fixed_float_qdq_multi: both tensor lists must be non-empty (use the single-op multi calls otherwise)");
  TORCH_CHECK(scales.size() == xs.size() && zero_points.size() == xs.size(), "fixed_float_qdq_multi: one scale and one zero_point tensor per input");
  std::vector<dmxq_affine_desc> d(xs.size());
  std::vector<dmxq_tensor_desc> fd(fs.size());
  for (size_t i = 0; i < xs.size(); i++) {
    ins.push_back(prep(xs[i], "fixed_float_qdq_multi"));
    TORCH_CHECK(ins[i].scalar_type() == ins[0].scalar_type() && ins[i].device() == ins[0].device(), "fixed_float_qdq_multi: all tensors must share one dtype and one device");
    outs.push_back(empty_like_shape(ins[i], c10::nullopt));
    scs.push_back(scales[i].detach().to(ins[i].device(), at::kFloat).contiguous());
    zps.push_back(zero_points[i].detach().to(ins[i].device(), at::kLong).contiguous());
    const int64_t gs = std::max<int64_t>(group_size, 1);
    Split3 s = ins[i].dim() > 0 ? split3(ins[i], 0) : Split3{1, 1, 1};
    const int64_t need = (group_size > 0 || scs[i].numel() != 1) ? (s.L + gs - 1) / gs : 1;
    TORCH_CHECK_VALUE(scs[i].numel() >= need && zps[i].numel() >= need, "fixed_float_qdq_multi: tensor ", i, " needs ", need, " scale/zero_point entries, got ",
                      scs[i].numel(), "/", zps[i].numel());
    if (need == 1) s = Split3{1, 1, ins[i].numel()};
    d[i] = dmxq_affine_desc{ins[i].data_ptr(), outs[i].data_ptr(), (const float*)scs[i].data_ptr(), (const int64_t*)zps[i].data_ptr(), s.outer, s.L, s.inner};
  }
  for (size_t i = 0; i < fs.size(); i++) {
    fins.push_back(prep(fs[i], "fixed_float_qdq_multi"));
    TORCH_CHECK(fins[i].scalar_type() == ins[0].scalar_type() && fins[i].device() == ins[0].device(), "fixed_float_qdq_multi: all tensors must share one dtype and one device");
    fouts.push_back(empty_like_shape(fins[i], c10::nullopt));
    fd[i] = dmxq_tensor_desc{fins[i].data_ptr(), fouts[i].data_ptr(), 1, fins[i].numel(), 1};
  }
  Launch l(ins[0]);
  check(dmxq_fixed_float_qdq_multi(d.data(), (int64_t)d.size(), (int)precision, (int)fraction, clamp, symmetric, (int)rounding, std::max<int64_t>(group_size, 1),
                                   fd.data(), (int64_t)fd.size(), (int)man, (int)exp, (int)bias, flush, unsigned_abs, (int)rounding_float,
                                   dt_code(ins[0].scalar_type()), (uint64_t)seed, l.stream), "dmxq_fixed_float_qdq_multi");
  return {outs, fouts};
}
std::tuple<std::vector<Tensor>, std::vector<Tensor>> fixed_float_qdq_multi_meta(at::TensorList xs, int64_t, int64_t, bool, bool, int64_t, at::TensorList, at::TensorList,
                                                                                int64_t, at::TensorList fs, int64_t, int64_t, int64_t, bool, bool, int64_t, int64_t) {
  std::vector<Tensor> outs, fouts;
  for (const Tensor& x : xs) outs.push_back(empty_like_shape(x, c10::nullopt));
  for (const Tensor& x : fs) fouts.push_back(empty_like_shape(x, c10::nullopt));
  return {outs, fouts};
}

Tensor fixed_qdq(const Tensor& x, int64_t precision, int64_t fraction, bool clamp, bool symmetric, int64_t rounding,
                 const OptTensor& scale, const OptTensor& zero_point, c10::optional<int64_t> ch_axis,
                 c10::optional<int64_t> group_size, OptDtype out_dtype, int64_t seed) {
  const Tensor xc = prep(x, "fixed_qdq");
  Tensor out = empty_like_shape(xc, out_dtype);
  Tensor sc, zp;
  Split3 s{1, 1, xc.numel()};
  int64_t gs = 1;
  if (scale.has_value() && scale->defined()) {
    TORCH_CHECK(zero_point.has_value() && zero_point->defined(), "fixed_qdq: scale without zero_point");
    sc = scale->detach().to(xc.device(), at::kFloat).contiguous();
    zp = zero_point->detach().to(xc.device(), at::kLong).contiguous();
    int64_t need = 1;
    if (ch_axis.has_value() && xc.dim() > 0) {
      s = split3(xc, *ch_axis);
      gs = group_size.value_or(1);
      if (gs < 1) gs = 1;
      need = (s.L + gs - 1) / gs;
    }
    TORCH_CHECK_VALUE(sc.numel() >= need && zp.numel() >= need, "fixed_qdq: need ", need, " scale/zero_point entries, got ",
                      sc.numel(), "/", zp.numel());
  }
  Launch l(xc);
  check(dmxq_fixed_qdq(xc.data_ptr(), out.data_ptr(), dt_code(xc.scalar_type()), dt_code(out.scalar_type()), s.outer, s.L, s.inner,
                       (int)precision, (int)fraction, clamp, symmetric, (int)rounding, sc.defined() ? (const float*)sc.data_ptr() : nullptr,
                       zp.defined() ? (const int64_t*)zp.data_ptr() : nullptr, gs, (uint64_t)seed, l.stream), "dmxq_fixed_qdq");
  return out;
}
Tensor fixed_qdq_meta(const Tensor& x, int64_t, int64_t, bool, bool, int64_t, const OptTensor&, const OptTensor&, c10::optional<int64_t>,
                      c10::optional<int64_t>, OptDtype out_dtype, int64_t) {
  return empty_like_shape(x, out_dtype);
}

std::vector<Tensor> fixed_qdq_multi(at::TensorList xs, int64_t precision, int64_t fraction, bool clamp, bool symmetric, int64_t rounding,
                                    at::TensorList scales, at::TensorList zero_points, int64_t group_size, OptDtype out_dtype, int64_t seed) {
  // every tensor is [C, inner] (or any shape with ONE scale: C == 1) with its own scale / zero-point vectors, channels along dim 0
  std::vector<Tensor> outs, ins, scs, zps;
  if (xs.empty()) return outs;
  TORCH_CHECK(scales.size() == xs.size() && zero_points.size() == xs.size(), "fixed_qdq_multi: one scale and one zero_point tensor per input");
  std::vector<dmxq_affine_desc> d(xs.size());
  for (size_t i = 0; i < xs.size(); i++) {
    ins.push_back(prep(xs[i], "fixed_qdq_multi"));
    TORCH_CHECK(ins[i].scalar_type() == ins[0].scalar_type() && ins[i].device() == ins[0].device(),
                "fixed_qdq_multi: all tensors must share one dtype and one device");
    outs.push_back(empty_like_shape(ins[i], out_dtype));
    scs.push_back(scales[i].detach().to(ins[i].device(), at::kFloat).contiguous());
    zps.push_back(zero_points[i].detach().to(ins[i].device(), at::kLong).contiguous());
    // group_size <= 0: none asked for (a one-entry scale then means per-tensor).  With a group_size a weight needs
    // ceil(C / group_size) entries exactly like fixed_qdq(ch_axis = 0, group_size): an uncalibrated cast (scale = [1.0]) raises
    const int64_t gs = std::max<int64_t>(group_size, 1);
    Split3 s = ins[i].dim() > 0 ? split3(ins[i], 0) : Split3{1, 1, 1};
    const int64_t need = (group_size > 0 || scs[i].numel() != 1) ? (s.L + gs - 1) / gs : 1;
    TORCH_CHECK_VALUE(scs[i].numel() >= need && zps[i].numel() >= need, "fixed_qdq_multi: tensor ", i, " needs ", need,
                      " scale/zero_point entries, got ", scs[i].numel(), "/", zps[i].numel());
    if (need == 1) s = Split3{1, 1, ins[i].numel()};
    d[i] = dmxq_affine_desc{ins[i].data_ptr(), outs[i].data_ptr(), (const float*)scs[i].data_ptr(), (const int64_t*)zps[i].data_ptr(), s.outer, s.L, s.inner};
  }
  Launch l(ins[0]);
  check(dmxq_fixed_qdq_multi(d.data(), (int64_t)d.size(), dt_code(ins[0].scalar_type()), dt_code(outs[0].scalar_type()), (int)precision,
                             (int)fraction, clamp, symmetric, (int)rounding, std::max<int64_t>(group_size, 1), (uint64_t)seed, l.stream),
        "dmxq_fixed_qdq_multi");
  return outs;
}
std::vector<Tensor> fixed_qdq_multi_meta(at::TensorList xs, int64_t, int64_t, bool, bool, int64_t, at::TensorList, at::TensorList, int64_t,
                                         OptDtype out_dtype, int64_t) {
  std::vector<Tensor> outs;
  for (const Tensor& x : xs) outs.push_back(empty_like_shape(x, out_dtype));
  return outs;
}

// ------------------------------------------------------------------------------------------------ sparsity
// (mask, y): an output that was not requested comes back as an empty 1-d tensor
Tensor none_like(const Tensor& x) { return at::empty({0}, x.options()); }

std::tuple<Tensor, Tensor> nm_mask(const Tensor& score, const OptTensor& x, int64_t K, int64_t M, int64_t block_dim, bool want_mask,
                                   bool want_y, OptDtype mask_dtype, OptDtype y_dtype) {
  const Tensor sc = prep(score, "nm_mask");
  TORCH_CHECK(sc.dim() > 0 && M > 0 && sc.size(block_dim) % M == 0, "score has size ", sc.sizes(), " at dimension ", block_dim,
              ", not a multiple of block size ", M);
  const Split3 s = split3(sc, block_dim);
  Tensor xc;
  if (want_y) {
    TORCH_CHECK(x.has_value() && x->defined(), "nm_sparsify: x required");
    xc = prep(*x, "nm_sparsify");
    if (xc.sizes() != sc.sizes()) xc = xc.expand(sc.sizes()).contiguous();
  }
  Tensor mask = want_mask ? empty_like_shape(sc, mask_dtype) : none_like(sc);
  Tensor y = want_y ? empty_like_shape(sc, y_dtype.value_or(at::promote_types(xc.scalar_type(), sc.scalar_type()))) : none_like(sc);
  Launch l(sc);
  check(dmxq_nm_mask(sc.data_ptr(), dt_code(sc.scalar_type()), want_y ? xc.data_ptr() : nullptr, want_y ? dt_code(xc.scalar_type()) : 0,
                     want_mask ? mask.data_ptr() : nullptr, want_mask ? dt_code(mask.scalar_type()) : 0,
                     want_y ? y.data_ptr() : nullptr, want_y ? dt_code(y.scalar_type()) : 0, s.outer, s.L, s.inner, (int)K, (int)M,
                     l.stream), "dmxq_nm_mask");
  return {mask, y};
}
std::tuple<Tensor, Tensor> nm_mask_meta(const Tensor& score, const OptTensor& x, int64_t, int64_t, int64_t, bool want_mask, bool want_y,
                                        OptDtype mask_dtype, OptDtype y_dtype) {
  Tensor mask = want_mask ? empty_like_shape(score, mask_dtype) : none_like(score);
  Tensor y = want_y ? empty_like_shape(score, y_dtype.value_or(at::promote_types(x->scalar_type(), score.scalar_type()))) : none_like(score);
  return {mask, y};
}

std::tuple<Tensor, Tensor> topk_mask(const Tensor& score, const OptTensor& x, int64_t n_zero, bool want_mask, bool want_y,
                                     OptDtype mask_dtype, OptDtype y_dtype) {
  const Tensor sc = prep(score, "topk_mask");
  const int64_t n = sc.numel();
  Tensor xc;
  if (want_y) {
    TORCH_CHECK(x.has_value() && x->defined(), "topk_sparsify: x required");
    xc = prep(*x, "topk_sparsify");
    if (xc.sizes() != sc.sizes()) xc = xc.expand(sc.sizes()).contiguous();
  }
  Tensor mask = want_mask ? empty_like_shape(sc, mask_dtype) : none_like(sc);
  Tensor y = want_y ? empty_like_shape(sc, y_dtype.value_or(at::promote_types(xc.scalar_type(), sc.scalar_type()))) : none_like(sc);
  const int64_t ws_bytes = dmxq_topk_workspace_bytes(n);
  Tensor ws = at::empty({std::max<int64_t>(1, (ws_bytes + 7) / 8)}, sc.options().dtype(at::kLong));
  Launch l(sc);
  check(dmxq_topk_mask(sc.data_ptr(), dt_code(sc.scalar_type()), want_y ? xc.data_ptr() : nullptr, want_y ? dt_code(xc.scalar_type()) : 0,
                       want_mask ? mask.data_ptr() : nullptr, want_mask ? dt_code(mask.scalar_type()) : 0,
                       want_y ? y.data_ptr() : nullptr, want_y ? dt_code(y.scalar_type()) : 0, n, n_zero, ws.data_ptr(), l.stream),
        "dmxq_topk_mask");
  return {mask, y};
}
std::tuple<Tensor, Tensor> topk_mask_meta(const Tensor& score, const OptTensor& x, int64_t, bool want_mask, bool want_y,
                                          OptDtype mask_dtype, OptDtype y_dtype) {
  return nm_mask_meta(score, x, 0, 1, -1, want_mask, want_y, mask_dtype, y_dtype);
}

Tensor bernoulli_mask(const Tensor& score, int64_t seed, OptDtype mask_dtype) {
  const Tensor sc = prep(score, "bernoulli_mask");
  Tensor mask = empty_like_shape(sc, mask_dtype);
  Launch l(sc);
  check(dmxq_bernoulli_mask(sc.data_ptr(), mask.data_ptr(), dt_code(sc.scalar_type()), dt_code(mask.scalar_type()), sc.numel(),
                            (uint64_t)seed, l.stream), "dmxq_bernoulli_mask");
  return mask;
}
Tensor bernoulli_mask_meta(const Tensor& score, int64_t, OptDtype mask_dtype) { return empty_like_shape(score, mask_dtype); }

// ------------------------------------------------------------------------------------------------ calibration
std::tuple<Tensor, Tensor> group_minmax(const Tensor& x, int64_t ch_axis, int64_t group_size) {
  const Tensor xc = prep(x, "group_minmax");
  TORCH_CHECK(group_size >= 1, "group_minmax: group_size must be positive");
  const Split3 s = split3(xc, ch_axis);
  const int64_t G = (s.L + group_size - 1) / group_size;
  Tensor mn = at::empty({G}, xc.options().dtype(at::kFloat)), mx = at::empty({G}, xc.options().dtype(at::kFloat));
  Launch l(xc);
  check(dmxq_group_minmax(xc.data_ptr(), dt_code(xc.scalar_type()), s.outer, s.L, s.inner, group_size, (float*)mn.data_ptr(),
                          (float*)mx.data_ptr(), l.stream), "dmxq_group_minmax");
  return {mn, mx};
}
std::tuple<Tensor, Tensor> group_minmax_meta(const Tensor& x, int64_t ch_axis, int64_t group_size) {
  const Split3 s = split3(x, ch_axis);
  const int64_t G = (s.L + std::max<int64_t>(group_size, 1) - 1) / std::max<int64_t>(group_size, 1);
  return {at::empty({G}, x.options().dtype(at::kFloat)), at::empty({G}, x.options().dtype(at::kFloat))};
}

// running min / max updated in place, one launch (dmxq_group_minmax_accumulate); returns nothing new: mn / mx ARE the state
void group_minmax_accumulate(const Tensor& x, int64_t ch_axis, int64_t group_size, Tensor mn, Tensor mx) {
  const Tensor xc = prep(x, "group_minmax_accumulate");
  const Split3 s = split3(xc, ch_axis);
  const int64_t gs = std::max<int64_t>(group_size, 1), G = (s.L + gs - 1) / gs;
  TORCH_CHECK(mn.is_cuda() && mx.is_cuda() && mn.device() == xc.device() && mx.device() == xc.device() && mn.scalar_type() == at::kFloat &&
              mx.scalar_type() == at::kFloat && mn.is_contiguous() && mx.is_contiguous() && mn.numel() == G && mx.numel() == G,
              "group_minmax_accumulate: running min / max must be contiguous float32 tensors of ", G, " entries on the input's device");
  Launch l(xc);
  check(dmxq_group_minmax_accumulate(xc.data_ptr(), dt_code(xc.scalar_type()), s.outer, s.L, s.inner, gs, (float*)mn.data_ptr(),
                                     (float*)mx.data_ptr(), l.stream), "dmxq_group_minmax_accumulate");
}
void group_minmax_accumulate_meta(const Tensor&, int64_t, int64_t, Tensor, Tensor) {}

std::tuple<Tensor, Tensor> qparams(const Tensor& mn, const Tensor& mx, int64_t qmin, int64_t qmax, bool symmetric) {
  TORCH_CHECK(mn.is_cuda(), "qparams: tensors must be on the GPU (no CPU fallback)");
  const Tensor a = mn.to(at::kFloat).contiguous(), b = mx.to(at::kFloat).contiguous();
  Tensor scale = at::empty_like(a), zp = at::empty(a.sizes(), a.options().dtype(at::kLong));
  Launch l(a);
  check(dmxq_qparams((const float*)a.data_ptr(), (const float*)b.data_ptr(), a.numel(), (int)qmin, (int)qmax, symmetric,
                     (float*)scale.data_ptr(), (int64_t*)zp.data_ptr(), l.stream), "dmxq_qparams");
  return {scale, zp};
}
std::tuple<Tensor, Tensor> qparams_meta(const Tensor& mn, const Tensor&, int64_t, int64_t, bool) {
  return {at::empty(mn.sizes(), mn.options().dtype(at::kFloat)), at::empty(mn.sizes(), mn.options().dtype(at::kLong))};
}

Tensor histc(const Tensor& x, int64_t bins, double lo, double hi) {
  const Tensor xc = prep(x, "histc").reshape({-1});
  Tensor out = at::empty({bins}, xc.options().dtype(at::kFloat));
  Launch l(xc);
  check(dmxq_histc(xc.data_ptr(), dt_code(xc.scalar_type()), xc.numel(), bins, (float)lo, (float)hi, (float*)out.data_ptr(), l.stream),
        "dmxq_histc");
  return out;
}
Tensor histc_meta(const Tensor& x, int64_t bins, double, double) { return at::empty({bins}, x.options().dtype(at::kFloat)); }

Tensor channel_maxabs(const Tensor& x, int64_t ch_axis) {
  const Tensor xc = prep(x, "channel_maxabs");
  const Split3 s = split3(xc, ch_axis);
  Tensor out = at::empty({s.L}, xc.options().dtype(at::kFloat));
  Launch l(xc);
  check(dmxq_channel_maxabs(xc.data_ptr(), dt_code(xc.scalar_type()), s.outer, s.L, s.inner, (float*)out.data_ptr(), l.stream),
        "dmxq_channel_maxabs");
  return out;
}
Tensor channel_maxabs_meta(const Tensor& x, int64_t ch_axis) { return at::empty({split3(x, ch_axis).L}, x.options().dtype(at::kFloat)); }

Tensor smoothquant_scale(const Tensor& a_maxabs, const Tensor& b_maxabs, double alpha, double scale_min) {
  TORCH_CHECK(a_maxabs.is_cuda(), "smoothquant_scale: tensors must be on the GPU (no CPU fallback)");
  const Tensor a = a_maxabs.to(at::kFloat).contiguous(), b = b_maxabs.to(a.device(), at::kFloat).contiguous();
  Tensor out = at::empty_like(a);
  Launch l(a);
  check(dmxq_smoothquant_scale((const float*)a.data_ptr(), (const float*)b.data_ptr(), a.numel(), (float)alpha, (float)scale_min,
                               (float*)out.data_ptr(), l.stream), "dmxq_smoothquant_scale");
  return out;
}
Tensor smoothquant_scale_meta(const Tensor& a, const Tensor&, double, double) { return at::empty(a.sizes(), a.options().dtype(at::kFloat)); }

Tensor scale_channels(const Tensor& x, const Tensor& scale, int64_t ch_axis, bool divide, OptDtype out_dtype) {
  const Tensor xc = prep(x, "scale_channels");
  const Split3 s = split3(xc, ch_axis);
  const Tensor sc = scale.detach().to(xc.device(), at::kFloat).contiguous();
  TORCH_CHECK_VALUE(sc.numel() == s.L, "scale_channels: scale has ", sc.numel(), " entries for ", s.L, " channels");
  Tensor out = empty_like_shape(xc, out_dtype);
  Launch l(xc);
  check(dmxq_scale_channels(xc.data_ptr(), out.data_ptr(), dt_code(xc.scalar_type()), dt_code(out.scalar_type()), s.outer, s.L, s.inner,
                            (const float*)sc.data_ptr(), divide, l.stream), "dmxq_scale_channels");
  return out;
}
Tensor scale_channels_meta(const Tensor& x, const Tensor&, int64_t, bool, OptDtype out_dtype) { return empty_like_shape(x, out_dtype); }

// ------------------------------------------------------------------------------------------------ approximator slot
// kind: the dmxq_unary_kind of include/dmxq.h (exact gelu / tanh gelu / silu / quick_gelu / exp / experimental silu)
Tensor unary(const Tensor& x, int64_t kind, double param, OptDtype out_dtype) {
  const Tensor xc = prep(x, "unary");
  Tensor out = empty_like_shape(xc, out_dtype);
  Launch l(xc);
  check(dmxq_unary(xc.data_ptr(), out.data_ptr(), dt_code(xc.scalar_type()), dt_code(out.scalar_type()), xc.numel(), (int)kind, (float)param,
                   l.stream), "dmxq_unary");
  return out;
}
Tensor unary_meta(const Tensor& x, int64_t, double, OptDtype out_dtype) { return empty_like_shape(x, out_dtype); }

// x: [B, n1, n2, D]; cos / sin: [B, S, D] with S = n2 (unsqueeze_dim = 1) or n1 (unsqueeze_dim = 2)
Tensor rope(const Tensor& x, const Tensor& cos_t, const Tensor& sin_t, int64_t unsqueeze_dim) {
  const Tensor xc = prep(x, "rope");
  TORCH_CHECK_NOT_IMPLEMENTED(xc.dim() == 4 && cos_t.dim() == 3 && sin_t.dim() == 3 && (unsqueeze_dim == 1 || unsqueeze_dim == 2),
                              "rope: expects x [B, n1, n2, D], cos / sin [B, S, D], unsqueeze_dim 1 or 2");
  TORCH_CHECK_NOT_IMPLEMENTED(cos_t.scalar_type() == xc.scalar_type() && sin_t.scalar_type() == xc.scalar_type(),
                              "rope: x, cos and sin must share one dtype (torch's promotion rules are not reproduced)");
  const Tensor c = prep(cos_t, "rope"), sn = prep(sin_t, "rope");
  const int64_t B = xc.size(0), n1 = xc.size(1), n2 = xc.size(2), D = xc.size(3), S = unsqueeze_dim == 1 ? n2 : n1;
  TORCH_CHECK_NOT_IMPLEMENTED(c.size(0) == B && c.size(1) == S && c.size(2) == D && sn.sizes() == c.sizes(), "rope: cos / sin shape");
  Tensor out = at::empty_like(xc);
  Launch l(xc);
  check(dmxq_rope(xc.data_ptr(), c.data_ptr(), sn.data_ptr(), out.data_ptr(), dt_code(xc.scalar_type()), B, n1, n2, D, unsqueeze_dim == 1,
                  l.stream), "dmxq_rope");
  return out;
}
Tensor rope_cast(const Tensor& x, const Tensor& cos_t, const Tensor& sin_t, int64_t unsqueeze_dim, at::IntArrayRef cast_x, at::IntArrayRef cast_cos,
                 at::IntArrayRef cast_sin, at::IntArrayRef cast_out) {
  const Tensor xc = prep(x, "rope_cast");
  TORCH_CHECK_NOT_IMPLEMENTED(xc.dim() == 4 && cos_t.dim() == 3 && sin_t.dim() == 3 && (unsqueeze_dim == 1 || unsqueeze_dim == 2),
                              "rope_cast: expects x [B, n1, n2, D], cos / sin [B, S, D], unsqueeze_dim 1 or 2");
  TORCH_CHECK_NOT_IMPLEMENTED(cos_t.scalar_type() == xc.scalar_type() && sin_t.scalar_type() == xc.scalar_type(), "rope_cast: one dtype");
  const Tensor c = prep(cos_t, "rope_cast"), sn = prep(sin_t, "rope_cast");
  const int64_t B = xc.size(0), n1 = xc.size(1), n2 = xc.size(2), D = xc.size(3), S = unsqueeze_dim == 1 ? n2 : n1;
  TORCH_CHECK_NOT_IMPLEMENTED(c.size(0) == B && c.size(1) == S && c.size(2) == D && sn.sizes() == c.sizes(), "rope_cast: cos / sin shape");
  Tensor out = at::empty_like(xc);
  dmxq_float_fmt fx, fc, fs, fo;
  Launch l(xc);
  check(dmxq_rope_cast(xc.data_ptr(), c.data_ptr(), sn.data_ptr(), out.data_ptr(), dt_code(xc.scalar_type()), B, n1, n2, D, unsqueeze_dim == 1,
                       fmt_of(cast_x, &fx), fmt_of(cast_cos, &fc), fmt_of(cast_sin, &fs), fmt_of(cast_out, &fo), l.stream), "dmxq_rope_cast");
  return out;
}
Tensor rope_cast_meta(const Tensor& x, const Tensor&, const Tensor&, int64_t, at::IntArrayRef, at::IntArrayRef, at::IntArrayRef, at::IntArrayRef) {
  return at::empty_like(x, x.options().memory_format(at::MemoryFormat::Contiguous));
}
Tensor rope_meta(const Tensor& x, const Tensor&, const Tensor&, int64_t) { return at::empty_like(x, x.options().memory_format(at::MemoryFormat::Contiguous)); }

Tensor softmax(const Tensor& x, double clamp_min, OptDtype out_dtype) {  // over the contiguous last dim
  const Tensor xc = prep(x, "softmax");
  const int64_t cols = xc.dim() ? xc.size(-1) : 1;
  const int64_t rows = cols ? xc.numel() / cols : 0;
  Tensor out = empty_like_shape(xc, out_dtype);
  Launch l(xc);
  check(dmxq_softmax(xc.data_ptr(), out.data_ptr(), dt_code(xc.scalar_type()), dt_code(out.scalar_type()), rows, cols, (float)clamp_min,
                     l.stream), "dmxq_softmax");
  return out;
}
Tensor softmax_meta(const Tensor& x, double, OptDtype out_dtype) { return empty_like_shape(x, out_dtype); }

// norm: 0 = LayerNorm (mean / variance), 1 = RMSNorm; over the trailing `cols` elements
Tensor norm(const Tensor& x, int64_t cols, const OptTensor& weight, const OptTensor& bias, double eps, int64_t kind, OptDtype out_dtype) {
  const Tensor xc = prep(x, "norm");
  const int64_t rows = cols ? xc.numel() / cols : 0;
  Tensor w, b;
  if (weight.has_value() && weight->defined()) w = weight->detach().contiguous();
  if (bias.has_value() && bias->defined()) b = bias->detach().contiguous();
  if (w.defined() && b.defined() && w.scalar_type() != b.scalar_type()) b = b.to(w.scalar_type());
  const int wb = w.defined() ? dt_code(w.scalar_type()) : (b.defined() ? dt_code(b.scalar_type()) : 0);
  Tensor out = empty_like_shape(xc, out_dtype);
  Launch l(xc);
  if (kind == 0)
    check(dmxq_layernorm(xc.data_ptr(), out.data_ptr(), dt_code(xc.scalar_type()), dt_code(out.scalar_type()), rows, cols,
                         w.defined() ? w.data_ptr() : nullptr, b.defined() ? b.data_ptr() : nullptr, wb, (float)eps, l.stream), "dmxq_layernorm");
  else
    check(dmxq_rmsnorm(xc.data_ptr(), out.data_ptr(), dt_code(xc.scalar_type()), dt_code(out.scalar_type()), rows, cols,
                       w.defined() ? w.data_ptr() : nullptr, wb, (float)eps, l.stream), "dmxq_rmsnorm");
  return out;
}
Tensor norm_meta(const Tensor& x, int64_t, const OptTensor&, const OptTensor&, double, int64_t, OptDtype out_dtype) {
  return empty_like_shape(x, out_dtype);
}

// ---- an activation / normalisation module in one launch: cast_out(f(cast_in(x)))  (include/dmxq.h dmxq_unary_cast ...)
Tensor unary_cast(const Tensor& x, int64_t kind, double param, at::IntArrayRef cast_in, at::IntArrayRef cast_out) {
  const Tensor xc = prep(x, "unary_cast");
  Tensor out = empty_like_shape(xc, xc.scalar_type());
  dmxq_float_fmt fi, fo;
  Launch l(xc);
  check(dmxq_unary_cast(xc.data_ptr(), out.data_ptr(), dt_code(xc.scalar_type()), xc.numel(), (int)kind, (float)param, fmt_of(cast_in, &fi),
                        fmt_of(cast_out, &fo), l.stream), "dmxq_unary_cast");
  return out;
}
Tensor unary_cast_meta(const Tensor& x, int64_t, double, at::IntArrayRef, at::IntArrayRef) { return empty_like_shape(x, x.scalar_type()); }

// the 65,536-entry table of a unary module on a 16-bit dtype (dmxq_unary_cast_table) and its application (dmxq_lut16_apply)
Tensor unary_cast_table(const Tensor& like, int64_t kind, double param, at::IntArrayRef cast_in, at::IntArrayRef cast_out) {
  TORCH_CHECK(like.is_cuda() && (like.scalar_type() == at::kBFloat16 || like.scalar_type() == at::kHalf),
              "unary_cast_table: a bfloat16 / float16 GPU tensor names the dtype and the device");
  Tensor table = at::empty({65536}, like.options().dtype(at::kShort));
  dmxq_float_fmt fi, fo;
  Launch l(like);
  check(dmxq_unary_cast_table(dt_code(like.scalar_type()), (int)kind, (float)param, fmt_of(cast_in, &fi), fmt_of(cast_out, &fo), table.data_ptr(),
                              l.stream), "dmxq_unary_cast_table");
  return table;
}
Tensor unary_cast_table_meta(const Tensor& like, int64_t, double, at::IntArrayRef, at::IntArrayRef) {
  return at::empty({65536}, like.options().dtype(at::kShort));
}
Tensor lut16_apply(const Tensor& x, const Tensor& table) {
  const Tensor xc = prep(x, "lut16_apply");
  TORCH_CHECK(xc.element_size() == 2 && table.is_cuda() && table.device() == xc.device() && table.numel() == 65536 && table.element_size() == 2 &&
              table.is_contiguous(), "lut16_apply: a 16-bit tensor and a 65536-entry 16-bit table on its device");
  Tensor out = empty_like_shape(xc, xc.scalar_type());
  Launch l(xc);
  check(dmxq_lut16_apply(xc.data_ptr(), out.data_ptr(), xc.numel(), table.data_ptr(), l.stream), "dmxq_lut16_apply");
  return out;
}
Tensor lut16_apply_meta(const Tensor& x, const Tensor&) { return empty_like_shape(x, x.scalar_type()); }

Tensor softmax_cast(const Tensor& x, double clamp_min, at::IntArrayRef cast_in, at::IntArrayRef cast_out, int64_t bfp_block,
                    int64_t bfp_precision) {  // over the contiguous last dim; bfp_block > 0: the consumer's BFP input cast applied too
  const Tensor xc = prep(x, "softmax_cast");
  const int64_t cols = xc.dim() ? xc.size(-1) : 1;
  const int64_t rows = cols ? xc.numel() / cols : 0;
  Tensor out = empty_like_shape(xc, xc.scalar_type());
  dmxq_float_fmt fi, fo;
  Launch l(xc);
  if (bfp_block > 0)
    check(dmxq_softmax_cast_bfp(xc.data_ptr(), out.data_ptr(), dt_code(xc.scalar_type()), rows, cols, (float)clamp_min, fmt_of(cast_in, &fi),
                                fmt_of(cast_out, &fo), bfp_block, (int)bfp_precision, l.stream), "dmxq_softmax_cast_bfp");
  else
    check(dmxq_softmax_cast(xc.data_ptr(), out.data_ptr(), dt_code(xc.scalar_type()), rows, cols, (float)clamp_min, fmt_of(cast_in, &fi),
                            fmt_of(cast_out, &fo), l.stream), "dmxq_softmax_cast");
  return out;
}
Tensor softmax_cast_meta(const Tensor& x, double, at::IntArrayRef, at::IntArrayRef, int64_t, int64_t) { return empty_like_shape(x, x.scalar_type()); }

Tensor norm_cast(const Tensor& x, int64_t cols, const OptTensor& weight, const OptTensor& bias, double eps, int64_t kind, at::IntArrayRef cast_in,
                 at::IntArrayRef cast_out, int64_t bfp_block, int64_t bfp_precision) {  // bfp_block > 0: the consumers' BFP input cast too
  const Tensor xc = prep(x, "norm_cast");
  const int64_t rows = cols ? xc.numel() / cols : 0;
  Tensor w, b;
  if (weight.has_value() && weight->defined()) w = weight->detach().contiguous();
  if (bias.has_value() && bias->defined()) b = bias->detach().contiguous();
  TORCH_CHECK_NOT_IMPLEMENTED((!w.defined() || (w.scalar_type() == xc.scalar_type() && w.device() == xc.device() && w.numel() == cols)) &&
                              (!b.defined() || (b.scalar_type() == xc.scalar_type() && b.device() == xc.device() && b.numel() == cols)),
                              "norm_cast: weight / bias must be in the row dtype, on the row's device, one per column");
  Tensor out = empty_like_shape(xc, xc.scalar_type());
  dmxq_float_fmt fi, fo;
  Launch l(xc);
  if (bfp_block > 0 && kind == 0)
    check(dmxq_layernorm_cast_bfp(xc.data_ptr(), out.data_ptr(), dt_code(xc.scalar_type()), rows, cols, w.defined() ? w.data_ptr() : nullptr,
                                  b.defined() ? b.data_ptr() : nullptr, (float)eps, fmt_of(cast_in, &fi), fmt_of(cast_out, &fo), bfp_block,
                                  (int)bfp_precision, l.stream), "dmxq_layernorm_cast_bfp");
  else if (bfp_block > 0)
    check(dmxq_rmsnorm_cast_bfp(xc.data_ptr(), out.data_ptr(), dt_code(xc.scalar_type()), rows, cols, w.defined() ? w.data_ptr() : nullptr,
                                (float)eps, fmt_of(cast_in, &fi), fmt_of(cast_out, &fo), bfp_block, (int)bfp_precision, l.stream),
          "dmxq_rmsnorm_cast_bfp");
  else if (kind == 0)
    check(dmxq_layernorm_cast(xc.data_ptr(), out.data_ptr(), dt_code(xc.scalar_type()), rows, cols, w.defined() ? w.data_ptr() : nullptr,
                              b.defined() ? b.data_ptr() : nullptr, (float)eps, fmt_of(cast_in, &fi), fmt_of(cast_out, &fo), l.stream),
          "dmxq_layernorm_cast");
  else
    check(dmxq_rmsnorm_cast(xc.data_ptr(), out.data_ptr(), dt_code(xc.scalar_type()), rows, cols, w.defined() ? w.data_ptr() : nullptr, (float)eps,
                            fmt_of(cast_in, &fi), fmt_of(cast_out, &fo), l.stream), "dmxq_rmsnorm_cast");
  return out;
}
Tensor norm_cast_meta(const Tensor& x, int64_t, const OptTensor&, const OptTensor&, double, int64_t, at::IntArrayRef, at::IntArrayRef, int64_t, int64_t) {
  return empty_like_shape(x, x.scalar_type());
}

// ------------------------------------------------------------------------------------------------ GPTQ
// the 12 fields of a dmxq_gptq_format in the struct's order, as every raw op that takes a format passes them: one format, or one
// format's slice of a list
inline dmxq_gptq_format gptq_format_of(at::IntArrayRef v, const char* what) {
  TORCH_CHECK(v.size() == 12, what, ": fmt is the 12 fields of dmxq_gptq_format");
  return dmxq_gptq_format{(int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5], (int)v[6], (int)v[7], (int)v[8], (int)v[9], (int)v[10],
                          (int)v[11]};
}
// one column block of GPTQ's in-block loop (dmxq_gptq_block): q and err are written in place (views of the caller's Q and E)
inline void gptq_matrix(const Tensor& t, const Tensor& w, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == w.device() && t.scalar_type() == at::kFloat && t.dim() == 2 && (t.size(1) <= 1 || t.stride(1) == 1),
              "gptq_block: ", name, " must be a float32 matrix with unit column stride on w's GPU");
}
void gptq_block(const Tensor& w, const Tensor& hinv, const Tensor& inv_d, int64_t microblock, at::IntArrayRef fmt, const OptTensor& scale,
                const OptTensor& zero_point, Tensor q, Tensor err) {
  TORCH_CHECK(w.is_cuda(), "gptq_block: tensor is on ", w.device(), "; dmx_compressor_amd runs on MI355X (HIP) tensors only and has no CPU fallback");
  gptq_matrix(w, w, "w"); gptq_matrix(hinv, w, "hinv"); gptq_matrix(q, w, "q"); gptq_matrix(err, w, "err");
  const dmxq_gptq_format f = gptq_format_of(fmt, "gptq_block");
  TORCH_CHECK(microblock >= 1, "gptq_block: microblock must be positive");
  const int64_t rows = w.size(0), count = w.size(1), nmb = (count + microblock - 1) / microblock;
  TORCH_CHECK(q.size(0) == rows && q.size(1) == count && err.size(0) == rows && err.size(1) == count && hinv.size(0) == count &&
              hinv.size(1) == count, "gptq_block: w, q, err must be [rows, count] and hinv [count, count]");
  TORCH_CHECK(inv_d.is_cuda() && inv_d.device() == w.device() && inv_d.scalar_type() == at::kFloat && inv_d.is_contiguous() &&
              inv_d.numel() == nmb * microblock * microblock, "gptq_block: inv_d must be a contiguous float32 [", nmb, ", ", microblock, ", ",
              microblock, "] tensor on w's GPU");
  const bool has_sc = scale.has_value() && scale->defined(), has_zp = zero_point.has_value() && zero_point->defined();
  TORCH_CHECK(!has_sc || (scale->is_cuda() && scale->device() == w.device() && scale->scalar_type() == at::kFloat && scale->is_contiguous()),
              "gptq_block: scale must be a contiguous float32 tensor on w's GPU");
  TORCH_CHECK(!has_zp || (zero_point->is_cuda() && zero_point->device() == w.device() && zero_point->scalar_type() == at::kLong &&
              zero_point->is_contiguous()), "gptq_block: zero_point must be a contiguous int64 tensor on w's GPU");
  TORCH_CHECK(f.kind != DMXQ_GPTQ_FIXED || !f.per_row || (has_sc && has_zp && scale->numel() >= rows && zero_point->numel() >= rows),
              "gptq_block: a per-row fixed point cast needs a scale and a zero point per row");
  TORCH_CHECK(f.kind != DMXQ_GPTQ_FIXED || (has_sc && has_zp && scale->numel() >= 1 && zero_point->numel() >= 1),
              "gptq_block: a fixed point cast needs its scale and zero point");
  auto ld = [count](const Tensor& t) { return t.size(0) <= 1 ? std::max<int64_t>(t.stride(0), count) : t.stride(0); };
  Launch l(w);
  check(dmxq_gptq_block((const float*)w.data_ptr(), ld(w), (float*)q.data_ptr(), ld(q), (float*)err.data_ptr(), ld(err), rows, count,
                        (const float*)hinv.data_ptr(), ld(hinv), (const float*)inv_d.data_ptr(), microblock, &f,
                        has_sc ? (const float*)scale->data_ptr() : nullptr, has_zp ? (const int64_t*)zero_point->data_ptr() : nullptr, l.stream),
        "dmxq_gptq_block");
}
void gptq_block_meta(const Tensor&, const Tensor&, const Tensor&, int64_t, at::IntArrayRef, const OptTensor&, const OptTensor&, Tensor, Tensor) {}

// the same block with dynamic per-group integer scales (dmxq_gptq_block_dynamic): scale_out / zp_out [rows, count / group] are written in
// place as well (views of the caller's [rows, ncols / group] tensors)
void gptq_block_dynamic(const Tensor& w, const Tensor& hinv, const Tensor& inv_d, int64_t microblock, at::IntArrayRef fmt, int64_t rounding,
                        int64_t group, int64_t qmin, int64_t qmax, bool symmetric_qscheme, Tensor q, Tensor err, Tensor scale_out, Tensor zp_out) {
  TORCH_CHECK(w.is_cuda(), "gptq_block_dynamic: tensor is on ", w.device(), "; dmx_compressor_amd runs on MI355X (HIP) tensors only and has no CPU fallback");
  gptq_matrix(w, w, "w"); gptq_matrix(hinv, w, "hinv"); gptq_matrix(q, w, "q"); gptq_matrix(err, w, "err"); gptq_matrix(scale_out, w, "scale_out");
  const dmxq_gptq_format f = gptq_format_of(fmt, "gptq_block_dynamic");
  TORCH_CHECK(microblock >= 1 && group >= 1, "gptq_block_dynamic: microblock and group must be positive");
  const int64_t rows = w.size(0), count = w.size(1), nmb = (count + microblock - 1) / microblock, ng = count / group;
  TORCH_CHECK(q.size(0) == rows && q.size(1) == count && err.size(0) == rows && err.size(1) == count && hinv.size(0) == count &&
              hinv.size(1) == count, "gptq_block_dynamic: w, q, err must be [rows, count] and hinv [count, count]");
  TORCH_CHECK(inv_d.is_cuda() && inv_d.device() == w.device() && inv_d.scalar_type() == at::kFloat && inv_d.is_contiguous() &&
              inv_d.numel() == nmb * microblock * microblock, "gptq_block_dynamic: inv_d must be a contiguous float32 [", nmb, ", ", microblock,
              ", ", microblock, "] tensor on w's GPU");
  TORCH_CHECK(zp_out.is_cuda() && zp_out.device() == w.device() && zp_out.scalar_type() == at::kLong && zp_out.dim() == 2 &&
              (zp_out.size(1) <= 1 || zp_out.stride(1) == 1), "gptq_block_dynamic: zp_out must be an int64 matrix with unit column stride on w's GPU");
  TORCH_CHECK(scale_out.size(0) == rows && scale_out.size(1) == ng && zp_out.size(0) == rows && zp_out.size(1) == ng,
              "gptq_block_dynamic: scale_out and zp_out must be [rows, count / group] = [", rows, ", ", ng, "]");
  auto ld = [](const Tensor& t, int64_t n) { return t.size(0) <= 1 ? std::max<int64_t>(t.stride(0), n) : t.stride(0); };
  Launch l(w);
  check(dmxq_gptq_block_dynamic((const float*)w.data_ptr(), ld(w, count), (float*)q.data_ptr(), ld(q, count), (float*)err.data_ptr(), ld(err, count),
                                rows, count, (const float*)hinv.data_ptr(), ld(hinv, count), (const float*)inv_d.data_ptr(), microblock, &f,
                                (int)rounding, group, (int)qmin, (int)qmax, symmetric_qscheme ? 1 : 0, (float*)scale_out.data_ptr(),
                                ld(scale_out, ng), (int64_t*)zp_out.data_ptr(), ld(zp_out, ng), l.stream),
        "dmxq_gptq_block_dynamic");
}
void gptq_block_dynamic_meta(const Tensor&, const Tensor&, const Tensor&, int64_t, at::IntArrayRef, int64_t, int64_t, int64_t, int64_t, bool, Tensor,
                             Tensor, Tensor, Tensor) {}

// ------------------------------------------------------------------------------------------------ HistogramObserver
// one observation of G groups (dmxq_hist_observe): hist [G, bins], min_val / max_val [G], status [1] (int32) are the observer's state,
// updated in place; scratch: (2 + bins) * G words of any contiguous device tensor
inline void hist_state(const Tensor& t, const Tensor& like, at::ScalarType dt, int64_t numel, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device() && t.scalar_type() == dt && t.is_contiguous() && t.numel() == numel,
              "hist_observe: ", what, " must be a contiguous ", c10::toString(dt), " tensor of ", numel, " entries on the input's device");
}
void hist_observe(const Tensor& x, int64_t ch_axis, int64_t group_size, int64_t upsample_rate, Tensor hist, Tensor min_val, Tensor max_val,
                  Tensor status, Tensor scratch) {
  const Tensor xc = prep(x, "hist_observe");
  TORCH_CHECK(group_size >= 1 && upsample_rate >= 1, "hist_observe: group_size and upsample_rate must be positive");
  const Split3 s = split3(xc, ch_axis);
  const int64_t G = (s.L + group_size - 1) / group_size;
  TORCH_CHECK(G >= 1 && hist.numel() % G == 0 && hist.numel() >= G, "hist_observe: the histogram must hold ", G, " groups of bins");
  hist_state(hist, xc, at::kFloat, hist.numel(), "hist");
  hist_state(min_val, xc, at::kFloat, G, "min_val");
  hist_state(max_val, xc, at::kFloat, G, "max_val");
  hist_state(status, xc, at::kInt, 1, "status");
  TORCH_CHECK(scratch.is_cuda() && scratch.device() == xc.device() && scratch.is_contiguous(), "hist_observe: scratch must be a contiguous tensor on the input's device");
  Launch l(xc);
  check(dmxq_hist_observe(xc.data_ptr(), dt_code(xc.scalar_type()), s.outer, s.L, s.inner, group_size, hist.numel() / G, upsample_rate,
                          (float*)hist.data_ptr(), (float*)min_val.data_ptr(), (float*)max_val.data_ptr(), (int*)status.data_ptr(),
                          scratch.data_ptr(), (int64_t)(scratch.numel() * scratch.element_size()), l.stream),
        "dmxq_hist_observe");
}
void hist_observe_meta(const Tensor&, int64_t, int64_t, int64_t, Tensor, Tensor, Tensor, Tensor, Tensor) {}

// the range search and (scale, zero_point) of every group (dmxq_hist_qparams): two [G] tensors
std::tuple<Tensor, Tensor> hist_qparams(const Tensor& hist, const Tensor& min_val, const Tensor& max_val, int64_t precision, int64_t qmin,
                                        int64_t qmax, bool symmetric_qscheme) {
  TORCH_CHECK(hist.is_cuda(), "hist_qparams: tensor is on ", hist.device(), "; dmx_compressor_amd runs on MI355X (HIP) tensors only and has no CPU fallback");
  const int64_t G = min_val.numel();
  TORCH_CHECK(G >= 1 && hist.numel() % G == 0 && hist.numel() >= G, "hist_qparams: the histogram must hold ", G, " groups of bins");
  hist_state(hist, hist, at::kFloat, hist.numel(), "hist");
  hist_state(min_val, hist, at::kFloat, G, "min_val");
  hist_state(max_val, hist, at::kFloat, G, "max_val");
  Tensor scale = at::empty({G}, hist.options().dtype(at::kFloat)), zp = at::empty({G}, hist.options().dtype(at::kLong));
  Launch l(hist);
  check(dmxq_hist_qparams((const float*)hist.data_ptr(), (const float*)min_val.data_ptr(), (const float*)max_val.data_ptr(), G, hist.numel() / G,
                          (int)precision, (int)qmin, (int)qmax, symmetric_qscheme, (float*)scale.data_ptr(), (int64_t*)zp.data_ptr(), l.stream),
        "dmxq_hist_qparams");
  return {scale, zp};
}
std::tuple<Tensor, Tensor> hist_qparams_meta(const Tensor& hist, const Tensor& min_val, const Tensor&, int64_t, int64_t, int64_t, bool) {
  return {at::empty({min_val.numel()}, hist.options().dtype(at::kFloat)), at::empty({min_val.numel()}, hist.options().dtype(at::kLong))};
}

// ------------------------------------------------------------------------------------------------ error statistics
// rows of [sum_sq_err, sum_sq_ref, max_abs_err, count] (dmxq_error_stats, dmxq_cast_error): stats is float64 [.., 4], written (or merged
// into) in place; scratch: dmxq_error_scratch_bytes bytes of any contiguous device tensor
inline void error_rows(const Tensor& stats, const Tensor& scratch, const Tensor& like, int64_t rows, const char* op) {
  TORCH_CHECK(stats.is_cuda() && stats.device() == like.device() && stats.scalar_type() == at::kDouble && stats.is_contiguous() &&
              stats.numel() == 4 * rows, op, ": stats must be a contiguous float64 tensor of ", rows, " x 4 entries on the input's device");
  TORCH_CHECK(scratch.is_cuda() && scratch.device() == like.device() && scratch.is_contiguous(), op,
              ": scratch must be a contiguous tensor on the input's device");
}
void error_stats(const Tensor& ref, const Tensor& test, bool accumulate, Tensor stats, Tensor scratch) {
  const Tensor rc = prep(ref, "error_stats"), tc = prep(test, "error_stats");
  TORCH_CHECK(rc.device() == tc.device() && rc.numel() == tc.numel(), "error_stats: ref and test must hold the same number of elements on one device");
  error_rows(stats, scratch, rc, 1, "error_stats");
  Launch l(rc);
  check(dmxq_error_stats(rc.data_ptr(), dt_code(rc.scalar_type()), tc.data_ptr(), dt_code(tc.scalar_type()), rc.numel(), accumulate,
                         (double*)stats.data_ptr(), scratch.data_ptr(), (int64_t)(scratch.numel() * scratch.element_size()), l.stream),
        "dmxq_error_stats");
}
void error_stats_meta(const Tensor&, const Tensor&, bool, Tensor, Tensor) {}

// x: [rows, L] (any leading dims, blocks along the last); fmts: 12 fields of dmxq_gptq_format per format; scale / zero_point: one entry
// per format (read for the fixed point ones)
void cast_error(const Tensor& x, at::IntArrayRef fmts, const OptTensor& scale, const OptTensor& zero_point, bool accumulate, Tensor stats,
                Tensor scratch) {
  const Tensor xc = prep(x, "cast_error");
  TORCH_CHECK(!fmts.empty() && fmts.size() % 12 == 0, "cast_error: fmts is the 12 fields of dmxq_gptq_format per format");
  const int64_t K = (int64_t)fmts.size() / 12;
  error_rows(stats, scratch, xc, K, "cast_error");
  const bool has_sc = scale.has_value() && scale->defined(), has_zp = zero_point.has_value() && zero_point->defined();
  TORCH_CHECK(!has_sc || (scale->is_cuda() && scale->device() == xc.device() && scale->scalar_type() == at::kFloat && scale->is_contiguous() &&
              scale->numel() >= K), "cast_error: scale must be a contiguous float32 tensor with an entry per format on x's GPU");
  TORCH_CHECK(!has_zp || (zero_point->is_cuda() && zero_point->device() == xc.device() && zero_point->scalar_type() == at::kLong &&
              zero_point->is_contiguous() && zero_point->numel() >= K),
              "cast_error: zero_point must be a contiguous int64 tensor with an entry per format on x's GPU");
  std::vector<dmxq_gptq_format> f((size_t)K);
  for (int64_t k = 0; k < K; k++) f[(size_t)k] = gptq_format_of(fmts.slice(12 * k, 12), "cast_error");
  const int64_t L = xc.dim() ? xc.size(-1) : 1, rows = L ? xc.numel() / L : 0;
  Launch l(xc);
  check(dmxq_cast_error(xc.data_ptr(), dt_code(xc.scalar_type()), rows, L, f.data(), (int)K, has_sc ? (const float*)scale->data_ptr() : nullptr,
                        has_zp ? (const int64_t*)zero_point->data_ptr() : nullptr, accumulate, (double*)stats.data_ptr(), scratch.data_ptr(),
                        (int64_t)(scratch.numel() * scratch.element_size()), l.stream),
        "dmxq_cast_error");
}
void cast_error_meta(const Tensor&, at::IntArrayRef, const OptTensor&, const OptTensor&, bool, Tensor, Tensor) {}

// ------------------------------------------------------------------------------------------------ Hadamard rotation
// x: [rows, L] (any leading dims; blocks of `size` along the last dim); fmt: empty = rotation only, else the 12 fields of dmxq_gptq_format;
// scale / zero_point: one entry, or one per row when the format says per_row (read for a fixed point format)
Tensor hadamard_qdq(const Tensor& x, int64_t size, bool inverse, at::IntArrayRef fmt, const OptTensor& scale, const OptTensor& zero_point,
                    OptDtype out_dtype) {
  const Tensor xc = prep(x, "hadamard_qdq");
  TORCH_CHECK(fmt.empty() || fmt.size() == 12, "hadamard_qdq: fmt is empty (rotation only) or the 12 fields of dmxq_gptq_format");
  TORCH_CHECK(xc.dim() >= 1, "hadamard_qdq: expects a tensor with at least one dimension");
  Tensor out = empty_like_shape(xc, out_dtype);
  const int64_t L = xc.size(-1), rows = L ? xc.numel() / L : 0;
  dmxq_gptq_format f{};
  if (!fmt.empty()) f = gptq_format_of(fmt, "hadamard_qdq");
  const bool has_sc = scale.has_value() && scale->defined(), has_zp = zero_point.has_value() && zero_point->defined();
  const int64_t need = (!fmt.empty() && f.kind == DMXQ_GPTQ_FIXED) ? (f.per_row ? rows : 1) : 0;
  TORCH_CHECK(!has_sc || (scale->is_cuda() && scale->device() == xc.device() && scale->scalar_type() == at::kFloat && scale->is_contiguous()),
              "hadamard_qdq: scale must be a contiguous float32 tensor on x's GPU");
  TORCH_CHECK(!has_zp || (zero_point->is_cuda() && zero_point->device() == xc.device() && zero_point->scalar_type() == at::kLong &&
              zero_point->is_contiguous()), "hadamard_qdq: zero_point must be a contiguous int64 tensor on x's GPU");
  TORCH_CHECK(need == 0 || (has_sc && has_zp && scale->numel() >= need && zero_point->numel() >= need),
              "hadamard_qdq: a fixed point cast needs its scale and zero point (one per row when per_row)");
  Launch l(xc);
  check(dmxq_hadamard_qdq(xc.data_ptr(), out.data_ptr(), dt_code(xc.scalar_type()), dt_code(out.scalar_type()), rows, L, size, inverse ? 1 : 0,
                          fmt.empty() ? nullptr : &f, has_sc ? (const float*)scale->data_ptr() : nullptr,
                          has_zp ? (const int64_t*)zero_point->data_ptr() : nullptr, l.stream), "dmxq_hadamard_qdq");
  return out;
}
Tensor hadamard_qdq_meta(const Tensor& x, int64_t, bool, at::IntArrayRef, const OptTensor&, const OptTensor&, OptDtype out_dtype) {
  return empty_like_shape(x, out_dtype);
}

// ------------------------------------------------------------------------------------------------ dynamic integer cast
// x: contiguous, numel % segment == 0; -> (out, scale [n_segments] float32, zero_point [n_segments] int64), the last two empty unless
// want_qparams.  DMXQ_ERR_UNSUPPORTED (NotImplementedError, nothing launched): the front end runs the three-launch chain.
std::tuple<Tensor, Tensor, Tensor> dynamic_fixed_qdq(const Tensor& x, int64_t segment, bool whole_rows, int64_t precision, int64_t fraction,
                                                     bool clamp, bool symmetric, int64_t rounding, int64_t qmin, int64_t qmax,
                                                     bool symmetric_qscheme, bool want_qparams, OptDtype out_dtype) {
  const Tensor xc = prep(x, "dynamic_fixed_qdq");
  TORCH_CHECK(segment >= 1 && xc.numel() % segment == 0, "dynamic_fixed_qdq: the segment must divide the number of elements");
  const int64_t n = xc.numel() / segment;
  Tensor out = empty_like_shape(xc, out_dtype);
  Tensor sc = at::empty({want_qparams ? n : 0}, xc.options().dtype(at::kFloat));
  Tensor zp = at::empty({want_qparams ? n : 0}, xc.options().dtype(at::kLong));
  Launch l(xc);
  check(dmxq_dynamic_fixed_qdq(xc.data_ptr(), out.data_ptr(), dt_code(xc.scalar_type()), dt_code(out.scalar_type()), n, segment, whole_rows ? 1 : 0,
                               (int)precision, (int)fraction, clamp ? 1 : 0, symmetric ? 1 : 0, (int)rounding, (int)qmin, (int)qmax,
                               symmetric_qscheme ? 1 : 0, want_qparams ? (float*)sc.data_ptr() : nullptr,
                               want_qparams ? (int64_t*)zp.data_ptr() : nullptr, l.stream), "dmxq_dynamic_fixed_qdq");
  return std::make_tuple(out, sc, zp);
}
std::tuple<Tensor, Tensor, Tensor> dynamic_fixed_qdq_meta(const Tensor& x, int64_t segment, bool, int64_t, int64_t, bool, bool, int64_t, int64_t,
                                                          int64_t, bool, bool want_qparams, OptDtype out_dtype) {
  const int64_t n = (want_qparams && segment >= 1) ? x.numel() / segment : 0;
  return std::make_tuple(empty_like_shape(x, out_dtype), at::empty({n}, x.options().dtype(at::kFloat)), at::empty({n}, x.options().dtype(at::kLong)));
}

// ------------------------------------------------------------------------------------------------ learned step size (backward)
// x, g: contiguous, one shape, numel % segment == 0; scale, zero_point: float32 [n_segments]; whole_rows: 0 groups, 1 rows, 2 the whole
// tensor (the partial rows' scratch is allocated here) -> (dx, empty unless want_dx: then nothing is stored; ds float32 [n_segments];
// dz float32 [n_segments], empty unless want_dz).
// DMXQ_ERR_UNSUPPORTED (NotImplementedError, nothing launched): the front end runs its chain of torch operations.
std::tuple<Tensor, Tensor, Tensor> lsq_backward(const Tensor& x, const Tensor& g, const Tensor& scale, const Tensor& zero_point, int64_t segment,
                                                int64_t whole_rows, int64_t precision, int64_t rounding, int64_t qmin, int64_t qmax,
                                                double grad_factor, bool want_dz, bool want_dx) {
  const Tensor xc = prep(x, "lsq_backward"), gc = prep(g, "lsq_backward");
  TORCH_CHECK(gc.device() == xc.device() && gc.numel() == xc.numel(), "lsq_backward: x and g must hold the same number of elements on one device");
  TORCH_CHECK(segment >= 1 && xc.numel() % segment == 0, "lsq_backward: the segment must divide the number of elements");
  const int64_t n = xc.numel() / segment;
  TORCH_CHECK(scale.is_cuda() && scale.device() == xc.device() && scale.scalar_type() == at::kFloat && scale.is_contiguous() && scale.numel() == n &&
              zero_point.is_cuda() && zero_point.device() == xc.device() && zero_point.scalar_type() == at::kFloat && zero_point.is_contiguous() &&
              zero_point.numel() == n, "lsq_backward: scale and zero_point must be contiguous float32 tensors of ", n, " entries on x's GPU");
  Tensor dx = want_dx ? empty_like_shape(xc, c10::nullopt) : at::empty({0}, xc.options());
  Tensor ds = at::empty({n}, xc.options().dtype(at::kFloat));
  Tensor dz = at::empty({want_dz ? n : 0}, xc.options().dtype(at::kFloat));
  const int64_t sb = whole_rows == 2 ? dmxq_lsq_scratch_bytes(segment) : 0;
  Tensor scratch = at::empty({sb / 8}, xc.options().dtype(at::kDouble));
  Launch l(xc);
  check(dmxq_lsq_backward(xc.data_ptr(), gc.data_ptr(), want_dx ? dx.data_ptr() : nullptr, dt_code(xc.scalar_type()), dt_code(gc.scalar_type()),
                          dt_code(dx.scalar_type()), n, segment, (int)whole_rows, (int)precision, (int)rounding, (int)qmin, (int)qmax,
                          (const float*)scale.data_ptr(), (const float*)zero_point.data_ptr(), grad_factor, want_dz ? 1 : 0,
                          (float*)ds.data_ptr(), want_dz ? (float*)dz.data_ptr() : nullptr, sb ? scratch.data_ptr() : nullptr, sb, l.stream),
        "dmxq_lsq_backward");
  return std::make_tuple(dx, ds, dz);
}
std::tuple<Tensor, Tensor, Tensor> lsq_backward_meta(const Tensor& x, const Tensor&, const Tensor&, const Tensor&, int64_t segment, int64_t, int64_t,
                                                     int64_t, int64_t, int64_t, double, bool want_dz, bool want_dx) {
  const int64_t n = segment >= 1 ? x.numel() / segment : 0;
  return std::make_tuple(want_dx ? empty_like_shape(x, c10::nullopt) : at::empty({0}, x.options()), at::empty({n}, x.options().dtype(at::kFloat)),
                         at::empty({want_dz ? n : 0}, x.options().dtype(at::kFloat)));
}

// ------------------------------------------------------------------------------------------------ dynamic scaled float cast
// x: contiguous; mode: dmxq_dynamic_float_mode; -> (out, scale float32 [n_segments], or [..., R / g, C / g] for tiles; empty unless
// want_scale).  DMXQ_ERR_UNSUPPORTED (NotImplementedError, nothing launched): the front end runs its chain of launches.
std::vector<int64_t> dynamic_float_scale_shape(const Tensor& x, int64_t mode, int64_t segment, const char* what) {
  TORCH_CHECK(segment >= 1, what, ": the segment must be positive");
  if (mode == DMXQ_DYNF_TILE) {
    TORCH_CHECK(x.dim() >= 2 && x.size(-2) % segment == 0 && x.size(-1) % segment == 0, what,
                ": the tile size must divide the last two dimensions");
    std::vector<int64_t> shape(x.sizes().begin(), x.sizes().end());
    shape[shape.size() - 2] /= segment;
    shape[shape.size() - 1] /= segment;
    return shape;
  }
  TORCH_CHECK(x.numel() % segment == 0, what, ": the segment must divide the number of elements");
  return {x.numel() / segment};
}
std::tuple<Tensor, Tensor> dynamic_float_qdq(const Tensor& x, int64_t mode, int64_t segment, int64_t man, int64_t exp, int64_t bias,
                                             bool flush_subnormal, int64_t rounding, bool pow2_scale, bool want_scale, OptDtype out_dtype) {
  const Tensor xc = prep(x, "dynamic_float_qdq");
  const std::vector<int64_t> shape = dynamic_float_scale_shape(xc, mode, segment, "dynamic_float_qdq");
  int64_t n = 1;
  for (int64_t d : shape) n *= d;
  const bool tile = mode == DMXQ_DYNF_TILE;
  const int64_t cols = tile ? xc.size(-1) : 0, rows = tile && cols ? xc.numel() / cols : 0;
  Tensor out = empty_like_shape(xc, out_dtype);
  Tensor sc = want_scale ? at::empty(shape, xc.options().dtype(at::kFloat)) : at::empty({0}, xc.options().dtype(at::kFloat));
  Launch l(xc);
  check(dmxq_dynamic_float_qdq(xc.data_ptr(), out.data_ptr(), dt_code(xc.scalar_type()), dt_code(out.scalar_type()), (int)mode, n, segment, rows,
                               cols, (int)man, (int)exp, (int)bias, flush_subnormal ? 1 : 0, (int)rounding, pow2_scale ? 1 : 0,
                               want_scale ? (float*)sc.data_ptr() : nullptr, l.stream), "dmxq_dynamic_float_qdq");
  return std::make_tuple(out, sc);
}
std::tuple<Tensor, Tensor> dynamic_float_qdq_meta(const Tensor& x, int64_t mode, int64_t segment, int64_t, int64_t, int64_t, bool, int64_t, bool,
                                                  bool want_scale, OptDtype out_dtype) {
  const std::vector<int64_t> shape = dynamic_float_scale_shape(x, mode, segment, "dynamic_float_qdq");
  return std::make_tuple(empty_like_shape(x, out_dtype),
                         want_scale ? at::empty(shape, x.options().dtype(at::kFloat)) : at::empty({0}, x.options().dtype(at::kFloat)));
}

// ------------------------------------------------------------------------------------------------ codebook casts
// x: contiguous; mode: DMXQ_DYNF_GROUP / DMXQ_DYNF_ROWS; levels: contiguous float32 [K] on x's GPU; norm <= 0: the table's own maximum
// -> (out, scale float32 [n_segments], index uint8 in x's shape; the last two empty unless wanted).
// DMXQ_ERR_UNSUPPORTED (NotImplementedError, nothing launched): the front end runs its chain of launches.
void codebook_args(const Tensor& xc, int64_t segment, const Tensor& levels, const char* what) {
  TORCH_CHECK(segment >= 1 && xc.numel() % segment == 0, what, ": the segment must divide the number of elements");
  TORCH_CHECK(levels.is_cuda() && levels.device() == xc.device() && levels.scalar_type() == at::kFloat && levels.is_contiguous() &&
              levels.dim() == 1, what, ": the levels must be a contiguous 1-d float32 tensor on x's GPU");
}
std::tuple<Tensor, Tensor, Tensor> codebook_qdq(const Tensor& x, int64_t mode, int64_t segment, const Tensor& levels, double norm, bool want_scale,
                                                bool want_index, OptDtype out_dtype) {
  const Tensor xc = prep(x, "codebook_qdq");
  codebook_args(xc, segment, levels, "codebook_qdq");
  const int64_t n = xc.numel() / segment;
  Tensor out = empty_like_shape(xc, out_dtype);
  Tensor sc = at::empty({want_scale ? n : 0}, xc.options().dtype(at::kFloat));
  Tensor idx = want_index ? empty_like_shape(xc, at::kByte) : at::empty({0}, xc.options().dtype(at::kByte));
  Launch l(xc);
  check(dmxq_codebook_qdq(xc.data_ptr(), out.data_ptr(), dt_code(xc.scalar_type()), dt_code(out.scalar_type()), (int)mode, n, segment,
                          (const float*)levels.data_ptr(), (int)levels.numel(), (float)norm, want_scale ? (float*)sc.data_ptr() : nullptr,
                          want_index ? (uint8_t*)idx.data_ptr() : nullptr, l.stream), "dmxq_codebook_qdq");
  return std::make_tuple(out, sc, idx);
}
std::tuple<Tensor, Tensor, Tensor> codebook_qdq_meta(const Tensor& x, int64_t, int64_t segment, const Tensor&, double, bool want_scale,
                                                     bool want_index, OptDtype out_dtype) {
  const int64_t n = (want_scale && segment >= 1) ? x.numel() / segment : 0;
  return std::make_tuple(empty_like_shape(x, out_dtype), at::empty({n}, x.options().dtype(at::kFloat)),
                         want_index ? empty_like_shape(x, at::kByte) : at::empty({0}, x.options().dtype(at::kByte)));
}
// acc (float64 [K, 3]) (+)= the Lloyd statistics of x under the table; the partial rows' workspace is allocated here
void codebook_accumulate(const Tensor& x, int64_t mode, int64_t segment, const Tensor& levels, double norm, Tensor acc, bool accumulate) {
  const Tensor xc = prep(x, "codebook_accumulate");
  codebook_args(xc, segment, levels, "codebook_accumulate");
  TORCH_CHECK(acc.is_cuda() && acc.device() == xc.device() && acc.scalar_type() == at::kDouble && acc.is_contiguous() &&
              acc.numel() == levels.numel() * 3, "codebook_accumulate: acc must be a contiguous float64 [K, 3] tensor on x's GPU");
  const int64_t n = xc.numel() / segment;
  const int64_t wb = dmxq_codebook_workspace_bytes(dt_code(xc.scalar_type()), (int)mode, n, segment);
  Tensor ws = at::empty({wb / 8 + 1}, xc.options().dtype(at::kDouble));
  Launch l(xc);
  check(dmxq_codebook_accumulate(xc.data_ptr(), dt_code(xc.scalar_type()), (int)mode, n, segment, (const float*)levels.data_ptr(),
                                 (int)levels.numel(), (float)norm, (double*)acc.data_ptr(), accumulate ? 1 : 0, ws.data_ptr(), l.stream),
        "dmxq_codebook_accumulate");
}
void codebook_accumulate_meta(const Tensor&, int64_t, int64_t, const Tensor&, double, Tensor, bool) {}

// ------------------------------------------------------------------------------------------------ vector codebook casts
// x: contiguous; mode: DMXQ_DYNF_GROUP / DMXQ_DYNF_ROWS; table: contiguous float32 [K, d] on x's GPU; norm <= 0: the table's own maximum
// -> (out, scale float32 [n_segments], index uint8 x.shape[:-1] + (L / d,); the last two empty unless wanted).
// DMXQ_ERR_UNSUPPORTED (NotImplementedError, nothing launched): the front end runs its chain of torch operations.
void vq_args(const Tensor& xc, int64_t segment, const Tensor& table, const char* what) {
  TORCH_CHECK(segment >= 1 && xc.numel() % segment == 0, what, ": the segment must divide the number of elements");
  TORCH_CHECK(table.is_cuda() && table.device() == xc.device() && table.scalar_type() == at::kFloat && table.is_contiguous() &&
              table.dim() == 2 && table.size(1) >= 1, what, ": the table must be a contiguous float32 [K, d] tensor on x's GPU");
  TORCH_CHECK(xc.dim() >= 1 && xc.size(-1) % table.size(1) == 0, what, ": the last dimension must be a multiple of the table's d");
}
Tensor vq_index_like(const Tensor& x, int64_t d, bool want) {
  if (!want) return at::empty({0}, x.options().dtype(at::kByte));
  std::vector<int64_t> shape = x.sizes().vec();
  shape.back() /= d;
  return at::empty(shape, x.options().dtype(at::kByte));
}
std::tuple<Tensor, Tensor, Tensor> vq_qdq(const Tensor& x, int64_t mode, int64_t segment, const Tensor& table, double norm, bool want_scale,
                                          bool want_index, OptDtype out_dtype) {
  const Tensor xc = prep(x, "vq_qdq");
  vq_args(xc, segment, table, "vq_qdq");
  const int64_t n = xc.numel() / segment;
  Tensor out = empty_like_shape(xc, out_dtype);
  Tensor sc = at::empty({want_scale ? n : 0}, xc.options().dtype(at::kFloat));
  Tensor idx = vq_index_like(xc, table.size(1), want_index);
  Launch l(xc);
  check(dmxq_vq_qdq(xc.data_ptr(), out.data_ptr(), dt_code(xc.scalar_type()), dt_code(out.scalar_type()), (int)mode, n, segment,
                    (const float*)table.data_ptr(), (int)table.size(1), (int)table.size(0), (float)norm,
                    want_scale ? (float*)sc.data_ptr() : nullptr, want_index ? (uint8_t*)idx.data_ptr() : nullptr, l.stream), "dmxq_vq_qdq");
  return std::make_tuple(out, sc, idx);
}
std::tuple<Tensor, Tensor, Tensor> vq_qdq_meta(const Tensor& x, int64_t, int64_t segment, const Tensor& table, double, bool want_scale,
                                               bool want_index, OptDtype out_dtype) {
  const int64_t n = (want_scale && segment >= 1) ? x.numel() / segment : 0;
  return std::make_tuple(empty_like_shape(x, out_dtype), at::empty({n}, x.options().dtype(at::kFloat)),
                         vq_index_like(x, table.size(1), want_index));
}
// acc (float64 [K, d + 2]) (+)= the k-means statistics of x under the table; the partial blocks' workspace is allocated here
void vq_accumulate(const Tensor& x, int64_t mode, int64_t segment, const Tensor& table, double norm, Tensor acc, bool accumulate) {
  const Tensor xc = prep(x, "vq_accumulate");
  vq_args(xc, segment, table, "vq_accumulate");
  TORCH_CHECK(acc.is_cuda() && acc.device() == xc.device() && acc.scalar_type() == at::kDouble && acc.is_contiguous() &&
              acc.numel() == table.size(0) * (table.size(1) + 2), "vq_accumulate: acc must be a contiguous float64 [K, d + 2] tensor on x's GPU");
  const int64_t n = xc.numel() / segment;
  const int64_t wb = dmxq_vq_workspace_bytes(dt_code(xc.scalar_type()), (int)mode, n, segment, (int)table.size(1), (int)table.size(0));
  Tensor ws = at::empty({wb / 8 + 1}, xc.options().dtype(at::kDouble));
  Launch l(xc);
  check(dmxq_vq_accumulate(xc.data_ptr(), dt_code(xc.scalar_type()), (int)mode, n, segment, (const float*)table.data_ptr(),
                           (int)table.size(1), (int)table.size(0), (float)norm, (double*)acc.data_ptr(), accumulate ? 1 : 0, ws.data_ptr(),
                           l.stream), "dmxq_vq_accumulate");
}
void vq_accumulate_meta(const Tensor&, int64_t, int64_t, const Tensor&, double, Tensor, bool) {}

// ------------------------------------------------------------------------------------------------ HQQ
// x: contiguous; segment: the group size -> (out, scale float32 [n_segments], zero float32 [n_segments], codes uint8 in x's shape; the
// qparams empty unless want_qparams, the codes empty unless want_codes).
// DMXQ_ERR_UNSUPPORTED (NotImplementedError, nothing launched): the front end runs its chain of torch operations.
std::tuple<Tensor, Tensor, Tensor, Tensor> hqq_qdq(const Tensor& x, int64_t segment, int64_t rounding, int64_t qmin, int64_t qmax, double lp_norm,
                                                   double beta, double kappa, int64_t iters, bool want_qparams, bool want_codes,
                                                   OptDtype out_dtype) {
  const Tensor xc = prep(x, "hqq_qdq");
  TORCH_CHECK(segment >= 1 && xc.numel() % segment == 0, "hqq_qdq: the group size must divide the number of elements");
  const int64_t n = xc.numel() / segment;
  Tensor out = empty_like_shape(xc, out_dtype);
  Tensor sc = at::empty({want_qparams ? n : 0}, xc.options().dtype(at::kFloat));
  Tensor zero = at::empty({want_qparams ? n : 0}, xc.options().dtype(at::kFloat));
  Tensor codes = want_codes ? empty_like_shape(xc, at::kByte) : at::empty({0}, xc.options().dtype(at::kByte));
  Launch l(xc);
  check(dmxq_hqq_qdq(xc.data_ptr(), out.data_ptr(), dt_code(xc.scalar_type()), dt_code(out.scalar_type()), n, segment, (int)rounding, (int)qmin,
                     (int)qmax, (float)lp_norm, (float)beta, (float)kappa, (int)iters, want_qparams ? (float*)sc.data_ptr() : nullptr,
                     want_qparams ? (float*)zero.data_ptr() : nullptr, want_codes ? (uint8_t*)codes.data_ptr() : nullptr, l.stream),
        "dmxq_hqq_qdq");
  return std::make_tuple(out, sc, zero, codes);
}
std::tuple<Tensor, Tensor, Tensor, Tensor> hqq_qdq_meta(const Tensor& x, int64_t segment, int64_t, int64_t, int64_t, double, double, double, int64_t,
                                                        bool want_qparams, bool want_codes, OptDtype out_dtype) {
  const int64_t n = (want_qparams && segment >= 1) ? x.numel() / segment : 0;
  return std::make_tuple(empty_like_shape(x, out_dtype), at::empty({n}, x.options().dtype(at::kFloat)), at::empty({n}, x.options().dtype(at::kFloat)),
                         want_codes ? empty_like_shape(x, at::kByte) : at::empty({0}, x.options().dtype(at::kByte)));
}

// ------------------------------------------------------------------------------------------------ outlier-aware dynamic cast
// x: contiguous; segment: the group size; k: outliers per group; outlier_fmt: [man_bits, exp_bits, exp_bias, flush_subnormal] or empty = the
// input's own bits -> (out, scale float32 [n_segments], zero_point int64 [n_segments], idx int32 [n_segments, k], val [n_segments, k] of
// out's dtype; the qparams empty unless want_qparams, idx / val empty unless want_outliers).
// DMXQ_ERR_UNSUPPORTED (NotImplementedError, nothing launched): the front end runs its chain.
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> outlier_fixed_qdq(const Tensor& x, int64_t segment, int64_t k, int64_t precision, int64_t fraction,
                                                                     bool clamp, bool symmetric, int64_t rounding, int64_t qmin, int64_t qmax,
                                                                     bool symmetric_qscheme, at::IntArrayRef outlier_fmt, bool want_qparams,
                                                                     bool want_outliers, OptDtype out_dtype) {
  const Tensor xc = prep(x, "outlier_fixed_qdq");
  TORCH_CHECK(segment >= 1 && xc.numel() % segment == 0, "outlier_fixed_qdq: the segment must divide the number of elements");
  TORCH_CHECK(k >= 0, "outlier_fixed_qdq: k must not be negative");
  const int64_t n = xc.numel() / segment;
  Tensor out = empty_like_shape(xc, out_dtype);
  Tensor sc = at::empty({want_qparams ? n : 0}, xc.options().dtype(at::kFloat));
  Tensor zp = at::empty({want_qparams ? n : 0}, xc.options().dtype(at::kLong));
  Tensor idx = at::empty({want_outliers ? n : 0, k}, xc.options().dtype(at::kInt));
  Tensor val = at::empty({want_outliers ? n : 0, k}, out.options());
  dmxq_float_fmt fo;
  Launch l(xc);
  check(dmxq_outlier_fixed_qdq(xc.data_ptr(), out.data_ptr(), dt_code(xc.scalar_type()), dt_code(out.scalar_type()), n, segment, (int)k,
                               (int)precision, (int)fraction, clamp ? 1 : 0, symmetric ? 1 : 0, (int)rounding, (int)qmin, (int)qmax,
                               symmetric_qscheme ? 1 : 0, fmt_of(outlier_fmt, &fo), want_qparams ? (float*)sc.data_ptr() : nullptr,
                               want_qparams ? (int64_t*)zp.data_ptr() : nullptr, want_outliers ? (int32_t*)idx.data_ptr() : nullptr,
                               want_outliers ? val.data_ptr() : nullptr, l.stream),
        "dmxq_outlier_fixed_qdq");
  return std::make_tuple(out, sc, zp, idx, val);
}
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> outlier_fixed_qdq_meta(const Tensor& x, int64_t segment, int64_t k, int64_t, int64_t, bool, bool,
                                                                          int64_t, int64_t, int64_t, bool, at::IntArrayRef, bool want_qparams,
                                                                          bool want_outliers, OptDtype out_dtype) {
  const int64_t all = segment >= 1 ? x.numel() / segment : 0;
  const int64_t n = want_qparams ? all : 0, m = want_outliers ? all : 0;
  Tensor out = empty_like_shape(x, out_dtype);
  return std::make_tuple(out, at::empty({n}, x.options().dtype(at::kFloat)), at::empty({n}, x.options().dtype(at::kLong)),
                         at::empty({m, k}, x.options().dtype(at::kInt)), at::empty({m, k}, out.options()));
}

// ------------------------------------------------------------------------------------------------ Wanda
// acc (float64 [C], C = x's last dim) += the sum of squares over every other dim; scratch: dmxq_channel_sumsq_workspace_bytes bytes of
// any contiguous device tensor
typedef int (*channel_sum_fn)(const void*, int, int64_t, int64_t, double*, void*, void*);
void channel_sum(const Tensor& x, Tensor acc, Tensor scratch, channel_sum_fn fn, const char* what);
void channel_sumsq(const Tensor& x, Tensor acc, Tensor scratch) { channel_sum(x, acc, scratch, dmxq_channel_sumsq_accumulate, "channel_sumsq"); }
// the |x| twin (AWQ): same checks, same scratch
void channel_sumabs(const Tensor& x, Tensor acc, Tensor scratch) { channel_sum(x, acc, scratch, dmxq_channel_sumabs_accumulate, "channel_sumabs"); }
void channel_sum(const Tensor& x, Tensor acc, Tensor scratch, channel_sum_fn fn, const char* what) {
  const Tensor xc = prep(x, what);
  const int64_t C = xc.dim() ? xc.size(-1) : 1, rows = C ? xc.numel() / C : 0;
  TORCH_CHECK(acc.is_cuda() && acc.device() == xc.device() && acc.scalar_type() == at::kDouble && acc.is_contiguous() && acc.numel() == C,
              what, ": acc must be a contiguous float64 tensor of ", C, " entries on the input's device");
  const int64_t need = dmxq_channel_sumsq_workspace_bytes(rows, C);
  TORCH_CHECK(scratch.is_cuda() && scratch.device() == xc.device() && scratch.is_contiguous() &&
              (int64_t)(scratch.numel() * scratch.element_size()) >= need && (uintptr_t)scratch.data_ptr() % 8 == 0,
              what, ": scratch must be a contiguous 8-byte aligned tensor of at least ", need, " bytes on the input's device");
  Launch l(xc);
  check(fn(xc.data_ptr(), dt_code(xc.scalar_type()), rows, C, (double*)acc.data_ptr(), scratch.data_ptr(), l.stream), what);
}
void channel_sumsq_meta(const Tensor&, Tensor, Tensor) {}
void channel_sumabs_meta(const Tensor&, Tensor, Tensor) {}

// -> (score float32, mask, y): an output that was not requested comes back as an empty 1-d tensor
std::tuple<Tensor, Tensor, Tensor> wanda_nm(const Tensor& w, const Tensor& act_norm, int64_t K, int64_t M, bool want_score, bool want_mask,
                                            bool want_y, OptDtype mask_dtype, OptDtype y_dtype) {
  const Tensor wc = prep(w, "wanda_nm");
  TORCH_CHECK(wc.dim() == 2, "wanda_nm: the weight must be a [rows, L] matrix");
  TORCH_CHECK(act_norm.is_cuda() && act_norm.device() == wc.device() && act_norm.scalar_type() == at::kFloat && act_norm.is_contiguous() &&
              act_norm.numel() == wc.size(1), "wanda_nm: act_norm must be a contiguous float32 tensor of ", wc.size(1),
              " entries on the weight's device");
  Tensor score = want_score ? empty_like_shape(wc, at::kFloat) : at::empty({0}, wc.options().dtype(at::kFloat));
  Tensor mask = want_mask ? empty_like_shape(wc, mask_dtype.value_or(at::kFloat)) : none_like(wc);
  Tensor y = want_y ? empty_like_shape(wc, y_dtype.value_or(at::promote_types(wc.scalar_type(), at::kFloat))) : none_like(wc);
  Launch l(wc);
  check(dmxq_wanda_nm(wc.data_ptr(), dt_code(wc.scalar_type()), (const float*)act_norm.data_ptr(), want_score ? (float*)score.data_ptr() : nullptr,
                      want_mask ? mask.data_ptr() : nullptr, want_mask ? dt_code(mask.scalar_type()) : 0, want_y ? y.data_ptr() : nullptr,
                      want_y ? dt_code(y.scalar_type()) : 0, wc.size(0), wc.size(1), (int)K, (int)M, l.stream), "dmxq_wanda_nm");
  return std::make_tuple(score, mask, y);
}
std::tuple<Tensor, Tensor, Tensor> wanda_nm_meta(const Tensor& w, const Tensor&, int64_t, int64_t, bool want_score, bool want_mask, bool want_y,
                                                 OptDtype mask_dtype, OptDtype y_dtype) {
  return std::make_tuple(want_score ? empty_like_shape(w, at::kFloat) : at::empty({0}, w.options().dtype(at::kFloat)),
                         want_mask ? empty_like_shape(w, mask_dtype.value_or(at::kFloat)) : none_like(w),
                         want_y ? empty_like_shape(w, y_dtype.value_or(at::promote_types(w.scalar_type(), at::kFloat))) : none_like(w));
}

// ------------------------------------------------------------------------------------------------ AWQ
// -> (d float32, wq in w's dtype): wq comes back as an empty 1-d tensor when it was not requested
std::tuple<Tensor, Tensor> awq_group_error(const Tensor& w, const Tensor& s, int64_t group, int64_t precision, int64_t fraction, bool clamp,
                                           bool symmetric, int64_t qmin, int64_t qmax, bool symmetric_qscheme, bool want_wq) {
  const Tensor wc = prep(w, "awq_group_error");
  TORCH_CHECK(wc.dim() == 2, "awq_group_error: the weight must be a [rows, L] matrix");
  TORCH_CHECK(s.is_cuda() && s.device() == wc.device() && s.scalar_type() == at::kFloat && s.is_contiguous() && s.numel() == wc.size(1),
              "awq_group_error: s must be a contiguous float32 tensor of ", wc.size(1), " entries on the weight's device");
  Tensor d = empty_like_shape(wc, at::kFloat);
  Tensor wq = want_wq ? empty_like_shape(wc, wc.scalar_type()) : none_like(wc);
  Launch l(wc);
  check(dmxq_awq_group_error(wc.data_ptr(), dt_code(wc.scalar_type()), (const float*)s.data_ptr(), (float*)d.data_ptr(),
                             want_wq ? wq.data_ptr() : nullptr, wc.size(0), wc.size(1), group, (int)precision, (int)fraction, clamp, symmetric,
                             (int)qmin, (int)qmax, symmetric_qscheme, l.stream), "dmxq_awq_group_error");
  return std::make_tuple(d, wq);
}
std::tuple<Tensor, Tensor> awq_group_error_meta(const Tensor& w, const Tensor&, int64_t, int64_t, int64_t, bool, bool, int64_t, int64_t, bool,
                                                bool want_wq) {
  return std::make_tuple(empty_like_shape(w, at::kFloat), want_wq ? empty_like_shape(w, w.scalar_type()) : none_like(w));
}

// y (w's dtype and shape, may be w itself) is written -> (best uint8 [rows, G], clip float32 [rows, G], losses float32 [rows, G, n]): empty
// 1-d tensors unless wanted.  DMXQ_ERR_UNSUPPORTED (NotImplementedError, nothing launched): the front end runs its chain.
std::tuple<Tensor, Tensor, Tensor> awq_clip(const Tensor& w, const Tensor& blocks, const Tensor& ratios, Tensor y, int64_t group, int64_t precision,
                                            int64_t fraction, bool clamp, bool symmetric, int64_t qmin, int64_t qmax, bool symmetric_qscheme,
                                            bool want_best, bool want_clip, bool want_losses) {
  const Tensor wc = prep(w, "awq_clip");
  TORCH_CHECK(wc.dim() == 2 && group >= 1 && wc.size(1) % group == 0, "awq_clip: the weight must be a [rows, L] matrix with the group size dividing L");
  const int64_t rows = wc.size(0), G = wc.size(1) / group, n = ratios.numel();
  TORCH_CHECK(blocks.is_cuda() && blocks.device() == wc.device() && blocks.scalar_type() == at::kFloat && blocks.is_contiguous() &&
                  blocks.dim() == 3 && blocks.size(0) == G && blocks.size(1) == group && blocks.size(2) == group,
              "awq_clip: blocks must be a contiguous float32 [", G, ", ", group, ", ", group, "] tensor on the weight's device");
  TORCH_CHECK(ratios.is_cuda() && ratios.device() == wc.device() && ratios.scalar_type() == at::kFloat && ratios.is_contiguous() && ratios.dim() == 1,
              "awq_clip: ratios must be a contiguous float32 [n] tensor on the weight's device");
  TORCH_CHECK(y.is_cuda() && y.device() == wc.device() && y.scalar_type() == wc.scalar_type() && y.is_contiguous() && y.sizes() == wc.sizes(),
              "awq_clip: y must be a contiguous tensor of the weight's dtype and shape on its device");
  Tensor best = want_best ? at::empty({rows, G}, wc.options().dtype(at::kByte)) : at::empty({0}, wc.options().dtype(at::kByte));
  Tensor clip = want_clip ? at::empty({rows, G}, wc.options().dtype(at::kFloat)) : at::empty({0}, wc.options().dtype(at::kFloat));
  Tensor losses = want_losses ? at::empty({rows, G, n}, wc.options().dtype(at::kFloat)) : at::empty({0}, wc.options().dtype(at::kFloat));
  Launch l(wc);
  check(dmxq_awq_clip(wc.data_ptr(), dt_code(wc.scalar_type()), (const float*)blocks.data_ptr(), (const float*)ratios.data_ptr(), (int)n, y.data_ptr(),
                      want_best ? (uint8_t*)best.data_ptr() : nullptr, want_clip ? (float*)clip.data_ptr() : nullptr,
                      want_losses ? (float*)losses.data_ptr() : nullptr, rows, wc.size(1), group, (int)precision, (int)fraction, clamp, symmetric,
                      (int)qmin, (int)qmax, symmetric_qscheme, l.stream), "dmxq_awq_clip");
  return std::make_tuple(best, clip, losses);
}
std::tuple<Tensor, Tensor, Tensor> awq_clip_meta(const Tensor& w, const Tensor&, const Tensor& ratios, Tensor, int64_t group, int64_t, int64_t, bool, bool,
                                                 int64_t, int64_t, bool, bool want_best, bool want_clip, bool want_losses) {
  const int64_t rows = w.size(0), G = group >= 1 ? w.size(1) / group : 0, n = ratios.numel();
  return std::make_tuple(want_best ? at::empty({rows, G}, w.options().dtype(at::kByte)) : at::empty({0}, w.options().dtype(at::kByte)),
                         want_clip ? at::empty({rows, G}, w.options().dtype(at::kFloat)) : at::empty({0}, w.options().dtype(at::kFloat)),
                         want_losses ? at::empty({rows, G, n}, w.options().dtype(at::kFloat)) : at::empty({0}, w.options().dtype(at::kFloat)));
}

// ------------------------------------------------------------------------------------------------ AdaRound
// w: contiguous, numel % segment == 0; V: contiguous float32 of w's element count; scale, zero_point: float32 [n_segments] (the zero
// points integers).  DMXQ_ERR_UNSUPPORTED (NotImplementedError, nothing launched): the front end runs its chain of torch operations.
static int64_t adaround_args(const Tensor& wc, const Tensor& V, const Tensor& scale, const Tensor& zero_point, int64_t segment, const char* what) {
  TORCH_CHECK(segment >= 1 && wc.numel() % segment == 0, what, ": the segment must divide the number of elements");
  const int64_t n = wc.numel() / segment;
  TORCH_CHECK(V.is_cuda() && V.device() == wc.device() && V.scalar_type() == at::kFloat && V.is_contiguous() && V.numel() == wc.numel(), what,
              ": V must be a contiguous float32 tensor of the weight's element count on its GPU");
  TORCH_CHECK(scale.is_cuda() && scale.device() == wc.device() && scale.scalar_type() == at::kFloat && scale.is_contiguous() && scale.numel() == n &&
              zero_point.is_cuda() && zero_point.device() == wc.device() && zero_point.scalar_type() == at::kFloat && zero_point.is_contiguous() &&
              zero_point.numel() == n, what, ": scale and zero_point must be contiguous float32 tensors of ", n, " entries on the weight's GPU");
  return n;
}
Tensor adaround_forward(const Tensor& w, const Tensor& V, const Tensor& scale, const Tensor& zero_point, int64_t segment, int64_t qmin, int64_t qmax,
                        bool hard, c10::optional<at::ScalarType> out_dtype) {
  const Tensor wc = prep(w, "adaround_forward");
  const int64_t n = adaround_args(wc, V, scale, zero_point, segment, "adaround_forward");
  Tensor y = empty_like_shape(wc, out_dtype);
  Launch l(wc);
  check(dmxq_adaround_forward(wc.data_ptr(), (const float*)V.data_ptr(), y.data_ptr(), dt_code(wc.scalar_type()), dt_code(y.scalar_type()), n, segment,
                              (int)qmin, (int)qmax, (const float*)scale.data_ptr(), (const float*)zero_point.data_ptr(), hard ? 1 : 0, l.stream),
        "dmxq_adaround_forward");
  return y;
}
Tensor adaround_forward_meta(const Tensor& w, const Tensor&, const Tensor&, const Tensor&, int64_t, int64_t, int64_t, bool,
                             c10::optional<at::ScalarType> out_dtype) {
  return empty_like_shape(w, out_dtype);
}
// -> (dV float32 in w's shape; reg float64 [1], empty unless want_reg: then no sum is formed).  The partial sums' scratch is allocated here.
std::tuple<Tensor, Tensor> adaround_backward(const Tensor& w, const Tensor& V, const Tensor& g, const Tensor& scale, const Tensor& zero_point,
                                             int64_t segment, int64_t qmin, int64_t qmax, double beta, double reg_weight, bool want_reg) {
  const Tensor wc = prep(w, "adaround_backward"), gc = prep(g, "adaround_backward");
  TORCH_CHECK(gc.device() == wc.device() && gc.numel() == wc.numel(), "adaround_backward: w and g must hold the same number of elements on one device");
  const int64_t n = adaround_args(wc, V, scale, zero_point, segment, "adaround_backward");
  Tensor dV = empty_like_shape(wc, at::kFloat);
  Tensor reg = at::empty({want_reg ? 1 : 0}, wc.options().dtype(at::kDouble));
  const int64_t sb = want_reg ? dmxq_adaround_scratch_bytes(wc.numel()) : 0;
  Tensor scratch = at::empty({sb / 8}, wc.options().dtype(at::kDouble));
  Launch l(wc);
  check(dmxq_adaround_backward(wc.data_ptr(), (const float*)V.data_ptr(), gc.data_ptr(), (float*)dV.data_ptr(), dt_code(wc.scalar_type()),
                               dt_code(gc.scalar_type()), n, segment, (int)qmin, (int)qmax, (const float*)scale.data_ptr(),
                               (const float*)zero_point.data_ptr(), (float)beta, (float)reg_weight, want_reg ? (double*)reg.data_ptr() : nullptr,
                               sb ? scratch.data_ptr() : nullptr, sb, l.stream),
        "dmxq_adaround_backward");
  return std::make_tuple(dV, reg);
}
std::tuple<Tensor, Tensor> adaround_backward_meta(const Tensor& w, const Tensor&, const Tensor&, const Tensor&, const Tensor&, int64_t, int64_t, int64_t,
                                                  double, double, bool want_reg) {
  return std::make_tuple(empty_like_shape(w, at::kFloat), at::empty({want_reg ? 1 : 0}, w.options().dtype(at::kDouble)));
}

// ------------------------------------------------------------------------------------------------ block-scaled float cast
// x: contiguous; groups of `group` consecutive elements; fmt / scale_fmt: (man, exp, bias, flush, rounding); tensor_scale: None (t = 1) or
// ONE float32 on x's device, read by the kernel only -> (out, scale, scale_code_value: float32 [n_groups], empty unless wanted).
// DMXQ_ERR_UNSUPPORTED (NotImplementedError, nothing launched): the front end runs its chain of launches.
std::tuple<Tensor, Tensor, Tensor> block_scaled_float_qdq(const Tensor& x, int64_t group, at::IntArrayRef fmt, at::IntArrayRef scale_fmt,
                                                          double scale_max, const OptTensor& tensor_scale, bool want_scale, bool want_code,
                                                          OptDtype out_dtype) {
  const Tensor xc = prep(x, "block_scaled_float_qdq");
  TORCH_CHECK(fmt.size() == 5 && scale_fmt.size() == 5, "block_scaled_float_qdq: a format is (man, exp, bias, flush, rounding)");
  TORCH_CHECK(group >= 1 && xc.numel() % group == 0, "block_scaled_float_qdq: the group must divide the number of elements");
  const float* tp = nullptr;
  if (tensor_scale.has_value() && tensor_scale->defined()) {
    const Tensor& t = *tensor_scale;
    TORCH_CHECK(t.is_cuda() && t.device() == xc.device() && t.scalar_type() == at::kFloat && t.numel() == 1,
                "block_scaled_float_qdq: tensor_scale must be ONE float32 on the input's device");
    tp = (const float*)t.data_ptr();
  }
  const int64_t n = xc.numel() / group;
  Tensor out = empty_like_shape(xc, out_dtype);
  Tensor sc = at::empty({want_scale ? n : 0}, xc.options().dtype(at::kFloat));
  Tensor sq = at::empty({want_code ? n : 0}, xc.options().dtype(at::kFloat));
  Launch l(xc);
  check(dmxq_block_scaled_float_qdq(xc.data_ptr(), out.data_ptr(), dt_code(xc.scalar_type()), dt_code(out.scalar_type()), n, group, (int)fmt[0],
                                    (int)fmt[1], (int)fmt[2], (int)fmt[3], (int)fmt[4], (int)scale_fmt[0], (int)scale_fmt[1], (int)scale_fmt[2],
                                    (int)scale_fmt[3], (int)scale_fmt[4], (float)scale_max, tp, want_scale ? (float*)sc.data_ptr() : nullptr,
                                    want_code ? (float*)sq.data_ptr() : nullptr, l.stream), "dmxq_block_scaled_float_qdq");
  return std::make_tuple(out, sc, sq);
}
// the dynamic tensor scale of a contiguous tensor -> float32 [1] on its device (DMXQ_ERR_UNSUPPORTED: the front end's group_minmax route)
Tensor block_scaled_tensor_scale(const Tensor& x, double fmax, double scale_max) {
  const Tensor xc = prep(x, "block_scaled_tensor_scale");
  Tensor t = at::empty({1}, xc.options().dtype(at::kFloat));
  Launch l(xc);
  check(dmxq_block_scaled_tensor_scale(xc.data_ptr(), dt_code(xc.scalar_type()), xc.numel(), (float)fmax, (float)scale_max, (float*)t.data_ptr(),
                                       l.stream), "dmxq_block_scaled_tensor_scale");
  return t;
}
Tensor block_scaled_tensor_scale_meta(const Tensor& x, double, double) { return at::empty({1}, x.options().dtype(at::kFloat)); }
std::tuple<Tensor, Tensor, Tensor> block_scaled_float_qdq_meta(const Tensor& x, int64_t group, at::IntArrayRef, at::IntArrayRef, double,
                                                               const OptTensor&, bool want_scale, bool want_code, OptDtype out_dtype) {
  TORCH_CHECK(group >= 1 && x.numel() % group == 0, "block_scaled_float_qdq: the group must divide the number of elements");
  const int64_t n = x.numel() / group;
  return std::make_tuple(empty_like_shape(x, out_dtype), at::empty({want_scale ? n : 0}, x.options().dtype(at::kFloat)),
                         at::empty({want_code ? n : 0}, x.options().dtype(at::kFloat)));
}

}  // namespace

TORCH_LIBRARY(dmxq, m) {
  m.def("bfp_qdq(Tensor x, int precision, int block_size, int block_dim=-1, bool symmetric=True, int rounding=2, ScalarType? out_dtype=None, int seed=0) -> Tensor");
  m.def("bfp_qdq_nograd(Tensor x, int precision, int block_size, int block_dim=-1, bool symmetric=True, int rounding=2, ScalarType? out_dtype=None, int seed=0) -> Tensor");  // the same kernel without the Python STE autograd wrapper (2.5 us per call)
  m.def("block_quantize(Tensor a, int wl, bool symmetric, int rounding, int seed=0) -> Tensor");
  m.def("weight_hypernet_multi(Tensor[] ws, int precision, int block_size, bool symmetric, Tensor[] scores, int K, int M, Tensor[] sq_scales, ScalarType? out_dtype=None) -> Tensor[]");
  m.def("bfp_qdq_multi(Tensor[] xs, int precision, int block_size, int block_dim=-1, bool symmetric=True, int rounding=2, ScalarType? out_dtype=None, int seed=0) -> Tensor[]");
  m.def("bfp_pack(Tensor x, int precision, int block_size, bool symmetric=True) -> (Tensor, Tensor)");
  m.def("bfp_unpack(Tensor mant, Tensor exps, int precision, int block_size, ScalarType out_dtype) -> Tensor");
  m.def("weight_hypernet(Tensor w, int precision, int block_size, bool symmetric, Tensor? score, int K, int M, Tensor? sq_scale, ScalarType? out_dtype=None, int block_dim=-1) -> Tensor");
  m.def("input_hypernet(Tensor x, Tensor sq_scale, int precision, int block_size, bool symmetric) -> Tensor");
  m.def("binary_cast(Tensor a, Tensor b, int op, int[] cast_a, int[] cast_b, int[] cast_out, int bfp_block=0, int bfp_precision=0) -> Tensor");
  m.def("relu_cast(Tensor x, int[] cast_in, int[] cast_out, int bfp_block=0, int bfp_precision=0) -> Tensor");
  m.def("sbfp_qdq(Tensor x, int precision, int block_size, int scaler_man, int scaler_exp, int scaler_bias, bool scaler_flush, bool clamp, bool symmetric, int block_dim=-1, ScalarType? out_dtype=None) -> Tensor");
  m.def("sbfp_qdq_nograd(Tensor x, int precision, int block_size, int scaler_man, int scaler_exp, int scaler_bias, bool scaler_flush, bool clamp, bool symmetric, int block_dim=-1, ScalarType? out_dtype=None) -> Tensor");
  m.def("mxfp_qdq(Tensor x, int man, int exp, int block_size, int block_dim=-1, ScalarType? out_dtype=None) -> Tensor");
  m.def("mxfp_qdq_nograd(Tensor x, int man, int exp, int block_size, int block_dim=-1, ScalarType? out_dtype=None) -> Tensor");
  m.def("float_qdq(Tensor x, int man, int exp, int bias, bool flush_subnormal, bool unsigned_abs=False, int rounding=2, ScalarType? out_dtype=None, int seed=0) -> Tensor");
  m.def("float_qdq_nograd(Tensor x, int man, int exp, int bias, bool flush_subnormal, bool unsigned_abs=False, int rounding=2, ScalarType? out_dtype=None, int seed=0) -> Tensor");  // the same kernel without the Python STE autograd wrapper (2.5 us per call)
  m.def("fixed_qdq(Tensor x, int precision, int fraction, bool clamp, bool symmetric, int rounding, Tensor? scale, Tensor? zero_point, int? ch_axis, int? group_size, ScalarType? out_dtype=None, int seed=0) -> Tensor");
  m.def("fixed_qdq_nograd(Tensor x, int precision, int fraction, bool clamp, bool symmetric, int rounding, Tensor? scale, Tensor? zero_point, int? ch_axis, int? group_size, ScalarType? out_dtype=None, int seed=0) -> Tensor");  // the same kernel without the Python STE autograd wrapper (2.5 us per call)
  m.def("float_qdq_multi(Tensor[] xs, int man, int exp, int bias, bool flush_subnormal, bool unsigned_abs=False, int rounding=2, ScalarType? out_dtype=None, int seed=0) -> Tensor[]");
  m.def("fixed_float_qdq_multi(Tensor[] xs, int precision, int fraction, bool clamp, bool symmetric, int rounding, Tensor[] scales, Tensor[] zero_points, int group_size, Tensor[] fs, int man, int exp, int bias, bool flush_subnormal, bool unsigned_abs, int rounding_float, int seed=0) -> (Tensor[], Tensor[])");
  m.def("fixed_qdq_multi(Tensor[] xs, int precision, int fraction, bool clamp, bool symmetric, int rounding, Tensor[] scales, Tensor[] zero_points, int group_size, ScalarType? out_dtype=None, int seed=0) -> Tensor[]");
  m.def("nm_mask(Tensor score, Tensor? x, int K, int M, int block_dim, bool want_mask, bool want_y, ScalarType? mask_dtype=None, ScalarType? y_dtype=None) -> (Tensor, Tensor)");
  m.def("topk_mask(Tensor score, Tensor? x, int n_zero, bool want_mask, bool want_y, ScalarType? mask_dtype=None, ScalarType? y_dtype=None) -> (Tensor, Tensor)");
  m.def("bernoulli_mask(Tensor score, int seed, ScalarType? mask_dtype=None) -> Tensor");
  m.def("group_minmax(Tensor x, int ch_axis, int group_size) -> (Tensor, Tensor)");
  m.def("group_minmax_accumulate(Tensor x, int ch_axis, int group_size, Tensor(a!) mn, Tensor(b!) mx) -> ()");
  m.def("qparams(Tensor mn, Tensor mx, int qmin, int qmax, bool symmetric_qscheme) -> (Tensor, Tensor)");
  m.def("histc(Tensor x, int bins, float lo, float hi) -> Tensor");
  m.def("channel_maxabs(Tensor x, int ch_axis) -> Tensor");
  m.def("smoothquant_scale(Tensor a_maxabs, Tensor b_maxabs, float alpha, float scale_min) -> Tensor");
  m.def("scale_channels(Tensor x, Tensor scale, int ch_axis, bool divide, ScalarType? out_dtype=None) -> Tensor");
  m.def("unary(Tensor x, int kind, float param=0.0, ScalarType? out_dtype=None) -> Tensor");
  m.def("rope(Tensor x, Tensor cos, Tensor sin, int unsqueeze_dim=1) -> Tensor");
  m.def("rope_cast(Tensor x, Tensor cos, Tensor sin, int unsqueeze_dim, int[] cast_x, int[] cast_cos, int[] cast_sin, int[] cast_out) -> Tensor");
  m.def("softmax(Tensor x, float clamp_min, ScalarType? out_dtype=None) -> Tensor");
  m.def("norm(Tensor x, int cols, Tensor? weight, Tensor? bias, float eps, int kind, ScalarType? out_dtype=None) -> Tensor");
  m.def("unary_cast(Tensor x, int kind, float param, int[] cast_in, int[] cast_out) -> Tensor");
  m.def("softmax_cast(Tensor x, float clamp_min, int[] cast_in, int[] cast_out, int bfp_block=0, int bfp_precision=0) -> Tensor");
  m.def("unary_cast_table(Tensor like, int kind, float param, int[] cast_in, int[] cast_out) -> Tensor");
  m.def("lut16_apply(Tensor x, Tensor table) -> Tensor");
  m.def("norm_cast(Tensor x, int cols, Tensor? weight, Tensor? bias, float eps, int kind, int[] cast_in, int[] cast_out, int bfp_block=0, int bfp_precision=0) -> Tensor");
  m.def("gptq_block(Tensor w, Tensor hinv, Tensor inv_d, int microblock, int[] fmt, Tensor? scale, Tensor? zero_point, Tensor(a!) q, Tensor(b!) err) -> ()");
  m.def("gptq_block_dynamic(Tensor w, Tensor hinv, Tensor inv_d, int microblock, int[] fmt, int rounding, int group, int qmin, int qmax, bool symmetric_qscheme, Tensor(a!) q, Tensor(b!) err, Tensor(c!) scale_out, Tensor(d!) zp_out) -> ()");
  m.def("hist_observe(Tensor x, int ch_axis, int group_size, int upsample_rate, Tensor(a!) hist, Tensor(b!) min_val, Tensor(c!) max_val, Tensor(d!) status, Tensor(e!) scratch) -> ()");
  m.def("hist_qparams(Tensor hist, Tensor min_val, Tensor max_val, int precision, int qmin, int qmax, bool symmetric_qscheme) -> (Tensor, Tensor)");
  m.def("error_stats(Tensor ref, Tensor test, bool accumulate, Tensor(a!) stats, Tensor(b!) scratch) -> ()");
  m.def("cast_error(Tensor x, int[] fmts, Tensor? scale, Tensor? zero_point, bool accumulate, Tensor(a!) stats, Tensor(b!) scratch) -> ()");
  m.def("hadamard_qdq(Tensor x, int size, bool inverse, int[] fmt, Tensor? scale, Tensor? zero_point, ScalarType? out_dtype=None) -> Tensor");
  m.def("dynamic_fixed_qdq(Tensor x, int segment, bool whole_rows, int precision, int fraction, bool clamp, bool symmetric, int rounding, int qmin, int qmax, bool symmetric_qscheme, bool want_qparams, ScalarType? out_dtype=None) -> (Tensor, Tensor, Tensor)");
  m.def("dynamic_float_qdq(Tensor x, int mode, int segment, int man, int exp, int bias, bool flush_subnormal, int rounding, bool pow2_scale, bool want_scale, ScalarType? out_dtype=None) -> (Tensor, Tensor)");
  m.def("channel_sumsq(Tensor x, Tensor(a!) acc, Tensor(b!) scratch) -> ()");
  m.def("wanda_nm(Tensor w, Tensor act_norm, int K, int M, bool want_score, bool want_mask, bool want_y, ScalarType? mask_dtype=None, ScalarType? y_dtype=None) -> (Tensor, Tensor, Tensor)");
  m.def("channel_sumabs(Tensor x, Tensor(a!) acc, Tensor(b!) scratch) -> ()");
  m.def("awq_group_error(Tensor w, Tensor s, int group, int precision, int fraction, bool clamp, bool symmetric, int qmin, int qmax, bool symmetric_qscheme, bool want_wq) -> (Tensor, Tensor)");
  m.def("awq_clip(Tensor w, Tensor blocks, Tensor ratios, Tensor(a!) y, int group, int precision, int fraction, bool clamp, bool symmetric, int qmin, int qmax, bool symmetric_qscheme, bool want_best, bool want_clip, bool want_losses) -> (Tensor, Tensor, Tensor)");
  m.def("block_scaled_float_qdq(Tensor x, int group, int[] fmt, int[] scale_fmt, float scale_max, Tensor? tensor_scale, bool want_scale, bool want_code, ScalarType? out_dtype=None) -> (Tensor, Tensor, Tensor)");
  m.def("block_scaled_tensor_scale(Tensor x, float fmax, float scale_max) -> Tensor");
  m.def("lsq_backward(Tensor x, Tensor g, Tensor scale, Tensor zero_point, int segment, int whole_rows, int precision, int rounding, int qmin, int qmax, float grad_factor, bool want_dz, bool want_dx) -> (Tensor, Tensor, Tensor)");
  m.def("codebook_qdq(Tensor x, int mode, int segment, Tensor levels, float norm, bool want_scale, bool want_index, ScalarType? out_dtype=None) -> (Tensor, Tensor, Tensor)");
  m.def("codebook_accumulate(Tensor x, int mode, int segment, Tensor levels, float norm, Tensor(a!) acc, bool accumulate) -> ()");
  m.def("vq_qdq(Tensor x, int mode, int segment, Tensor table, float norm, bool want_scale, bool want_index, ScalarType? out_dtype=None) -> (Tensor, Tensor, Tensor)");
  m.def("vq_accumulate(Tensor x, int mode, int segment, Tensor table, float norm, Tensor(a!) acc, bool accumulate) -> ()");
  m.def("hqq_qdq(Tensor x, int segment, int rounding, int qmin, int qmax, float lp_norm, float beta, float kappa, int iters, bool want_qparams, bool want_codes, ScalarType? out_dtype=None) -> (Tensor, Tensor, Tensor, Tensor)");
  m.def("outlier_fixed_qdq(Tensor x, int segment, int k, int precision, int fraction, bool clamp, bool symmetric, int rounding, int qmin, int qmax, bool symmetric_qscheme, int[] outlier_fmt, bool want_qparams, bool want_outliers, ScalarType? out_dtype=None) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
  m.def("adaround_forward(Tensor w, Tensor V, Tensor scale, Tensor zero_point, int segment, int qmin, int qmax, bool hard, ScalarType? out_dtype=None) -> Tensor");
  m.def("adaround_backward(Tensor w, Tensor V, Tensor g, Tensor scale, Tensor zero_point, int segment, int qmin, int qmax, float beta, float reg_weight, bool want_reg) -> (Tensor, Tensor)");
}

#define DMXQ_IMPL(m, name) m.impl(#name, &name)
#define DMXQ_META(m, name) m.impl(#name, &name##_meta)
#define DMXQ_FOR_ALL(X, m) \
  X(m, bfp_qdq); X(m, block_quantize); X(m, bfp_qdq_multi); X(m, weight_hypernet_multi); X(m, bfp_pack); X(m, bfp_unpack); X(m, weight_hypernet); X(m, input_hypernet); X(m, binary_cast); X(m, relu_cast); X(m, sbfp_qdq); X(m, mxfp_qdq);   \
  X(m, float_qdq); X(m, float_qdq_multi); X(m, fixed_qdq); X(m, fixed_qdq_multi); X(m, fixed_float_qdq_multi); X(m, nm_mask); X(m, topk_mask); X(m, bernoulli_mask); X(m, group_minmax); X(m, qparams); \
  X(m, histc); X(m, channel_maxabs); X(m, smoothquant_scale); X(m, scale_channels); X(m, unary); X(m, rope); X(m, rope_cast); X(m, softmax); X(m, norm); \
  X(m, unary_cast); X(m, unary_cast_table); X(m, lut16_apply); X(m, softmax_cast); X(m, norm_cast); X(m, group_minmax_accumulate); X(m, gptq_block); X(m, hist_observe); X(m, hist_qparams); \
  X(m, error_stats); X(m, cast_error); X(m, hadamard_qdq); X(m, dynamic_fixed_qdq); X(m, gptq_block_dynamic); X(m, dynamic_float_qdq); \
  X(m, channel_sumsq); X(m, wanda_nm); X(m, channel_sumabs); X(m, awq_group_error); X(m, block_scaled_float_qdq); X(m, block_scaled_tensor_scale); \
  X(m, lsq_backward); X(m, codebook_qdq); X(m, codebook_accumulate); X(m, hqq_qdq); X(m, outlier_fixed_qdq); X(m, awq_clip); \
  X(m, adaround_forward); X(m, adaround_backward); X(m, vq_qdq); X(m, vq_accumulate)

// "CUDA" is the dispatch key of HIP tensors in a ROCm build of PyTorch
TORCH_LIBRARY_IMPL(dmxq, CUDA, m) {
  DMXQ_FOR_ALL(DMXQ_IMPL, m);
  m.impl("bfp_qdq_nograd", &bfp_qdq); m.impl("float_qdq_nograd", &float_qdq); m.impl("fixed_qdq_nograd", &fixed_qdq);
  m.impl("sbfp_qdq_nograd", &sbfp_qdq); m.impl("mxfp_qdq_nograd", &mxfp_qdq);
}
TORCH_LIBRARY_IMPL(dmxq, Meta, m) {
  DMXQ_FOR_ALL(DMXQ_META, m);
  m.impl("bfp_qdq_nograd", &bfp_qdq_meta); m.impl("float_qdq_nograd", &float_qdq_meta); m.impl("fixed_qdq_nograd", &fixed_qdq_meta);
  m.impl("sbfp_qdq_nograd", &sbfp_qdq_meta); m.impl("mxfp_qdq_nograd", &mxfp_qdq_meta);
}

// ---------------------------------------------------------------------------------------------------- direct entry points (round 6)
// The SAME C++ functions as the dispatcher's CUDA kernels above, callable from Python without the dispatcher: `PyInit_dmxq_fast` lives in
// this shared object next to the TORCH_LIBRARY registration (dmx-compressor_amd/_backend_torch.py loads both).  A `torch.ops.dmxq.*` call
// costs ~2 us of schema matching, boxing and dispatch on top of the launch (5.9 us against 4.0-4.4 for the C-ABI call through ctypes,
// profiles/r06_host_overhead.txt), 26 times per forward of an opt-125m decoder layer; eager INFERENCE calls -- no autograd, no tracing:
// _backend_torch.py falls back to the dispatcher op while torch.compile traces -- take these.  Same checks, same errors (c10::Error ->
// RuntimeError, c10::NotImplementedError -> NotImplementedError through torch's pybind exception translator), same results.
#include <pybind11/stl.h>
#include <torch/csrc/utils/pybind.h>

PYBIND11_MODULE(dmxq_fast, m) {
  namespace py = pybind11;
  m.doc() = "dispatcher-free entry points of dmxq_torch.so (eager inference calls; see csrc/torch_binding.cpp)";
  m.def("bfp_qdq", &bfp_qdq, py::arg("x"), py::arg("precision"), py::arg("block_size"), py::arg("block_dim") = -1, py::arg("symmetric") = true,
        py::arg("rounding") = 2, py::arg("out_dtype") = py::none(), py::arg("seed") = 0);
  m.def("float_qdq", &float_qdq, py::arg("x"), py::arg("man"), py::arg("exp"), py::arg("bias"), py::arg("flush_subnormal"), py::arg("unsigned_abs") = false,
        py::arg("rounding") = 2, py::arg("out_dtype") = py::none(), py::arg("seed") = 0);
  m.def("fixed_qdq", &fixed_qdq, py::arg("x"), py::arg("precision"), py::arg("fraction"), py::arg("clamp"), py::arg("symmetric"), py::arg("rounding"),
        py::arg("scale"), py::arg("zero_point"), py::arg("ch_axis"), py::arg("group_size"), py::arg("out_dtype") = py::none(), py::arg("seed") = 0);
  m.def("sbfp_qdq", &sbfp_qdq, py::arg("x"), py::arg("precision"), py::arg("block_size"), py::arg("scaler_man"), py::arg("scaler_exp"), py::arg("scaler_bias"),
        py::arg("scaler_flush"), py::arg("clamp"), py::arg("symmetric"), py::arg("block_dim") = -1, py::arg("out_dtype") = py::none());
  m.def("mxfp_qdq", &mxfp_qdq, py::arg("x"), py::arg("man"), py::arg("exp"), py::arg("block_size"), py::arg("block_dim") = -1, py::arg("out_dtype") = py::none());
  m.def("weight_hypernet", &weight_hypernet, py::arg("w"), py::arg("precision"), py::arg("block_size"), py::arg("symmetric"), py::arg("score"), py::arg("K"),
        py::arg("M"), py::arg("sq_scale"), py::arg("out_dtype") = py::none(), py::arg("block_dim") = -1);
  m.def("input_hypernet", &input_hypernet);
  m.def("binary_cast", &binary_cast, py::arg("a"), py::arg("b"), py::arg("op"), py::arg("cast_a"), py::arg("cast_b"), py::arg("cast_out"),
        py::arg("bfp_block") = 0, py::arg("bfp_precision") = 0);
  m.def("relu_cast", &relu_cast, py::arg("x"), py::arg("cast_in"), py::arg("cast_out"), py::arg("bfp_block") = 0, py::arg("bfp_precision") = 0);
  m.def("scale_channels", &scale_channels, py::arg("x"), py::arg("scale"), py::arg("ch_axis"), py::arg("divide"), py::arg("out_dtype") = py::none());
  m.def("rope_cast", &rope_cast);
  m.def("unary_cast", &unary_cast);
  m.def("lut16_apply", &lut16_apply);
  m.def("softmax_cast", &softmax_cast, py::arg("x"), py::arg("clamp_min"), py::arg("cast_in"), py::arg("cast_out"), py::arg("bfp_block") = 0,
        py::arg("bfp_precision") = 0);
  m.def("norm_cast", &norm_cast, py::arg("x"), py::arg("cols"), py::arg("weight"), py::arg("bias"), py::arg("eps"), py::arg("kind"), py::arg("cast_in"),
        py::arg("cast_out"), py::arg("bfp_block") = 0, py::arg("bfp_precision") = 0);
  m.def("hist_observe", &hist_observe);
  m.def("hist_qparams", &hist_qparams);
  m.def("error_stats", &error_stats);
  m.def("cast_error", &cast_error);
  m.def("hadamard_qdq", &hadamard_qdq, py::arg("x"), py::arg("size"), py::arg("inverse"), py::arg("fmt"), py::arg("scale"), py::arg("zero_point"),
        py::arg("out_dtype") = py::none());
  m.def("dynamic_fixed_qdq", &dynamic_fixed_qdq, py::arg("x"), py::arg("segment"), py::arg("whole_rows"), py::arg("precision"), py::arg("fraction"),
        py::arg("clamp"), py::arg("symmetric"), py::arg("rounding"), py::arg("qmin"), py::arg("qmax"), py::arg("symmetric_qscheme"),
        py::arg("want_qparams"), py::arg("out_dtype") = py::none());
  m.def("dynamic_float_qdq", &dynamic_float_qdq, py::arg("x"), py::arg("mode"), py::arg("segment"), py::arg("man"), py::arg("exp"), py::arg("bias"),
        py::arg("flush_subnormal"), py::arg("rounding"), py::arg("pow2_scale"), py::arg("want_scale"), py::arg("out_dtype") = py::none());
  m.def("block_scaled_float_qdq", &block_scaled_float_qdq, py::arg("x"), py::arg("group"), py::arg("fmt"), py::arg("scale_fmt"), py::arg("scale_max"),
        py::arg("tensor_scale"), py::arg("want_scale"), py::arg("want_code"), py::arg("out_dtype") = py::none());
  m.def("block_scaled_tensor_scale", &block_scaled_tensor_scale);
  m.def("lsq_backward", &lsq_backward);
  m.def("codebook_qdq", &codebook_qdq, py::arg("x"), py::arg("mode"), py::arg("segment"), py::arg("levels"), py::arg("norm"), py::arg("want_scale"),
        py::arg("want_index"), py::arg("out_dtype") = py::none());
  m.def("codebook_accumulate", &codebook_accumulate);
  m.def("vq_qdq", &vq_qdq, py::arg("x"), py::arg("mode"), py::arg("segment"), py::arg("table"), py::arg("norm"), py::arg("want_scale"),
        py::arg("want_index"), py::arg("out_dtype") = py::none());
  m.def("vq_accumulate", &vq_accumulate);
  m.def("hqq_qdq", &hqq_qdq, py::arg("x"), py::arg("segment"), py::arg("rounding"), py::arg("qmin"), py::arg("qmax"), py::arg("lp_norm"), py::arg("beta"),
        py::arg("kappa"), py::arg("iters"), py::arg("want_qparams"), py::arg("want_codes"), py::arg("out_dtype") = py::none());
  m.def("outlier_fixed_qdq", &outlier_fixed_qdq, py::arg("x"), py::arg("segment"), py::arg("k"), py::arg("precision"), py::arg("fraction"), py::arg("clamp"),
        py::arg("symmetric"), py::arg("rounding"), py::arg("qmin"), py::arg("qmax"), py::arg("symmetric_qscheme"), py::arg("outlier_fmt"),
        py::arg("want_qparams"), py::arg("want_outliers"), py::arg("out_dtype") = py::none());
  m.def("awq_clip", &awq_clip);
  m.def("adaround_forward", &adaround_forward, py::arg("w"), py::arg("V"), py::arg("scale"), py::arg("zero_point"), py::arg("segment"), py::arg("qmin"),
        py::arg("qmax"), py::arg("hard"), py::arg("out_dtype") = py::none());
  m.def("adaround_backward", &adaround_backward);
}
