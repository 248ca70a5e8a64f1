// PyTorch bindings for the gfx950 kernel library (module `smdt_amd._C`).
//
// This is the only translation unit that sees ATen. Each binding validates shapes / dtypes /
// contiguity on the host (a kernel is never launched on operands it does not expect), allocates
// outputs through the caching allocator, and forwards raw pointers plus the current HIP stream
// to the C launchers in kernels/launchers.h.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <c10/hip/HIPGuard.h>

#include "kernels/launchers.h"

namespace {

using torch::Tensor;
using OptT = std::optional<Tensor>;

hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

int dcode(const Tensor& t) {
  switch (t.scalar_type()) {
    case at::kFloat: return 0;
    case at::kBFloat16: return 1;
    case at::kHalf: return 2;
    default: TORCH_CHECK(false, "smdt_amd: unsupported dtype ", t.scalar_type());
  }
}

void check(hipError_t e, const char* what) {
  TORCH_CHECK(e == hipSuccess, "smdt_amd kernel '", what, "' failed: ", hipGetErrorString(e));
}

void need_cuda(const Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), "smdt_amd: '", name, "' must be a GPU tensor");
}

void need_contig(const Tensor& t, const char* name) {
  need_cuda(t, name);
  TORCH_CHECK(t.is_contiguous(), "smdt_amd: '", name, "' must be contiguous");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, "smdt_amd: '", name,
              "' must be 16-byte aligned");
}

const void* optr(const OptT& t) { return t.has_value() ? t->data_ptr() : nullptr; }

// ------------------------------------------------------------------ LayerNorm / RMSNorm
// out_y (optional): a contiguous tensor of x's size and dtype the normalised output is written
// into — a slice of a sequence-parallel all-gather buffer, so the gather needs no local copy.
static Tensor out_or_new(const OptT& out, const Tensor& like, const char* n) {
  if (!out) return torch::empty_like(like);
  TORCH_CHECK(out->is_contiguous() && out->numel() == like.numel() && out->dtype() == like.dtype() &&
                  out->device() == like.device(),
              n, ": output buffer must be contiguous with the input's size, dtype and device");
  return out->view(like.sizes());
}

std::vector<Tensor> layernorm_fwd(Tensor x, OptT res, OptT bias, Tensor gamma, OptT beta,
                                  double eps, double p_drop, int64_t seed, int64_t offset,
                                  bool rms, bool want_s, OptT out_y, OptT x2) {
  need_contig(x, "x");
  need_contig(gamma, "gamma");
  const int64_t H = x.size(-1);
  const int64_t rows = x.numel() / H;
  TORCH_CHECK(gamma.numel() == H, "layernorm: gamma size mismatch");
  if (res) { need_contig(*res, "residual"); TORCH_CHECK(res->sizes() == x.sizes() && res->dtype() == x.dtype(), "layernorm: residual mismatch"); }
  if (bias) { need_contig(*bias, "bias"); TORCH_CHECK(bias->numel() == H && bias->dtype() == gamma.dtype(), "layernorm: bias mismatch"); }
  if (beta) { need_contig(*beta, "beta"); TORCH_CHECK(beta->numel() == H && beta->dtype() == gamma.dtype(), "layernorm: beta mismatch"); }
  if (x2) { need_contig(*x2, "x2"); TORCH_CHECK(x2->sizes() == x.sizes() && x2->dtype() == x.dtype(), "layernorm: x2 mismatch"); }
  auto y = out_or_new(out_y, x, "layernorm_fwd");
  Tensor s;
  const bool make_s = want_s || res.has_value() || bias.has_value() || p_drop > 0.0 || x2.has_value();
  if (make_s) s = torch::empty_like(x);
  auto f32 = x.options().dtype(at::kFloat);
  auto mean = torch::empty({rows}, f32);
  auto rstd = torch::empty({rows}, f32);
  check(smdt_layernorm_fwd(dcode(x), dcode(gamma), x.data_ptr(), optr(res), optr(bias),
                           gamma.data_ptr(), optr(beta), y.data_ptr(),
                           make_s ? s.data_ptr() : nullptr, mean.data_ptr<float>(),
                           rstd.data_ptr<float>(), rows, (int)H, (float)eps, (float)p_drop,
                           (uint64_t)seed, (uint64_t)offset, rms ? 1 : 0, optr(x2), cur_stream()),
        "layernorm_fwd");
  return {y, make_s ? s : x, mean, rstd};
}

// dgamma_acc / dbeta_acc / dbias_acc (optional): fp32 [H] buffers (DDP main_grad views) the
// parameter gradients are ACCUMULATED into instead of being returned.
static Tensor acc_target(const OptT& t, int64_t H, const char* n) {
  if (!t) return Tensor();
  TORCH_CHECK(t->scalar_type() == at::kFloat && t->is_contiguous() && t->numel() == H, n,
              ": accumulate target must be a contiguous fp32 tensor of ", H, " elements");
  return *t;
}

std::vector<Tensor> layernorm_bwd(Tensor dy, OptT ds_in, Tensor s, Tensor gamma, Tensor mean,
                                  Tensor rstd, double p_drop, int64_t seed, int64_t offset,
                                  bool rms, bool want_dx, bool want_dbias, OptT dgamma_acc,
                                  OptT dbeta_acc, OptT dbias_acc, OptT out_dx, OptT dy2) {
  need_contig(dy, "dy");
  need_contig(s, "s");
  need_contig(gamma, "gamma");
  const int64_t H = s.size(-1);
  const int64_t rows = s.numel() / H;
  TORCH_CHECK(dy.sizes() == s.sizes() && dy.dtype() == s.dtype(), "layernorm_bwd: dy mismatch");
  if (ds_in) { need_contig(*ds_in, "ds_in"); TORCH_CHECK(ds_in->sizes() == s.sizes() && ds_in->dtype() == s.dtype(), "layernorm_bwd: ds_in mismatch"); }
  if (dy2) { need_contig(*dy2, "dy2"); TORCH_CHECK(dy2->sizes() == s.sizes() && dy2->dtype() == s.dtype(), "layernorm_bwd: dy2 mismatch"); }
  // out_dx (optional): where dx goes (a slice of an all-gather buffer, see layernorm_fwd); without
  // dropout dx IS ds, so ds lands there too
  const bool sep = want_dx && p_drop > 0.0;
  auto ds = (out_dx && !sep) ? out_or_new(out_dx, s, "layernorm_bwd") : torch::empty_like(s);
  Tensor dx = sep ? out_or_new(out_dx, s, "layernorm_bwd") : ds;
  const int nb = smdt_ln_bwd_nblocks(rows, (int)H);
  auto f32 = s.options().dtype(at::kFloat);
  auto partials = torch::empty({nb, 3, H}, f32);
  Tensor ga = acc_target(dgamma_acc, H, "dgamma_acc"), ba = acc_target(dbeta_acc, H, "dbeta_acc"),
         bia = acc_target(dbias_acc, H, "dbias_acc");
  const int acc_mask = (ga.defined() ? 1 : 0) | (ba.defined() ? 2 : 0) | (bia.defined() ? 4 : 0);
  auto dgamma = ga.defined() ? ga : torch::empty({H}, f32);
  Tensor dbeta = rms ? Tensor() : (ba.defined() ? ba : torch::empty({H}, f32));
  Tensor dbias = want_dbias ? (bia.defined() ? bia : torch::empty({H}, f32)) : Tensor();
  check(smdt_layernorm_bwd(dcode(s), dcode(gamma), dy.data_ptr(), optr(ds_in), s.data_ptr(),
                           gamma.data_ptr(), rms ? nullptr : mean.data_ptr<float>(),
                           rstd.data_ptr<float>(), ds.data_ptr(), dx.data_ptr(),
                           partials.data_ptr<float>(), nb, dgamma.data_ptr<float>(),
                           rms ? nullptr : dbeta.data_ptr<float>(),
                           want_dbias ? dbias.data_ptr<float>() : nullptr, rows, (int)H,
                           (float)p_drop, (uint64_t)seed, (uint64_t)offset, rms ? 1 : 0, acc_mask,
                           optr(dy2), cur_stream()),
        "layernorm_bwd");
  return {ds, dx, dgamma, rms ? dgamma.new_empty({0}) : dbeta,
          want_dbias ? dbias : dgamma.new_empty({0})};
}

// ------------------------------------------------------------------ bias + activation
Tensor bias_act_fwd(Tensor x, OptT bias, int64_t act) {
  need_contig(x, "x");
  const int64_t N = x.size(-1), rows = x.numel() / N;
  if (bias) { need_contig(*bias, "bias"); TORCH_CHECK(bias->numel() == N && bias->dtype() == x.dtype(), "bias_act: bias mismatch"); }
  auto y = torch::empty_like(x);
  check(smdt_bias_act_fwd(dcode(x), (int)act, x.data_ptr(), optr(bias), y.data_ptr(), rows, (int)N,
                          cur_stream()),
        "bias_act_fwd");
  return y;
}

std::vector<Tensor> bias_act_bwd(Tensor dy, Tensor x, OptT bias, int64_t act, bool want_dbias,
                                 OptT dbias_acc) {
  need_contig(dy, "dy");
  need_contig(x, "x");
  TORCH_CHECK(dy.sizes() == x.sizes() && dy.dtype() == x.dtype(), "bias_act_bwd: shape mismatch");
  const int64_t N = x.size(-1), rows = x.numel() / N;
  auto dx = torch::empty_like(x);
  Tensor part, dbias;
  if (want_dbias) {
    const int slices = smdt_bias_act_slices(rows, (int)N);
    part = torch::empty({slices, N}, x.options().dtype(at::kFloat));
    dbias = dbias_acc ? acc_target(dbias_acc, N, "dbias_acc") : torch::empty({N}, x.options().dtype(at::kFloat));
  }
  check(smdt_bias_act_bwd(dcode(x), (int)act, dy.data_ptr(), x.data_ptr(), optr(bias),
                          dx.data_ptr(), want_dbias ? part.data_ptr<float>() : nullptr,
                          want_dbias ? dbias.data_ptr<float>() : nullptr, rows, (int)N,
                          dbias_acc ? 1 : 0, cur_stream()),
        "bias_act_bwd");
  return {dx, want_dbias ? dbias : dx.new_empty({0})};
}

Tensor swiglu_fwd(Tensor x) {
  need_contig(x, "x");
  const int64_t F2 = x.size(-1), rows = x.numel() / F2;
  TORCH_CHECK(F2 % 2 == 0, "swiglu: last dim must be even");
  auto sizes = x.sizes().vec();
  sizes.back() = F2 / 2;
  auto y = torch::empty(sizes, x.options());
  check(smdt_swiglu_fwd(dcode(x), x.data_ptr(), y.data_ptr(), rows, (int)(F2 / 2), cur_stream()),
        "swiglu_fwd");
  return y;
}

Tensor swiglu_bwd(Tensor dy, Tensor x) {
  need_contig(dy, "dy");
  need_contig(x, "x");
  const int64_t F2 = x.size(-1), rows = x.numel() / F2;
  TORCH_CHECK(dy.numel() * 2 == x.numel(), "swiglu_bwd: shape mismatch");
  auto dx = torch::empty_like(x);
  check(smdt_swiglu_bwd(dcode(x), dy.data_ptr(), x.data_ptr(), dx.data_ptr(), rows, (int)(F2 / 2),
                        cur_stream()),
        "swiglu_bwd");
  return dx;
}

// ------------------------------------------------------------------ masked softmax
Tensor softmax_fwd(Tensor x, OptT mask, int64_t mode, double scale) {
  need_contig(x, "x");
  TORCH_CHECK(x.dim() == 4, "softmax: expects [b, np, sq, sk]");
  const int64_t sk = x.size(3), sq = x.size(2), heads = x.size(1);
  const int64_t rows = x.numel() / sk;
  if (mode == 2) {
    TORCH_CHECK(mask.has_value(), "softmax: mode 2 needs a mask");
    need_contig(*mask, "mask");
    TORCH_CHECK(mask->scalar_type() == at::kBool || mask->scalar_type() == at::kByte, "softmax: mask must be bool/uint8");
    TORCH_CHECK(mask->numel() == x.size(0) * sq * sk, "softmax: mask must be [b, 1, sq, sk]");
  }
  auto y = torch::empty_like(x);
  check(smdt_softmax_fwd(dcode(x), (int)mode, x.data_ptr(),
                         mode == 2 ? (const uint8_t*)mask->data_ptr() : nullptr, y.data_ptr(), rows,
                         (int)sq, (int)sk, (int)heads, (float)scale, cur_stream()),
        "softmax_fwd");
  return y;
}

Tensor softmax_bwd(Tensor dy, Tensor y, int64_t mode, double scale) {
  need_contig(dy, "dy");
  need_contig(y, "y");
  TORCH_CHECK(dy.sizes() == y.sizes(), "softmax_bwd: shape mismatch");
  const int64_t sk = y.size(3), sq = y.size(2), rows = y.numel() / sk;
  auto dx = torch::empty_like(y);
  check(smdt_softmax_bwd(dcode(y), (int)mode, dy.data_ptr(), y.data_ptr(), dx.data_ptr(), rows,
                         (int)sq, (int)sk, (float)scale, cur_stream()),
        "softmax_bwd");
  return dx;
}

// ------------------------------------------------------------------ graph-safe dropout RNG
// counter: a persistent device int32 [1] (None: off). While set, every dropout kernel (flash
// attention, fused LayerNorm) mixes *counter into its keys at run time; the training step
// advances it on the device, so HIP-graph replays of a captured step draw fresh masks.
static Tensor g_rng_counter;
void set_rng_step(OptT counter) {
  if (counter) {
    TORCH_CHECK(counter->is_cuda() && counter->scalar_type() == at::kInt && counter->numel() == 1,
                "set_rng_step: device int32 [1] counter");
    g_rng_counter = *counter;
    smdt_set_rng_step(reinterpret_cast<uint32_t*>(counter->data_ptr<int>()));
  } else {
    g_rng_counter = Tensor();
    smdt_set_rng_step(nullptr);
  }
}

// ------------------------------------------------------------------ optimizer
void adam(Tensor master, Tensor grad, Tensor m, Tensor v, OptT model_out, double lr, double beta1,
          double beta2, double eps, double wd, int64_t step, bool adamw, OptT grad_mul,
          OptT found_inf) {
  for (auto* t : {&master, &grad, &m, &v}) {
    need_contig(*t, "adam buffer");
    TORCH_CHECK(t->scalar_type() == at::kFloat, "adam: fp32 buffers expected");
    TORCH_CHECK(t->numel() == master.numel(), "adam: buffer size mismatch");
  }
  int mdt = 0;
  if (model_out) {
    need_contig(*model_out, "model_out");
    TORCH_CHECK(model_out->numel() == master.numel(), "adam: model_out size mismatch");
    mdt = dcode(*model_out);
    TORCH_CHECK(mdt != 0, "adam: model_out must be bf16/fp16 (fp32 masters ARE the model)");
  }
  if (grad_mul) TORCH_CHECK(grad_mul->scalar_type() == at::kFloat && grad_mul->is_cuda(), "adam: grad_mul fp32 scalar");
  if (found_inf) TORCH_CHECK(found_inf->scalar_type() == at::kInt && found_inf->is_cuda(), "adam: found_inf int32 scalar");
  const double bc1 = 1.0 - std::pow(beta1, (double)step);
  const double bc2 = 1.0 - std::pow(beta2, (double)step);
  check(smdt_adam(master.data_ptr<float>(), grad.data_ptr<float>(), m.data_ptr<float>(),
                  v.data_ptr<float>(), model_out ? model_out->data_ptr() : nullptr, mdt,
                  master.numel(), (float)lr, (float)beta1, (float)beta2, (float)eps, (float)wd,
                  (float)bc1, (float)bc2, adamw ? 1 : 0,
                  grad_mul ? grad_mul->data_ptr<float>() : nullptr,
                  found_inf ? found_inf->data_ptr<int>() : nullptr, nullptr, cur_stream()),
        "adam");
}

// HIP-graph capturable form: lr and the bias corrections come from the device tensor
// hyper = [lr, 1 - beta1^t, 1 - beta2^t] (fp32, updated on the device each step), so a captured
// step replays with the current step count and learning rate.
void adam_capturable(Tensor master, Tensor grad, Tensor m, Tensor v, OptT model_out, Tensor hyper,
                     double beta1, double beta2, double eps, double wd, bool adamw, OptT grad_mul,
                     OptT found_inf) {
  for (auto* t : {&master, &grad, &m, &v}) {
    need_contig(*t, "adam buffer");
    TORCH_CHECK(t->scalar_type() == at::kFloat, "adam: fp32 buffers expected");
    TORCH_CHECK(t->numel() == master.numel(), "adam: buffer size mismatch");
  }
  TORCH_CHECK(hyper.scalar_type() == at::kFloat && hyper.is_cuda() && hyper.numel() == 3 && hyper.is_contiguous(),
              "adam_capturable: hyper = device fp32 [lr, bc1, bc2]");
  int mdt = 0;
  if (model_out) {
    need_contig(*model_out, "model_out");
    TORCH_CHECK(model_out->numel() == master.numel(), "adam: model_out size mismatch");
    mdt = dcode(*model_out);
    TORCH_CHECK(mdt != 0, "adam: model_out must be bf16/fp16 (fp32 masters ARE the model)");
  }
  if (grad_mul) TORCH_CHECK(grad_mul->scalar_type() == at::kFloat && grad_mul->is_cuda(), "adam: grad_mul fp32 scalar");
  if (found_inf) TORCH_CHECK(found_inf->scalar_type() == at::kInt && found_inf->is_cuda(), "adam: found_inf int32 scalar");
  check(smdt_adam(master.data_ptr<float>(), grad.data_ptr<float>(), m.data_ptr<float>(),
                  v.data_ptr<float>(), model_out ? model_out->data_ptr() : nullptr, mdt,
                  master.numel(), 0.f, (float)beta1, (float)beta2, (float)eps, (float)wd, 1.f, 1.f,
                  adamw ? 1 : 0, grad_mul ? grad_mul->data_ptr<float>() : nullptr,
                  found_inf ? found_inf->data_ptr<int>() : nullptr, hyper.data_ptr<float>(), cur_stream()),
        "adam_capturable");
}

Tensor sumsq(Tensor x, OptT found_inf) {
  need_contig(x, "x");
  const int64_t n = x.numel();
  const int nb = smdt_sumsq_nblocks(n);
  auto f32 = x.options().dtype(at::kFloat);
  auto partial = torch::empty({nb}, f32);
  auto out = torch::empty({1}, f32);
  if (found_inf) TORCH_CHECK(found_inf->scalar_type() == at::kInt && found_inf->is_cuda(), "sumsq: found_inf int32");
  check(smdt_sumsq(dcode(x), x.data_ptr(), n, partial.data_ptr<float>(), nb, out.data_ptr<float>(),
                   found_inf ? found_inf->data_ptr<int>() : nullptr, cur_stream()),
        "sumsq");
  return out;
}

std::vector<Tensor> clip_coef(Tensor sumsq_t, double max_norm, double inv_scale) {
  TORCH_CHECK(sumsq_t.scalar_type() == at::kFloat && sumsq_t.is_cuda(), "clip_coef: fp32 scalar");
  auto mul = torch::empty({1}, sumsq_t.options());
  auto norm = torch::empty({1}, sumsq_t.options());
  check(smdt_clip_coef(sumsq_t.data_ptr<float>(), (float)max_norm, (float)inv_scale,
                       mul.data_ptr<float>(), norm.data_ptr<float>(), cur_stream()),
        "clip_coef");
  return {mul, norm};
}

void scale_(Tensor x, OptT mul, double cmul) {
  need_contig(x, "x");
  check(smdt_scale(dcode(x), x.data_ptr(), x.numel(), mul ? mul->data_ptr<float>() : nullptr,
                   (float)cmul, cur_stream()),
        "scale");
}

void cast_(Tensor x, Tensor y, bool accumulate) {
  need_contig(x, "x");
  need_contig(y, "y");
  TORCH_CHECK(x.numel() == y.numel(), "cast: size mismatch");
  check(smdt_cast(dcode(x), dcode(y), x.data_ptr(), y.data_ptr(), x.numel(), accumulate ? 1 : 0,
                  cur_stream()),
        "cast");
}

// ------------------------------------------------------------------ augmentation filters (fp32)
// y [N, C, H, W] = x (*) k[n] per sample (reflect padding); k [N, KS, KS], KS in {3, 5, 7}.
Tensor aug_depthwise(Tensor x, Tensor k) {
  TORCH_CHECK(x.is_cuda() && k.is_cuda() && x.scalar_type() == at::kFloat && k.scalar_type() == at::kFloat,
              "aug_depthwise: fp32 GPU tensors");
  TORCH_CHECK(x.dim() == 4 && k.dim() == 3 && k.size(0) == x.size(0) && k.size(1) == k.size(2), "aug_depthwise: shapes");
  x = x.contiguous();
  k = k.contiguous();
  auto y = torch::empty_like(x);
  check(smdt_aug_depthwise(x.data_ptr<float>(), k.data_ptr<float>(), y.data_ptr<float>(), (int)x.size(0),
                           (int)x.size(1), (int)x.size(2), (int)x.size(3), (int)k.size(1), cur_stream()),
        "aug_depthwise");
  return y;
}

// y = 3 x 3 median of every channel of x [N, C, H, W] (reflect padding).
Tensor aug_median3(Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kFloat && x.dim() == 4, "aug_median3: fp32 [N, C, H, W] GPU tensor");
  x = x.contiguous();
  auto y = torch::empty_like(x);
  check(smdt_aug_median3(x.data_ptr<float>(), y.data_ptr<float>(), (int)(x.size(0) * x.size(1)), (int)x.size(2),
                         (int)x.size(3), cur_stream()),
        "aug_median3");
  return y;
}

// ------------------------------------------------------------------ row gather with zero fill
// out[r] = map[r] >= 0 ? src[map[r]] : 0; src [Ns, ...] contiguous, map int64 [Nd] on the device
Tensor gather_rows(Tensor src, Tensor map) {
  need_contig(src, "src");
  need_contig(map, "map");
  TORCH_CHECK(map.scalar_type() == at::kLong && map.dim() == 1 && map.device() == src.device(),
              "gather_rows: map must be a 1-D int64 tensor on src's device");
  TORCH_CHECK(src.dim() >= 1, "gather_rows: src must have a row dimension");
  const int64_t rb = src.numel() / std::max<int64_t>(src.size(0), 1) * src.element_size();
  TORCH_CHECK(rb % 16 == 0, "gather_rows: row bytes must be a multiple of 16");
  auto sizes = src.sizes().vec();
  sizes[0] = map.size(0);
  auto out = torch::empty(sizes, src.options());
  check(smdt_gather_rows(src.data_ptr(), map.data_ptr<int64_t>(), out.data_ptr(), map.size(0), src.size(0), rb,
                         cur_stream()),
        "gather_rows");
  return out;
}

// ------------------------------------------------------------------ FP8 quantisation (delayed scaling)
// x [M, K] bf16 / fp16 -> q [M, K] (and qt [K, M] with transpose) in float8_e4m3fn (fmt 0) or
// float8_e5m2 (fmt 1); scale / amax: one fp32 each on x's device (slots of the model's FP8 table).
static void need_f32_slot(const Tensor& t, const Tensor& like, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device() && t.scalar_type() == at::kFloat && t.numel() == 1,
              "fp8_quantize: '", name, "' must be one fp32 value on x's device");
}

std::vector<Tensor> fp8_quantize(Tensor x, Tensor scale, Tensor amax, int64_t fmt, bool transpose) {
  need_contig(x, "x");
  TORCH_CHECK(x.dim() == 2, "fp8_quantize: x must be 2-D, got ", x.dim(), "-D");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kHalf, "fp8_quantize: bf16 / fp16 only");
  TORCH_CHECK(fmt == 0 || fmt == 1, "fp8_quantize: fmt must be 0 (e4m3) or 1 (e5m2)");
  const int64_t M = x.size(0), K = x.size(1);
  TORCH_CHECK(M >= 1 && K >= 16 && K % 16 == 0, "fp8_quantize: need M >= 1 and K a multiple of 16, got [", M, ", ",
              K, "]");
  need_f32_slot(scale, x, "scale");
  need_f32_slot(amax, x, "amax");
  const auto qopt = x.options().dtype(fmt == 0 ? at::kFloat8_e4m3fn : at::kFloat8_e5m2);
  auto q = torch::empty({M, K}, qopt);
  Tensor qt;
  if (transpose) qt = torch::empty({K, M}, qopt);
  check(smdt_fp8_quantize(x.data_ptr(), q.data_ptr(), transpose ? qt.data_ptr() : nullptr, scale.data_ptr<float>(),
                          amax.data_ptr<float>(), M, K, dcode(x), (int)fmt, cur_stream()),
        "fp8_quantize");
  if (transpose) return {q, qt};
  return {q};
}

// ------------------------------------------------------------------ MX (block-scaled) FP8
// x [R, C] bf16 / fp16 -> the row form (q [R, C], s [R, C / 32]) and / or the column form
// (qt [C, R], st [C, R / 32]: the quantisation of x^T) in float8_e4m3fn (fmt 0) or float8_e5m2
// (fmt 1) with uint8 E8M0 scales; returns the requested forms in that order.
std::vector<Tensor> mx_quantize(Tensor x, int64_t fmt, bool rows, bool cols) {
  need_contig(x, "x");
  TORCH_CHECK(x.dim() == 2, "mx_quantize: x must be 2-D, got ", x.dim(), "-D");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kHalf, "mx_quantize: bf16 / fp16 only");
  TORCH_CHECK(fmt == 0 || fmt == 1, "mx_quantize: fmt must be 0 (e4m3) or 1 (e5m2)");
  TORCH_CHECK(rows || cols, "mx_quantize: nothing to produce");
  const int64_t R = x.size(0), C = x.size(1);
  TORCH_CHECK(R >= 1 && C >= 1, "mx_quantize: empty input [", R, ", ", C, "]");
  TORCH_CHECK(!rows || C % 32 == 0, "mx_quantize: the row form needs columns in multiples of 32, got [", R, ", ", C, "]");
  TORCH_CHECK(!cols || (R % 32 == 0 && C % 16 == 0),
              "mx_quantize: the column form needs rows in multiples of 32 and columns of 16, got [", R, ", ", C, "]");
  const auto qopt = x.options().dtype(fmt == 0 ? at::kFloat8_e4m3fn : at::kFloat8_e5m2);
  const auto sopt = x.options().dtype(at::kByte);
  Tensor q, s, qt, st;
  if (rows) { q = torch::empty({R, C}, qopt); s = torch::empty({R, C / 32}, sopt); }
  if (cols) { qt = torch::empty({C, R}, qopt); st = torch::empty({C, R / 32}, sopt); }
  check(smdt_mx_quantize(x.data_ptr(), rows ? q.data_ptr() : nullptr, rows ? s.data_ptr() : nullptr,
                         cols ? qt.data_ptr() : nullptr, cols ? st.data_ptr() : nullptr, R, C, dcode(x), (int)fmt,
                         cur_stream()),
        "mx_quantize");
  std::vector<Tensor> out;
  if (rows) { out.push_back(q); out.push_back(s); }
  if (cols) { out.push_back(qt); out.push_back(st); }
  return out;
}

bool gemm_mx_supported(int64_t M, int64_t N, int64_t K) { return smdt_gemm_mx_supported(M, N, K) != 0; }

// out [M, N] = a [M, K] . b [N, K]^T on MX operands (+ bias [N]); see kernels/gemm_mx.hip.
Tensor gemm_mx(Tensor a, Tensor sa, Tensor b, Tensor sb, OptT bias, int64_t out_dtype, int64_t max_blocks) {
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && sa.dim() == 2 && sb.dim() == 2, "gemm_mx: 2-D operands and scales");
  const int64_t M = a.size(0), K = a.size(1), N = b.size(0);
  TORCH_CHECK(a.is_cuda() && b.is_cuda() && sa.is_cuda() && sb.is_cuda(), "gemm_mx: GPU tensors only");
  TORCH_CHECK(a.is_contiguous() && b.is_contiguous() && sa.is_contiguous() && sb.is_contiguous(),
              "gemm_mx: operands and scales must be contiguous (M x N x K = ", M, " x ", N, " x ", K, ")");
  TORCH_CHECK(b.size(1) == K && smdt_gemm_mx_supported(M, N, K) != 0, "gemm_mx: M x N x K = ", M, " x ", N, " x ",
              b.size(1) == K ? K : -1, " refused: M, N and K must be multiples of 128 and the operands' K must agree");
  TORCH_CHECK(a.scalar_type() == at::kFloat8_e4m3fn || a.scalar_type() == at::kFloat8_e5m2,
              "gemm_mx: a must be float8_e4m3fn or float8_e5m2");
  TORCH_CHECK(b.scalar_type() == at::kFloat8_e4m3fn, "gemm_mx: b must be float8_e4m3fn");
  TORCH_CHECK(sa.scalar_type() == at::kByte && sb.scalar_type() == at::kByte && sa.size(0) == M &&
                  sa.size(1) == K / 32 && sb.size(0) == N && sb.size(1) == K / 32,
              "gemm_mx: scales must be uint8 [rows, K / 32]");
  for (const Tensor* t : {&a, &b, &sa, &sb}) {
    TORCH_CHECK(t->device() == a.device(), "gemm_mx: operands on different devices");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0, "gemm_mx: operands must be 16-byte aligned");
  }
  TORCH_CHECK(out_dtype == 1 || out_dtype == 2, "gemm_mx: out_dtype must be 1 (bf16) or 2 (fp16)");
  auto out = torch::empty({M, N}, a.options().dtype(out_dtype == 1 ? at::kBFloat16 : at::kHalf));
  if (bias) {
    need_contig(*bias, "bias");
    TORCH_CHECK(bias->numel() == N && bias->scalar_type() == out.scalar_type() && bias->device() == a.device(),
                "gemm_mx: bias must be [N] of the output dtype");
  }
  check(smdt_gemm_mx((int)out_dtype, a.scalar_type() == at::kFloat8_e5m2 ? 1 : 0, a.data_ptr(), sa.data_ptr(),
                     b.data_ptr(), sb.data_ptr(), out.data_ptr(), optr(bias), M, N, K, (int)max_blocks, cur_stream()),
        "gemm_mx");
  return out;
}

// In place on scale [T], hist [T, H], amax [T]; fmt_max [T] (448 or 57344 per tensor).
void fp8_update_scales(Tensor scale, Tensor hist, Tensor amax, Tensor fmt_max, int64_t margin, bool use_max) {
  need_contig(scale, "scale");
  need_contig(hist, "amax_history");
  need_contig(amax, "amax");
  need_contig(fmt_max, "fmt_max");
  TORCH_CHECK(scale.dim() == 1 && hist.dim() == 2 && amax.dim() == 1 && fmt_max.dim() == 1,
              "fp8_update_scales: scale [T], amax_history [T, H], amax [T], fmt_max [T]");
  const int64_t T = scale.size(0), H = hist.size(1);
  TORCH_CHECK(T >= 1 && H >= 1 && hist.size(0) == T && amax.size(0) == T && fmt_max.size(0) == T,
              "fp8_update_scales: table sizes do not match");
  for (const Tensor* t : {&scale, &hist, &amax, &fmt_max})
    TORCH_CHECK(t->scalar_type() == at::kFloat && t->device() == scale.device(), "fp8_update_scales: fp32 tables "
                "on one device");
  TORCH_CHECK(margin >= 0 && margin <= 64, "fp8_update_scales: margin out of range");
  check(smdt_fp8_update_scales(scale.data_ptr<float>(), hist.data_ptr<float>(), amax.data_ptr<float>(),
                               fmt_max.data_ptr<float>(), T, H, (int)margin, use_max ? 1 : 0, cur_stream()),
        "fp8_update_scales");
}

// ------------------------------------------------------------------ 2-D transpose (16-bit)
// out [C, R] = x [R, C]^T, contiguous (feeds the dgrad GEMMs in the TN layout).
Tensor transpose2d(Tensor x) {
  need_contig(x, "x");
  TORCH_CHECK(x.dim() == 2, "transpose2d: x must be 2-D");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kHalf, "transpose2d: bf16 / fp16 only");
  TORCH_CHECK(x.size(0) % 8 == 0 && x.size(1) % 8 == 0, "transpose2d: both dims must be multiples of 8");
  auto out = torch::empty({x.size(1), x.size(0)}, x.options());
  check(smdt_transpose16(x.data_ptr(), out.data_ptr(), x.size(0), x.size(1), cur_stream()), "transpose2d");
  return out;
}

// ------------------------------------------------------------------ paced link stand-in
// recv <- send on `blocks` workgroups, held until `ns` have passed (comm/loopback.py)
void paced_copy(Tensor recv, Tensor send, int64_t blocks, int64_t ns) {
  need_contig(recv, "recv");
  need_contig(send, "send");
  TORCH_CHECK(recv.is_cuda() && send.is_cuda(), "paced_copy: CUDA tensors");
  const int64_t nb = send.numel() * send.element_size();
  TORCH_CHECK(nb == recv.numel() * recv.element_size() && nb % 16 == 0, "paced_copy: equal sizes, multiple of 16 B");
  TORCH_CHECK((uintptr_t)send.data_ptr() % 16 == 0 && (uintptr_t)recv.data_ptr() % 16 == 0, "paced_copy: 16-B aligned");
  check(smdt_paced_copy(send.data_ptr(), recv.data_ptr(), nb, (int)blocks, ns, cur_stream()), "paced_copy");
}

// ------------------------------------------------------------------ RoPE
// x: [ntok, nh, d] strided view (last dim contiguous), rotary applied in place to the first
// `rot` elements of each head.
void rope_(Tensor x, Tensor cos_t, Tensor sin_t, int64_t rot, int64_t pos_div, int64_t pos_mod,
           bool backward) {
  need_cuda(x, "x");
  TORCH_CHECK(x.dim() == 3 && x.stride(2) == 1, "rope: x must be [ntok, nh, d] with unit last stride");
  need_contig(cos_t, "cos");
  need_contig(sin_t, "sin");
  TORCH_CHECK(cos_t.scalar_type() == at::kFloat && sin_t.scalar_type() == at::kFloat, "rope: fp32 tables");
  TORCH_CHECK(rot <= x.size(2) && rot % 16 == 0 && cos_t.size(-1) == rot / 2, "rope: rotary dim mismatch");
  TORCH_CHECK(x.stride(0) % 8 == 0 && x.stride(1) % 8 == 0, "rope: strides must keep 16-byte alignment");
  check(smdt_rope(dcode(x), x.data_ptr(), x.size(0), (int)x.size(1), x.stride(0), x.stride(1),
                  (int)rot, cos_t.data_ptr<float>(), sin_t.data_ptr<float>(), (int)pos_div,
                  (int)pos_mod, backward ? 1 : 0, cur_stream()),
        "rope");
}

// ------------------------------------------------------------------ forward / dgrad GEMM (MFMA)
// out[M, N] = a[M, K] . b[N, K]^T with the epilogue `epi` (0 none, 1 + bias, 2 bias + GeLU-tanh:
// out = pre-activation, out2 = activation). Returns false (and does nothing) for an unsupported
// shape / layout so the caller can take the library GEMM; out / out2 may be given (e.g. a slice of
// a larger buffer), else they are allocated.
bool gemm_tn_supported(Tensor a, Tensor b) {
  if (!a.is_cuda() || !b.is_cuda() || a.dim() != 2 || b.dim() != 2 || !a.is_contiguous() || !b.is_contiguous()) return false;
  if ((a.scalar_type() != at::kBFloat16 && a.scalar_type() != at::kHalf) || b.scalar_type() != a.scalar_type()) return false;
  if (a.size(1) != b.size(1)) return false;
  if (reinterpret_cast<uintptr_t>(a.data_ptr()) % 16 || reinterpret_cast<uintptr_t>(b.data_ptr()) % 16) return false;
  return smdt_gemm_tn_supported(a.size(0), b.size(0), a.size(1)) != 0;
}

std::vector<Tensor> gemm_tn(Tensor a, Tensor b, int64_t epi, OptT bias, OptT out, OptT out2, int64_t max_blocks,
                            int64_t var, OptT aux) {
  TORCH_CHECK(gemm_tn_supported(a, b), "gemm_tn: unsupported operands");
  TORCH_CHECK(epi >= 0 && epi <= 3, "gemm_tn: epilogue");
  const int64_t M = a.size(0), N = b.size(0), K = a.size(1);
  if (epi >= 1) {
    TORCH_CHECK(bias.has_value(), "gemm_tn: the epilogue needs a bias");
    need_contig(*bias, "bias");
    TORCH_CHECK(bias->numel() == N && bias->scalar_type() == a.scalar_type(), "gemm_tn: bias mismatch");
  }
  if (epi == 3) {
    TORCH_CHECK(aux.has_value(), "gemm_tn: the GeLU-backward epilogue needs the pre-activation");
    need_contig(*aux, "aux");
    TORCH_CHECK(aux->numel() == M * N && aux->scalar_type() == a.scalar_type() && aux->device() == a.device(),
                "gemm_tn: pre-activation mismatch");
  }
  auto mk = [&](const OptT& o, const char* n) {
    if (!o) return torch::empty({M, N}, a.options());
    need_contig(*o, n);
    TORCH_CHECK(o->numel() == M * N && o->scalar_type() == a.scalar_type() && o->device() == a.device(),
                "gemm_tn: output buffer mismatch");
    return *o;
  };
  Tensor c = mk(out, "out");
  Tensor c2 = epi == 2 ? mk(out2, "out2") : Tensor();
  check(smdt_gemm_tn_var(dcode(a), (int)epi, a.data_ptr(), b.data_ptr(), c.data_ptr(),
                         epi == 2 ? c2.data_ptr() : nullptr, optr(bias), epi == 3 ? aux->data_ptr() : nullptr, M,
                         N, K, (int)max_blocks, (int)var, cur_stream()),
        "gemm_tn");
  if (epi == 2) return {c, c2};
  return {c};
}

// The GeLU-backward epilogue (epi 3) that also makes the bias gradient of the linear whose dY it
// writes: out = (a . b^T) * gelu_tanh'(aux + bias), and dbias[N] (fp32) = / += the column sums of
// the fp32 output values before their 16-bit rounding (per-half-tile partials from the kernel,
// added in a fixed order by the column-sum kernel: no atomics, bitwise reproducible).
Tensor gemm_tn_dgelu_dbias(Tensor a, Tensor b, Tensor bias, Tensor aux, Tensor dbias, bool accumulate, OptT out,
                           int64_t max_blocks) {
  TORCH_CHECK(gemm_tn_supported(a, b), "gemm_tn_dgelu_dbias: unsupported operands");
  const int64_t M = a.size(0), N = b.size(0), K = a.size(1);
  need_contig(bias, "bias");
  need_contig(aux, "aux");
  TORCH_CHECK(bias.numel() == N && bias.scalar_type() == a.scalar_type(), "gemm_tn_dgelu_dbias: bias mismatch");
  TORCH_CHECK(aux.numel() == M * N && aux.scalar_type() == a.scalar_type() && aux.device() == a.device(),
              "gemm_tn_dgelu_dbias: pre-activation mismatch");
  Tensor db = acc_target(dbias, N, "gemm_tn_dgelu_dbias dbias");
  TORCH_CHECK(db.device() == a.device(), "gemm_tn_dgelu_dbias: dbias on another device");
  Tensor c;
  if (out) {
    need_contig(*out, "out");
    TORCH_CHECK(out->numel() == M * N && out->scalar_type() == a.scalar_type() && out->device() == a.device(),
                "gemm_tn_dgelu_dbias: output buffer mismatch");
    c = *out;
  } else {
    c = torch::empty({M, N}, a.options());
  }
  auto part = torch::empty({M / 128, N}, a.options().dtype(at::kFloat));
  check(smdt_gemm_tn_dgelu_sums(dcode(a), a.data_ptr(), b.data_ptr(), c.data_ptr(), bias.data_ptr(), aux.data_ptr(),
                                part.data_ptr<float>(), M, N, K, (int)max_blocks, cur_stream()),
        "gemm_tn_dgelu_dbias");
  check(smdt_col_sum(part.data_ptr<float>(), (int)(M / 128), (int)N, db.data_ptr<float>(), accumulate ? 1 : 0,
                     cur_stream()),
        "gemm_tn_dgelu_dbias column sums");
  return c;
}

// ------------------------------------------------------------------ Switch MLP: device routing + grouped GEMM
// Top-1 routing of logits [T, E] (fp32 / bf16 / fp16, E <= 64) into the expert-sorted, tile-padded
// layout (kernels/moe_route.hip). Returns (top_p fp32 [T], expert_of_token int32 [T], row_of_token
// int32 [T], token_of_row int64 [R], tile_expert int32 [R / 256], seg int32 [E, 2], counts int32 [E]);
// the tables are allocated uninitialised and every word is written.
std::vector<Tensor> moe_route(Tensor logits) {
  need_contig(logits, "logits");
  TORCH_CHECK(logits.dim() == 2 && logits.size(0) > 0 && logits.size(1) > 0 && logits.size(1) <= 64,
              "moe_route: logits must be [T, E] with E <= 64");
  const int64_t T = logits.size(0), E = logits.size(1), R = smdt_moe_rows(T, E);
  auto i32 = logits.options().dtype(at::kInt);
  Tensor top_p = torch::empty({T}, logits.options().dtype(at::kFloat));
  Tensor top_e = torch::empty({T}, i32), row_of = torch::empty({T}, i32);
  Tensor tok_of = torch::empty({R}, logits.options().dtype(at::kLong));
  Tensor tile_e = torch::empty({R / 256}, i32), seg = torch::empty({E, 2}, i32), counts = torch::empty({E}, i32);
  Tensor hist = torch::empty({(T + 255) / 256, E}, i32);
  check(smdt_moe_route(dcode(logits), logits.data_ptr(), T, E, top_p.data_ptr<float>(), top_e.data_ptr<int>(),
                       row_of.data_ptr<int>(), tok_of.data_ptr<int64_t>(), tile_e.data_ptr<int>(),
                       seg.data_ptr<int>(), counts.data_ptr<int>(), hist.data_ptr<int>(), cur_stream()),
        "moe_route");
  return {top_p, top_e, row_of, tok_of, tile_e, seg, counts};
}

// The same into caller-made buffers (any prior contents; every word is overwritten).
void moe_route_into(Tensor logits, Tensor top_p, Tensor top_e, Tensor row_of, Tensor tok_of, Tensor tile_e, Tensor seg,
                    Tensor counts) {
  need_contig(logits, "logits");
  TORCH_CHECK(logits.dim() == 2 && logits.size(0) > 0 && logits.size(1) > 0 && logits.size(1) <= 64,
              "moe_route: logits must be [T, E] with E <= 64");
  const int64_t T = logits.size(0), E = logits.size(1), R = smdt_moe_rows(T, E);
  auto ok = [&](const Tensor& t, at::ScalarType ty, int64_t n) {
    return t.is_cuda() && t.is_contiguous() && t.scalar_type() == ty && t.numel() == n && t.device() == logits.device();
  };
  TORCH_CHECK(ok(top_p, at::kFloat, T) && ok(top_e, at::kInt, T) && ok(row_of, at::kInt, T) && ok(tok_of, at::kLong, R) &&
                  ok(tile_e, at::kInt, R / 256) && ok(seg, at::kInt, 2 * E) && ok(counts, at::kInt, E),
              "moe_route_into: table buffer mismatch");
  Tensor hist = torch::empty({(T + 255) / 256, E}, logits.options().dtype(at::kInt));
  check(smdt_moe_route(dcode(logits), logits.data_ptr(), T, E, top_p.data_ptr<float>(), top_e.data_ptr<int>(),
                       row_of.data_ptr<int>(), tok_of.data_ptr<int64_t>(), tile_e.data_ptr<int>(),
                       seg.data_ptr<int>(), counts.data_ptr<int>(), hist.data_ptr<int>(), cur_stream()),
        "moe_route");
}

// The device table of the base pointers of same-shaped, same-typed contiguous GPU tensors (one per
// expert) that gemm_tn_grouped picks its B / bias from. The caller keeps the tensors alive and
// rebuilds the table when one of them is reallocated.
Tensor ptr_table(std::vector<Tensor> ts) {
  TORCH_CHECK(!ts.empty(), "ptr_table: empty list");
  std::vector<int64_t> p(ts.size());
  for (size_t i = 0; i < ts.size(); ++i) {
    need_contig(ts[i], "ptr_table entry");
    TORCH_CHECK(ts[i].sizes() == ts[0].sizes() && ts[i].scalar_type() == ts[0].scalar_type() &&
                    ts[i].device() == ts[0].device(),
                "ptr_table: entries must share shape, dtype and device");
    p[i] = (int64_t)reinterpret_cast<uintptr_t>(ts[i].data_ptr());
  }
  return torch::tensor(p, torch::dtype(at::kLong)).to(ts[0].device());
}

// out[M, n] = a[M, K] . B_e^T per 256-row tile, e = tile_expert[tile] (an entry < 0: an unused tail
// tile, computed on expert 0), B_e the [n, K] tensor btab[e] points to, with gemm_tn's epilogues
// (bias from biastab[e]). sums (epi 3): also returns the fp32 [M / 128, n] column sums per half tile.
std::vector<Tensor> gemm_tn_grouped(Tensor a, Tensor btab, int64_t n, Tensor tile_expert, int64_t epi, OptT biastab,
                                    OptT aux, bool sums, int64_t max_blocks) {
  need_contig(a, "a");
  need_contig(btab, "btab");
  need_contig(tile_expert, "tile_expert");
  TORCH_CHECK(a.dim() == 2 && (a.scalar_type() == at::kBFloat16 || a.scalar_type() == at::kHalf),
              "gemm_tn_grouped: a must be a 2-D bf16 / fp16 tensor");
  const int64_t M = a.size(0), K = a.size(1), N = n;
  TORCH_CHECK(smdt_gemm_tn_supported(M, N, K) != 0, "gemm_tn_grouped: unsupported shape");
  TORCH_CHECK(btab.scalar_type() == at::kLong && btab.dim() == 1 && btab.numel() >= 1 && btab.device() == a.device(),
              "gemm_tn_grouped: btab must be an int64 pointer table on a's device");
  const int64_t E = btab.numel();
  TORCH_CHECK(tile_expert.scalar_type() == at::kInt && tile_expert.numel() == M / 256 &&
                  tile_expert.device() == a.device(),
              "gemm_tn_grouped: tile_expert must be int32 [M / 256] on a's device");
  TORCH_CHECK(epi >= 0 && epi <= 3 && (!sums || epi == 3), "gemm_tn_grouped: epilogue");
  if (epi >= 1) {
    TORCH_CHECK(biastab.has_value(), "gemm_tn_grouped: the epilogue needs a bias table");
    need_contig(*biastab, "biastab");
    TORCH_CHECK(biastab->scalar_type() == at::kLong && biastab->numel() == E && biastab->device() == a.device(),
                "gemm_tn_grouped: biastab mismatch");
  }
  if (epi == 3) {
    TORCH_CHECK(aux.has_value(), "gemm_tn_grouped: the GeLU-backward epilogue needs the pre-activation");
    need_contig(*aux, "aux");
    TORCH_CHECK(aux->numel() == M * N && aux->scalar_type() == a.scalar_type() && aux->device() == a.device(),
                "gemm_tn_grouped: pre-activation mismatch");
  }
  Tensor c = torch::empty({M, N}, a.options());
  const void* const* bt = reinterpret_cast<const void* const*>(btab.data_ptr<int64_t>());
  const void* const* bi = epi >= 1 ? reinterpret_cast<const void* const*>(biastab->data_ptr<int64_t>()) : nullptr;
  if (sums) {
    Tensor part = torch::empty({M / 128, N}, a.options().dtype(at::kFloat));
    check(smdt_gemm_tn_grouped_dgelu_sums(dcode(a), a.data_ptr(), bt, c.data_ptr(), bi, aux->data_ptr(),
                                          part.data_ptr<float>(), tile_expert.data_ptr<int>(), (int)E, M, N, K,
                                          (int)max_blocks, cur_stream()),
          "gemm_tn_grouped (sums)");
    return {c, part};
  }
  Tensor c2 = epi == 2 ? torch::empty({M, N}, a.options()) : Tensor();
  check(smdt_gemm_tn_grouped(dcode(a), (int)epi, a.data_ptr(), bt, c.data_ptr(), epi == 2 ? c2.data_ptr() : nullptr,
                             bi, epi == 3 ? aux->data_ptr() : nullptr, tile_expert.data_ptr<int>(), (int)E, M, N, K,
                             (int)max_blocks, cur_stream()),
        "gemm_tn_grouped");
  if (epi == 2) return {c, c2};
  return {c};
}

// ------------------------------------------------------------------ weight gradient (MFMA)
// The operand checks the wgrad bindings share, in the order every one of them makes them (the FP8
// binding raises for a misplaced dequantisation factor between the two): an fp32 contiguous device
// target, 2-D contiguous operands of a permitted type (dy one of dy_a / dy_b; x of x_type, or of
// dy's type when x_type is Undefined), on the target's device when `same_device` (the single launch
// never asked) ...
static bool wgrad_operands_ok(const Tensor& mg, const Tensor& dy, const Tensor& x, at::ScalarType dy_a,
                              at::ScalarType dy_b, at::ScalarType x_type, bool same_device) {
  if (!mg.is_cuda() || mg.scalar_type() != at::kFloat || !mg.is_contiguous()) return false;
  if (dy.dim() != 2 || x.dim() != 2 || !dy.is_contiguous() || !x.is_contiguous()) return false;
  if ((dy.scalar_type() != dy_a && dy.scalar_type() != dy_b) ||
      x.scalar_type() != (x_type == at::ScalarType::Undefined ? dy.scalar_type() : x_type))
    return false;
  return !same_device || (dy.get_device() == mg.get_device() && x.get_device() == mg.get_device());
}
// ... and dy [M, N], x [M, K], a target of N K elements, a shape the kernel takes.
static bool wgrad_shape_ok(const Tensor& mg, const Tensor& dy, const Tensor& x,
                           int (*supported)(int64_t, int64_t, int64_t)) {
  const int64_t M = dy.size(0), N = dy.size(1), K = x.size(1);
  return x.size(0) == M && mg.numel() == N * K && supported(M, N, K);
}

// main_grad[N, K] (fp32) += dy[M, N]^T . x[M, K]; returns false when the shape is unsupported.
bool wgrad_mfma(Tensor main_grad, Tensor dy, Tensor x, int64_t max_splits) {
  if (!wgrad_operands_ok(main_grad, dy, x, at::kBFloat16, at::kHalf, at::ScalarType::Undefined, false) ||
      !wgrad_shape_ok(main_grad, dy, x, smdt_wgrad_supported))
    return false;
  const int64_t M = dy.size(0), N = dy.size(1), K = x.size(1);
  check(smdt_wgrad_accumulate_t(dcode(dy), dy.data_ptr(), x.data_ptr(), main_grad.data_ptr<float>(), M, N, K, (int)max_splits,
                              cur_stream()),
        "wgrad_mfma");
  return true;
}

// Grouped form: main_grads[i] += dys[i]^T . xs[i] for every i in ONE launch per 32 problems.
// Returns false (and does nothing) when any problem is unsupported. The targets must not overlap.
// ``biases`` (optional, one per problem; an empty tensor = none): fp32 [N] targets that receive
// the column sums of dy — the bias gradient — from the same launch.
// overwrite (optional, per problem): the main_grad holds no data yet (a lazily zeroed gradient
// buffer): the kernel stores dy^T x instead of adding it (no read of the target).
// mranges / experts (optional, per problem; an empty tensor = none): a ranged problem, whose m range
// is the segment of `experts[i]` in the int32 [nexp, 2] device table `mranges[i]` (moe_route's seg).
bool wgrad_grouped(std::vector<Tensor> main_grads, std::vector<Tensor> dys, std::vector<Tensor> xs,
                   std::vector<Tensor> biases, std::vector<bool> overwrite, int64_t cus,
                   std::vector<Tensor> mranges, std::vector<int64_t> experts) {
  const size_t n = main_grads.size();
  TORCH_CHECK(mranges.empty() || (mranges.size() == n && experts.size() == n), "wgrad_grouped: mranges / experts list length");
  TORCH_CHECK(dys.size() == n && xs.size() == n, "wgrad_grouped: list lengths differ");
  TORCH_CHECK(biases.empty() || biases.size() == n, "wgrad_grouped: biases list length");
  TORCH_CHECK(overwrite.empty() || overwrite.size() == n, "wgrad_grouped: overwrite list length");
  std::vector<SmdtWgradProblem> probs(n);
  for (size_t i = 0; i < n; ++i) {
    const Tensor &mg = main_grads[i], &dy = dys[i], &x = xs[i];
    if (!wgrad_operands_ok(mg, dy, x, at::kBFloat16, at::kHalf, at::ScalarType::Undefined, true) ||
        dy.scalar_type() != dys[0].scalar_type() || !wgrad_shape_ok(mg, dy, x, smdt_wgrad_supported))
      return false;
    const int64_t M = dy.size(0), N = dy.size(1), K = x.size(1);
    float* bg = nullptr;
    if (!biases.empty() && biases[i].numel() > 0) {
      const Tensor& bt = biases[i];
      if (!bt.is_cuda() || bt.scalar_type() != at::kFloat || !bt.is_contiguous() || bt.numel() != N ||
          bt.get_device() != mg.get_device())
        return false;
      bg = bt.data_ptr<float>();
    }
    const int* mr = nullptr;
    int ex = 0;
    if (!mranges.empty() && mranges[i].numel() > 0) {
      const Tensor& sg = mranges[i];
      if (!sg.is_cuda() || sg.scalar_type() != at::kInt || !sg.is_contiguous() || sg.dim() != 2 || sg.size(1) != 2 ||
          sg.get_device() != mg.get_device() || experts[i] < 0 || experts[i] >= sg.size(0) || M % 256 != 0)
        return false;
      mr = sg.data_ptr<int>();
      ex = (int)experts[i];
    }
    probs[i] = SmdtWgradProblem{dy.data_ptr(), x.data_ptr(), mg.data_ptr<float>(), M, N, K, bg,
                                (!overwrite.empty() && overwrite[i]) ? 1 : 0, mr, ex};
  }
  if (n == 0) return true;
  check(smdt_wgrad_grouped_cus(dcode(dys[0]), probs.data(), (int)n, (int)cus, cur_stream()), "wgrad_grouped");
  return true;
}

// FP8 form (wgrad_fp8.hip): main_grads[i] (+)= (inv_dys[i] * inv_xs[i]) * dys[i]^T . xs[i] with
// dys in float8_e5m2 or float8_e4m3fn (one format per call) and xs in float8_e4m3fn. inv_dys /
// inv_xs are one-element fp32 device tensors the kernel reads (no host sync). Returns false (and
// does nothing) when any problem is unsupported. The targets must not overlap.
bool wgrad_fp8_grouped(std::vector<Tensor> main_grads, std::vector<Tensor> dys, std::vector<Tensor> xs,
                       std::vector<Tensor> inv_dys, std::vector<Tensor> inv_xs, std::vector<bool> overwrite,
                       int64_t cus) {
  const size_t n = main_grads.size();
  TORCH_CHECK(dys.size() == n && xs.size() == n && inv_dys.size() == n && inv_xs.size() == n,
              "wgrad_fp8_grouped: list lengths differ");
  TORCH_CHECK(overwrite.empty() || overwrite.size() == n, "wgrad_fp8_grouped: overwrite list length");
  std::vector<SmdtWgradFp8Problem> probs(n);
  for (size_t i = 0; i < n; ++i) {
    const Tensor &mg = main_grads[i], &dy = dys[i], &x = xs[i], &idy = inv_dys[i], &ix = inv_xs[i];
    if (!wgrad_operands_ok(mg, dy, x, at::kFloat8_e5m2, at::kFloat8_e4m3fn, at::kFloat8_e4m3fn, true) ||
        dy.scalar_type() != dys[0].scalar_type())
      return false;
    for (const Tensor* t : {&idy, &ix})
      TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kFloat && t->numel() == 1 &&
                      t->get_device() == mg.get_device(),
                  "wgrad_fp8_grouped: a dequantisation factor must be one fp32 value on the target's device");
    if (!wgrad_shape_ok(mg, dy, x, smdt_wgrad_fp8_supported)) return false;
    const int64_t M = dy.size(0), N = dy.size(1), K = x.size(1);
    for (size_t j = 0; j < i; ++j) {    // overlapping targets would race
      const char *a0 = (const char*)mg.data_ptr(), *b0 = (const char*)main_grads[j].data_ptr();
      if (a0 < b0 + main_grads[j].numel() * 4 && b0 < a0 + mg.numel() * 4) return false;
    }
    probs[i] = SmdtWgradFp8Problem{dy.data_ptr(), x.data_ptr(), mg.data_ptr<float>(), M, N, K,
                                   idy.data_ptr<float>(), ix.data_ptr<float>(),
                                   dy.scalar_type() == at::kFloat8_e5m2 ? 1 : 0,
                                   (!overwrite.empty() && overwrite[i]) ? 1 : 0};
  }
  if (n == 0) return true;
  check(smdt_wgrad_fp8_grouped_cus(probs.data(), (int)n, (int)cus, cur_stream()), "wgrad_fp8_grouped");
  return true;
}

bool wgrad_fp8_supported(int64_t M, int64_t N, int64_t K) { return smdt_wgrad_fp8_supported(M, N, K) != 0; }

// ------------------------------------------------------------------ bias gradient
// out[N] (fp32) = / += column sums of dy [.., N]
void bias_grad(Tensor dy, Tensor out, bool accumulate) {
  need_contig(dy, "dy");
  const int64_t N = dy.size(-1), rows = dy.numel() / N;
  Tensor o = acc_target(out, N, "bias_grad out");
  const int slices = smdt_bias_act_slices(rows, (int)N);
  auto part = torch::empty({slices, N}, dy.options().dtype(at::kFloat));
  check(smdt_bias_grad(dcode(dy), dy.data_ptr(), rows, (int)N, part.data_ptr<float>(),
                       o.data_ptr<float>(), accumulate ? 1 : 0, cur_stream()),
        "bias_grad");
}

// ------------------------------------------------------------------ cross entropy
// loss[rows] fp32; logits (16-bit, [rows, V]) are overwritten with softmax - onehot
Tensor ce_fused(Tensor logits, Tensor target, int64_t ignore_index, int64_t vvalid) {
  need_contig(logits, "logits");
  need_contig(target, "target");
  TORCH_CHECK(target.scalar_type() == at::kLong, "ce_fused: int64 targets");
  const int64_t V = logits.size(-1), rows = logits.numel() / V;
  TORCH_CHECK(target.numel() == rows, "ce_fused: target size mismatch");
  auto loss = torch::empty({rows}, logits.options().dtype(at::kFloat));
  check(smdt_ce_fused(dcode(logits), logits.data_ptr(), target.data_ptr<int64_t>(), loss.data_ptr<float>(),
                      rows, (int)V, (int)(vvalid > 0 ? vvalid : V), ignore_index, 0, 0, cur_stream()),
        "ce_fused");
  return loss;
}

// Vocab-parallel form: logits [rows, V] = this rank's vocab slice starting at vstart, overwritten
// with exp(x - m_local); returns stats [3, rows] fp32 = (m_local, sum, target logit or 0).
Tensor ce_fused_local(Tensor logits, Tensor target, int64_t vstart, int64_t vvalid) {
  need_contig(logits, "logits");
  need_contig(target, "target");
  TORCH_CHECK(target.scalar_type() == at::kLong, "ce_fused_local: int64 targets");
  const int64_t V = logits.size(-1), rows = logits.numel() / V;
  TORCH_CHECK(target.numel() == rows, "ce_fused_local: target size mismatch");
  auto stats = torch::empty({3, rows}, logits.options().dtype(at::kFloat));
  check(smdt_ce_fused(dcode(logits), logits.data_ptr(), target.data_ptr<int64_t>(), stats.data_ptr<float>(),
                      rows, (int)V, (int)(vvalid > 0 ? vvalid : V), -100, 1, vstart, cur_stream()),
        "ce_fused_local");
  return stats;
}

std::vector<Tensor> ce_stats(Tensor logits, Tensor target, int64_t vstart, int64_t vvalid) {
  need_contig(logits, "logits");
  need_contig(target, "target");
  TORCH_CHECK(target.scalar_type() == at::kLong, "ce: int64 targets");
  const int64_t V = logits.size(-1), rows = logits.numel() / V;
  TORCH_CHECK(target.numel() == rows, "ce: target size mismatch");
  auto f32 = logits.options().dtype(at::kFloat);
  auto mx = torch::empty({rows}, f32), se = torch::empty({rows}, f32), tg = torch::empty({rows}, f32);
  check(smdt_ce_stats(dcode(logits), logits.data_ptr(), target.data_ptr<int64_t>(), rows, (int)V,
                      (int)(vvalid > 0 ? vvalid : V), vstart, mx.data_ptr<float>(), se.data_ptr<float>(), tg.data_ptr<float>(),
                      cur_stream()),
        "ce_stats");
  return {mx, se, tg};
}

void ce_bwd(Tensor logits, Tensor target, Tensor gmax, Tensor gsum, Tensor dloss, Tensor out,
            int64_t vstart, int64_t ignore_index, int64_t vvalid) {
  need_contig(logits, "logits");
  need_contig(out, "dlogits");
  TORCH_CHECK(out.sizes() == logits.sizes() && out.dtype() == logits.dtype(), "ce_bwd: out mismatch");
  const int64_t V = logits.size(-1), rows = logits.numel() / V;
  for (auto* t : {&gmax, &gsum, &dloss}) {
    need_contig(*t, "ce row stat");
    TORCH_CHECK(t->scalar_type() == at::kFloat && t->numel() == rows, "ce_bwd: fp32 [rows] stats");
  }
  check(smdt_ce_bwd(dcode(logits), logits.data_ptr(), target.data_ptr<int64_t>(),
                    gmax.data_ptr<float>(), gsum.data_ptr<float>(), dloss.data_ptr<float>(),
                    out.data_ptr(), rows, (int)V, (int)(vvalid > 0 ? vvalid : V), vstart,
                    ignore_index, cur_stream()),
        "ce_bwd");
}

// ------------------------------------------------------------------ flash attention
// q: [B, S, H, D], k/v: [B, S, Hkv, D] (unit last stride, any other strides).
void fa_check(const Tensor& t, const char* n) {
  need_cuda(t, n);
  TORCH_CHECK(t.dim() == 4 && t.stride(3) == 1, "flash: '", n, "' must be [B, S, H, D] with unit last stride");
  TORCH_CHECK(t.scalar_type() == at::kBFloat16 || t.scalar_type() == at::kHalf, "flash: bf16 / fp16 only");
  TORCH_CHECK(t.stride(0) % 8 == 0 && t.stride(1) % 8 == 0 && t.stride(2) % 8 == 0 &&
                  reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              "flash: '", n, "' must keep 16-byte row alignment");
}

// Per-document descriptor (doc_start / doc_end): int32, contiguous [B, S], on q's device.
const int* fa_doc_ptr(const OptT& d, const Tensor& q, const char* n) {
  if (!d) return nullptr;
  need_cuda(*d, n);
  TORCH_CHECK(d->scalar_type() == at::kInt, "flash: '", n, "' must be int32");
  TORCH_CHECK(d->dim() == 2 && d->size(0) == q.size(0) && d->size(1) == q.size(1) && d->is_contiguous(),
              "flash: '", n, "' must be a contiguous [B, S] tensor");
  TORCH_CHECK(d->device() == q.device(), "flash: '", n, "' is on another device than q");
  return d->data_ptr<int>();
}

// ------------------------------------------------------------------ Swin window attention
// qkv [B, ph, pw, 3 heads d] on the padded, unrolled grid; table fp32 [(2 ws - 1)^2, heads].
// Everything the kernel does not take is refused here, before any launch.
struct WaDims { int B, ph, pw, heads, ws, shift; int64_t C, nW, N, E; };
static WaDims wa_check(const Tensor& qkv, const Tensor& table, int64_t window, int64_t shift, int64_t heads) {
  need_contig(qkv, "qkv");
  need_contig(table, "table");
  TORCH_CHECK(qkv.dim() == 4, "window_attn: qkv must be [B, ph, pw, 3 C]");
  TORCH_CHECK(qkv.scalar_type() == at::kBFloat16 || qkv.scalar_type() == at::kHalf,
              "window_attn: qkv must be bf16 or fp16, got ", qkv.scalar_type());
  TORCH_CHECK(heads > 0 && qkv.size(3) % (3 * heads) == 0, "window_attn: last dim is not (3, heads, d)");
  const int64_t d = qkv.size(3) / (3 * heads);
  TORCH_CHECK(window > 0 && window < 1024 && qkv.numel() > 0 && qkv.size(1) < (1 << 20) && qkv.size(2) < (1 << 20),
              "window_attn: bad shape");
  TORCH_CHECK(smdt_window_attn_supported(dcode(qkv), (int)d, (int)window, (int)qkv.size(1), (int)qkv.size(2),
                                         (int)shift),
              "window_attn: unsupported (needs d == 32, window <= 8, ph and pw multiples of the window, "
              "0 <= shift < window): d ", d, ", window ", window, ", grid ", qkv.size(1), " x ", qkv.size(2),
              ", shift ", shift);
  WaDims w{(int)qkv.size(0), (int)qkv.size(1), (int)qkv.size(2), (int)heads, (int)window, (int)shift,
           heads * d, (qkv.size(1) / window) * (qkv.size(2) / window), window * window,
           (2 * window - 1) * (2 * window - 1)};
  TORCH_CHECK(table.scalar_type() == at::kFloat && table.dim() == 2 && table.size(0) == w.E &&
                  table.size(1) == heads && table.device() == qkv.device(),
              "window_attn: table must be fp32 [(2 window - 1)^2, heads] on qkv's device");
  return w;
}

std::vector<Tensor> window_attn_fwd(Tensor qkv, Tensor table, int64_t window, int64_t shift, int64_t heads) {
  const WaDims w = wa_check(qkv, table, window, shift, heads);
  auto out = torch::empty({w.B, w.ph, w.pw, w.C}, qkv.options());
  auto lse = torch::empty({w.B, w.nW, w.heads, w.N}, qkv.options().dtype(at::kFloat));
  check(smdt_window_attn_fwd(dcode(qkv), qkv.data_ptr(), table.data_ptr<float>(), out.data_ptr(),
                             lse.data_ptr<float>(), w.B, w.ph, w.pw, w.heads, w.ws, w.shift, cur_stream()),
        "window_attn_fwd");
  return {out, lse};
}

// -> dqkv (qkv's shape and dtype), dtable (fp32, table's shape)
std::vector<Tensor> window_attn_bwd(Tensor qkv, Tensor table, Tensor lse, Tensor dout, int64_t window,
                                    int64_t shift, int64_t heads) {
  const WaDims w = wa_check(qkv, table, window, shift, heads);
  need_contig(lse, "lse");
  need_contig(dout, "dout");
  TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.numel() == (int64_t)w.B * w.nW * w.heads * w.N &&
                  lse.device() == qkv.device(), "window_attn_bwd: lse must be fp32 [B, nW, heads, N]");
  TORCH_CHECK(dout.scalar_type() == qkv.scalar_type() && dout.dim() == 4 && dout.size(0) == w.B &&
                  dout.size(1) == w.ph && dout.size(2) == w.pw && dout.size(3) == w.C &&
                  dout.device() == qkv.device(), "window_attn_bwd: dout must be [B, ph, pw, C] of qkv's dtype");
  auto dqkv = torch::empty_like(qkv);
  auto f32 = qkv.options().dtype(at::kFloat);
  auto partials = torch::empty({(int64_t)w.B * w.nW, w.E * w.heads}, f32);
  auto dtable = torch::empty({w.E, (int64_t)w.heads}, f32);
  check(smdt_window_attn_bwd(dcode(qkv), qkv.data_ptr(), table.data_ptr<float>(), lse.data_ptr<float>(),
                             dout.data_ptr(), dqkv.data_ptr(), partials.data_ptr<float>(),
                             dtable.data_ptr<float>(), w.B, w.ph, w.pw, w.heads, w.ws, w.shift, cur_stream()),
        "window_attn_bwd");
  return {dqkv, dtable};
}

// ------------------------------------------------------------------ incremental decoding
// q [B, nh, D], caches [B, cap, nkv, D], lens int32 [B] on the device (valid keys per sequence, the
// new token included); max_len <= cap bounds the grid (0: cap). Everything the kernel does not
// take is refused here, before any launch.
static bool aligned16(const Tensor& t) { return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0; }

static void dec_check_cache(const Tensor& k_cache, const Tensor& v_cache, const Tensor& like, const char* what) {
  need_contig(k_cache, "k_cache");
  need_contig(v_cache, "v_cache");
  TORCH_CHECK(like.scalar_type() == at::kBFloat16 || like.scalar_type() == at::kHalf, what,
              ": bf16 or fp16 operands, got ", like.scalar_type());
  TORCH_CHECK(k_cache.dim() == 4 && v_cache.sizes() == k_cache.sizes() && k_cache.scalar_type() == like.scalar_type() &&
                  v_cache.scalar_type() == like.scalar_type() && k_cache.device() == like.device() &&
                  v_cache.device() == like.device() && k_cache.size(0) == like.size(0),
              what, ": k_cache / v_cache must be [B, cap, nkv, D] of the new token's dtype and device");
  TORCH_CHECK(k_cache.size(1) > 0 && k_cache.size(1) < (1LL << 31) && k_cache.size(0) <= 65535 &&
                  k_cache.size(2) <= 65535, what, ": cache shape out of range");
}

static const int* dec_index(const Tensor& t, const Tensor& like, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device() && t.scalar_type() == at::kInt && t.dim() == 1 &&
                  t.size(0) == like.size(0) && t.is_contiguous(),
              what, ": lens / pos must be a contiguous int32 [B] tensor on the operands' device");
  return t.data_ptr<int>();
}

int64_t decode_attn_chunk() { return smdt_decode_attn_chunk(); }

// What an attention op allocates: the checked max_len (0: cap) and the split-KV workspaces of its
// `heads` partial rows per sequence (nh, or T nh for the multi-token step).
struct DecWork {
  int64_t max_len;
  Tensor ws_ml, ws_acc;
};
static DecWork dec_work(const Tensor& q, int64_t cap, int64_t max_len, int64_t heads, int64_t D, const char* what) {
  if (max_len <= 0) max_len = cap;
  TORCH_CHECK(max_len <= cap, what, ": max_len ", max_len, " exceeds the cache capacity ", cap);
  const int64_t C = smdt_decode_attn_chunk(), nchunks = (max_len + C - 1) / C;
  auto f32 = q.options().dtype(at::kFloat);
  return {max_len, torch::empty({q.size(0), heads, nchunks, 2}, f32), torch::empty({q.size(0), heads, nchunks, D}, f32)};
}

bool decode_attn_supported(int64_t dtype, int64_t D, int64_t nh, int64_t nkv) {
  return nh < (1 << 20) && nkv < (1 << 20) && D < (1 << 20) &&
         smdt_decode_attn_supported((int)dtype, (int)D, (int)nh, (int)nkv) != 0;
}

Tensor decode_attn(Tensor q, Tensor k_cache, Tensor v_cache, Tensor lens, double scale, int64_t max_len) {
  need_contig(q, "q");
  TORCH_CHECK(q.dim() == 3, "decode_attn: q must be [B, nh, D]");
  dec_check_cache(k_cache, v_cache, q, "decode_attn");
  const int64_t B = q.size(0), nh = q.size(1), D = q.size(2), cap = k_cache.size(1), nkv = k_cache.size(2);
  TORCH_CHECK(k_cache.size(3) == D, "decode_attn: head dim of q and the caches differ");
  TORCH_CHECK(decode_attn_supported(dcode(q), D, nh, nkv),
              "decode_attn: unsupported (needs D in {64, 128} and nh / nkv in {1, 2, 4, 8}): D ", D, ", nh ", nh,
              ", nkv ", nkv);
  const DecWork w = dec_work(q, cap, max_len, nh, D, "decode_attn");
  const int* lp = dec_index(lens, q, "decode_attn");
  auto out = torch::empty_like(q);
  check(smdt_decode_attn(dcode(q), q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), lp,
                         w.ws_ml.data_ptr<float>(), w.ws_acc.data_ptr<float>(), out.data_ptr(), (int)B, (int)nh,
                         (int)nkv, (int)D, (int)cap, (int)w.max_len, (float)scale, cur_stream()),
        "decode_attn");
  return out;
}

// cos / sin (fp32 [max_pos, rot / 2]) of an op that rotates the first rot elements (rot == 0: none).
struct RopeTables {
  const float *cos = nullptr, *sin = nullptr;
  int64_t max_pos = 0;
};
static RopeTables dec_rope_tables(const OptT& cos_t, const OptT& sin_t, int64_t rot, int64_t D, const Tensor& qkv,
                                  const char* what) {
  RopeTables rt;
  if (rot > 0) {
    TORCH_CHECK(cos_t.has_value() && sin_t.has_value(), what, ": rot > 0 needs the cos / sin tables");
    need_contig(*cos_t, "cos");
    need_contig(*sin_t, "sin");
    TORCH_CHECK(cos_t->scalar_type() == at::kFloat && sin_t->scalar_type() == at::kFloat && cos_t->dim() == 2 &&
                    sin_t->sizes() == cos_t->sizes() && cos_t->device() == qkv.device() &&
                    sin_t->device() == qkv.device(),
                what, ": fp32 [max_pos, rot / 2] tables on qkv's device");
    TORCH_CHECK(rot <= D && rot % 16 == 0 && cos_t->size(1) == rot / 2, what, ": rotary dim mismatch");
    rt.max_pos = cos_t->size(0);
    TORCH_CHECK(rt.max_pos < (1LL << 31), what, ": table too long");
    rt.cos = cos_t->data_ptr<float>();
    rt.sin = sin_t->data_ptr<float>();
  } else {
    TORCH_CHECK(rot == 0, what, ": negative rotary dim");
  }
  return rt;
}

// The qkv row width of an append op: (nh + 2 nkv) D with D % 8 == 0.
static void dec_check_qkv(const Tensor& qkv, int64_t nh, int64_t nkv, int64_t D, const char* what) {
  const int64_t W = qkv.size(-1);
  TORCH_CHECK(nh > 0 && nh < (1 << 20) && D % 8 == 0 && D < (1 << 20) && W == (nh + 2 * nkv) * D, what,
              ": qkv width ", W, " is not (nh + 2 nkv) D with D % 8 == 0");
}

// The 16-bit append of both decode steps (one kernel, decode_attn_multi.hip). cos / sin (fp32
// [max_pos, rot / 2]) and rot > 0 rotate q and k; without them the op is a copy.
//   qkv [B, (nh + 2 nkv) D], contiguous: one new token per sequence, rotated at pos[b] and written
//     into cache row pos[b]; -> q [B, nh, D] (`decode_rope_append` in the messages).
//   qkv [B, T, (nh + 2 nkv) D]: any batch / token strides (multiples of 8 elements) over contiguous
//     rows, so the model's sequence-first [T, B, W] is passed as a transposed view without a copy.
//     Token t of sequence b is rotated at pos[b] + t and appended to that cache row; -> q [B, T, nh,
//     D] (`decode_rope_append_multi`).
Tensor decode_rope_append(Tensor qkv, Tensor k_cache, Tensor v_cache, Tensor pos, int64_t nh, OptT cos_t,
                          OptT sin_t, int64_t rot) {
  const bool multi = qkv.dim() == 3;
  const char* what = multi ? "decode_rope_append_multi" : "decode_rope_append";
  if (multi) {
    TORCH_CHECK(qkv.is_cuda(), "decode_rope_append_multi: qkv must be a GPU [B, T, (nh + 2 nkv) D]");
  } else {
    need_contig(qkv, "qkv");
    TORCH_CHECK(qkv.dim() == 2, "decode_rope_append: qkv must be [B, (nh + 2 nkv) D]");
  }
  dec_check_cache(k_cache, v_cache, qkv, what);
  const int64_t B = qkv.size(0), T = multi ? qkv.size(1) : 1, cap = k_cache.size(1), nkv = k_cache.size(2),
                D = k_cache.size(3);
  if (multi)
    TORCH_CHECK(T >= 1 && T <= smdt_decode_attn_multi_max_t(), "decode_rope_append_multi: T ", T, " is outside 1 .. ",
                smdt_decode_attn_multi_max_t());
  dec_check_qkv(qkv, nh, nkv, D, what);
  if (multi)
    TORCH_CHECK(qkv.stride(2) == 1 && qkv.stride(0) % 8 == 0 && qkv.stride(1) % 8 == 0 && qkv.stride(0) >= 0 &&
                    qkv.stride(1) >= 0 && aligned16(qkv),
                "decode_rope_append_multi: qkv rows must be contiguous and 16-byte aligned (strides ", qkv.strides(), ")");
  const int* pp = dec_index(pos, qkv, what);
  const RopeTables rt = dec_rope_tables(cos_t, sin_t, rot, D, qkv, what);
  auto q = multi ? torch::empty({B, T, nh, D}, qkv.options()) : torch::empty({B, nh, D}, qkv.options());
  check(smdt_decode_rope_append_multi(dcode(qkv), qkv.data_ptr(), multi ? qkv.stride(0) : qkv.size(1),
                                      multi ? qkv.stride(1) : 0, q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
                                      pp, (int)B, (int)T, (int)nh, (int)nkv, (int)D, (int)cap, (int)rot, rt.cos, rt.sin,
                                      (int)rt.max_pos, cur_stream()),
        what);
  return q;
}

// ------------------------------------------------------------------ multi-token decode (decode_attn_multi.hip)
// q [B, T, nh, D] against the 16-bit caches; lens counts the keys after the T appends and query t
// sees keys 0 .. lens[b] - T + t. Returns out [B, T, nh, D].
int64_t decode_attn_multi_max_t() { return smdt_decode_attn_multi_max_t(); }

bool decode_attn_multi_supported(int64_t dtype, int64_t D, int64_t nh, int64_t nkv, int64_t T) {
  return nh < (1 << 20) && nkv < (1 << 20) && D < (1 << 20) && T < (1 << 20) &&
         smdt_decode_attn_multi_supported((int)dtype, (int)D, (int)nh, (int)nkv, (int)T) != 0;
}

Tensor decode_attn_multi(Tensor q, Tensor k_cache, Tensor v_cache, Tensor lens, double scale, int64_t max_len) {
  need_contig(q, "q");
  TORCH_CHECK(q.dim() == 4, "decode_attn_multi: q must be [B, T, nh, D]");
  dec_check_cache(k_cache, v_cache, q, "decode_attn_multi");
  const int64_t B = q.size(0), T = q.size(1), nh = q.size(2), D = q.size(3), cap = k_cache.size(1),
                nkv = k_cache.size(2);
  TORCH_CHECK(k_cache.size(3) == D, "decode_attn_multi: head dim of q and the caches differ");
  TORCH_CHECK(decode_attn_multi_supported(dcode(q), D, nh, nkv, T) && T * nh <= 65535,
              "decode_attn_multi: unsupported (needs D in {64, 128}, nh / nkv in {1, 2, 4, 8} and 1 <= T <= ",
              smdt_decode_attn_multi_max_t(), "): D ", D, ", nh ", nh, ", nkv ", nkv, ", T ", T);
  TORCH_CHECK(aligned16(q) && aligned16(k_cache) && aligned16(v_cache),
              "decode_attn_multi: q and the caches must be 16-byte aligned");
  const DecWork w = dec_work(q, cap, max_len, T * nh, D, "decode_attn_multi");
  const int* lp = dec_index(lens, q, "decode_attn_multi");
  auto out = torch::empty_like(q);
  check(smdt_decode_attn_multi(dcode(q), q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), lp,
                               w.ws_ml.data_ptr<float>(), w.ws_acc.data_ptr<float>(), out.data_ptr(), (int)B, (int)T,
                               (int)nh, (int)nkv, (int)D, (int)cap, (int)w.max_len, (float)scale, cur_stream()),
        "decode_attn_multi");
  return out;
}

// ------------------------------------------------------------------ MXFP8 K/V cache (decode_attn_mx.hip)
// kq / vq [B, cap, nkv, D] E4M3, ksc / vsc [B, cap, nkv, D / 32] uint8 E8M0; q / qkv stay 16-bit.
static void dec_check_cache_mx(const Tensor& kq, const Tensor& ks, const Tensor& vq, const Tensor& vs,
                               const Tensor& like, const char* what) {
  TORCH_CHECK(like.scalar_type() == at::kBFloat16 || like.scalar_type() == at::kHalf, what,
              ": bf16 or fp16 q / qkv, got ", like.scalar_type());
  for (const Tensor* t : {&kq, &ks, &vq, &vs}) {
    TORCH_CHECK(t->is_cuda() && t->device() == like.device() && t->is_contiguous() && t->dim() == 4 && aligned16(*t),
                what, ": the cache tensors must be contiguous, 16-byte aligned and 4-D on the new token's device");
  }
  TORCH_CHECK(kq.scalar_type() == at::kFloat8_e4m3fn && vq.scalar_type() == at::kFloat8_e4m3fn &&
                  ks.scalar_type() == at::kByte && vs.scalar_type() == at::kByte,
              what, ": the cache must be float8_e4m3fn elements and uint8 (E8M0) scales");
  const int64_t D = kq.size(3);
  TORCH_CHECK(D % 32 == 0 && vq.sizes() == kq.sizes() && vs.sizes() == ks.sizes() && ks.size(0) == kq.size(0) &&
                  ks.size(1) == kq.size(1) && ks.size(2) == kq.size(2) && ks.size(3) == D / 32 &&
                  kq.size(0) == like.size(0),
              what, ": the cache must be q [B, cap, nkv, D] and s [B, cap, nkv, D / 32] with D % 32 == 0");
  TORCH_CHECK(kq.size(1) > 0 && kq.size(1) < (1LL << 31) && kq.size(0) <= 65535 && kq.size(2) <= 65535, what,
              ": cache shape out of range");
}

Tensor decode_attn_mx(Tensor q, Tensor kq, Tensor ks, Tensor vq, Tensor vs, Tensor lens, double scale,
                      int64_t max_len) {
  need_contig(q, "q");
  TORCH_CHECK(q.dim() == 3, "decode_attn_mx: q must be [B, nh, D]");
  dec_check_cache_mx(kq, ks, vq, vs, q, "decode_attn_mx");
  const int64_t B = q.size(0), nh = q.size(1), D = q.size(2), cap = kq.size(1), nkv = kq.size(2);
  TORCH_CHECK(kq.size(3) == D, "decode_attn_mx: head dim of q and the cache differ");
  TORCH_CHECK(decode_attn_supported(dcode(q), D, nh, nkv),
              "decode_attn_mx: unsupported (needs D in {64, 128} and nh / nkv in {1, 2, 4, 8}): D ", D, ", nh ", nh,
              ", nkv ", nkv);
  TORCH_CHECK(aligned16(q), "decode_attn_mx: q must be 16-byte aligned");
  const DecWork w = dec_work(q, cap, max_len, nh, D, "decode_attn_mx");
  const int* lp = dec_index(lens, q, "decode_attn_mx");
  auto out = torch::empty_like(q);
  check(smdt_decode_attn_mx(dcode(q), q.data_ptr(), kq.data_ptr(), ks.data_ptr(), vq.data_ptr(), vs.data_ptr(), lp,
                            w.ws_ml.data_ptr<float>(), w.ws_acc.data_ptr<float>(), out.data_ptr(), (int)B, (int)nh,
                            (int)nkv, (int)D, (int)cap, (int)w.max_len, (float)scale, cur_stream()),
        "decode_attn_mx");
  return out;
}

Tensor decode_rope_append_mx(Tensor qkv, Tensor kq, Tensor ks, Tensor vq, Tensor vs, Tensor pos, int64_t nh,
                             OptT cos_t, OptT sin_t, int64_t rot) {
  need_contig(qkv, "qkv");
  TORCH_CHECK(qkv.dim() == 2, "decode_rope_append_mx: qkv must be [B, (nh + 2 nkv) D]");
  dec_check_cache_mx(kq, ks, vq, vs, qkv, "decode_rope_append_mx");
  const int64_t B = qkv.size(0), cap = kq.size(1), nkv = kq.size(2), D = kq.size(3);
  dec_check_qkv(qkv, nh, nkv, D, "decode_rope_append_mx");
  TORCH_CHECK(nkv * D <= 8192, "decode_rope_append_mx: nkv * D = ", nkv * D, " exceeds 8192 (the kernel stages the "
              "token's k and v rows in LDS)");
  TORCH_CHECK(aligned16(qkv), "decode_rope_append_mx: qkv must be 16-byte aligned");
  const int* pp = dec_index(pos, qkv, "decode_rope_append_mx");
  const RopeTables rt = dec_rope_tables(cos_t, sin_t, rot, D, qkv, "decode_rope_append_mx");
  auto q = torch::empty({B, nh, D}, qkv.options());
  check(smdt_decode_rope_append_mx(dcode(qkv), qkv.data_ptr(), q.data_ptr(), kq.data_ptr(), ks.data_ptr(),
                                   vq.data_ptr(), vs.data_ptr(), pp, (int)B, (int)nh, (int)nkv, (int)D, (int)cap,
                                   (int)rot, rt.cos, rt.sin, (int)rt.max_pos, cur_stream()),
        "decode_rope_append_mx");
  return q;
}

// ------------------------------------------------------------------ decode linear (decode_linear.hip)
// fmt: 0 native, 1 mxfp8, 2 mxfp4. The limits live in smdt_decode_linear_supported alone.
bool decode_linear_supported(int64_t dtype, int64_t fmt, int64_t M, int64_t N, int64_t K) {
  return fmt >= 0 && fmt <= 2 && smdt_decode_linear_supported((int)dtype, (int)fmt, M, N, K) != 0;
}

// {rows per workgroup, largest M, "split K below this many workgroups", k per workgroup step and
// steps per unrolled iteration for fmt 0, 1, 2}
std::vector<int64_t> decode_linear_constants() {
  return {smdt_decode_linear_rows(), smdt_decode_linear_max_m(), smdt_decode_linear_split_below(),
          smdt_decode_linear_step_k(0), smdt_decode_linear_step_k(1), smdt_decode_linear_step_k(2),
          smdt_decode_linear_unroll(0), smdt_decode_linear_unroll(1), smdt_decode_linear_unroll(2)};
}

// (splits, slice length in k) of a weight [N, K] in format fmt
std::vector<int64_t> decode_linear_plan(int64_t fmt, int64_t N, int64_t K) {
  TORCH_CHECK(fmt >= 0 && fmt <= 2 && N >= 8 && K >= 32 && N < (1LL << 30) && K < (1LL << 30),
              "decode_linear_plan: fmt ", fmt, ", N ", N, ", K ", K);
  int s = 1, sl = 0;
  smdt_decode_linear_plan((int)fmt, N, K, &s, &sl);
  return {s, sl};
}

Tensor decode_linear(Tensor x, Tensor w, OptT scales, OptT bias, int64_t fmt, OptT workspace, OptT out_) {
  need_contig(x, "x");
  need_contig(w, "w");
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2, "decode_linear: x must be [M, K] and w 2-D");
  TORCH_CHECK(fmt >= 0 && fmt <= 2, "decode_linear: fmt must be 0 (native), 1 (mxfp8) or 2 (mxfp4), got ", fmt);
  const int64_t M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kHalf, "decode_linear: bf16 or fp16 x, got ",
              x.scalar_type());
  TORCH_CHECK(fmt == 0 || x.scalar_type() == at::kBFloat16,
              "decode_linear: the quantised formats dequantise to bf16 (fp16 cannot hold the small blocks); x is ",
              x.scalar_type());
  TORCH_CHECK(decode_linear_supported(dcode(x), fmt, M, N, K), "decode_linear: unsupported M x N x K = ", M, " x ", N,
              " x ", K, " (smdt_decode_linear_supported; the largest M is ", smdt_decode_linear_max_m(), ")");
  TORCH_CHECK(w.device() == x.device(), "decode_linear: w is on another device");
  const void* sp = nullptr;
  if (fmt == 0) {
    TORCH_CHECK(w.scalar_type() == x.scalar_type() && w.size(1) == K, "decode_linear: native w must be [N, K] of x's "
                "dtype, got ", w.sizes(), " ", w.scalar_type());
  } else {
    TORCH_CHECK(scales.has_value(), "decode_linear: the quantised formats need scales");
    need_contig(*scales, "scales");
    TORCH_CHECK(scales->scalar_type() == at::kByte && scales->dim() == 2 && scales->size(0) == N &&
                    scales->size(1) == K / 32 && scales->device() == x.device(),
                "decode_linear: scales must be uint8 [N, K / 32] on x's device");
    if (fmt == 1) {
      TORCH_CHECK(w.scalar_type() == at::kFloat8_e4m3fn && w.size(1) == K, "decode_linear: mxfp8 w must be E4M3 [N, K]");
    } else {
      TORCH_CHECK(w.scalar_type() == at::kByte && w.size(1) == K / 2, "decode_linear: mxfp4 w must be uint8 [N, K / 2]");
    }
    sp = scales->data_ptr();
  }
  const void* bp = nullptr;
  if (bias.has_value()) {
    need_contig(*bias, "bias");
    TORCH_CHECK(bias->scalar_type() == x.scalar_type() && bias->dim() == 1 && bias->size(0) == N &&
                    bias->device() == x.device(), "decode_linear: bias must be [N] of x's dtype on its device");
    bp = bias->data_ptr();
  }
  TORCH_CHECK(aligned16(x) && aligned16(w), "decode_linear: x and w must be 16-byte aligned");
  int S = 1, slice = 0;
  smdt_decode_linear_plan((int)fmt, N, K, &S, &slice);
  float* wsp = nullptr;
  if (S > 1) {
    TORCH_CHECK(workspace.has_value(), "decode_linear: N ", N, " x K ", K, " splits K ", S,
                " ways and needs a workspace of ", S * M * N, " fp32 elements");
    TORCH_CHECK(workspace->scalar_type() == at::kFloat && workspace->is_contiguous() && workspace->device() == x.device() &&
                    workspace->numel() >= S * M * N && aligned16(*workspace),
                "decode_linear: the workspace must be contiguous fp32 on x's device with at least ", S * M * N, " elements");
    wsp = workspace->data_ptr<float>();
  }
  Tensor out;
  if (out_.has_value()) {
    out = *out_;
    need_contig(out, "out");
    TORCH_CHECK(out.dim() == 2 && out.size(0) == M && out.size(1) == N && out.scalar_type() == x.scalar_type() &&
                    out.device() == x.device() && aligned16(out),
                "decode_linear: out must be a contiguous, 16-byte aligned [M, N] tensor of x's dtype on its device");
  } else {
    out = torch::empty({M, N}, x.options());
  }
  check(smdt_decode_linear(dcode(x), (int)fmt, x.data_ptr(), w.data_ptr(), sp, bp, out.data_ptr(), wsp, M, N, K,
                           cur_stream()),
        "decode_linear");
  return out;
}

// `out` (optional) is a preallocated [B, S, H, D] view with any strides (e.g. the [s, b, h]
// activation layout used by the transformer trunk). `doc_start` (optional, causal only) selects the
// per-document kernels.
std::vector<Tensor> flash_fwd(Tensor q, Tensor k, Tensor v, double scale, bool causal, OptT out,
                              double dropout_p, int64_t seed, int64_t offset, OptT doc_start) {
  fa_check(q, "q"); fa_check(k, "k"); fa_check(v, "v");
  TORCH_CHECK(k.scalar_type() == q.scalar_type() && v.scalar_type() == q.scalar_type(), "flash: q/k/v dtypes differ");
  const int64_t B = q.size(0), S = q.size(1), H = q.size(2), D = q.size(3), Hkv = k.size(2);
  TORCH_CHECK(k.size(0) == B && k.size(1) == S && k.size(3) == D && v.sizes() == k.sizes(), "flash: k/v shape mismatch");
  TORCH_CHECK((D == 64 || D == 128) && S % 128 == 0 && H % Hkv == 0, "flash: needs D in {64,128}, S % 128 == 0, H % Hkv == 0");
  Tensor o;
  if (out) {
    o = *out;
    fa_check(o, "out");
    TORCH_CHECK(o.sizes() == q.sizes(), "flash: out shape mismatch");
  } else {
    o = torch::empty({B, S, H, D}, q.options());
  }
  auto lse = torch::empty({B, H, S}, q.options().dtype(at::kFloat));
  TORCH_CHECK(o.scalar_type() == q.scalar_type(), "flash: out dtype mismatch");
  if (const int* ds = fa_doc_ptr(doc_start, q, "doc_start")) {
    TORCH_CHECK(causal, "flash: doc_start needs causal attention");
    check(smdt_flash_fwd_doc(dcode(q), q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                             lse.data_ptr<float>(), (int)B, (int)H, (int)Hkv, (int)S, (int)D, q.stride(0),
                             q.stride(1), q.stride(2), k.stride(0), k.stride(1), k.stride(2), v.stride(0),
                             v.stride(1), v.stride(2), o.stride(0), o.stride(1), o.stride(2), (float)scale,
                             (float)dropout_p, (uint64_t)seed, (uint64_t)offset, ds, cur_stream()),
          "flash_fwd_doc");
    return {o, lse};
  }
  check(smdt_flash_fwd(dcode(q), q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr<float>(),
                       (int)B, (int)H, (int)Hkv, (int)S, (int)D, q.stride(0), q.stride(1), q.stride(2),
                       k.stride(0), k.stride(1), k.stride(2), v.stride(0), v.stride(1), v.stride(2),
                       o.stride(0), o.stride(1), o.stride(2), (float)scale, causal ? 1 : 0, (float)dropout_p,
                       (uint64_t)seed, (uint64_t)offset, cur_stream()),
        "flash_fwd");
  return {o, lse};
}

// dq / dk / dv (optional) are preallocated [B, S, H(kv), D] views with any strides, typically
// views into one fused d(QKV) buffer so the QKV projection backward needs no concatenation.
// ``dbias`` (flash_bwd_dbias; fp32 [(H + 2 Hkv) D]): = / += the sums over all tokens of the fp32
// dQ | dK | dV before their 16-bit rounding, i.e. the bias gradient of the fused QKV projection
// whose output q / k / v are views of — per-block partials from the kernels, added in a fixed
// order by the column-sum kernel (no atomics, bitwise reproducible).
static std::vector<Tensor> flash_bwd_any(Tensor q, Tensor k, Tensor v, Tensor o, Tensor dout, Tensor lse,
                                         double scale, bool causal, OptT dq_out, OptT dk_out, OptT dv_out,
                                         double dropout_p, int64_t seed, int64_t offset, OptT doc_start,
                                         OptT doc_end, OptT dbias, bool accumulate) {
  fa_check(q, "q"); fa_check(k, "k"); fa_check(v, "v"); fa_check(o, "o");
  TORCH_CHECK(k.scalar_type() == q.scalar_type() && v.scalar_type() == q.scalar_type() &&
              o.scalar_type() == q.scalar_type() && dout.scalar_type() == q.scalar_type(), "flash_bwd: dtypes differ");
  const int64_t B = q.size(0), S = q.size(1), H = q.size(2), D = q.size(3), Hkv = k.size(2);
  TORCH_CHECK((D == 64 || D == 128) && S % 128 == 0 && H % Hkv == 0, "flash_bwd: unsupported shape");
  TORCH_CHECK(dout.sizes() == o.sizes(), "flash_bwd: dout shape mismatch");
  if (dout.stride(3) != 1 || dout.stride(0) % 8 || dout.stride(1) % 8 || dout.stride(2) % 8) dout = dout.contiguous();
  fa_check(dout, "dout");
  TORCH_CHECK(lse.is_contiguous() && lse.numel() == B * H * S, "flash_bwd: lse mismatch");
  auto mk = [&](const OptT& given, int64_t heads, const char* n) {
    if (given) {
      fa_check(*given, n);
      TORCH_CHECK(given->size(0) == B && given->size(1) == S && given->size(2) == heads && given->size(3) == D,
                  "flash_bwd: '", n, "' shape mismatch");
      return *given;
    }
    return torch::empty({B, S, heads, D}, q.options());
  };
  Tensor dq = mk(dq_out, H, "dq"), dk = mk(dk_out, Hkv, "dk"), dv = mk(dv_out, Hkv, "dv");
  // -delta' rows | (unused) | 16-byte term rows of -lse log2 e and of -delta' (flash_attn.hip)
  auto delta = torch::empty({10, B, H, S}, q.options().dtype(at::kFloat));
  int64_t st[24];
  const Tensor* ts[8] = {&q, &k, &v, &o, &dout, &dq, &dk, &dv};
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < 3; ++j) st[3 * i + j] = ts[i]->stride(j);
  const int* ds = fa_doc_ptr(doc_start, q, "doc_start");
  const int* de = fa_doc_ptr(doc_end, q, "doc_end");
  TORCH_CHECK((ds == nullptr) == (de == nullptr), "flash_bwd: doc_start and doc_end come together");
  if (dbias) {
    TORCH_CHECK(!ds || causal, "flash_bwd: doc_start needs causal attention");
    const int64_t N = (H + 2 * Hkv) * D, nblk = B * (S / 128);
    Tensor db = acc_target(dbias, N, "flash_bwd_dbias dbias");
    TORCH_CHECK(db.device() == q.device(), "flash_bwd_dbias: dbias on another device");
    auto part = torch::empty({nblk, N}, q.options().dtype(at::kFloat));
    check(smdt_flash_bwd_sums(dcode(q), q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), dout.data_ptr(),
                              lse.data_ptr<float>(), delta.data_ptr<float>(), dq.data_ptr(), dk.data_ptr(),
                              dv.data_ptr(), (int)B, (int)H, (int)Hkv, (int)S, (int)D, st, (float)scale,
                              causal ? 1 : 0, (float)dropout_p, (uint64_t)seed, (uint64_t)offset, ds, de,
                              part.data_ptr<float>(), cur_stream()),
          "flash_bwd_dbias");
    check(smdt_col_sum(part.data_ptr<float>(), (int)nblk, (int)N, db.data_ptr<float>(), accumulate ? 1 : 0,
                       cur_stream()),
          "flash_bwd_dbias column sums");
    return {dq, dk, dv};
  }
  if (ds) {
    TORCH_CHECK(causal, "flash_bwd: doc_start needs causal attention");
    check(smdt_flash_bwd_doc(dcode(q), q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), dout.data_ptr(),
                             lse.data_ptr<float>(), delta.data_ptr<float>(), dq.data_ptr(), dk.data_ptr(),
                             dv.data_ptr(), (int)B, (int)H, (int)Hkv, (int)S, (int)D, st, (float)scale,
                             (float)dropout_p, (uint64_t)seed, (uint64_t)offset, ds, de, cur_stream()),
          "flash_bwd_doc");
    return {dq, dk, dv};
  }
  check(smdt_flash_bwd(dcode(q), q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), dout.data_ptr(),
                       lse.data_ptr<float>(), delta.data_ptr<float>(), dq.data_ptr(), dk.data_ptr(),
                       dv.data_ptr(), (int)B, (int)H, (int)Hkv, (int)S, (int)D, st, (float)scale,
                       causal ? 1 : 0, (float)dropout_p, (uint64_t)seed, (uint64_t)offset, cur_stream()),
        "flash_bwd");
  return {dq, dk, dv};
}

std::vector<Tensor> flash_bwd(Tensor q, Tensor k, Tensor v, Tensor o, Tensor dout, Tensor lse,
                              double scale, bool causal, OptT dq_out, OptT dk_out, OptT dv_out,
                              double dropout_p, int64_t seed, int64_t offset, OptT doc_start, OptT doc_end) {
  return flash_bwd_any(q, k, v, o, dout, lse, scale, causal, dq_out, dk_out, dv_out, dropout_p, seed, offset,
                       doc_start, doc_end, c10::nullopt, false);
}

std::vector<Tensor> flash_bwd_dbias(Tensor q, Tensor k, Tensor v, Tensor o, Tensor dout, Tensor lse,
                                    double scale, bool causal, Tensor dbias, bool accumulate, OptT dq_out,
                                    OptT dk_out, OptT dv_out, double dropout_p, int64_t seed, int64_t offset,
                                    OptT doc_start, OptT doc_end) {
  return flash_bwd_any(q, k, v, o, dout, lse, scale, causal, dq_out, dk_out, dv_out, dropout_p, seed, offset,
                       doc_start, doc_end, dbias, accumulate);
}

// ------------------------------------------------------------------ xGMI all-reduce (HIP IPC)
// Raw device pointers cross the Python boundary as int64 (they are IPC mappings, not tensors).
void* vp(int64_t p) { return reinterpret_cast<void*>(static_cast<uintptr_t>(p)); }

int64_t ipc_malloc(int64_t bytes, bool uncached) {
  TORCH_CHECK(bytes > 0, "ipc_malloc: bytes must be positive");
  void* p = nullptr;
  check(smdt_ipc_malloc(bytes, uncached ? 1 : 0, &p), "ipc_malloc");
  return (int64_t)(uintptr_t)p;
}

void ipc_free(int64_t p) { check(smdt_ipc_free(vp(p)), "ipc_free"); }

pybind11::bytes ipc_get_handle(int64_t p) {
  std::string h((size_t)smdt_ipc_handle_bytes(), '\0');
  check(smdt_ipc_get_handle(vp(p), h.data()), "ipc_get_handle");
  return pybind11::bytes(h);
}

int64_t ipc_open(pybind11::bytes handle) {
  const std::string h = handle;
  TORCH_CHECK((int)h.size() == smdt_ipc_handle_bytes(), "ipc_open: handle must be ", smdt_ipc_handle_bytes(), " bytes");
  void* p = nullptr;
  check(smdt_ipc_open(h.data(), &p), "ipc_open");
  return (int64_t)(uintptr_t)p;
}

void ipc_close(int64_t p) { check(smdt_ipc_close(vp(p)), "ipc_close"); }

// One uint32 word of an engine's (uncached) signal buffer as an int32 tensor aliasing device
// memory: the DDP reads the sticky error word back asynchronously (no host sync in the step), and
// tests lower the spin limit to inject a timeout. The tensor does not own the memory.
Tensor signal_word(int64_t sig, int64_t byte_offset) {
  TORCH_CHECK(sig != 0 && byte_offset >= 0 && byte_offset % 4 == 0, "signal_word: bad pointer / offset");
  auto opts = torch::TensorOptions().dtype(torch::kInt32).device(torch::kCUDA, c10::hip::current_device());
  return torch::from_blob(static_cast<char*>(vp(sig)) + byte_offset, {1}, opts);
}

int64_t ar_read_error(int64_t sig) {
  int e = 0;
  check(smdt_ar_read_error(vp(sig), &e), "ar_read_error");
  return e;
}

// out = scale * sum_ranks(in). nranks_local > 1 (loopback tests): in/out are [nranks_local, n]
// and ranks rank .. rank + nranks_local - 1 run in one launch.
void xgmi_allreduce(Tensor in, Tensor out, std::vector<int64_t> data_ptrs, std::vector<int64_t> sig_ptrs,
                    int64_t rank, int64_t nranks_local, int64_t region_bytes, bool two_shot, int64_t blocks,
                    double scale) {
  need_contig(in, "in");
  need_contig(out, "out");
  TORCH_CHECK(in.sizes() == out.sizes() && in.dtype() == out.dtype() && in.device() == out.device(),
              "xgmi_allreduce: in / out mismatch");
  const int world = (int)data_ptrs.size();
  TORCH_CHECK(sig_ptrs.size() == data_ptrs.size() && world >= 2 && world <= smdt_ar_max_ranks(),
              "xgmi_allreduce: need 2..", smdt_ar_max_ranks(), " ranks");
  TORCH_CHECK(blocks >= 1 && blocks <= smdt_ar_max_blocks(), "xgmi_allreduce: blocks out of range");
  int64_t n = in.numel(), stride = 0;
  if (nranks_local > 1) {
    TORCH_CHECK(in.dim() >= 2 && in.size(0) == nranks_local, "xgmi_allreduce loopback: in must be [nranks_local, ...]");
    TORCH_CHECK(blocks * nranks_local <= 512, "xgmi_allreduce loopback: blocks x ranks must stay co-resident (<= 512)");
    n /= nranks_local;
    stride = n;
  }
  std::vector<void*> d(world), s(world);
  for (int r = 0; r < world; ++r) {
    d[r] = vp(data_ptrs[r]);
    s[r] = vp(sig_ptrs[r]);
  }
  TORCH_CHECK(in.is_cuda() && in.device().index() == c10::hip::current_device(),
              "xgmi_allreduce: tensors must live on the current device");
  check(smdt_xgmi_allreduce(dcode(in), in.data_ptr(), out.data_ptr(), stride, n, (float)scale, d.data(), s.data(),
                            world, (int)rank, (int)nranks_local, region_bytes, two_shot ? 1 : 0, (int)blocks,
                            cur_stream()),
        "xgmi_allreduce");
}


// contiguous, bias [N] or None. epi 0: y = x w^T; 1: + bias; 2: h = x w^T + bias, y = gelu(h).
// Returns [y] or [y, h].
// General form: mode 0/1 all-reduce (n = elements), 2 reduce-scatter, 3 all-gather (n = elements
// per slice, slices slice_stride elements apart in the input (RS) / output (AG)). in / out are raw
// views (the reduce-scatter output may alias the input's slice `rank`, the all-gather input may
// alias the output's). Loopback (nranks_local > 1): in / out are [nranks_local, ...] with one row
// per virtual rank. Every element the kernel touches is bounds-checked here against the tensors.
void xgmi_collective(int64_t mode, Tensor in, Tensor out, std::vector<int64_t> data_ptrs, std::vector<int64_t> sig_ptrs,
                     int64_t rank, int64_t nranks_local, int64_t region_bytes, int64_t blocks, int64_t n,
                     int64_t slice_stride, double scale) {
  TORCH_CHECK(mode >= 0 && mode <= 3, "xgmi_collective: mode must be 0..3");
  TORCH_CHECK(in.dtype() == out.dtype() && in.device() == out.device(), "xgmi_collective: in / out mismatch");
  TORCH_CHECK(in.is_cuda() && in.device().index() == c10::hip::current_device(),
              "xgmi_collective: tensors must live on the current device");
  const int world = (int)data_ptrs.size();
  TORCH_CHECK(sig_ptrs.size() == data_ptrs.size() && world >= 2 && world <= smdt_ar_max_ranks(),
              "xgmi_collective: need 2..", smdt_ar_max_ranks(), " ranks");
  TORCH_CHECK(blocks >= 1 && blocks <= smdt_ar_max_blocks(), "xgmi_collective: blocks out of range");
  TORCH_CHECK(n > 0, "xgmi_collective: empty message");
  int64_t in_per = in.numel(), out_per = out.numel(), in_rs = 0, out_rs = 0;
  if (nranks_local > 1) {
    TORCH_CHECK(in.dim() == 2 && out.dim() == 2 && in.size(0) == nranks_local && out.size(0) == nranks_local &&
                    in.stride(1) == 1 && out.stride(1) == 1,
                "xgmi_collective loopback: in / out must be [nranks_local, m] with unit inner stride");
    TORCH_CHECK(blocks * nranks_local <= 512, "xgmi_collective loopback: blocks x ranks must stay co-resident (<= 512)");
    in_per = in.size(1);
    out_per = out.size(1);
    in_rs = in.stride(0);
    out_rs = out.stride(0);
  } else {
    TORCH_CHECK(in.is_contiguous() && out.is_contiguous(), "xgmi_collective: contiguous tensors");
  }
  const int64_t span = (int64_t)(world - 1) * slice_stride + n;
  const int64_t need_in = mode == 2 ? span : n, need_out = mode == 3 ? span : n;
  TORCH_CHECK(in_per >= need_in && out_per >= need_out, "xgmi_collective: tensors too small for n = ", n,
              ", slice stride ", slice_stride);
  std::vector<void*> d(world), s(world);
  for (int r = 0; r < world; ++r) {
    d[r] = vp(data_ptrs[r]);
    s[r] = vp(sig_ptrs[r]);
  }
  check(smdt_xgmi_collective((int)mode, dcode(in), in.data_ptr(), out.data_ptr(), in_rs, out_rs, n, slice_stride,
                             (float)scale, d.data(), s.data(), world, (int)rank, (int)nranks_local, region_bytes,
                             (int)blocks, cur_stream()),
        "xgmi_collective");
}

int64_t relay_read_error(int64_t sig) {
  int e = 0;
  check(smdt_relay_read_error(vp(sig), &e), "relay_read_error");
  return e;
}

// Pairwise TP exchange over all xGMI links (xgmi_relay.hip): out (on this rank) = in of the
// partner. Loopback (nranks_local > 1): in / out are [nranks_local, m] rows, one per virtual rank.
void xgmi_relay(Tensor in, Tensor out, std::vector<int64_t> stage_ptrs, std::vector<int64_t> sig_ptrs,
                std::vector<int64_t> partners, int64_t rank, int64_t nranks_local, int64_t slot_bytes, int64_t sub,
                int64_t epoch, bool dev_epoch) {
  TORCH_CHECK(in.dtype() == out.dtype() && in.device() == out.device(), "xgmi_relay: in / out mismatch");
  TORCH_CHECK(in.is_cuda() && in.device().index() == c10::hip::current_device(),
              "xgmi_relay: tensors must live on the current device");
  TORCH_CHECK(in.scalar_type() == at::kFloat || in.scalar_type() == at::kBFloat16 || in.scalar_type() == at::kHalf,
              "xgmi_relay: fp32 / bf16 / fp16");
  const int world = (int)stage_ptrs.size();
  TORCH_CHECK(sig_ptrs.size() == stage_ptrs.size() && partners.size() == stage_ptrs.size() &&
                  (world == 2 || world == 4 || world == 8),
              "xgmi_relay: 2, 4 or 8 ranks");
  TORCH_CHECK(sub >= 1 && sub <= smdt_relay_max_sub(), "xgmi_relay: sub out of range");
  TORCH_CHECK(epoch >= 1 && epoch <= 0xffffffffll, "xgmi_relay: epoch must be a positive uint32");
  int64_t n = in.numel(), in_rs = 0, out_rs = 0;
  if (nranks_local > 1) {
    TORCH_CHECK(in.dim() == 2 && out.dim() == 2 && in.size(0) == nranks_local && out.size(0) == nranks_local &&
                    in.stride(1) == 1 && out.stride(1) == 1 && out.size(1) == in.size(1),
                "xgmi_relay loopback: in / out must be [nranks_local, m] with unit inner stride");
    TORCH_CHECK(2 * sub * world * nranks_local <= 512, "xgmi_relay loopback: blocks must stay co-resident (<= 512)");
    n = in.size(1);
    in_rs = in.stride(0);
    out_rs = out.stride(0);
  } else {
    TORCH_CHECK(in.is_contiguous() && out.is_contiguous() && out.numel() == n, "xgmi_relay: contiguous, equal sizes");
  }
  std::vector<void*> d(world), s(world);
  std::vector<int> p(world);
  for (int r = 0; r < world; ++r) {
    d[r] = vp(stage_ptrs[r]);
    s[r] = vp(sig_ptrs[r]);
    p[r] = (int)partners[r];
  }
  check(smdt_xgmi_relay(dcode(in), in.data_ptr(), out.data_ptr(), in_rs, out_rs, n, d.data(), s.data(), p.data(), world,
                        (int)rank, (int)nranks_local, slot_bytes, (int)sub, (uint32_t)epoch, dev_epoch ? 1 : 0,
                        cur_stream()),
        "xgmi_relay");
}

void relay_reset(int64_t sig) { check(smdt_relay_reset(vp(sig), cur_stream()), "relay_reset"); }

// Device epochs (xgmi_relay.hip): advance the local ranks' call counters by n on the current stream.
void relay_epoch_bump(std::vector<int64_t> sig_ptrs, int64_t rank, int64_t nranks_local, int64_t n) {
  std::vector<void*> s(sig_ptrs.size());
  for (size_t r = 0; r < sig_ptrs.size(); ++r) s[r] = vp(sig_ptrs[r]);
  TORCH_CHECK(n >= 1 && n <= 0xffffll, "relay_epoch_bump: n out of range");
  check(smdt_relay_epoch_bump(s.data(), (int)s.size(), (int)rank, (int)nranks_local, (uint32_t)n, cur_stream()),
        "relay_epoch_bump");
}

}  // namespace

void register_blaslt(pybind11::module_& m);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "smdt_amd gfx950 (MI355X) HIP kernel library";
  register_blaslt(m);
  using pybind11::arg;
  m.def("layernorm_fwd", &layernorm_fwd, arg("x"), arg("res"), arg("bias"), arg("gamma"), arg("beta"),
        arg("eps"), arg("p_drop"), arg("seed"), arg("offset"), arg("rms"), arg("want_s"),
        arg("out_y") = pybind11::none(), arg("x2") = pybind11::none());
  m.def("layernorm_bwd", &layernorm_bwd, arg("dy"), arg("ds_in"), arg("s"), arg("gamma"), arg("mean"),
        arg("rstd"), arg("p_drop"), arg("seed"), arg("offset"), arg("rms"), arg("want_dx"), arg("want_dbias"),
        arg("dgamma_acc") = pybind11::none(), arg("dbeta_acc") = pybind11::none(),
        arg("dbias_acc") = pybind11::none(), arg("out_dx") = pybind11::none(), arg("dy2") = pybind11::none());
  m.def("bias_act_fwd", &bias_act_fwd);
  m.def("bias_act_bwd", &bias_act_bwd, arg("dy"), arg("x"), arg("bias"), arg("act"), arg("want_dbias"),
        arg("dbias_acc") = pybind11::none());
  m.def("swiglu_fwd", &swiglu_fwd);
  m.def("swiglu_bwd", &swiglu_bwd);
  m.def("softmax_fwd", &softmax_fwd);
  m.def("softmax_bwd", &softmax_bwd);
  m.def("adam", &adam);
  m.def("sumsq", &sumsq);
  m.def("clip_coef", &clip_coef);
  m.def("scale_", &scale_);
  m.def("cast_", &cast_);
  m.def("rope_", &rope_);
  m.def("transpose2d", &transpose2d);
  m.def("fp8_quantize", &fp8_quantize);
  m.def("fp8_update_scales", &fp8_update_scales);
  m.def("mx_quantize", &mx_quantize, arg("x"), arg("fmt"), arg("rows") = true, arg("cols") = false);
  m.def("gemm_mx", &gemm_mx, arg("a"), arg("sa"), arg("b"), arg("sb"), arg("bias") = pybind11::none(),
        arg("out_dtype") = 1, arg("max_blocks") = 0);
  m.def("gemm_mx_supported", &gemm_mx_supported);
  m.def("paced_copy", &paced_copy);
  m.def("gather_rows", &gather_rows);
  m.def("aug_depthwise", &aug_depthwise);
  m.def("aug_median3", &aug_median3);
  m.def("bias_grad", &bias_grad);
  m.def("gemm_tn_supported", &gemm_tn_supported, arg("a"), arg("b"));
  m.def("gemm_tn", &gemm_tn, arg("a"), arg("b"), arg("epi") = 0, arg("bias") = pybind11::none(),
        arg("out") = pybind11::none(), arg("out2") = pybind11::none(), arg("max_blocks") = 0,
        arg("var") = 0, arg("aux") = pybind11::none());
  m.def("wgrad_mfma", &wgrad_mfma, arg("main_grad"), arg("dy"), arg("x"), arg("max_splits") = 0);
  m.def("wgrad_grouped", &wgrad_grouped, arg("main_grads"), arg("dys"), arg("xs"),
        arg("biases") = std::vector<Tensor>{}, arg("overwrite") = std::vector<bool>{}, arg("cus") = 0,
        arg("mranges") = std::vector<Tensor>{}, arg("experts") = std::vector<int64_t>{});
  m.def("moe_rows", [](int64_t T, int64_t E) { return smdt_moe_rows(T, E); });
  m.def("gemm_tn_shape_supported", [](int64_t M, int64_t N, int64_t K) { return smdt_gemm_tn_supported(M, N, K) != 0; });
  m.def("moe_route", &moe_route);
  m.def("moe_route_into", &moe_route_into);
  m.def("ptr_table", &ptr_table);
  m.def("gemm_tn_grouped", &gemm_tn_grouped, arg("a"), arg("btab"), arg("n"), arg("tile_expert"), arg("epi") = 0,
        arg("biastab") = pybind11::none(), arg("aux") = pybind11::none(), arg("sums") = false,
        arg("max_blocks") = 0);
  m.def("wgrad_fp8_grouped", &wgrad_fp8_grouped, arg("main_grads"), arg("dys"), arg("xs"), arg("inv_dys"),
        arg("inv_xs"), arg("overwrite") = std::vector<bool>{}, arg("cus") = 0);
  m.def("wgrad_fp8_supported", &wgrad_fp8_supported);
  m.def("decode_attn_chunk", &decode_attn_chunk);
  m.def("decode_attn_supported", &decode_attn_supported, arg("dtype"), arg("D"), arg("nh"), arg("nkv"));
  m.def("decode_attn", &decode_attn, arg("q"), arg("k_cache"), arg("v_cache"), arg("lens"), arg("scale"),
        arg("max_len") = 0);
  m.def("decode_rope_append", &decode_rope_append, arg("qkv"), arg("k_cache"), arg("v_cache"), arg("pos"), arg("nh"),
        arg("cos") = pybind11::none(), arg("sin") = pybind11::none(), arg("rot") = 0);
  m.def("decode_attn_multi_max_t", &decode_attn_multi_max_t);
  m.def("decode_attn_multi_supported", &decode_attn_multi_supported, arg("dtype"), arg("D"), arg("nh"), arg("nkv"),
        arg("T"));
  m.def("decode_attn_multi", &decode_attn_multi, arg("q"), arg("k_cache"), arg("v_cache"), arg("lens"), arg("scale"),
        arg("max_len") = 0);
  m.def("decode_attn_mx", &decode_attn_mx, arg("q"), arg("kq"), arg("ks"), arg("vq"), arg("vs"), arg("lens"),
        arg("scale"), arg("max_len") = 0);
  m.def("decode_rope_append_mx", &decode_rope_append_mx, arg("qkv"), arg("kq"), arg("ks"), arg("vq"), arg("vs"),
        arg("pos"), arg("nh"), arg("cos") = pybind11::none(), arg("sin") = pybind11::none(), arg("rot") = 0);
  m.def("decode_linear_supported", &decode_linear_supported, arg("dtype"), arg("fmt"), arg("M"), arg("N"), arg("K"));
  m.def("decode_linear_constants", &decode_linear_constants);
  m.def("decode_linear_plan", &decode_linear_plan, arg("fmt"), arg("N"), arg("K"));
  m.def("decode_linear", &decode_linear, arg("x"), arg("w"), arg("scales") = pybind11::none(),
        arg("bias") = pybind11::none(), arg("fmt") = 0, arg("workspace") = pybind11::none(),
        arg("out") = pybind11::none());
  m.def("window_attn_fwd", &window_attn_fwd, arg("qkv"), arg("table"), arg("window"), arg("shift"), arg("heads"));
  m.def("window_attn_bwd", &window_attn_bwd, arg("qkv"), arg("table"), arg("lse"), arg("dout"), arg("window"),
        arg("shift"), arg("heads"));
  m.def("ce_stats", &ce_stats);
  m.def("set_rng_step", &set_rng_step);
  m.def("adam_capturable", &adam_capturable);
  m.def("ce_fused_local", &ce_fused_local);
  m.def("ce_bwd", &ce_bwd);
  m.def("ce_fused", &ce_fused);
  namespace py = pybind11;
  m.def("flash_fwd", &flash_fwd, py::arg("q"), py::arg("k"), py::arg("v"), py::arg("scale"), py::arg("causal"),
        py::arg("out") = py::none(), py::arg("dropout_p") = 0.0, py::arg("seed") = 0, py::arg("offset") = 0,
        py::arg("doc_start") = py::none());
  m.def("ipc_malloc", &ipc_malloc, py::arg("bytes"), py::arg("uncached"));
  m.def("ipc_free", &ipc_free);
  m.def("ipc_get_handle", &ipc_get_handle);
  m.def("ipc_open", &ipc_open);
  m.def("ipc_close", &ipc_close);
  m.def("ar_read_error", &ar_read_error);
  m.def("signal_word", &signal_word, py::arg("sig"), py::arg("byte_offset"));
  m.def("ar_word_offset", &smdt_ar_word_offset);
  m.def("relay_word_offset", &smdt_relay_word_offset);
  m.def("ar_signal_bytes", &smdt_ar_signal_bytes);
  m.def("ar_max_blocks", &smdt_ar_max_blocks);
  m.def("xgmi_allreduce", &xgmi_allreduce, py::arg("input"), py::arg("out"), py::arg("data_ptrs"), py::arg("sig_ptrs"),
        py::arg("rank"), py::arg("nranks_local"), py::arg("region_bytes"), py::arg("two_shot"), py::arg("blocks"),
        py::arg("scale") = 1.0);
  m.def("xgmi_collective", &xgmi_collective, py::arg("mode"), py::arg("input"), py::arg("out"), py::arg("data_ptrs"),
        py::arg("sig_ptrs"), py::arg("rank"), py::arg("nranks_local"), py::arg("region_bytes"), py::arg("blocks"),
        py::arg("n"), py::arg("slice_stride"), py::arg("scale") = 1.0);
  m.def("xgmi_relay", &xgmi_relay, py::arg("input"), py::arg("out"), py::arg("stage_ptrs"), py::arg("sig_ptrs"),
        py::arg("partners"), py::arg("rank"), py::arg("nranks_local"), py::arg("slot_bytes"), py::arg("sub"),
        py::arg("epoch"), py::arg("dev_epoch") = false);
  m.def("relay_reset", &relay_reset, py::arg("sig"));
  m.def("relay_epoch_bump", &relay_epoch_bump, py::arg("sig_ptrs"), py::arg("rank"), py::arg("nranks_local"),
        py::arg("n"));
  m.def("relay_signal_bytes", &smdt_relay_signal_bytes);
  m.def("relay_read_error", &relay_read_error);
  m.def("flash_bwd", &flash_bwd, py::arg("q"), py::arg("k"), py::arg("v"), py::arg("o"), py::arg("dout"),
        py::arg("lse"), py::arg("scale"), py::arg("causal"), py::arg("dq") = py::none(), py::arg("dk") = py::none(),
        py::arg("dv") = py::none(), py::arg("dropout_p") = 0.0, py::arg("seed") = 0, py::arg("offset") = 0,
        py::arg("doc_start") = py::none(), py::arg("doc_end") = py::none());
  m.def("flash_bwd_dbias", &flash_bwd_dbias, py::arg("q"), py::arg("k"), py::arg("v"), py::arg("o"), py::arg("dout"),
        py::arg("lse"), py::arg("scale"), py::arg("causal"), py::arg("dbias"), py::arg("accumulate"),
        py::arg("dq") = py::none(), py::arg("dk") = py::none(), py::arg("dv") = py::none(),
        py::arg("dropout_p") = 0.0, py::arg("seed") = 0, py::arg("offset") = 0,
        py::arg("doc_start") = py::none(), py::arg("doc_end") = py::none());
  m.def("gemm_tn_dgelu_dbias", &gemm_tn_dgelu_dbias, py::arg("a"), py::arg("b"), py::arg("bias"), py::arg("aux"),
        py::arg("dbias"), py::arg("accumulate"), py::arg("out") = py::none(), py::arg("max_blocks") = 0);
}
