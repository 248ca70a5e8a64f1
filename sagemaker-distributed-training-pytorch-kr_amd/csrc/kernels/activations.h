// GeLU (tanh form) and its derivative, shared by the elementwise bias-activation kernels
// (bias_act.hip) and the GEMM epilogues (gemm_tn.hip).
#pragma once
#include "common.h"

namespace smdt {

using f32x2 = __attribute__((ext_vector_type(2))) float;

// Element-wise 2^v and 1 / v on one float or a pair. Arithmetic on a pair compiles to gfx950's
// packed fp32 VALU (v_pk_mul_f32 / v_pk_fma_f32 / v_pk_add_f32: two elements per issue slot);
// v_exp_f32 and v_rcp_f32 have no packed form.
__device__ __forceinline__ float act_exp2(float v) { return __builtin_amdgcn_exp2f(v); }
__device__ __forceinline__ float act_rcp(float v) { return __builtin_amdgcn_rcpf(v); }
__device__ __forceinline__ f32x2 act_exp2(f32x2 v) {
  return f32x2{__builtin_amdgcn_exp2f(v[0]), __builtin_amdgcn_exp2f(v[1])};
}
__device__ __forceinline__ f32x2 act_rcp(f32x2 v) {
  return f32x2{__builtin_amdgcn_rcpf(v[0]), __builtin_amdgcn_rcpf(v[1])};
}

// Sigmoid form of the tanh GeLU. With u = k0 (x + k1 x^3), 0.5 (1 + tanh(u)) = sigmoid(2 u), so
//     s        = 1 / (1 + 2^(-2 u log2 e)) = 1 / (1 + 2^(x (c0 + c1 x^2)))
//     gelu(x)  = x s
//     gelu'(x) = s + x s (1 - s) (d0 + d1 x^2)            (d0 + d1 x^2 = 2 u'(x))
// One v_exp_f32 + one v_rcp_f32 per element as the former 1 - 2 / (1 + 2^(2 u log2 e)) tanh had,
// and 5 (forward) / 9 (derivative) full-rate ops instead of 10 / 15; no libm tanhf, whose
// ~20-instruction sequence made the bias-GeLU kernels VALU-bound at [16k, 4096]. Saturates
// without NaN for every finite x whose square is finite: 2^t -> inf gives s = 0, 2^t -> 0 gives
// s = 1, and 1 - s is formed as such (not as 2^t s, which would be inf * 0). Absolute error ~1e-7,
// far below bf16 resolution; the negative tail no longer cancels (1 + tanh(u) did).
constexpr double kGeluK0 = 0.7978845608028654;   // sqrt(2 / pi)
constexpr double kGeluK1 = 0.044715;
constexpr double kLog2e = 1.4426950408889634;
constexpr float kGeluC0 = (float)(-2.0 * kGeluK0 * kLog2e);
constexpr float kGeluC1 = (float)(-2.0 * kGeluK0 * kGeluK1 * kLog2e);
constexpr float kGeluD0 = (float)(2.0 * kGeluK0);
constexpr float kGeluD1 = (float)(6.0 * kGeluK0 * kGeluK1);

// V: float or f32x2; x2 = x * x (shared with the derivative's polynomial)
template <class V>
__device__ __forceinline__ V gelu_sigmoid(V x, V x2) {
  return act_rcp(1.f + act_exp2(x * (x2 * kGeluC1 + kGeluC0)));
}
template <class V>
__device__ __forceinline__ V gelu_tanh(V x) {
  return x * gelu_sigmoid(x, x * x);
}
template <class V>
__device__ __forceinline__ V gelu_tanh_grad(V x) {
  const V x2 = x * x;
  const V s = gelu_sigmoid(x, x2);
  const V w = (x * s) * (x2 * kGeluD1 + kGeluD0);
  return w * (1.f - s) + s;
}
}  // namespace smdt
