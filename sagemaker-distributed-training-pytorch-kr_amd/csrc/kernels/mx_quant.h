// Device helpers of the OCP MX block format shared by the kernels that write it (mx_quant.hip,
// decode_attn_mx.hip): the block exponent, the saturating FP8 conversion and the E8M0 scale. The
// rule itself is stated at the top of mx_quant.hip; ops/functional.py's mx_quantize_ref is its twin.
#pragma once
#include "common.h"

namespace smdt {
namespace mxq {

template <bool BF8> constexpr float fp8_max() { return BF8 ? 57344.f : 448.f; }
template <bool BF8> constexpr int fp8_emax() { return BF8 ? 15 : 8; }

// Four floats -> four FP8 bytes (element 0 in the low byte), NaN as 0x7f | sign.
template <bool BF8>
__device__ __forceinline__ unsigned cvt4(float a, float b, float c, float d) {
  int w = 0;
  if constexpr (BF8) {
    w = __builtin_amdgcn_cvt_pk_bf8_f32(a, b, w, false);
    w = __builtin_amdgcn_cvt_pk_bf8_f32(c, d, w, true);
  } else {
    w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, w, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
  }
  unsigned u = (unsigned)w;
  const float v[4] = {a, b, c, d};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (v[i] != v[i]) {
      const unsigned nan = 0x7Fu | ((__float_as_uint(v[i]) >> 24) & 0x80u);
      u = (u & ~(0xFFu << (8 * i))) | (nan << (8 * i));
    }
  }
  return u;
}

template <typename T>
__device__ __forceinline__ float raw_to_f32(unsigned short bits) {
  T t;
  __builtin_memcpy(&t, &bits, 2);
  return to_f32(t);
}

// |f| as a bit pattern when finite, else 0: non-negative floats order as unsigned integers.
__device__ __forceinline__ unsigned finite_abs_bits(float f) {
  const unsigned ab = __float_as_uint(f) & 0x7FFFFFFFu;
  return ab < 0x7F800000u ? ab : 0u;
}

// The block exponent e of a block whose finite amax has the bit pattern `am`.
template <bool BF8>
__device__ __forceinline__ int block_exp(unsigned am) {
  if (am == 0u) return 0;
  const int e = (int)(am >> 23) - 127 - fp8_emax<BF8>();
  return e < -127 ? -127 : (e > 127 ? 127 : e);
}

__device__ __forceinline__ float pow2_neg(int e) { return __uint_as_float((unsigned)(127 - e) << 23); }

// 16 floats * mult, saturated -> 16 FP8 bytes
template <bool BF8>
__device__ __forceinline__ u32x4 quant16(const float (&f)[16], float mult) {
  constexpr float kMax = fp8_max<BF8>();
  float v[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    float s = f[j] * mult;
    s = s > kMax ? kMax : s;      // compares are false for NaN: it passes through
    s = s < -kMax ? -kMax : s;
    v[j] = s;
  }
  u32x4 o;
#pragma unroll
  for (int k = 0; k < 4; ++k) o[k] = cvt4<BF8>(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
  return o;
}

// 2^(s - 127) for an E8M0 byte s (0: the fp32 subnormal 2^-127; 255, the E8M0 NaN: NaN).
__device__ __forceinline__ float e8m0_to_f32(unsigned s) {
  return __uint_as_float(s == 0u ? 0x00400000u : (s == 255u ? 0x7FC00000u : s << 23));
}

}  // namespace mxq
}  // namespace smdt
