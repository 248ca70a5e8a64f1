// The device-side rule of per-tensor (delayed-scaling) FP8 quantisation, shared by the stand-alone
// quantise kernels (fp8_quant.hip) and by the producers that write their output already quantised
// (layernorm.hip, bias_act.hip), so that a fused producer and the chain "store 16 bits, quantise"
// give the same bytes and the same amax.
//
//   q    = fp8( clamp(x * scale, -max, max) )     round-to-nearest-even (v_cvt_pk_*_f32)
//   amax = max(amax, max |x|)                      before scaling, merged by a vector atomic max
//
// x is a value of the 16-bit model dtype widened to fp32: a producer rounds to that dtype first
// (round16x8). The clamp is written with compares, which keep a NaN (fminf / fmaxf would drop it),
// so a NaN comes out as an FP8 NaN and +-inf saturates. A NaN is stored as 0x7f | sign in both
// formats, the byte PyTorch's own cast produces. |x| is merged as its bit pattern: non-negative
// floats order as unsigned integers, inf sorts above every finite value and NaN above inf, so a
// non-finite input always leaves a non-finite amax.
#pragma once
#include "common.h"

namespace smdt {

using u32x2 = __attribute__((ext_vector_type(2))) unsigned;

template <bool BF8> constexpr float fp8_max() { return BF8 ? 57344.f : 448.f; }

// Four floats -> four FP8 bytes (element 0 in the low byte).
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
    if (v[i] != v[i]) {   // canonical NaN byte, sign kept
      const unsigned nan = 0x7Fu | ((__float_as_uint(v[i]) >> 24) & 0x80u);
      u = (u & ~(0xFFu << (8 * i))) | (nan << (8 * i));
    }
  }
  return u;
}

// Eight values rounded to the 16-bit type T, as a store of T followed by a load would leave them;
// returns the eight 16-bit patterns (what that store writes). One vector conversion: a scalar
// cast next to the multiply that made the value may be merged with it into a mixed-precision
// instruction that rounds once, and the bytes must be those of "round to fp32, then to T".
template <typename T>
__device__ __forceinline__ u16x8 round16x8(float (&x)[8]) {
  using f32x8 = __attribute__((ext_vector_type(8))) float;
  using tx8 = __attribute__((ext_vector_type(8))) T;
  f32x8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = x[j];
  const tx8 h = __builtin_convertvector(v, tx8);
  const f32x8 w = __builtin_convertvector(h, f32x8);
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = w[j];
  return __builtin_bit_cast(u16x8, h);
}

// N (a multiple of 4) values -> N FP8 bytes in N / 4 words; returns max |x| as a bit pattern.
template <bool BF8, int N>
__device__ __forceinline__ unsigned quant_f32(const float (&x)[N], float scale, unsigned (&out)[N / 4]) {
  static_assert(N % 4 == 0, "four bytes per word");
  constexpr float kMax = fp8_max<BF8>();
  float v[N];
  unsigned am = 0;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const unsigned ab = __float_as_uint(x[j]) & 0x7FFFFFFFu;
    am = ab > am ? ab : am;
    float s = x[j] * scale;
    s = s > kMax ? kMax : s;      // compares are false for NaN: it passes through
    s = s < -kMax ? -kMax : s;
    v[j] = s;
  }
#pragma unroll
  for (int k = 0; k < N / 4; ++k) out[k] = cvt4<BF8>(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
  return am;
}

__device__ __forceinline__ unsigned wave_umax(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned w = (unsigned)__shfl_xor((int)v, o, kWave);
    v = w > v ? w : v;
  }
  return v;
}

// Max of the bit patterns over a block of 256 threads (every thread calls), merged into *amax by
// one atomic per block. red: four words of LDS.
__device__ __forceinline__ void merge_amax(unsigned am, unsigned* red, float* __restrict__ amax) {
  am = wave_umax(am);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) red[wid] = am;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned m = red[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) m = red[w] > m ? red[w] : m;
    if (m != 0) atomicMax(reinterpret_cast<unsigned*>(amax), m);
  }
}

// 16 FP8 bytes that a pair of neighbouring lanes holds as 8 + 8 (the even lane the lower
// addresses) for each of two places A and B: after the swap the even lane owns all 16 bytes of
// A and the odd lane all 16 of B, so each lane issues one 16-byte store instead of two 8-byte
// ones. Every lane of the wave must call.
__device__ __forceinline__ u32x4 pair_bytes16(const unsigned (&a)[2], const unsigned (&b)[2], bool odd) {
  const unsigned s0 = odd ? a[0] : b[0], s1 = odd ? a[1] : b[1];
  const unsigned r0 = (unsigned)__shfl_xor((int)s0, 1, kWave), r1 = (unsigned)__shfl_xor((int)s1, 1, kWave);
  u32x4 o;
  if (odd) { o[0] = r0; o[1] = r1; o[2] = b[0]; o[3] = b[1]; }
  else     { o[0] = a[0]; o[1] = a[1]; o[2] = r0; o[3] = r1; }
  return o;
}

}  // namespace smdt
