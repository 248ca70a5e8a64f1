// Incremental decoding against an MXFP8 K/V cache for gfx950 (generate(kv_cache_format="mxfp8")).
//
// A cache tensor is q [B, cap, nkv, D] of E4M3 bytes and s [B, cap, nkv, D / 32] of E8M0 scale
// bytes (bias 127): every (sequence, position, kv head) row of D elements is D / 32 MX blocks, the
// bytes mx_quant.hip's row form writes for the 16-bit row (ops/functional.py's mx_quantize_ref is
// the definition). A value is q * 2^(s - 127). The cache is 51.6 % of the 16-bit one, and reading
// it is what a long-context decode step costs. Two entry points, the MX forms of the 16-bit ones:
//
//   smdt_decode_attn_mx         split-KV attention of q [B, nh, D] (bf16 / fp16) against the cache
//   smdt_decode_rope_append_mx  RoPE on the new token's q / k, then the quantising store of its
//                               k / v into row pos[b]
//
// Attention is decode_common.h's decode_attn_partial_kernel, with its guarantees, reading the cache
// through DecKvMx below; decode_attn.hip's combine kernel finishes (smdt_decode_attn_combine).
// There is no LDS staging of the cache.
//
// A lane's 16-byte load is 16 elements, half of one MX block, so one scale belongs to everything
// the lane holds and never enters the inner products: D / 16 lanes cover a key row, the lane sums
// q . k over its 16 raw FP8 values (v_cvt_pk_f32_fp8 to fp32, exact), multiplies the sum by
// 2^(sk - 127) once and only then joins the row butterfly. For V the lane folds 2^(sv - 127) into
// the key's probability once per query head and accumulates p' * v_fp8. Both are the twin's
// arithmetic up to the place of one exact power-of-two factor (exact unless a product leaves the
// fp32 normal range, where the twin's dequantised value does too).
//
// Scale bytes 0 and 255 in a VALID row mean what they mean in the twin (_e8m0_to_f32): 0 is
// 2^-127, an fp32 subnormal, which mx_quantize_ref emits only for blocks whose amax is below
// 2^-119 (such a block's values are below 2^-118 and contribute what the twin's do); 255 is the
// E8M0 NaN, which mx_quantize_ref never emits, and makes that row's score / value NaN exactly as
// the twin's dequantisation does. Neither is special-cased beyond the conversion.
//
// The append kernel is the 16-bit one with the store replaced: q goes out in 16 bits with the same
// bytes, k (rotated) and v are first rounded to the model dtype into LDS (dec_rope_token with an
// LDS destination), exactly the values the 16-bit cache would hold, then one thread per 32-block
// quantises by mx_quant.hip's rule (shared helpers, mx_quant.h) and writes 32 element bytes and
// the scale byte of row pos[b] with plain vector stores.
#include "decode_common.h"
#include "launchers.h"
#include "mx_quant.h"

namespace smdt {

// 16 E4M3 bytes (element 0 in the low byte of word 0) -> 16 floats, exact.
__device__ __forceinline__ void fp8x16_to_f32(const u32x4& w, float (&f)[16]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
    const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
    f[4 * i] = lo[0];
    f[4 * i + 1] = lo[1];
    f[4 * i + 2] = hi[0];
    f[4 * i + 3] = hi[1];
  }
}

// One MXFP8 cache tensor as decode_attn_partial_kernel reads it (DecKv16's interface): a lane's 16
// raw FP8 values, two lanes to an MX block, and the block's 2^(s - 127).
struct DecKvMx {
  static constexpr int kEPL = 16;
  static constexpr bool kScaled = true;
  const uint8_t* __restrict__ q;
  const uint8_t* __restrict__ s;
  using Raw = u32x4;
  __device__ __forceinline__ Raw load(int64_t e) const { return __builtin_nontemporal_load(reinterpret_cast<const Raw*>(q + e)); }
  static __device__ __forceinline__ void to_f32(const Raw& r, float (&f)[kEPL]) { fp8x16_to_f32(r, f); }
  __device__ __forceinline__ float scale(int64_t i) const { return mxq::e8m0_to_f32(s[i]); }
};

// One workgroup per new token. Dynamic LDS: the token's k row [nkv, D] then its v row, as the
// model dtype's bits (2 * nkv * D * 2 bytes).
template <typename T>
__global__ __launch_bounds__(256) void decode_rope_append_mx_kernel(
    const T* __restrict__ qkv, T* __restrict__ q_out, uint8_t* __restrict__ kq, uint8_t* __restrict__ ksc,
    uint8_t* __restrict__ vq, uint8_t* __restrict__ vsc, const int* __restrict__ pos_t, int nh, int nkv, int D,
    int cap, int rot, const float* __restrict__ cos_t, const float* __restrict__ sin_t, int max_pos, float sign) {
  extern __shared__ __attribute__((aligned(16))) unsigned short stage[];
  const int b = blockIdx.x;
  const int pos = pos_t[b];
  if (!dec_pos_ok(pos, cap, rot, max_pos)) return;      // the whole workgroup leaves, before the barrier
  T* kd = reinterpret_cast<T*>(stage);      // rounded to the model dtype: what a 16-bit cache holds
  dec_rope_token(qkv + (int64_t)b * (nh + 2 * nkv) * D, q_out + (int64_t)b * nh * D, kd, kd + nkv * D, pos, nh, nkv,
                 D, rot, cos_t, sin_t, sign);
  __syncthreads();
  // one thread per MX block: the staged k row's nkv D / 32 blocks, then the v row's
  const int nb = nkv * D / 32;
  const int64_t row = (int64_t)b * cap + pos;
  for (int i = threadIdx.x; i < 2 * nb; i += 256) {
    const bool isv = i >= nb;
    const int j = isv ? i - nb : i;
    const u16x8* p = reinterpret_cast<const u16x8*>(stage + i * 32);
    float f[2][16];
    unsigned am = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const u16x8 lo = p[2 * h], hi = p[2 * h + 1];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        f[h][e] = mxq::raw_to_f32<T>(e < 8 ? lo[e] : hi[e - 8]);
        const unsigned ab = mxq::finite_abs_bits(f[h][e]);
        am = ab > am ? ab : am;
      }
    }
    const int e = mxq::block_exp<false>(am);
    const float mult = mxq::pow2_neg(e);
    u32x4* o = reinterpret_cast<u32x4*>((isv ? vq : kq) + (row * nb + j) * 32);
    o[0] = mxq::quant16<false>(f[0], mult);
    o[1] = mxq::quant16<false>(f[1], mult);
    (isv ? vsc : ksc)[row * nb + j] = (uint8_t)(e + 127);
  }
}

}  // namespace smdt

using namespace smdt;

extern "C" hipError_t smdt_decode_attn_mx(int dtype, const void* q, const void* kq, const void* ksc, const void* vq,
                                          const void* vsc, const int* lens, float* ws_ml, float* ws_acc, void* out,
                                          int B, int nh, int nkv, int D, int cap, int max_len, float scale,
                                          hipStream_t st) {
  const int nchunks = dec_nchunks(B, nkv, cap, max_len);
  if (!smdt_decode_attn_supported(dtype, D, nh, nkv) || nchunks == 0) return hipErrorInvalidValue;
  const DecKvMx kc{(const uint8_t*)kq, (const uint8_t*)ksc}, vc{(const uint8_t*)vq, (const uint8_t*)vsc};
  const hipError_t e = dec_dispatch(dtype, D, [&](auto tag, auto d) {
    using T = typename decltype(tag)::type;
    return decode_attn_partial_launch<T, decltype(d)::value>(q, kc, vc, lens, ws_ml, ws_acc, B, nh, nkv, cap, nchunks,
                                                             scale, st);
  });
  if (e != hipSuccess) return e;
  return smdt_decode_attn_combine(dtype, ws_ml, ws_acc, lens, out, B, nh, D, cap, nchunks, st);
}

extern "C" hipError_t smdt_decode_rope_append_mx(int dtype, const void* qkv, void* q_out, void* kq, void* ksc,
                                                 void* vq, void* vsc, const int* pos, int B, int nh, int nkv, int D,
                                                 int cap, int rot, const float* cos_t, const float* sin_t,
                                                 int max_pos, hipStream_t st) {
  if (B <= 0 || nh <= 0 || nkv <= 0 || D <= 0 || D % 32 || rot % 16 || rot < 0 || rot > D || cap <= 0 ||
      (int64_t)nkv * D > 8192 || (rot > 0 && (cos_t == nullptr || sin_t == nullptr || max_pos <= 0)))
    return hipErrorInvalidValue;
  const unsigned lds = 2u * (unsigned)(nkv * D) * 2u;      // the staged k and v rows: at most 32 KiB
  return dec_dispatch(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(decode_rope_append_mx_kernel<T>, dim3((unsigned)B), dim3(256), lds, st, (const T*)qkv,
                       (T*)q_out, (uint8_t*)kq, (uint8_t*)ksc, (uint8_t*)vq, (uint8_t*)vsc, pos, nh, nkv, D, cap, rot,
                       cos_t, sin_t, max_pos, 1.f);
    return hipGetLastError();
  });
}
