// Incremental decoding against an MXFP8 K/V cache for gfx950 (generate(kv_cache_format="mxfp8")).
//
// A cache tensor is q [B, cap, nkv, D] of E4M3 bytes and s [B, cap, nkv, D / 32] of E8M0 scale
// bytes (bias 127): every (sequence, position, kv head) row of D elements is D / 32 MX blocks, the
// bytes mx_quant.hip's row form writes for the 16-bit row (ops/functional.py's mx_quantize_ref is
// the definition). A value is q * 2^(s - 127). The cache is 51.6 % of the 16-bit one, and reading
// it is what a long-context decode step costs. Two entry points, the MX forms of decode_attn.hip's:
//
//   smdt_decode_attn_mx         split-KV attention of q [B, nh, D] (bf16 / fp16) against the cache
//   smdt_decode_rope_append_mx  RoPE on the new token's q / k, then the quantising store of its
//                               k / v into row pos[b]
//
// Attention keeps decode_attn.hip's structure and guarantees: one 256-thread workgroup per (key
// chunk of 256, kv head, sequence) serves all G = nh / nkv query heads; `lens` stays on the device;
// a key at or beyond lens[b] reads row lens[b] - 1 instead, element bytes AND scale byte, and is
// selected out, so nothing in the unused part of the cache (NaN bytes, scale 255) is ever loaded;
// fp32 partials, no atomics, the same fixed summation order every call; decode_attn.hip's combine
// kernel finishes (smdt_decode_attn_combine). There is no LDS staging of the cache.
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
// The append kernel is decode_rope_append_kernel with the store replaced: q goes out in 16 bits
// with the same bytes, k (rotated) and v are first rounded to the model dtype into LDS, exactly the
// values the 16-bit cache would hold, then one thread per 32-block quantises by mx_quant.hip's rule
// (shared helpers, mx_quant.h) and writes 32 element bytes and the scale byte of row pos[b] with
// plain vector stores. A position outside [0, cap) or the RoPE table writes nothing.
#include "common.h"
#include "launchers.h"
#include "mx_quant.h"

namespace smdt {

constexpr int kMxChunk = 256;     // keys per workgroup == threads per workgroup (decode_attn.hip's)
constexpr int kMxThreads = 256;
constexpr int kMxWaves = kMxThreads / kWave;

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

template <typename T, int D, int G>
__global__ __launch_bounds__(kMxThreads) void decode_attn_mx_partial_kernel(
    const T* __restrict__ q, const uint8_t* __restrict__ kq, const uint8_t* __restrict__ ksc,
    const uint8_t* __restrict__ vq, const uint8_t* __restrict__ vsc, const int* __restrict__ lens,
    float* __restrict__ ws_ml, float* __restrict__ ws_acc, int cap, int nkv, float scale) {
  constexpr int LPK = D / 16;                 // lanes per key row (two lanes to an MX block)
  constexpr int KPB = kMxThreads / LPK;       // keys per workgroup step
  constexpr int STEPS = kMxChunk / KPB;
  constexpr int SPR = D / 32;                 // scale bytes per key row
  const int chunk = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
  const int nchunks = gridDim.x, nh = nkv * G;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int lk = tid % LPK, ks = tid / LPK;
  int len = lens[b];
  len = len < 0 ? 0 : (len > cap ? cap : len);
  const int k0 = chunk * kMxChunk;
  const int64_t part0 = ((int64_t)b * nh + (int64_t)kvh * G) * nchunks + chunk;   // head g: + g * nchunks
  if (k0 >= len) {      // no key of this sequence in the chunk: a partial the combine skips
    if (tid < G) {
      ws_ml[(part0 + (int64_t)tid * nchunks) * 2] = -INFINITY;
      ws_ml[(part0 + (int64_t)tid * nchunks) * 2 + 1] = 0.f;
    }
    return;
  }
  __shared__ float sc[G][kMxChunk];                // scores, then probabilities
  __shared__ float red[2][G][kMxWaves];
  __shared__ float racc[kMxWaves][G][D];

  const int64_t row0 = (int64_t)b * cap * nkv + kvh;          // row of key 0; key k: + k * nkv
  const int64_t ebase = row0 * D + lk * 16;                   // element bytes of this lane
  const int64_t sbase = row0 * SPR + lk / 2;                  // its block's scale byte
  const int64_t erow = (int64_t)nkv * D, srow = (int64_t)nkv * SPR;

  // ---- pass 1: scores
  {
    float qf[G][16];
#pragma unroll
    for (int g = 0; g < G; ++g) load_vec<T, 16>(q + ((int64_t)b * nh + kvh * G + g) * D + lk * 16, qf[g]);
#pragma unroll 4
    for (int it = 0; it < STEPS; ++it) {
      const int kl = it * KPB + ks;
      const int key = k0 + kl;
      // a key at or beyond len reads row len - 1 instead (a valid row, bytes and scale: the loads
      // stay unconditional and all in flight together) and is selected out
      const int kr = key < len ? key : len - 1;
      const u32x4 kw = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(kq + ebase + (int64_t)kr * erow));
      const float kscale = mxq::e8m0_to_f32(ksc[sbase + (int64_t)kr * srow]);
      float kf[16];
      fp8x16_to_f32(kw, kf);
      float s[G];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        s[g] = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) s[g] += qf[g][j] * kf[j];
        s[g] *= kscale;                           // the block's 2^(sk - 127), once per lane
      }
#pragma unroll
      for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int o = LPK / 2; o > 0; o >>= 1) s[g] += __shfl_xor(s[g], o, kWave);
      }
#pragma unroll
      for (int g = 0; g < G; ++g)                 // every lane of the row holds all G sums
        if (lk == g % LPK) sc[g][kl] = key < len ? s[g] * scale : -INFINITY;
    }
  }
  __syncthreads();

  // ---- chunk maximum, probabilities and their sum (thread t owns key t of the chunk)
  float sv[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    sv[g] = sc[g][tid];
    const float wm = wave_max(sv[g]);
    if (lane == 0) red[0][g][wid] = wm;
  }
  __syncthreads();
  float m[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    m[g] = red[0][g][0];
#pragma unroll
    for (int w = 1; w < kMxWaves; ++w) m[g] = fmaxf(m[g], red[0][g][w]);
    // key k0 is valid, so m is finite unless a valid score is itself -inf
    const float p = sv[g] == -INFINITY ? 0.f : __expf(sv[g] - m[g]);
    sc[g][tid] = p;
    const float wsum = wave_sum(p);
    if (lane == 0) red[1][g][wid] = wsum;
  }
  __syncthreads();

  // ---- pass 2: acc[g] += (p[g][key] * 2^(sv - 127)) * v_fp8[key]
  float acc[G][16];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[g][j] = 0.f;
#pragma unroll 4
  for (int it = 0; it < STEPS; ++it) {
    const int kl = it * KPB + ks;
    const int key = k0 + kl;
    const int kr = key < len ? key : len - 1;       // as in pass 1; such a key's p is 0
    const u32x4 vw = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(vq + ebase + (int64_t)kr * erow));
    const float vscale = mxq::e8m0_to_f32(vsc[sbase + (int64_t)kr * srow]);
    float vf[16];
    fp8x16_to_f32(vw, vf);
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const float p = sc[g][kl] * vscale;
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[g][j] += p * vf[j];
    }
  }
  // the key slots of a wave (lanes with equal lk), in a fixed order
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int j = 0; j < 16; ++j) {
#pragma unroll
      for (int o = LPK; o < kWave; o <<= 1) acc[g][j] += __shfl_xor(acc[g][j], o, kWave);
    }
  if (lane < LPK) {
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int j = 0; j < 16; ++j) racc[wid][g][lk * 16 + j] = acc[g][j];
  }
  __syncthreads();
  for (int i = tid; i < G * D; i += kMxThreads) {
    const int g = i / D, d = i - g * D;
    float a = racc[0][g][d];
#pragma unroll
    for (int w = 1; w < kMxWaves; ++w) a += racc[w][g][d];
    ws_acc[(part0 + (int64_t)g * nchunks) * D + d] = a;
  }
  if (tid < G) {
    float mx = red[0][tid][0], l = red[1][tid][0];
#pragma unroll
    for (int w = 1; w < kMxWaves; ++w) {
      mx = fmaxf(mx, red[0][tid][w]);
      l += red[1][tid][w];
    }
    ws_ml[(part0 + (int64_t)tid * nchunks) * 2] = mx;
    ws_ml[(part0 + (int64_t)tid * nchunks) * 2 + 1] = l;
  }
}

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
  if (pos < 0 || pos >= cap || (rot > 0 && pos >= max_pos)) return;      // the whole workgroup leaves
  const int half = rot / 2;
  const int groups = half / 8;              // rotated 8-pair groups per head
  const int tail = (D - rot) / 8;           // unrotated 16-byte pieces per head
  const int W = (nh + 2 * nkv) * D;
  const T* src = qkv + (int64_t)b * W;
  T* qd = q_out + (int64_t)b * nh * D;
  T* kd = reinterpret_cast<T*>(stage);
  T* vd = kd + nkv * D;
  const float* ct = cos_t + (int64_t)pos * half;
  const float* stb = sin_t + (int64_t)pos * half;
  for (int i = threadIdx.x; i < (nh + nkv) * groups; i += 256) {
    const int h = i / groups, gidx = i - h * groups;
    const T* base = src + (int64_t)h * D + gidx * 8;
    T* dst = (h < nh ? qd + (int64_t)h * D : kd + (h - nh) * D) + gidx * 8;
    float a[8], bb[8], c[8], s[8];
    load_vec<T, 8>(base, a);
    load_vec<T, 8>(base + half, bb);
    load_vec<float, 8>(ct + gidx * 8, c);
    load_vec<float, 8>(stb + gidx * 8, s);
    float oa[8], ob[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float sn = sign * s[j];
      oa[j] = a[j] * c[j] - bb[j] * sn;
      ob[j] = bb[j] * c[j] + a[j] * sn;
    }
    store_vec<T, 8>(dst, oa);               // rounded to the model dtype: what a 16-bit cache holds
    store_vec<T, 8>(dst + half, ob);
  }
  // the unrotated tail of the q / k heads, and v: 16-byte copies
  for (int i = threadIdx.x; i < (nh + nkv) * tail; i += 256) {
    const int h = i / tail, o = rot + (i - h * tail) * 8;
    T* dst = (h < nh ? qd + (int64_t)h * D : kd + (h - nh) * D) + o;
    *reinterpret_cast<u16x8*>(dst) = *reinterpret_cast<const u16x8*>(src + (int64_t)h * D + o);
  }
  const T* vs = src + (int64_t)(nh + nkv) * D;
  for (int i = threadIdx.x; i < nkv * D / 8; i += 256)
    *reinterpret_cast<u16x8*>(vd + i * 8) = *reinterpret_cast<const u16x8*>(vs + i * 8);
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

template <typename T, int D>
hipError_t decode_attn_mx_launch(const void* q, const void* kq, const void* ksc, const void* vq, const void* vsc,
                                 const int* lens, float* ws_ml, float* ws_acc, int B, int nh, int nkv, int cap,
                                 int nchunks, float scale, hipStream_t st) {
  const dim3 grid((unsigned)nchunks, (unsigned)nkv, (unsigned)B);
#define SMDT_DEC_MX(G)                                                                                   \
  hipLaunchKernelGGL((decode_attn_mx_partial_kernel<T, D, G>), grid, dim3(kMxThreads), 0, st, (const T*)q, \
                     (const uint8_t*)kq, (const uint8_t*)ksc, (const uint8_t*)vq, (const uint8_t*)vsc, lens,  \
                     ws_ml, ws_acc, cap, nkv, scale)
  switch (nh / nkv) {
    case 1: SMDT_DEC_MX(1); break;
    case 2: SMDT_DEC_MX(2); break;
    case 4: SMDT_DEC_MX(4); break;
    case 8: SMDT_DEC_MX(8); break;
    default: return hipErrorInvalidValue;
  }
#undef SMDT_DEC_MX
  return hipGetLastError();
}

}  // namespace smdt

using namespace smdt;

extern "C" hipError_t smdt_decode_attn_mx(int dtype, const void* q, const void* kq, const void* ksc, const void* vq,
                                          const void* vsc, const int* lens, float* ws_ml, float* ws_acc, void* out,
                                          int B, int nh, int nkv, int D, int cap, int max_len, float scale,
                                          hipStream_t st) {
  if (!smdt_decode_attn_supported(dtype, D, nh, nkv) || smdt_decode_attn_chunk() != kMxChunk || B <= 0 ||
      B > 65535 || nkv > 65535 || cap <= 0 || max_len <= 0 || max_len > cap)
    return hipErrorInvalidValue;
  const int nchunks = (max_len + kMxChunk - 1) / kMxChunk;
  hipError_t e;
  if (dtype == 1)
    e = D == 64 ? decode_attn_mx_launch<bf16, 64>(q, kq, ksc, vq, vsc, lens, ws_ml, ws_acc, B, nh, nkv, cap, nchunks, scale, st)
                : decode_attn_mx_launch<bf16, 128>(q, kq, ksc, vq, vsc, lens, ws_ml, ws_acc, B, nh, nkv, cap, nchunks, scale, st);
  else
    e = D == 64 ? decode_attn_mx_launch<f16, 64>(q, kq, ksc, vq, vsc, lens, ws_ml, ws_acc, B, nh, nkv, cap, nchunks, scale, st)
                : decode_attn_mx_launch<f16, 128>(q, kq, ksc, vq, vsc, lens, ws_ml, ws_acc, B, nh, nkv, cap, nchunks, scale, st);
  if (e != hipSuccess) return e;
  return smdt_decode_attn_combine(dtype, ws_ml, ws_acc, lens, out, B, nh, D, cap, nchunks, st);
}

extern "C" hipError_t smdt_decode_rope_append_mx(int dtype, const void* qkv, void* q_out, void* kq, void* ksc,
                                                 void* vq, void* vsc, const int* pos, int B, int nh, int nkv, int D,
                                                 int cap, int rot, const float* cos_t, const float* sin_t,
                                                 int max_pos, hipStream_t st) {
  if ((dtype != 1 && dtype != 2) || B <= 0 || nh <= 0 || nkv <= 0 || D <= 0 || D % 32 || rot % 16 || rot < 0 ||
      rot > D || cap <= 0 || (int64_t)nkv * D > 8192 ||
      (rot > 0 && (cos_t == nullptr || sin_t == nullptr || max_pos <= 0)))
    return hipErrorInvalidValue;
  const unsigned lds = 2u * (unsigned)(nkv * D) * 2u;      // the staged k and v rows: at most 32 KiB
  if (dtype == 1)
    hipLaunchKernelGGL(decode_rope_append_mx_kernel<bf16>, dim3((unsigned)B), dim3(256), lds, st, (const bf16*)qkv,
                       (bf16*)q_out, (uint8_t*)kq, (uint8_t*)ksc, (uint8_t*)vq, (uint8_t*)vsc, pos, nh, nkv, D, cap,
                       rot, cos_t, sin_t, max_pos, 1.f);
  else
    hipLaunchKernelGGL(decode_rope_append_mx_kernel<f16>, dim3((unsigned)B), dim3(256), lds, st, (const f16*)qkv,
                       (f16*)q_out, (uint8_t*)kq, (uint8_t*)ksc, (uint8_t*)vq, (uint8_t*)vsc, pos, nh, nkv, D, cap,
                       rot, cos_t, sin_t, max_pos, 1.f);
  return hipGetLastError();
}
