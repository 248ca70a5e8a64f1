// Incremental decoding for gfx950: one new query per sequence against a growing K/V cache.
//
// The training kernels (flash_attn.hip, rope.hip) take all queries at once at S % 128 == 0. A
// decode step has ONE query row per head: the work is reading the cache once (2 S nkv D elements
// per sequence) and the launch count, not the matrix core. Two entry points:
//
//   smdt_decode_attn         split-KV attention of q [B, nh, D] against k / v [B, cap, nkv, D]
//   smdt_decode_rope_append  RoPE on the new token's q / k (bitwise rope.hip's) and the append of
//                            its k / v into row pos[b] of the caches
//
// Neither reads a length on the host: `lens` / `pos` are device int32 [B], so with static shapes a
// decode step can be captured in a graph.
//
// Attention, first launch: one 256-thread workgroup per (key chunk of 256, kv head, sequence). It
// serves ALL G = nh / nkv query heads of its kv head, so every K / V byte is read once whatever
// the group size. A lane loads 16 bytes along D (8 elements), D / 8 adjacent lanes cover one key
// row and the workgroup covers 256 / (D / 8) keys per step. Pass 1 puts the G scaled scores of
// every key of the chunk in LDS (plain fp32 FMAs, a butterfly over the D / 8 lanes of a row);
// the chunk maximum and the probabilities follow; pass 2 accumulates p V in registers and the
// key slots are summed in a fixed order (wave shuffles, then the four waves through LDS). Keys at
// or beyond lens[b] are never loaded (such a slot reads the last valid row instead) and their score
// is -inf by selection, so NaN / Inf in the unused part of the cache cannot reach the result. The
// workgroup writes fp32 partials (max m, sum l, unnormalised accumulator) to a workspace. A chunk
// wholly beyond lens[b] writes m = -inf, l = 0 and leaves.
//
// Second launch: one workgroup per (query head, sequence) combines the partials of the chunks that
// hold keys, rescaling each by exp(m_c - max m). Chunks with l = 0 are skipped by selection, so
// (-inf) - (-inf) is never formed. No atomics anywhere: the result is bitwise repeatable.
#include "common.h"
#include "launchers.h"

namespace smdt {

constexpr int kDecChunk = 256;    // keys per workgroup == threads per workgroup
constexpr int kDecThreads = 256;
constexpr int kDecWaves = kDecThreads / kWave;

template <typename T, int D, int G>
__global__ __launch_bounds__(kDecThreads) void decode_attn_partial_kernel(
    const T* __restrict__ q, const T* __restrict__ kc, const T* __restrict__ vc,
    const int* __restrict__ lens, float* __restrict__ ws_ml, float* __restrict__ ws_acc, int cap,
    int nkv, float scale) {
  constexpr int LPK = D / 8;                  // lanes per key row
  constexpr int KPB = kDecThreads / LPK;      // keys per workgroup step
  constexpr int STEPS = kDecChunk / KPB;
  constexpr int KPW = kWave / LPK;            // key slots per wave
  const int chunk = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
  const int nchunks = gridDim.x, nh = nkv * G;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int lk = tid % LPK, ks = tid / LPK;
  int len = lens[b];
  len = len < 0 ? 0 : (len > cap ? cap : len);
  const int k0 = chunk * kDecChunk;
  const int64_t part0 = ((int64_t)b * nh + (int64_t)kvh * G) * nchunks + chunk;   // head g: + g * nchunks
  if (k0 >= len) {      // no key of this sequence in the chunk: a partial the combine skips
    if (tid < G) {
      ws_ml[(part0 + (int64_t)tid * nchunks) * 2] = -INFINITY;
      ws_ml[(part0 + (int64_t)tid * nchunks) * 2 + 1] = 0.f;
    }
    return;
  }
  __shared__ float sc[G][kDecChunk];               // scores, then probabilities
  __shared__ float red[2][G][kDecWaves];
  __shared__ float racc[kDecWaves][G][D];

  const int64_t row_stride = (int64_t)nkv * D;
  const int64_t base = ((int64_t)b * cap * nkv + kvh) * D + lk * 8;

  // ---- pass 1: scores
  {
    float qf[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g) load_vec<T, 8>(q + ((int64_t)b * nh + kvh * G + g) * D + lk * 8, qf[g]);
#pragma unroll 4
    for (int it = 0; it < STEPS; ++it) {
      const int kl = it * KPB + ks;
      const int key = k0 + kl;
      // a key at or beyond len reads row len - 1 instead (a valid row: the load stays
      // unconditional, so the unrolled steps' loads are all in flight together) and is selected out
      const int kr = key < len ? key : len - 1;
      float kf[8];
      load_vec<T, 8, true>(kc + base + (int64_t)kr * row_stride, kf);
      float s[G];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        s[g] = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) s[g] += qf[g][j] * kf[j];
      }
#pragma unroll
      for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int o = LPK / 2; o > 0; o >>= 1) s[g] += __shfl_xor(s[g], o, kWave);
      }
#pragma unroll
      for (int g = 0; g < G; ++g)
        if (lk == g) sc[g][kl] = key < len ? s[g] * scale : -INFINITY;
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
    for (int w = 1; w < kDecWaves; ++w) m[g] = fmaxf(m[g], red[0][g][w]);
    // key k0 is valid, so m is finite unless a valid score is itself -inf
    const float p = sv[g] == -INFINITY ? 0.f : __expf(sv[g] - m[g]);
    sc[g][tid] = p;
    const float wsum = wave_sum(p);
    if (lane == 0) red[1][g][wid] = wsum;
  }
  __syncthreads();

  // ---- pass 2: acc[g] += p[g][key] * v[key]
  float acc[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[g][j] = 0.f;
#pragma unroll 4
  for (int it = 0; it < STEPS; ++it) {
    const int kl = it * KPB + ks;
    const int key = k0 + kl;
    const int kr = key < len ? key : len - 1;       // as in pass 1; such a key's p is 0
    float vf[8];
    load_vec<T, 8, true>(vc + base + (int64_t)kr * row_stride, vf);
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const float p = sc[g][kl];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[g][j] += p * vf[j];
    }
  }
  // the key slots of a wave (lanes with equal lk), in a fixed order
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
#pragma unroll
      for (int o = LPK; o < kWave; o <<= 1) acc[g][j] += __shfl_xor(acc[g][j], o, kWave);
    }
  static_assert(KPW >= 1, "a key row fits in a wave");
  if (lane < LPK) {
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int j = 0; j < 8; ++j) racc[wid][g][lk * 8 + j] = acc[g][j];
  }
  __syncthreads();
  for (int i = tid; i < G * D; i += kDecThreads) {
    const int g = i / D, d = i - g * D;
    float a = racc[0][g][d];
#pragma unroll
    for (int w = 1; w < kDecWaves; ++w) a += racc[w][g][d];
    ws_acc[(part0 + (int64_t)g * nchunks) * D + d] = a;
  }
  if (tid < G) {
    float mx = red[0][tid][0], l = red[1][tid][0];
#pragma unroll
    for (int w = 1; w < kDecWaves; ++w) {
      mx = fmaxf(mx, red[0][tid][w]);
      l += red[1][tid][w];
    }
    ws_ml[(part0 + (int64_t)tid * nchunks) * 2] = mx;
    ws_ml[(part0 + (int64_t)tid * nchunks) * 2 + 1] = l;
  }
}

// out[b, h, :] = sum_c w_c acc_c / sum_c w_c l_c with w_c = exp(m_c - max_c m_c) over the chunks
// that hold keys of sequence b. One thread per output column; chunks in index order.
template <typename T, int D>
__global__ __launch_bounds__(D) void decode_attn_combine_kernel(const float* __restrict__ ws_ml,
                                                                const float* __restrict__ ws_acc,
                                                                const int* __restrict__ lens,
                                                                T* __restrict__ out, int cap, int nchunks) {
  const int h = blockIdx.x, b = blockIdx.y, nh = gridDim.x, d = threadIdx.x;
  int len = lens[b];
  len = len < 0 ? 0 : (len > cap ? cap : len);
  int nc = (len + kDecChunk - 1) / kDecChunk;
  nc = nc > nchunks ? nchunks : nc;
  const int64_t p0 = ((int64_t)b * nh + h) * nchunks;
  float M = -INFINITY;
  for (int c = 0; c < nc; ++c) {
    const float mc = ws_ml[(p0 + c) * 2], lc = ws_ml[(p0 + c) * 2 + 1];
    if (lc > 0.f) M = fmaxf(M, mc);
  }
  float num = 0.f, den = 0.f;
  for (int c = 0; c < nc; ++c) {
    const float mc = ws_ml[(p0 + c) * 2], lc = ws_ml[(p0 + c) * 2 + 1];
    if (lc > 0.f) {       // an empty partial (m = -inf, l = 0) is skipped, never multiplied
      const float w = __expf(mc - M);
      num += w * ws_acc[(p0 + c) * D + d];
      den += w * lc;
    }
  }
  out[((int64_t)b * nh + h) * D + d] = from_f32<T>(den > 0.f ? num / den : 0.f);
}

// One workgroup per new token: rotate q and k at position pos[b] (rope.hip's arithmetic, so the
// bytes equal what the prefill path stores for the same row), copy what is not rotated, and write
// q to q_out [B, nh, D], k and v to row pos[b] of the caches [B, cap, nkv, D]. rot == 0: no RoPE
// (learned positions), a pure copy. A position outside [0, cap) or the table writes nothing.
template <typename T>
__global__ __launch_bounds__(256) void decode_rope_append_kernel(
    const T* __restrict__ qkv, T* __restrict__ q_out, T* __restrict__ kc, T* __restrict__ vc,
    const int* __restrict__ pos_t, int nh, int nkv, int D, int cap, int rot,
    const float* __restrict__ cos_t, const float* __restrict__ sin_t, int max_pos, float sign) {
  const int b = blockIdx.x;
  const int pos = pos_t[b];
  if (pos < 0 || pos >= cap || (rot > 0 && pos >= max_pos)) return;
  const int half = rot / 2;
  const int groups = half / 8;              // rotated 8-pair groups per head
  const int tail = (D - rot) / 8;           // unrotated 16-byte pieces per head
  const int W = (nh + 2 * nkv) * D;
  const T* src = qkv + (int64_t)b * W;
  T* qd = q_out + (int64_t)b * nh * D;
  T* kd = kc + ((int64_t)b * cap + pos) * nkv * D;
  T* vd = vc + ((int64_t)b * cap + pos) * nkv * D;
  const float* ct = cos_t + (int64_t)pos * half;
  const float* stb = sin_t + (int64_t)pos * half;
  for (int i = threadIdx.x; i < (nh + nkv) * groups; i += 256) {
    const int h = i / groups, gidx = i - h * groups;
    const T* base = src + (int64_t)h * D + gidx * 8;
    T* dst = (h < nh ? qd + (int64_t)h * D : kd + (int64_t)(h - nh) * D) + gidx * 8;
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
    store_vec<T, 8>(dst, oa);
    store_vec<T, 8>(dst + half, ob);
  }
  // the unrotated tail of the q / k heads, and v: 16-byte copies
  for (int i = threadIdx.x; i < (nh + nkv) * tail; i += 256) {
    const int h = i / tail, o = rot + (i - h * tail) * 8;
    T* dst = (h < nh ? qd + (int64_t)h * D : kd + (int64_t)(h - nh) * D) + o;
    *reinterpret_cast<u16x8*>(dst) = *reinterpret_cast<const u16x8*>(src + (int64_t)h * D + o);
  }
  const T* vs = src + (int64_t)(nh + nkv) * D;
  for (int i = threadIdx.x; i < nkv * D / 8; i += 256)
    *reinterpret_cast<u16x8*>(vd + i * 8) = *reinterpret_cast<const u16x8*>(vs + i * 8);
}

template <typename T, int D>
hipError_t decode_attn_launch(const void* q, const void* kc, const void* vc, const int* lens, float* ws_ml,
                              float* ws_acc, void* out, int B, int nh, int nkv, int cap, int nchunks,
                              float scale, hipStream_t st) {
  const dim3 grid((unsigned)nchunks, (unsigned)nkv, (unsigned)B);
#define SMDT_DEC(G)                                                                                    \
  hipLaunchKernelGGL((decode_attn_partial_kernel<T, D, G>), grid, dim3(kDecThreads), 0, st, (const T*)q, \
                     (const T*)kc, (const T*)vc, lens, ws_ml, ws_acc, cap, nkv, scale)
  switch (nh / nkv) {
    case 1: SMDT_DEC(1); break;
    case 2: SMDT_DEC(2); break;
    case 4: SMDT_DEC(4); break;
    case 8: SMDT_DEC(8); break;
    default: return hipErrorInvalidValue;
  }
#undef SMDT_DEC
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((decode_attn_combine_kernel<T, D>), dim3((unsigned)nh, (unsigned)B), dim3(D), 0, st, ws_ml,
                     ws_acc, lens, (T*)out, cap, nchunks);
  return hipGetLastError();
}

}  // namespace smdt

using namespace smdt;

extern "C" int smdt_decode_attn_chunk() { return kDecChunk; }

extern "C" int smdt_decode_attn_supported(int dtype, int D, int nh, int nkv) {
  if (dtype != 1 && dtype != 2) return 0;
  if (D != 64 && D != 128) return 0;
  if (nh <= 0 || nkv <= 0 || nh % nkv) return 0;
  const int g = nh / nkv;
  return g == 1 || g == 2 || g == 4 || g == 8;
}

extern "C" hipError_t smdt_decode_attn(int dtype, const void* q, const void* k_cache, const void* v_cache,
                                       const int* lens, float* ws_ml, float* ws_acc, void* out, int B, int nh,
                                       int nkv, int D, int cap, int max_len, float scale, hipStream_t st) {
  if (!smdt_decode_attn_supported(dtype, D, nh, nkv) || B <= 0 || B > 65535 || nkv > 65535 || cap <= 0 ||
      max_len <= 0 || max_len > cap)
    return hipErrorInvalidValue;
  const int nchunks = (max_len + kDecChunk - 1) / kDecChunk;
  if (dtype == 1) {
    if (D == 64) return decode_attn_launch<bf16, 64>(q, k_cache, v_cache, lens, ws_ml, ws_acc, out, B, nh, nkv, cap, nchunks, scale, st);
    return decode_attn_launch<bf16, 128>(q, k_cache, v_cache, lens, ws_ml, ws_acc, out, B, nh, nkv, cap, nchunks, scale, st);
  }
  if (D == 64) return decode_attn_launch<f16, 64>(q, k_cache, v_cache, lens, ws_ml, ws_acc, out, B, nh, nkv, cap, nchunks, scale, st);
  return decode_attn_launch<f16, 128>(q, k_cache, v_cache, lens, ws_ml, ws_acc, out, B, nh, nkv, cap, nchunks, scale, st);
}

extern "C" hipError_t smdt_decode_rope_append(int dtype, const void* qkv, void* q_out, void* k_cache, void* v_cache,
                                              const int* pos, int B, int nh, int nkv, int D, int cap, int rot,
                                              const float* cos_t, const float* sin_t, int max_pos,
                                              hipStream_t st) {
  if ((dtype != 1 && dtype != 2) || B <= 0 || D % 8 || rot % 16 || rot < 0 || rot > D || cap <= 0 ||
      (rot > 0 && (cos_t == nullptr || sin_t == nullptr || max_pos <= 0)))
    return hipErrorInvalidValue;
  if (dtype == 1)
    hipLaunchKernelGGL(decode_rope_append_kernel<bf16>, dim3((unsigned)B), dim3(256), 0, st, (const bf16*)qkv,
                       (bf16*)q_out, (bf16*)k_cache, (bf16*)v_cache, pos, nh, nkv, D, cap, rot, cos_t, sin_t,
                       max_pos, 1.f);
  else
    hipLaunchKernelGGL(decode_rope_append_kernel<f16>, dim3((unsigned)B), dim3(256), 0, st, (const f16*)qkv,
                       (f16*)q_out, (f16*)k_cache, (f16*)v_cache, pos, nh, nkv, D, cap, rot, cos_t, sin_t,
                       max_pos, 1.f);
  return hipGetLastError();
}

// The combine launch alone, for partials written by another kernel with this file's workspace
// layout and chunk length (decode_attn_mx.hip).
extern "C" hipError_t smdt_decode_attn_combine(int dtype, const float* ws_ml, const float* ws_acc, const int* lens,
                                               void* out, int B, int nh, int D, int cap, int nchunks, hipStream_t st) {
  if ((dtype != 1 && dtype != 2) || (D != 64 && D != 128) || B <= 0 || B > 65535 || nh <= 0 || cap <= 0 ||
      nchunks <= 0)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)nh, (unsigned)B);
  if (dtype == 1) {
    if (D == 64) hipLaunchKernelGGL((decode_attn_combine_kernel<bf16, 64>), grid, dim3(64), 0, st, ws_ml, ws_acc, lens, (bf16*)out, cap, nchunks);
    else hipLaunchKernelGGL((decode_attn_combine_kernel<bf16, 128>), grid, dim3(128), 0, st, ws_ml, ws_acc, lens, (bf16*)out, cap, nchunks);
  } else {
    if (D == 64) hipLaunchKernelGGL((decode_attn_combine_kernel<f16, 64>), grid, dim3(64), 0, st, ws_ml, ws_acc, lens, (f16*)out, cap, nchunks);
    else hipLaunchKernelGGL((decode_attn_combine_kernel<f16, 128>), grid, dim3(128), 0, st, ws_ml, ws_acc, lens, (f16*)out, cap, nchunks);
  }
  return hipGetLastError();
}
