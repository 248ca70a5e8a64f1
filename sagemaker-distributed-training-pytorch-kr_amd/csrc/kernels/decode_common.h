// What the decode kernels share: decode_attn.hip (16-bit cache), decode_attn_mx.hip (MXFP8 cache)
// and decode_attn_multi.hip (T new tokens per sequence).
//
// The guarantees of the decode path, stated once. Every kernel here and in those files keeps them:
//
//   * Never load beyond lens. `lens` / `pos` are device int32 [B] and are never read on the host.
//     A key at or beyond lens[b] is not loaded: its slot reads row lens[b] - 1 instead (a valid
//     row, element bytes and scale byte alike), so the loads stay unconditional and in flight
//     together, and NaN / Inf / scale 255 in the unused part of a cache cannot reach a result.
//   * Selection, not arithmetic, masks. Such a key's score is -inf and its probability 0 by a
//     select; a chunk wholly beyond lens[b] writes the empty partial (m = -inf, l = 0) and leaves;
//     the combine kernel skips empty partials by a select, so (-inf) - (-inf) is never formed.
//   * Fixed order, no atomics. Partials are fp32 (max m, sum l, unnormalised accumulator) in a
//     workspace, ws_ml [B, heads, nchunks, 2] and ws_acc [B, heads, nchunks, D]; lanes, waves and
//     chunks are summed in one fixed order, so every result is bitwise repeatable.
//   * Append bytes are rope.hip's. Both append kernels rotate in dec_rope_token, which repeats the
//     `rope_` kernels' arithmetic statement for statement, so a row appended at pos[b] holds the
//     bytes the prefill stores for that row. A position outside [0, cap) or the RoPE table writes
//     nothing.
#pragma once
#include <type_traits>

#include "common.h"

namespace smdt {

constexpr int kDecChunk = 256;    // keys per workgroup == threads per workgroup
constexpr int kDecThreads = 256;
constexpr int kDecWaves = kDecThreads / kWave;

__device__ __forceinline__ int dec_clamp_len(int len, int cap) { return len < 0 ? 0 : (len > cap ? cap : len); }

// Workspace index of a chunk's partial for flat head index bh = b * heads + head.
__device__ __forceinline__ int64_t dec_part(int64_t bh, int nchunks, int chunk) { return bh * nchunks + chunk; }
__device__ __forceinline__ void dec_store_ml(float* __restrict__ ws_ml, int64_t part, float m, float l) {
  ws_ml[part * 2] = m;
  ws_ml[part * 2 + 1] = l;
}
// The partial of a chunk that holds no key of the sequence: the combine skips it.
__device__ __forceinline__ void dec_store_empty(float* __restrict__ ws_ml, int64_t part) {
  dec_store_ml(ws_ml, part, -INFINITY, 0.f);
}

// Key chunks of a launch over max_len keys; 0 when the grid or the lengths are out of range.
inline int dec_nchunks(int B, int nkv, int cap, int max_len) {
  if (B <= 0 || B > 65535 || nkv > 65535 || cap <= 0 || max_len <= 0 || max_len > cap) return 0;
  return (max_len + kDecChunk - 1) / kDecChunk;
}

// f(tag) with tag.type the element type of dtype code 1 (bf16) / 2 (fp16); f(tag, D) with D an
// std::integral_constant for head dims 64 / 128. Anything else: hipErrorInvalidValue, f not called.
template <typename T>
struct DecType {
  using type = T;
};
template <typename F>
hipError_t dec_dispatch(int dtype, F&& f) {
  if (dtype == 1) return f(DecType<bf16>{});
  if (dtype == 2) return f(DecType<f16>{});
  return hipErrorInvalidValue;
}
template <typename F>
hipError_t dec_dispatch(int dtype, int D, F&& f) {
  return dec_dispatch(dtype, [&](auto tag) -> hipError_t {
    if (D == 64) return f(tag, std::integral_constant<int, 64>{});
    if (D == 128) return f(tag, std::integral_constant<int, 128>{});
    return hipErrorInvalidValue;
  });
}

// One cache tensor (K or V) as the partial kernel reads it: kEPL elements per lane and 16-byte
// load, load(e, f) of the lane's piece at element offset e, and, with kScaled, scale(s) of the
// piece's block at scale offset s. This is the 16-bit cache, [B, cap, nkv, D] of T; the MXFP8 one
// is in decode_attn_mx.hip.
template <typename T>
struct DecKv16 {
  static constexpr int kEPL = 8;
  static constexpr bool kScaled = false;
  using Raw = u16x8;
  const T* __restrict__ p;
  __device__ __forceinline__ Raw load(int64_t e) const { return __builtin_nontemporal_load(reinterpret_cast<const Raw*>(p + e)); }
  static __device__ __forceinline__ void to_f32(const Raw& r, float (&f)[kEPL]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      unsigned short bits = r[j];
      T t;
      __builtin_memcpy(&t, &bits, 2);
      f[j] = smdt::to_f32(t);
    }
  }
};

// Split-KV attention of one query per sequence, first launch: one 256-thread workgroup per (key
// chunk of 256, kv head, sequence). It serves ALL G = nh / nkv query heads of its kv head, so every
// K / V byte is read once whatever the group size. A lane loads 16 bytes along D (KV::kEPL
// elements), LPK adjacent lanes cover one key row and the workgroup covers 256 / LPK keys per
// step. Pass 1 puts the G scaled scores of every key of the chunk in LDS (plain fp32 FMAs, a
// butterfly over the LPK lanes of a row); the chunk maximum and the probabilities follow; pass 2
// accumulates p V in registers and the key slots are summed in a fixed order (wave shuffles, then
// the four waves through LDS). A scaled cache holds one block scale per lane piece: it multiplies
// the lane's q . k sum once, before the butterfly, and the key's probability once per query head.
template <typename T, int D, int G, typename KV>
__global__ __launch_bounds__(kDecThreads) void decode_attn_partial_kernel(
    const T* __restrict__ q, const KV kc, const KV vc, const int* __restrict__ lens, float* __restrict__ ws_ml,
    float* __restrict__ ws_acc, int cap, int nkv, float scale) {
  constexpr int EPL = KV::kEPL;               // elements per lane
  constexpr int LPK = D / EPL;                // lanes per key row
  constexpr int KPB = kDecThreads / LPK;      // keys per workgroup step
  constexpr int STEPS = kDecChunk / KPB;
  constexpr int BPL = 32 / EPL;               // lanes per 32-element scale block
  constexpr int SPR = D / 32;                 // scale bytes per key row
  static_assert(kWave / LPK >= 1, "a key row fits in a wave");
  const int chunk = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
  const int nchunks = gridDim.x, nh = nkv * G;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int lk = tid % LPK, ks = tid / LPK;
  const int len = dec_clamp_len(lens[b], cap);
  const int k0 = chunk * kDecChunk;
  const int64_t part0 = dec_part((int64_t)b * nh + (int64_t)kvh * G, nchunks, chunk);     // head g: + g * nchunks
  if (k0 >= len) {
    if (tid < G) dec_store_empty(ws_ml, part0 + (int64_t)tid * nchunks);
    return;
  }
  __shared__ float sc[G][kDecChunk];               // scores, then probabilities
  __shared__ float red[2][G][kDecWaves];
  __shared__ float racc[kDecWaves][G][D];

  const int64_t row0 = (int64_t)b * cap * nkv + kvh;          // row of key 0; key k: + k * nkv
  const int64_t ebase = row0 * D + lk * EPL;                  // elements of this lane
  const int64_t sbase = row0 * SPR + lk / BPL;                // its block's scale
  const int64_t erow = (int64_t)nkv * D, srow = (int64_t)nkv * SPR;

  // ---- pass 1: scores
  {
    float qf[G][EPL];
#pragma unroll
    for (int g = 0; g < G; ++g) load_vec<T, EPL>(q + ((int64_t)b * nh + kvh * G + g) * D + lk * EPL, qf[g]);
#pragma unroll 4
    for (int it = 0; it < STEPS; ++it) {
      const int kl = it * KPB + ks;
      const int key = k0 + kl;
      const int kr = key < len ? key : len - 1;     // a valid row, selected out below
      const typename KV::Raw kw = kc.load(ebase + (int64_t)kr * erow);
      [[maybe_unused]] float kscale;
      if constexpr (KV::kScaled) kscale = kc.scale(sbase + (int64_t)kr * srow);
      float kf[EPL];
      KV::to_f32(kw, kf);
      float s[G];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        s[g] = 0.f;
#pragma unroll
        for (int j = 0; j < EPL; ++j) s[g] += qf[g][j] * kf[j];
        if constexpr (KV::kScaled) s[g] *= kscale;
      }
#pragma unroll
      for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int o = LPK / 2; o > 0; o >>= 1) s[g] += __shfl_xor(s[g], o, kWave);
      }
#pragma unroll
      for (int g = 0; g < G; ++g)                   // every lane of the row holds all G sums
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
    for (int w = 1; w < kDecWaves; ++w) m[g] = fmaxf(m[g], red[0][g][w]);
    // key k0 is valid, so m is finite unless a valid score is itself -inf
    const float p = sv[g] == -INFINITY ? 0.f : __expf(sv[g] - m[g]);
    sc[g][tid] = p;
    const float wsum = wave_sum(p);
    if (lane == 0) red[1][g][wid] = wsum;
  }
  __syncthreads();

  // ---- pass 2: acc[g] += p[g][key] * v[key]
  float acc[G][EPL];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int j = 0; j < EPL; ++j) acc[g][j] = 0.f;
#pragma unroll 4
  for (int it = 0; it < STEPS; ++it) {
    const int kl = it * KPB + ks;
    const int key = k0 + kl;
    const int kr = key < len ? key : len - 1;       // as in pass 1; such a key's p is 0
    const typename KV::Raw vw = vc.load(ebase + (int64_t)kr * erow);
    [[maybe_unused]] float vscale;
    if constexpr (KV::kScaled) vscale = vc.scale(sbase + (int64_t)kr * srow);
    float vf[EPL];
    KV::to_f32(vw, vf);
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float p = sc[g][kl];
      if constexpr (KV::kScaled) p *= vscale;
#pragma unroll
      for (int j = 0; j < EPL; ++j) acc[g][j] += p * vf[j];
    }
  }
  // the key slots of a wave (lanes with equal lk), in a fixed order
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int j = 0; j < EPL; ++j) {
#pragma unroll
      for (int o = LPK; o < kWave; o <<= 1) acc[g][j] += __shfl_xor(acc[g][j], o, kWave);
    }
  if (lane < LPK) {
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int j = 0; j < EPL; ++j) racc[wid][g][lk * EPL + j] = acc[g][j];
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
    dec_store_ml(ws_ml, part0 + (int64_t)tid * nchunks, mx, l);
  }
}

// The partial launch over the supported group sizes G = nh / nkv.
template <typename T, int D, typename KV>
hipError_t decode_attn_partial_launch(const void* q, KV kc, KV vc, const int* lens, float* ws_ml, float* ws_acc, int B,
                                      int nh, int nkv, int cap, int nchunks, float scale, hipStream_t st) {
  const dim3 grid((unsigned)nchunks, (unsigned)nkv, (unsigned)B);
#define SMDT_DEC(G)                                                                                          \
  hipLaunchKernelGGL((decode_attn_partial_kernel<T, D, G, KV>), grid, dim3(kDecThreads), 0, st, (const T*)q, \
                     kc, vc, lens, ws_ml, ws_acc, cap, nkv, scale)
  switch (nh / nkv) {
    case 1: SMDT_DEC(1); break;
    case 2: SMDT_DEC(2); break;
    case 4: SMDT_DEC(4); break;
    case 8: SMDT_DEC(8); break;
    default: return hipErrorInvalidValue;
  }
#undef SMDT_DEC
  return hipGetLastError();
}

__device__ __forceinline__ bool dec_pos_ok(int64_t pos, int cap, int rot, int max_pos) {
  return pos >= 0 && pos < cap && (rot <= 0 || pos < max_pos);
}

// One new token, by one 256-thread workgroup: rotate the q and k heads of its row `src`
// [(nh + 2 nkv) D] at position pos over their first rot elements and copy what is not rotated; q
// goes to qd [nh, D], k to kd and v to vd [nkv, D] (a cache row, or an LDS stage). rot == 0: no
// RoPE (learned positions), a pure copy. The caller has checked the position (dec_pos_ok).
template <typename T>
__device__ __forceinline__ void dec_rope_token(const T* src, T* qd, T* kd, T* vd, int64_t pos, int nh, int nkv, int D,
                                               int rot, const float* cos_t, const float* sin_t, float sign) {
  const int half = rot / 2;
  const int groups = half / 8;              // rotated 8-pair groups per head
  const int tail = (D - rot) / 8;           // unrotated 16-byte pieces per head
  const float* ct = cos_t + pos * half;
  const float* stb = sin_t + pos * half;
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
    for (int j = 0; j < 8; ++j) {            // rope.hip's statements
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

}  // namespace smdt
