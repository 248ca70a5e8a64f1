// A decode step with T new tokens per sequence for gfx950 (speculative verification: the target
// model checks k drafted tokens and the last emitted one, T = k + 1, in one pass over its weights).
//
//   smdt_decode_rope_append_multi  RoPE on the T new tokens' q / k (bitwise rope.hip's) and the
//                                  append of their k / v into cache rows pos[b] .. pos[b] + T - 1;
//                                  T = 1 is the single-token decode step's append
//   smdt_decode_attn_multi         split-KV attention of q [B, T, nh, D] against k / v
//                                  [B, cap, nkv, D]; query t sees keys 0 .. lens[b] - T + t
//
// decode_common.h states the guarantees these keep (lengths stay on the device, nothing beyond
// lens[b] is loaded, masking by selection, fixed order, no atomics).
//
// Attention. The grid is the single-query kernel's: one 256-thread workgroup per (key chunk of 256,
// kv head, sequence). It serves all R = T G query rows of its kv head (G = nh / nkv; row r = t G + g),
// so every cache byte is still read once. With R rows the score and P V products are matrix
// products and run on v_mfma_f32_16x16x32 (lane l: c = l & 15, qd = l >> 4; A[row c][k = 8 qd + j],
// B[k = 8 qd + j][col c], D[row 4 qd + reg][col c]); the rows are padded to RT = ceil(R / 16) tiles
// (a padding row reads row R - 1 and is never stored).
//
//   * Wave w owns keys 64 w .. 64 w + 63 of the chunk. Scores are formed TRANSPOSED, S^T = K Q^T:
//     the A operand is a key row and the B operand a query row, both 16-byte global loads in
//     operand layout, no LDS. A lane then holds S^T[key 4 qd + reg][row c]: its query row is fixed,
//     so the row's key limit is a per-lane scalar and a row statistic is a reduction over the
//     registers, the four qd groups (two shuffles) and the four waves (LDS).
//   * A key at or beyond lens[b] is never loaded (the lane reads row lens[b] - 1 instead); a key at
//     or beyond a ROW's limit lens[b] - T + t + 1 gets score -inf and probability 0, both by
//     selection. Rows in between are the new tokens after t: real rows of finite values that the
//     product multiplies by an exact zero, so their bits cannot reach query t's result. NaN / Inf
//     beyond lens[b] is harmless.
//   * P = exp(S - chunk maximum) is rounded to the 16-bit type and is, as it lies in the registers,
//     the B operand of O^T = V^T P^T with the contraction index permuted: element j of lane group
//     qd is key 16 (j >> 2) + 4 qd + (j & 3) of a 32-key step. V^T, the A operand, takes the same
//     keys: the wave stages its 32 V rows in LDS (rows of 2 D + 32 bytes, so the 8 rows a 32-lane
//     half reads lie on 8 distinct 32-byte bank groups) and reads them with ds_read_b64_tr_b16, two
//     4-row blocks per fragment. The row sum l adds the unrounded fp32 probabilities.
//   * The four waves' O^T tiles are summed in a fixed order, (w0 + w1) + (w2 + w3), through LDS.
//
// Partials go to decode_attn.hip's workspace with nh' = T nh heads per sequence and head t nh + h;
// smdt_decode_attn_combine finishes them (a row with no visible key in a chunk has l = 0 there and
// is skipped by selection; a query with no visible key at all returns zeros).
#include "decode_common.h"
#include "launchers.h"
#include "mfma_tile.h"

namespace smdt {

constexpr int kDecMultiMaxT = 8;        // R = T G <= 64: four 16-row tiles
static_assert(kDecChunk == 256 && kDecThreads == 256, "four waves of 64 keys: the tiling below is written for 256");

__device__ __forceinline__ f32x4 mt_mma(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mt_mma(mt::f16x8 a, mt::f16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

template <typename E, int D, int RT>
__global__ __launch_bounds__(kDecThreads) void decode_attn_multi_kernel(
    const E* __restrict__ q, const E* __restrict__ kc, const E* __restrict__ vc, const int* __restrict__ lens,
    float* __restrict__ ws_ml, float* __restrict__ ws_acc, int cap, int nkv, int G, int Tn, float scale) {
  using V8 = mt::v8_t<E>;
  constexpr int KS = D / 32;                 // MFMA k-steps of the score product
  constexpr int DT = D / 16;                 // 16-wide d tiles of O^T
  constexpr int VS = 2 * D + 32;             // bytes per staged V row
  constexpr int VN = D / 16;                 // 16-byte pieces a lane stages per 32-key step
  constexpr int NT = DT * RT;                // O^T tiles per wave
  constexpr int NP = NT < 16 ? NT : 16;      // tiles per reduction pass
  constexpr int kStage = 4 * 32 * VS, kRed = 2 * NP * 64 * 16;
  const int chunk = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
  const int nchunks = gridDim.x, nh = nkv * G, R = Tn * G;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int c = lane & 15, qd = lane >> 4;
  const int len = dec_clamp_len(lens[b], cap);
  const int k0 = chunk * kDecChunk;
  // workspace index of query row r = t G + g: head t nh + kvh G + g of nh' = T nh
  auto part = [&](int r) -> int64_t {
    const int t = r / G, g = r - t * G;
    return dec_part((int64_t)b * Tn * nh + (int64_t)t * nh + kvh * G + g, nchunks, chunk);
  };
  if (k0 >= len) {
    if (tid < R) dec_store_empty(ws_ml, part(tid));
    return;
  }
  __shared__ __attribute__((aligned(16))) char smem[kStage > kRed ? kStage : kRed];
  __shared__ float red_m[4][RT * 16];
  __shared__ float red_l[4][RT * 16];

  const int64_t row_stride = (int64_t)nkv * D;
  const int64_t cbase = ((int64_t)b * cap * nkv + kvh) * D;
  const int kw = k0 + wid * 64;              // the wave's first key

  // ---- the V rows of the wave's two 32-key steps: loaded now, staged before their product
  u16x8 vreg[2][VN];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk)
#pragma unroll
    for (int n = 0; n < VN; ++n) {
      const int idx = lane + 64 * n, i = idx / (D / 8), piece = idx - i * (D / 8);
      const int key = kw + kk * 32 + i;
      const int kr = key < len ? key : len - 1;      // a valid row; its probability is 0
      vreg[kk][n] = *reinterpret_cast<const u16x8*>(vc + cbase + (int64_t)kr * row_stride + piece * 8);
    }

  // ---- scores S^T[key][row] = K Q^T, scaled; a key at or beyond the row's limit: -inf
  f32x4 s[4][RT];
  int lim[RT];
  {
    V8 qf[RT][KS];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const int r = rt * 16 + c, rr = r < R ? r : R - 1;
      const int t = rr / G, g = rr - t * G;
      const int lm = len - Tn + t + 1;               // query t sees keys 0 .. len - T + t
      lim[rt] = r < R && lm > 0 ? lm : 0;
      const E* qp = q + (((int64_t)b * Tn + t) * nh + kvh * G + g) * D + 8 * qd;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) qf[rt][ks] = *reinterpret_cast<const V8*>(qp + 32 * ks);
    }
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const int key = kw + kt * 16 + c;
      const int kr = key < len ? key : len - 1;
      const E* kp = kc + cbase + (int64_t)kr * row_stride + 8 * qd;
      V8 kf[KS];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) kf[ks] = *reinterpret_cast<const V8*>(kp + 32 * ks);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) a = mt_mma(kf[ks], qf[rt][ks], a);
#pragma unroll
        for (int e = 0; e < 4; ++e) a[e] = kw + kt * 16 + 4 * qd + e < lim[rt] ? a[e] * scale : -INFINITY;
        s[kt][rt] = a;
      }
    }
  }

  // ---- chunk maximum of every row
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    float m = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int e = 0; e < 4; ++e) m = fmaxf(m, s[kt][rt][e]);
    m = fmaxf(m, __shfl_xor(m, 16, kWave));
    m = fmaxf(m, __shfl_xor(m, 32, kWave));
    if (qd == 0) red_m[wid][rt * 16 + c] = m;
  }
  __syncthreads();

  // ---- probabilities: their fp32 sum, and rounded to E as the B operand of O^T = V^T P^T
  V8 pf[2][RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int r = rt * 16 + c;
    const float m = fmaxf(fmaxf(red_m[0][r], red_m[1][r]), fmaxf(red_m[2][r], red_m[3][r]));
    float l = 0.f;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        // a row with no key in the chunk has m = -inf and every score selected out
        const float p = s[kt][rt][e] == -INFINITY ? 0.f : __expf(s[kt][rt][e] - m);
        l += p;
        pf[kt >> 1][rt][4 * (kt & 1) + e] = (E)p;
      }
    l += __shfl_xor(l, 16, kWave);
    l += __shfl_xor(l, 32, kWave);
    if (qd == 0) red_l[wid][r] = l;
  }

  // ---- O^T[d][row] += V^T P^T over the wave's two 32-key steps
  f32x4 o[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) o[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  char* vst = smem + wid * 32 * VS;
  // lane 4 q' + p of a 16-lane group addresses row q', columns 4 p .. 4 p + 3 of the group's block
  const int tr0 = (4 * qd + (c >> 2)) * VS + 8 * (c & 3);
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    if (kk) __syncthreads();                 // the reads of step 0 are done
#pragma unroll
    for (int n = 0; n < VN; ++n) {
      const int idx = lane + 64 * n, i = idx / (D / 8), piece = idx - i * (D / 8);
      *reinterpret_cast<u16x8*>(vst + i * VS + piece * 16) = vreg[kk][n];
    }
    __syncthreads();
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      // element j of lane group qd: key 16 (j >> 2) + 4 qd + (j & 3), column 16 dt + c
      const mt::s16x4 x = __builtin_amdgcn_ds_read_tr16_b64_v4i16((mt::lds_s16x4*)(vst + tr0 + 32 * dt));
      const mt::s16x4 y = __builtin_amdgcn_ds_read_tr16_b64_v4i16((mt::lds_s16x4*)(vst + tr0 + 16 * VS + 32 * dt));
      const V8 vf = __builtin_bit_cast(V8, __builtin_shufflevector(x, y, 0, 1, 2, 3, 4, 5, 6, 7));
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) o[dt * RT + rt] = mt_mma(vf, pf[kk][rt], o[dt * RT + rt]);
    }
  }

  // ---- the four waves' tiles in a fixed order: (w0 + w1) + (w2 + w3)
  f32x4* rb = reinterpret_cast<f32x4*>(smem);
#pragma unroll
  for (int p0 = 0; p0 < NT; p0 += NP) {
    __syncthreads();                         // the staged rows / the previous pass have been read
    if (wid & 1) {
#pragma unroll
      for (int i = 0; i < NP; ++i) rb[((wid >> 1) * NP + i) * 64 + lane] = o[p0 + i];
    }
    __syncthreads();
    if (!(wid & 1)) {
#pragma unroll
      for (int i = 0; i < NP; ++i) o[p0 + i] += rb[((wid >> 1) * NP + i) * 64 + lane];
    }
    __syncthreads();
    if (wid == 2) {
#pragma unroll
      for (int i = 0; i < NP; ++i) rb[i * 64 + lane] = o[p0 + i];
    }
    __syncthreads();
    if (wid == 0) {
#pragma unroll
      for (int i = 0; i < NP; ++i) o[p0 + i] += rb[i * 64 + lane];
    }
  }
  if (wid == 0) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const int r = rt * 16 + c;
      if (r < R) {
        float* dst = ws_acc + part(r) * D + 4 * qd;        // O^T[d = 16 dt + 4 qd + e][row r]
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) *reinterpret_cast<f32x4*>(dst + 16 * dt) = o[dt * RT + rt];
      }
    }
  }
  if (tid < R) {        // red_l was written before the product's barriers
    const float m = fmaxf(fmaxf(red_m[0][tid], red_m[1][tid]), fmaxf(red_m[2][tid], red_m[3][tid]));
    const float l = ((red_l[0][tid] + red_l[1][tid]) + red_l[2][tid]) + red_l[3][tid];
    dec_store_ml(ws_ml, part(tid), m, l);
  }
}

// The 16-bit RoPE-and-append kernel, one workgroup per (token t, sequence b): the token's row is at
// qkv + b stride_b + t stride_t, its position is pos[b] + t, q goes to q_out [B, T, nh, D] and k /
// v to cache row pos[b] + t (dec_rope_token). A position outside [0, cap) or the table writes
// nothing. One new token per sequence is T = 1 with stride_b = (nh + 2 nkv) D.
template <typename T>
__global__ __launch_bounds__(256) void decode_rope_append_kernel(
    const T* __restrict__ qkv, int64_t stride_b, int64_t stride_t, T* __restrict__ q_out, T* __restrict__ kc,
    T* __restrict__ vc, const int* __restrict__ pos_t, int nh, int nkv, int D, int cap, int rot,
    const float* __restrict__ cos_t, const float* __restrict__ sin_t, int max_pos, float sign) {
  const int t = blockIdx.x, b = blockIdx.y, Tn = gridDim.x;
  const int64_t pos = (int64_t)pos_t[b] + t;
  if (!dec_pos_ok(pos, cap, rot, max_pos)) return;
  const int64_t row = ((int64_t)b * cap + pos) * nkv * D;
  dec_rope_token(qkv + (int64_t)b * stride_b + (int64_t)t * stride_t, q_out + ((int64_t)b * Tn + t) * nh * D, kc + row,
                 vc + row, pos, nh, nkv, D, rot, cos_t, sin_t, sign);
}

template <typename E, int D>
hipError_t decode_attn_multi_launch(const void* q, const void* kc, const void* vc, const int* lens, float* ws_ml,
                                    float* ws_acc, int B, int Tn, int nh, int nkv, int cap, int nchunks, float scale,
                                    hipStream_t st) {
  const dim3 grid((unsigned)nchunks, (unsigned)nkv, (unsigned)B);
  const int G = nh / nkv;
#define SMDT_DEC_MT(RT)                                                                                     \
  hipLaunchKernelGGL((decode_attn_multi_kernel<E, D, RT>), grid, dim3(kDecThreads), 0, st, (const E*)q,     \
                     (const E*)kc, (const E*)vc, lens, ws_ml, ws_acc, cap, nkv, G, Tn, scale)
  switch ((Tn * G + 15) / 16) {
    case 1: SMDT_DEC_MT(1); break;
    case 2: SMDT_DEC_MT(2); break;
    case 3: SMDT_DEC_MT(3); break;
    case 4: SMDT_DEC_MT(4); break;
    default: return hipErrorInvalidValue;
  }
#undef SMDT_DEC_MT
  return hipGetLastError();
}

}  // namespace smdt

using namespace smdt;

extern "C" int smdt_decode_attn_multi_max_t() { return kDecMultiMaxT; }

extern "C" int smdt_decode_attn_multi_supported(int dtype, int D, int nh, int nkv, int T) {
  return smdt_decode_attn_supported(dtype, D, nh, nkv) && T >= 1 && T <= kDecMultiMaxT;
}

extern "C" hipError_t smdt_decode_attn_multi(int dtype, const void* q, const void* k_cache, const void* v_cache,
                                             const int* lens, float* ws_ml, float* ws_acc, void* out, int B, int T,
                                             int nh, int nkv, int D, int cap, int max_len, float scale,
                                             hipStream_t st) {
  const int nchunks = dec_nchunks(B, nkv, cap, max_len);
  if (!smdt_decode_attn_multi_supported(dtype, D, nh, nkv, T) || (int64_t)T * nh > 65535 || nchunks == 0)
    return hipErrorInvalidValue;
  const hipError_t e = dec_dispatch(dtype, D, [&](auto tag, auto d) {
    return decode_attn_multi_launch<typename decltype(tag)::type, decltype(d)::value>(
        q, k_cache, v_cache, lens, ws_ml, ws_acc, B, T, nh, nkv, cap, nchunks, scale, st);
  });
  if (e != hipSuccess) return e;
  return smdt_decode_attn_combine(dtype, ws_ml, ws_acc, lens, out, B, T * nh, D, cap, nchunks, st);
}

extern "C" hipError_t smdt_decode_rope_append_multi(int dtype, const void* qkv, int64_t stride_b, int64_t stride_t,
                                                    void* q_out, void* k_cache, void* v_cache, const int* pos, int B,
                                                    int T, int nh, int nkv, int D, int cap, int rot,
                                                    const float* cos_t, const float* sin_t, int max_pos,
                                                    hipStream_t st) {
  if (B <= 0 || B > 65535 || T <= 0 || T > kDecMultiMaxT || D % 8 || rot % 16 || rot < 0 || rot > D || cap <= 0 ||
      stride_b % 8 || stride_t % 8 || (rot > 0 && (cos_t == nullptr || sin_t == nullptr || max_pos <= 0)))
    return hipErrorInvalidValue;
  return dec_dispatch(dtype, [&](auto tag) {
    using E = typename decltype(tag)::type;
    hipLaunchKernelGGL(decode_rope_append_kernel<E>, dim3((unsigned)T, (unsigned)B), dim3(256), 0, st, (const E*)qkv,
                       stride_b, stride_t, (E*)q_out, (E*)k_cache, (E*)v_cache, pos, nh, nkv, D, cap, rot, cos_t, sin_t,
                       max_pos, 1.f);
    return hipGetLastError();
  });
}
