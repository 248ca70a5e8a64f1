// Chunked / prefix-cached prefill for gfx950: many new tokens per sequence against a K/V cache that
// already holds a prefix (generate(prefill_chunk=..., cached_prefix=...)).
//
//   smdt_prefill_rope_append  RoPE on the T new tokens' q / k (bitwise rope.hip's, dec_rope_token)
//                             and the append of their k / v into cache rows pos[b] + t, for the
//                             rows below lens[b] only; any T >= 1
//   smdt_prefill_attn         one-pass flash forward of q [B, T, nh, D] over k / v [B, cap, nkv, D]:
//                             query t of sequence b sits at cache row r = pos[b] + t and, if
//                             r < lens[b], attends keys 0 .. r; otherwise it is padding and its
//                             output row is exact zeros. pos = lens - T is decode_attn_multi's
//                             meaning.
//
// decode_common.h states the guarantees these keep: pos / lens stay on the device, no key row at or
// beyond lens[b] is loaded (its slot reads row lens[b] - 1 and gets probability 0), masking is by
// selection, one fixed summation order (bitwise repeatable), no atomics.
//
// Work split. A 256-thread workgroup owns 128 query ROWS of one (sequence, kv head), a row being
// (token t, group member g): row = t G + g with G = nh / nkv. So a block covers 128 / G tokens and
// every K / V byte it stages serves all G query heads of the kv head. Each wave owns 32 rows. The
// grid is ceil(T G / 128) x nkv x B, flattened and dispatched heaviest first: the latest token
// block of every (sequence, kv head) sweeps the most keys and goes out first, then every pair's
// next one (the reasoning of SMDT_FA_ORDER in flash_attn.hip).
//
// Products (mfma_tile.h has the lane maps). S^T = K Q^T on v_mfma_f32_32x32x16: the key is the A
// row, the query the B column, so a lane holds one query row's scores over the keys in its 32
// registers of a 64-key tile, the row's key limit is a per-lane scalar, and the online softmax runs
// in registers: log2 domain with raw v_exp_f32, the row maximum and sum cross the two half-waves
// with v_permlane32_swap. P is rounded to the 16-bit type and is, as it lies, the B operand of
// O^T += V^T P^T, whose A operand ds_read_b64_tr_b16 gathers from the row-major V tile. The running
// maximum m moves on every tile (alpha = exp2(m - m'); l and O^T are rescaled in fp32, l sums the
// unrounded p): the rounding points prefill_attention_ref(emulate=True) places.
//
// Data movement. K / V tiles are 64 keys x D, read from the cache with row stride nkv D by 16-byte
// loads into registers, written to LDS in the swizzled Geo<D> image (both the ds_read_b128 row
// reads and the transposed reads are conflict free at D = 64 and 128) and double-buffered: the
// loads of tile i + 1 are issued before the products of tile i and stored after them, one barrier
// per tile. Q fragments are loaded once per block, straight from global memory in operand layout.
//
// Key sweep. A block sweeps keys 0 .. min(lens[b], pos[b] + its last token + 1). A tile that lies
// wholly below the wave's first row's limit needs no mask: that is the whole cached prefix. Only
// the tiles that straddle the wave's diagonal or lens[b] take the per-lane select (a wave-uniform
// branch), and a wave skips the products of tiles past its last row. A block whose first row is at
// or beyond lens[b] stores zeros and returns; a sequence with no new token is such a block.
//
// Not built: a split of one block's keys over several workgroups (a short chunk on a very long
// prefix at small batch runs on ceil(T G / 128) nkv B workgroups), an MXFP8 cache, dropout, a
// backward.
#include <climits>

#include "decode_common.h"
#include "launchers.h"
#include "mfma_tile.h"

namespace smdt {
namespace pf {

using namespace mt;

constexpr int kBlockRows = 128;      // query rows of a workgroup: 4 waves x 32
constexpr float kLog2e = 1.4426950408889634f;

__device__ __forceinline__ float fexp2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }
__device__ __forceinline__ int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }

// max / sum of x with the value of lane ^ 32: the same query row, the other half of its keys
__device__ __forceinline__ float xhalf_max(float x) {
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float xhalf_sum(float x) {
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// Global -> register -> LDS staging of one 64-key tile of a cache tensor: chunk i of thread tid is
// 16 bytes of tile row rowi[i]; a row at or beyond len is read from row len - 1.
template <int D>
struct KvStage {
  static constexpr int N = kTile * Geo<D>::CH / 256;
  u16x8 v[N];
  template <class E>
  __device__ __forceinline__ void load(const E* base, int64_t row_stride, int kb, int len) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int idx = threadIdx.x + 256 * i, r = idx / Geo<D>::CH, c = idx % Geo<D>::CH;
      const int key = kb + r, kr = key < len ? key : len - 1;
      v[i] = *reinterpret_cast<const u16x8*>(base + (int64_t)kr * row_stride + c * 8);
    }
  }
  __device__ __forceinline__ void store(char* tile) const {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int idx = threadIdx.x + 256 * i, r = idx / Geo<D>::CH, c = idx % Geo<D>::CH;
      *reinterpret_cast<u16x8*>(tile + Geo<D>::off(r, c)) = v[i];
    }
  }
};

// gs = log2(G). Block i of the flat grid runs token block nqb - 1 - i / (nkv B) of pair i % (nkv B).
template <class E, int D>
__global__ __launch_bounds__(256, 2) void prefill_attn_kernel(
    const E* __restrict__ Q, const E* __restrict__ KC, const E* __restrict__ VC, const int* __restrict__ pos_t,
    const int* __restrict__ lens, E* __restrict__ O, int Tn, int nkv, int gs, int cap, int nqb, float scale) {
  using G = Geo<D>;
  __shared__ __attribute__((aligned(16))) char L0[2 * G::TB], L1[2 * G::TB];      // [K | V] x 2

  const int lane = threadIdx.x & 63, h = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int npairs = gridDim.x / nqb;
  const int qb = nqb - 1 - (int)(blockIdx.x / npairs);
  const int pair = blockIdx.x % npairs, b = pair / nkv, kvh = pair - b * nkv;
  const int nh = nkv << gs, R = Tn << gs;              // query rows of this (b, kvh)
  const int len = dec_clamp_len(lens[b], cap);
  const int pos = pos_t[b];

  const int r0 = qb * kBlockRows;                      // the block's first row; r0 < R
  const int rw = r0 + 32 * w;                          // the wave's
  const int my_row = rw + (lane & 31);
  const bool in_range = my_row < R;
  const int row = in_range ? my_row : R - 1;           // a row to load; never stored
  const int t = row >> gs, g = row & ((1 << gs) - 1);
  const int64_t qo = (((int64_t)b * Tn + t) * nh + (kvh << gs) + g) * D;
  // keys this row sees: 0 for padding (a token at or beyond lens[b]) and for a row before key 0
  const int64_t rpos = (int64_t)pos + t;
  const int lim = in_range && rpos < len && rpos >= 0 ? (int)rpos + 1 : 0;
  E* op = O + qo;

  // the block's sweep: keys 0 .. bhi - 1, bhi = min(len, pos + last token + 1)
  const int t_first = r0 >> gs, t_last = (min(r0 + kBlockRows, R) - 1) >> gs;
  const int64_t bhi64 = min64(len, (int64_t)pos + t_last + 1);
  if ((int64_t)pos + t_first >= len || bhi64 <= 0) {   // every row is padding: zeros
    if (in_range) {                                    // lanes l and l ^ 32 share a row: 16-byte pieces 2 i + h
#pragma unroll
      for (int i = 0; i < D / 16; ++i) *reinterpret_cast<u16x8*>(op + 16 * i + 8 * h) = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
    return;
  }
  const int bhi = (int)bhi64;
  const int ntiles = (bhi + kTile - 1) / kTile;
  // the wave's rows: limits wlo (first row) .. whi (last row in range and below lens[b]). A wave
  // whose first row is padding computes nothing; it still stages tiles.
  int wlo = 0, whi = 0;
  if (rw < R && (int64_t)pos + (rw >> gs) < len) {
    const int tl = (min(rw + 32, R) - 1) >> gs;
    wlo = (int)max64(0, (int64_t)pos + (rw >> gs) + 1);
    whi = (int)max64(0, min64(len, (int64_t)pos + tl + 1));
  }
  // a padding lane of a live wave runs unmasked (its column of S^T is its own; never stored)
  const int lim_m = lim > 0 ? lim : INT_MAX;

  const E* Kb = KC + ((int64_t)b * cap * nkv + kvh) * D;
  const E* Vb = VC + ((int64_t)b * cap * nkv + kvh) * D;
  const int64_t rs = (int64_t)nkv * D;

  Frag<D, E> fr;
  fr.init(lane);
  v8_t<E> qf[G::KS];
  {
    const E* qp = Q + qo + 8 * h;
#pragma unroll
    for (int ks = 0; ks < G::KS; ++ks) qf[ks] = *reinterpret_cast<const v8_t<E>*>(qp + 16 * ks);
  }
  const float c2 = scale * kLog2e;                     // scores to the log2 domain; scale > 0

  f32x16 o[G::DT];
#pragma unroll
  for (int dt = 0; dt < G::DT; ++dt) o[dt] = zero16();
  float m = -INFINITY, l = 0.f;

  KvStage<D> sk, sv;
  sk.load(Kb, rs, 0, len);
  sv.load(Vb, rs, 0, len);
  sk.store(L0);
  sv.store(L0 + G::TB);
  __syncthreads();

  for (int it = 0; it < ntiles; ++it) {
    const char* kt = (it & 1) ? L1 : L0;
    char* nxt = (it & 1) ? L0 : L1;
    const char* vt = kt + G::TB;
    const int kb = it * kTile;
    const bool more = it + 1 < ntiles;
    if (more) {
      sk.load(Kb, rs, kb + kTile, len);
      sv.load(Vb, rs, kb + kTile, len);
    }
    if (kb < whi) {
      f32x16 st[2];
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        st[tt] = mfma(fr.rowf(kt, 32 * tt, 0), qf[0], zero16());
#pragma unroll
        for (int ks = 1; ks < G::KS; ++ks) st[tt] = mfma(fr.rowf(kt, 32 * tt, ks), qf[ks], st[tt]);
      }
      if (kb + kTile > wlo) {          // the tile straddles the wave's diagonal or lens[b]
        const int rel = (lim_m - kb > 2 * kTile ? 2 * kTile : lim_m - kb) - 4 * h;
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
          for (int i = 0; i < 16; ++i)
            st[tt][i] = 32 * tt + (i & 3) + 8 * (i >> 2) < rel ? st[tt][i] : -INFINITY;
      }
      float tmax = st[0][0];
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int i = 0; i < 16; ++i) tmax = fmaxf(tmax, st[tt][i]);
      tmax = xhalf_max(tmax) * c2;
      const float mn = fmaxf(m, tmax);
      const float ms = mn == -INFINITY ? 0.f : mn;     // no visible key yet: every p below is exp2(-inf) = 0
      const float alpha = fexp2(m - ms);               // m = -inf: 0, and l = o = 0
      m = mn;
      float rs0 = 0.f, rs1 = 0.f;
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int i = 0; i < 16; i += 2) {
          const float p0 = fexp2(fmaf(st[tt][i], c2, -ms)), p1 = fexp2(fmaf(st[tt][i + 1], c2, -ms));
          rs0 += p0;
          rs1 += p1;
          st[tt][i] = p0;
          st[tt][i + 1] = p1;
        }
      l = l * alpha + xhalf_sum(rs0 + rs1);
      if (__builtin_amdgcn_ballot_w64(alpha != 1.f) != 0) {
#pragma unroll
        for (int dt = 0; dt < G::DT; ++dt) o[dt] *= alpha;
      }
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const v8_t<E> pb = pack8<E>(st[tt], s);
#pragma unroll
          for (int dt = 0; dt < G::DT; ++dt) o[dt] = mfma(fr.trf(vt, 32 * tt, s, dt), pb, o[dt]);
        }
    }
    if (more) {
      sk.store(nxt);
      sv.store(nxt + G::TB);
    }
    __syncthreads();
  }

  // O[row, d] = O^T / l; a padding row (and a row that saw no key) is zeros by selection
  if (in_range) {
    const bool live = lim > 0 && l > 0.f;
    const float inv = live ? 1.f / l : 0.f;
#pragma unroll
    for (int dt = 0; dt < G::DT; ++dt)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        v4_t<E> v4;
#pragma unroll
        for (int j = 0; j < 4; ++j) v4[j] = live ? (E)(o[dt][4 * g4 + j] * inv) : (E)0.f;
        *reinterpret_cast<v4_t<E>*>(op + 32 * dt + 8 * g4 + 4 * h) = v4;
      }
  }
}

// One workgroup per (token t, sequence b), as decode_rope_append_kernel, with the guard of the
// ragged prefill: a token at or beyond lens[b] (padding) writes no cache row and leaves q zeros.
template <typename T>
__global__ __launch_bounds__(256) void prefill_rope_append_kernel(
    const T* __restrict__ qkv, int64_t stride_b, int64_t stride_t, T* __restrict__ q_out, T* __restrict__ kc,
    T* __restrict__ vc, const int* __restrict__ pos_t, const int* __restrict__ lens, int nh, int nkv, int D, int cap,
    int rot, const float* __restrict__ cos_t, const float* __restrict__ sin_t, int max_pos) {
  const int t = blockIdx.x, b = blockIdx.y, Tn = gridDim.x;
  const int64_t pos = (int64_t)pos_t[b] + t;
  T* qd = q_out + ((int64_t)b * Tn + t) * nh * D;
  if (pos >= dec_clamp_len(lens[b], cap) || !dec_pos_ok(pos, cap, rot, max_pos)) {
    for (int i = threadIdx.x; i < nh * D / 8; i += 256)
      *reinterpret_cast<u16x8*>(qd + i * 8) = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
    return;
  }
  const int64_t row = ((int64_t)b * cap + pos) * nkv * D;
  dec_rope_token(qkv + (int64_t)b * stride_b + (int64_t)t * stride_t, qd, kc + row, vc + row, pos, nh, nkv, D, rot,
                 cos_t, sin_t, 1.f);
}

}  // namespace pf
}  // namespace smdt

using namespace smdt;

extern "C" int smdt_prefill_attn_supported(int dtype, int D, int nh, int nkv) {
  return smdt_decode_attn_supported(dtype, D, nh, nkv);
}

extern "C" hipError_t smdt_prefill_attn(int dtype, const void* q, const void* k_cache, const void* v_cache,
                                        const int* pos, const int* lens, void* out, int B, int T, int nh, int nkv,
                                        int D, int cap, float scale, hipStream_t st) {
  if (!smdt_prefill_attn_supported(dtype, D, nh, nkv) || B <= 0 || cap <= 0 || T <= 0 || T > cap || !(scale > 0.f) ||
      ((uintptr_t)q | (uintptr_t)k_cache | (uintptr_t)v_cache | (uintptr_t)out) % 16)
    return hipErrorInvalidValue;
  const int G = nh / nkv, gs = G == 1 ? 0 : G == 2 ? 1 : G == 4 ? 2 : 3;
  const int64_t nqb = ((int64_t)T * G + pf::kBlockRows - 1) / pf::kBlockRows, blocks = nqb * nkv * B;
  if ((int64_t)T * G > INT_MAX || blocks > INT_MAX) return hipErrorInvalidValue;
  return dec_dispatch(dtype, D, [&](auto tag, auto d) {
    using E = typename decltype(tag)::type;
    hipLaunchKernelGGL((pf::prefill_attn_kernel<E, decltype(d)::value>), dim3((unsigned)blocks), dim3(256), 0, st,
                       (const E*)q, (const E*)k_cache, (const E*)v_cache, pos, lens, (E*)out, T, nkv, gs, cap,
                       (int)nqb, scale);
    return hipGetLastError();
  });
}

extern "C" hipError_t smdt_prefill_rope_append(int dtype, const void* qkv, int64_t stride_b, int64_t stride_t,
                                               void* q_out, void* k_cache, void* v_cache, const int* pos,
                                               const int* lens, int B, int T, int nh, int nkv, int D, int cap, int rot,
                                               const float* cos_t, const float* sin_t, int max_pos, hipStream_t st) {
  if (B <= 0 || B > 65535 || T <= 0 || nh <= 0 || nkv <= 0 || D % 8 || rot % 16 || rot < 0 || rot > D || cap <= 0 ||
      stride_b % 8 || stride_t % 8 || (rot > 0 && (cos_t == nullptr || sin_t == nullptr || max_pos <= 0)))
    return hipErrorInvalidValue;
  return dec_dispatch(dtype, [&](auto tag) {
    using E = typename decltype(tag)::type;
    hipLaunchKernelGGL(pf::prefill_rope_append_kernel<E>, dim3((unsigned)T, (unsigned)B), dim3(256), 0, st,
                       (const E*)qkv, stride_b, stride_t, (E*)q_out, (E*)k_cache, (E*)v_cache, pos, lens, nh, nkv, D,
                       cap, rot, cos_t, sin_t, max_pos);
    return hipGetLastError();
  });
}
