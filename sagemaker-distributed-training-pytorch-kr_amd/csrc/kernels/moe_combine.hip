// Rows out of the expert-sorted, tile-padded layout of moe_route.hip and back into it when a token
// owns k rows (--moe-router-topk with --moe-grouped-gemm). y / dys are [R, h] in that layout,
// out / dout [T, h] per token, row_of_token int32 [T, k], token_of_row int64 [R] (-1 on pad rows),
// p_of_row fp32 [R] (0 on pad rows). 16-bit elements, h a multiple of 8, k <= 8.
//
//   combine_fwd     out[t] = sum_j w[t, j] * y[row_of_token[t, j]]: the k rows of a token are read
//                   with k independent 16-byte loads per lane (all issued before the first add),
//                   accumulated in fp32 in slot order and rounded once. w null: weights of 1, the
//                   dx combine of the backward. Replaces k index_selects, a multiply and a sum.
//   scatter_scaled  dys[r] = p_of_row[r] * dout[token_of_row[r]], zeros on pad rows: a gather in
//                   the destination's order, so every row of dys is written exactly once (no zero
//                   fill, no scatter; gather_rows_kernel's scheme with the gate weight folded in).
//   gate_grad       dp[t, j] = <dout[t], y[row_of_token[t, j]]> in fp32: one wave per token keeps
//                   dout[t] in registers (2048 elements at a time) across the k dot products, the
//                   lane partials meet in a shuffle butterfly. No atomics: bitwise repeatable.
//
// Work split: combine_fwd and scatter_scaled give one wave a (row, 512-element chunk) item, a lane
// 8 elements of it; the wave index is made uniform with readfirstlane so the k row indices and
// gate weights of the item are scalar loads. No LDS: every element is touched by one lane only.
#include "common.h"
#include "launchers.h"

namespace smdt {
namespace moec {

constexpr int kWaves = 8;        // waves (items) per block of combine_fwd / scatter_scaled
constexpr int kChunk = 512;      // elements of a row per wave: 64 lanes x 16 bytes
constexpr int kGateWaves = 4;    // tokens per block of gate_grad
constexpr int kGateChunks = 4;   // chunks of dout[t] a lane holds at a time (16 registers)

template <class T>
__device__ __forceinline__ void cvt8(const u16x8& v, float (&f)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const unsigned short bits = v[i];
    T x;
    __builtin_memcpy(&x, &bits, 2);
    f[i] = to_f32(x);
  }
}

template <class T, int K, bool W>
__global__ __launch_bounds__(kWaves * 64) void combine_fwd_kernel(const T* __restrict__ y,
                                                                  const int* __restrict__ row_of_token,
                                                                  const float* __restrict__ w, T* __restrict__ out,
                                                                  int64_t items, int64_t chunks, int64_t h, int R) {
  const int64_t item = (int64_t)blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (item >= items) return;
  const int64_t t = item / chunks;
  const int64_t off = (item - t * chunks) * kChunk + (int64_t)(threadIdx.x & 63) * 8;
  int r[K];
  float g[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    r[j] = row_of_token[t * K + j];
    g[j] = W ? w[t * K + j] : 1.f;
  }
  if (off >= h) return;
  u16x8 v[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    v[j] = u16x8{};
    if (r[j] >= 0 && r[j] < R) v[j] = *reinterpret_cast<const u16x8*>(y + (int64_t)r[j] * h + off);
  }
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < K; ++j) {
    float f[8];
    cvt8<T>(v[j], f);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = W ? fmaf(g[j], f[i], acc[i]) : acc[i] + f[i];
  }
  store_vec<T, 8>(out + t * h + off, acc);
}

template <class T>
__global__ __launch_bounds__(kWaves * 64) void scatter_scaled_kernel(const T* __restrict__ dout,
                                                                     const int64_t* __restrict__ token_of_row,
                                                                     const float* __restrict__ p_of_row,
                                                                     T* __restrict__ dys, int64_t items,
                                                                     int64_t chunks, int64_t h, int64_t Tn) {
  const int64_t item = (int64_t)blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (item >= items) return;
  const int64_t r = item / chunks;
  const int64_t off = (item - r * chunks) * kChunk + (int64_t)(threadIdx.x & 63) * 8;
  const int64_t s = token_of_row[r];
  const float p = p_of_row[r];
  if (off >= h) return;
  T* dst = dys + r * h + off;
  if (s < 0 || s >= Tn) {     // a pad row: zeros
    *reinterpret_cast<u16x8*>(dst) = u16x8{};
    return;
  }
  float f[8];
  cvt8<T>(__builtin_nontemporal_load(reinterpret_cast<const u16x8*>(dout + s * h + off)), f);
#pragma unroll
  for (int i = 0; i < 8; ++i) f[i] *= p;
  store_vec<T, 8>(dst, f);
}

template <class T, int K>
__global__ __launch_bounds__(kGateWaves * 64) void gate_grad_kernel(const T* __restrict__ dout, const T* __restrict__ y,
                                                                    const int* __restrict__ row_of_token,
                                                                    float* __restrict__ dp, int64_t Tn, int64_t h,
                                                                    int R) {
  const int64_t t = (int64_t)blockIdx.x * kGateWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (t >= Tn) return;
  const int lane = threadIdx.x & 63;
  int r[K];
  float acc[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    r[j] = row_of_token[t * K + j];
    acc[j] = 0.f;
  }
  const T* drow = dout + t * h;
  for (int64_t base = 0; base < h; base += kGateChunks * kChunk) {
    float d[kGateChunks][8];
#pragma unroll
    for (int c = 0; c < kGateChunks; ++c) {
      const int64_t off = base + c * kChunk + lane * 8;
      u16x8 v = {};
      if (off < h) v = *reinterpret_cast<const u16x8*>(drow + off);
      cvt8<T>(v, d[c]);
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
      if (r[j] < 0 || r[j] >= R) continue;
      const T* yrow = y + (int64_t)r[j] * h;
      u16x8 v[kGateChunks];
#pragma unroll
      for (int c = 0; c < kGateChunks; ++c) {
        const int64_t off = base + c * kChunk + lane * 8;
        v[c] = u16x8{};
        if (off < h) v[c] = *reinterpret_cast<const u16x8*>(yrow + off);
      }
#pragma unroll
      for (int c = 0; c < kGateChunks; ++c) {
        float f[8];
        cvt8<T>(v[c], f);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[j] = fmaf(d[c][i], f[i], acc[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < K; ++j) acc[j] = wave_sum(acc[j]);
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < K; ++j) dp[t * K + j] = acc[j];
  }
}

// one launch per k = 1 .. 8
#define SMDT_MOEC_K(k, CALL)   \
  switch (k) {                 \
    case 1: CALL(1); break;    \
    case 2: CALL(2); break;    \
    case 3: CALL(3); break;    \
    case 4: CALL(4); break;    \
    case 5: CALL(5); break;    \
    case 6: CALL(6); break;    \
    case 7: CALL(7); break;    \
    default: CALL(8); break;   \
  }

template <class T>
hipError_t combine_fwd(const void* y, const int* row_of_token, const float* w, void* out, int64_t Tn, int64_t R,
                       int64_t h, int k, hipStream_t st) {
  const int64_t chunks = (h + kChunk - 1) / kChunk, items = Tn * chunks;
  const int64_t blocks = (items + kWaves - 1) / kWaves;
  if (blocks > 0x7FFFFFFF) return hipErrorInvalidValue;
#define SMDT_CALL(KK)                                                                                              \
  if (w)                                                                                                           \
    hipLaunchKernelGGL((combine_fwd_kernel<T, KK, true>), dim3((unsigned)blocks), dim3(kWaves * 64), 0, st,        \
                       (const T*)y, row_of_token, w, (T*)out, items, chunks, h, (int)R);                           \
  else                                                                                                             \
    hipLaunchKernelGGL((combine_fwd_kernel<T, KK, false>), dim3((unsigned)blocks), dim3(kWaves * 64), 0, st,       \
                       (const T*)y, row_of_token, w, (T*)out, items, chunks, h, (int)R)
  SMDT_MOEC_K(k, SMDT_CALL)
#undef SMDT_CALL
  return hipGetLastError();
}

template <class T>
hipError_t gate_grad(const void* dout, const void* y, const int* row_of_token, float* dp, int64_t Tn, int64_t R,
                     int64_t h, int k, hipStream_t st) {
  const int64_t blocks = (Tn + kGateWaves - 1) / kGateWaves;
#define SMDT_CALL(KK)                                                                                          \
  hipLaunchKernelGGL((gate_grad_kernel<T, KK>), dim3((unsigned)blocks), dim3(kGateWaves * 64), 0, st,          \
                     (const T*)dout, (const T*)y, row_of_token, dp, Tn, h, (int)R)
  SMDT_MOEC_K(k, SMDT_CALL)
#undef SMDT_CALL
  return hipGetLastError();
}

}  // namespace moec
}  // namespace smdt

using namespace smdt;

extern "C" int smdt_moe_combine_supported(int dtype, int64_t T, int64_t R, int64_t h, int k) {
  return (dtype == 1 || dtype == 2) && T > 0 && R > 0 && h > 0 && h % 8 == 0 && k >= 1 && k <= 8 &&
         T * k < (1ll << 31) && R < (1ll << 31);
}

extern "C" hipError_t smdt_moe_combine_fwd(int dtype, const void* y, const int* row_of_token, const float* w,
                                           void* out, int64_t T, int64_t R, int64_t h, int k, hipStream_t st) {
  if (!smdt_moe_combine_supported(dtype, T, R, h, k)) return hipErrorInvalidValue;
  return dtype == 1 ? moec::combine_fwd<bf16>(y, row_of_token, w, out, T, R, h, k, st)
                    : moec::combine_fwd<f16>(y, row_of_token, w, out, T, R, h, k, st);
}

extern "C" hipError_t smdt_moe_scatter_scaled(int dtype, const void* dout, const int64_t* token_of_row,
                                              const float* p_of_row, void* dys, int64_t T, int64_t R, int64_t h,
                                              hipStream_t st) {
  if (!smdt_moe_combine_supported(dtype, T, R, h, 1)) return hipErrorInvalidValue;
  const int64_t chunks = (h + moec::kChunk - 1) / moec::kChunk, items = R * chunks;
  const int64_t blocks = (items + moec::kWaves - 1) / moec::kWaves;
  if (blocks > 0x7FFFFFFF) return hipErrorInvalidValue;
  if (dtype == 1)
    hipLaunchKernelGGL(moec::scatter_scaled_kernel<bf16>, dim3((unsigned)blocks), dim3(moec::kWaves * 64), 0, st,
                       (const bf16*)dout, token_of_row, p_of_row, (bf16*)dys, items, chunks, h, T);
  else
    hipLaunchKernelGGL(moec::scatter_scaled_kernel<f16>, dim3((unsigned)blocks), dim3(moec::kWaves * 64), 0, st,
                       (const f16*)dout, token_of_row, p_of_row, (f16*)dys, items, chunks, h, T);
  return hipGetLastError();
}

extern "C" hipError_t smdt_moe_gate_grad(int dtype, const void* dout, const void* y, const int* row_of_token,
                                         float* dp, int64_t T, int64_t R, int64_t h, int k, hipStream_t st) {
  if (!smdt_moe_combine_supported(dtype, T, R, h, k)) return hipErrorInvalidValue;
  return dtype == 1 ? moec::gate_grad<bf16>(dout, y, row_of_token, dp, T, R, h, k, st)
                    : moec::gate_grad<f16>(dout, y, row_of_token, dp, T, R, h, k, st);
}
