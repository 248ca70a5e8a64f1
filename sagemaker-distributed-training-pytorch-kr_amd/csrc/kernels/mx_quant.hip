// OCP MX quantisation for gfx950 (--fp8-recipe mxfp8): one-byte elements (E4M3 = float8_e4m3fn or
// E5M2 = float8_e5m2, the OCP encodings) with one E8M0 scale byte (bias 127) per block of 32
// elements along the contraction dimension. Per block:
//
//   a = max |v| over the block's finite values
//   e = clamp(floor(log2 a) - emax, -127, 127)     emax = 8 (E4M3) / 15 (E5M2); e = 0 when a == 0
//   s = e + 127                                    (never 255, the E8M0 NaN)
//   q = fp8(clamp(v * 2^-e, -max, max))            round-to-nearest-even (v_cvt_pk_*_f32)
//
// floor(log2 a) is the exponent field of the fp32 a minus 127 (an fp32 subnormal a, which only a
// bf16 subnormal gives, reads -127 and clamps to e = -127 like its true value would), and 2^-e is
// built from its exponent field (127 - e is in [8, 254]), so v * 2^-e is one exact fp32 multiply
// wherever the result can round to a non-zero FP8 value. The clamp is written with compares, which
// keep a NaN: a NaN comes out as the byte 0x7f | sign (what fp8_quant.hip and PyTorch's cast
// write), +-inf saturates, and neither enters a. ops/functional.py's mx_quantize_ref is the twin;
// the kernels match it byte for byte.
//
// Two kernels:
//   * mx_quantize_rows: x [M, K] -> q [M, K], s [M, K / 32]. One lane per block: four 16-byte
//     loads, two 16-byte stores and the scale byte.
//   * mx_quantize_tile: x [R, C] -> qT [C, R], sT [C, R / 32] with the blocks along R (the
//     quantisation of the transpose: the block direction differs from the row form, so the bytes
//     differ too), and with ROWS also the row form of the same tile, so a weight is read once
//     for both. A 64 x 64 tile is staged through LDS as raw 16-bit elements, as fp8_quant.hip's
//     weight form stages bytes; the column pass reads LDS down a column (bank-conflicted), and
//     runs once per weight per optimizer step, so the simple form is kept.
#include "common.h"
#include "launchers.h"
#include "mx_quant.h"

namespace smdt {
namespace mxq {

constexpr int kQT = 64;    // tile edge of the transposing kernel (elements)
constexpr int kPad = 2;    // LDS row padding in 16-bit elements (rows stay 4-byte aligned)

template <typename T, bool BF8>
__global__ __launch_bounds__(256) void mx_quantize_rows(const T* __restrict__ x, uint8_t* __restrict__ q,
                                                        uint8_t* __restrict__ s, int64_t nblocks) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nblocks; i += (int64_t)gridDim.x * 256) {
    const u16x8* p = reinterpret_cast<const u16x8*>(x + i * 32);
    float f[2][16];
    unsigned am = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const u16x8 lo = __builtin_nontemporal_load(p + 2 * h);
      const u16x8 hi = __builtin_nontemporal_load(p + 2 * h + 1);
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        f[h][j] = raw_to_f32<T>(j < 8 ? lo[j] : hi[j - 8]);
        const unsigned ab = finite_abs_bits(f[h][j]);
        am = ab > am ? ab : am;
      }
    }
    const int e = block_exp<BF8>(am);
    const float mult = pow2_neg(e);
    u32x4* o = reinterpret_cast<u32x4*>(q + i * 32);
    o[0] = quant16<BF8>(f[0], mult);
    o[1] = quant16<BF8>(f[1], mult);
    s[i] = (uint8_t)(e + 127);
  }
}

// R % 32 == 0, C % 16 == 0 (C % 32 == 0 with ROWS). Thread pairs (lanes 2p, 2p + 1) share a block
// in both passes; the tile's edge cuts between pairs, never inside one.
template <typename T, bool BF8, bool ROWS>
__global__ __launch_bounds__(256) void mx_quantize_tile(const T* __restrict__ x, uint8_t* __restrict__ q,
                                                        uint8_t* __restrict__ s, uint8_t* __restrict__ qt,
                                                        uint8_t* __restrict__ st, int R, int C) {
  __shared__ __attribute__((aligned(16))) unsigned short t[kQT][kQT + kPad];
  const int r0 = blockIdx.x * kQT, c0 = blockIdx.y * kQT;
  // 64 rows x 4 chunks of 16 elements: one chunk per thread
  const int rr = threadIdx.x >> 2, cv = (threadIdx.x & 3) * 16;
  const int r = r0 + rr, c = c0 + cv;
  const bool in = r < R && c < C;   // C % 16 == 0: a chunk is fully inside or fully outside
  u16x8 lo = {0, 0, 0, 0, 0, 0, 0, 0}, hi = lo;
  if (in) {
    const u16x8* p = reinterpret_cast<const u16x8*>(x + (int64_t)r * C + c);
    lo = __builtin_nontemporal_load(p);
    hi = __builtin_nontemporal_load(p + 1);
  }
  // rows / columns past the edge hold zeros in LDS and are never stored
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    *reinterpret_cast<unsigned*>(&t[rr][cv + 2 * k]) = (unsigned)lo[2 * k] | ((unsigned)lo[2 * k + 1] << 16);
    *reinterpret_cast<unsigned*>(&t[rr][cv + 8 + 2 * k]) = (unsigned)hi[2 * k] | ((unsigned)hi[2 * k + 1] << 16);
  }
  if constexpr (ROWS) {
    float f[16];
    unsigned am = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      f[j] = raw_to_f32<T>(j < 8 ? lo[j] : hi[j - 8]);
      const unsigned ab = finite_abs_bits(f[j]);
      am = ab > am ? ab : am;
    }
    const unsigned other = (unsigned)__shfl_xor((int)am, 1, kWave);   // the block's other half
    am = other > am ? other : am;
    const int e = block_exp<BF8>(am);
    if (in) {
      *reinterpret_cast<u32x4*>(q + (int64_t)r * C + c) = quant16<BF8>(f, pow2_neg(e));
      if (!(threadIdx.x & 1)) s[(int64_t)r * (C / 32) + c / 32] = (uint8_t)(e + 127);
    }
  }
  __syncthreads();
  // qT row (c0 + cc) holds column cc of the tile: 4 chunks of 16 rows, two chunks to a block
  const int cc = threadIdx.x >> 2, rv = (threadIdx.x & 3) * 16;
  const int oc = c0 + cc, orow = r0 + rv;
  float f[16];
  unsigned am = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    f[j] = raw_to_f32<T>(t[rv + j][cc]);
    const unsigned ab = finite_abs_bits(f[j]);
    am = ab > am ? ab : am;
  }
  const unsigned other = (unsigned)__shfl_xor((int)am, 1, kWave);
  am = other > am ? other : am;
  const int e = block_exp<BF8>(am);
  if (oc < C && orow < R) {   // R % 32 == 0: 16-byte aligned, fully inside
    *reinterpret_cast<u32x4*>(qt + (int64_t)oc * R + orow) = quant16<BF8>(f, pow2_neg(e));
    if (!(threadIdx.x & 1)) st[(int64_t)oc * (R / 32) + orow / 32] = (uint8_t)(e + 127);
  }
}

template <typename T, bool BF8>
static hipError_t launch(const void* x, void* q, void* s, void* qt, void* st, int64_t R, int64_t C, hipStream_t stream) {
  if (qt == nullptr) {
    const int64_t nblocks = R * C / 32;
    hipLaunchKernelGGL((mx_quantize_rows<T, BF8>), dim3(stream_grid(nblocks, 256)), dim3(256), 0, stream,
                       (const T*)x, (uint8_t*)q, (uint8_t*)s, nblocks);
    return hipGetLastError();
  }
  const int64_t gx = (R + kQT - 1) / kQT, gy = (C + kQT - 1) / kQT;
  if (gy > 65535 || gx > 0x7FFFFFFF) return hipErrorInvalidValue;
  const dim3 grid((unsigned)gx, (unsigned)gy);
  if (q != nullptr)
    hipLaunchKernelGGL((mx_quantize_tile<T, BF8, true>), grid, dim3(256), 0, stream, (const T*)x, (uint8_t*)q,
                       (uint8_t*)s, (uint8_t*)qt, (uint8_t*)st, (int)R, (int)C);
  else
    hipLaunchKernelGGL((mx_quantize_tile<T, BF8, false>), grid, dim3(256), 0, stream, (const T*)x,
                       (uint8_t*)nullptr, (uint8_t*)nullptr, (uint8_t*)qt, (uint8_t*)st, (int)R, (int)C);
  return hipGetLastError();
}

}  // namespace mxq
}  // namespace smdt

using namespace smdt;

// Row form (q, s), column form (qt, st), or both in one launch. Row form: C % 32 == 0; column form:
// R % 32 == 0 and C % 16 == 0.
extern "C" hipError_t smdt_mx_quantize(const void* x, void* q, void* s, void* qt, void* st, int64_t R, int64_t C,
                                       int dtype, int bf8, hipStream_t stream) {
  if (R < 1 || C < 1 || R > (1 << 30) || C > (1 << 30)) return hipErrorInvalidValue;
  const bool rows = q != nullptr, cols = qt != nullptr;
  if ((!rows && !cols) || (rows && !s) || (cols && !st)) return hipErrorInvalidValue;
  if (rows && C % 32 != 0) return hipErrorInvalidValue;
  if (cols && (R % 32 != 0 || C % 16 != 0)) return hipErrorInvalidValue;
  if (dtype == (int)DType::kBF16)
    return bf8 ? mxq::launch<bf16, true>(x, q, s, qt, st, R, C, stream) : mxq::launch<bf16, false>(x, q, s, qt, st, R, C, stream);
  if (dtype == (int)DType::kF16)
    return bf8 ? mxq::launch<f16, true>(x, q, s, qt, st, R, C, stream) : mxq::launch<f16, false>(x, q, s, qt, st, R, C, stream);
  return hipErrorInvalidValue;
}
