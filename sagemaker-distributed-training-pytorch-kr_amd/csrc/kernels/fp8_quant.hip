// FP8 quantisation with delayed (per-tensor) scaling for gfx950, and the scale update that goes
// with it. gfx950 speaks the OCP encodings: E4M3 is torch.float8_e4m3fn (max 448, no inf, NaN =
// 0x7f), E5M2 is torch.float8_e5m2 (max 57344). Not the FNUZ encodings of gfx942.
//
//   q[i] = fp8( clamp(float(x[i]) * scale, -max, max) )     round-to-nearest-even (v_cvt_pk_*_f32)
//   amax = max(amax, max_i |float(x[i])|)                    before scaling, merged atomically
//
// The clamp is written with compares, which keep a NaN (fminf / fmaxf would drop it), so a NaN
// input comes out as an FP8 NaN and +-inf saturates. A NaN is stored as 0x7f | sign in both
// formats, the byte PyTorch's own cast produces. |x| is merged as its bit pattern: non-negative
// floats order as unsigned integers, inf sorts above every finite value and NaN above inf, so a
// non-finite input always leaves a non-finite amax. The merge is a max, so quantising the same
// tensor again (activation recompute) changes nothing.
//
// Two kernels:
//   * fp8_quantize_flat: activations and gradients. A flat stream, 16 elements (two 16-byte
//     loads, one 16-byte store) per lane per iteration, fully coalesced.
//   * fp8_quantize_tile: weights, which the dgrad GEMM also needs transposed (the library wants a
//     K-contiguous second operand). A 16-bit transpose followed by a second quantise would read
//     the tensor twice; here a 64 x 64 tile is converted once, stored as q[M, K] from registers
//     and staged through LDS as bytes (as transpose.hip stages 16-bit elements) for qt[K, M].
//     Both stores are 16-byte vectors when M % 16 == 0; other M take byte stores for qt. The
//     transposed pass reads LDS a byte at a time down a column (row stride 68 bytes), which is
//     bank-conflicted; the kernel runs once per weight per optimizer step (8-18 us at the GPT-2
//     345M shapes, profiles/fp8_linear/README.md), so the simple form is kept.
//
// fp8_update_scales: one launch over the table of every FP8 tensor of a model. Everything stays on
// the device (no host sync), so a captured training step advances its own scales.
#include "common.h"
#include "launchers.h"

namespace smdt {

constexpr int kQT = 64;          // tile edge of the transposing kernel (elements)
constexpr int kQPad = 4;         // LDS row padding in bytes (keeps rows 4-byte aligned)

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

// 16 raw 16-bit elements -> 16 FP8 bytes; returns max |x| of them as a bit pattern.
template <typename T, bool BF8>
__device__ __forceinline__ unsigned quant16(const u16x8& lo, const u16x8& hi, float scale, u32x4& out) {
  constexpr float kMax = fp8_max<BF8>();
  float v[16];
  unsigned am = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const unsigned short bits = j < 8 ? lo[j] : hi[j - 8];
    T t;
    __builtin_memcpy(&t, &bits, 2);
    const float f = to_f32(t);
    const unsigned ab = __float_as_uint(f) & 0x7FFFFFFFu;
    am = ab > am ? ab : am;
    float s = f * scale;
    s = s > kMax ? kMax : s;      // compares are false for NaN: it passes through
    s = s < -kMax ? -kMax : s;
    v[j] = s;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) out[k] = cvt4<BF8>(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
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

// Block-wide max of the bit patterns, merged into *amax by one atomic per block.
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

template <typename T, bool BF8>
__global__ __launch_bounds__(256) void fp8_quantize_flat(const T* __restrict__ x, uint8_t* __restrict__ q,
                                                         const float* __restrict__ scale_p,
                                                         float* __restrict__ amax, int64_t nchunks) {
  __shared__ unsigned red[4];
  const float scale = *scale_p;
  unsigned am = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nchunks; i += (int64_t)gridDim.x * 256) {
    const u16x8* p = reinterpret_cast<const u16x8*>(x + i * 16);
    const u16x8 lo = __builtin_nontemporal_load(p);
    const u16x8 hi = __builtin_nontemporal_load(p + 1);
    u32x4 o;
    const unsigned a = quant16<T, BF8>(lo, hi, scale, o);
    am = a > am ? a : am;
    *reinterpret_cast<u32x4*>(q + i * 16) = o;
  }
  merge_amax(am, red, amax);
}

template <typename T, bool BF8>
__global__ __launch_bounds__(256) void fp8_quantize_tile(const T* __restrict__ x, uint8_t* __restrict__ q,
                                                         uint8_t* __restrict__ qt,
                                                         const float* __restrict__ scale_p,
                                                         float* __restrict__ amax, int M, int K) {
  __shared__ __attribute__((aligned(16))) uint8_t t[kQT][kQT + kQPad];
  __shared__ unsigned red[4];
  const float scale = *scale_p;
  const int r0 = blockIdx.x * kQT, c0 = blockIdx.y * kQT;
  // 64 rows x 4 chunks of 16 elements: one chunk per thread
  const int rr = threadIdx.x >> 2, cv = (threadIdx.x & 3) * 16;
  const int r = r0 + rr, c = c0 + cv;
  unsigned am = 0;
  u32x4 o = {0u, 0u, 0u, 0u};
  if (r < M && c < K) {   // K % 16 == 0: a chunk is either fully inside or fully outside
    const u16x8* p = reinterpret_cast<const u16x8*>(x + (int64_t)r * K + c);
    const u16x8 lo = __builtin_nontemporal_load(p);
    const u16x8 hi = __builtin_nontemporal_load(p + 1);
    am = quant16<T, BF8>(lo, hi, scale, o);
    *reinterpret_cast<u32x4*>(q + (int64_t)r * K + c) = o;
  }
  // rows / columns past the edge hold zeros in LDS and are never stored
#pragma unroll
  for (int k = 0; k < 4; ++k) *reinterpret_cast<unsigned*>(&t[rr][cv + 4 * k]) = o[k];
  __syncthreads();
  // qt row (c0 + cc) holds column cc of the tile: 4 chunks of 16 rows each
  const int cc = threadIdx.x >> 2, rv = (threadIdx.x & 3) * 16;
  const int oc = c0 + cc, orow = r0 + rv;
  if (oc < K && orow < M) {
    uint8_t b[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) b[j] = t[rv + j][cc];
    uint8_t* dst = qt + (int64_t)oc * M + orow;
    if ((M & 15) == 0) {   // rows of qt are 16-byte aligned and a chunk is fully inside
      u32x4 y;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        y[k] = (unsigned)b[4 * k] | ((unsigned)b[4 * k + 1] << 8) | ((unsigned)b[4 * k + 2] << 16) |
               ((unsigned)b[4 * k + 3] << 24);
      *reinterpret_cast<u32x4*>(dst) = y;
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (orow + j < M) dst[j] = b[j];
    }
  }
  merge_amax(am, red, amax);
}

// One thread per FP8 tensor: hist[t, 1:] = hist[t, :-1]; hist[t, 0] = amax[t]; amax[t] = 0;
// a = hist[t, 0] (most_recent) or max(hist[t, :]); scale[t] = (fmt_max[t] / a) / 2^margin, kept
// when a is 0 or not finite (or the quotient overflows).
__global__ void fp8_update_scales_kernel(float* __restrict__ scale, float* __restrict__ hist,
                                         float* __restrict__ amax, const float* __restrict__ fmt_max,
                                         int T, int H, float inv_pow2_margin, int use_max) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  float* h = hist + (int64_t)t * H;
  const float cur = amax[t];
  amax[t] = 0.f;
  unsigned red = __float_as_uint(cur) & 0x7FFFFFFFu;
  for (int i = H - 1; i > 0; --i) {
    const float v = h[i - 1];
    h[i] = v;
    const unsigned b = __float_as_uint(v) & 0x7FFFFFFFu;
    if (use_max) red = b > red ? b : red;   // bit-pattern max: inf / NaN win, as for the amax merge
  }
  h[0] = cur;
  const float a = __uint_as_float(red);
  if (red == 0u || red >= 0x7F800000u) return;
  const float s = (fmt_max[t] / a) * inv_pow2_margin;
  if ((__float_as_uint(s) & 0x7FFFFFFFu) >= 0x7F800000u) return;
  scale[t] = s;
}

template <typename T, bool BF8>
static hipError_t launch_quant(const void* x, void* q, void* qt, const float* scale, float* amax, int64_t M,
                               int64_t K, hipStream_t st) {
  if (qt == nullptr) {
    const int64_t nchunks = M * K / 16;
    hipLaunchKernelGGL((fp8_quantize_flat<T, BF8>), dim3(stream_grid(nchunks, 256)), dim3(256), 0, st,
                       (const T*)x, (uint8_t*)q, scale, amax, nchunks);
  } else {
    const int64_t gx = (M + kQT - 1) / kQT, gy = (K + kQT - 1) / kQT;
    if (gy > 65535 || gx > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL((fp8_quantize_tile<T, BF8>), dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, st,
                       (const T*)x, (uint8_t*)q, (uint8_t*)qt, scale, amax, (int)M, (int)K);
  }
  return hipGetLastError();
}

}  // namespace smdt

using namespace smdt;

extern "C" hipError_t smdt_fp8_quantize(const void* x, void* q, void* qt, const float* scale, float* amax,
                                        int64_t M, int64_t K, int dtype, int bf8, hipStream_t st) {
  if (M < 1 || K < 16 || K % 16 != 0 || M > (1 << 30) || K > (1 << 30)) return hipErrorInvalidValue;
  if (dtype == (int)DType::kBF16)
    return bf8 ? launch_quant<bf16, true>(x, q, qt, scale, amax, M, K, st)
               : launch_quant<bf16, false>(x, q, qt, scale, amax, M, K, st);
  if (dtype == (int)DType::kF16)
    return bf8 ? launch_quant<f16, true>(x, q, qt, scale, amax, M, K, st)
               : launch_quant<f16, false>(x, q, qt, scale, amax, M, K, st);
  return hipErrorInvalidValue;
}

extern "C" hipError_t smdt_fp8_update_scales(float* scale, float* hist, float* amax, const float* fmt_max,
                                             int64_t T, int64_t H, int margin, int use_max, hipStream_t st) {
  if (T < 1 || H < 1 || T > (1 << 24) || H > (1 << 16) || margin < 0 || margin > 64) return hipErrorInvalidValue;
  const float inv = __builtin_ldexpf(1.f, -margin);
  hipLaunchKernelGGL(fp8_update_scales_kernel, dim3((unsigned)((T + 127) / 128)), dim3(128), 0, st, scale, hist,
                     amax, fmt_max, (int)T, (int)H, inv, use_max);
  return hipGetLastError();
}
