// Weight-streaming linear for decode steps on gfx950: out[M, N] = x[M, K] . W[N, K]^T (+ bias[N])
// with M <= 16 rows of activations. The work is reading W once; the kernel is built so that every
// weight byte is loaded exactly once per launch, straight into registers.
//
// W comes in one of three forms (one template, one code path):
//   native  the 16-bit parameter itself, [N, K]
//   mxfp8   E4M3 bytes [N, K] + one E8M0 scale byte per 32 elements along K, [N, K / 32]
//           (the row form of mx_quant.hip)
//   mxfp4   E2M1 nibbles [N, K / 2], element 2j in the low nibble of byte j, scales as for mxfp8
// The quantised forms are dequantised in registers to bf16 by gfx950's scaled pack conversions
// (v_cvt_scalef32_pk_bf16_fp8 / _fp4). A 3-bit (1-bit) mantissa times a power of two is exact in
// bf16, so the kernel computes what a bf16 linear over dequant(quant(W)) computes, up to the
// summation order. fp16 cannot hold the small blocks: the quantised forms take bf16 only.
//
// Decomposition. A workgroup (4 waves) owns kDlRows = 16 rows of W, i.e. 16 output columns, and a
// K slice [ks, ke). The products go on the 16x16x32 MFMA with the 16 W rows as the A side and the
// batch as the 16-wide B side; this one form serves every M (batch lanes m >= M read row M - 1 of
// x instead of a row that is not there, and their output column is never stored, so what they
// hold does not matter). The contraction index of an MFMA is permuted: lane (r = lane & 15,
// g = lane >> 4) takes ONE 16-byte load of row r, a "chunk" of CH = 8 / 16 / 32 consecutive
// elements (native / mxfp8 / mxfp4; for mxfp4 exactly one scale block), and feeds CH / 8 MFMAs
// from it; its x fragment holds the same CH elements of batch row r. In one step the four g
// lanes of a row read 64 contiguous bytes and the four waves 256; kDlUnroll steps are issued
// before the first is used (loads are asynchronous until their wait; no LDS round trip for W).
// A chunk index beyond the slice reads the slice's last chunk instead (so the unrolled loads stay
// unconditional) with its x fragment selected to zero. W rows n >= N read row N - 1 and are not
// stored. The four waves' accumulators meet in LDS and are summed in wave order.
//
// Split K: when ceil(N / 16) workgroups would leave CUs idle (fewer than kDlSplitBelow), K is cut
// into S slices (multiples of the workgroup's k per step); slice s writes its fp32 partial to
// ws[s, M, N] (caller's workspace) and a second launch sums the slices in index order and adds the
// bias. No atomics: the result is bitwise repeatable. With S = 1 the first launch adds the bias in
// fp32 and rounds once.
//
// Limits (smdt_decode_linear_supported is the single place they live): 1 <= M <= 16, N a multiple
// of 8, K a multiple of 32, bf16 or fp16 (native) / bf16 (mxfp8, mxfp4).
#include "common.h"
#include "launchers.h"

namespace smdt {
namespace dl {

constexpr int kDlRows = 16;          // W rows per workgroup (one MFMA tile)
constexpr int kDlMaxM = 16;          // batch rows: the other 16-wide side of the MFMA
constexpr int kDlWaves = 4;
constexpr int kDlThreads = kDlWaves * kWave;
constexpr int kDlSplitBelow = 256;   // fewer workgroups than this over N: split K
constexpr int kDlMaxSplits = 16;

constexpr int chunk_elems(int fmt) { return fmt == 0 ? 8 : (fmt == 1 ? 16 : 32); }   // per 16-byte load
constexpr int step_k(int fmt) { return kDlWaves * 4 * chunk_elems(fmt); }            // per workgroup step
constexpr int unroll(int fmt) { return fmt == 2 ? 4 : 8; }

using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;

__device__ __forceinline__ f32x4 mma(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mma(f16x8 a, f16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// 2^(s - 127) for an E8M0 byte s (0: the fp32 subnormal 2^-127; 255, the E8M0 NaN: NaN).
__device__ __forceinline__ float e8m0_to_f32(unsigned s) {
  return __uint_as_float(s == 0u ? 0x00400000u : (s == 255u ? 0x7FC00000u : s << 23));
}

// Elements 8 i .. 8 i + 7 of a 16-byte chunk as a bf16 MFMA fragment.
template <int FMT>
__device__ __forceinline__ bf16x8 dequant8(const u32x4& q, int i, float scale) {
  bf16x2 p[4];
  if constexpr (FMT == 1) {        // bytes 8 i .. 8 i + 7: words 2 i and 2 i + 1, two bytes a convert
    p[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q[2 * i], scale, false);
    p[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q[2 * i], scale, true);
    p[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q[2 * i + 1], scale, false);
    p[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q[2 * i + 1], scale, true);
  } else {                         // nibbles 8 i .. 8 i + 7: word i, one byte (low nibble first) a convert
    p[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q[i], scale, 0);
    p[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q[i], scale, 1);
    p[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q[i], scale, 2);
    p[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q[i], scale, 3);
  }
  bf16x8 a;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    a[2 * j] = p[j][0];
    a[2 * j + 1] = p[j][1];
  }
  return a;
}

template <typename T, int FMT>
__global__ __launch_bounds__(kDlThreads) void decode_linear_kernel(
    const T* __restrict__ x, const uint8_t* __restrict__ w, const uint8_t* __restrict__ sc,
    const T* __restrict__ bias, T* __restrict__ out, float* __restrict__ ws, int M, int N, int K, int slice) {
  constexpr int CH = chunk_elems(FMT);
  constexpr int U = unroll(FMT);
  constexpr int NM = CH / 8;                    // MFMAs fed by one chunk
  using Frag = typename std::conditional<std::is_same<T, bf16>::value, bf16x8, f16x8>::type;
  static_assert(FMT == 0 || std::is_same<T, bf16>::value, "the quantised forms dequantise to bf16");

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * kDlRows;
  const int ks = blockIdx.y * slice;
  const int ke = ks + slice < K ? ks + slice : K;
  const int nchunks = (ke - ks) / CH;           // K % 32 == 0 and slice % step_k == 0: whole chunks
  const int nrow = n0 + r < N ? n0 + r : N - 1;
  const int mrow = r < M ? r : M - 1;
  // bytes per element of W: 2 / 1 / one half
  const int64_t row_bytes = FMT == 0 ? (int64_t)K * 2 : (FMT == 1 ? (int64_t)K : (int64_t)K / 2);
  const uint8_t* wrow = w + (int64_t)nrow * row_bytes;
  const uint8_t* srow = FMT == 0 ? nullptr : sc + (int64_t)nrow * (K / 32);
  const T* xrow = x + (int64_t)mrow * K;

  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int c0 = 0; c0 < nchunks; c0 += U * kDlWaves * 4) {
    u32x4 wq[U];
    u32x4 xq[U][NM];
    unsigned sb[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int c = c0 + (u * kDlWaves + wv) * 4 + g;
      ok[u] = c < nchunks;
      const int k = ks + (ok[u] ? c : nchunks - 1) * CH;
      wq[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wrow + (int64_t)k * 16 / CH));
      if constexpr (FMT != 0) sb[u] = srow[k >> 5];
#pragma unroll
      for (int i = 0; i < NM; ++i) xq[u][i] = *reinterpret_cast<const u32x4*>(xrow + k + 8 * i);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float scale = 1.f;
      if constexpr (FMT != 0) scale = e8m0_to_f32(sb[u]);
#pragma unroll
      for (int i = 0; i < NM; ++i) {
        const u32x4 zero = {0u, 0u, 0u, 0u};
        const Frag b = __builtin_bit_cast(Frag, ok[u] ? xq[u][i] : zero);
        Frag a;
        if constexpr (FMT == 0) a = __builtin_bit_cast(Frag, wq[u]);
        else a = dequant8<FMT>(wq[u], i, scale);
        acc = mma(a, b, acc);
      }
    }
  }

  // the four waves' tiles, summed in wave order by wave 0
  __shared__ f32x4 red[kDlWaves][kWave];
  red[wv][lane] = acc;
  __syncthreads();
  if (wv != 0) return;
  f32x4 s = red[0][lane];
#pragma unroll
  for (int v = 1; v < kDlWaves; ++v) s += red[v][lane];
  // accumulator element e of lane (r, g): W row n0 + 4 g + e, batch row r
  const int n = n0 + 4 * g;
  if (r >= M || n >= N) return;                 // N % 8 == 0: four columns are all inside or all outside
  if (ws != nullptr) {
    *reinterpret_cast<f32x4*>(ws + ((int64_t)blockIdx.y * M + r) * N + n) = s;
    return;
  }
  T o[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = from_f32<T>(bias != nullptr ? s[e] + to_f32(bias[n + e]) : s[e]);
  uint2 pk;
  __builtin_memcpy(&pk, o, 8);
  *reinterpret_cast<uint2*>(out + (int64_t)r * N + n) = pk;
}

// out[m, n] = sum_s ws[s, m, n] (+ bias[n]), slices in index order; four columns per thread.
template <typename T>
__global__ __launch_bounds__(256) void decode_linear_combine_kernel(const float* __restrict__ ws,
                                                                    const T* __restrict__ bias, T* __restrict__ out,
                                                                    int64_t MN, int N, int S) {
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= MN) return;
  f32x4 s = *reinterpret_cast<const f32x4*>(ws + i);
  for (int k = 1; k < S; ++k) s += *reinterpret_cast<const f32x4*>(ws + (int64_t)k * MN + i);
  const int n = (int)(i % N);
  T o[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = from_f32<T>(bias != nullptr ? s[e] + to_f32(bias[n + e]) : s[e]);
  uint2 pk;
  __builtin_memcpy(&pk, o, 8);
  *reinterpret_cast<uint2*>(out + i) = pk;
}

inline int step_k_rt(int fmt) { return fmt == 0 ? step_k(0) : (fmt == 1 ? step_k(1) : step_k(2)); }

// (splits, slice length): one slice unless N alone leaves CUs idle; slices are multiples of the
// workgroup's k per step.
inline void plan(int N, int K, int fmt, int* splits, int* slice) {
  const int step = step_k_rt(fmt);
  const int nwg = (N + kDlRows - 1) / kDlRows;
  int S = 1;
  if (nwg < kDlSplitBelow) {
    S = (kDlSplitBelow + nwg - 1) / nwg;
    const int most = K / step > 1 ? K / step : 1;
    S = S > most ? most : S;
    S = S > kDlMaxSplits ? kDlMaxSplits : S;
  }
  int sl = (K + S - 1) / S;
  sl = (sl + step - 1) / step * step;
  *slice = sl;
  *splits = (K + sl - 1) / sl;
}

template <typename T, int FMT>
hipError_t launch(const void* x, const void* w, const void* sc, const void* bias, void* out, float* ws, int M,
                  int N, int K, hipStream_t st) {
  int S, slice;
  plan(N, K, FMT, &S, &slice);
  if (S > 1 && ws == nullptr) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((N + kDlRows - 1) / kDlRows), (unsigned)S);
  hipLaunchKernelGGL((decode_linear_kernel<T, FMT>), grid, dim3(kDlThreads), 0, st, (const T*)x, (const uint8_t*)w,
                     (const uint8_t*)sc, (const T*)bias, (T*)out, S > 1 ? ws : nullptr, M, N, K, slice);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || S == 1) return e;
  const int64_t MN = (int64_t)M * N;
  hipLaunchKernelGGL(decode_linear_combine_kernel<T>, dim3((unsigned)((MN / 4 + 255) / 256)), dim3(256), 0, st, ws,
                     (const T*)bias, (T*)out, MN, N, S);
  return hipGetLastError();
}

}  // namespace dl
}  // namespace smdt

using namespace smdt;

extern "C" int smdt_decode_linear_rows() { return dl::kDlRows; }
extern "C" int smdt_decode_linear_max_m() { return dl::kDlMaxM; }
extern "C" int smdt_decode_linear_split_below() { return dl::kDlSplitBelow; }
extern "C" int smdt_decode_linear_step_k(int fmt) { return fmt < 0 || fmt > 2 ? 0 : dl::step_k_rt(fmt); }
extern "C" int smdt_decode_linear_unroll(int fmt) { return fmt < 0 || fmt > 2 ? 0 : (fmt == 2 ? dl::unroll(2) : dl::unroll(0)); }

extern "C" int smdt_decode_linear_supported(int dtype, int fmt, int64_t M, int64_t N, int64_t K) {
  if (fmt < 0 || fmt > 2) return 0;
  if (dtype != (int)DType::kBF16 && !(dtype == (int)DType::kF16 && fmt == 0)) return 0;
  if (M < 1 || M > dl::kDlMaxM || N < 8 || N % 8 || K < 32 || K % 32) return 0;
  return N < (1LL << 30) && K < (1LL << 30) && M * N < (1LL << 31);
}

extern "C" void smdt_decode_linear_plan(int fmt, int64_t N, int64_t K, int* splits, int* slice) {
  dl::plan((int)N, (int)K, fmt, splits, slice);
}

extern "C" hipError_t smdt_decode_linear(int dtype, int fmt, const void* x, const void* w, const void* scales,
                                         const void* bias, void* out, float* ws, int64_t M, int64_t N, int64_t K,
                                         hipStream_t st) {
  if (!smdt_decode_linear_supported(dtype, fmt, M, N, K) || (fmt != 0 && scales == nullptr))
    return hipErrorInvalidValue;
  if (dtype == (int)DType::kF16) return dl::launch<f16, 0>(x, w, scales, bias, out, ws, (int)M, (int)N, (int)K, st);
  switch (fmt) {
    case 0: return dl::launch<bf16, 0>(x, w, scales, bias, out, ws, (int)M, (int)N, (int)K, st);
    case 1: return dl::launch<bf16, 1>(x, w, scales, bias, out, ws, (int)M, (int)N, (int)K, st);
    default: return dl::launch<bf16, 2>(x, w, scales, bias, out, ws, (int)M, (int)N, (int)K, st);
  }
}
