// MX-weight GEMM on gfx950: out[M, N] = x[M, K] . dequant(Wq[N, K], s[N, K / 32])^T (+ bias[N]) for
// any M, reading the quantised copy of decode_linear.hip directly and dequantising inside the tile:
//   mxfp8   E4M3 bytes [N, K] + one E8M0 scale byte per 32 elements along K, [N, K / 32]
//   mxfp4   E2M1 nibbles [N, K / 2], element 2j in the low nibble of byte j, scales as for mxfp8
// x, bias and out are bf16. The numerical contract is decode_linear.hip's: the scaled pack
// conversions (v_cvt_scalef32_pk_bf16_fp8 / _fp4) give the exact bf16 value of every weight, the
// products accumulate in fp32, the bias is added in fp32 and there is one rounding at the end, so
// the kernel computes a bf16 linear over dequant(quant(W)) up to the summation order.
//
// Decomposition. A 256-thread workgroup (4 waves) owns a BM x kBN tile of out (BM = 32 / 64 / 128
// rows of x, kBN = 128 rows of W) and a K slice, and walks it in kBK = 64 wide steps. Wave v owns W
// rows 32 v .. 32 v + 31 of the tile against all BM rows of x: BM / 32 accumulators of
// v_mfma_f32_32x32x16_bf16 with W as the A side (so a lane ends up holding four consecutive output
// columns of one row of x: 8-byte stores) and x as the B side.
//
// Data movement per step. W: each thread takes 16-byte loads of quantised W (two loads of 16 E4M3
// bytes, or one of 32 E2M1 nibbles) and the E8M0 byte of each, converts them in registers and writes
// bf16 chunks to a [kBN][kBK] LDS tile in mfma_tile.h's swizzled geometry (Geo<64>); a W element is
// converted once per workgroup and reused by every row of the M tile. x: 16-byte loads to registers,
// written to a [BM][kBK] tile of the same geometry. All four waves read their MFMA operands from the
// two tiles with ds_read_b128. Both tiles are double-buffered: the global loads of step k + 1 are
// issued before the MFMAs of step k and land in the other buffer after them; one barrier per step.
//
// Two regimes (plan): skinny, M <= 128: one M tile, the grid runs over N tiles and every W byte is
// read from HBM once per launch; wide: BM = 128 and a grid over M tiles x N tiles with the M tile
// as the fast index, so consecutive workgroups share a W tile. When the tile count is below
// kSplitBelow, K is cut into S slices of whole steps; slice s writes fp32 partials to ws[s, M, N]
// (caller's workspace) and a second launch sums them in index order and adds the bias. No atomics:
// results are bitwise repeatable.
//
// Edges: rows >= M of x and rows >= N of W read the last valid row instead and are never stored;
// a chunk at k >= the slice's end reads the slice's first chunk instead and contributes zeros (both
// operands are zeroed). Limits live in smdt_wq_gemm_supported alone.
#include "common.h"
#include "launchers.h"
#include "mfma_tile.h"

namespace smdt {
namespace wq {

constexpr int kBN = 128;             // W rows (output columns) per workgroup
constexpr int kBK = 64;              // k per step
constexpr int kThreads = 256;
constexpr int kBMs[3] = {32, 64, 128};
constexpr int kSkinnyMaxM = 128;     // up to here one workgroup holds every row of x
constexpr int kSplitBelow = 256;     // fewer tiles than this: split K
constexpr int kMaxSplits = 16;

using G = mt::Geo<kBK>;              // 128-byte rows, 8 swizzled 16-byte chunks
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;

// 2^(s - 127) for an E8M0 byte s (0: the fp32 subnormal 2^-127; 255, the E8M0 NaN: NaN).
__device__ __forceinline__ float e8m0_to_f32(unsigned s) {
  return __uint_as_float(s == 0u ? 0x00400000u : (s == 255u ? 0x7FC00000u : s << 23));
}

// Elements 8 i .. 8 i + 7 of a 16-byte load of quantised W as one bf16 LDS chunk.
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

// One step's operands on their way from global memory to LDS. FMT 1 / 2; MB = BM / 32.
template <int FMT, int MB>
struct Stage {
  static constexpr int WE = FMT == 1 ? 16 : 32;       // W elements per 16-byte load
  static constexpr int WC = kBK / WE;                 // loads per W row per step
  static constexpr int WL = kBN * WC / kThreads;      // loads per thread per step: 2 / 1
  static constexpr int XL = 32 * MB * 8 / kThreads;   // 16-byte loads of x per thread per step
  const uint8_t* wrow[WL];     // the thread's (clamped) W row, bytes
  const uint8_t* srow[WL];
  const bf16* xrow[XL];
  int wk[WL], xk[XL];          // k offset of the load inside a step
  int wlds[WL], xlds[XL];      // LDS byte offset of the load's first chunk inside its tile
  u32x4 wq[WL], xq[XL];
  unsigned sb[WL];
  bool wok[WL];

  __device__ __forceinline__ void init(const bf16* x, const uint8_t* w, const uint8_t* sc, int m0, int n0, int M,
                                       int N, int K) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < WL; ++i) {
      const int idx = tid + kThreads * i, r = idx / WC, c = idx % WC;
      const int n = n0 + r < N ? n0 + r : N - 1;
      wrow[i] = w + (int64_t)n * (FMT == 1 ? (int64_t)K : (int64_t)K / 2);
      srow[i] = sc + (int64_t)n * (K / 32);
      wk[i] = c * WE;
      wlds[i] = r * G::RB;       // the chunk index is swizzled per store (it depends on the row)
    }
#pragma unroll
    for (int i = 0; i < XL; ++i) {
      const int idx = tid + kThreads * i, r = idx / 8, c = idx % 8;
      const int m = m0 + r < M ? m0 + r : M - 1;
      xrow[i] = x + (int64_t)m * K;
      xk[i] = c * 8;
      xlds[i] = G::off(r, c);
    }
  }

  // Loads of the step at k0 of the slice [ks, ke). A chunk at or beyond ke reads the slice's first
  // chunk (always there) and is zeroed: K % 32 == 0, so a chunk is all inside or all outside.
  __device__ __forceinline__ void load(int k0, int ks, int ke) {
#pragma unroll
    for (int i = 0; i < WL; ++i) {
      wok[i] = k0 + wk[i] < ke;
      const int k = wok[i] ? k0 + wk[i] : ks;
      wq[i] = *reinterpret_cast<const u32x4*>(wrow[i] + (FMT == 1 ? k : k / 2));
      sb[i] = srow[i][k >> 5];
    }
#pragma unroll
    for (int i = 0; i < XL; ++i) {
      const bool ok = k0 + xk[i] < ke;
      const u32x4 v = *reinterpret_cast<const u32x4*>(xrow[i] + (ok ? k0 + xk[i] : ks));
      const u32x4 zero = {0u, 0u, 0u, 0u};
      xq[i] = ok ? v : zero;
    }
  }

  // Convert W and write both operands to the tiles wt [kBN][kBK] and xt [32 MB][kBK].
  __device__ __forceinline__ void store(char* wt, char* xt) const {
#pragma unroll
    for (int i = 0; i < WL; ++i) {
      const float scale = e8m0_to_f32(sb[i]);
      const int r = (threadIdx.x + kThreads * i) / WC;
#pragma unroll
      for (int j = 0; j < WE / 8; ++j) {
        const u32x4 zero = {0u, 0u, 0u, 0u};
        const u32x4 d = __builtin_bit_cast(u32x4, dequant8<FMT>(wq[i], j, scale));
        const int c = wk[i] / 8 + j;
        *reinterpret_cast<u32x4*>(wt + wlds[i] + 16 * (c ^ G::f(r))) = wok[i] ? d : zero;
      }
    }
#pragma unroll
    for (int i = 0; i < XL; ++i) *reinterpret_cast<u32x4*>(xt + xlds[i]) = xq[i];
  }
};

template <int FMT, int MB>
__global__ __launch_bounds__(kThreads) void wq_gemm_kernel(const bf16* __restrict__ x, const uint8_t* __restrict__ w,
                                                           const uint8_t* __restrict__ sc,
                                                           const bf16* __restrict__ bias, bf16* __restrict__ out,
                                                           float* __restrict__ ws, int M, int N, int K, int mtiles,
                                                           int slice) {
  constexpr int BM = 32 * MB;
  constexpr int WT = kBN * G::RB, XT = BM * G::RB;      // bytes per tile
  __shared__ __attribute__((aligned(16))) char lds[2 * (WT + XT)];

  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int m0 = ((int)blockIdx.x % mtiles) * BM;       // the M tile is the fast index
  const int n0 = ((int)blockIdx.x / mtiles) * kBN;
  const int ks = blockIdx.y * slice;
  const int ke = ks + slice < K ? ks + slice : K;
  const int nsteps = (ke - ks + kBK - 1) / kBK;

  Stage<FMT, MB> st;
  st.init(x, w, sc, m0, n0, M, N, K);
  int frag[kBK / 16];                                   // row fragment of k-step s for tile rows 0 .. 31
#pragma unroll
  for (int s = 0; s < kBK / 16; ++s) frag[s] = G::off(l31, 2 * s + h);

  f32x16 acc[MB];
#pragma unroll
  for (int b = 0; b < MB; ++b) acc[b] = mt::zero16();

  st.load(ks, ks, ke);
  st.store(lds, lds + WT);
  __syncthreads();
  for (int s = 0; s < nsteps; ++s) {
    char* cur = lds + (s & 1) * (WT + XT);
    char* nxt = lds + ((s + 1) & 1) * (WT + XT);
    const bool more = s + 1 < nsteps;
    if (more) st.load(ks + (s + 1) * kBK, ks, ke);      // in flight under this step's MFMAs
    const char* wt = cur + wv * 32 * G::RB;
    const char* xt = cur + WT;
#pragma unroll
    for (int k = 0; k < kBK / 16; ++k) {
      const bf16x8 a = *reinterpret_cast<const bf16x8*>(wt + frag[k]);
#pragma unroll
      for (int b = 0; b < MB; ++b) {
        const bf16x8 xb = *reinterpret_cast<const bf16x8*>(xt + b * 32 * G::RB + frag[k]);
        acc[b] = mt::mfma(a, xb, acc[b]);
      }
    }
    // the other buffer was last read in step s - 1, which every wave left at that step's barrier
    if (more) st.store(nxt, nxt + WT);
    __syncthreads();
  }

  // accumulator registers 4 g .. 4 g + 3 of lane (l31, h): W rows 32 wv + 8 g + 4 h .. + 3, row l31 of x
#pragma unroll
  for (int b = 0; b < MB; ++b) {
    const int m = m0 + 32 * b + l31;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int n = n0 + 32 * wv + 8 * g + 4 * h;
      if (m >= M || n >= N) continue;                   // N % 8 == 0: four columns are all inside or all outside
      f32x4 v = {acc[b][4 * g], acc[b][4 * g + 1], acc[b][4 * g + 2], acc[b][4 * g + 3]};
      if (ws != nullptr) {
        *reinterpret_cast<f32x4*>(ws + ((int64_t)blockIdx.y * M + m) * N + n) = v;
        continue;
      }
      bf16 o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (bf16)(bias != nullptr ? v[e] + (float)bias[n + e] : v[e]);
      uint2 pk;
      __builtin_memcpy(&pk, o, 8);
      *reinterpret_cast<uint2*>(out + (int64_t)m * N + n) = pk;
    }
  }
}

// out[m, n] = sum_s ws[s, m, n] (+ bias[n]), slices in index order; four columns per thread.
__global__ __launch_bounds__(256) void wq_gemm_combine_kernel(const float* __restrict__ ws,
                                                              const bf16* __restrict__ bias, bf16* __restrict__ out,
                                                              int64_t MN, int N, int S) {
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= MN) return;
  f32x4 s = *reinterpret_cast<const f32x4*>(ws + i);
  for (int k = 1; k < S; ++k) s += *reinterpret_cast<const f32x4*>(ws + (int64_t)k * MN + i);
  const int n = (int)(i % N);
  bf16 o[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = (bf16)(bias != nullptr ? s[e] + (float)bias[n + e] : s[e]);
  uint2 pk;
  __builtin_memcpy(&pk, o, 8);
  *reinterpret_cast<uint2*>(out + i) = pk;
}

struct Plan {
  int bm, mtiles, ntiles, splits, slice;
};

// Skinny (M <= kSkinnyMaxM): the smallest BM that holds M, one M tile. Wide: BM = 128. One slice
// unless the tiles alone leave CUs idle; slices are whole steps.
inline Plan plan(int64_t M, int64_t N, int64_t K) {
  Plan p;
  p.bm = M <= kBMs[0] ? kBMs[0] : (M <= kBMs[1] ? kBMs[1] : kBMs[2]);
  p.mtiles = (int)((M + p.bm - 1) / p.bm);
  p.ntiles = (int)((N + kBN - 1) / kBN);
  const int64_t tiles = (int64_t)p.mtiles * p.ntiles;
  int64_t S = 1;
  if (tiles < kSplitBelow) {
    S = (kSplitBelow + tiles - 1) / tiles;
    const int64_t most = K / kBK > 1 ? K / kBK : 1;
    S = S > most ? most : S;
    S = S > kMaxSplits ? kMaxSplits : S;
  }
  int64_t sl = (K + S - 1) / S;
  sl = (sl + kBK - 1) / kBK * kBK;
  p.slice = (int)sl;
  p.splits = (int)((K + sl - 1) / sl);
  return p;
}

template <int FMT, int MB>
hipError_t launch_tile(const Plan& p, const void* x, const void* w, const void* sc, const void* bias, void* out,
                       float* ws, int M, int N, int K, hipStream_t st) {
  const dim3 grid((unsigned)(p.mtiles * p.ntiles), (unsigned)p.splits);
  hipLaunchKernelGGL((wq_gemm_kernel<FMT, MB>), grid, dim3(kThreads), 0, st, (const bf16*)x, (const uint8_t*)w,
                     (const uint8_t*)sc, (const bf16*)bias, (bf16*)out, p.splits > 1 ? ws : nullptr, M, N, K,
                     p.mtiles, p.slice);
  return hipGetLastError();
}

template <int FMT>
hipError_t launch(const void* x, const void* w, const void* sc, const void* bias, void* out, float* ws, int M, int N,
                  int K, hipStream_t st) {
  const Plan p = plan(M, N, K);
  if (p.splits > 1 && ws == nullptr) return hipErrorInvalidValue;
  hipError_t e;
  if (p.bm == kBMs[0]) e = launch_tile<FMT, 1>(p, x, w, sc, bias, out, ws, M, N, K, st);
  else if (p.bm == kBMs[1]) e = launch_tile<FMT, 2>(p, x, w, sc, bias, out, ws, M, N, K, st);
  else e = launch_tile<FMT, 4>(p, x, w, sc, bias, out, ws, M, N, K, st);
  if (e != hipSuccess || p.splits == 1) return e;
  const int64_t MN = (int64_t)M * N;
  hipLaunchKernelGGL(wq_gemm_combine_kernel, dim3((unsigned)((MN / 4 + 255) / 256)), dim3(256), 0, st, ws,
                     (const bf16*)bias, (bf16*)out, MN, N, p.splits);
  return hipGetLastError();
}

}  // namespace wq
}  // namespace smdt

using namespace smdt;

extern "C" int smdt_wq_gemm_bn() { return wq::kBN; }
extern "C" int smdt_wq_gemm_bk() { return wq::kBK; }
extern "C" int smdt_wq_gemm_bm(int i) { return i < 0 || i > 2 ? 0 : wq::kBMs[i]; }
extern "C" int smdt_wq_gemm_skinny_max_m() { return wq::kSkinnyMaxM; }
extern "C" int smdt_wq_gemm_split_below() { return wq::kSplitBelow; }

extern "C" int smdt_wq_gemm_supported(int dtype, int fmt, int64_t M, int64_t N, int64_t K) {
  if (dtype != (int)DType::kBF16 || (fmt != 1 && fmt != 2)) return 0;
  if (M < 1 || N < 8 || N % 8 || K < 32 || K % 32) return 0;
  // int indices in the kernel: rows and columns, an M x N offset per slice, the linear tile index
  return M < (1LL << 30) && N < (1LL << 30) && K < (1LL << 30) && M * N < (1LL << 31);
}

extern "C" void smdt_wq_gemm_plan(int fmt, int64_t M, int64_t N, int64_t K, int* bm, int* mtiles, int* ntiles,
                                  int* splits, int* slice) {
  (void)fmt;                     // both formats share the tile
  const wq::Plan p = wq::plan(M, N, K);
  *bm = p.bm;
  *mtiles = p.mtiles;
  *ntiles = p.ntiles;
  *splits = p.splits;
  *slice = p.slice;
}

extern "C" hipError_t smdt_wq_gemm(int dtype, int fmt, const void* x, const void* w, const void* scales,
                                   const void* bias, void* out, float* ws, int64_t M, int64_t N, int64_t K,
                                   hipStream_t st) {
  if (!smdt_wq_gemm_supported(dtype, fmt, M, N, K) || scales == nullptr) return hipErrorInvalidValue;
  if (fmt == 1) return wq::launch<1>(x, w, scales, bias, out, ws, (int)M, (int)N, (int)K, st);
  return wq::launch<2>(x, w, scales, bias, out, ws, (int)M, (int)N, (int)K, st);
}
