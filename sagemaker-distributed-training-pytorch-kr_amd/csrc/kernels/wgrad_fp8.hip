// Weight-gradient GEMM on FP8 operands with fp32 accumulation into the DDP main_grad:
//     C[n, k] (fp32) (+)= (*inv_dy * *inv_x) * sum_m A[m, n] * B[m, k]
// A = q(dY) [M, N] in E5M2 or E4M3, B = q(x) [M, K] in E4M3, both row-major, the OCP encodings
// fp8_quant.hip writes (--fp8-wgrad; the reference's fp8_wgrad, megatron/arguments.py
// "--no-fp8-wgrad"). Both operands exist already: q(x) is made for the forward GEMM and q(dY) for
// the input-gradient GEMM, so this kernel adds no quantise pass. inv_dy / inv_x are device pointers
// to the two dequantisation factors (rows of FP8State.scale_inv): read here, never on the host.
//
// The kernel is wgrad_gemm.hip with one-byte operands. That kernel is bound by its LDS-DMA operand
// stream (profiles/r3_wgrad16/), which FP8 halves. What carries over unchanged: the 256 x 256
// output tile, 8 waves as 2 (n) x 4 (k) with 4 x 2 accumulators of 32x32 each, operand stages
// copied global -> LDS by 16-byte global_load_lds DMA into a ring of four buffers with three stages
// in flight and counted vmcnt waits, the swizzle applied to the DMA's SOURCE address, the work-item
// order and XCD remap, the grouped launch whose tail tiles are split along m with fp32 atomics,
// the `cus` sizing, and clamped loads / skipped stores on partial tiles (wgrad_sched.h).
// What differs:
//   * a stage is 64 rows of m (16 KB per operand, the DMA granularity of the 16-bit kernel: two
//     1 KB wave instructions per operand per wave), so M must be a multiple of 64 and one barrier
//     covers 32 MFMAs per wave instead of 16;
//   * an operand fragment is ONE ds_read_b64_tr_b8 (mfma_tile.h Geo8 / Frag8) and the MFMA is
//     v_mfma_f32_32x32x16_bf8_fp8 (E5M2 dY) or _fp8_fp8 (E4M3 dY);
//   * the epilogue multiplies by the product of the two dequantisation factors;
//   * no bias form: a bias gradient is not summed from FP8 bytes.
#include "common.h"
#include "launchers.h"
#include "mfma_tile.h"
#include "wgrad_sched.h"

namespace smdt {
namespace wg8 {

using namespace mt;
using namespace wg;
constexpr int BT = 256;              // output tile edge (n and k)
constexpr int BM = 64;               // m rows per stage
using G = Geo8<BT>;                  // rows of 256 B, XOR-swizzled 16-byte chunks (row bits 0..2)
using F = Frag8<BT>;
constexpr int SB = BM * G::RB;       // bytes per operand stage image (16 KB)
constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kGlds = SB / 1024 / kWaves;  // 1 KB wave-instructions per operand per stage per wave (2)
constexpr int kNBuf = 4;

// Copy one 64 x 256 byte stage of an operand into its LDS image. Wave instruction i (of 16) fills
// image rows 4i .. 4i + 3; lane l lands at slot (row 4i + l / 16, chunk l % 16) and therefore loads
// the global chunk whose swizzled position that is: chunk (l % 16) ^ f(row).
struct Glds {
  int off[kGlds];   // byte offsets within the stage (row * ld + clamped column)
  __device__ __forceinline__ void init(int wave, int lane, int ld, int col0, int ncols) {
#pragma unroll
    for (int j = 0; j < kGlds; ++j) {
      const int r = 4 * (wave * kGlds + j) + (lane >> 4);
      const int c = (lane & 15) ^ G::f(r);
      int col = col0 + 16 * c;
      if (col > ncols - 16) col = ncols - 16;  // partial tile: any in-bounds column, never stored
      off[j] = r * ld + col;
    }
  }
  __device__ __forceinline__ void issue(const char* stage_base, char* img, int wave) const {
#pragma unroll
    for (int j = 0; j < kGlds; ++j)
      __builtin_amdgcn_global_load_lds((const void*)(stage_base + off[j]),
                                       (lds_void*)(img + (wave * kGlds + j) * 1024), 16, 0, 0);
  }
};

// One 256 x 256 output tile over stages [0, nst) of 64 rows starting at A / B row mstart.
template <bool ATOMIC, bool BF8>
__device__ __forceinline__ void tile_gemm(const char* __restrict__ A, const char* __restrict__ B,
                                          float* __restrict__ C, int N, int K, int n0, int k0, int64_t mstart,
                                          int nst, char* L0, char* L1, char* L2, char* L3,
                                          const float* __restrict__ inv_dy, const float* __restrict__ inv_x,
                                          bool ovw) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), h = lane >> 5;
  const int wn = wave >> 2, wk = wave & 3;  // wave tile: n rows [128 wn, +128), k cols [64 wk, +64)
  int oa[4], ob[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) oa[i] = F::tr_off(lane, 4 * wn + i);
#pragma unroll
  for (int j = 0; j < 2; ++j) ob[j] = F::tr_off(lane, 2 * wk + j);
  f32x16 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = zero16();

  Glds ga, gb;
  ga.init(wave, lane, N, n0, N);
  gb.init(wave, lane, K, k0, K);
  const char* Ab = A + mstart * N;
  const char* Bb = B + mstart * K;
  const int64_t sa = (int64_t)BM * N, sbk = (int64_t)BM * K;

  auto issue = [&](int s, char* img) {
    ga.issue(Ab + s * sa, img, wave);
    gb.issue(Bb + s * sbk, img + SB, wave);
  };
  // Prologue: stages 0 .. kNBuf-2 in flight, wait for stage 0. Every stage issues exactly one
  // DMA (past the end it re-reads the last stage into a buffer nobody reads again), so the
  // counted waits below are uniform and the compiler's own wait insertion stays out of the loop.
  issue(0, L0);
  issue(min(1, nst - 1), L1);
  issue(min(2, nst - 1), L2);
  wait_vm<2 * 2 * kGlds>();
  __builtin_amdgcn_s_barrier();

  // Stage s: prefetch stage s+kNBuf-1 into `pre` (the buffer stage s-1 read, released by the
  // barrier that ended it), MFMA over `cur`, retire stage s+1's DMA, barrier.
  auto stage = [&](int s, const char* cur, char* pre) {
    issue(min(s + kNBuf - 1, nst - 1), pre);
    const char* at = cur;
    const char* bt = cur + SB;
#pragma unroll
    for (int ks = 0; ks < BM / 16; ++ks) {
      const long b0 = F::trf_at(bt, ks, ob[0]);
      const long b1 = F::trf_at(bt, ks, ob[1]);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long a = F::trf_at(at, ks, oa[i]);
        acc[i][0] = mfma8<BF8>(a, b0, acc[i][0]);
        acc[i][1] = mfma8<BF8>(a, b1, acc[i][1]);
      }
    }
    // Stages s+2 .. s+kNBuf-1 stay in flight; stage s+1 must have landed.
    wait_vm<(kNBuf - 2) * 2 * kGlds>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  };
  int s = 0;
  for (; s + kNBuf <= nst; s += kNBuf) {
    stage(s, L0, L3);
    stage(s + 1, L1, L0);
    stage(s + 2, L2, L1);
    stage(s + 3, L3, L2);
  }
  if (s < nst) stage(s, L0, L3);
  if (s + 1 < nst) stage(s + 1, L1, L0);
  if (s + 2 < nst) stage(s + 2, L2, L1);
  wait_vm<0>();  // drain the trailing re-reads before the workgroup's LDS is released

  // Epilogue: dequantise, then as the 16-bit kernel: register r of acc[i][j] is
  // C[n0 + 128 wn + 32 i + acc_row(r, h)][k0 + 64 wk + 32 j + lane&31].
  const float sc = *inv_dy * *inv_x;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int k = k0 + 64 * wk + 32 * j + (lane & 31);
    const bool kok = k < K;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int nb = n0 + 128 * wn + 32 * i;
      float* cp = C + (int64_t)nb * K + k;
      if (nb + 32 <= N && kok) {
        if constexpr (ATOMIC) {
#pragma unroll
          for (int r2 = 0; r2 < 16; ++r2) unsafeAtomicAdd(cp + (int64_t)acc_row(r2, h) * K, sc * acc[i][j][r2]);
        } else if (ovw) {   // first gradient of the step into an unzeroed buffer: store only
#pragma unroll
          for (int r2 = 0; r2 < 16; ++r2) cp[(int64_t)acc_row(r2, h) * K] = sc * acc[i][j][r2];
        } else {
          float old[16];
#pragma unroll
          for (int r2 = 0; r2 < 16; ++r2) old[r2] = cp[(int64_t)acc_row(r2, h) * K];
#pragma unroll
          for (int r2 = 0; r2 < 16; ++r2) cp[(int64_t)acc_row(r2, h) * K] = old[r2] + sc * acc[i][j][r2];
        }
      } else if (kok) {
        for (int r2 = 0; r2 < 16; ++r2) {
          const int rr = acc_row(r2, h);
          if (nb + rr >= N) continue;
          float* p = cp + (int64_t)rr * K;
          const float v = sc * acc[i][j][r2];
          if constexpr (ATOMIC)
            unsafeAtomicAdd(p, v);
          else
            *p = ovw ? v : *p + v;
        }
      }
    }
  }
}

struct Problem {
  const char* A;
  const char* B;
  float* C;
  const float* inv_dy;
  const float* inv_x;
  int M, N, K, ntn, ntk, gn, tile0;
  int ovw;         // C holds no data yet: the epilogue stores instead of read-add-store
};
constexpr int kMaxGroup = 32;
struct Group {
  Problem p[kMaxGroup];
  int nprob;
  int nfull;    // blocks 0 .. nfull-1: whole tiles (a multiple of the round when a tail is split)
  int splits;   // the tail tiles nfull .. : `splits` blocks each, `mps` stages of the m range apiece
  int mps;
};

// The grouped launch of wgrad_gemm.hip (problem table in the kernel arguments, whole tiles in
// XCD-aware order, tail tiles cut along m into pieces that add with fp32 atomics).
template <bool BF8>
__global__ __launch_bounds__(kThreads, 1) void wgrad_fp8_grouped_kernel(const Group g) {
  __shared__ __attribute__((aligned(1024))) char L0[2 * SB];
  __shared__ __attribute__((aligned(1024))) char L1[2 * SB];
  __shared__ __attribute__((aligned(1024))) char L2[2 * SB];
  __shared__ __attribute__((aligned(1024))) char L3[2 * SB];
  const int bid = blockIdx.x;
  int w, piece = -1;
  if (bid < g.nfull) {
    w = xcd_remap(bid, g.nfull);
  } else {
    const int j = bid - g.nfull;
    w = g.nfull + j / g.splits;
    piece = j % g.splits;
  }
  int pi = 0;
  while (pi + 1 < g.nprob && w >= g.p[pi + 1].tile0) ++pi;
  const Problem& P = g.p[pi];
  int tn, tk;
  tile_coords(w - P.tile0, P.ntn, P.ntk, P.gn, tn, tk);
  const int stages = P.M / BM;
  if (piece < 0) {
    tile_gemm<false, BF8>(P.A, P.B, P.C, P.N, P.K, tn * BT, tk * BT, 0, stages, L0, L1, L2, L3, P.inv_dy, P.inv_x,
                          P.ovw != 0);
  } else {
    const int s0 = piece * g.mps;
    const int nst = min(stages, s0 + g.mps) - s0;
    if (nst <= 0) return;  // a smaller-M problem in the tail: nothing left for this piece (whole block exits)
    tile_gemm<true, BF8>(P.A, P.B, P.C, P.N, P.K, tn * BT, tk * BT, (int64_t)s0 * BM, nst, L0, L1, L2, L3, P.inv_dy,
                         P.inv_x, false);
  }
}

}  // namespace wg8
}  // namespace smdt

using namespace smdt;

extern "C" int smdt_wgrad_fp8_supported(int64_t M, int64_t N, int64_t K) {
  return M > 0 && M % wg8::BM == 0 && N >= 16 && K >= 16 && N % 16 == 0 && K % 16 == 0 && M < (1ll << 31) &&
         N * K < (1ll << 31) && (int64_t)wg8::BM * (N > K ? N : K) < (1ll << 31);
}

// One launch per 32 problems, the table passed by value; `cus` as in smdt_wgrad_grouped_cus. The
// problems of one call share dy_fmt (the MFMA opcode is per launch).
extern "C" hipError_t smdt_wgrad_fp8_grouped_cus(const SmdtWgradFp8Problem* probs, int n, int cus, hipStream_t st) {
  const int R = (cus > 0 && cus < 256) ? cus : 256;
  for (int i = 0; i < n; ++i) {
    const SmdtWgradFp8Problem& q = probs[i];
    if (!smdt_wgrad_fp8_supported(q.M, q.N, q.K) || (q.dy_fmt != 0 && q.dy_fmt != 1) || q.dy_fmt != probs[0].dy_fmt ||
        !q.dy || !q.x || !q.main_grad || !q.inv_dy || !q.inv_x)
      return hipErrorInvalidValue;
  }
  for (int base = 0; base < n; base += wg8::kMaxGroup) {
    wg8::Group g;
    const int cnt = n - base < wg8::kMaxGroup ? n - base : wg8::kMaxGroup;
    int tiles = 0, max_stages = 0;
    for (int i = 0; i < cnt; ++i) {
      const SmdtWgradFp8Problem& q = probs[base + i];
      wg8::Problem& p = g.p[i];
      p.A = (const char*)q.dy;
      p.B = (const char*)q.x;
      p.C = q.main_grad;
      p.inv_dy = q.inv_dy;
      p.inv_x = q.inv_x;
      p.M = (int)q.M;
      p.N = (int)q.N;
      p.K = (int)q.K;
      p.ntn = (int)((q.N + wg8::BT - 1) / wg8::BT);
      p.ntk = (int)((q.K + wg8::BT - 1) / wg8::BT);
      p.gn = wg::group_width(p.ntk);
      p.tile0 = tiles;
      p.ovw = q.overwrite ? 1 : 0;
      tiles += p.ntn * p.ntk;
      max_stages = max_stages > p.M / wg8::BM ? max_stages : p.M / wg8::BM;
    }
    for (int i = cnt; i < wg8::kMaxGroup; ++i) g.p[i] = g.p[cnt - 1];
    g.nprob = cnt;
    int splits, mps;
    wg::tail_split(tiles, R, max_stages, splits, mps);
    if (splits <= 1) {
      g.nfull = tiles;
      g.splits = 1;
      g.mps = 0;
    } else {
      g.nfull = tiles - tiles % R;
      g.splits = splits;
      g.mps = mps;
      // the split tail adds partial sums with atomics: an overwrite problem with tail tiles is
      // zeroed first and accumulates like the rest
      for (int i = 0; i < cnt; ++i) {
        wg8::Problem& p = g.p[i];
        if (p.ovw && p.tile0 + p.ntn * p.ntk > g.nfull) {
          hipError_t e = hipMemsetAsync(p.C, 0, (size_t)p.N * (size_t)p.K * sizeof(float), st);
          if (e != hipSuccess) return e;
          p.ovw = 0;
        }
      }
    }
    const int nblocks = g.nfull + (tiles - g.nfull) * g.splits;
    if (probs[0].dy_fmt == 1)
      hipLaunchKernelGGL((wg8::wgrad_fp8_grouped_kernel<true>), dim3(nblocks), dim3(wg8::kThreads), 0, st, g);
    else
      hipLaunchKernelGGL((wg8::wgrad_fp8_grouped_kernel<false>), dim3(nblocks), dim3(wg8::kThreads), 0, st, g);
  }
  return hipGetLastError();
}
