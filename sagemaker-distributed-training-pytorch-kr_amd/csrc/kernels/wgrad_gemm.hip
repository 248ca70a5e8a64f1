// Weight-gradient GEMM with fp32 accumulation into the DDP main_grad, 16-bit operands:
//     C[n, k] (fp32) += sum_m A[m, n] * B[m, k]       A = dY [M, N], B = X [M, K], bf16 / fp16 row-major
// (Megatron's gradient-accumulation fusion; /root/reference/3_training_megatron-lm/
// megatron/arguments.py:850-854). The tile, its stage ring and epilogue, the problem table and the
// host code that fills it are wgrad_core.h (shared with the FP8 form, wgrad_fp8.hip); this file has
// the kernels' entry points and the launchers.
//
// Three launch forms:
//   * smdt_wgrad_accumulate_t: one GEMM; small outputs are split along m (split-K) to cover the
//     256 CUs and the split partials are added with fp32 atomics (~1.3 TB/s chip-wide, so the
//     split count is chosen against that cost); one split does a plain read-modify-write.
//   * smdt_wgrad_grouped_cus: many independent GEMMs (e.g. several layers' QKV / proj / fc1 / fc2
//     weight gradients queued by the deferred-wgrad path) in ONE launch, every tile over its full
//     m range, deterministic, and the tile count of a whole group fills the machine where a
//     single small GEMM cannot. Only the tiles past the last full round of 256 are split along m
//     with fp32 atomics (wgrad_core.h, grouped_block).
//   * the same with ranged problems, whose m range is read on the device (wgrad_ranged_kernel).
#include "common.h"
#include "launchers.h"
#include "wgrad_core.h"

#include <vector>

namespace smdt {
namespace wg {

constexpr int BM = Op16<bf16>::BM;   // m rows per stage

template <bool ATOMIC, int VAR = 0, class E = bf16>
__global__ __launch_bounds__(kThreads, 1) void wgrad_kernel(const E* __restrict__ A, const E* __restrict__ B,
                                                          float* __restrict__ C, int M, int N, int K, int ntn,
                                                          int ntk, int gn, int m_per_split, int nblocks) {
  SMDT_WGRAD_LDS
  const int w = xcd_remap(blockIdx.x, nblocks);
  const int tiles = ntn * ntk;
  const int split = w / tiles;
  int tn, tk;
  tile_coords(w - split * tiles, ntn, ntk, gn, tn, tk);
  const int mstart = split * m_per_split;
  const int nst = (min(M, mstart + m_per_split) - mstart) / BM;
  tile_gemm<Op16<E>, ATOMIC, false, VAR>(A, B, C, N, K, tn * BT, tk * BT, mstart, nst, L0, L1, L2, L3, nullptr, nullptr,
                                         nullptr, false);
}

template <class E>
__global__ __launch_bounds__(kThreads, 1) void wgrad_grouped_kernel(const Group<Bias> g) {
  SMDT_WGRAD_LDS
  grouped_block<Op16<E>>(g, L0, L1, L2, L3);
}

// Ranged problems (the Switch MLP's experts under --moe-grouped-gemm): the m range of a problem is
// not known on the host. It is the segment of expert `expert` in the expert-sorted, tile-padded row
// layout, (start, rows) = mrange[2 expert], mrange[2 expert + 1], written on the device by
// moe_route.hip (rows is a multiple of 256, so of BM). Every block reads its problem's range and
// runs the tile over it: whole tiles only (a tail split would need the length on the host), the
// grid is ntn x ntk per problem whatever the routing was, deterministic. An expert without tokens
// (rows == 0) leaves its gradient as it is, or stores zeros with `ovw`; the block returns before
// any barrier. M of a ranged problem is the row count of A / B: a range outside [0, M] is ignored.
struct Ranged : Bias {
  const int* mrange;   // int32 [nexp, 2] on the device
  int expert;
};

template <class E>
__global__ __launch_bounds__(kThreads, 1) void wgrad_ranged_kernel(const Group<Ranged> g) {
  SMDT_WGRAD_LDS
  int tn, tk;
  const Problem<Ranged>& P = find_tile(g, xcd_remap(blockIdx.x, gridDim.x), tn, tk);
  const int mstart = P.x.mrange[2 * P.x.expert], rows = P.x.mrange[2 * P.x.expert + 1];
  if (mstart < 0 || rows < 0 || rows % BM != 0 || (int64_t)mstart + rows > P.M) return;
  if (rows == 0) {
    if (P.ovw) {   // the target holds no data yet: this expert's gradient is zero
      for (int i = threadIdx.x; i < BT * BT; i += kThreads) {
        const int n = tn * BT + i / BT, k = tk * BT + i % BT;
        if (n < P.N && k < P.K) P.C[(int64_t)n * P.K + k] = 0.f;
      }
    }
    return;
  }
  problem_tile<Op16<E>, false>(P, tn, tk, mstart, rows / BM, P.ovw != 0, L0, L1, L2, L3);
}

}  // namespace wg
}  // namespace smdt

using namespace smdt;

extern "C" int smdt_wgrad_supported(int64_t M, int64_t N, int64_t K) {
  return M > 0 && M % wg::BM == 0 && N >= 8 && K >= 8 && N % 8 == 0 && K % 8 == 0 && M < (1ll << 31) &&
         N * K < (1ll << 31) && (int64_t)wg::BM * (N > K ? N : K) < (1ll << 31);
}

extern "C" hipError_t smdt_wgrad_accumulate_t(int dtype, const void* dy, const void* x, float* main_grad, int64_t M,
                                              int64_t N, int64_t K, int max_splits, hipStream_t st) {
  if (dtype != 1 && dtype != 2) return hipErrorInvalidValue;
  if (!smdt_wgrad_supported(M, N, K)) return hipErrorInvalidValue;
  const int ntn = (int)((N + wg::BT - 1) / wg::BT), ntk = (int)((K + wg::BT - 1) / wg::BT);
  const int tiles = ntn * ntk;
  const int64_t stages = M / wg::BM;
  // Split count: modelled time = rounds of 256 blocks x (stages per split + the atomic epilogue,
  // which costs about as much as 48 stages of 32 rows when every CU adds a 256 KB partial).
  int splits = 1;
  if (max_splits != 1) {
    const int cap = max_splits > 0 ? max_splits : 16;
    double best_t = 1e30;
    for (int s = 1; s <= cap; ++s) {
      if (s > 1 && stages / s < 8) break;
      const int64_t blocks = (int64_t)tiles * s;
      const int64_t rounds = (blocks + 255) / 256;
      const double per = (double)((stages + s - 1) / s) +
                         (s > 1 ? 48.0 * (double)(blocks < 256 ? blocks : 256) / 256.0 : 0.0);
      const double t = rounds * per;
      if (t < best_t * 0.97) {
        best_t = t;
        splits = s;
      }
    }
  }
  const int m_per_split = (int)(((stages + splits - 1) / splits) * wg::BM);
  splits = (int)((M + m_per_split - 1) / m_per_split);
  const int nblocks = tiles * splits;
  const int gn = wg::group_width(ntk);
#define SMDT_WG(AT, ET)                                                                                      \
  hipLaunchKernelGGL((wg::wgrad_kernel<AT, 0, ET>), dim3(nblocks), dim3(wg::kThreads), 0, st, (const ET*)dy, \
                     (const ET*)x, main_grad, (int)M, (int)N, (int)K, ntn, ntk, gn, m_per_split, nblocks)
  if (dtype == 2) {
    if (splits > 1) SMDT_WG(true, f16); else SMDT_WG(false, f16);
  } else {
    if (splits > 1) SMDT_WG(true, bf16); else SMDT_WG(false, bf16);
  }
#undef SMDT_WG
  return hipGetLastError();
}

// Problems with `mrange` (see wgrad_ranged_kernel): one launch per 32, ntn x ntk blocks per problem.
static hipError_t wgrad_ranged_launch(int dtype, const SmdtWgradProblem* probs, int n, hipStream_t st) {
  for (int base = 0; base < n; base += wg::kMaxGroup) {
    wg::Group<wg::Ranged> g;
    const int cnt = n - base < wg::kMaxGroup ? n - base : wg::kMaxGroup;
    for (int i = 0; i < cnt; ++i)
      if (probs[base + i].expert < 0) return hipErrorInvalidValue;
    int tiles;
    hipError_t e = wg::fill_group(g, probs + base, cnt, wg::BM, 0, st, tiles, [](const SmdtWgradProblem& q) {
      return wg::Ranged{{q.bias_grad}, q.mrange, q.expert};
    });
    if (e != hipSuccess) return e;
    if (dtype == 2)
      hipLaunchKernelGGL((wg::wgrad_ranged_kernel<f16>), dim3(tiles), dim3(wg::kThreads), 0, st, g);
    else
      hipLaunchKernelGGL((wg::wgrad_ranged_kernel<bf16>), dim3(tiles), dim3(wg::kThreads), 0, st, g);
  }
  return hipGetLastError();
}

// Grouped form: one launch per 32 problems, the table passed by value.
// `cus`: the CUs this launch can use at once (0 = 256). A launch beside a transfer that holds CUs
// (a filler in a TP exchange wait, parallel/tensor_parallel.DeferredWgrad.fill_one) sizes its
// rounds and its tail split to what is left, so no tail piece waits for the transfer to end.
// Tail split: r = tiles mod 256 tail tiles, ~256 / r pieces each of at least 8 stages; off with
// SMDT_WGRAD_TAIL_SPLIT=0. Ranged problems (device-side m range, see wgrad_ranged_kernel) go to
// launches of their own, never split.
extern "C" hipError_t smdt_wgrad_grouped_cus(int dtype, const SmdtWgradProblem* probs, int n, int cus,
                                             hipStream_t st) {
  if (dtype != 1 && dtype != 2) return hipErrorInvalidValue;
  const int R = (cus > 0 && cus < 256) ? cus : 256;
  for (int i = 0; i < n; ++i)
    if (!smdt_wgrad_supported(probs[i].M, probs[i].N, probs[i].K)) return hipErrorInvalidValue;
  bool any_ranged = false;
  for (int i = 0; i < n; ++i) any_ranged = any_ranged || probs[i].mrange != nullptr;
  if (any_ranged) {
    std::vector<SmdtWgradProblem> plain, ranged;
    for (int i = 0; i < n; ++i) (probs[i].mrange ? ranged : plain).push_back(probs[i]);
    if (!plain.empty()) {
      hipError_t e = smdt_wgrad_grouped_cus(dtype, plain.data(), (int)plain.size(), cus, st);
      if (e != hipSuccess) return e;
    }
    return wgrad_ranged_launch(dtype, ranged.data(), (int)ranged.size(), st);
  }
  for (int base = 0; base < n; base += wg::kMaxGroup) {
    wg::Group<wg::Bias> g;
    const int cnt = n - base < wg::kMaxGroup ? n - base : wg::kMaxGroup;
    int nblocks;
    hipError_t e = wg::fill_group(g, probs + base, cnt, wg::BM, R, st, nblocks,
                                  [](const SmdtWgradProblem& q) { return wg::Bias{q.bias_grad}; });
    if (e != hipSuccess) return e;
    if (dtype == 2)
      hipLaunchKernelGGL((wg::wgrad_grouped_kernel<f16>), dim3(nblocks), dim3(wg::kThreads), 0, st, g);
    else
      hipLaunchKernelGGL((wg::wgrad_grouped_kernel<bf16>), dim3(nblocks), dim3(wg::kThreads), 0, st, g);
  }
  return hipGetLastError();
}
