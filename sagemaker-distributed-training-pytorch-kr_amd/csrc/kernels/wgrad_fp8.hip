// Weight-gradient GEMM on FP8 operands with fp32 accumulation into the DDP main_grad:
//     C[n, k] (fp32) (+)= (*inv_dy * *inv_x) * sum_m A[m, n] * B[m, k]
// A = q(dY) [M, N] in E5M2 or E4M3, B = q(x) [M, K] in E4M3, both row-major, the OCP encodings
// fp8_quant.hip writes (--fp8-wgrad; the reference's fp8_wgrad, megatron/arguments.py
// "--no-fp8-wgrad"). Both operands exist already: q(x) is made for the forward GEMM and q(dY) for
// the input-gradient GEMM, so this kernel adds no quantise pass. inv_dy / inv_x are device pointers
// to the two dequantisation factors (rows of FP8State.scale_inv): read here, never on the host.
//
// The kernel is the tile of wgrad_core.h with the one-byte operand policy Op8: a stage of 64 rows
// (so M must be a multiple of 64), one ds_read_b64_tr_b8 per fragment, the FP8 MFMA, a
// dequantising epilogue and no bias form. Everything else is the 16-bit kernel's (wgrad_gemm.hip).
#include "common.h"
#include "launchers.h"
#include "wgrad_core.h"

namespace smdt {
namespace wg8 {

using namespace wg;
constexpr int BM = Op8<true>::BM;    // m rows per stage

// The grouped launch of wgrad_gemm.hip (problem table in the kernel arguments, whole tiles in
// XCD-aware order, tail tiles cut along m into pieces that add with fp32 atomics).
template <bool BF8>
__global__ __launch_bounds__(kThreads, 1) void wgrad_fp8_grouped_kernel(const Group<Dequant> g) {
  SMDT_WGRAD_LDS
  grouped_block<Op8<BF8>>(g, L0, L1, L2, L3);
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
  for (int base = 0; base < n; base += wg::kMaxGroup) {
    wg::Group<wg::Dequant> g;
    const int cnt = n - base < wg::kMaxGroup ? n - base : wg::kMaxGroup;
    int nblocks;
    hipError_t e = wg::fill_group(g, probs + base, cnt, wg8::BM, R, st, nblocks,
                                  [](const SmdtWgradFp8Problem& q) { return wg::Dequant{q.inv_dy, q.inv_x}; });
    if (e != hipSuccess) return e;
    if (probs[0].dy_fmt == 1)
      hipLaunchKernelGGL((wg8::wgrad_fp8_grouped_kernel<true>), dim3(nblocks), dim3(wg::kThreads), 0, st, g);
    else
      hipLaunchKernelGGL((wg8::wgrad_fp8_grouped_kernel<false>), dim3(nblocks), dim3(wg::kThreads), 0, st, g);
  }
  return hipGetLastError();
}
