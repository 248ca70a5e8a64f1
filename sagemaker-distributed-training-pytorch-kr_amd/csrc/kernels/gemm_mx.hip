// Block-scaled (OCP MX) FP8 GEMM on gfx950's scaled matrix instruction (--fp8-recipe mxfp8):
//     C[m, n] = sum_k A[m, k] 2^(sa[m, k / 32] - 127) * B[n, k] 2^(sb[n, k / 32] - 127)  (+ bias[n])
// A [M, K] bytes (E4M3 or E5M2), B [N, K] bytes (E4M3), both K-contiguous (gemm_tn's TN layout);
// sa [M, K / 32], sb [N, K / 32] E8M0 bytes as mx_quant.hip writes them; fp32 accumulation,
// C [M, N] bf16 / fp16. M, N and K are multiples of 128; the host refuses anything else.
//
// The instruction is v_mfma_scale_f32_16x16x128_f8f6f4. Its operand lane map, measured on the
// MI355X with one-hot operands and per-block scales (profiles/mxfp8/README.md): lane l (row l & 15,
// g = l >> 4) holds k 16 g .. + 15 in registers 0-3 and k 64 + 16 g .. + 15 in registers 4-7 (the
// 128-deep step is two 64-deep halves of the 16-byte-per-lane FP8 map, NOT 32 consecutive k per
// lane), and the scale byte lane l supplies (byte 0 of its scale register, op_sel 0) is that of
// row l & 15, MX block g = k 32 g .. + 31. The element formats are the cbsz / blgp immediates.
// The operands are swapped as in gemm_tn (B rows as the first operand), so a lane's accumulator
// holds four consecutive n of one row m and the epilogue stores 8 bytes per lane. The lane maps
// are pinned by tests/test_mxfp8_gpu.py's exact-data cases (independent operand and scale bytes).
//
// Structure, from gemm_tn.hip as far as it carries, in a plain main loop:
//   * persistent: up to two 256-thread workgroups per CU walk the 128 x 128 output tiles; blockIdx
//     is remapped so an XCD's workgroups take consecutive tiles, ordered in groups of 8 row
//     blocks (row fastest) so they share few A / B panels in that XCD's L2;
//   * a stage is 128 deep in K: a 128-byte LDS row is one K-step of a one-byte operand, so the
//     line-per-row LDS-DMA (16-byte global_load_lds) and the XOR swizzle on its per-lane SOURCE
//     address (row bits 1..3, the LDS image stays lane-linear) are gemm_tn's. The four scale
//     bytes of a row for the stage are one dword and ride with the stage (one 4-byte DMA per
//     thread covers the 128 A rows and the 128 B rows);
//   * two LDS slots: stage kt + 1 is in flight while stage kt is multiplied. One counted wait
//     (vmcnt 0: the next stage is issued after it) and one raw s_barrier per stage publish the
//     stage and retire the reads of the slot the next DMA overwrites;
//   * 4 waves as 2 (m) x 2 (n), each 64 x 64 outputs = 4 x 4 accumulators; a fragment is 32 bytes
//     per lane (two ds_read_b128), the scale one ds_read_u8.
// There is no wave stagger, no cross-tile prefetch and no staged epilogue; what that costs is in
// profiles/mxfp8/README.md.
#include "common.h"
#include "launchers.h"

namespace smdt {
namespace gmx {

constexpr int kT = 128;                  // output tile edge
constexpr int kBK = 128;                 // K (= bytes) per stage
constexpr int kThreads = 256;
constexpr int kOp = kT * kBK;            // 16 KB: one operand of a stage
constexpr int kSc = kT * 4;              // 512 B: one operand's scale dwords of a stage
constexpr int kSlot = 2 * kOp + 2 * kSc; // [A | B | sa | sb]
constexpr int kGl = kOp / 1024 / 4;      // 1-KB DMA wave-instructions per wave per operand (4)

using i32x4 = __attribute__((ext_vector_type(4))) int;
using i32x8 = __attribute__((ext_vector_type(8))) int;
using u32x2 = __attribute__((ext_vector_type(2))) unsigned;

struct Args {
  const uint8_t* A;
  const uint8_t* B;
  const uint8_t* sa;
  const uint8_t* sb;
  void* C;
  const void* bias;
  int M, N, K;
  int ntm, ntn;   // M / 128, N / 128
  int gm;         // tile order: groups of gm row blocks x all column blocks, rows fastest inside
  int tiles;
  int nt;         // K / 128
};

template <class E>
__device__ __forceinline__ u32x2 pack4(float a, float b, float c, float d) {
  using v4 = __attribute__((ext_vector_type(4))) E;
  v4 v = {(E)a, (E)b, (E)c, (E)d};
  return __builtin_bit_cast(u32x2, v);
}

// acc (+)= first (E4M3) x second (E5M2 when ABF8, else E4M3), each lane's block scaled by the low
// byte of its s1 / s2
template <bool ABF8>
__device__ __forceinline__ f32x4 mma(i32x8 first, i32x8 second, f32x4 c, int s1, int s2) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(first, second, c, 0, ABF8 ? 1 : 0, 0, s1, 0, s2);
}

template <class E, bool ABF8, bool BIAS>
__global__ __launch_bounds__(kThreads, 2) void gemm_mx_kernel(const Args g) {
  __shared__ __attribute__((aligned(1024))) char L[2 * kSlot];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = wave >> 1, wc = wave & 1;
  const int G = gridDim.x;
  const int rb = xcd_remap(blockIdx.x, G);
  const int K = g.K, sK = K / 32;

  // per-lane DMA byte offsets: wave-instruction j of an operand writes LDS rows
  // 8 (kGl wave + j) + lane / 8, 16-byte slot lane % 8, which holds chunk slot ^ f(row)
  uint32_t voff[kGl];
#pragma unroll
  for (int j = 0; j < kGl; ++j) {
    const int r = 8 * (kGl * wave + j) + (lane >> 3);
    const int c = (lane & 7) ^ ((r >> 1) & 7);
    voff[j] = (uint32_t)r * (uint32_t)K + 16 * c;
  }
  // fragment reads: row (lane & 15) of a 16-row block, 16-byte chunks (lane >> 4) and 4 + (lane >> 4)
  // (the two 64-deep halves of the step), swizzled by row bits 1..3 (16 r + row has the row's
  // bits 1..3): the 16 lanes of a group hit 16 distinct 16-byte bank slots
  uint32_t fro[2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
    fro[h] = (lane & 15) * kBK + 16 * ((4 * h + (lane >> 4)) ^ ((lane >> 1) & 7));
  // scale bytes: dword (row) of the stage, byte lane >> 4
  const uint32_t sro = 4 * (lane & 15) + (lane >> 4);
  // scale DMA: thread t < 128 brings A row t's dword, t >= 128 B row t - 128's (wave-uniform choice)
  const int srow = threadIdx.x & 127;
  const bool s_is_b = wave >= 2;

  auto coords = [&](int t, int& tm, int& tn) {
    const int per = g.gm * g.ntn;
    const int grp = t / per, first = grp * g.gm;
    const int gsz = min(g.ntm - first, g.gm);
    const int r = t - grp * per;
    tm = first + r % gsz;
    tn = r / gsz;
  };

  for (int tile = rb; tile < g.tiles; tile += G) {
    int tm, tn;
    coords(tile, tm, tn);
    const uint8_t* a_base = g.A + (int64_t)tm * kT * K;
    const uint8_t* b_base = g.B + (int64_t)tn * kT * K;
    const uint8_t* s_src = s_is_b ? g.sb + ((int64_t)tn * kT + srow) * sK : g.sa + ((int64_t)tm * kT + srow) * sK;

    auto issue = [&](int kt) {
      char* slot = L + (kt & 1) * kSlot;
#pragma unroll
      for (int j = 0; j < kGl; ++j)
        __builtin_amdgcn_global_load_lds((const void*)(a_base + voff[j] + (uint32_t)kt * kBK),
                                         (lds_void*)(slot + (kGl * wave + j) * 1024), 16, 0, 0);
#pragma unroll
      for (int j = 0; j < kGl; ++j)
        __builtin_amdgcn_global_load_lds((const void*)(b_base + voff[j] + (uint32_t)kt * kBK),
                                         (lds_void*)(slot + kOp + (kGl * wave + j) * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((const void*)(s_src + 4 * kt), (lds_void*)(slot + 2 * kOp + wave * 256), 4, 0, 0);
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    issue(0);
    for (int kt = 0; kt < g.nt; ++kt) {
      // stage kt has landed (nothing else of this wave is in flight), in every wave after the
      // barrier; every wave has also finished stage kt - 1, whose slot the next DMA overwrites
      wait_vm<0>();
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      if (kt + 1 < g.nt) issue(kt + 1);
      const char* slot = L + (kt & 1) * kSlot;
      const char* la = slot + wr * 64 * kBK;
      const char* lb = slot + kOp + wc * 64 * kBK;
      const char* lsa = slot + 2 * kOp + wr * 64 * 4;
      const char* lsb = slot + 2 * kOp + kSc + wc * 64 * 4;
      i32x8 fb[4];
      int sbv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const i32x4 lo = *(const i32x4*)(lb + j * 16 * kBK + fro[0]);
        const i32x4 hi = *(const i32x4*)(lb + j * 16 * kBK + fro[1]);
        fb[j] = i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        sbv[j] = *(const uint8_t*)(lsb + j * 64 + sro);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const i32x4 lo = *(const i32x4*)(la + i * 16 * kBK + fro[0]);
        const i32x4 hi = *(const i32x4*)(la + i * 16 * kBK + fro[1]);
        const i32x8 fa = i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        const int sav = *(const uint8_t*)(lsa + i * 64 + sro);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = mma<ABF8>(fb[j], fa, acc[i][j], sbv[j], sav);
      }
    }
    // the last stage's reads retire before the next tile's first DMA reuses its slot
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);

    // epilogue: acc[i][j][v] is C[m, n + v], m = 64 wr + 16 i + (lane & 15), n = 64 wc + 16 j + 4 (lane >> 4)
    E* C = (E*)g.C;
    const int64_t m0 = (int64_t)tm * kT + 64 * wr + (lane & 15);
    const int n0 = tn * kT + 64 * wc + 4 * (lane >> 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float bv[4] = {0.f, 0.f, 0.f, 0.f};
      if constexpr (BIAS) {
        using v4 = __attribute__((ext_vector_type(4))) E;
        const v4 b4 = *(const v4*)((const E*)g.bias + n0 + 16 * j);
#pragma unroll
        for (int v = 0; v < 4; ++v) bv[v] = (float)b4[v];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const f32x4 a = acc[i][j];
        *(u32x2*)(C + (m0 + 16 * i) * g.N + n0 + 16 * j) = pack4<E>(a[0] + bv[0], a[1] + bv[1], a[2] + bv[2], a[3] + bv[3]);
      }
    }
  }
}

static int num_cus() {
  static int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
      v = 256;
    return v;
  }();
  return n;
}

template <class E, bool ABF8>
static void launch(const Args& g, bool bias, int grid, hipStream_t st) {
  if (bias) hipLaunchKernelGGL((gemm_mx_kernel<E, ABF8, true>), dim3(grid), dim3(kThreads), 0, st, g);
  else hipLaunchKernelGGL((gemm_mx_kernel<E, ABF8, false>), dim3(grid), dim3(kThreads), 0, st, g);
}

}  // namespace gmx
}  // namespace smdt

using namespace smdt;

extern "C" int smdt_gemm_mx_supported(int64_t M, int64_t N, int64_t K) {
  return M > 0 && N > 0 && K > 0 && M % gmx::kT == 0 && N % gmx::kT == 0 && K % gmx::kBK == 0 &&
         M * K < (1ll << 31) && N * K < (1ll << 31) && M * N < (1ll << 31) &&
         (M / gmx::kT) * (N / gmx::kT) < (1ll << 30);
}

// dtype: the output's (1 bf16, 2 fp16; the bias has it too); a_bf8: A is E5M2. max_blocks > 0 caps
// the number of workgroups (tests: 1 makes a single workgroup walk every tile).
extern "C" hipError_t smdt_gemm_mx(int dtype, int a_bf8, const void* a, const void* sa, const void* b, const void* sb,
                                   void* c, const void* bias, int64_t M, int64_t N, int64_t K, int max_blocks,
                                   hipStream_t st) {
  if (dtype != (int)DType::kBF16 && dtype != (int)DType::kF16) return hipErrorInvalidValue;
  if (!smdt_gemm_mx_supported(M, N, K) || !a || !sa || !b || !sb || !c) return hipErrorInvalidValue;
  gmx::Args g;
  g.A = (const uint8_t*)a; g.B = (const uint8_t*)b; g.sa = (const uint8_t*)sa; g.sb = (const uint8_t*)sb;
  g.C = c; g.bias = bias;
  g.M = (int)M; g.N = (int)N; g.K = (int)K;
  g.ntm = (int)(M / gmx::kT); g.ntn = (int)(N / gmx::kT);
  g.gm = 8;
  g.tiles = g.ntm * g.ntn;
  g.nt = (int)(K / gmx::kBK);
  int grid = 2 * gmx::num_cus();
  if (max_blocks > 0 && max_blocks < grid) grid = max_blocks;
  if (grid > g.tiles) grid = g.tiles;
  if (dtype == (int)DType::kBF16) {
    if (a_bf8) gmx::launch<bf16, true>(g, bias != nullptr, grid, st);
    else gmx::launch<bf16, false>(g, bias != nullptr, grid, st);
  } else {
    if (a_bf8) gmx::launch<f16, true>(g, bias != nullptr, grid, st);
    else gmx::launch<f16, false>(g, bias != nullptr, grid, st);
  }
  return hipGetLastError();
}
