// The weight-gradient GEMM core, shared by its 16-bit form (wgrad_gemm.hip) and its FP8 form
// (wgrad_fp8.hip):
//     C[n, k] (fp32) (+)= sum_m A[m, n] * B[m, k]       A = dY [M, N], B = X [M, K], row-major
//
// Why a hand-written kernel: the reduction index m (tokens) is the SLOW index of both operands.
// Library GEMMs treat that as the "NT" layout and stage each operand through an LDS transpose;
// gfx950's ds_read_b64_tr_b16 / _b8 read a row-major [m][n] LDS tile by COLUMNS, which is exactly
// an MFMA operand fragment with 8 consecutive m per lane — so both operands are staged row-major
// and read transposed from LDS (mfma_tile.h, the same images the flash-attention kernels use). No
// transpose pass exists anywhere.
//
// Tile: 256 (n) x 256 (k) output per workgroup, 8 waves as 2 (n) x 4 (k), each wave 128 x 64 =
// 4 x 2 MFMA 32x32x16 accumulators. Stages of 16 KB per operand (32 rows of 16-bit, 64 rows of
// FP8) are copied global -> LDS by global_load_lds_dwordx4 (no VGPR staging, no ds_write pass):
// the LDS image is lane-linear, so the XOR swizzle that keeps the transposed reads bank-conflict
// free is applied to the per-lane SOURCE address. Four stage buffers form a ring with three
// stages in flight: a stage waits with a counted vmcnt for its own DMA only, then one raw
// s_barrier publishes it (measured on MI355X: with one stage in flight the kernel spent ~35 % of
// its time waiting for the DMA — benchmarks/wgrad_micro.hip). Each buffer is its own __shared__
// object so the compiler can see that reads of one buffer do not alias the DMA into another and
// does not drain the queue. The kernel is bound by this LDS-DMA operand stream, not by the MFMA
// clock (profiles/r3_wgrad16/), which is why FP8 operands, half the bytes, pay.
//
// What a format brings is its operand policy (Op16<E>, Op8<BF8> below); the DMA descriptor, the
// ring, the epilogue, the problem table with its block decode and the host code that fills it are
// written here once.
// Work items are ordered (problem, n-group, k, n-in-group) and remapped so that the consecutive
// items an XCD runs share A and B strips in that XCD's L2. Partial tiles (N or K not a multiple
// of 256, as the 50304-row LM head) load clamped columns and skip their stores.
#pragma once
#include <cstdlib>

#include "common.h"
#include "mfma_tile.h"

namespace smdt {
namespace wg {

using namespace mt;
constexpr int BT = 256;              // output tile edge (n and k)
constexpr int SB = 16 * 1024;        // bytes per operand stage image, whatever the format
constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kGlds = SB / 1024 / kWaves;  // 1 KB wave-instructions per operand per stage per wave (2)
constexpr int kNBuf = 4;

// Operand policies. E: element type of the global pointers, V: one MFMA operand fragment, G / F:
// the LDS image and its transposed read, BM: rows of m per stage, kOffs: per-lane read offsets of
// a fragment. kRotate: accumulator i holds A fragment (i + wk) & 3, so that every wave meets the
// fragment its bias sum takes (wk) at compile-time index 0. kBias: a bias form exists. kScale: the
// epilogue multiplies by the product of two dequantisation factors read from the device.
template <class E_>
struct Op16 {   // bf16 / f16: rows of 512 B, XOR-swizzled 16-byte chunks (row bits 0..3)
  using E = E_;
  using V = v8_t<E>;
  using G = Geo<BT>;
  using F = Frag<BT, E>;
  static constexpr int BM = 32, kOffs = 2;
  static constexpr bool kRotate = true, kBias = true, kScale = false;
  __device__ static __forceinline__ void offs(int lane, int dt, int (&o)[kOffs]) {
    o[0] = F::tr_off(lane, dt, 0);
    o[1] = F::tr_off(lane, dt, 1);
  }
  __device__ static __forceinline__ V frag(const char* img, int ks, const int (&o)[kOffs]) {
    return F::trf_at(img, 0, ks, o[0], o[1]);
  }
  __device__ static __forceinline__ f32x16 mma(V a, V b, f32x16 c) { return mfma(a, b, c); }
};
// FP8: rows of 256 B, XOR-swizzled 16-byte chunks (row bits 0..2). A stage is 64 rows of m (the DMA
// granularity of the 16-bit form), so one barrier covers 32 MFMAs per wave instead of 16; a
// fragment is ONE ds_read_b64_tr_b8 and the MFMA is v_mfma_f32_32x32x16_bf8_fp8 (E5M2 dY) or
// _fp8_fp8 (E4M3 dY). No bias form: a bias gradient is not summed from FP8 bytes.
template <bool BF8>
struct Op8 {
  using E = char;
  using V = long;
  using G = Geo8<BT>;
  using F = Frag8<BT>;
  static constexpr int BM = 64, kOffs = 1;
  static constexpr bool kRotate = false, kBias = false, kScale = true;
  __device__ static __forceinline__ void offs(int lane, int dt, int (&o)[kOffs]) { o[0] = F::tr_off(lane, dt); }
  __device__ static __forceinline__ V frag(const char* img, int ks, const int (&o)[kOffs]) {
    return F::trf_at(img, ks, o[0]);
  }
  __device__ static __forceinline__ f32x16 mma(V a, V b, f32x16 c) { return mfma8<BF8>(a, b, c); }
};

// What a problem carries besides its operands and target, per kernel.
struct Bias {
  float* bias;             // column sums of A (bias gradient) or null
};
struct Dequant {
  const float* inv_dy;     // device pointers to the two dequantisation factors
  const float* inv_x;
};

// Copy one BM-row x 256-column stage of an operand into its LDS image. Wave instruction i (of 16)
// fills kRows image rows (1 KB); lane l lands at slot (row kRows i + l / kCh, chunk l % kCh) and
// therefore loads the global chunk whose swizzled position that is: chunk (l % kCh) ^ f(row).
// 16-bit: 2 rows / 32 chunks of 8 elements; FP8: 4 rows / 16 chunks of 16.
template <class Op>
struct Glds {
  using G = typename Op::G;
  static constexpr unsigned kRows = 1024 / G::RB, kCh = G::RB / 16;
  static constexpr int kEl = 16 / (int)sizeof(typename Op::E);
  int off[kGlds];   // element offsets within the stage (row * ld + clamped column)
  __device__ __forceinline__ void init(int wave, int lane, int ld, int col0, int ncols) {
#pragma unroll
    for (int j = 0; j < kGlds; ++j) {
      const int r = kRows * (wave * kGlds + j) + (unsigned)lane / kCh;
      const int c = ((unsigned)lane % kCh) ^ G::f(r);
      int col = col0 + kEl * c;
      if (col > ncols - kEl) col = ncols - kEl;  // partial tile: any in-bounds column, never stored
      off[j] = r * ld + col;
    }
  }
  __device__ __forceinline__ void issue(const typename Op::E* stage_base, char* img, int wave) const {
#pragma unroll
    for (int j = 0; j < kGlds; ++j)
      __builtin_amdgcn_global_load_lds((const void*)(stage_base + off[j]),
                                       (lds_void*)(img + (wave * kGlds + j) * 1024), 16, 0, 0);
  }
};

// Sum of the 8 16-bit values of an operand fragment, in fp32.
template <class V>
__device__ __forceinline__ float sum8(V x) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) s += (float)x[j];
  return s;
}

// One 256 x 256 output tile over stages [0, nst) of Op::BM rows starting at A / B row mstart.
// `bias` is read only by the BIAS form, `inv_dy` / `inv_x` only where Op::kScale. (They are
// __restrict__ parameters of this function, not fields behind a reference: that is what lets the
// compiler read the two factors with scalar loads after the loop.)
// VAR is a diagnostic knob for benchmarks/wgrad_micro.hip only (the library uses VAR = 0):
// bit 0 skips the in-loop DMA, bit 2 the fragment reads. (A v_mfma_f32_16x16x32 form of this
// tile measured +1.7 % on the grouped microbenchmark and neutral-to-slower in the training step,
// profiles/r3_wgrad16/: the kernel is bound by its LDS-DMA operand stream, not by the MFMA clock;
// it was removed.)
//
// BIAS (the k0 == 0 tiles of a problem with a bias): bias[n0 + r] += sum over this tile's m range
// of A[m, n0 + r] — the bias gradient of the linear whose weight gradient this is, from the A (dY)
// fragments the MFMAs read anyway. All four wk waves of a wn read the same A fragments; wave wk
// sums fragment wk, which it processes first (its accumulators are rotated by wk, so the choice is
// a compile-time index): ~16 VALU per 8 MFMAs on these tiles, on the vector pipe the MFMA-bound
// loop leaves idle, no extra LDS reads (replaces the col_sum_rows +
// col_partials_reduce kernels). Tiles without a bias run the BIAS = false instantiation, i.e. the
// round-3 loop. Earlier forms, measured on the GPT-2 345M step (profiles/r4_wgrad_bias/): a fp32
// VALU sum of the fragment was if-converted by the compiler into sums of all four fragments on
// every tile (35.8 -> 45.0 ms of grouped wgrad); picking fragment wk inside the i loop made it
// branch around an MFMA per fragment (bias tiles ~2.5x slower: 37.0 -> 43.8 ms); the re-read
// fragment times an all-ones B operand (one extra MFMA per 8), or the re-read fragment summed by
// VALU, both cost ~2.7 ms (39.7 / 40.4 ms): the tiles of a launch run in rounds of 256, so a slower
// k = 0 tile in every round stretches every round. For that reason the flagship step no longer
// passes a bias here: the QKV and fc1 sums come from the kernels that write those dY (flash_attn.hip
// and gemm_tn.hip SUMS, profiles/bias_from_producer/); FP8, TP / SP and unfused paths still do.
template <class Op, bool ATOMIC, bool BIAS, int VAR>
__device__ __forceinline__ void tile_gemm(const typename Op::E* __restrict__ A, const typename Op::E* __restrict__ B,
                                          float* __restrict__ C, int N, int K, int n0, int k0, int64_t mstart,
                                          int nst, char* L0, char* L1, char* L2, char* L3, float* __restrict__ bias,
                                          const float* __restrict__ inv_dy, const float* __restrict__ inv_x,
                                          bool ovw) {
  static_assert(!BIAS || Op::kBias, "this operand format has no bias form");
  using V = typename Op::V;
  constexpr int BM = Op::BM;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), h = lane >> 5;
  const int wn = wave >> 2, wk = wave & 3;  // wave tile: n rows [128 wn, +128), k cols [64 wk, +64)
  const auto arow = [&](int i) { return Op::kRotate ? (i + wk) & 3 : i; };  // A fragment of accumulator i
  int oa[4][Op::kOffs], ob[2][Op::kOffs];
#pragma unroll
  for (int i = 0; i < 4; ++i) Op::offs(lane, 4 * wn + arow(i), oa[i]);
#pragma unroll
  for (int j = 0; j < 2; ++j) Op::offs(lane, 2 * wk + j, ob[j]);
  f32x16 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = zero16();
  float cs = 0.f;  // BIAS: fp32 sum of this lane's 8 rows of column (lane & 31) of fragment wk

  Glds<Op> ga, gb;
  ga.init(wave, lane, N, n0, N);
  gb.init(wave, lane, K, k0, K);
  const typename Op::E* Ab = A + mstart * N;
  const typename Op::E* Bb = B + mstart * K;
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
    if (!(VAR & 1)) issue(min(s + kNBuf - 1, nst - 1), pre);
    const char* at = cur;
    const char* bt = cur + SB;
#pragma unroll
    for (int ks = 0; ks < BM / 16; ++ks) {
      V b0, b1;
      if constexpr (VAR & 4) {
        const f32x4 t4 = {acc[0][0][4 * ks], acc[0][1][4 * ks], acc[1][0][4 * ks], acc[1][1][4 * ks]};
        b0 = __builtin_bit_cast(V, t4);
        b1 = b0;
      } else {
        b0 = Op::frag(bt, ks, ob[0]);
        b1 = Op::frag(bt, ks, ob[1]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        V a;
        if constexpr (VAR & 4) a = b1;
        else a = Op::frag(at, ks, oa[i]);
        acc[i][0] = Op::mma(a, b0, acc[i][0]);
        acc[i][1] = Op::mma(a, b1, acc[i][1]);
        if constexpr (BIAS) {
          if (i == 0) cs += sum8(a);   // fragment wk (see arow)
        }
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

  if constexpr (BIAS) {
    // lanes l and l ^ 32 summed the two 8-row halves of each 16-row k-step of one column
    cs = __shfl_xor(cs, 32, 64) + cs;
    const int n = n0 + 128 * wn + 32 * wk + (lane & 31);
    if (h == 0 && n < N) {
      if constexpr (ATOMIC) unsafeAtomicAdd(bias + n, cs);
      else bias[n] += cs;
    }
  }

  // Epilogue: register r of acc[i][j] is C[n0 + 128 wn + 32 arow(i) + acc_row(r, h)][k0 + 64 wk + 32 j + lane&31];
  // the 32 lanes of a half write 32 consecutive fp32 (128 B) per register. Full 32-row blocks
  // issue all 16 loads before the adds (one round trip per block, not per element). The FP8 form
  // dequantises on the way; the 16-bit form has no multiply here.
  float sc = 1.f;
  if constexpr (Op::kScale) sc = *inv_dy * *inv_x;
  const auto val = [&](float a) {
    if constexpr (Op::kScale) return sc * a;
    else return a;
  };
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int k = k0 + 64 * wk + 32 * j + (lane & 31);
    const bool kok = k < K;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int nb = n0 + 128 * wn + 32 * arow(i);
      float* cp = C + (int64_t)nb * K + k;
      if (nb + 32 <= N && kok) {
        if constexpr (ATOMIC) {
#pragma unroll
          for (int r2 = 0; r2 < 16; ++r2) unsafeAtomicAdd(cp + (int64_t)acc_row(r2, h) * K, val(acc[i][j][r2]));
        } else if (ovw) {   // first gradient of the step into an unzeroed buffer: store only
#pragma unroll
          for (int r2 = 0; r2 < 16; ++r2) cp[(int64_t)acc_row(r2, h) * K] = val(acc[i][j][r2]);
        } else {
          float old[16];
#pragma unroll
          for (int r2 = 0; r2 < 16; ++r2) old[r2] = cp[(int64_t)acc_row(r2, h) * K];
#pragma unroll
          for (int r2 = 0; r2 < 16; ++r2) cp[(int64_t)acc_row(r2, h) * K] = old[r2] + val(acc[i][j][r2]);
        }
      } else if (kok) {
        for (int r2 = 0; r2 < 16; ++r2) {
          const int rr = acc_row(r2, h);
          if (nb + rr >= N) continue;
          float* p = cp + (int64_t)rr * K;
          const float v = val(acc[i][j][r2]);
          if constexpr (ATOMIC)
            unsafeAtomicAdd(p, v);
          else
            *p = ovw ? v : *p + v;
        }
      }
    }
  }
}

// The four stage buffers of a kernel: separate objects, for the aliasing reason above.
#define SMDT_WGRAD_LDS                                                  \
  __shared__ __attribute__((aligned(1024))) char L0[2 * smdt::wg::SB];  \
  __shared__ __attribute__((aligned(1024))) char L1[2 * smdt::wg::SB];  \
  __shared__ __attribute__((aligned(1024))) char L2[2 * smdt::wg::SB];  \
  __shared__ __attribute__((aligned(1024))) char L3[2 * smdt::wg::SB];

// Tile t of an ntn x ntk grid in groups of gn n-tiles x all k-tiles, n fastest inside a group.
__device__ __forceinline__ void tile_coords(int t, int ntn, int ntk, int gn, int& tn, int& tk) {
  const int grp = t / (gn * ntk);
  const int gn_eff = min(gn, ntn - grp * gn);
  const int tg = t - grp * gn * ntk;
  tn = grp * gn + tg % gn_eff;
  tk = tg / gn_eff;
}

inline int group_width(int ntk) { return ntk <= 4 ? 8 : 4; }

// The problem table of a grouped launch travels in the kernel arguments (~2 KB), read from the
// kernarg segment. X: Bias, Dequant, or the ranged kernel's fields.
template <class X>
struct Problem {
  const void* A;
  const void* B;
  float* C;
  X x;
  int M, N, K, ntn, ntk, gn, tile0;
  int ovw;         // C holds no data yet: the epilogue stores instead of read-add-store
};
constexpr int kMaxGroup = 32;
template <class X>
struct Group {
  Problem<X> p[kMaxGroup];
  int nprob;
  int nfull;    // blocks 0 .. nfull-1: whole tiles (a multiple of the round when a tail is split)
  int splits;   // the tail tiles nfull .. : `splits` blocks each, `mps` stages of the m range apiece
  int mps;
};

// Work item w of a group -> its problem and tile.
template <class X>
__device__ __forceinline__ const Problem<X>& find_tile(const Group<X>& g, int w, int& tn, int& tk) {
  int pi = 0;
  while (pi + 1 < g.nprob && w >= g.p[pi + 1].tile0) ++pi;
  const Problem<X>& P = g.p[pi];
  tile_coords(w - P.tile0, P.ntn, P.ntk, P.gn, tn, tk);
  return P;
}

// Tile (tn, tk) of P over stages [0, nst) from row mstart; the k0 == 0 tiles of a problem with a
// bias take the BIAS form.
template <class Op, bool ATOMIC, class X>
__device__ __forceinline__ void problem_tile(const Problem<X>& P, int tn, int tk, int64_t mstart, int nst, bool ovw,
                                             char* L0, char* L1, char* L2, char* L3) {
  const typename Op::E* A = (const typename Op::E*)P.A;
  const typename Op::E* B = (const typename Op::E*)P.B;
  if constexpr (Op::kScale) {
    tile_gemm<Op, ATOMIC, false, 0>(A, B, P.C, P.N, P.K, tn * BT, tk * BT, mstart, nst, L0, L1, L2, L3, nullptr,
                                    P.x.inv_dy, P.x.inv_x, ovw);
  } else if (P.x.bias != nullptr && tk == 0) {
    tile_gemm<Op, ATOMIC, true, 0>(A, B, P.C, P.N, P.K, tn * BT, 0, mstart, nst, L0, L1, L2, L3, P.x.bias, nullptr,
                                   nullptr, ovw);
  } else {
    tile_gemm<Op, ATOMIC, false, 0>(A, B, P.C, P.N, P.K, tn * BT, tk * BT, mstart, nst, L0, L1, L2, L3, nullptr,
                                    nullptr, nullptr, ovw);
  }
}

// The body of a grouped kernel: block -> (problem, tile, tail piece).
//
// Tail split: whole tiles run in rounds of 256 (one workgroup per CU), so a launch of 256 q + r
// tiles costs q + 1 full rounds even when r is small. The GPT-2 345M LM head alone is
// 197 x 4 = 788 tiles (3 rounds + 20), so every step paid a round with 236 CUs idle. The last r
// tiles of the launch are therefore cut along m into ~256 / r pieces that run together in one
// short round and add their partial sums with fp32 atomics (tail tiles only: their sum order is
// not fixed; everything else stays deterministic). The whole tiles keep the XCD-aware order; the
// pieces go round-robin over the XCDs.
template <class Op, class X>
__device__ __forceinline__ void grouped_block(const Group<X>& g, char* L0, char* L1, char* L2, char* L3) {
  const int bid = blockIdx.x;
  int w, piece = -1;
  if (bid < g.nfull) {
    w = xcd_remap(bid, g.nfull);
  } else {
    const int j = bid - g.nfull;
    w = g.nfull + j / g.splits;
    piece = j % g.splits;
  }
  int tn, tk;
  const Problem<X>& P = find_tile(g, w, tn, tk);
  const int stages = P.M / Op::BM;
  if (piece < 0) {
    problem_tile<Op, false>(P, tn, tk, 0, stages, P.ovw != 0, L0, L1, L2, L3);
  } else {
    const int s0 = piece * g.mps;
    const int nst = min(stages, s0 + g.mps) - s0;
    if (nst <= 0) return;  // a smaller-M problem in the tail: nothing left for this piece (whole block exits)
    problem_tile<Op, true>(P, tn, tk, (int64_t)s0 * Op::BM, nst, false, L0, L1, L2, L3);
  }
}

// SMDT_WGRAD_TAIL_SPLIT=0 turns the split of a grouped launch's tail tiles off.
inline bool tail_split_enabled() {
  static const int on = [] {
    const char* v = getenv("SMDT_WGRAD_TAIL_SPLIT");
    return (v && v[0] == '0') ? 0 : 1;
  }();
  return on != 0;
}

// Tail split of a grouped launch of `tiles` output tiles on R CUs: the r = tiles mod R tail tiles
// are cut along m into `splits` pieces of `mps` stages (at least 8 stages each, at most 16
// pieces); splits = 1 leaves every tile whole.
inline void tail_split(int tiles, int R, int max_stages, int& splits, int& mps) {
  const int r = tiles % R;
  splits = 1;
  mps = 0;
  if (r > 0 && tail_split_enabled()) {
    splits = R / r;
    if (splits > 16) splits = 16;
    if (splits > max_stages / 8) splits = max_stages / 8;
    if (splits > 1) {
      mps = (max_stages + splits - 1) / splits;
      splits = (max_stages + mps - 1) / mps;
    }
  }
  if (splits < 1) splits = 1;
}

// Host: fill a group from `cnt` (<= kMaxGroup) of the caller's problems (SmdtWgradProblem /
// SmdtWgradFp8Problem; extra(q) makes the X of one), pad the table, and split the tail for rounds
// of R CUs (R = 0: every tile whole). The split tail adds partial sums with atomics, so an overwrite
// problem with tail tiles is zeroed on `st` first and accumulates like the rest. Returns the
// grid size in `nblocks`.
template <class X, class Q, class F>
inline hipError_t fill_group(Group<X>& g, const Q* probs, int cnt, int BM, int R, hipStream_t st, int& nblocks,
                             F extra) {
  int tiles = 0, max_stages = 0;
  for (int i = 0; i < cnt; ++i) {
    const Q& q = probs[i];
    Problem<X>& p = g.p[i];
    p.A = q.dy;
    p.B = q.x;
    p.C = q.main_grad;
    p.x = extra(q);
    p.M = (int)q.M;
    p.N = (int)q.N;
    p.K = (int)q.K;
    p.ntn = (int)((q.N + BT - 1) / BT);
    p.ntk = (int)((q.K + BT - 1) / BT);
    p.gn = group_width(p.ntk);
    p.tile0 = tiles;
    p.ovw = q.overwrite ? 1 : 0;
    tiles += p.ntn * p.ntk;
    max_stages = max_stages > p.M / BM ? max_stages : p.M / BM;
  }
  for (int i = cnt; i < kMaxGroup; ++i) g.p[i] = g.p[cnt - 1];
  g.nprob = cnt;
  g.nfull = tiles;
  g.splits = 1;
  g.mps = 0;
  if (R > 0) tail_split(tiles, R, max_stages, g.splits, g.mps);
  if (g.splits > 1) {
    g.nfull = tiles - tiles % R;
    for (int i = 0; i < cnt; ++i) {
      Problem<X>& p = g.p[i];
      if (p.ovw && p.tile0 + p.ntn * p.ntk > g.nfull) {
        hipError_t e = hipMemsetAsync(p.C, 0, (size_t)p.N * (size_t)p.K * sizeof(float), st);
        if (e != hipSuccess) return e;
        p.ovw = 0;
      }
    }
  } else {
    g.mps = 0;
  }
  nblocks = g.nfull + (tiles - g.nfull) * g.splits;
  return hipSuccess;
}

}  // namespace wg
}  // namespace smdt
