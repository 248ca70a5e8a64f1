// Device-side top-1 router for the Switch MLP (--moe-grouped-gemm): from the router logits [T, E]
// to the expert-sorted, tile-padded row layout the grouped expert GEMMs run on, with no host sync.
//
// Layout: R = (T / 256 + E) * 256 rows (known from the shapes). Expert e owns rows
// [start_e, start_e + rows_e), rows_e = ceil(count_e / 256) * 256, start_e the running sum of the
// earlier rows_e; inside a segment the tokens keep their original order (stable), pad rows follow.
// sum rows_e <= R always; row tiles past the last segment are unused.
//
// Tables (every word written on every call; the buffers may be uninitialised and are reused under
// graph replay):
//   tile_expert[R / 256]  expert of each 256-row tile, -1 for the unused tail tiles
//   seg[E, 2]             (start_e, rows_e)
//   row_of_token[T]       destination row of each token
//   token_of_row[R]       source token of each row, -1 for pad rows (int64: smdt_gather_rows' map)
//   counts[E]             real tokens per expert
//   expert_of_token[T]    the arg-max (a tie goes to the lowest index)
//   top_p[T]              fp32 softmax probability of that expert
//
// A stable counting sort in three launches (no grid-wide spin, no atomics of any kind, so the
// tables are the same on every run):
//   1. route_top1: 256 tokens per block; softmax maximum / arg-max per token in fp32, then the
//      block's histogram [nblk, E] from wave ballots;
//   2. route_scan (one block): counts, seg, tile_expert and the exclusive scan over (expert, block)
//      that gives every block its first row per expert (written over the histogram);
//   3. route_place: every block ranks its own tokens again with the same ballots (an in-block
//      exclusive scan per expert), writes row_of_token / token_of_row, and the blocks together
//      fill the pad rows of token_of_row with -1.
#include "common.h"
#include "launchers.h"

namespace smdt {
namespace moe {

constexpr int kB = 256;      // tokens per block (4 waves)
constexpr int kMaxE = 64;

// Rank of this thread's token among the block's earlier tokens of the same expert `e` (-1: no
// token), and the per-wave counts wcnt[4][kMaxE]. Ends with a block barrier.
__device__ __forceinline__ int block_rank(int e, int E, int* wcnt) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int rk = 0;
  for (int x = 0; x < E; ++x) {
    const unsigned long long m = __ballot(e == x);
    if (lane == 0) wcnt[wave * kMaxE + x] = __popcll(m);
    if (e == x) rk = __popcll(m & ((1ull << lane) - 1ull));
  }
  __syncthreads();
  if (e >= 0)
    for (int w = 0; w < wave; ++w) rk += wcnt[w * kMaxE + e];
  return rk;
}

template <class T>
__global__ __launch_bounds__(kB) void route_top1_kernel(const T* __restrict__ logits, int Tn, int E,
                                                        float* __restrict__ top_p, int* __restrict__ top_e,
                                                        int* __restrict__ hist) {
  __shared__ int wcnt[4 * kMaxE];
  const int t = blockIdx.x * kB + threadIdx.x;
  int e = -1;
  if (t < Tn) {
    const T* row = logits + (int64_t)t * E;
    float m = to_f32(row[0]);
    e = 0;
    for (int i = 1; i < E; ++i) {
      const float v = to_f32(row[i]);
      if (v > m) {   // strict: a tie stays with the lowest index
        m = v;
        e = i;
      }
    }
    float s = 0.f;
    for (int i = 0; i < E; ++i) s += expf(to_f32(row[i]) - m);
    top_p[t] = 1.f / s;   // exp(m - m) / sum
    top_e[t] = e;
  }
  block_rank(e, E, wcnt);
  if (threadIdx.x < E) {
    const int x = threadIdx.x;
    hist[blockIdx.x * E + x] = wcnt[x] + wcnt[kMaxE + x] + wcnt[2 * kMaxE + x] + wcnt[3 * kMaxE + x];
  }
}

// One block of 64 threads, thread e = expert e. hist[b, e] in: tokens of expert e in block b; out:
// the row of block b's first token of expert e.
__global__ __launch_bounds__(64) void route_scan_kernel(int* __restrict__ hist, int nblk, int E, int ntiles,
                                                        int* __restrict__ counts, int* __restrict__ seg,
                                                        int* __restrict__ tile_expert) {
  __shared__ int cnt[kMaxE], start[kMaxE + 1];
  const int e = threadIdx.x;
  if (e < E) {
    int c = 0;
    for (int b = 0; b < nblk; ++b) c += hist[b * E + e];
    cnt[e] = c;
    counts[e] = c;
  }
  __syncthreads();
  if (e == 0) {
    int s = 0;
    for (int x = 0; x < E; ++x) {
      start[x] = s;
      s += (cnt[x] + 255) / 256 * 256;
    }
    start[E] = s;
  }
  __syncthreads();
  if (e < E) {
    seg[2 * e] = start[e];
    seg[2 * e + 1] = start[e + 1] - start[e];
    int run = start[e];
    for (int b = 0; b < nblk; ++b) {
      const int c = hist[b * E + e];
      hist[b * E + e] = run;
      run += c;
    }
  }
  for (int i = e; i < ntiles; i += 64) {
    const int r = i * 256;
    int x = -1;
    for (int q = 0; q < E; ++q)
      if (r >= start[q] && r < start[q + 1]) x = q;
    tile_expert[i] = x;
  }
}

__global__ __launch_bounds__(kB) void route_place_kernel(const int* __restrict__ top_e, const int* __restrict__ first,
                                                         const int* __restrict__ counts, const int* __restrict__ seg,
                                                         const int* __restrict__ tile_expert, int Tn, int E, int R,
                                                         int* __restrict__ row_of_token,
                                                         int64_t* __restrict__ token_of_row) {
  __shared__ int wcnt[4 * kMaxE];
  const int t = blockIdx.x * kB + threadIdx.x;
  const int e = t < Tn ? top_e[t] : -1;
  const int rk = block_rank(e, E, wcnt);
  if (e >= 0) {
    const int r = first[blockIdx.x * E + e] + rk;
    row_of_token[t] = r;
    if (r >= 0 && r < R) token_of_row[r] = t;
  }
  // the pad rows (no token writes them): past the tokens of their segment, or in a tail tile
  for (int r = blockIdx.x * kB + threadIdx.x; r < R; r += gridDim.x * kB) {
    const int x = tile_expert[r >> 8];
    if (x < 0 || r >= seg[2 * x] + counts[x]) token_of_row[r] = -1;
  }
}

}  // namespace moe
}  // namespace smdt

using namespace smdt;

extern "C" int64_t smdt_moe_rows(int64_t T, int64_t E) { return (T / 256 + E) * 256; }

// hist: int32 scratch of ceil(T / 256) * E words.
extern "C" hipError_t smdt_moe_route(int dtype, const void* logits, int64_t T, int64_t E, float* top_p,
                                     int* expert_of_token, int* row_of_token, int64_t* token_of_row,
                                     int* tile_expert, int* seg, int* counts, int* hist, hipStream_t st) {
  if (T <= 0 || E <= 0 || E > moe::kMaxE || dtype < 0 || dtype > 2) return hipErrorInvalidValue;
  const int64_t R = smdt_moe_rows(T, E);
  if (R >= (1ll << 31) || T * E >= (1ll << 31)) return hipErrorInvalidValue;
  const int nblk = (int)((T + moe::kB - 1) / moe::kB);
#define SMDT_RT(TY)                                                                                              \
  hipLaunchKernelGGL((moe::route_top1_kernel<TY>), dim3(nblk), dim3(moe::kB), 0, st, (const TY*)logits, (int)T, \
                     (int)E, top_p, expert_of_token, hist)
  if (dtype == 0) SMDT_RT(float);
  else if (dtype == 1) SMDT_RT(bf16);
  else SMDT_RT(f16);
#undef SMDT_RT
  hipLaunchKernelGGL(moe::route_scan_kernel, dim3(1), dim3(64), 0, st, hist, nblk, (int)E, (int)(R / 256), counts,
                     seg, tile_expert);
  hipLaunchKernelGGL(moe::route_place_kernel, dim3(nblk), dim3(moe::kB), 0, st, expert_of_token, hist, counts, seg,
                     tile_expert, (int)T, (int)E, (int)R, row_of_token, token_of_row);
  return hipGetLastError();
}
