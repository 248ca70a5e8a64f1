// Fused BatchNorm (+ residual add) (+ ReLU) for channels-last activations on gfx950: the training
// forward (statistics sweep + apply sweep), the eval forward (apply alone) and the training
// backward (reduction sweep + dx sweep). COMPONENTS K17c; reached through
// ops.functional.batch_norm_act and ResNet(fused_bn=True).
//
// Operands: x / residual / y / dy / dx / dres are row-major [M, C] (M = N H W of an NHWC tensor),
// bf16 or fp16, one dtype for all; gamma / beta / running statistics / mean / invstd / dgamma /
// dbeta are fp32 [C]; C % 8 == 0, so a row is G = C / 8 channel groups of one 16-byte access each.
//
// Work split (bn_plan, the one place that chooses it; exported as smdt_bn_act_plan):
//   * grid.x = channel tiles. A tile is tg <= 64 channel groups; G is split into ceil(G / 64)
//     tiles of equal size (G = 65 gives 33 + 32, not 64 + 1).
//   * grid.y = row slabs of `slab` rows (a multiple of rl), sized so that tiles x slabs is about
//     1024 workgroups but no thread walks fewer than 8 rows: [802816, 64] is 1 x 1004 workgroups
//     of 25 rows a thread, [3136, 2048] is 4 x 98 of 8 rows a thread.
//   * a workgroup is 256 threads = rl row lanes x tg groups (rl = 256 / tg; the 256 - rl tg left
//     over idle). Thread (r, g) owns channel group g of the tile for rows r, r + rl, ... of the
//     slab: consecutive threads read consecutive 16 bytes, a wave reads whole rows.
//
// What a thread holds: for its 8 channels the per-channel constants (a, b or mean, c1, c2) and, in
// the two reductions, 16 fp32 accumulators; the loads of 8 (statistics) or 4 (other sweeps) of its
// rows are issued before the first is converted.
//
// Statistics: a thread takes its rows 8 at a time. Per channel the chunk mean and the chunk's sum
// of squared deviations FROM THAT MEAN are formed from the 8 registers (two passes over registers,
// no cancellation) and merged into the thread's running (n, mean, M2) by Chan's formula; the two
// weights of the merge depend on the counts alone and are computed once per chunk, not per
// channel. Left-over rows are single Welford updates. E[x^2] - mean^2 is never formed.
//
// Cross-thread reductions: the rl row lanes of a group meet once per workgroup through LDS (each
// thread writes its 8 channels' values, then one thread per channel c < 8 tg, two channels a thread
// past 256, merges lane 0 .. rl - 1 of channel c in lane order) and one partial per (slab, channel) goes to an fp32 workspace [2, nslab, C]
// (mean and M2, or sum g and sum g (x - mean); a slab's count follows from its index and is not
// stored). A finalize launch of 16 channels x 16 slab lanes a workgroup merges slabs l, l + 16, ...
// in lane l and then the 16 lanes in order, writes mean / invstd (or dgamma / dbeta) and updates
// the running statistics on the device. No atomics anywhere: one summation order, bitwise
// repeatable, nothing read on the host.
//
// Not built: NCHW-contiguous and fp32 activations, C % 8 != 0 (the torch twin takes them),
// cross-rank statistics (SyncBatchNorm), folding the statistics sweep into the convolution.

#include "common.h"
#include "launchers.h"

namespace smdt {
namespace {

constexpr int kBnThreads = 256;
constexpr int kBnMaxTileGroups = 64;   // channel groups (of 8 channels) per workgroup at most
constexpr int kBnMinRows = 8;          // a slab is not split below this many rows a thread
constexpr int kBnTargetBlocks = 1024;  // tiles x slabs aimed at (4 workgroups a CU)
constexpr int kBnFinLanes = 16;        // slab lanes of the finalize kernels
constexpr int kBnFinCh = 16;           // channels of a finalize workgroup
constexpr int kBnStatRows = 8;         // rows in flight per thread, statistics sweep
constexpr int kBnRows = 4;             // rows in flight per thread, the other sweeps

struct BnPlan {
  int tg, ntile, rl, nslab;
  int64_t slab;
};

inline BnPlan bn_plan(int64_t M, int64_t C) {
  BnPlan p;
  const int64_t G = C / 8;
  p.ntile = (int)((G + kBnMaxTileGroups - 1) / kBnMaxTileGroups);
  p.tg = (int)((G + p.ntile - 1) / p.ntile);
  p.rl = kBnThreads / p.tg;
  const int64_t per = p.ntile >= kBnTargetBlocks ? 1 : kBnTargetBlocks / p.ntile;  // slabs aimed at
  int64_t slab = (M + per - 1) / per;
  if (slab < (int64_t)p.rl * kBnMinRows) slab = (int64_t)p.rl * kBnMinRows;
  p.slab = (slab + p.rl - 1) / p.rl * p.rl;
  p.nslab = (int)((M + p.slab - 1) / p.slab);  // <= per <= kBnTargetBlocks
  return p;
}

struct BnThread {
  int r, g;      // row lane and channel group within the tile
  int64_t col;   // first of the thread's 8 channels
  bool active;
};

__device__ __forceinline__ BnThread bn_thread(int tg, int rl, int C) {
  BnThread t;
  t.r = (int)threadIdx.x / tg;
  t.g = (int)threadIdx.x - t.r * tg;
  const int gg = (int)blockIdx.x * tg + t.g;
  t.col = (int64_t)gg * 8;
  t.active = t.r < rl && gg < C / 8;
  return t;
}

// (na, ma, qa) <- (na, ma, qa) + (nb, mb, qb): counts, means and sums of squared deviations (Chan).
__device__ __forceinline__ void chan_merge(float& na, float& ma, float& qa, float nb, float mb, float qb) {
  if (nb == 0.f) return;
  const float n = na + nb, d = mb - ma, f = nb / n;
  ma += d * f;
  qa += qb + d * d * na * f;
  na = n;
}

// rows of the slab [r0, r1) that row lane r of rl walks
__device__ __forceinline__ float lane_rows(int64_t len, int r, int rl) {
  return r < len ? (float)((len - r + rl - 1) / rl) : 0.f;
}

template <typename T>
__global__ __launch_bounds__(kBnThreads) void bn_stats_kernel(const T* __restrict__ x, float* __restrict__ ws,
                                                              int64_t M, int C, int tg, int rl, int64_t slab) {
  __shared__ float sm[2][kBnThreads * 8];
  constexpr int KR = kBnStatRows;
  const BnThread t = bn_thread(tg, rl, C);
  const int64_t r0 = (int64_t)blockIdx.y * slab, r1 = r0 + slab < M ? r0 + slab : M;
  float mean[8], m2[8], n = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) mean[j] = m2[j] = 0.f;
  if (t.active) {
    const T* p = x + t.col;
    int64_t row = r0 + t.r;
    for (; row + (int64_t)(KR - 1) * rl < r1; row += (int64_t)KR * rl) {
      Raw8<T> raw[KR];
#pragma unroll
      for (int u = 0; u < KR; ++u) raw[u] = load_raw8_nt(p + (row + (int64_t)u * rl) * C);
      float v[KR][8];
#pragma unroll
      for (int u = 0; u < KR; ++u) cvt_raw8<T>(raw[u], v[u]);
      const float wb = (float)KR / (n + (float)KR), wq = n * wb;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float s = 0.f, q = 0.f;
#pragma unroll
        for (int u = 0; u < KR; ++u) s += v[u][j];
        const float cm = s * (1.f / KR);
#pragma unroll
        for (int u = 0; u < KR; ++u) q = fmaf(v[u][j] - cm, v[u][j] - cm, q);
        const float d = cm - mean[j];
        mean[j] = fmaf(d, wb, mean[j]);
        m2[j] += fmaf(d * d, wq, q);
      }
      n += (float)KR;
    }
    for (; row < r1; row += rl) {
      float v[8];
      cvt_raw8<T>(load_raw8_nt(p + row * C), v);
      n += 1.f;
      const float inv = 1.f / n;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = v[j] - mean[j];
        mean[j] = fmaf(d, inv, mean[j]);
        m2[j] = fmaf(d, v[j] - mean[j], m2[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    sm[0][threadIdx.x * 8 + j] = mean[j];
    sm[1][threadIdx.x * 8 + j] = m2[j];
  }
  __syncthreads();
  // c: channel of the tile (up to 512, two a thread); lane r's value of it is at sm[.][r tg 8 + c]
  for (int c = threadIdx.x; c < tg * 8; c += kBnThreads) {
    const int64_t col = (int64_t)blockIdx.x * tg * 8 + c;
    if (col >= C) break;
    float na = 0.f, ma = 0.f, qa = 0.f;
    for (int r = 0; r < rl; ++r)
      chan_merge(na, ma, qa, lane_rows(r1 - r0, r, rl), sm[0][r * tg * 8 + c], sm[1][r * tg * 8 + c]);
    const int64_t nslab = gridDim.y;
    ws[(int64_t)blockIdx.y * C + col] = ma;
    ws[(nslab + blockIdx.y) * C + col] = qa;
  }
}

// grid.x = ceil(C / 16); thread = (slab lane, channel)
__global__ __launch_bounds__(kBnThreads) void bn_stats_finalize_kernel(const float* __restrict__ ws, int nslab,
                                                                       int64_t slab, int64_t M, int C, float eps,
                                                                       float momentum, float* __restrict__ mean,
                                                                       float* __restrict__ invstd,
                                                                       float* __restrict__ running_mean,
                                                                       float* __restrict__ running_var) {
  __shared__ float sm[3][kBnFinLanes][kBnFinCh + 1];
  const int ch = threadIdx.x % kBnFinCh, lane = threadIdx.x / kBnFinCh;
  const int c = blockIdx.x * kBnFinCh + ch;
  float na = 0.f, ma = 0.f, qa = 0.f;
  if (c < C)
    for (int s = lane; s < nslab; s += kBnFinLanes) {
      const int64_t left = M - (int64_t)s * slab;
      chan_merge(na, ma, qa, (float)(left < slab ? left : slab), ws[(int64_t)s * C + c],
                 ws[((int64_t)nslab + s) * C + c]);
    }
  sm[0][lane][ch] = na;
  sm[1][lane][ch] = ma;
  sm[2][lane][ch] = qa;
  __syncthreads();
  if (lane == 0 && c < C) {
    for (int l = 1; l < kBnFinLanes; ++l) chan_merge(na, ma, qa, sm[0][l][ch], sm[1][l][ch], sm[2][l][ch]);
    const float var = qa / (float)M;
    mean[c] = ma;
    invstd[c] = 1.f / sqrtf(var + eps);
    if (running_mean) running_mean[c] = fmaf(momentum, ma - running_mean[c], running_mean[c]);
    if (running_var) {
      const float unb = qa / (float)(M - 1);
      running_var[c] = fmaf(momentum, unb - running_var[c], running_var[c]);
    }
  }
}

// y = act(a x + b (+ residual)), a = gamma invstd, b = beta - mean a. stat is invstd, or the
// variance (eval mode: the running one) when stat_is_var.
template <typename T, bool RELU, bool RES>
__global__ __launch_bounds__(kBnThreads) void bn_apply_kernel(const T* __restrict__ x, const T* __restrict__ res,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ beta,
                                                              const float* __restrict__ mean,
                                                              const float* __restrict__ stat, T* __restrict__ y,
                                                              int64_t M, int C, int tg, int rl, int64_t slab,
                                                              float eps, int stat_is_var) {
  constexpr int KR = kBnRows;
  const BnThread t = bn_thread(tg, rl, C);
  if (!t.active) return;
  const int64_t r0 = (int64_t)blockIdx.y * slab, r1 = r0 + slab < M ? r0 + slab : M;
  float a[8], b[8];
  load_vec<float, 8>(gamma + t.col, a);
  load_vec<float, 8>(stat + t.col, b);
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] *= stat_is_var ? 1.f / sqrtf(b[j] + eps) : b[j];
  {
    float mu[8];
    load_vec<float, 8>(mean + t.col, mu);
    load_vec<float, 8>(beta + t.col, b);
#pragma unroll
    for (int j = 0; j < 8; ++j) b[j] = fmaf(-mu[j], a[j], b[j]);
  }
  auto row_op = [&](int64_t row, const Raw8<T>& rx, const Raw8<T>& rr) {
    float v[8], q[8];
    cvt_raw8<T>(rx, v);
    if constexpr (RES) cvt_raw8<T>(rr, q);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float o = fmaf(a[j], v[j], b[j]);
      if constexpr (RES) o += q[j];
      if constexpr (RELU) o = o > 0.f ? o : 0.f;
      v[j] = o;
    }
    store_vec<T, 8>(y + row * C + t.col, v);  // plain store: the next convolution reads y right after
  };
  int64_t row = r0 + t.r;
  for (; row + (int64_t)(KR - 1) * rl < r1; row += (int64_t)KR * rl) {
    Raw8<T> rx[KR], rr[KR];
#pragma unroll
    for (int u = 0; u < KR; ++u) {
      const int64_t off = (row + (int64_t)u * rl) * C + t.col;
      rx[u] = load_raw8_nt(x + off);
      if constexpr (RES) rr[u] = load_raw8_nt(res + off);
      else rr[u] = rx[u];
    }
#pragma unroll
    for (int u = 0; u < KR; ++u) row_op(row + (int64_t)u * rl, rx[u], rr[u]);
  }
  for (; row < r1; row += rl) {
    const Raw8<T> rx = load_raw8_nt(x + row * C + t.col);
    row_op(row, rx, RES ? load_raw8_nt(res + row * C + t.col) : rx);
  }
}

// g = dy (y > 0) (RELU: the mask is the sign of the stored output) or dy.
template <typename T, bool RELU>
__device__ __forceinline__ void bn_masked_grad(const Raw8<T>& rdy, const Raw8<T>& ry, float (&g)[8]) {
  cvt_raw8<T>(rdy, g);
  if constexpr (RELU) {
    float o[8];
    cvt_raw8<T>(ry, o);
#pragma unroll
    for (int j = 0; j < 8; ++j) g[j] = o[j] > 0.f ? g[j] : 0.f;
  }
}

// per (slab, channel): sum g -> ws[0], sum g (x - mean) -> ws[1]
template <typename T, bool RELU>
__global__ __launch_bounds__(kBnThreads) void bn_bwd_reduce_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                                   const T* __restrict__ y,
                                                                   const float* __restrict__ mean,
                                                                   float* __restrict__ ws, int64_t M, int C, int tg,
                                                                   int rl, int64_t slab) {
  __shared__ float sm[2][kBnThreads * 8];
  constexpr int KR = kBnRows;
  const BnThread t = bn_thread(tg, rl, C);
  const int64_t r0 = (int64_t)blockIdx.y * slab, r1 = r0 + slab < M ? r0 + slab : M;
  float s1[8], s2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s1[j] = s2[j] = 0.f;
  if (t.active) {
    float mu[8];
    load_vec<float, 8>(mean + t.col, mu);
    auto row_op = [&](const Raw8<T>& rdy, const Raw8<T>& rx, const Raw8<T>& ry) {
      float g[8], v[8];
      bn_masked_grad<T, RELU>(rdy, ry, g);
      cvt_raw8<T>(rx, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        s1[j] += g[j];
        s2[j] = fmaf(g[j], v[j] - mu[j], s2[j]);
      }
    };
    int64_t row = r0 + t.r;
    for (; row + (int64_t)(KR - 1) * rl < r1; row += (int64_t)KR * rl) {
      Raw8<T> rdy[KR], rx[KR], ry[KR];
#pragma unroll
      for (int u = 0; u < KR; ++u) {
        const int64_t off = (row + (int64_t)u * rl) * C + t.col;
        rdy[u] = load_raw8_nt(dy + off);
        rx[u] = load_raw8(x + off);  // x and y are read again by the dx sweep
        if constexpr (RELU) ry[u] = load_raw8(y + off);
        else ry[u] = rx[u];
      }
#pragma unroll
      for (int u = 0; u < KR; ++u) row_op(rdy[u], rx[u], ry[u]);
    }
    for (; row < r1; row += rl) {
      const int64_t off = row * C + t.col;
      const Raw8<T> rx = load_raw8(x + off);
      row_op(load_raw8_nt(dy + off), rx, RELU ? load_raw8(y + off) : rx);
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    sm[0][threadIdx.x * 8 + j] = s1[j];
    sm[1][threadIdx.x * 8 + j] = s2[j];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < tg * 8; c += kBnThreads) {
    const int64_t col = (int64_t)blockIdx.x * tg * 8 + c;
    if (col >= C) break;
    float a1 = 0.f, a2 = 0.f;
    for (int r = 0; r < rl; ++r) {
      a1 += sm[0][r * tg * 8 + c];
      a2 += sm[1][r * tg * 8 + c];
    }
    const int64_t nslab = gridDim.y;
    ws[(int64_t)blockIdx.y * C + col] = a1;
    ws[(nslab + blockIdx.y) * C + col] = a2;
  }
}

__global__ __launch_bounds__(kBnThreads) void bn_bwd_finalize_kernel(const float* __restrict__ ws, int nslab, int C,
                                                                     const float* __restrict__ invstd,
                                                                     float* __restrict__ dgamma,
                                                                     float* __restrict__ dbeta) {
  __shared__ float sm[2][kBnFinLanes][kBnFinCh + 1];
  const int ch = threadIdx.x % kBnFinCh, lane = threadIdx.x / kBnFinCh;
  const int c = blockIdx.x * kBnFinCh + ch;
  float a1 = 0.f, a2 = 0.f;
  if (c < C)
    for (int s = lane; s < nslab; s += kBnFinLanes) {
      a1 += ws[(int64_t)s * C + c];
      a2 += ws[((int64_t)nslab + s) * C + c];
    }
  sm[0][lane][ch] = a1;
  sm[1][lane][ch] = a2;
  __syncthreads();
  if (lane == 0 && c < C) {
    for (int l = 1; l < kBnFinLanes; ++l) {
      a1 += sm[0][l][ch];
      a2 += sm[1][l][ch];
    }
    dbeta[c] = a1;
    dgamma[c] = a2 * invstd[c];
  }
}

// dx = a (g - dbeta / M - xhat dgamma / M), a = gamma invstd, xhat = (x - mean) invstd; inv_m is
// 1 / M, or 0 when the statistics are constants (eval mode): dx = a g. dres = g.
template <typename T, bool RELU, bool RES>
__global__ __launch_bounds__(kBnThreads) void bn_bwd_dx_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                               const T* __restrict__ y,
                                                               const float* __restrict__ gamma,
                                                               const float* __restrict__ mean,
                                                               const float* __restrict__ invstd,
                                                               const float* __restrict__ dgamma,
                                                               const float* __restrict__ dbeta, T* __restrict__ dx,
                                                               T* __restrict__ dres, int64_t M, int C, int tg, int rl,
                                                               int64_t slab, float inv_m) {
  constexpr int KR = kBnRows;
  const BnThread t = bn_thread(tg, rl, C);
  if (!t.active) return;
  const int64_t r0 = (int64_t)blockIdx.y * slab, r1 = r0 + slab < M ? r0 + slab : M;
  float a[8], mu[8], c1[8], c2[8];
  {
    float is[8];
    load_vec<float, 8>(gamma + t.col, a);
    load_vec<float, 8>(invstd + t.col, is);
    load_vec<float, 8>(mean + t.col, mu);
    load_vec<float, 8>(dbeta + t.col, c1);
    load_vec<float, 8>(dgamma + t.col, c2);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      a[j] *= is[j];
      c1[j] *= inv_m;
      c2[j] *= is[j] * inv_m;
    }
  }
  auto row_op = [&](int64_t row, const Raw8<T>& rdy, const Raw8<T>& rx, const Raw8<T>& ry) {
    float g[8], v[8];
    bn_masked_grad<T, RELU>(rdy, ry, g);
    cvt_raw8<T>(rx, v);
    if constexpr (RES) store_vec8_nt<T>(dres + row * C + t.col, g);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = a[j] * (g[j] - c1[j] - (v[j] - mu[j]) * c2[j]);
    store_vec<T, 8>(dx + row * C + t.col, v);  // the convolution's backward reads dx right after
  };
  int64_t row = r0 + t.r;
  for (; row + (int64_t)(KR - 1) * rl < r1; row += (int64_t)KR * rl) {
    Raw8<T> rdy[KR], rx[KR], ry[KR];
#pragma unroll
    for (int u = 0; u < KR; ++u) {
      const int64_t off = (row + (int64_t)u * rl) * C + t.col;
      rdy[u] = load_raw8_nt(dy + off);
      rx[u] = load_raw8_nt(x + off);
      if constexpr (RELU) ry[u] = load_raw8_nt(y + off);
      else ry[u] = rx[u];
    }
#pragma unroll
    for (int u = 0; u < KR; ++u) row_op(row + (int64_t)u * rl, rdy[u], rx[u], ry[u]);
  }
  for (; row < r1; row += rl) {
    const int64_t off = row * C + t.col;
    const Raw8<T> rx = load_raw8_nt(x + off);
    row_op(row, load_raw8_nt(dy + off), rx, RELU ? load_raw8_nt(y + off) : rx);
  }
}

inline dim3 bn_grid(const BnPlan& p) { return dim3((unsigned)p.ntile, (unsigned)p.nslab); }
inline int bn_fin_grid(int64_t C) { return (int)((C + kBnFinCh - 1) / kBnFinCh); }

template <typename T>
hipError_t bn_stats_t(const void* x, float* ws, float* mean, float* invstd, float* rm, float* rv, int64_t M, int64_t C,
                      float eps, float momentum, hipStream_t st) {
  const BnPlan p = bn_plan(M, C);
  bn_stats_kernel<T><<<bn_grid(p), kBnThreads, 0, st>>>((const T*)x, ws, M, (int)C, p.tg, p.rl, p.slab);
  bn_stats_finalize_kernel<<<bn_fin_grid(C), kBnThreads, 0, st>>>(ws, p.nslab, p.slab, M, (int)C, eps, momentum, mean,
                                                                  invstd, rm, rv);
  return hipGetLastError();
}

template <typename T, bool RELU, bool RES>
hipError_t bn_apply_t(const void* x, const void* res, const float* gamma, const float* beta, const float* mean,
                      const float* stat, void* y, int64_t M, int64_t C, float eps, int stat_is_var, hipStream_t st) {
  const BnPlan p = bn_plan(M, C);
  bn_apply_kernel<T, RELU, RES><<<bn_grid(p), kBnThreads, 0, st>>>((const T*)x, (const T*)res, gamma, beta, mean, stat,
                                                                   (T*)y, M, (int)C, p.tg, p.rl, p.slab, eps,
                                                                   stat_is_var);
  return hipGetLastError();
}

template <typename T, bool RELU>
hipError_t bn_bwd_reduce_t(const void* dy, const void* x, const void* y, const float* mean, const float* invstd,
                           float* ws, float* dgamma, float* dbeta, int64_t M, int64_t C, hipStream_t st) {
  const BnPlan p = bn_plan(M, C);
  bn_bwd_reduce_kernel<T, RELU><<<bn_grid(p), kBnThreads, 0, st>>>((const T*)dy, (const T*)x, (const T*)y, mean, ws, M,
                                                                   (int)C, p.tg, p.rl, p.slab);
  bn_bwd_finalize_kernel<<<bn_fin_grid(C), kBnThreads, 0, st>>>(ws, p.nslab, (int)C, invstd, dgamma, dbeta);
  return hipGetLastError();
}

template <typename T, bool RELU, bool RES>
hipError_t bn_bwd_dx_t(const void* dy, const void* x, const void* y, const float* gamma, const float* mean,
                       const float* invstd, const float* dgamma, const float* dbeta, void* dx, void* dres, int64_t M,
                       int64_t C, float inv_m, hipStream_t st) {
  const BnPlan p = bn_plan(M, C);
  bn_bwd_dx_kernel<T, RELU, RES><<<bn_grid(p), kBnThreads, 0, st>>>((const T*)dy, (const T*)x, (const T*)y, gamma, mean,
                                                                    invstd, dgamma, dbeta, (T*)dx, (T*)dres, M, (int)C,
                                                                    p.tg, p.rl, p.slab, inv_m);
  return hipGetLastError();
}

// the three modes ResNet uses: plain, + ReLU, + residual + ReLU
inline int bn_mode(bool relu, bool res) { return !res ? (relu ? 1 : 0) : (relu ? 2 : -1); }

}  // namespace
}  // namespace smdt

using namespace smdt;

extern "C" {

int smdt_bn_act_supported(int dtype, int64_t M, int64_t C) {
  return (dtype == 1 || dtype == 2) && M >= 1 && C >= 8 && C % 8 == 0 && C <= (1 << 24) && M <= ((int64_t)1 << 40) &&
         M * C < ((int64_t)1 << 62);
}

void smdt_bn_act_plan(int64_t M, int64_t C, int* tile_groups, int* ntiles, int* row_lanes, int64_t* slab_rows,
                      int* nslabs) {
  const BnPlan p = bn_plan(M, C);
  *tile_groups = p.tg;
  *ntiles = p.ntile;
  *row_lanes = p.rl;
  *slab_rows = p.slab;
  *nslabs = p.nslab;
}

int smdt_bn_act_constant(int which) {
  constexpr int v[] = {kBnThreads, kBnMaxTileGroups, kBnMinRows, kBnTargetBlocks, kBnFinLanes, kBnFinCh};
  return which >= 0 && which < 6 ? v[which] : -1;
}

hipError_t smdt_bn_stats(int dtype, const void* x, float* ws, float* mean, float* invstd, float* running_mean,
                         float* running_var, int64_t M, int64_t C, float eps, float momentum, hipStream_t st) {
  if (!smdt_bn_act_supported(dtype, M, C)) return hipErrorInvalidValue;
  return dtype == 1 ? bn_stats_t<bf16>(x, ws, mean, invstd, running_mean, running_var, M, C, eps, momentum, st)
                    : bn_stats_t<f16>(x, ws, mean, invstd, running_mean, running_var, M, C, eps, momentum, st);
}

#define SMDT_BN_MODES(T, FN, ...)                           \
  switch (mode) {                                           \
    case 0: return FN<T, false, false>(__VA_ARGS__);        \
    case 1: return FN<T, true, false>(__VA_ARGS__);         \
    case 2: return FN<T, true, true>(__VA_ARGS__);          \
    default: return hipErrorInvalidValue;                   \
  }

hipError_t smdt_bn_apply(int dtype, const void* x, const void* res, const float* gamma, const float* beta,
                         const float* mean, const float* stat, void* y, int64_t M, int64_t C, int relu, float eps,
                         int stat_is_var, hipStream_t st) {
  if (!smdt_bn_act_supported(dtype, M, C)) return hipErrorInvalidValue;
  const int mode = bn_mode(relu != 0, res != nullptr);
  if (dtype == 1) { SMDT_BN_MODES(bf16, bn_apply_t, x, res, gamma, beta, mean, stat, y, M, C, eps, stat_is_var, st) }
  SMDT_BN_MODES(f16, bn_apply_t, x, res, gamma, beta, mean, stat, y, M, C, eps, stat_is_var, st)
}

hipError_t smdt_bn_bwd_reduce(int dtype, const void* dy, const void* x, const void* y, const float* mean,
                              const float* invstd, float* ws, float* dgamma, float* dbeta, int64_t M, int64_t C,
                              hipStream_t st) {
  if (!smdt_bn_act_supported(dtype, M, C)) return hipErrorInvalidValue;
  if (dtype == 1)
    return y ? bn_bwd_reduce_t<bf16, true>(dy, x, y, mean, invstd, ws, dgamma, dbeta, M, C, st)
             : bn_bwd_reduce_t<bf16, false>(dy, x, y, mean, invstd, ws, dgamma, dbeta, M, C, st);
  return y ? bn_bwd_reduce_t<f16, true>(dy, x, y, mean, invstd, ws, dgamma, dbeta, M, C, st)
           : bn_bwd_reduce_t<f16, false>(dy, x, y, mean, invstd, ws, dgamma, dbeta, M, C, st);
}

hipError_t smdt_bn_bwd_dx(int dtype, const void* dy, const void* x, const void* y, const float* gamma,
                          const float* mean, const float* invstd, const float* dgamma, const float* dbeta, void* dx,
                          void* dres, int64_t M, int64_t C, int training, hipStream_t st) {
  if (!smdt_bn_act_supported(dtype, M, C)) return hipErrorInvalidValue;
  const int mode = bn_mode(y != nullptr, dres != nullptr);
  const float inv_m = training ? (float)(1.0 / (double)M) : 0.f;
  if (dtype == 1) { SMDT_BN_MODES(bf16, bn_bwd_dx_t, dy, x, y, gamma, mean, invstd, dgamma, dbeta, dx, dres, M, C, inv_m, st) }
  SMDT_BN_MODES(f16, bn_bwd_dx_t, dy, x, y, gamma, mean, invstd, dgamma, dbeta, dx, dres, M, C, inv_m, st)
}

#undef SMDT_BN_MODES

}  // extern "C"
