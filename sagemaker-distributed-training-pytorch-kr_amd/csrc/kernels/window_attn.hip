// Fused shifted-window attention (Swin v1) for gfx950: forward and backward of
//
//   out = softmax(scale Q K^T + relative-position bias (+ -100 shift mask)) V
//
// per (window, head), reading q / k / v straight out of the qkv linear's output on the padded,
// UNROLLED grid [B, ph, pw, 3 C] and writing the result at the same unrolled positions. The cyclic
// roll, the window partition, the head split and their inverses are address arithmetic: window
// (wy, wx) token (iy, ix) is rolled coordinate (y, x) = (wy ws + iy, wx ws + ix), which lives at
// source coordinate ((y + shift) mod ph, (x + shift) mod pw).
//
// One wave owns one (window, head): N = ws^2 <= 64 tokens padded to 64, head dim 32. All products
// run on v_mfma_f32_32x32x16 (mfma_tile.h); scores and the softmax stay in fp32 registers.
//
//   * The score tile is computed TRANSPOSED (rows = keys, columns = queries), so a lane holds one
//     query's scores over its 16 registers x 2 key tiles: the row max / sum are in-lane plus one
//     exchange with lane ^ 32, and the accumulator registers are directly the B operand of
//     O^T = V^T P^T (pack8). The matching A operand (a column of V over the same permuted 8 keys)
//     is a transposed LDS read of the staged V rows.
//   * The backward recomputes P from qkv and lse. dQ comes from the transposed tile (lane = query),
//     dK / dV from a second, untransposed tile (lane = key) whose per-row lse and
//     delta_i = sum_j P_ij dP_ij are read from LDS.
//   * Table gradient: the wave writes its fp32 dS (64 x 64) to LDS, then lane e sums the <= N pairs
//     (i, j) that share table entry e in a fixed order and writes one partial row per (batch,
//     window); smdt_col_sum adds the rows (layernorm.hip's partial-slab scheme). No atomics: two
//     runs give the same bits.
//
// Rows >= N are never stored and are loaded as zeros; key columns >= N get -inf before the softmax.
#include "common.h"
#include "launchers.h"
#include "mfma_tile.h"

namespace smdt {
namespace {

using namespace mt;

constexpr int kD = 32;                     // head dim
constexpr int kT = 64;                     // padded tokens per window
constexpr int kRS = 2 * kD + 16;           // bytes per staged LDS row (16 bytes of padding)
constexpr int kMaxWs = 8;
constexpr int kMaxE = (2 * kMaxWs - 1) * (2 * kMaxWs - 1);
constexpr int kFwdWaves = 4;
constexpr int kBwdWaves = 2;

struct Params {
  int B, ph, pw, heads, ws, shift, nwx, nW, N, E;
  int64_t total;                           // B * nW * heads waves of work
  float scale;
};

// Per-wave LDS. TILE bytes: the staged 64 x 32 operand rows (forward), aliased in the backward by
// the 64 x 64 fp32 dS of the table gradient.
template <int TILE>
struct alignas(16) WaveLds {
  char tile[TILE];
  float tab[kMaxE + 3];                    // this head's bias table column
  int c[kT];                               // iy (2 ws - 1) + ix of token t
  int reg[kT];                             // shift-mask region id of token t
  float lse[kT];
  float delta[kT];
};

struct Wave {
  int lane, h, l31;
  bool valid;
  int b, win, head, wy, wx;
  int nv;                                  // N for a wave with work, else 0: guards every access
};

__device__ __forceinline__ Wave wave_of(const Params& p, int wpb) {
  Wave w;
  w.lane = threadIdx.x & 63;
  w.h = w.lane >> 5;
  w.l31 = w.lane & 31;
  const int64_t id = (int64_t)blockIdx.x * wpb + (threadIdx.x >> 6);
  w.valid = id < p.total;
  const int64_t idc = w.valid ? id : 0;
  w.head = (int)(idc % p.heads);
  const int64_t bw = idc / p.heads;
  w.win = (int)(bw % p.nW);
  w.b = (int)(bw / p.nW);
  w.wy = w.win / p.nwx;
  w.wx = w.win - w.wy * p.nwx;
  w.nv = w.valid ? p.N : 0;
  return w;
}

// Index of window token t (< N) in the unrolled [B, ph, pw] token grid.
__device__ __forceinline__ int64_t tok_index(const Params& p, const Wave& w, int t) {
  const int iy = t / p.ws, ix = t - iy * p.ws;
  int sy = w.wy * p.ws + iy + p.shift, sx = w.wx * p.ws + ix + p.shift;
  if (sy >= p.ph) sy -= p.ph;
  if (sx >= p.pw) sx -= p.pw;
  return ((int64_t)w.b * p.ph + sy) * p.pw + sx;
}

// Bias table column, relative-coordinate codes and region ids of this wave's window.
template <int TILE>
__device__ __forceinline__ void fill_tables(WaveLds<TILE>& L, const Params& p, const Wave& w,
                                            const float* __restrict__ table) {
  for (int e = w.lane; e < p.E; e += 64) L.tab[e] = table[(int64_t)e * p.heads + w.head];
  const int t = w.lane;
  int c = 0, reg = 0;
  if (t < p.N) {
    const int iy = t / p.ws, ix = t - iy * p.ws;
    c = iy * (2 * p.ws - 1) + ix;
    const int y = w.wy * p.ws + iy, x = w.wx * p.ws + ix;
    const int ry = y < p.ph - p.ws ? 0 : (y < p.ph - p.shift ? 1 : 2);
    const int rx = x < p.pw - p.ws ? 0 : (x < p.pw - p.shift ? 1 : 2);
    reg = 3 * ry + rx;
  }
  L.c[t] = c;
  L.reg[t] = reg;
}

// Row-operand fragments of a [token, 32] matrix: f[t][ks] = row 32 t + (lane & 31), elements
// 16 ks + 8 (lane >> 5) .. + 7 (zeros for rows >= nv). base points at the matrix' column 0 of
// token 0; rs is the token stride in elements.
template <class E>
__device__ __forceinline__ void load_rows(const E* __restrict__ base, int64_t rs, const int64_t (&tok)[2],
                                          const Wave& w, v8_t<E> (&f)[2][2]) {
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const bool ok = 32 * t + w.l31 < w.nv;
    const E* src = base + (ok ? tok[t] : 0) * rs + 8 * w.h;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (ok) v = *reinterpret_cast<const u16x8*>(src + 16 * ks);
      f[t][ks] = __builtin_bit_cast(v8_t<E>, v);
    }
  }
}

// Lane t copies its token's 32 elements into LDS row t (zeros for t >= nv).
template <class E>
__device__ __forceinline__ void stage_rows(char* tile, const E* __restrict__ base, int64_t rs, int64_t tok,
                                           const Wave& w) {
  const bool ok = w.lane < w.nv;
  const E* src = base + (ok ? tok : 0) * rs;
#pragma unroll
  for (int ch = 0; ch < 4; ++ch) {
    u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (ok) v = *reinterpret_cast<const u16x8*>(src + 8 * ch);
    *reinterpret_cast<u16x8*>(tile + w.lane * kRS + 16 * ch) = v;
  }
}

// Transposed fragments of the staged rows: f[t][s] = column (lane & 31) over rows
// 32 t + 16 s + 4 h + {0..3, 8..11}: the row order of accumulator registers 8 s .. 8 s + 7, so it
// pairs with pack8(acc, s) in a product that sums over the tile rows (mfma_tile.h, Frag::trf).
template <class E>
__device__ __forceinline__ void load_cols(const char* tile, const Wave& w, v8_t<E> (&f)[2][2]) {
  const int q = (w.lane >> 2) & 3, pp = w.lane & 3, g = (w.lane >> 4) & 1;
  const int o0 = (4 * w.h + q) * kRS + 2 * (16 * g + 4 * pp);
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const char* b = tile + (32 * t + 16 * s) * kRS + o0;
      s16x4 x = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(b));
      s16x4 y = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(b + 8 * kRS));
      f[t][s] = __builtin_bit_cast(v8_t<E>, __builtin_shufflevector(x, y, 0, 1, 2, 3, 4, 5, 6, 7));
    }
}

// Raw products -> scores. The tile's column token is lt = 32 (column tile) + (lane & 31), its row
// tokens are 32 rtile + acc_row(r, h). QL: the lane (column) is the query and the rows are keys (the
// transposed tile); else the lane is the key. Key >= N: -inf. Query >= N: 0 (never stored, and its
// dO is zero, so it drops out of every gradient).
template <bool QL, int TILE>
__device__ __forceinline__ void fix_scores(f32x16& s, const WaveLds<TILE>& L, const Params& p, const Wave& w,
                                           int lt, int rtile) {
  const int cl = L.c[lt], gl = L.reg[lt];
  const int center = 2 * p.ws * (p.ws - 1);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int rt = 32 * rtile + acc_row(r, w.h);
    const int qt = QL ? lt : rt, kt = QL ? rt : lt;
    const int cr = L.c[rt], gr = L.reg[rt];
    float v = s[r] * p.scale;
    if (kt >= p.N) {
      v = -INFINITY;
    } else if (qt >= p.N) {
      v = 0.f;
    } else {
      const int idx = (QL ? cl - cr : cr - cl) + center;
      v += L.tab[idx];
      if (p.shift > 0 && gl != gr) v += -100.0f;
    }
    s[r] = v;
  }
}

// acc registers 4 g .. 4 g + 3 hold elements 8 g + 4 h .. + 3 of the lane's token: 8-byte stores.
template <class E>
__device__ __forceinline__ void store_token(E* __restrict__ dst, const f32x16& acc, float mul, const Wave& w) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    v4_t<E> v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (E)(acc[4 * g + j] * mul);
    *reinterpret_cast<v4_t<E>*>(dst + 8 * g + 4 * w.h) = v;
  }
}

template <class E>
__global__ __launch_bounds__(64 * kFwdWaves) void window_attn_fwd_kernel(
    const E* __restrict__ qkv, const float* __restrict__ table, E* __restrict__ out, float* __restrict__ lse,
    Params p) {
  using L_t = WaveLds<kT * kRS>;
  __shared__ L_t lds[kFwdWaves];
  L_t& L = lds[threadIdx.x >> 6];
  const Wave w = wave_of(p, kFwdWaves);
  const int C = p.heads * kD;
  const int64_t rs = 3 * (int64_t)C;

  fill_tables(L, p, w, table);
  int64_t tok[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) tok[t] = 32 * t + w.l31 < w.nv ? tok_index(p, w, 32 * t + w.l31) : 0;
  const int64_t tokl = w.h ? tok[1] : tok[0];

  const E* qb = qkv + w.head * kD;
  v8_t<E> Qf[2][2], Kf[2][2], VT[2][2];
  load_rows<E>(qb, rs, tok, w, Qf);
  load_rows<E>(qb + C, rs, tok, w, Kf);
  stage_rows<E>(L.tile, qb + 2 * C, rs, tokl, w);
  __syncthreads();
  load_cols<E>(L.tile, w, VT);

#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    const int lt = 32 * ct + w.l31;                      // this lane's query
    f32x16 st[2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      st[rt] = zero16();
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) st[rt] = mfma(Kf[rt][ks], Qf[ct][ks], st[rt]);
      fix_scores<true>(st[rt], L, p, w, lt, rt);
    }
    float m = -INFINITY;
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int r = 0; r < 16; ++r) m = fmaxf(m, st[rt][r]);
    m = fmaxf(m, __shfl_xor(m, 32, kWave));
    float sum = 0.f;
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        st[rt][r] = __expf(st[rt][r] - m);
        sum += st[rt][r];
      }
    sum += __shfl_xor(sum, 32, kWave);
    const float inv = 1.f / sum;
    f32x16 o = zero16();
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) st[rt][r] *= inv;
#pragma unroll
      for (int s = 0; s < 2; ++s) o = mfma(VT[rt][s], pack8<E>(st[rt], s), o);
    }
    if (lt < w.nv) {
      store_token<E>(out + tok[ct] * C + w.head * kD, o, 1.f, w);
      if (w.h == 0) lse[(((int64_t)w.b * p.nW + w.win) * p.heads + w.head) * p.N + lt] = m + __logf(sum);
    }
  }
}

template <class E>
__global__ __launch_bounds__(64 * kBwdWaves) void window_attn_bwd_kernel(
    const E* __restrict__ qkv, const float* __restrict__ table, const float* __restrict__ lse,
    const E* __restrict__ dout, E* __restrict__ dqkv, float* __restrict__ partials, Params p) {
  using L_t = WaveLds<kT * kT * 4>;
  __shared__ L_t lds[kBwdWaves];
  L_t& L = lds[threadIdx.x >> 6];
  float* dsm = reinterpret_cast<float*>(L.tile);         // dS, [key][query]
  const Wave w = wave_of(p, kBwdWaves);
  const int C = p.heads * kD;
  const int64_t rs = 3 * (int64_t)C;

  fill_tables(L, p, w, table);
  L.lse[w.lane] = w.lane < w.nv ? lse[(((int64_t)w.b * p.nW + w.win) * p.heads + w.head) * p.N + w.lane] : 0.f;
  int64_t tok[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) tok[t] = 32 * t + w.l31 < w.nv ? tok_index(p, w, 32 * t + w.l31) : 0;
  const int64_t tokl = w.h ? tok[1] : tok[0];

  const E* qb = qkv + w.head * kD;
  const E* dob = dout + w.head * kD;
  v8_t<E> Qf[2][2], Kf[2][2], Vf[2][2], Of[2][2], KT[2][2], QT[2][2], OT[2][2];
  load_rows<E>(qb, rs, tok, w, Qf);
  load_rows<E>(qb + C, rs, tok, w, Kf);
  load_rows<E>(qb + 2 * C, rs, tok, w, Vf);
  load_rows<E>(dob, C, tok, w, Of);
  stage_rows<E>(L.tile, qb + C, rs, tokl, w);
  __syncthreads();
  load_cols<E>(L.tile, w, KT);
  __syncthreads();
  stage_rows<E>(L.tile, qb, rs, tokl, w);
  __syncthreads();
  load_cols<E>(L.tile, w, QT);
  __syncthreads();
  stage_rows<E>(L.tile, dob, C, tokl, w);
  __syncthreads();
  load_cols<E>(L.tile, w, OT);
  __syncthreads();                                       // dS aliases the staged rows from here on

  // Pass A, transposed tiles (lane = query): delta, dS -> LDS, dQ.
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    const int lt = 32 * ct + w.l31;
    const float lse_l = L.lse[lt];
    f32x16 st[2], dp[2];
    float delta = 0.f;
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      st[rt] = zero16();
      dp[rt] = zero16();
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        st[rt] = mfma(Kf[rt][ks], Qf[ct][ks], st[rt]);
        dp[rt] = mfma(Vf[rt][ks], Of[ct][ks], dp[rt]);
      }
      fix_scores<true>(st[rt], L, p, w, lt, rt);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        st[rt][r] = __expf(st[rt][r] - lse_l);
        delta += st[rt][r] * dp[rt][r];
      }
    }
    delta += __shfl_xor(delta, 32, kWave);
    if (w.h == 0) L.delta[lt] = delta;
    f32x16 dq = zero16();
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float ds = st[rt][r] * (dp[rt][r] - delta);
        st[rt][r] = ds;
        dsm[(32 * rt + acc_row(r, w.h)) * kT + lt] = ds;
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) dq = mfma(KT[rt][s], pack8<E>(st[rt], s), dq);
    }
    if (lt < w.nv) store_token<E>(dqkv + tok[ct] * rs + w.head * kD, dq, p.scale, w);
  }
  __syncthreads();

  // Table gradient: lane e sums dS over the (query, key) pairs whose offset is entry e.
  {
    const int span = 2 * p.ws - 1;
    float* prow = partials + (((int64_t)w.b * p.nW + w.win) * p.E) * p.heads + w.head;
    for (int e = w.lane; e < p.E; e += 64) {
      const int dy = e / span - (p.ws - 1), dx = e - (e / span) * span - (p.ws - 1);
      float sum = 0.f;
      int jy = 0, jx = 0;
      for (int j = 0; j < p.N; ++j) {
        const int iy = jy + dy, ix = jx + dx;
        if (iy >= 0 && iy < p.ws && ix >= 0 && ix < p.ws) sum += dsm[j * kT + iy * p.ws + ix];
        if (++jx == p.ws) { jx = 0; ++jy; }
      }
      if (w.valid) prow[(int64_t)e * p.heads] = sum;
    }
  }

  // Pass B, untransposed tiles (lane = key): dK, dV.
#pragma unroll
  for (int jt = 0; jt < 2; ++jt) {
    const int lt = 32 * jt + w.l31;
    f32x16 dk = zero16(), dv = zero16();
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      f32x16 s = zero16(), dp = zero16();
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        s = mfma(Qf[it][ks], Kf[jt][ks], s);
        dp = mfma(Of[it][ks], Vf[jt][ks], dp);
      }
      fix_scores<false>(s, L, p, w, lt, it);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = 32 * it + acc_row(r, w.h);
        const float pr = __expf(s[r] - L.lse[i]);
        s[r] = pr;
        dp[r] = pr * (dp[r] - L.delta[i]);
      }
#pragma unroll
      for (int ss = 0; ss < 2; ++ss) {
        dv = mfma(OT[it][ss], pack8<E>(s, ss), dv);
        dk = mfma(QT[it][ss], pack8<E>(dp, ss), dk);
      }
    }
    if (lt < w.nv) {
      E* dst = dqkv + tok[jt] * rs + w.head * kD;
      store_token<E>(dst + C, dk, p.scale, w);
      store_token<E>(dst + 2 * C, dv, 1.f, w);
    }
  }
}

bool make_params(int B, int ph, int pw, int heads, int ws, int shift, Params& p) {
  if (B <= 0 || heads <= 0 || !smdt_window_attn_supported(1, kD, ws, ph, pw, shift)) return false;
  p.B = B; p.ph = ph; p.pw = pw; p.heads = heads; p.ws = ws; p.shift = shift;
  p.nwx = pw / ws;
  p.nW = (ph / ws) * p.nwx;
  p.N = ws * ws;
  p.E = (2 * ws - 1) * (2 * ws - 1);
  p.total = (int64_t)B * p.nW * heads;
  p.scale = 0.17677669529663687f;                        // 32^-0.5
  return p.total <= (int64_t)1 << 30;
}

}  // namespace
}  // namespace smdt

using namespace smdt;

extern "C" int smdt_window_attn_supported(int dtype, int d, int ws, int ph, int pw, int shift) {
  return (dtype == 1 || dtype == 2) && d == kD && ws >= 1 && ws <= kMaxWs && ph >= ws && pw >= ws &&
         ph % ws == 0 && pw % ws == 0 && shift >= 0 && shift < ws;
}

extern "C" hipError_t smdt_window_attn_fwd(int dtype, const void* qkv, const float* table, void* out, float* lse,
                                           int B, int ph, int pw, int heads, int ws, int shift, hipStream_t st) {
  Params p;
  if (!smdt_window_attn_supported(dtype, kD, ws, ph, pw, shift) || !make_params(B, ph, pw, heads, ws, shift, p))
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)((p.total + kFwdWaves - 1) / kFwdWaves)), block(64 * kFwdWaves);
  if (dtype == 1)
    window_attn_fwd_kernel<bf16><<<grid, block, 0, st>>>((const bf16*)qkv, table, (bf16*)out, lse, p);
  else
    window_attn_fwd_kernel<f16><<<grid, block, 0, st>>>((const f16*)qkv, table, (f16*)out, lse, p);
  return hipGetLastError();
}

// partials: fp32 [B * nW, (2 ws - 1)^2 * heads] scratch; dtable: fp32 [(2 ws - 1)^2, heads].
extern "C" hipError_t smdt_window_attn_bwd(int dtype, const void* qkv, const float* table, const float* lse,
                                           const void* dout, void* dqkv, float* partials, float* dtable, int B,
                                           int ph, int pw, int heads, int ws, int shift, hipStream_t st) {
  Params p;
  if (!smdt_window_attn_supported(dtype, kD, ws, ph, pw, shift) || !make_params(B, ph, pw, heads, ws, shift, p))
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)((p.total + kBwdWaves - 1) / kBwdWaves)), block(64 * kBwdWaves);
  if (dtype == 1)
    window_attn_bwd_kernel<bf16><<<grid, block, 0, st>>>((const bf16*)qkv, table, lse, (const bf16*)dout,
                                                         (bf16*)dqkv, partials, p);
  else
    window_attn_bwd_kernel<f16><<<grid, block, 0, st>>>((const f16*)qkv, table, lse, (const f16*)dout,
                                                        (f16*)dqkv, partials, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return smdt_col_sum(partials, B * p.nW, p.E * heads, dtable, 0, st);
}
