// Fused token sampler for generate(sampler="fused"): from the next-token logits [B, V] to the
// emitted token, the write into the sequence buffer and the finished flag, in one launch.
//
// One 1024-thread workgroup owns a row; no workspace, no float atomics. The rule (the float64 twin
// is ops.functional.sample_tokens_ref):
//   greedy    the lowest index of the row maximum;
//   sampling  p_i = exp((x_i - max) / T); top-k keeps x_i >= the k-th largest value (ties at that
//             value stay); top-p keeps a survivor iff the mass of the survivors with a strictly
//             greater logit is below top_p * Z_k (Z_k: the survivors' mass), so the most likely
//             token and a whole tie class at the cut stay; the token is the first kept index, in
//             vocabulary order, whose inclusive prefix mass exceeds u * Z (Z: the kept mass).
// -inf entries have mass 0 and are never chosen. Rows holding NaN or +inf are outside the contract:
// they return some index in 0 .. V - 1 and touch no memory outside the operands.
//
// How a row is worked:
//   * every element is handled through its order-preserving integer key (the bits of the raw logit
//     with the sign folded, -0 read as +0): 16 bits for bf16 / fp16, 32 for fp32. Dividing by T is
//     monotone, so the raw keys order the row as the tempered logits do.
//   * pass 1 reads the row from global memory (16-byte loads where the row start is 16-byte
//     aligned, scalar loads otherwise), reduces max / arg-max as one 64-bit integer (key, ~index)
//     and, for a 16-bit row of up to kStageMax entries, leaves the keys in LDS; every later pass
//     reads them there. Longer and fp32 rows are read again through L2.
//   * mass is fixed point: round(p_i * 2^40) in 64-bit integers (p_i <= 1 and V < 2^20, so a row
//     sums below 2^60). Integer adds commute: histograms, prefix sums and therefore the token are
//     the same on every run, bit for bit.
//   * both thresholds come from a radix select over the keys, 8 bits a level (two levels for 16-bit
//     keys, four for fp32). A level histograms the elements under the current prefix into 256 bins
//     of count and mass with LDS integer atomics; each bin has kCopies copies, picked by lane, so
//     the lanes of a wave that hit one hot bin (a softmax row fills a handful of exponent bins)
//     spread over kCopies addresses. 256 threads then scan the bins from the top and the level
//     keeps the lowest non-empty bin whose count (top-k) or mass (top-p) above it is still below
//     the target. The level-0 histogram is built once and serves both selects.
//   * top-k's threshold first, then top-p's against top_p * Z_k; the cut is the larger key.
//   * the draw scans the kept mass in vocabulary order, kChunk elements at a time (8 consecutive
//     elements per thread, a block-wide 64-bit prefix scan), and stops at the chunk where the
//     running sum passes floor(u * Z).
//   * thread 0 does the bookkeeping: a finished row emits pad (and skips all of the above),
//     seq[b, plen[b] + t] = tok, finished[b] |= tok == eos.
#include "common.h"
#include "launchers.h"

namespace smdt {
namespace sample {

using ull = unsigned long long;

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / kWave;
constexpr int kVec = 8;                     // consecutive elements a thread takes at a time
constexpr int kChunk = kThreads * kVec;     // elements per block-wide step
constexpr int kBins = 256;                  // 8 key bits per radix level
constexpr int kCopies = 8;                  // copies of every bin, picked by lane
constexpr int kStageMax = 65536;            // 16-bit keys kept in LDS (128 KB of the CU's 160 KB)
constexpr int kMaxV = 1 << 20;              // keeps a row's fixed-point mass below 2^60
constexpr float kMassOne = 0x1p40f;         // fixed-point 1.0

struct Args {
  const void* logits;
  int64_t stride;            // elements between rows
  int V;
  const float* u;            // [B], unused when greedy
  float log2e_over_t;
  int top_k;                 // outside 1 .. V - 1: no top-k
  double top_p;              // >= 1: no top-p
  int do_sample;
  int64_t* seq;              // [B, S] or null: no bookkeeping
  int64_t S;
  const int64_t* plen;
  int64_t t;
  unsigned char* finished;   // [B] bool, or null
  int64_t eos, pad;          // eos < 0: none
  int64_t* tok;
};

template <class T> constexpr int levels() { return sizeof(T) == 2 ? 2 : 4; }

// raw bits -> key: a larger value has a larger key (NaN aside); -0 and +0 share one key
template <class T>
__device__ __forceinline__ uint32_t key_of_bits(uint32_t b) {
  if constexpr (sizeof(T) == 2) {
    if (b == 0x8000u) b = 0;
    return (b & 0x8000u) ? (~b & 0xFFFFu) : (b | 0x8000u);
  } else {
    if (b == 0x80000000u) b = 0;
    return (b >> 31) ? ~b : (b | 0x80000000u);
  }
}

template <class T>
__device__ __forceinline__ float value_of_key(uint32_t k) {
  if constexpr (sizeof(T) == 2) {
    const unsigned short b = (unsigned short)((k & 0x8000u) ? (k ^ 0x8000u) : ~k);
    T x;
    __builtin_memcpy(&x, &b, 2);
    return to_f32(x);
  } else {
    return __uint_as_float((k >> 31) ? (k ^ 0x80000000u) : ~k);
  }
}

template <class T>
__device__ __forceinline__ uint32_t bits_of(T x) {
  if constexpr (sizeof(T) == 2) {
    unsigned short b;
    __builtin_memcpy(&b, &x, 2);
    return b;
  } else {
    return __float_as_uint(x);
  }
}

// round(exp((x - max) / T) * 2^40): one subtraction, one product and one v_exp_f32 in fp32. Every
// pass calls this with the same operands, so a key has one mass throughout the kernel.
template <class T>
__device__ __forceinline__ ull mass_of(uint32_t key, float xmax, float c) {
  const float a = __fmul_rn(__fsub_rn(value_of_key<T>(key), xmax), c);
  return __float2ull_rn(__builtin_amdgcn_exp2f(a) * kMassOne);
}

// Where a pass reads the row: the staged keys (lds) or global memory.
template <class T>
struct Row {
  const T* g;
  const unsigned short* lds;   // null: not staged
  int V;
  bool vec;                    // the row start is 16-byte aligned
};

// Keys of elements i .. i + 7 (i a multiple of 8, i < V); returns how many are inside the row, the
// rest read as key 0.
template <class T>
__device__ __forceinline__ int load8(const Row<T>& r, int i, uint32_t (&k)[kVec]) {
  const int n = min(kVec, r.V - i);
  if (r.lds != nullptr) {      // staged rows are padded to 8 entries
    const u16x8 v = *reinterpret_cast<const u16x8*>(r.lds + i);
#pragma unroll
    for (int j = 0; j < kVec; ++j) k[j] = v[j];
  } else if (r.vec && n == kVec) {
    const Raw8<T> raw = load_raw8(r.g + i);
    if constexpr (sizeof(T) == 2) {
      const u16x8 v = __builtin_bit_cast(u16x8, raw.v[0]);
#pragma unroll
      for (int j = 0; j < kVec; ++j) k[j] = key_of_bits<T>(v[j]);
    } else {
#pragma unroll
      for (int j = 0; j < kVec; ++j) k[j] = key_of_bits<T>(raw.v[j >> 2][j & 3]);
    }
  } else {
#pragma unroll
    for (int j = 0; j < kVec; ++j) k[j] = j < n ? key_of_bits<T>(bits_of(r.g[i + j])) : 0u;
  }
  return n;
}

struct Smem {
  unsigned hcnt[kBins * kCopies];
  ull hmass[kBins * kCopies];
  unsigned cnt0[kBins], cnt1[kBins];     // the reduced level-0 histogram, and the current deeper one
  ull mass0[kBins], mass1[kBins];
  ull wsum[kWaves];
  ull cut_mass, cut_cnt, cut_bin_mass;
  int sel;
  int tok;
};

// Exclusive prefix sum of v over the block in thread order; total: the block's sum.
__device__ __forceinline__ ull block_scan_excl(ull v, ull* wsum, ull& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  ull inc = v;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const ull up = __shfl_up(inc, o, kWave);
    if (lane >= o) inc += up;
  }
  if (lane == kWave - 1) wsum[wave] = inc;
  __syncthreads();
  ull base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const ull s = wsum[w];
    base += w < wave ? s : 0;
    tot += s;
  }
  __syncthreads();
  total = tot;
  return base + inc - v;
}

__device__ __forceinline__ ull block_max(ull v, ull* wsum) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const ull x = __shfl_xor(v, o, kWave);
    v = x > v ? x : v;
  }
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  ull r = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) r = wsum[w] > r ? wsum[w] : r;
  __syncthreads();
  return r;
}

// Count and mass per value of key digit `level` (0: the top 8 bits) over the elements whose higher
// digits equal `prefix`, into cnt / mass [kBins].
template <class T>
__device__ void build_hist(const Row<T>& r, int level, uint32_t prefix, float xmax, float c, Smem& s, unsigned* cnt,
                           ull* mass) {
  const int tid = threadIdx.x;
  for (int i = tid; i < kBins * kCopies; i += kThreads) {
    s.hcnt[i] = 0;
    s.hmass[i] = 0;
  }
  __syncthreads();
  const int shift = 8 * (levels<T>() - 1 - level);
  const int copy = tid & (kCopies - 1);
  for (int i = tid * kVec; i < r.V; i += kChunk) {
    uint32_t k[kVec];
    const int n = load8(r, i, k);
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
      if (j < n && (level == 0 || (k[j] >> ((shift + 8) & 31)) == prefix)) {
        const int slot = (int)((k[j] >> shift) & (kBins - 1)) * kCopies + copy;
        atomicAdd(&s.hcnt[slot], 1u);
        const ull m = mass_of<T>(k[j], xmax, c);
        if (m) atomicAdd(&s.hmass[slot], m);
      }
    }
  }
  __syncthreads();
  if (tid < kBins) {
    unsigned cs = 0;
    ull ms = 0;
#pragma unroll
    for (int q = 0; q < kCopies; ++q) {
      cs += s.hcnt[tid * kCopies + q];
      ms += s.hmass[tid * kCopies + q];
    }
    cnt[tid] = cs;
    mass[tid] = ms;
  }
  __syncthreads();
}

// A threshold key with the row's mass strictly above it (gt) and at or above it (ge).
struct Cut {
  uint32_t key;
  ull gt, ge;
};

// Radix select from the top digit down. by_count: the key of the target-th largest element (count
// above it < target <= count at or above it). Otherwise: the lowest key present in the row whose
// mass strictly above is < target. target >= 1, so the bin of the row maximum always qualifies.
template <class T>
__device__ Cut descend(const Row<T>& r, bool by_count, ull target, float xmax, float c, Smem& s) {
  const int tid = threadIdx.x;
  uint32_t prefix = 0;
  ull mbase = 0, cbase = 0, bin_mass = 0;
  for (int level = 0; level < levels<T>(); ++level) {
    unsigned* cnt = level == 0 ? s.cnt0 : s.cnt1;
    ull* mass = level == 0 ? s.mass0 : s.mass1;
    if (level > 0) build_hist(r, level, prefix, xmax, c, s, cnt, mass);
    if (tid == 0) s.sel = 0;
    // thread d < 256 holds bin 255 - d: thread order is descending key order
    const ull mc = tid < kBins ? cnt[kBins - 1 - tid] : 0;
    const ull mm = tid < kBins ? mass[kBins - 1 - tid] : 0;
    ull tot;
    const ull cb = cbase + block_scan_excl(mc, s.wsum, tot);
    const ull mb = mbase + block_scan_excl(mm, s.wsum, tot);
    if (mc > 0 && (by_count ? cb : mb) < target) atomicMax(&s.sel, tid);
    __syncthreads();
    const int sel = s.sel;
    if (tid == sel) {
      s.cut_cnt = cb;
      s.cut_mass = mb;
      s.cut_bin_mass = mm;
    }
    __syncthreads();
    cbase = s.cut_cnt;
    mbase = s.cut_mass;
    bin_mass = s.cut_bin_mass;
    prefix = (prefix << 8) | (uint32_t)(kBins - 1 - sel);
    __syncthreads();
  }
  return {prefix, mbase, mbase + bin_mass};   // at the last level a bin is one key value
}

template <class T>
__global__ __launch_bounds__(kThreads) void sample_kernel(const Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned short stage[];
  __shared__ Smem s;
  const int tid = threadIdx.x, b = blockIdx.x, V = a.V;
  const bool fin = a.finished != nullptr && a.finished[b] != 0;   // the same for the whole block
  int64_t tok = a.pad;
  if (!fin) {
    const T* g = reinterpret_cast<const T*>(a.logits) + (int64_t)b * a.stride;
    const Row<T> grow{g, nullptr, V, (reinterpret_cast<uintptr_t>(g) & 15) == 0};
    const bool staged = a.do_sample && sizeof(T) == 2 && V <= kStageMax;

    // ---- pass 1: (key, ~index) maximum, i.e. the largest value at its lowest index
    ull best = 0;
    for (int i = tid * kVec; i < V; i += kChunk) {
      uint32_t k[kVec];
      const int n = load8(grow, i, k);
#pragma unroll
      for (int j = 0; j < kVec; ++j) {
        const ull cand = ((ull)k[j] << 32) | (0xFFFFFFFFu - (uint32_t)(i + j));
        if (j < n && cand > best) best = cand;
      }
      if (staged) {
        u16x8 v;
#pragma unroll
        for (int j = 0; j < kVec; ++j) v[j] = (unsigned short)k[j];
        *reinterpret_cast<u16x8*>(stage + i) = v;
      }
    }
    best = block_max(best, s.wsum);     // its barriers also publish the staged keys
    const int amax = (int)(0xFFFFFFFFu - (uint32_t)best);
    tok = amax;

    if (a.do_sample) {
      const Row<T> row = staged ? Row<T>{g, stage, V, false} : grow;
      const float xmax = value_of_key<T>((uint32_t)(best >> 32)), c = a.log2e_over_t;
      build_hist(row, 0, 0u, xmax, c, s, s.cnt0, s.mass0);
      ull total;
      block_scan_excl(tid < kBins ? s.mass0[tid] : 0, s.wsum, total);

      Cut cut{0u, 0, total};                                        // keep everything
      if (a.top_k > 0 && a.top_k < V) cut = descend(row, true, (ull)a.top_k, xmax, c, s);
      if (a.top_p < 1.0) {
        const double pz = ceil(a.top_p * (double)cut.ge);          // integer G < top_p Z_k  <=>  G < ceil(..)
        const Cut cp = descend(row, false, pz < 1.0 ? 1ull : (ull)pz, xmax, c, s);
        if (cp.key > cut.key) cut = cp;
      }

      // ---- draw: the first kept index whose inclusive prefix mass exceeds R = floor(u Z)
      const ull Z = cut.ge;
      if (Z > 0) {
        const float u = fminf(fmaxf(a.u[b], 0.f), 1.f);
        ull R = (ull)((double)u * (double)Z);
        if (R >= Z) R = Z - 1;
        if (tid == 0) s.tok = amax;
        ull base = 0;
        for (int c0 = 0; c0 < V; c0 += kChunk) {
          const int i = c0 + tid * kVec;
          uint32_t k[kVec];
          ull m[kVec], sum = 0;
          const int n = i < V ? load8(row, i, k) : 0;
#pragma unroll
          for (int j = 0; j < kVec; ++j) {
            m[j] = (j < n && k[j] >= cut.key) ? mass_of<T>(k[j], xmax, c) : 0;
            sum += m[j];
          }
          ull tot;
          ull lo = base + block_scan_excl(sum, s.wsum, tot);
          if (base + tot > R) {           // the crossing is in this chunk, in exactly one thread
            if (lo <= R && R < lo + sum) {
              int at = kVec - 1;
              bool found = false;
              ull upto = lo;            // inclusive prefix through element j
#pragma unroll
              for (int j = 0; j < kVec; ++j) {
                upto += m[j];
                if (!found && upto > R) {
                  at = j;
                  found = true;
                }
              }
              s.tok = i + at;
            }
            break;
          }
          base += tot;
        }
        __syncthreads();
        tok = s.tok;
      }
    }
  }
  if (tid == 0) {
    a.tok[b] = tok;
    if (a.seq != nullptr) {
      const int64_t col = a.plen[b] + a.t;
      if (col >= 0 && col < a.S) a.seq[(int64_t)b * a.S + col] = tok;
    }
    if (a.finished != nullptr && a.eos >= 0 && tok == a.eos) a.finished[b] = 1;
  }
}

}  // namespace sample
}  // namespace smdt

using namespace smdt;

extern "C" int smdt_sample_stage_max() { return sample::kStageMax; }

extern "C" int smdt_sample_supported(int dtype, int64_t V, double temperature, double top_p) {
  return dtype >= 0 && dtype <= 2 && V >= 1 && V < sample::kMaxV && temperature > 0.0 && top_p > 0.0 && top_p <= 1.0;
}

extern "C" hipError_t smdt_sample_tokens(int dtype, const void* logits, int64_t stride, int64_t B, int64_t V,
                                         const float* u, double temperature, int64_t top_k, double top_p,
                                         int do_sample, int64_t* seq, int64_t S, const int64_t* plen, int64_t t,
                                         unsigned char* finished, int64_t eos, int64_t pad, int64_t* tok,
                                         hipStream_t st) {
  if (B < 1 || B >= (1ll << 31) || stride < V || !smdt_sample_supported(dtype, V, do_sample ? temperature : 1.0, top_p))
    return hipErrorInvalidValue;
  if ((do_sample && u == nullptr) || (seq != nullptr && plen == nullptr)) return hipErrorInvalidValue;
  sample::Args a;
  a.logits = logits;
  a.stride = stride;
  a.V = (int)V;
  a.u = u;
  a.log2e_over_t = (float)(1.4426950408889634 / (do_sample ? temperature : 1.0));
  a.top_k = top_k > 0 && top_k < V ? (int)top_k : 0;
  a.top_p = top_p;
  a.do_sample = do_sample;
  a.seq = seq;
  a.S = S;
  a.plen = plen;
  a.t = t;
  a.finished = finished;
  a.eos = eos;
  a.pad = pad;
  a.tok = tok;
  const bool staged = do_sample && dtype != 0 && V <= sample::kStageMax;
  const size_t lds = staged ? (size_t)((V + sample::kVec - 1) / sample::kVec * sample::kVec) * 2 : 0;
  // more than 64 KB of dynamic LDS has to be asked for, once per kernel
  static bool raised[3] = {false, false, false};
#define SMDT_SAMPLE(TY)                                                                                            \
  do {                                                                                                             \
    if (lds > 0 && !raised[dtype]) {                                                                               \
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&sample::sample_kernel<TY>),          \
                                               hipFuncAttributeMaxDynamicSharedMemorySize, sample::kStageMax * 2); \
      if (e != hipSuccess) return e;                                                                               \
      raised[dtype] = true;                                                                                        \
    }                                                                                                              \
    hipLaunchKernelGGL((sample::sample_kernel<TY>), dim3((unsigned)B), dim3(sample::kThreads), lds, st, a);        \
  } while (0)
  if (dtype == 0) SMDT_SAMPLE(float);
  else if (dtype == 1) SMDT_SAMPLE(bf16);
  else SMDT_SAMPLE(f16);
#undef SMDT_SAMPLE
  return hipGetLastError();
}
