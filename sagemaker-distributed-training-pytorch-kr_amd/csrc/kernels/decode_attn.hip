// Incremental decoding for gfx950: one new query per sequence against a growing K/V cache.
//
// The training kernels (flash_attn.hip, rope.hip) take all queries at once at S % 128 == 0. A
// decode step has ONE query row per head: the work is reading the cache once (2 S nkv D elements
// per sequence) and the launch count, not the matrix core.
//
//   smdt_decode_attn          split-KV attention of q [B, nh, D] against k / v [B, cap, nkv, D]
//   smdt_decode_attn_combine  its second launch alone, for the other decode files' partials
//
// First launch: decode_common.h's decode_attn_partial_kernel over the 16-bit cache (DecKv16), fp32
// partials per key chunk into a workspace. Second launch, here: one workgroup per (query head,
// sequence) combines the partials of the chunks that hold keys, rescaling each by
// exp(m_c - max m). The guarantees (lengths stay on the device, nothing beyond lens[b] is loaded,
// masking by selection, fixed summation order, no atomics) are stated in decode_common.h. The
// 16-bit RoPE-and-append kernel is in decode_attn_multi.hip (one token is its T = 1).
#include "decode_common.h"
#include "launchers.h"

namespace smdt {

// out[b, h, :] = sum_c w_c acc_c / sum_c w_c l_c with w_c = exp(m_c - max_c m_c) over the chunks
// that hold keys of sequence b. One thread per output column; chunks in index order.
template <typename T, int D>
__global__ __launch_bounds__(D) void decode_attn_combine_kernel(const float* __restrict__ ws_ml,
                                                                const float* __restrict__ ws_acc,
                                                                const int* __restrict__ lens,
                                                                T* __restrict__ out, int cap, int nchunks) {
  const int h = blockIdx.x, b = blockIdx.y, nh = gridDim.x, d = threadIdx.x;
  const int len = dec_clamp_len(lens[b], cap);
  int nc = (len + kDecChunk - 1) / kDecChunk;
  nc = nc > nchunks ? nchunks : nc;
  const int64_t p0 = dec_part((int64_t)b * nh + h, nchunks, 0);
  float M = -INFINITY;
  for (int c = 0; c < nc; ++c) {
    const float mc = ws_ml[(p0 + c) * 2], lc = ws_ml[(p0 + c) * 2 + 1];
    if (lc > 0.f) M = fmaxf(M, mc);
  }
  float num = 0.f, den = 0.f;
  for (int c = 0; c < nc; ++c) {
    const float mc = ws_ml[(p0 + c) * 2], lc = ws_ml[(p0 + c) * 2 + 1];
    if (lc > 0.f) {       // an empty partial (m = -inf, l = 0) is skipped, never multiplied
      const float w = __expf(mc - M);
      num += w * ws_acc[(p0 + c) * D + d];
      den += w * lc;
    }
  }
  out[((int64_t)b * nh + h) * D + d] = from_f32<T>(den > 0.f ? num / den : 0.f);
}

}  // namespace smdt

using namespace smdt;

extern "C" int smdt_decode_attn_chunk() { return kDecChunk; }

extern "C" int smdt_decode_attn_supported(int dtype, int D, int nh, int nkv) {
  if (dtype != 1 && dtype != 2) return 0;
  if (D != 64 && D != 128) return 0;
  if (nh <= 0 || nkv <= 0 || nh % nkv) return 0;
  const int g = nh / nkv;
  return g == 1 || g == 2 || g == 4 || g == 8;
}

extern "C" hipError_t smdt_decode_attn(int dtype, const void* q, const void* k_cache, const void* v_cache,
                                       const int* lens, float* ws_ml, float* ws_acc, void* out, int B, int nh,
                                       int nkv, int D, int cap, int max_len, float scale, hipStream_t st) {
  const int nchunks = dec_nchunks(B, nkv, cap, max_len);
  if (!smdt_decode_attn_supported(dtype, D, nh, nkv) || nchunks == 0) return hipErrorInvalidValue;
  const hipError_t e = dec_dispatch(dtype, D, [&](auto tag, auto d) {
    using T = typename decltype(tag)::type;
    const DecKv16<T> kc{(const T*)k_cache}, vc{(const T*)v_cache};
    return decode_attn_partial_launch<T, decltype(d)::value>(q, kc, vc, lens, ws_ml, ws_acc, B, nh, nkv, cap, nchunks,
                                                             scale, st);
  });
  if (e != hipSuccess) return e;
  return smdt_decode_attn_combine(dtype, ws_ml, ws_acc, lens, out, B, nh, D, cap, nchunks, st);
}

extern "C" hipError_t smdt_decode_attn_combine(int dtype, const float* ws_ml, const float* ws_acc, const int* lens,
                                               void* out, int B, int nh, int D, int cap, int nchunks, hipStream_t st) {
  if (B <= 0 || B > 65535 || nh <= 0 || cap <= 0 || nchunks <= 0) return hipErrorInvalidValue;
  return dec_dispatch(dtype, D, [&](auto tag, auto d) {
    using T = typename decltype(tag)::type;
    constexpr int kD = decltype(d)::value;
    hipLaunchKernelGGL((decode_attn_combine_kernel<T, kD>), dim3((unsigned)nh, (unsigned)B), dim3(kD), 0, st, ws_ml,
                       ws_acc, lens, (T*)out, cap, nchunks);
    return hipGetLastError();
  });
}
