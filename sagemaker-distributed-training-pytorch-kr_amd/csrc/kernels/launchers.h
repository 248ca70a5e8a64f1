// C ABI of the gfx950 kernel library. Kernel translation units (.hip) are compiled without any
// PyTorch headers (fast, torch-independent builds); `bindings.cpp` is the only file that sees
// ATen and forwards tensors + the current HIP stream to these launchers.
//
// dtype codes: 0 = fp32, 1 = bf16, 2 = fp16.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {

// layernorm.hip
int smdt_ln_bwd_nblocks(int64_t rows, int H);
hipError_t smdt_layernorm_fwd(int dtype, int wdtype, const void* x, const void* res,
                              const void* bias, const void* gamma, const void* beta, void* y,
                              void* s_out, float* mean, float* rstd, int64_t rows, int H,
                              float eps, float p_drop, uint64_t seed, uint64_t offset, int rms,
                              const void* x2, hipStream_t st);
hipError_t smdt_layernorm_bwd(int dtype, int wdtype, const void* dy, const void* ds_in,
                              const void* s, const void* gamma, const float* mean,
                              const float* rstd, void* ds_out, void* dx_out, float* partials,
                              int nblocks, float* dgamma, float* dbeta, float* dbias,
                              int64_t rows, int H, float p_drop, uint64_t seed, uint64_t offset,
                              int rms, int acc_mask, const void* dy2, hipStream_t st);

// bias_act.hip
int smdt_bias_act_slices(int64_t rows, int N);
hipError_t smdt_bias_act_fwd(int dtype, int act, const void* x, const void* bias, void* y,
                             int64_t rows, int N, hipStream_t st);
hipError_t smdt_bias_act_bwd(int dtype, int act, const void* dy, const void* x, const void* bias,
                             void* dx, float* partials, float* dbias, int64_t rows, int N,
                             int accumulate, hipStream_t st);
hipError_t smdt_col_sum(const float* partials, int nslices, int N, float* out, int accumulate,
                        hipStream_t st);
// column sums of dy [rows, N] into out[N] (fp32; accumulate = add into out)
hipError_t smdt_bias_grad(int dtype, const void* dy, int64_t rows, int N, float* partials,
                          float* out, int accumulate, hipStream_t st);
hipError_t smdt_swiglu_fwd(int dtype, const void* x, void* y, int64_t rows, int F,
                           hipStream_t st);
hipError_t smdt_swiglu_bwd(int dtype, const void* dy, const void* x, void* dx, int64_t rows,
                           int F, hipStream_t st);

// softmax.hip
hipError_t smdt_softmax_fwd(int dtype, int mode, const void* x, const uint8_t* mask, void* y,
                            int64_t rows, int sq, int sk, int heads, float scale,
                            hipStream_t st);
hipError_t smdt_softmax_bwd(int dtype, int mode, const void* dy, const void* y, void* dx,
                            int64_t rows, int sq, int sk, float scale, hipStream_t st);

// graph-safe dropout RNG (flash_attn.hip): the device step counter every dropout kernel mixes into
// its key at run time (null: none). Set by the bindings (set_rng_step), read by the launchers.
extern "C" void smdt_set_rng_step(uint32_t* counter);
extern "C" uint32_t* smdt_rng_step();

// optim.hip
hipError_t smdt_adam(float* master, const float* grad, float* m, float* v, void* model_out,
                     int model_dtype, int64_t n, float lr, float beta1, float beta2, float eps,
                     float wd, float bc1, float bc2, int adamw, const float* grad_mul,
                     const int* found_inf, const float* hyper, hipStream_t st);
int smdt_sumsq_nblocks(int64_t n);
hipError_t smdt_sumsq(int dtype, const void* x, int64_t n, float* partial, int nblocks,
                      float* out, int* found_inf, hipStream_t st);
hipError_t smdt_clip_coef(const float* sumsq, float max_norm, float inv_scale, float* mul_out,
                          float* norm_out, hipStream_t st);
hipError_t smdt_scale(int dtype, void* x, int64_t n, const float* mul, float cmul,
                      hipStream_t st);
hipError_t smdt_cast(int in_dtype, int out_dtype, const void* x, void* y, int64_t n,
                     int accumulate, hipStream_t st);

// rope.hip
hipError_t smdt_rope(int dtype, void* x, int64_t ntok, int nh, int64_t tok_stride,
                     int64_t head_stride, int rot, const float* cos_t, const float* sin_t,
                     int pos_div, int pos_mod, int backward, hipStream_t st);

// transpose.hip
hipError_t smdt_transpose16(const void* in, void* out, int64_t R, int64_t C, hipStream_t st);
// fp8_quant.hip: q[M, K] (and qt[K, M] when qt != nullptr) = fp8(clamp(x * *scale)), *amax =
// max(*amax, max |x|). bf8 = 0: E4M3 (OCP e4m3fn), 1: E5M2. K % 16 == 0; dtype bf16 / fp16.
hipError_t smdt_fp8_quantize(const void* x, void* q, void* qt, const float* scale, float* amax, int64_t M,
                             int64_t K, int dtype, int bf8, hipStream_t st);
// Delayed-scaling update of T tensors: roll hist [T, H], hist[:, 0] = amax, amax = 0,
// scale = (fmt_max / reduce(hist)) / 2^margin (kept when the reduced amax is 0 or not finite).
hipError_t smdt_fp8_update_scales(float* scale, float* hist, float* amax, const float* fmt_max, int64_t T,
                                  int64_t H, int margin, int use_max, hipStream_t st);
// mx_quant.hip: OCP MX quantisation of x [R, C] (bf16 / fp16) into one-byte elements (bf8 = 0: E4M3,
// 1: E5M2) with one E8M0 scale byte per 32 elements. Row form q [R, C], s [R, C / 32] (C % 32 ==
// 0) and / or column form qt [C, R], st [C, R / 32] with the blocks along R (R % 32 == 0, C % 16
// == 0); a null q or qt leaves that form out, both given read x once.
hipError_t smdt_mx_quantize(const void* x, void* q, void* s, void* qt, void* st, int64_t R, int64_t C, int dtype,
                            int bf8, hipStream_t st_);
// gemm_mx.hip: c [M, N] (dtype bf16 / fp16) = a [M, K] . b [N, K]^T on MX operands (a E5M2 when
// a_bf8, else E4M3; b E4M3; sa [M, K / 32], sb [N, K / 32] E8M0) (+ bias [N] of c's dtype).
// M, N, K multiples of 128. max_blocks > 0 caps the persistent grid.
int smdt_gemm_mx_supported(int64_t M, int64_t N, int64_t K);
hipError_t smdt_gemm_mx(int dtype, int a_bf8, const void* a, const void* sa, const void* b, const void* sb, void* c,
                        const void* bias, int64_t M, int64_t N, int64_t K, int max_blocks, hipStream_t st);
// link_standin.hip: paced copy standing in for a TP-pair exchange in single-GPU rank emulation
hipError_t smdt_paced_copy(const void* src, void* dst, int64_t nbytes, int blocks, int64_t ns, hipStream_t st);
// dst[r] = map[r] >= 0 ? src[map[r]] : 0 (rows of row_bytes, a multiple of 16)
hipError_t smdt_gather_rows(const void* src, const int64_t* map, void* dst, int64_t nrows, int64_t nsrc,
                            int64_t row_bytes, hipStream_t st);

// cross_entropy.hip
hipError_t smdt_ce_stats(int dtype, const void* logits, const int64_t* target, int64_t rows,
                         int V, int Vvalid, int64_t vstart, float* row_max, float* row_sumexp,
                         float* row_tgt, hipStream_t st);
hipError_t smdt_ce_bwd(int dtype, const void* logits, const int64_t* target, const float* gmax,
                       const float* gsum, const float* dloss, void* dlogits, int64_t rows, int V,
                       int Vvalid, int64_t vstart, int64_t ignore_index, hipStream_t st);
hipError_t smdt_ce_fused(int dtype, void* logits, const int64_t* target, float* loss, int64_t rows,
                         int V, int Vvalid, int64_t ignore_index, int local, int64_t vstart, hipStream_t st);

// augment.hip: per-sample depthwise filter (KS in {3, 5, 7}) and 3 x 3 median, fp32 NCHW
hipError_t smdt_aug_depthwise(const float* x, const float* k, float* y, int N, int C, int H, int W, int ks,
                              hipStream_t st);
hipError_t smdt_aug_median3(const float* x, float* y, int planes, int H, int W, hipStream_t st);

// flash_attn.hip
hipError_t smdt_flash_fwd(int dtype, const void* q, const void* k, const void* v, void* o,
                          float* lse, int B, int H, int Hkv, int S, int D, int64_t q_sb,
                          int64_t q_ss, int64_t q_sh, int64_t k_sb, int64_t k_ss, int64_t k_sh,
                          int64_t v_sb, int64_t v_ss, int64_t v_sh, int64_t o_sb, int64_t o_ss,
                          int64_t o_sh, float scale, int causal, float dropout_p, uint64_t seed,
                          uint64_t offset, hipStream_t st);
// delta: fp32 scratch of 2 x B x H x S (the backward's prepared per-query row constants).
hipError_t smdt_flash_bwd(int dtype, const void* q, const void* k, const void* v, const void* o,
                          const void* dout, const float* lse, float* delta, void* dq, void* dk,
                          void* dv, int B, int H, int Hkv, int S, int D, const int64_t* strides,
                          float scale, int causal, float dropout_p, uint64_t seed,
                          uint64_t offset, hipStream_t st);
// Per-document (block-diagonal causal) attention: doc_start[b, q] = first token of q's document,
// doc_end[b, k] = one past the last token of k's document, both int32 [B, S], non-decreasing in s.
hipError_t smdt_flash_fwd_doc(int dtype, const void* q, const void* k, const void* v, void* o,
                              float* lse, int B, int H, int Hkv, int S, int D, int64_t q_sb,
                              int64_t q_ss, int64_t q_sh, int64_t k_sb, int64_t k_ss, int64_t k_sh,
                              int64_t v_sb, int64_t v_ss, int64_t v_sh, int64_t o_sb, int64_t o_ss,
                              int64_t o_sh, float scale, float dropout_p, uint64_t seed,
                              uint64_t offset, const int* doc_start, hipStream_t st);
hipError_t smdt_flash_bwd_doc(int dtype, const void* q, const void* k, const void* v, const void* o,
                              const void* dout, const float* lse, float* delta, void* dq, void* dk,
                              void* dv, int B, int H, int Hkv, int S, int D, const int64_t* strides,
                              float scale, float dropout_p, uint64_t seed, uint64_t offset,
                              const int* doc_start, const int* doc_end, hipStream_t st);
// the backward (plain, or per-document with doc_start / doc_end) that also writes colpart, fp32
// [B * S / 128, (H + 2 Hkv) D]: per 128-token block the sums over its tokens of the fp32 dQ | dK |
// dV before their 16-bit rounding, in a fused QKV output's column order (smdt_col_sum adds the rows)
hipError_t smdt_flash_bwd_sums(int dtype, const void* q, const void* k, const void* v, const void* o,
                               const void* dout, const float* lse, float* delta, void* dq, void* dk,
                               void* dv, int B, int H, int Hkv, int S, int D, const int64_t* strides,
                               float scale, int causal, float dropout_p, uint64_t seed, uint64_t offset,
                               const int* doc_start, const int* doc_end, float* colpart, hipStream_t st);

// decode_attn.hip: incremental decoding (decode_common.h holds what the three decode files share,
// kernels and guarantees). smdt_decode_attn: out [B, nh, D] = attention of one query
// per sequence, q [B, nh, D], against k_cache / v_cache [B, cap, nkv, D] (contiguous, q's dtype:
// bf16 / fp16), keys 0 .. lens[b] - 1 (device int32 [B]); max_len <= cap only bounds the grid.
// Two launches, no atomics. Workspaces for nchunks = ceil(max_len / smdt_decode_attn_chunk()):
// ws_ml fp32 [B, nh, nchunks, 2], ws_acc fp32 [B, nh, nchunks, D]. Supported: D in {64, 128}, nh /
// nkv in {1, 2, 4, 8}; anything else returns hipErrorInvalidValue unlaunched.
int smdt_decode_attn_chunk();
int smdt_decode_attn_supported(int dtype, int D, int nh, int nkv);
hipError_t smdt_decode_attn(int dtype, const void* q, const void* k_cache, const void* v_cache, const int* lens,
                            float* ws_ml, float* ws_acc, void* out, int B, int nh, int nkv, int D, int cap,
                            int max_len, float scale, hipStream_t st);
// The second launch of smdt_decode_attn alone, over partials in its workspace layout.
hipError_t smdt_decode_attn_combine(int dtype, const float* ws_ml, const float* ws_acc, const int* lens, void* out,
                                    int B, int nh, int D, int cap, int nchunks, hipStream_t st);

// decode_attn_multi.hip: a decode step with T new tokens per sequence (speculative verification).
// smdt_decode_attn_multi: q [B, T, nh, D] against the 16-bit caches with lens[b] counting the keys
// AFTER the T appends; query t sees keys 0 .. lens[b] - T + t. The score and P V products run on
// v_mfma_f32_16x16x32 over the R = T nh / nkv query rows of a kv head. It writes partials only, in
// smdt_decode_attn's workspace layout with nh' = T nh heads per sequence and head index t nh + h
// (ws_ml fp32 [B, T nh, nchunks, 2], ws_acc fp32 [B, T nh, nchunks, D]) and finishes them with
// smdt_decode_attn_combine(nh' = T nh), which leaves out [B, T, nh, D]. Supported: bf16 /
// fp16, D in {64, 128}, nh / nkv in {1, 2, 4, 8}, 1 <= T <= smdt_decode_attn_multi_max_t().
int smdt_decode_attn_multi_max_t();
int smdt_decode_attn_multi_supported(int dtype, int D, int nh, int nkv, int T);
hipError_t smdt_decode_attn_multi(int dtype, const void* q, const void* k_cache, const void* v_cache,
                                  const int* lens, float* ws_ml, float* ws_acc, void* out, int B, int T, int nh,
                                  int nkv, int D, int cap, int max_len, float scale, hipStream_t st);
// The 16-bit RoPE-and-append, for one new token per sequence (T = 1, stride_b = (nh + 2 nkv) D) and
// for T of them. qkv: token t of sequence b at qkv + b * stride_b + t * stride_t (elements; rows of
// (nh + 2 nkv) D contiguous elements, so both [B, T, W] and the model's [T, B, W] are taken without
// a copy). Token t's q / k are rotated at pos[b] + t (device int32 [B]) over their first rot
// elements (rope.hip's arithmetic bit for bit; rot == 0: no RoPE, tables unused; cos / sin fp32
// [max_pos, rot / 2]); q -> q_out [B, T, nh, D], k / v -> cache row pos[b] + t.
hipError_t smdt_decode_rope_append_multi(int dtype, const void* qkv, int64_t stride_b, int64_t stride_t,
                                         void* q_out, void* k_cache, void* v_cache, const int* pos, int B, int T,
                                         int nh, int nkv, int D, int cap, int rot, const float* cos_t,
                                         const float* sin_t, int max_pos, hipStream_t st);

// decode_attn_mx.hip: the same two operations against an MXFP8 cache: kq / vq [B, cap, nkv, D] E4M3
// bytes, ksc / vsc [B, cap, nkv, D / 32] E8M0 bytes (mx_quant.hip's row form of every 16-bit row),
// all contiguous and 16-byte aligned. q / qkv / out stay bf16 / fp16. Attention: the limits,
// workspaces and guarantees of smdt_decode_attn. Append: D % 32 == 0 and nkv * D <= 8192 (the k and
// v rows are staged in LDS); k and v are rounded to the 16-bit dtype before they are quantised.
hipError_t smdt_decode_attn_mx(int dtype, const void* q, const void* kq, const void* ksc, const void* vq,
                               const void* vsc, const int* lens, float* ws_ml, float* ws_acc, void* out, int B,
                               int nh, int nkv, int D, int cap, int max_len, float scale, hipStream_t st);
hipError_t smdt_decode_rope_append_mx(int dtype, const void* qkv, void* q_out, void* kq, void* ksc, void* vq,
                                      void* vsc, const int* pos, int B, int nh, int nkv, int D, int cap, int rot,
                                      const float* cos_t, const float* sin_t, int max_pos, hipStream_t st);

// decode_linear.hip: weight-streaming out [M, N] = x [M, K] . W [N, K]^T (+ bias [N]) for decode steps
// (M <= smdt_decode_linear_max_m()). fmt 0: W is the 16-bit parameter (x's dtype); 1: E4M3 bytes
// [N, K] + E8M0 scales [N, K / 32] (mx_quant.hip's row form); 2: E2M1 nibbles [N, K / 2] (element
// 2 j in the low nibble of byte j) + the same scales. x / bias / out bf16 or fp16 (fmt 0), bf16
// (fmt 1, 2); N % 8 == 0, K % 32 == 0; x, W, out 16-byte aligned, ws too. smdt_decode_linear_plan
// gives the K split: with splits > 1 the caller provides ws, fp32 [splits, M, N], and a second
// launch sums it (no atomics). Anything unsupported returns hipErrorInvalidValue unlaunched.
int smdt_decode_linear_rows();
int smdt_decode_linear_max_m();
int smdt_decode_linear_split_below();
int smdt_decode_linear_step_k(int fmt);
int smdt_decode_linear_unroll(int fmt);
int smdt_decode_linear_supported(int dtype, int fmt, int64_t M, int64_t N, int64_t K);
void smdt_decode_linear_plan(int fmt, int64_t N, int64_t K, int* splits, int* slice);
hipError_t smdt_decode_linear(int dtype, int fmt, const void* x, const void* w, const void* scales, const void* bias,
                              void* out, float* ws, int64_t M, int64_t N, int64_t K, hipStream_t st);

// window_attn.hip: Swin shifted-window attention on the qkv linear's output over the padded,
// unrolled grid, qkv [B, ph, pw, 3 heads d] read as (3, heads, d); roll, window partition and head
// split are address arithmetic. table: fp32 [(2 ws - 1)^2, heads]. out [B, ph, pw, heads d] at the
// unrolled positions, lse fp32 [B, nW, heads, ws^2]. Supported: bf16 / fp16, d == 32, ws <= 8,
// ph and pw multiples of ws, 0 <= shift < ws; anything else returns hipErrorInvalidValue unlaunched.
int smdt_window_attn_supported(int dtype, int d, int ws, int ph, int pw, int shift);
hipError_t smdt_window_attn_fwd(int dtype, const void* qkv, const float* table, void* out, float* lse, int B,
                                int ph, int pw, int heads, int ws, int shift, hipStream_t st);
// partials: fp32 scratch [B nW, (2 ws - 1)^2 heads] (one row per window, summed by smdt_col_sum
// into dtable, fp32 [(2 ws - 1)^2, heads]); dqkv as qkv, every element written.
hipError_t smdt_window_attn_bwd(int dtype, const void* qkv, const float* table, const float* lse,
                                const void* dout, void* dqkv, float* partials, float* dtable, int B, int ph,
                                int pw, int heads, int ws, int shift, hipStream_t st);

// gemm_tn.hip: C[M, N] = A[M, K] . B[N, K]^T (16-bit in / out, fp32 accumulate) with an epilogue:
// epi 0 none, 1 + bias[n], 2 C = pre-activation and C2 = gelu_tanh(C + bias[n]) (bias_gelu fusion),
// 3 C = product * gelu_tanh'(aux + bias[n]) (fc2 dgrad + GeLU backward; aux = pre-activation [M, N]).
// max_blocks <= 0: one persistent workgroup per CU.
int smdt_gemm_tn_supported(int64_t M, int64_t N, int64_t K);
hipError_t smdt_gemm_tn(int dtype, int epi, const void* a, const void* b, void* c, void* c2, const void* bias,
                        const void* aux, int64_t M, int64_t N, int64_t K, int max_blocks, hipStream_t st);
// diagnostic ablations of the same kernel (benchmarks only): var bits as gemm_tn_kernel's VAR;
// bf16, epi 0, or epi 2 / 3 with the epilogue variants (8, 16, 24, 32; epi 3 also 512, 528)
hipError_t smdt_gemm_tn_var(int dtype, int epi, const void* a, const void* b, void* c, void* c2, const void* bias,
                            const void* aux, int64_t M, int64_t N, int64_t K, int max_blocks, int var,
                            hipStream_t st);
// epi 3 that also writes colpart, fp32 [M / 128, N]: per 128-row half tile the column sums of the
// fp32 output values before their 16-bit rounding (smdt_col_sum adds the rows: the fc1 bias gradient)
hipError_t smdt_gemm_tn_dgelu_sums(int dtype, const void* a, const void* b, void* c, const void* bias,
                                   const void* aux, float* colpart, int64_t M, int64_t N, int64_t K,
                                   int max_blocks, hipStream_t st);

// The grouped form (Switch MLP experts): row tile tm multiplies btab[tile_expert[tm]] ([N, K]) and
// takes its bias from biastab[tile_expert[tm]] (null with epi 0); btab / biastab ([nexp] pointers)
// and tile_expert (int32 [M / 256], -1 = unused tail tile) are device memory.
hipError_t smdt_gemm_tn_grouped(int dtype, int epi, const void* a, const void* const* btab, void* c, void* c2,
                                const void* const* biastab, const void* aux, const int* tile_expert, int nexp,
                                int64_t M, int64_t N, int64_t K, int max_blocks, hipStream_t st);
hipError_t smdt_gemm_tn_grouped_dgelu_sums(int dtype, const void* a, const void* const* btab, void* c,
                                           const void* const* biastab, const void* aux, float* colpart,
                                           const int* tile_expert, int nexp, int64_t M, int64_t N, int64_t K,
                                           int max_blocks, hipStream_t st);

// moe_route.hip: top-1 routing of logits [T, E] (dtype 0 / 1 / 2, E <= 64) into the expert-sorted,
// tile-padded layout of smdt_moe_rows(T, E) = (T / 256 + E) * 256 rows. Every word of every table is
// written; hist is int32 scratch of ceil(T / 256) * E words. Three launches, no atomics.
int64_t smdt_moe_rows(int64_t T, int64_t E);
hipError_t smdt_moe_route(int dtype, const void* logits, int64_t T, int64_t E, float* top_p, int* expert_of_token,
                          int* row_of_token, int64_t* token_of_row, int* tile_expert, int* seg, int* counts,
                          int* hist, hipStream_t st);

// wgrad_gemm.hip: main_grad[N, K] (fp32) += dy[M, N]^T . x[M, K] (bf16, or fp16 with dtype 2)
int smdt_wgrad_supported(int64_t M, int64_t N, int64_t K);
hipError_t smdt_wgrad_accumulate_t(int dtype, const void* dy, const void* x, float* main_grad, int64_t M,
                                   int64_t N, int64_t K, int max_splits, hipStream_t st);
struct SmdtWgradProblem {
  const void* dy;      // [M, N] bf16
  const void* x;       // [M, K] bf16
  float* main_grad;    // [N, K] fp32, += dy^T x
  int64_t M, N, K;
  float* bias_grad;    // [N] fp32, += column sums of dy (the linear's bias gradient), or null
  int overwrite;       // 1: main_grad holds no data yet — write dy^T x instead of adding (no read)
  // Ranged problem (null: the host M above is the range): the m range is rows [mrange[2 expert],
  // + mrange[2 expert + 1]) of dy / x, int32 words on the device (moe_route.hip's seg table); M is
  // then the row count of dy / x that bounds it. Never tail-split; a launch of their own.
  const int* mrange;
  int expert;
};
// Many independent wgrad accumulations in one launch per 32 (no split-K; only the tiles past the
// last full round add with atomics). The main_grad targets of one call must not overlap. The tail
// split is sized for `cus` concurrently usable CUs (0: 256, the whole chip).
hipError_t smdt_wgrad_grouped_cus(int dtype, const SmdtWgradProblem* probs, int n, int cus, hipStream_t st);

// wgrad_fp8.hip: main_grad[N, K] (fp32) (+)= (*inv_dy * *inv_x) * dy[M, N]^T . x[M, K] on FP8 bytes
// (the OCP encodings fp8_quant.hip writes). M % 64 == 0, N and K multiples of 16.
struct SmdtWgradFp8Problem {
  const void* dy;        // [M, N] E5M2 or E4M3 (dy_fmt), row-major
  const void* x;         // [M, K] E4M3, row-major
  float* main_grad;      // [N, K] fp32
  int64_t M, N, K;
  const float* inv_dy;   // device pointers to the dequantisation factors: read by the kernel,
  const float* inv_x;    // never by the host
  int dy_fmt;            // 0: E4M3, 1: E5M2 (the same for every problem of a call)
  int overwrite;         // 1: main_grad holds no data yet, store instead of adding (no read)
};
int smdt_wgrad_fp8_supported(int64_t M, int64_t N, int64_t K);
// Grouped launch (one per 32 problems), tail split sized for `cus` CUs (0: the whole chip). The
// main_grad targets of one call must not overlap.
hipError_t smdt_wgrad_fp8_grouped_cus(const SmdtWgradFp8Problem* probs, int n, int cus, hipStream_t st);

// xgmi_allreduce.hip: single-node all-reduce over HIP-IPC-mapped peer buffers.
int smdt_ar_max_ranks();
int smdt_ar_max_blocks();
int64_t smdt_ar_signal_bytes();
int smdt_ipc_handle_bytes();
hipError_t smdt_ipc_malloc(int64_t bytes, int uncached, void** ptr);  // zero-filled
hipError_t smdt_ipc_free(void* ptr);
hipError_t smdt_ipc_get_handle(void* ptr, void* handle_out);
hipError_t smdt_ipc_open(const void* handle, void** ptr);
hipError_t smdt_ipc_close(void* ptr);
hipError_t smdt_ar_read_error(void* sig, int* err);
int64_t smdt_ar_word_offset(int which);
// out = scale * sum over ranks of in (n elements, n * esize % 16 == 0). data_ptrs / sig_ptrs: the
// world ranks' staging (4 x region_bytes) and signal buffers. nranks_local > 1 = loopback: ranks
// rank .. rank + nranks_local - 1 in one launch, in/out strided by io_stride elements per rank.
// `blocks` is fixed per engine (every call of one engine must pass the same value).
hipError_t smdt_xgmi_allreduce(int dtype, const void* in, void* out, int64_t io_stride, int64_t n, float scale,
                               void* const* data_ptrs, void* const* sig_ptrs, int world, int rank,
                               int nranks_local, int64_t region_bytes, int two_shot, int blocks,
                               hipStream_t st);
// General form (xgmi_allreduce.hip header): mode 0 one-shot / 1 two-shot all-reduce, 2 reduce-scatter,
// 3 all-gather; in/out_rank_stride: loopback rows (elements).
hipError_t smdt_xgmi_collective(int mode, int dtype, const void* in, void* out, int64_t in_rank_stride,
                                int64_t out_rank_stride, int64_t n, int64_t slice_stride, float scale,
                                void* const* data_ptrs, void* const* sig_ptrs, int world, int rank, int nranks_local,
                                int64_t region_bytes, int blocks, hipStream_t st);

// xgmi_relay.hip: pairwise exchange of a TP pair routed over every xGMI link of the node (direct
// parts + relay parts staged in the other GPUs' buffers). stage_ptrs: world x (world x 2 x slot_bytes)
// staging buffers; partners[r] = r's TP partner; epoch = engine call counter (>= 1, same on both
// partners). n elements (n * esize % 16 == 0, 2 * ceil(n / world) vectors <= slot).
int64_t smdt_relay_signal_bytes();
int smdt_relay_max_sub();
hipError_t smdt_relay_read_error(void* sig, int* err);
int64_t smdt_relay_word_offset(int which);
hipError_t smdt_xgmi_relay(int dtype, const void* in, void* out, int64_t in_rank_stride, int64_t out_rank_stride,
                           int64_t n, void* const* stage_ptrs, void* const* sig_ptrs, const int* partners, int world,
                           int rank, int nranks_local, int64_t slot_bytes, int sub, uint32_t epoch, int dev_epoch,
                           hipStream_t st);
// zero one signal buffer's flags and device epoch (all ranks synchronised, no call in flight)
hipError_t smdt_relay_reset(void* sig, hipStream_t st);
// device epochs: advance the call counter of local ranks [rank, rank + nranks_local) by n
hipError_t smdt_relay_epoch_bump(void* const* sig_ptrs, int world, int rank, int nranks_local, uint32_t n,
                                 hipStream_t st);

}  // extern "C"
