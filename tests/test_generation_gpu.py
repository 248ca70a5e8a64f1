"""Incremental decoding on the MI355X: decode_attn.hip against float64, its RoPE-and-append kernel
against the ``rope_`` kernel bit for bit, and ``generate`` end to end (teacher-forced logits, graph
replay, no host synchronisation in the decode steps).

Tolerances are measured, not chosen: the kernel's max error against a float64 reference built from
the same 16-bit inputs must be at most 2x the error of the 16-bit torch twin on the same inputs
(both round the output once; the factor covers summation order), the rule of
tests/test_swin_window_attn_gpu.py."""
import math

import pytest
import torch

from smdt_amd.ops import _ext
from smdt_amd.ops import functional as SF

pytestmark = pytest.mark.gpu

C = SF.DECODE_CHUNK
DTYPES = [torch.bfloat16, torch.float16]
HEADS = [(4, 4), (8, 2), (8, 1), (4, 2)]
LENS = {"ones": ([1, 1, 1], 2 * C), "edge": ([C - 1, C, C + 1], 2 * C), "mixed": ([1, 2 * C + 37, 4 * C], 4 * C)}


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _nan_tail(k, v, lens):
    for b, n in enumerate(lens):
        k[b, n:] = float("nan")
        v[b, n:] = float("nan")


def _check_2x(q, k, v, lens_t, scale, max_len=None):
    """Print, then assert: kernel error <= 2 x twin error, both against float64 of the same inputs."""
    ref = SF.decode_attention_ref(q.double(), k.double(), v.double(), lens_t, scale)
    twin = SF.decode_attention_ref(q, k, v, lens_t, scale)
    out = SF.decode_attention(q, k, v, lens_t, scale, max_len=max_len)
    assert out.shape == q.shape and out.dtype == q.dtype
    assert torch.isfinite(out).all()
    e_k = (out.double() - ref).abs().max().item()
    e_t = (twin.double() - ref).abs().max().item()
    print(f"decode_attention max err: kernel {e_k:.3e} twin {e_t:.3e} (ref max {ref.abs().max().item():.3e})")
    assert e_k <= 2 * e_t, (e_k, e_t)
    return out


def test_chunk_length_exported():
    assert _ext.ext().decode_attn_chunk() == C


@pytest.mark.parametrize("pattern", sorted(LENS))
@pytest.mark.parametrize("nh,nkv", HEADS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_decode_attention_against_float64(dtype, D, nh, nkv, pattern):
    lens, cap = LENS[pattern]
    g = _gen(D + 7 * nh + 13 * nkv + len(pattern))
    q = torch.randn(3, nh, D, device="cuda", generator=g).to(dtype)
    k = torch.randn(3, cap, nkv, D, device="cuda", generator=g).to(dtype)
    v = torch.randn(3, cap, nkv, D, device="cuda", generator=g).to(dtype)
    _nan_tail(k, v, lens)
    lens_t = torch.tensor(lens, dtype=torch.int32, device="cuda")
    out = _check_2x(q, k, v, lens_t, 1.0 / math.sqrt(D))
    if pattern == "ones":            # a lone key: the output is its v row exactly
        assert torch.equal(out.view(3, nkv, nh // nkv, D), v[:, 0].unsqueeze(2).expand(3, nkv, nh // nkv, D))
    # a grid bound below the capacity gives the same bits
    if max(lens) < cap:
        again = SF.decode_attention(q, k, v, lens_t, 1.0 / math.sqrt(D), max_len=max(lens))
        assert torch.equal(again, out)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_large_scores_max_in_last_chunk(dtype):
    """Raw logits span about +-200; most of the large scores sit in the first chunk and the maximum
    in the last: a kernel that skips the cross-chunk rescale, or exponentiates before subtracting
    the maximum, is far off (or not finite)."""
    D, nh, nkv, cap = 64, 8, 2, 4 * C
    g = _gen(11)
    scale = 1.0 / math.sqrt(D)
    e = torch.randn(3, nkv, D, device="cuda", generator=g).sign()                  # a +-1 direction per kv head
    q = (e * 2.0).repeat_interleave(nh // nkv, dim=1)                              # q . e = 2 D
    target = torch.empty(3, cap, nkv, device="cuda").uniform_(-200.0, 0.0, generator=g)
    target[:, :C] = torch.empty(3, C, nkv, device="cuda").uniform_(190.0, 199.0, generator=g)
    target[:, -3] = 200.0                                                          # the maximum: last chunk
    k = target.unsqueeze(-1) * e.unsqueeze(1) / (2.0 * D * scale)
    k = k + 0.01 * torch.randn(3, cap, nkv, D, device="cuda", generator=g)
    v = torch.randn(3, cap, nkv, D, device="cuda", generator=g)
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    lens = [cap, cap, cap - 1]
    _nan_tail(k, v, lens)
    lens_t = torch.tensor(lens, dtype=torch.int32, device="cuda")
    s = torch.einsum("bhd,bckd->bhck", q.double(), k[:, :cap - 1].double().nan_to_num()) * scale
    assert s.max() > 150 and s.min() < -150
    _check_2x(q, k, v, lens_t, scale)


def test_bitwise_repeatable():
    g = _gen(5)
    q = torch.randn(4, 8, 128, device="cuda", generator=g).bfloat16()
    k = torch.randn(4, 3 * C + 5, 2, 128, device="cuda", generator=g).bfloat16()
    v = torch.randn(4, 3 * C + 5, 2, 128, device="cuda", generator=g).bfloat16()
    lens_t = torch.tensor([3 * C + 5, 7, C + 1, 2 * C], dtype=torch.int32, device="cuda")
    a = SF.decode_attention(q, k, v, lens_t, 0.1)
    b = SF.decode_attention(q, k, v, lens_t, 0.1)
    assert torch.equal(a, b)


@pytest.mark.parametrize("nh,nkv,D,rot", [(4, 2, 64, 64), (16, 4, 128, 128), (4, 4, 64, 32), (12, 12, 64, None)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_decode_rope_append_bitwise(dtype, nh, nkv, D, rot):
    """q / k bytes equal the ``rope_`` kernel's for the same rows at pos[b] (both of its forms: the
    grid-stride one and the token-per-block one it takes from 64 head groups up), v is copied, no
    other cache row changes; without RoPE the op is a copy."""
    B, cap = 4, 40
    g = _gen(7)
    qkv = torch.randn(B, (nh + 2 * nkv) * D, device="cuda", generator=g).to(dtype)
    pos = torch.tensor([0, cap - 1, 17, 5], dtype=torch.int32, device="cuda")
    kc = torch.randn(B, cap, nkv, D, device="cuda", generator=g).to(dtype)
    vc = torch.randn(B, cap, nkv, D, device="cuda", generator=g).to(dtype)
    k0, v0 = kc.clone(), vc.clone()
    rope = None
    want_qk = qkv[:, :(nh + nkv) * D].reshape(B, nh + nkv, D).clone()
    if rot is not None:
        cos, sin = SF.rope_tables(cap, rot, device="cuda")
        rope = (cos, sin, rot)
        for b in range(B):           # the existing kernel on a [cap] sequence holding the row at pos[b]
            x = torch.zeros(cap, nh + nkv, D, device="cuda", dtype=dtype)
            x[int(pos[b])] = want_qk[b]
            _ext.ext().rope_(x, cos, sin, rot, 1, cap, False)
            want_qk[b] = x[int(pos[b])]
    q = SF.decode_rope_append(qkv, kc, vc, pos, nh, nkv, D, rope=rope)
    assert q.shape == (B, nh, D) and torch.equal(q, want_qk[:, :nh])
    want_v = qkv[:, (nh + nkv) * D:].reshape(B, nkv, D)
    for b in range(B):
        p = int(pos[b])
        assert torch.equal(kc[b, p], want_qk[b, nh:])
        assert torch.equal(vc[b, p], want_v[b])
        k0[b, p], v0[b, p] = kc[b, p], vc[b, p]
    assert torch.equal(kc, k0) and torch.equal(vc, v0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_decode_rope_append_of_a_slice(dtype):
    """A [B, W] slice with a non-zero, 16-byte aligned storage offset gives the bytes of its
    contiguous clone: one token is the strided T-token kernel at T = 1, stride W."""
    nh, nkv, D, rot, B, cap = 4, 2, 64, 64, 4, 40
    g = _gen(9)
    big = torch.randn(B + 2, (nh + 2 * nkv) * D, device="cuda", generator=g).to(dtype)
    part = big[1:1 + B]
    assert part.storage_offset() > 0 and part.data_ptr() % 16 == 0 and part.is_contiguous()
    pos = torch.tensor([0, cap - 1, 17, 5], dtype=torch.int32, device="cuda")
    rope = (*SF.rope_tables(cap, rot, device="cuda"), rot)
    kc = torch.randn(B, cap, nkv, D, device="cuda", generator=g).to(dtype)
    vc = torch.randn(B, cap, nkv, D, device="cuda", generator=g).to(dtype)
    k1, v1 = kc.clone(), vc.clone()
    want = SF.decode_rope_append(part.clone(), k1, v1, pos, nh, nkv, D, rope=rope)
    got = SF.decode_rope_append(part, kc, vc, pos, nh, nkv, D, rope=rope)
    assert got.shape == (B, nh, D) and torch.equal(got, want)
    assert torch.equal(kc, k1) and torch.equal(vc, v1)


def test_refused_shapes_raise():
    def ops(nh, nkv, D, dtype):
        q = torch.zeros(2, nh, D, device="cuda", dtype=dtype)
        kc = torch.zeros(2, 16, nkv, D, device="cuda", dtype=dtype)
        return q, kc, kc.clone(), torch.ones(2, dtype=torch.int32, device="cuda")
    for nh, nkv, D, dtype in [(4, 4, 96, torch.bfloat16), (6, 4, 64, torch.bfloat16), (4, 4, 64, torch.float32),
                              (12, 4, 64, torch.float16)]:
        q, kc, vc, lens = ops(nh, nkv, D, dtype)
        assert not SF.decode_attention_supported(q, kc, vc)
        code = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}[dtype]      # the launcher agrees
        assert not _ext.ext().decode_attn_supported(code, D, nh, nkv)
        with pytest.raises((RuntimeError, ValueError)):
            SF.decode_attention(q, kc, vc, lens, 0.125)
    q, kc, vc, lens = ops(4, 4, 64, torch.bfloat16)
    assert SF.decode_attention_supported(q, kc, vc) and _ext.ext().decode_attn_supported(1, 64, 4, 4)
    with pytest.raises(ValueError):
        SF.decode_attention(q, kc, vc, lens, 0.125, max_len=17)
    with pytest.raises(RuntimeError):
        SF.decode_rope_append(torch.zeros(2, 12 * 64, device="cuda"), kc.float(), vc.float(), lens, 4, 4, 64)


# ------------------------------------------------------------------------------- end to end
FORMS = {
    "llama": dict(num_layers=2, hidden_size=256, num_attention_heads=4, num_query_groups=2,
                  activation="swiglu", normalization="RMSNorm", position_embedding_type="rope",
                  add_bias_linear=False, untie_embeddings_and_output_weights=True, layernorm_epsilon=1e-6),
    "opt": dict(num_layers=2, hidden_size=256, num_attention_heads=4, activation="relu",
                position_embedding_type="learned_absolute", position_offset=2),
}
_PAIRS = {}


def _pair(form):
    """(fp32 CPU model, bf16 GPU model) with the same (bf16-representable) weights, built once."""
    if form not in _PAIRS:
        from smdt_amd.models.gpt import GPTModel
        from smdt_amd.models.transformer import TransformerConfig
        from smdt_amd.parallel import state as ps
        ps.destroy_model_parallel()
        kw = dict(FORMS[form], max_position_embeddings=128, padded_vocab_size=512, hidden_dropout=0.0,
                  attention_dropout=0.0, seed=3)
        ref = GPTModel(TransformerConfig(**kw, params_dtype=torch.float32)).eval()
        gpu = GPTModel(TransformerConfig(**kw, params_dtype=torch.bfloat16), device="cuda").eval()
        with torch.no_grad():
            for pr, pg in zip(ref.parameters(), gpu.parameters()):
                pg.copy_(pr.to(torch.bfloat16))
                pr.copy_(pg.float().cpu())
        ref.loss_vocab_size = gpu.loss_vocab_size = 500
        _PAIRS[form] = (ref, gpu)
    return _PAIRS[form]


def _ragged_prompt():
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(3, 500, (2, 11), generator=g)
    mask = torch.ones(2, 11, dtype=torch.long)
    mask[0, 5:] = 0
    return ids, mask


@pytest.mark.parametrize("form", sorted(FORMS))
def test_cached_logits_as_close_to_fp32_as_full_forward(form):
    """Teacher-forced with the fp32 model's own greedy tokens for 12 steps from a ragged two-row
    prompt: the cached path's per-step logits may be at most 2x as far from the fp32 logits as the
    16-bit full forward's. Token equality is not asserted in 16 bits."""
    from smdt_amd.models.generation import KVCache, generate
    ref, gpu = _pair(form)
    ids, mask = _ragged_prompt()
    steps = 12
    seq = generate(ref, ids, mask, max_new_tokens=steps, eos_token_id=None)               # fp32 path
    plen = mask.sum(1)
    with torch.no_grad():
        cache = KVCache(gpu.cfg, 2, 11 + steps, torch.bfloat16, "cuda")
        cached = [gpu.forward_prefill(ids.cuda(), plen.cuda(), cache)]
        cache.lens.copy_(plen)
        for t in range(steps - 1):
            tok = torch.stack([seq[b, plen[b] + t] for b in range(2)]).cuda()
            cache.advance()
            cached.append(gpu.forward_decode(tok, cache))
        cached = torch.stack(cached, 1).float().cpu()[..., :500]                        # [2, steps, V]
        e_c = e_f = 0.0
        for b in range(2):
            n = int(plen[b])
            row = seq[b:b + 1, :n + steps - 1]
            want = ref(row)[0, n - 1:, :500]                                              # [steps, V] fp32
            full = gpu(row.cuda())[0, n - 1:, :500].float().cpu()
            e_c = max(e_c, (cached[b] - want).abs().max().item())
            e_f = max(e_f, (full - want).abs().max().item())
    print(f"{form}: max logit error vs fp32: cached {e_c:.4e}, full forward {e_f:.4e}")
    assert e_c <= 2 * e_f, (e_c, e_f)


@pytest.mark.parametrize("sample", [False, True], ids=["greedy", "sampled"])
def test_graph_replay_returns_the_eager_tokens(sample):
    from smdt_amd.models.generation import generate
    _, gpu = _pair("llama")
    ids, mask = _ragged_prompt()
    ids, mask = ids.cuda(), mask.cuda()
    kw = dict(max_new_tokens=20, eos_token_id=None, do_sample=sample, temperature=0.9, top_k=50, top_p=0.95)
    eager = generate(gpu, ids, mask, generator=_gen(21), **kw)
    graph = generate(gpu, ids, mask, generator=_gen(21), use_graph=True, **kw)
    again = generate(gpu, ids, mask, generator=_gen(21), use_graph=True, **kw)           # recaptures
    assert torch.equal(eager, graph) and torch.equal(eager, again)
    assert int(eager.max()) < 500


@pytest.mark.parametrize("form", sorted(FORMS))
def test_decode_steps_do_not_synchronise(form):
    from smdt_amd.models.generation import KVCache
    _, gpu = _pair(form)
    ids, mask = _ragged_prompt()
    ids, plen = ids.cuda(), mask.sum(1).cuda()
    with torch.no_grad():
        cache = KVCache(gpu.cfg, 2, 32, torch.bfloat16, "cuda")
        tok = gpu.forward_prefill(ids, plen, cache)[:, :500].argmax(-1)
        cache.lens.copy_(plen)
        cache.advance()
        gpu.forward_decode(tok, cache)                       # first use of every shape, outside the check
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for _ in range(8):
                cache.advance()
                tok = gpu.forward_decode(tok, cache)[:, :500].argmax(-1)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert int(cache.lens[0]) == int(plen[0]) + 9 and tok.shape == (2,)
