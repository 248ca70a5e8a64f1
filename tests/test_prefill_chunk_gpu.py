"""Chunked / prefix-cached prefill on the MI355X: prefill_attn.hip, its append, ``forward_chunk`` and
``generate(prefill_chunk=..., cached_prefix=...)``.

The attention kernel is judged as ``test_speculative_gpu`` judges the multi-token kernel
(``_numerics.flash_excess`` against float64 and the twin that places the kernel's rounding points),
the append bit for bit against T single-token calls, the model hooks by the 2 x rule against the
fp32 model, and ``generate`` by token equality with the plain call (or an fp32 tie)."""
import math

import pytest
import torch

from _numerics import flash_excess
from smdt_amd.ops import _ext
from smdt_amd.ops import functional as SF
from test_generation_gpu import FORMS, _pair, _ragged_prompt
from test_speculative_gpu import _assert_tokens_or_fp32_tie

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
# (pos, new tokens per row) of the three sequences
PATTERNS = {
    "fresh": lambda T: ([0, 0, 0], [T, T, T]),              # query 0 sees one key
    "edge": lambda T: ([63, 64, 65], [T, T, T]),            # the diagonal straddles a 64-key tile edge
    "ragged": lambda T: ([200, 7, 50], [T, 1, 0]),          # a full row, a single new token, none
}


def _operands(dtype, D, nh, nkv, T, pos, new, seed):
    """q, caches of capacity max(pos) + T with NaN in every row at or beyond lens[b], pos, lens."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    cap = max(pos) + T
    q = torch.randn(3, T, nh, D, device="cuda", generator=g).to(dtype)
    k = torch.randn(3, cap, nkv, D, device="cuda", generator=g).to(dtype)
    v = torch.randn(3, cap, nkv, D, device="cuda", generator=g).to(dtype)
    lens = [p + n for p, n in zip(pos, new)]
    for b, n in enumerate(lens):
        k[b, n:] = float("nan")
        v[b, n:] = float("nan")
    i32 = dict(dtype=torch.int32, device="cuda")
    return q, k, v, torch.tensor(pos, **i32), torch.tensor(lens, **i32)


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("T", [9, 40, 130])
@pytest.mark.parametrize("nh,nkv", [(4, 4), (8, 2), (8, 1), (4, 2)])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_prefill_attention_against_float64(dtype, D, nh, nkv, T, pattern):
    pos, new = PATTERNS[pattern](T)
    q, k, v, pos_t, lens_t = _operands(dtype, D, nh, nkv, T, pos, new, D + 7 * nh + 13 * nkv + 31 * T + len(pattern))
    scale = 1.0 / math.sqrt(D)
    ref = SF.prefill_attention_ref(q.double(), k.double(), v.double(), pos_t, lens_t, scale)
    emu = SF.prefill_attention_ref(q, k, v, pos_t, lens_t, scale, emulate=True)
    out = SF.prefill_attention(q, k, v, pos_t, lens_t, scale)
    assert out.shape == q.shape and out.dtype == q.dtype
    ratio, e_k, e_e = flash_excess(out, emu, ref, dtype)
    print(f"prefill_attention row-relative err: kernel {e_k:.3e} emulation {e_e:.3e} kernel/bound {ratio:.3f}")
    assert ratio <= 1.0, (ratio, e_k, e_e)
    assert torch.isfinite(out).all()
    for b, n in enumerate(new):          # padding rows: exact zeros
        assert out[b, n:].abs().sum() == 0
    if pattern == "fresh":               # query 0 sees a lone key: its output is that v row exactly
        assert torch.equal(out[:, 0].view(3, nkv, nh // nkv, D), v[:, 0].unsqueeze(2).expand(3, nkv, nh // nkv, D))


def test_future_blind_and_repeatable():
    """Other finite values in the cache rows of the new tokens after t leave the bits of the
    queries up to t unchanged, and two calls give equal bits."""
    T, D, nh, nkv = 40, 128, 8, 2
    pos, new = [63, 64, 0], [T, T, T]
    q, k, v, pos_t, lens_t = _operands(torch.bfloat16, D, nh, nkv, T, pos, new, 17)
    out = SF.prefill_attention(q, k, v, pos_t, lens_t, 0.09)
    assert torch.equal(SF.prefill_attention(q, k, v, pos_t, lens_t, 0.09), out)
    g = torch.Generator(device="cuda").manual_seed(18)
    for t in (0, 7, 31, T - 2):
        k2, v2 = k.clone(), v.clone()
        for b, p in enumerate(pos):
            k2[b, p + t + 1:p + T] = (37.0 * torch.randn(T - t - 1, nkv, D, device="cuda", generator=g)).to(k.dtype)
            v2[b, p + t + 1:p + T] = (37.0 * torch.randn(T - t - 1, nkv, D, device="cuda", generator=g)).to(k.dtype)
        again = SF.prefill_attention(q, k2, v2, pos_t, lens_t, 0.09)
        assert torch.equal(again[:, :t + 1], out[:, :t + 1]), t
        assert not torch.equal(again[:, t + 1:], out[:, t + 1:])


@pytest.mark.parametrize("rot", [64, None], ids=["rope", "norope"])
@pytest.mark.parametrize("seq_first", [False, True], ids=["bt", "tb"])
def test_prefill_rope_append_bitwise(seq_first, rot):
    """The bytes of T calls of ``decode_rope_append`` at pos + t for every row below lens (q and
    both caches); everything else in the caches is untouched and a padding token's q is zeros. Row 1
    is ragged: its padding would fall beyond the capacity."""
    B, T, cap, nh, nkv, D, dtype = 3, 40, 64, 4, 2, 64, torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(7)
    W = (nh + 2 * nkv) * D
    qkv = torch.randn(T, B, W, device="cuda", generator=g).to(dtype).transpose(0, 1) if seq_first else \
        torch.randn(B, T, W, device="cuda", generator=g).to(dtype)
    pos, new = [0, cap - 9, 17], [T, 9, 3]
    pos_t = torch.tensor(pos, dtype=torch.int32, device="cuda")
    lens_t = torch.tensor([p + n for p, n in zip(pos, new)], dtype=torch.int32, device="cuda")
    kc = torch.randn(B, cap, nkv, D, device="cuda", generator=g).to(dtype)
    vc = torch.randn(B, cap, nkv, D, device="cuda", generator=g).to(dtype)
    k1, v1 = kc.clone(), vc.clone()
    rope = None if rot is None else SF.rope_tables(cap, rot, device="cuda") + (rot,)
    want = torch.zeros(B, T, nh, D, device="cuda", dtype=dtype)
    for b in range(B):                   # one sequence at a time: only its real tokens are appended
        for t in range(new[b]):
            want[b, t] = SF.decode_rope_append(qkv[b:b + 1, t].contiguous(), k1[b:b + 1], v1[b:b + 1],
                                               pos_t[b:b + 1] + t, nh, nkv, D, rope=rope)[0]
    got = SF.prefill_rope_append(qkv, kc, vc, pos_t, lens_t, nh, nkv, D, rope=rope)
    assert got.shape == (B, T, nh, D) and torch.equal(got, want)
    assert torch.equal(kc, k1) and torch.equal(vc, v1)


def test_refused_operands_raise():
    def ops(nh, nkv, D, dtype):
        q = torch.zeros(2, 9, nh, D, device="cuda", dtype=dtype)
        kc = torch.zeros(2, 16, nkv, D, device="cuda", dtype=dtype)
        return q, kc, kc.clone(), torch.full((2,), 7, dtype=torch.int32, device="cuda")
    code = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
    for nh, nkv, D, dtype in [(4, 4, 96, torch.bfloat16), (6, 2, 64, torch.bfloat16), (4, 4, 64, torch.float32)]:
        q, kc, vc, pl = ops(nh, nkv, D, dtype)
        assert not SF.prefill_attention_supported(q, kc, vc)
        assert not _ext.ext().prefill_attn_supported(code[dtype], D, nh, nkv)
        with pytest.raises((RuntimeError, ValueError)):
            SF.prefill_attention(q, kc, vc, pl, pl + 9, 0.125)
    q, kc, vc, pl = ops(4, 4, 64, torch.bfloat16)
    assert SF.prefill_attention_supported(q, kc, vc) and _ext.ext().prefill_attn_supported(1, 64, 4, 4)
    k8 = kc.to(torch.float8_e4m3fn)                                  # an MXFP8 cache's element tensors
    assert not SF.prefill_attention_supported(q, k8, k8.clone())
    with pytest.raises(RuntimeError, match="MXFP8"):
        SF.prefill_attention(q, k8, k8.clone(), pl, pl + 9, 0.125)


# ------------------------------------------------------------------------------- the model hooks
@pytest.mark.parametrize("form", sorted(FORMS))
def test_forward_chunk_as_close_to_fp32_as_forward_prefill(form):
    """The ragged prompt in pieces of 4 (the rows end in different pieces) against one
    ``forward_prefill``: the last-token logits and the written K / V rows may be at most 2 x as far
    from the fp32 model's as ``forward_prefill``'s are."""
    from smdt_amd.models.generation import KVCache, _prefill_pieces
    ref, gpu = _pair(form)
    ids, mask = _ragged_prompt()
    plen = mask.sum(1)
    with torch.no_grad():
        c32 = KVCache(ref.cfg, 2, 16, torch.float32)
        want = ref.forward_prefill(ids, plen, c32)[:, :500]
        c0, c1 = (KVCache(gpu.cfg, 2, 16, torch.bfloat16, "cuda") for _ in range(2))
        full = gpu.forward_prefill(ids.cuda(), plen.cuda(), c0).float().cpu()[:, :500]
        chunked = _prefill_pieces(gpu, ids.cuda(), plen.cuda(), c1, 4, [0, 0]).float().cpu()[:, :500]
    e_f, e_c = (full - want).abs().max().item(), (chunked - want).abs().max().item()
    print(f"{form}: max logit error vs fp32: chunked prefill {e_c:.4e}, forward_prefill {e_f:.4e}")
    assert e_c <= 2 * e_f, (e_c, e_f)
    for name in ("k", "v"):              # the rows below plen of every layer's cache
        def err(c):
            return max((getattr(c, name)[i][b, :int(plen[b])].float().cpu() - getattr(c32, name)[i][b, :int(plen[b])])
                       .abs().max().item() for i in range(gpu.cfg.num_layers) for b in range(2))
        k_c, k_f = err(c1), err(c0)
        print(f"{form}: max {name} cache error vs fp32: chunked prefill {k_c:.4e}, forward_prefill {k_f:.4e}")
        assert k_c <= 2 * k_f, (name, k_c, k_f)


def test_forward_chunk_refuses_an_mx_cache():
    from smdt_amd.models.generation import KVCache
    _, gpu = _pair("llama")
    cache = KVCache(gpu.cfg, 2, 32, torch.bfloat16, "cuda", format="mxfp8")
    with torch.no_grad(), pytest.raises(NotImplementedError, match="mxfp8"):
        gpu.forward_chunk(torch.zeros(2, 9, dtype=torch.long, device="cuda"), cache)


# ------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("case", ["chunk", "prefix", "both"])
def test_generate_returns_the_plain_tokens(case):
    from smdt_amd.models.generation import KVCache, generate
    _, gpu = _pair("llama")
    ids, mask = _ragged_prompt()
    ids, mask = ids.cuda(), mask.cuda()
    kw = dict(max_new_tokens=22, eos_token_id=None)
    plain = generate(gpu, ids, mask, **kw)
    if case != "chunk":                  # a first call fills the cache the second one names rows of
        cache = KVCache(gpu.cfg, 2, 11 + 22, torch.bfloat16, "cuda")
        generate(gpu, ids, mask, cache=cache, **kw)
        kw.update(cache=cache, cached_prefix=[3, 5])
    if case != "prefix":
        kw.update(prefill_chunk=4)
    got = generate(gpu, ids, mask, **kw)
    _assert_tokens_or_fp32_tie(got, plain, ids, mask, case)
    if case == "both":
        assert torch.equal(generate(gpu, ids, mask, use_graph=True, **kw), got)


def test_generate_refusals():
    from smdt_amd.models.generation import KVCache, generate
    _, gpu = _pair("llama")
    ids, mask = _ragged_prompt()
    ids, mask = ids.cuda(), mask.cuda()
    cache = KVCache(gpu.cfg, 2, 16, torch.bfloat16, "cuda")
    with pytest.raises(NotImplementedError, match="draft model"):
        generate(gpu, ids, mask, max_new_tokens=4, prefill_chunk=4, draft_model=gpu)
    with pytest.raises(NotImplementedError, match="kv_cache_format"):
        generate(gpu, ids, mask, max_new_tokens=4, prefill_chunk=4, kv_cache_format="mxfp8")
    with pytest.raises(ValueError, match="needs cache="):
        generate(gpu, ids, mask, max_new_tokens=4, cached_prefix=2)
    with pytest.raises(ValueError, match="at least one new token"):
        generate(gpu, ids, mask, max_new_tokens=4, cache=cache, cached_prefix=[5, 5])
