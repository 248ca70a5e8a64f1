"""MXFP8 K/V cache on the MI355X: decode_attn_mx.hip's attention against float64, its quantising
append and the prefill store against their torch twins byte for byte, and
``generate(kv_cache_format="mxfp8")`` end to end (teacher-forced logits, graph replay, no host
synchronisation, together with a weight format).

Tolerances are measured, not chosen, by the rule of tests/test_generation_gpu.py: the kernel's max
error against a float64 reference built from the same (exactly dequantised) inputs must be at most
2x the error of the fp32 torch twin on the same inputs; the factor covers summation order."""
import math

import pytest
import torch

from smdt_amd.ops import functional as SF

pytestmark = pytest.mark.gpu

C = SF.DECODE_CHUNK
DTYPES = [torch.bfloat16, torch.float16]
HEADS = [(4, 4), (8, 2), (8, 1), (4, 2)]
LENS = {"ones": ([1, 1, 1], 2 * C), "edge": ([C - 1, C, C + 1], 2 * C), "mixed": ([1, 2 * C + 37, 4 * C], 4 * C)}


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _quantise(x):
    """MXFP8 cache tensors (q, s) of x [B, cap, nkv, D] (bf16): the twin's bytes."""
    D = x.shape[-1]
    q, s = SF.mx_quantize_ref(x.reshape(-1, D), "e4m3")
    return q.view(x.shape), s.view(*x.shape[:-1], D // 32)


def _random_cache(B, cap, nkv, D, g):
    """randn times a per-block power of two from 2^-12 .. 2^8: scales differ between blocks and lanes."""
    e = torch.randint(-12, 9, (B, cap, nkv, D // 32, 1), device="cuda", generator=g).float()
    x = torch.randn(B, cap, nkv, D // 32, 32, device="cuda", generator=g) * torch.exp2(e)
    return _quantise(x.reshape(B, cap, nkv, D).bfloat16())


def _nan_tail(lens, *pairs):
    """Unused rows: NaN element bytes (0x7F) and the E8M0 NaN (0xFF) as their scale."""
    for q, s in pairs:
        for b, n in enumerate(lens):
            q.view(torch.uint8)[b, n:] = 0x7F
            s[b, n:] = 0xFF


def _check_2x(q, kq, ks, vq, vs, lens_t, scale, max_len=None):
    """Print, then assert: kernel error <= 2 x twin error, both against float64 of the same inputs."""
    kd, vd = SF.kv_dequantize_mx(kq, ks), SF.kv_dequantize_mx(vq, vs)              # exact in fp32
    ref = SF.decode_attention_ref(q.double(), kd.double(), vd.double(), lens_t, scale)
    twin = SF.decode_attention_mx_ref(q, kq, ks, vq, vs, lens_t, scale)
    out = SF.decode_attention_mx(q, kq, ks, vq, vs, lens_t, scale, max_len=max_len)
    assert out.shape == q.shape and out.dtype == q.dtype
    assert torch.isfinite(out).all()
    e_k = (out.double() - ref).abs().max().item()
    e_t = (twin.double() - ref).abs().max().item()
    print(f"decode_attention_mx max err: kernel {e_k:.3e} twin {e_t:.3e} (ref max {ref.abs().max().item():.3e})")
    assert e_k <= 2 * e_t, (e_k, e_t)
    return out


@pytest.mark.parametrize("pattern", sorted(LENS))
@pytest.mark.parametrize("nh,nkv", HEADS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_decode_attention_mx_against_float64(dtype, D, nh, nkv, pattern):
    lens, cap = LENS[pattern]
    g = _gen(D + 7 * nh + 13 * nkv + len(pattern))
    q = torch.randn(3, nh, D, device="cuda", generator=g).to(dtype)
    kq, ks = _random_cache(3, cap, nkv, D, g)
    vq, vs = _random_cache(3, cap, nkv, D, g)
    _nan_tail(lens, (kq, ks), (vq, vs))
    lens_t = torch.tensor(lens, dtype=torch.int32, device="cuda")
    scale = 1.0 / math.sqrt(D)
    out = _check_2x(q, kq, ks, vq, vs, lens_t, scale)
    if pattern == "ones":            # a lone key: the output is its dequantised v row, rounded once
        want = SF.kv_dequantize_mx(vq[:, 0], vs[:, 0]).to(dtype)
        assert torch.equal(out.view(3, nkv, nh // nkv, D), want.unsqueeze(2).expand(3, nkv, nh // nkv, D))
    if max(lens) < cap:              # a grid bound below the capacity gives the same bits
        assert torch.equal(SF.decode_attention_mx(q, kq, ks, vq, vs, lens_t, scale, max_len=max(lens)), out)
    assert torch.equal(SF.decode_attention_mx(q, kq, ks, vq, vs, lens_t, scale), out)        # repeatable


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_large_scores_max_in_last_chunk(dtype):
    """The large-score case of tests/test_generation_gpu.py on a quantised cache: raw logits span
    about +-200, most of the large ones in the first chunk and the maximum in the last."""
    D, nh, nkv, cap = 64, 8, 2, 4 * C
    g = _gen(11)
    scale = 1.0 / math.sqrt(D)
    e = torch.randn(3, nkv, D, device="cuda", generator=g).sign()
    q = (e * 2.0).repeat_interleave(nh // nkv, dim=1)
    target = torch.empty(3, cap, nkv, device="cuda").uniform_(-200.0, 0.0, generator=g)
    target[:, :C] = torch.empty(3, C, nkv, device="cuda").uniform_(190.0, 199.0, generator=g)
    target[:, -3] = 200.0
    k = target.unsqueeze(-1) * e.unsqueeze(1) / (2.0 * D * scale)
    k = k + 0.01 * torch.randn(3, cap, nkv, D, device="cuda", generator=g)
    v = torch.randn(3, cap, nkv, D, device="cuda", generator=g)
    q = q.to(dtype)
    kq, ks = _quantise(k.bfloat16())
    vq, vs = _quantise(v.bfloat16())
    lens = [cap, cap, cap - 1]
    s = torch.einsum("bhd,bckd->bhck", q.double(), SF.kv_dequantize_mx(kq, ks)[:, :cap - 1].double()) * scale
    assert s.max() > 150 and s.min() < -150
    _nan_tail(lens, (kq, ks), (vq, vs))
    _check_2x(q, kq, ks, vq, vs, torch.tensor(lens, dtype=torch.int32, device="cuda"), scale)


@pytest.mark.parametrize("nh,nkv,D,rot", [(4, 2, 64, 64), (16, 4, 128, 128), (4, 4, 64, 32), (12, 12, 64, None)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_decode_rope_append_mx_bitwise(dtype, nh, nkv, D, rot):
    """q equals the 16-bit kernel's; the element and scale bytes of row pos[b] equal the twin's
    (mx_quantize_ref of the row the 16-bit kernel stores); no other row changes; an out-of-range
    position writes nothing."""
    B, cap = 5, 40
    g = _gen(7)
    e = torch.randint(-10, 7, (B, (nh + 2 * nkv) * D // 32, 1), device="cuda", generator=g).float()
    qkv = (torch.randn(B, (nh + 2 * nkv) * D // 32, 32, device="cuda", generator=g) * torch.exp2(e)).reshape(B, -1).to(dtype)
    pos = torch.tensor([0, cap - 1, 17, 5, cap], dtype=torch.int32, device="cuda")       # the last: out of range
    rope = None if rot is None else SF.rope_tables(cap, rot, device="cuda") + (rot,)
    k16 = torch.zeros(B, cap, nkv, D, device="cuda", dtype=dtype)
    v16 = torch.zeros_like(k16)
    q16 = SF.decode_rope_append(qkv, k16, v16, pos, nh, nkv, D, rope=rope)               # the existing kernel
    caches = []
    for _ in range(4):
        caches.append(torch.full((B, cap, nkv, D), 0x11, dtype=torch.uint8, device="cuda").view(torch.float8_e4m3fn))
        caches.append(torch.full((B, cap, nkv, D // 32), 0x22, dtype=torch.uint8, device="cuda"))
    kq, ks, vq, vs, tkq, tks, tvq, tvs = caches
    q = SF.decode_rope_append_mx(qkv, kq, ks, vq, vs, pos, nh, nkv, D, rope=rope)
    assert q.shape == (B, nh, D) and torch.equal(q[:4], q16[:4])
    SF.decode_rope_append_mx_ref(qkv[:4], tkq[:4], tks[:4], tvq[:4], tvs[:4], pos[:4], nh, nkv, D, rope=rope)
    for got, want in ((kq, tkq), (ks, tks), (vq, tvq), (vs, tvs)):
        assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))
    for b in range(4):               # and the twin's row is the quantised 16-bit row
        p = int(pos[b])
        wq, ws = SF.mx_quantize_ref(k16[b, p], "e4m3")
        assert torch.equal(kq[b, p].view(torch.uint8), wq.view(torch.uint8)) and torch.equal(ks[b, p], ws)
    assert (kq[4].view(torch.uint8) == 0x11).all() and (vs[4] == 0x22).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_prefill_store_bitwise(dtype):
    B, L, cap, nh, nkv, D = 2, 11, 13, 4, 2, 64
    g = _gen(4)
    qkv = (torch.randn(L, B, (nh + 2 * nkv) * D, device="cuda", generator=g) * 5).to(dtype)
    _, k, v = SF._qkv_views(qkv, nh, nkv, D, True)                                # strided views
    got = [torch.full((B, cap, nkv, D), 0x11, dtype=torch.uint8, device="cuda").view(torch.float8_e4m3fn),
           torch.full((B, cap, nkv, D // 32), 0x22, dtype=torch.uint8, device="cuda")]
    got += [t.clone() for t in got]
    want = [t.clone() for t in got]
    SF.kv_store_mx(k, v, got[0], got[1], got[2], got[3])
    SF.kv_store_mx_ref(k, v, want[0], want[1], want[2], want[3])
    for a, b in zip(got, want):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert (got[0][:, L:].view(torch.uint8) == 0x11).all() and (got[3][:, L:] == 0x22).all()
    assert not (got[0][:, :L].view(torch.uint8) == 0x11).all()


def test_refused_operands_raise():
    q = torch.zeros(2, 4, 64, device="cuda", dtype=torch.bfloat16)
    kq = torch.zeros(2, 16, 4, 64, device="cuda", dtype=torch.float8_e4m3fn)
    ks = torch.full((2, 16, 4, 2), 127, device="cuda", dtype=torch.uint8)
    lens = torch.ones(2, dtype=torch.int32, device="cuda")
    assert SF.decode_attention_mx_supported(q, kq, ks, kq, ks)
    SF.decode_attention_mx(q, kq, ks, kq.clone(), ks.clone(), lens, 0.125)
    with pytest.raises(RuntimeError, match="needs bf16 / fp16 q"):
        SF.decode_attention_mx(q.float(), kq, ks, kq, ks, lens, 0.125)
    with pytest.raises(RuntimeError, match=r"nh / nkv in \(1, 2, 4, 8\)"):
        SF.decode_attention_mx(torch.zeros(2, 12, 64, device="cuda", dtype=torch.bfloat16), kq, ks, kq, ks, lens, 0.125)
    k96 = torch.zeros(2, 16, 4, 96, device="cuda", dtype=torch.float8_e4m3fn)
    s96 = torch.zeros(2, 16, 4, 3, device="cuda", dtype=torch.uint8)
    with pytest.raises(RuntimeError, match=r"D in \(64, 128\)"):
        SF.decode_attention_mx(torch.zeros(2, 4, 96, device="cuda", dtype=torch.bfloat16), k96, s96, k96, s96, lens, 0.125)
    with pytest.raises(ValueError, match="max_len 17"):
        SF.decode_attention_mx(q, kq, ks, kq, ks, lens, 0.125, max_len=17)
    with pytest.raises(RuntimeError, match="needs bf16 / fp16 qkv"):
        SF.decode_rope_append_mx(torch.zeros(2, 12 * 64, device="cuda"), kq, ks, kq, ks, lens, 4, 4, 64)


# ------------------------------------------------------------------------------- end to end
FORMS = {
    "llama": dict(num_layers=2, hidden_size=256, num_attention_heads=4, num_query_groups=2,
                  activation="swiglu", normalization="RMSNorm", position_embedding_type="rope",
                  add_bias_linear=False, untie_embeddings_and_output_weights=True, layernorm_epsilon=1e-6),
    "opt": dict(num_layers=2, hidden_size=256, num_attention_heads=4, activation="relu",
                position_embedding_type="learned_absolute", position_offset=2),
}
_PAIRS = {}
STEPS = 12


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


def _teacher_forced(model, ids, plen, seq, fmt, weight_format=None):
    """Per-step logits [2, STEPS, 500] (fp32, CPU) of ``model`` fed ``seq``'s tokens through a cache."""
    from smdt_amd.models.generation import KVCache, _decode_weights
    from smdt_amd.parallel import tensor_parallel as tp
    dev = next(model.parameters()).device
    with torch.no_grad(), tp.decode_weights(_decode_weights(model, weight_format)):
        cache = KVCache(model.cfg, 2, 11 + STEPS, device=dev, format=fmt)
        out = [model.forward_prefill(ids.to(dev), plen.to(dev), cache)]
        cache.lens.copy_(plen)
        for t in range(STEPS - 1):
            tok = torch.stack([seq[b, plen[b] + t] for b in range(2)]).to(dev)
            cache.advance()
            out.append(model.forward_decode(tok, cache))
    return torch.stack(out, 1).float().cpu()[..., :500]


def _e2e_errors(form, monkeypatch, weight_format=None):
    from smdt_amd.models.generation import generate
    ref, gpu = _pair(form)
    ids, mask = _ragged_prompt()
    plen = mask.sum(1)
    seq = generate(ref, ids, mask, max_new_tokens=STEPS, eos_token_id=None)            # fp32, 16-bit-free path
    want = _teacher_forced(ref, ids, plen, seq, "mxfp8")                                # fp32 model, MXFP8 twins
    kern = _teacher_forced(gpu, ids, plen, seq, "mxfp8", weight_format)
    monkeypatch.setenv("SMDT_DISABLE_KERNELS", "1")
    with pytest.warns(UserWarning, match="SMDT_DISABLE_KERNELS"):
        twin = _teacher_forced(gpu, ids, plen, seq, "mxfp8", weight_format)
    monkeypatch.delenv("SMDT_DISABLE_KERNELS")
    e_k = (kern - want).abs().max().item()
    e_t = (twin - want).abs().max().item()
    return e_k, e_t, (ref, gpu, ids, plen, seq)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_cached_logits_as_close_to_the_fp32_twin_path_as_the_gpu_twins(form, monkeypatch):
    """Teacher-forced for 12 steps from a ragged two-row prompt. Reference: the fp32 CPU model
    through its own MXFP8 twin path. Yardstick: the bf16 GPU model with the same format on the torch
    twins. Both carry the same kind of FP8 rounding flips; the factor 2 covers summation order."""
    e_k, e_t, (ref, gpu, ids, plen, seq) = _e2e_errors(form, monkeypatch)
    print(f"{form}: max logit error vs the fp32 MXFP8 twin path: kernels {e_k:.4e}, GPU twins {e_t:.4e}")
    # what the format costs (printed, not asserted): the 16-bit-cache path against the plain fp32 model
    plain = _teacher_forced(ref, ids, plen, seq, None)
    e_16 = (_teacher_forced(gpu, ids, plen, seq, None) - plain).abs().max().item()
    e_mx = (_teacher_forced(gpu, ids, plen, seq, "mxfp8") - plain).abs().max().item()
    print(f"{form}: max logit error vs the plain fp32 model: 16-bit cache {e_16:.4e}, MXFP8 cache {e_mx:.4e}")
    assert e_k <= 2 * e_t, (e_k, e_t)


def test_with_weight_format_mxfp8(monkeypatch):
    e_k, e_t, _ = _e2e_errors("llama", monkeypatch, weight_format="mxfp8")
    print(f"llama, weight_format mxfp8: max logit error vs the fp32 MXFP8 twin path: kernels {e_k:.4e}, "
          f"GPU twins {e_t:.4e}")
    assert e_k <= 2 * e_t, (e_k, e_t)


@pytest.mark.parametrize("sample", [False, True], ids=["greedy", "sampled"])
def test_graph_replay_returns_the_eager_tokens(sample):
    from smdt_amd.models.generation import generate
    _, gpu = _pair("llama")
    ids, mask = _ragged_prompt()
    ids, mask = ids.cuda(), mask.cuda()
    kw = dict(max_new_tokens=20, eos_token_id=None, do_sample=sample, temperature=0.9, top_k=50, top_p=0.95,
              kv_cache_format="mxfp8")
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
        cache = KVCache(gpu.cfg, 2, 32, device="cuda", format="mxfp8")
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
