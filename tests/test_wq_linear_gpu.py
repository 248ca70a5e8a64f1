"""wq_gemm.hip on the MI355X (``SF.wq_linear``): against float64 under the project's criterion (max error
at most 2x that of the bf16 ``F.linear`` over the same dequantised weight), on exact data, at its bounds,
and ``generate(weight_gemm="fused")`` end to end. Shapes sit on the kernel's exported constants."""
import pytest
import torch
import torch.nn.functional as F

from smdt_amd.ops import functional as SF
from smdt_amd.parallel import tensor_parallel as tp

pytestmark = pytest.mark.gpu

QUANT = ["mxfp8", "mxfp4"]


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _shapes():
    """(Ms, Ns, Ks, a K that splits with a ragged last slice) on the tile constants."""
    c = SF.wq_linear_constants()
    top, bk = c["skinny_max_m"], c["bk"]
    assert top == max(c["bm"])
    return [17, 32, 33, top, top + 1, 2 * max(c["bm"]) + 5], [8, c["bn"] - 8, c["bn"] + 8], [32, bk, 3 * bk + 32], 5 * bk + 32


def _ws(M, N, K, fmt, pad=0):
    n = SF.wq_linear_workspace_numel(M, N, K, fmt)
    return torch.full((n + pad,), 555.0, device="cuda") if n + pad else None


def _weight(N, K, fmt, g):
    w = (torch.randn(N, K, device="cuda", generator=g) * 0.05).bfloat16()
    q, s = SF.decode_weight_quantize(w, fmt)
    return q, s, SF.decode_weight_dequantize(q, s, fmt)


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("fmt", QUANT)
def test_against_float64_and_repeatable(fmt, with_bias):
    Ms, Ns, Ks, ksplit = _shapes()
    for M in Ms:          # the ragged split at every M: slices of whole steps, the last one shorter
        p = SF.wq_linear_plan(M, Ns[0], ksplit, fmt)
        assert p["splits"] > 1 and p["slice"] % SF.wq_linear_constants()["bk"] == 0 and ksplit % p["slice"]
        assert p["regime"] == ("skinny" if M <= Ms[3] else "wide")
    for N in Ns:
        for K in Ks + [ksplit]:
            g = _gen(N + K)
            q, s, wd = _weight(N, K, fmt, g)
            b = torch.randn(N, device="cuda", generator=g).bfloat16() if with_bias else None
            xs = torch.randn(Ms[-1], K, device="cuda", generator=g).bfloat16()
            for M in Ms:
                x = xs[:M]
                ref = x.double() @ wd.double().t() + (b.double() if with_bias else 0)
                twin = F.linear(x, wd.bfloat16(), b)
                out = SF.wq_linear(x, q, s, b, fmt, _ws(M, N, K, fmt))
                assert out.shape == (M, N) and out.dtype == torch.bfloat16
                e_k = (out.double() - ref).abs().max().item()
                e_t = (twin.double() - ref).abs().max().item()
                print(f"{fmt} M {M} N {N} K {K} {SF.wq_linear_plan(M, N, K, fmt)}: kernel {e_k:.3e} twin {e_t:.3e}")
                assert e_k <= 2 * e_t, (fmt, M, N, K, e_k, e_t)
                assert torch.equal(SF.wq_linear(x, q, s, b, fmt, _ws(M, N, K, fmt)), out), (fmt, M, N, K)


@pytest.mark.parametrize("kind", ["skinny", "wide", "split"])
@pytest.mark.parametrize("fmt", QUANT)
def test_exact_data_is_bit_identical_to_float64(fmt, kind):
    """tests/test_decode_linear_gpu.py's construction: block scales 2^(e_b + d_n), e_b spanning -20 .. 20,
    x carrying 2^-e_b, small codes: every partial sum is exact in fp32 in any order, and a wrong nibble,
    scale byte, swizzle or k-order moves the result by orders of magnitude."""
    Ms, Ns, Ks, ksplit = _shapes()
    c = SF.wq_linear_constants()
    n_full = -(-c["split_below"] // 3) * c["bn"]             # with Ms[5]'s three M tiles: enough tiles, no split
    M, N, K = {"skinny": (Ms[2], Ns[2], Ks[2]), "wide": (Ms[5], n_full, Ks[2]), "split": (Ms[2] + 7, Ns[1], ksplit)}[kind]
    p = SF.wq_linear_plan(M, N, K, fmt)
    assert p["regime"] == ("wide" if kind == "wide" else "skinny") and (p["splits"] == 1) == (kind == "wide")
    g = _gen(K)
    nb = K // 32
    eb = torch.linspace(-20, 20, nb, device="cuda").round().int()[torch.randperm(nb, device="cuda", generator=g)]
    dn = torch.randint(0, 4, (N, 1), device="cuda", generator=g, dtype=torch.int32)
    s = (eb.unsqueeze(0) + dn + 127).to(torch.uint8)
    if fmt == "mxfp4":
        q = torch.randint(0, 256, (N, K // 2), device="cuda", generator=g, dtype=torch.int32).to(torch.uint8)
    else:
        q = torch.randint(-8, 9, (N, K), device="cuda", generator=g).float().to(torch.float8_e4m3fn)
    wd = SF.decode_weight_dequantize(q, s, fmt)
    assert torch.equal(wd.bfloat16().float(), wd)
    xi = torch.randint(-4, 5, (M, K), device="cuda", generator=g).float()
    x = (xi.view(M, nb, 32) * torch.ldexp(torch.ones((), device="cuda"), -eb).view(1, nb, 1)).view(M, K).bfloat16()
    bias = torch.randint(-64, 65, (N,), device="cuda", generator=g).bfloat16()
    ref = x.double() @ wd.double().t() + bias.double()
    assert ref.abs().max() < 2 ** 22 and torch.equal(ref.float().double(), ref)
    out = SF.wq_linear(x, q, s, bias, fmt, _ws(M, N, K, fmt))
    assert torch.equal(out, ref.float().bfloat16()), (fmt, M, N, K)


@pytest.mark.parametrize("kind", ["skinny", "wide-split"])
@pytest.mark.parametrize("fmt", QUANT)
def test_bounds(fmt, kind):
    """NaN rows behind x, 0xFF bytes behind Wq and the scales, canaries behind out and the workspace."""
    Ms, Ns, Ks, ksplit = _shapes()
    M, N, K = (Ms[2] + 4, Ns[2], Ks[1]) if kind == "skinny" else (Ms[5], Ns[2] + 64, ksplit)
    assert (SF.wq_linear_plan(M, N, K, fmt)["splits"] > 1) == (kind != "skinny")
    g = _gen(3)
    q, s, wd = _weight(N, K, fmt, g)

    def padded(t):
        buf = torch.full((t.numel() * t.element_size() + 4096,), 0xFF, dtype=torch.uint8, device="cuda")
        buf[:t.numel() * t.element_size()] = t.view(torch.uint8).reshape(-1)
        return buf[:t.numel() * t.element_size()].view(t.dtype).view(t.shape)
    xbuf = torch.full((M + 3, K), float("nan"), device="cuda", dtype=torch.bfloat16)
    xbuf[:M] = torch.randn(M, K, device="cuda", generator=g).bfloat16()
    obuf = torch.full((M + 3, N), 777.0, device="cuda", dtype=torch.bfloat16)
    n_ws = SF.wq_linear_workspace_numel(M, N, K, fmt)
    wsbuf = _ws(M, N, K, fmt, pad=1024)
    out = SF.wq_linear(xbuf[:M], padded(q), padded(s), None, fmt, wsbuf[:n_ws] if n_ws else None, out=obuf[:M])
    assert out.data_ptr() == obuf.data_ptr() and torch.isfinite(out).all()
    assert bool((obuf[M:] == 777.0).all()) and bool((wsbuf[n_ws:] == 555.0).all())
    want = F.linear(xbuf[:M], wd.bfloat16())
    assert (out.float() - want.float()).abs().max() <= 0.02 * want.float().abs().max()


def test_refusals_on_the_device():
    x = torch.zeros(20, 256, device="cuda", dtype=torch.bfloat16)
    q, s = SF.decode_weight_quantize(torch.zeros(64, 256, device="cuda", dtype=torch.bfloat16), "mxfp8")
    with pytest.raises(ValueError, match="fp16 cannot hold"):
        SF.wq_linear(x.half(), q, s, None, "mxfp8")
    with pytest.raises(RuntimeError, match="does not take M x N x K = 20 x 60 x 256"):
        SF.wq_linear(x, q[:60].contiguous(), s[:60].contiguous(), None, "mxfp8")
    with pytest.raises(RuntimeError, match="workspace"):                          # a split shape without one
        SF.wq_linear(x, q, s, None, "mxfp8")


# ------------------------------------------------------------------------------- end to end
FORMS = {
    "llama": dict(num_layers=2, hidden_size=256, num_attention_heads=4, num_query_groups=2,
                  activation="swiglu", normalization="RMSNorm", position_embedding_type="rope",
                  add_bias_linear=False, untie_embeddings_and_output_weights=True, layernorm_epsilon=1e-6),
    "opt": dict(num_layers=2, hidden_size=256, num_attention_heads=4, activation="relu",
                position_embedding_type="learned_absolute", position_offset=2),
}
_PAIRS = {}


def _pair(form, fmt=None):
    """(fp32 CPU model, bf16 GPU model), same weights; with ``fmt`` the layer linears hold dequant(quant(W))."""
    key = (form, fmt)
    if key not in _PAIRS:
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
            for m in gpu.decoder.modules() if fmt else ():
                if isinstance(m, (tp.ColumnParallelLinear, tp.RowParallelLinear)):
                    m.weight.copy_(SF.decode_weight_dequantize(*SF.decode_weight_quantize(m.weight, fmt), fmt))
            for pr, pg in zip(ref.parameters(), gpu.parameters()):
                pr.copy_(pg.float().cpu())
        ref.loss_vocab_size = gpu.loss_vocab_size = 500
        _PAIRS[key] = (ref, gpu)
    return _PAIRS[key]


@pytest.mark.parametrize("rows", [(17, 1), (4, 5)], ids=["decode-17-rows", "verify-4x5-rows"])
@pytest.mark.parametrize("fmt", QUANT)
@pytest.mark.parametrize("form", sorted(FORMS))
def test_fused_logits_as_close_to_fp32_as_full_forward(form, fmt, rows):
    """Teacher-forced: the prefill of a B x 9 prompt, then one decode step at batch 17 or one
    ``forward_extend`` of 4 x 5 tokens (the verify step, 20 rows), under ``weight_gemm="fused"``: at most
    2x as far from the fp32 dequantised-weight model as the bf16 full forward of that model."""
    from smdt_amd.models.generation import KVCache, _decode_weights, generate
    B, T = rows
    L = 9
    _, gpu = _pair(form)
    ref, oracle = _pair(form, fmt)
    ids = torch.randint(3, 500, (B, L), generator=torch.Generator().manual_seed(6))
    seq = generate(ref, ids, max_new_tokens=T + 1, eos_token_id=None)[:, :L + T]
    toks, plen = seq[:, L:].cuda(), torch.full((B,), L, device="cuda")
    with torch.no_grad():
        want = ref(seq)[:, L - 1:, :500]
        full = oracle(seq.cuda())[:, L - 1:, :500].float().cpu()
        state = _decode_weights(gpu, fmt, "fused", (B * L, B * T))
        with tp.decode_weights(state):
            cache = KVCache(gpu.cfg, B, L + T, torch.bfloat16, "cuda")
            first = gpu.forward_prefill(ids.cuda(), plen, cache)
            cache.lens.copy_(plen)
            cache.advance(T)
            rest = gpu.forward_decode(toks[:, 0], cache).unsqueeze(1) if T == 1 else gpu.forward_extend(toks, cache)
        assert state.scratch is None
    got = torch.cat([first.unsqueeze(1), rest], 1)[..., :500].float().cpu()
    e_c, e_f = (got - want).abs().max().item(), (full - want).abs().max().item()
    print(f"{form} {fmt} {B} x {T}: max logit error vs fp32: fused {e_c:.4e}, full forward {e_f:.4e}")
    assert e_c <= 2 * e_f, (e_c, e_f)


@pytest.mark.parametrize("fmt", QUANT)
def test_graph_replay_returns_the_eager_tokens_and_steps_do_not_synchronise(fmt):
    from smdt_amd.models.generation import KVCache, _decode_weights, generate
    _, gpu = _pair("llama")
    ids = torch.randint(3, 500, (17, 9), generator=torch.Generator().manual_seed(8)).cuda()
    kw = dict(max_new_tokens=12, eos_token_id=None, weight_format=fmt, weight_gemm="fused")
    eager = generate(gpu, ids, **kw)
    assert torch.equal(eager, generate(gpu, ids, use_graph=True, **kw)) and int(eager.max()) < 500
    plen = torch.full((17,), 9, device="cuda")
    with torch.no_grad(), tp.decode_weights(_decode_weights(gpu, fmt, "fused", (17 * 9, 17))):
        cache = KVCache(gpu.cfg, 17, 32, torch.bfloat16, "cuda")
        tok = gpu.forward_prefill(ids, plen, cache)[:, :500].argmax(-1)
        cache.lens.copy_(plen)
        cache.advance()
        gpu.forward_decode(tok, cache)                       # first use of every shape, outside the check
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for _ in range(4):
                cache.advance()
                tok = gpu.forward_decode(tok, cache)[:, :500].argmax(-1)
        finally:
            torch.cuda.set_sync_debug_mode("default")
