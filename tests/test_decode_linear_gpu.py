"""decode_linear.hip on the MI355X: the weight-streaming M <= 16 linear in its three weight formats
against float64, on exact data, at its bounds, and ``generate(weight_format=...)`` end to end.

The accuracy criterion is the project's (tests/test_generation_gpu.py): the kernel's max error
against a float64 product of the same (dequantised) operands is at most 2x the error of the 16-bit
``F.linear`` over the same dequantised weight; both round once, the factor covers summation order.
Shapes sit on the kernel's exported tiling constants."""
import copy

import pytest
import torch
import torch.nn.functional as F

from smdt_amd.ops import _ext
from smdt_amd.ops import functional as SF
from smdt_amd.parallel import tensor_parallel as tp

pytestmark = pytest.mark.gpu

QUANT = ["mxfp8", "mxfp4"]
FORMATS = ["native"] + QUANT
CASES = [("native", torch.bfloat16), ("native", torch.float16), ("mxfp8", torch.bfloat16), ("mxfp4", torch.bfloat16)]
CASE_IDS = ["native-bf16", "native-fp16", "mxfp8-bf16", "mxfp4-bf16"]
MS = [1, 2, 3, 8, 15, 16]


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _consts():
    return SF.decode_linear_constants()


def _weight(N, K, fmt, dtype, g, std=0.05):
    """(kernel operand, scales, dequantised fp32 weight)"""
    w = (torch.randn(N, K, device="cuda", generator=g) * std).to(dtype)
    if fmt == "native":
        return w, None, w.float()
    q, s = SF.decode_weight_quantize(w, fmt)
    return q, s, SF.decode_weight_dequantize(q, s, fmt)


def _ws(M, N, K, fmt):
    n = SF.decode_linear_workspace_numel(M, N, K, fmt)
    return torch.empty(n, dtype=torch.float32, device="cuda") if n else None


def test_constants_exported():
    c = _consts()
    assert c["rows"] == 16 and c["max_m"] == SF.decode_linear_max_m() == 16 and c["split_below"] >= 1
    for fmt in FORMATS:
        assert c["step_k"][fmt] % 32 == 0 and c["unroll"][fmt] >= 1
    # the K split: none once N fills the chip, slices in whole steps below that
    n_full = c["split_below"] * c["rows"]
    for fmt in FORMATS:
        assert SF.decode_linear_plan(n_full, 8 * c["step_k"][fmt], fmt)[0] == 1
        s, sl = SF.decode_linear_plan(n_full - c["rows"], 8 * c["step_k"][fmt], fmt)
        assert s > 1 and sl % c["step_k"][fmt] == 0 and (s - 1) * sl < 8 * c["step_k"][fmt] <= s * sl


def _shapes(fmt):
    c = _consts()
    it = c["step_k"][fmt] * c["unroll"][fmt]              # k of one unrolled iteration of a workgroup
    rows = c["rows"]
    ks = [it, it + 32, 768, 1600, 11008]
    ns = sorted({8, rows - 8, rows + 8})
    out = [(n, k) for k in ks for n in ns]
    out.append(((c["split_below"] - 1) * rows, 2 * c["step_k"][fmt] + 32))   # split K, a ragged last slice
    out.append((c["split_below"] * rows, 2 * c["step_k"][fmt] + 32))         # just not split
    return out


@pytest.mark.parametrize("fmt,dtype", CASES, ids=CASE_IDS)
def test_against_float64(fmt, dtype):
    for N, K in _shapes(fmt):
        g = _gen(N + K)
        w, s, wd = _weight(N, K, fmt, dtype, g)
        bias = torch.randn(N, device="cuda", generator=g).to(dtype)
        xs = torch.randn(16, K, device="cuda", generator=g).to(dtype)
        splits = SF.decode_linear_plan(N, K, fmt)[0]
        for M in MS:
            x = xs[:M]
            for b in (None, bias):
                ref = x.double() @ wd.double().t()
                if b is not None:
                    ref = ref + b.double()
                twin = F.linear(x, wd.to(dtype), b)
                out = SF.decode_linear(x, w, s, b, fmt, _ws(M, N, K, fmt))
                assert out.shape == (M, N) and out.dtype == dtype and torch.isfinite(out).all()
                e_k = (out.double() - ref).abs().max().item()
                e_t = (twin.double() - ref).abs().max().item()
                print(f"{fmt} {dtype} M {M} N {N} K {K} splits {splits} bias {b is not None}: "
                      f"kernel {e_k:.3e} twin {e_t:.3e} (ref max {ref.abs().max().item():.3e})")
                assert e_k <= 2 * e_t, (fmt, M, N, K, e_k, e_t)


@pytest.mark.parametrize("fmt", FORMATS)
def test_exact_data_is_bit_identical_to_float64(fmt):
    """Codes are small values, block b carries the scale 2^(e_b + d_n) with e_b spanning -20 .. 20
    along a row and d_n varying by row, and x carries 2^-e_b in block b: every product is a small
    multiple of one half and every partial sum is exact in fp32, so any summation order gives the
    float64 result; a wrong nibble, scale byte or k-permutation moves it by orders of magnitude."""
    c = _consts()
    it = c["step_k"][fmt] * c["unroll"][fmt]
    for N, K in [(24, it + 96), ((c["split_below"] - 1) * c["rows"], 2 * c["step_k"][fmt] + 32)]:
        g = _gen(K)
        nb = K // 32
        eb = torch.linspace(-20, 20, nb, device="cuda").round().int()[torch.randperm(nb, device="cuda", generator=g)]
        dn = torch.randint(0, 4, (N, 1), device="cuda", generator=g, dtype=torch.int32)
        s = (eb.unsqueeze(0) + dn + 127).to(torch.uint8)                                   # [N, K / 32]
        if fmt == "mxfp4":
            q = torch.randint(0, 256, (N, K // 2), device="cuda", generator=g, dtype=torch.int32).to(torch.uint8)
            wd = SF.mx4_dequantize_ref(q, s)
            w = q
        else:
            vals = torch.randint(-8, 9, (N, K), device="cuda", generator=g).float()
            q = vals.to(torch.float8_e4m3fn)
            wd = SF.decode_weight_dequantize(q, s, "mxfp8")
            w = q if fmt == "mxfp8" else wd.bfloat16()
        assert torch.equal(wd.bfloat16().float(), wd)
        xi = torch.randint(-4, 5, (16, K), device="cuda", generator=g).float()
        x = (xi.view(16, nb, 32) * torch.ldexp(torch.ones((), device="cuda"), -eb).view(1, nb, 1)).view(16, K).bfloat16()
        bias = torch.randint(-64, 65, (N,), device="cuda", generator=g).bfloat16()
        ref = (x.double() @ wd.double().t() + bias.double())
        assert ref.abs().max() < 2 ** 22 and torch.equal(ref.float().double(), ref)
        for M in (1, 5, 16):
            out = SF.decode_linear(x[:M], w, None if fmt == "native" else s, bias, fmt, _ws(M, N, K, fmt))
            assert torch.equal(out, ref[:M].float().bfloat16()), (fmt, M, N, K)


@pytest.mark.parametrize("fmt", FORMATS)
def test_bounds(fmt):
    """NaN rows behind x, NaN / 0xFF bytes behind W and the scales in the same allocation, canaries
    behind out and the workspace: the result is finite and nothing beyond M rows is written."""
    c = _consts()
    for N, K in [(c["rows"] + 8, 1600), ((c["split_below"] - 1) * c["rows"], 2 * c["step_k"][fmt] + 32)]:
        g = _gen(3)
        w, s, wd = _weight(N, K, fmt, torch.bfloat16, g)
        wbuf = torch.full((w.numel() * w.element_size() + 4096,), 0xFF, dtype=torch.uint8, device="cuda")
        wbuf[:w.numel() * w.element_size()] = w.view(torch.uint8).reshape(-1)
        wv = wbuf[:w.numel() * w.element_size()].view(w.dtype).view(w.shape)
        sv = None
        if s is not None:
            sbuf = torch.full((s.numel() + 4096,), 0xFF, dtype=torch.uint8, device="cuda")
            sbuf[:s.numel()] = s.reshape(-1)
            sv = sbuf[:s.numel()].view(s.shape)
        for M in (1, 7, 16):
            xbuf = torch.full((M + 3, K), float("nan"), device="cuda", dtype=torch.bfloat16)
            xbuf[:M] = torch.randn(M, K, device="cuda", generator=g).bfloat16()
            obuf = torch.full((M + 3, N), 777.0, device="cuda", dtype=torch.bfloat16)
            n_ws = SF.decode_linear_workspace_numel(M, N, K, fmt)
            wsbuf = torch.full((n_ws + 1024,), 555.0, device="cuda")
            out = SF.decode_linear(xbuf[:M], wv, sv, None, fmt, wsbuf[:n_ws] if n_ws else None, out=obuf[:M])
            assert out.data_ptr() == obuf.data_ptr() and torch.isfinite(out).all()
            assert bool((obuf[M:] == 777.0).all()) and bool((wsbuf[n_ws:] == 555.0).all())
            want = F.linear(xbuf[:M], wd.bfloat16())
            assert (out.float() - want.float()).abs().max() <= 0.02 * want.float().abs().max()


@pytest.mark.parametrize("fmt", FORMATS)
def test_bitwise_repeatable(fmt):
    c = _consts()
    for N, K in [(c["rows"] + 8, 11008), ((c["split_below"] - 1) * c["rows"], 4 * c["step_k"][fmt])]:
        g = _gen(17)
        w, s, _ = _weight(N, K, fmt, torch.bfloat16, g)
        x = torch.randn(16, K, device="cuda", generator=g).bfloat16()
        ws = _ws(16, N, K, fmt)
        first = SF.decode_linear(x, w, s, None, fmt, ws)
        for _ in range(9):
            assert torch.equal(SF.decode_linear(x, w, s, None, fmt, ws), first)


def test_refusals_on_the_device():
    c = _consts()
    x = torch.zeros(4, 256, device="cuda", dtype=torch.float16)
    w = torch.zeros(64, 256, device="cuda", dtype=torch.float16)
    q, s = SF.decode_weight_quantize(w.bfloat16(), "mxfp8")
    with pytest.raises(ValueError, match="fp16 cannot hold"):
        SF.decode_linear(x, q, s, None, "mxfp8")
    q4, s4 = SF.decode_weight_quantize(w.bfloat16(), "mxfp4")
    with pytest.raises(ValueError, match="fp16 cannot hold"):
        SF.decode_linear(x, q4, s4, None, "mxfp4")
    assert SF.decode_linear_supported(4, 64, 256, torch.float16, "native")
    assert not SF.decode_linear_supported(4, 64, 256, torch.float16, "mxfp8")
    bound = c["max_m"]
    for fmt in FORMATS:
        assert SF.decode_linear_supported(bound, 64, 256, torch.bfloat16, fmt)
        assert not SF.decode_linear_supported(bound + 1, 64, 256, torch.bfloat16, fmt)
        assert not SF.decode_linear_supported(4, 60, 256, torch.bfloat16, fmt)
        assert not SF.decode_linear_supported(4, 64, 240, torch.bfloat16, fmt)
    assert not SF.decode_linear_supported(4, 64, 256, torch.float32, "native")
    with pytest.raises(RuntimeError, match="does not take M x N x K = 17"):
        SF.decode_linear(torch.zeros(bound + 1, 256, device="cuda", dtype=torch.bfloat16), w.bfloat16())
    n = (c["split_below"] - 1) * c["rows"]
    with pytest.raises(RuntimeError, match="workspace"):                          # a split shape without one
        SF.decode_linear(torch.zeros(2, 1024, device="cuda", dtype=torch.bfloat16),
                         torch.zeros(n, 1024, device="cuda", dtype=torch.bfloat16))


# ------------------------------------------------------------------------------- end to end
FORMS = {
    "llama": dict(num_layers=2, hidden_size=256, num_attention_heads=4, num_query_groups=2,
                  activation="swiglu", normalization="RMSNorm", position_embedding_type="rope",
                  add_bias_linear=False, untie_embeddings_and_output_weights=True, layernorm_epsilon=1e-6),
    "opt": dict(num_layers=2, hidden_size=256, num_attention_heads=4, activation="relu",
                position_embedding_type="learned_absolute", position_offset=2),
}
_PAIRS = {}


def _build(kw, fmt):
    """(fp32 CPU model, bf16 GPU model) holding the same weights; with ``fmt`` the layer linears of
    both hold dequant(quant(W))."""
    from smdt_amd.models.gpt import GPTModel
    from smdt_amd.models.transformer import TransformerConfig
    from smdt_amd.parallel import state as ps
    ps.destroy_model_parallel()
    ref = GPTModel(TransformerConfig(**kw, params_dtype=torch.float32)).eval()
    gpu = GPTModel(TransformerConfig(**kw, params_dtype=torch.bfloat16), device="cuda").eval()
    with torch.no_grad():
        for pr, pg in zip(ref.parameters(), gpu.parameters()):
            pg.copy_(pr.to(torch.bfloat16))
        if fmt is not None:
            for m in gpu.decoder.modules():
                if isinstance(m, (tp.ColumnParallelLinear, tp.RowParallelLinear)):
                    q, s = SF.decode_weight_quantize(m.weight, fmt)
                    m.weight.copy_(SF.decode_weight_dequantize(q, s, fmt))
        for pr, pg in zip(ref.parameters(), gpu.parameters()):
            pr.copy_(pg.float().cpu())
    ref.loss_vocab_size = gpu.loss_vocab_size = 500
    return ref, gpu


def _pair(form, fmt=None):
    """fmt None: the 16-bit weights; else the oracle pair whose layer weights are dequant(quant(W))
    of the same initial weights (the LM head untouched)."""
    if (form, fmt) not in _PAIRS:
        kw = dict(FORMS[form], max_position_embeddings=128, padded_vocab_size=512, hidden_dropout=0.0,
                  attention_dropout=0.0, seed=3)
        _PAIRS[(form, fmt)] = _build(kw, None if fmt in (None, "native") else fmt)
    return _PAIRS[(form, fmt)]


def _ragged_prompt():
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(3, 500, (2, 11), generator=g)
    mask = torch.ones(2, 11, dtype=torch.long)
    mask[0, 5:] = 0
    return ids, mask


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("form", sorted(FORMS))
def test_cached_logits_as_close_to_fp32_as_full_forward(form, fmt):
    """Teacher-forced for 12 steps from the ragged two-row prompt: prefill + decode logits of the
    16-bit-weight model under ``fmt`` against the fp32 forward of the dequantised-weight model, at
    most 2x as far as the 16-bit full forward of that same model."""
    from smdt_amd.models.generation import KVCache, _decode_weights, generate
    _, gpu = _pair(form)                       # the model generation runs on: 16-bit weights
    ref, oracle = _pair(form, fmt)             # fp32 / bf16 models over dequant(quant(W))
    ids, mask = _ragged_prompt()
    steps = 12
    seq = generate(ref, ids, mask, max_new_tokens=steps, eos_token_id=None)
    plen = mask.sum(1)
    with torch.no_grad():
        cache = KVCache(gpu.cfg, 2, 11 + steps, torch.bfloat16, "cuda")
        with tp.decode_weights(_decode_weights(gpu, fmt)):
            cached = [gpu.forward_prefill(ids.cuda(), plen.cuda(), cache)]
            cache.lens.copy_(plen)
            for t in range(steps - 1):
                tok = torch.stack([seq[b, plen[b] + t] for b in range(2)]).cuda()
                cache.advance()
                cached.append(gpu.forward_decode(tok, cache))
        cached = torch.stack(cached, 1).float().cpu()[..., :500]
        e_c = e_f = 0.0
        for b in range(2):
            n = int(plen[b])
            row = seq[b:b + 1, :n + steps - 1]
            want = ref(row)[0, n - 1:, :500]
            full = oracle(row.cuda())[0, n - 1:, :500].float().cpu()
            e_c = max(e_c, (cached[b] - want).abs().max().item())
            e_f = max(e_f, (full - want).abs().max().item())
    print(f"{form} {fmt}: max logit error vs fp32: cached {e_c:.4e}, full forward {e_f:.4e}")
    assert e_c <= 2 * e_f, (e_c, e_f)


def test_prefill_uses_the_quantised_values_where_the_fused_mlp_would_apply():
    """One GeLU-with-bias layer, 8 x 512 tokens x ffn 4096 = 256 tiles: the shape at which the fused
    MLP forms (which read fc1.weight / fc2.weight themselves) apply on 256 CUs. Under mxfp4 the
    prefill logits must follow the dequantised weights, not the 16-bit ones."""
    from smdt_amd.models.generation import KVCache, _decode_weights
    kw = dict(num_layers=1, hidden_size=1024, ffn_hidden_size=4096, num_attention_heads=16,
              max_position_embeddings=512, padded_vocab_size=512, hidden_dropout=0.0, attention_dropout=0.0, seed=5)
    _, gpu = _build(kw, None)
    ref, oracle = _build(kw, "mxfp4")
    assert gpu.cfg.activation == "gelu" and gpu.cfg.bias_gelu_fusion and gpu.cfg.add_bias_linear
    with torch.no_grad():
        for m in (gpu, ref, oracle):
            for p in m.decoder.layers[0].mlp.fc1.bias, m.decoder.layers[0].mlp.fc2.bias:
                p.copy_(torch.linspace(-0.5, 0.5, p.numel()).bfloat16().to(p.dtype))
    ids = torch.randint(3, 500, (8, 512), generator=torch.Generator().manual_seed(2))
    plen = torch.full((8,), 512)
    with torch.no_grad():
        want = ref.forward_prefill(ids, plen, KVCache(ref.cfg, 8, 512))[:, :500]
        plain_ref = copy.deepcopy(ref)
        for pr, pg in zip(plain_ref.parameters(), gpu.parameters()):
            pr.copy_(pg.float().cpu())
        twin_gap = (plain_ref.forward_prefill(ids, plen, KVCache(ref.cfg, 8, 512))[:, :500] - want).abs().max().item()
        c = lambda: KVCache(gpu.cfg, 8, 512, torch.bfloat16, "cuda")
        full = oracle.forward_prefill(ids.cuda(), plen.cuda(), c())[:, :500].float().cpu()
        plain = gpu.forward_prefill(ids.cuda(), plen.cuda(), c())[:, :500].float().cpu()
        with tp.decode_weights(_decode_weights(gpu, "mxfp4")):
            got = gpu.forward_prefill(ids.cuda(), plen.cuda(), c())[:, :500].float().cpu()
    e_q, e_f, e_p = ((t - want).abs().max().item() for t in (got, full, plain))
    print(f"prefill under mxfp4: {e_q:.4e}; 16-bit forward of the dequantised model: {e_f:.4e}; "
          f"16-bit weights: {e_p:.4e} (fp32 twin gap {twin_gap:.4e})")
    assert twin_gap > 2 * e_f, "the weights do not separate the two models"
    assert e_q <= 2 * e_f, (e_q, e_f)
    assert e_p > 2 * e_f, (e_p, e_f)


@pytest.mark.parametrize("sample", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_graph_replay_returns_the_eager_tokens(fmt, sample):
    from smdt_amd.models.generation import generate
    _, gpu = _pair("llama")
    ids, mask = _ragged_prompt()
    ids, mask = ids.cuda(), mask.cuda()
    kw = dict(max_new_tokens=20, eos_token_id=None, do_sample=sample, temperature=0.9, top_k=50, top_p=0.95,
              weight_format=fmt)
    eager = generate(gpu, ids, mask, generator=_gen(21), **kw)
    graph = generate(gpu, ids, mask, generator=_gen(21), use_graph=True, **kw)
    assert torch.equal(eager, graph)
    assert int(eager.max()) < 500


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", [(1, 4), (3, 5), (1, 16), (16, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_short_prompts_whose_prefill_takes_the_kernel(fmt, shape):
    """B * Lmax <= 16: the prefill's linears have M = B * Lmax > B rows and run the kernel too, on
    linears that split K (fc2 in every format, all four in 16-bit). Eager and graph replay agree, and
    the prefill logits meet the 2x criterion against the fp32 dequantised-weight model."""
    from smdt_amd.models.generation import KVCache, _decode_weights, generate
    B, L = shape
    _, gpu = _pair("opt")
    ref, oracle = _pair("opt", fmt)
    c = _consts()
    fc2 = gpu.decoder.layers[0].mlp.fc2.weight                                   # 256 x 1024: split in every format
    assert SF.decode_linear_plan(fc2.shape[0], fc2.shape[1], fmt)[0] > 1
    assert B * L <= c["max_m"]
    ids = torch.randint(3, 500, (B, L), generator=torch.Generator().manual_seed(B + L))
    kw = dict(max_new_tokens=6, eos_token_id=None, weight_format=fmt)
    eager = generate(gpu, ids.cuda(), **kw)
    graph = generate(gpu, ids.cuda(), use_graph=True, **kw)
    assert torch.equal(eager, graph) and eager.shape == (B, L + 6)
    plen = torch.full((B,), L)
    with torch.no_grad():
        want = ref.forward_prefill(ids, plen, KVCache(ref.cfg, B, L))[:, :500]
        full = oracle.forward_prefill(ids.cuda(), plen.cuda(), KVCache(gpu.cfg, B, L, torch.bfloat16, "cuda"))
        with tp.decode_weights(_decode_weights(gpu, fmt)):
            got = gpu.forward_prefill(ids.cuda(), plen.cuda(), KVCache(gpu.cfg, B, L, torch.bfloat16, "cuda"))
    e_k = (got[:, :500].float().cpu() - want).abs().max().item()
    e_f = (full[:, :500].float().cpu() - want).abs().max().item()
    print(f"{fmt} prompt {B} x {L}: prefill logit error vs fp32: kernel path {e_k:.4e}, full forward {e_f:.4e}")
    assert e_k <= 2 * e_f, (e_k, e_f)


@pytest.mark.parametrize("fmt", FORMATS)
def test_decode_steps_do_not_synchronise(fmt):
    from smdt_amd.models.generation import KVCache, _decode_weights
    _, gpu = _pair("opt")
    ids, mask = _ragged_prompt()
    ids, plen = ids.cuda(), mask.sum(1).cuda()
    with torch.no_grad(), tp.decode_weights(_decode_weights(gpu, fmt)):
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


@pytest.mark.parametrize("fmt", QUANT)
def test_batch_above_the_bound_goes_through_the_scratch_path(fmt):
    """M = 17 is reported unsupported; a decode step at that batch dequantises into the scratch and
    runs the ordinary linear, which is what the dequantised-weight model computes: same logits."""
    from smdt_amd.models.generation import KVCache, _decode_weights
    B = _consts()["max_m"] + 1
    _, gpu = _pair("llama")
    _, oracle = _pair("llama", fmt)
    ids = torch.randint(3, 500, (B, 9), generator=torch.Generator().manual_seed(6)).cuda()
    plen = torch.full((B,), 9, device="cuda")

    def run(model, state):
        with torch.no_grad(), tp.decode_weights(state):
            cache = KVCache(model.cfg, B, 16, torch.bfloat16, "cuda")
            tok = model.forward_prefill(ids, plen, cache)[:, :500].argmax(-1)
            cache.lens.copy_(plen)
            cache.advance()
            return model.forward_decode(tok, cache)
    state = _decode_weights(gpu, fmt)
    assert state.scratch is not None
    assert torch.equal(run(gpu, state), run(oracle, None))
