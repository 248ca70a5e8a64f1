"""Weight formats for text generation, on the CPU: the MXFP4 quantiser's torch twin against a brute
force over the E2M1 grid, ``decode_linear_ref``, ``generate(weight_format=...)`` against a copy of
the model whose layer weights were replaced by dequant(quant(W)) (exact: both run the same
F.linear), the quantised-copy cache, and every refusal."""
import copy
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

from smdt_amd.ops import functional as SF
from smdt_amd.parallel import decode_weights as dw
from smdt_amd.parallel import tensor_parallel as tp

FP4 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
QUANT = ["mxfp8", "mxfp4"]


def _brute_code(v: float) -> int:
    """Nearest E2M1 value to v, ties to the even code, saturating; sign in bit 3."""
    a = min(abs(v), 6.0)
    best = min(range(8), key=lambda c: (abs(FP4[c] - a), c % 2))
    return best | (8 if math.copysign(1.0, v) < 0 else 0)                  # -0.0 keeps its sign


def _codes(q):
    return torch.stack((q & 0xF, q >> 4), dim=-1).reshape(q.shape[0], -1)


def _dq(w, fmt):
    return SF.decode_weight_dequantize(*SF.decode_weight_quantize(w, fmt), fmt)


# ------------------------------------------------------------------------------- MXFP4 twin
@pytest.mark.parametrize("e", [-20, -3, 0, 5, 20])
def test_mx4_all_codes_round_trip(e):
    """All 16 codes at block exponent e (a 6 in the block pins it): codes, scale and values exact."""
    vals = FP4 + [-x for x in FP4]
    row = torch.tensor(vals + vals, dtype=torch.float32) * 2.0 ** e            # 32 elements, amax 6 * 2^e
    q, s = SF.mx4_quantize_ref(row.view(1, 32))
    assert q.shape == (1, 16) and s.shape == (1, 1) and q.dtype == torch.uint8 and s.dtype == torch.uint8
    assert int(s[0, 0]) == e + 127                                              # floor(log2 6 * 2^e) - 2 = e
    want = list(range(16)) + list(range(16))                                     # -0.0 keeps its sign: code 8
    assert _codes(q)[0].tolist() == want
    assert torch.equal(SF.mx4_dequantize_ref(q, s), row.view(1, 32))


def test_mx4_nearest_ties_to_even_and_saturation():
    pts = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]                               # every midpoint of the grid
    grid = sorted(set(pts + [p - 0.01 for p in pts] + [p + 0.01 for p in pts] + FP4 + [0.1, 5.5, 5.99]))
    for sign, e in itertools.product((1.0, -1.0), (-7, 0, 9)):
        for chunk in range(0, len(grid), 31):
            vs = grid[chunk:chunk + 31]
            row = torch.zeros(32)
            row[0] = 6.0                                                         # pins the block exponent at e
            row[1:1 + len(vs)] = torch.tensor(vs) * sign
            q, s = SF.mx4_quantize_ref((row * 2.0 ** e).view(1, 32))
            assert int(s[0, 0]) == e + 127
            got = _codes(q)[0].tolist()
            assert got[1:1 + len(vs)] == [_brute_code(sign * v) for v in vs], (sign, e, vs)
    for mid, want in zip(pts, [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]):              # the ties, spelled out
        assert FP4[_brute_code(mid) & 7] == want
    # saturation: amax 7.9 has floor(log2) = 2, so e = 0 and 7.9 / 6.5 / 7 all clamp to 6
    row = torch.zeros(32)
    row[:4] = torch.tensor([7.9, -6.5, 7.0, 6.0])
    q, s = SF.mx4_quantize_ref(row.view(1, 32))
    assert int(s[0, 0]) == 127 and _codes(q)[0, :4].tolist() == [7, 15, 7, 7]


def test_mx4_scale_rule_zero_block_and_nibble_order():
    def scale_of(amax):
        row = torch.zeros(32)
        row[5] = amax
        return int(SF.mx4_quantize_ref(row.view(1, 32))[1][0, 0])
    below = torch.nextafter(torch.tensor(8.0), torch.tensor(0.0)).item()
    assert scale_of(8.0) == 127 + 3 - 2 and scale_of(below) == 127 + 2 - 2      # floor(log2 amax) - emax
    assert scale_of(2.0 ** -30) == 127 - 30 - 2
    z = torch.zeros(2, 64)
    q, s = SF.mx4_quantize_ref(z)
    _, s8 = SF.mx_quantize_ref(z.bfloat16(), "e4m3")
    assert torch.equal(s, s8) and int(q.max()) == 0                            # the zero block's scale of mx_quantize_ref
    row = torch.zeros(32)
    row[0], row[1], row[2] = 1.0, -6.0, 0.5                                      # codes 2, 15, 1; e = 0
    q, _ = SF.mx4_quantize_ref(row.view(1, 32))
    assert int(q[0, 0]) == (15 << 4) | 2 and int(q[0, 1]) == 1                  # element 0 in the low nibble


def test_mx4_round_trip_is_idempotent_and_non_finite_raises():
    g = torch.Generator().manual_seed(1)
    w = torch.randn(24, 96, generator=g) * torch.logspace(-6, 6, 24).unsqueeze(1)
    q, s = SF.mx4_quantize_ref(w)
    d = SF.mx4_dequantize_ref(q, s)
    q2, s2 = SF.mx4_quantize_ref(d)
    assert torch.equal(q, q2) and torch.equal(s, s2) and torch.equal(SF.mx4_dequantize_ref(q2, s2), d)
    assert torch.equal(d.bfloat16().float(), d)                                  # exact in bf16
    for bad in (float("nan"), float("inf"), float("-inf")):
        w2 = w.clone()
        w2[3, 40] = bad
        with pytest.raises(ValueError, match="layers.0.qkv.*NaN or Inf"):
            SF.mx4_quantize_ref(w2, "layers.0.qkv")
    with pytest.raises(ValueError, match="multiple of 32"):
        SF.mx4_quantize_ref(torch.zeros(4, 48))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("fmt", QUANT)
def test_dequantise_into_a_buffer_equals_the_twin(fmt, dtype):
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(24, 160, generator=g) * torch.logspace(-8, 8, 24).unsqueeze(1)).bfloat16()
    q, s = SF.decode_weight_quantize(w, fmt)
    if fmt == "mxfp4":
        q = q.clone()
        q[0, :8] = torch.arange(0, 256, 32, dtype=torch.uint8) | torch.arange(8, 16, dtype=torch.uint8)   # every code
    want = SF.decode_weight_dequantize(q, s, fmt)
    out = torch.full((24, 160), float("nan"), dtype=dtype)
    assert SF.decode_weight_dequantize_into(out, q, s, fmt) is out
    assert torch.equal(out.float(), want)


# ------------------------------------------------------------------------------- decode_linear_ref
@pytest.mark.parametrize("fmt", ["native"] + QUANT)
def test_decode_linear_ref_is_the_linear_over_the_dequantised_weight(fmt):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(5, 96, generator=g)
    w = torch.randn(40, 96, generator=g).bfloat16().float()
    bias = torch.randn(40, generator=g)
    if fmt == "native":
        assert torch.equal(SF.decode_linear_ref(x, w, None, bias, fmt), F.linear(x, w, bias))
        assert torch.equal(SF.decode_linear(x, w, None, bias, fmt), F.linear(x, w, bias))
        return
    q, s = SF.decode_weight_quantize(w, fmt)
    wd = SF.decode_weight_dequantize(q, s, fmt)
    assert wd.dtype == torch.float32 and not torch.equal(wd, w)
    assert torch.equal(SF.decode_linear_ref(x, q, s, bias, fmt), F.linear(x, wd, bias))
    assert torch.equal(SF.decode_linear(x, q, s, None, fmt), F.linear(x, wd))
    with pytest.raises(ValueError, match="scales"):
        SF.decode_linear(x, q, None, None, fmt)
    with pytest.raises(ValueError, match="one of"):
        SF.decode_linear(x, w, None, None, "int4")


# ------------------------------------------------------------------------------- generate on the CPU
FORMS = {
    "llama": dict(num_layers=2, hidden_size=256, num_attention_heads=4, num_query_groups=2,
                  activation="swiglu", normalization="RMSNorm", position_embedding_type="rope",
                  add_bias_linear=False, untie_embeddings_and_output_weights=True, layernorm_epsilon=1e-6),
    "opt": dict(num_layers=2, hidden_size=256, num_attention_heads=4, activation="relu",
                position_embedding_type="learned_absolute", position_offset=2),
}
_MODELS = {}


def _model(form, **over):
    """fp32 CPU model with bf16-representable weights, built once per form."""
    key = (form, tuple(sorted(over.items())))
    if key not in _MODELS:
        from smdt_amd.models.gpt import GPTModel
        from smdt_amd.models.transformer import TransformerConfig
        from smdt_amd.parallel import state as ps
        ps.destroy_model_parallel()
        kw = dict(FORMS[form], max_position_embeddings=128, padded_vocab_size=512, hidden_dropout=0.0,
                  attention_dropout=0.0, seed=3, params_dtype=torch.float32)
        kw.update(over)
        m = GPTModel(TransformerConfig(**kw)).eval()
        with torch.no_grad():
            for p in m.parameters():
                p.copy_(p.bfloat16().float())
        m.loss_vocab_size = 500
        _MODELS[key] = m
    return _MODELS[key]


def _layer_linears(model):
    return [(n, m) for n, m in model.decoder.named_modules()
            if isinstance(m, (tp.ColumnParallelLinear, tp.RowParallelLinear))]


def _oracle(model, fmt):
    """A deep copy whose layer-linear weights are dequant(quant(W)); the head is untouched."""
    o = copy.deepcopy(model)
    with torch.no_grad():
        for _, lin in _layer_linears(o):
            lin.weight.copy_(_dq(lin.weight, fmt))
    return o


def _ragged_prompt():
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(3, 500, (2, 11), generator=g)
    mask = torch.ones(2, 11, dtype=torch.long)
    mask[0, 5:] = 0
    return ids, mask


@pytest.mark.parametrize("fmt", ["native"] + QUANT)
@pytest.mark.parametrize("form", sorted(FORMS))
def test_generate_matches_the_dequantised_weight_model(form, fmt):
    from smdt_amd.models.generation import generate
    model = _model(form)
    ids, mask = _ragged_prompt()
    kw = dict(max_new_tokens=10, eos_token_id=None)
    plain = generate(model, ids, mask, **kw)
    got = generate(model, ids, mask, weight_format=fmt, **kw)
    if fmt == "native":
        assert torch.equal(got, plain)
        return
    oracle = _oracle(model, fmt)
    assert len(_layer_linears(model)) == 8                                       # qkv, proj, fc1, fc2 x 2 layers
    head = lambda m: m.output_weight if m.output_weight is not None else m.embedding.weight
    assert torch.equal(head(oracle), head(model))
    assert torch.equal(got, generate(oracle, ids, mask, **kw))
    # sampling and a reused cache go through the same routing
    from smdt_amd.models.generation import KVCache
    cache = KVCache(model.cfg, 2, 11 + 10)
    skw = dict(kw, do_sample=True, top_k=20, temperature=0.8)
    a = generate(model, ids, mask, weight_format=fmt, cache=cache, generator=torch.Generator().manual_seed(4), **skw)
    b = generate(oracle, ids, mask, generator=torch.Generator().manual_seed(4), **skw)
    assert torch.equal(a, b)


@pytest.mark.parametrize("fmt", QUANT)
def test_cache_follows_the_weights_and_stays_out_of_the_state_dict(fmt):
    from smdt_amd.models.generation import generate
    model = copy.deepcopy(_model("opt"))
    ids, mask = _ragged_prompt()
    kw = dict(max_new_tokens=8, eos_token_id=None)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    dw._DECODE_WQ.clear()
    generate(model, ids, mask, **kw)
    generate(model, ids, mask, weight_format="native", **kw)
    assert not dw._DECODE_WQ                                                     # None / native never make a copy
    first = generate(model, ids, mask, weight_format=fmt, **kw)
    assert len(dw._DECODE_WQ) == 8
    held = {k: v[1][0] for k, v in dw._DECODE_WQ.items()}
    generate(model, ids, mask, weight_format=fmt, **kw)
    assert all(dw._DECODE_WQ[k][1][0] is q for k, q in held.items())            # reused, not re-made
    after = model.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert not any("decode" in n or "quant" in n for n, _ in model.named_buffers())
    lin = model.decoder.layers[0].mlp.fc1
    with torch.no_grad():
        lin.weight.mul_(2)                                                       # an in-place edit: _version moves
    second = generate(model, ids, mask, weight_format=fmt, **kw)
    assert torch.equal(second, generate(_oracle(model, fmt), ids, mask, **kw))
    assert dw._DECODE_WQ[id(lin.weight)][1][0] is not held[id(lin.weight)]
    tp.params_changed()                                                          # an optimizer step: every copy goes
    assert not dw._DECODE_WQ
    generate(model, ids, mask, weight_format=fmt, **kw)
    assert all(dw._DECODE_WQ[k][1][0] is not q for k, q in held.items())
    other = [f for f in QUANT if f != fmt][0]                                    # one copy per weight, not one per format
    generate(model, ids, mask, weight_format=other, **kw)
    assert len(dw._DECODE_WQ) == 8 and all(v[0][-1] == other for v in dw._DECODE_WQ.values())
    tp.drop_cached_weight_t([lin.weight])
    assert id(lin.weight) not in dw._DECODE_WQ and len(dw._DECODE_WQ) == 7
    del lin, held
    del model                                                                    # a deleted model takes its copies along
    import gc
    gc.collect()
    assert not dw._DECODE_WQ
    assert first.shape == second.shape


def test_refusals():
    from smdt_amd.models.generation import generate
    ids, mask = _ragged_prompt()
    kw = dict(max_new_tokens=4, eos_token_id=None)
    model = _model("opt")
    with pytest.raises(ValueError, match="weight_format must be None or one of"):
        generate(model, ids, mask, weight_format="int8", **kw)
    # fp16 with a quantised format
    half = copy.deepcopy(model).half()
    for fmt in QUANT:
        with pytest.raises(ValueError, match="fp16.*bf16 models"):
            generate(half, ids, mask, weight_format=fmt, **kw)
    # a linear whose K the format cannot take (K = 48 is no multiple of the block)
    odd = _model("opt", hidden_size=48, num_attention_heads=2, ffn_hidden_size=64)
    for fmt in QUANT:
        with pytest.raises(ValueError, match="layers.0.attention.qkv.*cannot take the " + fmt):
            generate(odd, ids, mask, weight_format=fmt, **kw)
    # Switch MLP
    moe = _model("opt", num_experts=2)
    with pytest.raises(NotImplementedError, match="num_experts"):
        generate(moe, ids, mask, weight_format="mxfp8", **kw)
    # linears that carry _fp8
    fp8 = copy.deepcopy(model)
    object.__setattr__(fp8.decoder.layers[1].mlp.fc2, "_fp8", (object(), 0))
    with pytest.raises(RuntimeError, match="layers.1.mlp.fc2 carries _fp8"):
        generate(fp8, ids, mask, weight_format="native", **kw)
    with tp.decode_weights(tp.DecodeWeights("native")):
        with pytest.raises(RuntimeError, match="carries _fp8"):
            fp8.decoder.layers[1].mlp.fc2(torch.zeros(1, 2, 1024))
    # a non-finite weight under mxfp4 names the linear
    bad = copy.deepcopy(model)
    with torch.no_grad():
        bad.decoder.layers[0].attention.proj.weight[0, 0] = float("inf")
    with pytest.raises(ValueError, match="layers.0.attention.proj.*NaN or Inf"):
        generate(bad, ids, mask, weight_format="mxfp4", **kw)
    assert dw._DECODE["state"] is None                                           # every raise left the context
