"""``generate(weight_gemm="fused")`` and ``SF.wq_linear`` on the CPU: the torch twin, the routing
(same tokens as the default mode: both run ``decode_linear_ref``'s values) and every refusal."""
import copy

import pytest
import torch
import torch.nn.functional as F

from smdt_amd.ops import functional as SF
from smdt_amd.parallel import decode_weights as dw

QUANT = ["mxfp8", "mxfp4"]
_MODELS = {}


def _model(**over):
    """fp32 CPU OPT-form model with bf16-representable weights, built once per variant."""
    key = tuple(sorted(over.items()))
    if key not in _MODELS:
        from smdt_amd.models.gpt import GPTModel
        from smdt_amd.models.transformer import TransformerConfig
        from smdt_amd.parallel import state as ps
        ps.destroy_model_parallel()
        kw = dict(num_layers=2, hidden_size=256, num_attention_heads=4, activation="relu",
                  position_embedding_type="learned_absolute", position_offset=2, max_position_embeddings=128,
                  padded_vocab_size=512, hidden_dropout=0.0, attention_dropout=0.0, seed=3, params_dtype=torch.float32)
        kw.update(over)
        m = GPTModel(TransformerConfig(**kw)).eval()
        with torch.no_grad():
            for p in m.parameters():
                p.copy_(p.bfloat16().float())
        m.loss_vocab_size = 500
        _MODELS[key] = m
    return _MODELS[key]


def _prompt(B=3, L=7):
    return torch.randint(3, 500, (B, L), generator=torch.Generator().manual_seed(9))


@pytest.mark.parametrize("fmt", QUANT)
def test_twin_and_supported(fmt):
    g = torch.Generator().manual_seed(2)
    x, w, bias = torch.randn(20, 96, generator=g), torch.randn(40, 96, generator=g), torch.randn(40, generator=g)
    q, s = SF.decode_weight_quantize(w, fmt)
    want = F.linear(x, SF.decode_weight_dequantize(q, s, fmt), bias)
    assert torch.equal(SF.wq_linear(x, q, s, bias, fmt), want)
    out = torch.empty(20, 40)
    assert SF.wq_linear(x, q, s, bias, fmt, out=out) is out and torch.equal(out, want)
    with pytest.raises(ValueError, match="one of"):
        SF.wq_linear(x, w, s, None, "native")
    with pytest.raises(ValueError, match="scales"):
        SF.wq_linear(x, q, None, None, fmt)
    assert SF.wq_linear_supported(20, 64, 256, torch.bfloat16, fmt)
    assert SF.wq_linear_supported(1, 8, 32, torch.bfloat16, fmt) and not SF.wq_linear_supported(0, 8, 32, torch.bfloat16, fmt)
    for M, N, K, dtype in [(20, 64, 256, torch.float16), (20, 64, 240, torch.bfloat16), (20, 60, 256, torch.bfloat16)]:
        assert not SF.wq_linear_supported(M, N, K, dtype, fmt)
    assert not SF.wq_linear_supported(20, 64, 256, torch.bfloat16, "native")


@pytest.mark.parametrize("extra", [{}, {"prefill_chunk": 3}, {"sampler": "fused"}, {"draft": True}], ids=str)
@pytest.mark.parametrize("fmt", QUANT)
def test_fused_mode_returns_the_default_modes_tokens(fmt, extra):
    from smdt_amd.models.generation import generate
    model = _model()
    kw = dict(max_new_tokens=6, eos_token_id=None, weight_format=fmt, **extra)
    if kw.pop("draft", False):
        kw.update(draft_model=model, num_draft_tokens=4)
    ids = _prompt()                                             # 21 prefill rows, 15 verify rows
    assert torch.equal(generate(model, ids, weight_gemm="fused", **kw), generate(model, ids, **kw))
    assert dw._DECODE["state"] is None


def test_refusals():
    from smdt_amd.models.generation import generate
    model, ids = _model(), _prompt()
    kw = dict(max_new_tokens=2, eos_token_id=None)
    for fmt in (None, "native"):
        with pytest.raises(ValueError, match="weight_gemm='fused'.*needs a quantised weight_format"):
            generate(model, ids, weight_format=fmt, weight_gemm="fused", **kw)
    with pytest.raises(ValueError, match="weight_gemm must be one of"):
        generate(model, ids, weight_format="mxfp8", weight_gemm="tiled", **kw)
    with pytest.raises(ValueError, match="weight_gemm must be one of"):
        dw.DecodeWeights("mxfp8", gemm="tiled")
    with pytest.raises(ValueError, match="fp16.*bf16 models"):
        generate(copy.deepcopy(model).half(), ids, weight_format="mxfp8", weight_gemm="fused", **kw)
    odd = _model(ffn_hidden_size=100)                                            # fc1 has N = 100, no multiple of 8
    with pytest.raises(ValueError, match=r"layers.0.mlp.fc1 \[100, 256\] is not taken"):
        generate(odd, ids, weight_format="mxfp8", weight_gemm="fused", **kw)
    assert dw._DECODE["state"] is None
