"""Gating of the producer-made bias gradients (SMDT_BIAS_FROM_PRODUCER) without a GPU: CPU tensors
always keep the old routing, and a CPU backward still fills the QKV and fc1 bias gradients."""
import torch


def _cpu_layer():
    from smdt_amd.models.gpt import GPTModel
    from smdt_amd.models.transformer import TransformerConfig
    from smdt_amd.parallel import state as ps
    ps.destroy_model_parallel()
    cfg = TransformerConfig(num_layers=1, hidden_size=64, num_attention_heads=1, max_position_embeddings=128,
                            padded_vocab_size=256, hidden_dropout=0.0, attention_dropout=0.0, seed=3,
                            params_dtype=torch.bfloat16)
    return GPTModel(cfg)


def test_cpu_tensors_keep_the_wgrad_routing():
    from smdt_amd.parallel import tensor_parallel as tp
    model = _cpu_layer()
    named = dict(model.named_parameters())
    qkv_bias = next(p for n, p in named.items() if n.endswith("qkv.bias"))
    fc1_bias = next(p for n, p in named.items() if n.endswith("fc1.bias"))
    for p in (qkv_bias, fc1_bias):       # what DDP attaches: an fp32 main_grad and a readiness callback
        p.main_grad = torch.zeros(p.numel())
        p._smdt_grad_ready = lambda q: None
    x = torch.zeros(128, 1, 64, dtype=torch.bfloat16)
    assert tp._BIAS_FROM_PRODUCER                      # the switch is on by default
    assert not tp.bias_from_producer(qkv_bias, x)
    assert not tp.bias_from_producer(fc1_bias, x)
    assert not tp.bias_from_producer(None, x)
    attn = next(m for m in model.modules() if type(m).__name__ == "ParallelAttention")
    assert attn._qkv_bias_from_attention(x) is None
    toks = torch.randint(0, 200, (1, 129), generator=torch.Generator().manual_seed(1))
    model(toks[:, :-1], labels=toks[:, 1:]).float().mean().backward()
    for p in (qkv_bias, fc1_bias):       # the old path: autograd's .grad on the CPU
        assert p.grad is not None and torch.isfinite(p.grad.float()).all() and p.grad.float().abs().max() > 0
