"""--fp8-fused-quantize, CPU side: the torch twins of the FP8-output producers against
``fp8_quantize_ref`` of the producer's output, the flag's refusals, and a 2-layer GPT step on the
twins with the flag on against the same step with it off."""
import pytest
import torch

from smdt_amd.ops import functional as SF

BASE = ["--num-layers", "2", "--hidden-size", "64", "--num-attention-heads", "4", "--seq-length", "32",
        "--max-position-embeddings", "32", "--micro-batch-size", "2", "--bf16"]


def _producers():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(17, 64, generator=g).bfloat16()
    res = torch.randn(17, 64, generator=g).bfloat16()
    gamma = (1 + 0.1 * torch.randn(64, generator=g)).bfloat16()
    beta, bias = (0.1 * torch.randn(2, 64, generator=g)).bfloat16()
    return {
        "layer_norm": lambda **k: SF.layer_norm(x, gamma, beta, **k),
        "rms_norm": lambda **k: SF.rms_norm(x, gamma, **k),
        "bda_norm": lambda **k: SF.bias_dropout_add_norm(x, bias, res, gamma, beta, 0.0, True, **k)[0],
        "gelu_tanh": lambda **k: SF.bias_gelu(x, bias, "tanh", **k),
        "gelu_erf": lambda **k: SF.bias_gelu(x, bias, "none", **k),
        "swiglu": lambda **k: SF.swiglu(x, **k),
    }


@pytest.mark.parametrize("keep16", [True, False])
@pytest.mark.parametrize("name", sorted(_producers()))
def test_twin_fp8_out_is_the_quantised_output(name, keep16):
    f = _producers()[name]
    y = f()
    scale, amax, amax_ref = torch.tensor([37.0]), torch.tensor([0.5]), torch.tensor([0.5])
    q_ref = SF.fp8_quantize_ref(y, scale, amax_ref, "e4m3")
    y16, q = f(fp8_out=(scale, amax), keep16=keep16)
    assert q.dtype == torch.float8_e4m3fn and torch.equal(q.view(torch.uint8), q_ref.view(torch.uint8))
    assert torch.equal(amax, amax_ref) and amax.item() > 0.5
    assert torch.equal(y16, y)              # the twins always have the 16-bit output


@pytest.mark.parametrize("extra,names", [
    ([], ["--fp8-hybrid", "--fp8-e4m3"]),
    (["--fp8-hybrid", "--fp8-recipe", "mxfp8"], ["--fp8-recipe mxfp8"]),
    (["--fp8-hybrid", "--num-experts", "4"], ["--num-experts"]),
    (["--fp8-hybrid", "--apply-residual-connection-post-layernorm"], ["--apply-residual-connection-post-layernorm"]),
])
def test_flag_refusals_name_the_conflict(extra, names, monkeypatch):
    from smdt_amd.train import arguments as A
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(ValueError) as e:
        A.validate_args(A.parse_args(argv=BASE + ["--fp8-fused-quantize"] + extra), {"tokenizer_type": "GPT2BPETokenizer"})
    assert "--fp8-fused-quantize" in str(e.value) and all(n in str(e.value) for n in names)


def test_flag_reaches_the_config_and_the_config_refuses_too(monkeypatch):
    from smdt_amd.models.transformer import TransformerConfig
    from smdt_amd.train import arguments as A
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setenv("RANK", "0")
    for flags in (["--fp8-fused-quantize"], []):
        a = A.validate_args(A.parse_args(argv=BASE + ["--fp8-hybrid"] + flags), {"tokenizer_type": "GPT2BPETokenizer"})
        a.padded_vocab_size = 64
        assert A.core_transformer_config_from_args(a).fp8_fused_quantize is bool(flags)
    for kw in ({}, {"fp8": "hybrid", "fp8_recipe": "mxfp8"}, {"fp8": "e4m3", "apply_residual_connection_post_layernorm": True}):
        with pytest.raises(ValueError):
            TransformerConfig(fp8_fused_quantize=True, **kw)


@pytest.mark.parametrize("fp8_wgrad", [False, True])
@pytest.mark.parametrize("activation", ["gelu", "swiglu"])
def test_gpt_step_on_the_twins_equals_the_unfused_step(activation, fp8_wgrad):
    """Loss, every main_grad and the FP8 table after the optimizer step, flag on against flag off."""
    from smdt_amd.models.gpt import GPTModel
    from smdt_amd.models.transformer import TransformerConfig
    from smdt_amd.optim.optimizer import MixedPrecisionAdam
    from smdt_amd.parallel import state as ps
    from smdt_amd.parallel.distributed import DistributedDataParallel
    kw = dict(num_layers=2, hidden_size=64, num_attention_heads=4, max_position_embeddings=32, padded_vocab_size=256,
              hidden_dropout=0.0, attention_dropout=0.0, seed=3, params_dtype=torch.bfloat16, fp8="hybrid",
              activation=activation, ffn_hidden_size=256, fp8_wgrad=fp8_wgrad, layernorm_zero_centered_gamma=True)
    t = torch.randint(0, 250, (2, 33), generator=torch.Generator().manual_seed(4))

    def run(fused):
        ps.destroy_model_parallel()
        model = GPTModel(TransformerConfig(**kw, fp8_fused_quantize=fused))
        ddp = DistributedDataParallel(model, grad_dtype=torch.float32)
        opt = MixedPrecisionAdam(ddp, lr=1e-3, weight_decay=0.0, clip_grad=1.0)
        ddp.zero_grad_buffer()
        loss = model(t[:, :-1], labels=t[:, 1:]).float().mean()
        loss.backward()
        ddp.finish_grad_sync()
        grads = ddp.grad_data.clone()
        opt.step()
        st = model.decoder.fp8_state
        return loss.item(), grads, st.scale.clone(), st.amax_history.clone()

    on, off = run(True), run(False)
    assert on[0] == off[0] and (off[2] != 1).all()
    for a, b in zip(on[1:], off[1:]):
        assert torch.equal(a, b)
