"""The fused sampler's rule on the CPU (``SF.sample_tokens_ref``, the float64 twin of sample.hip)
and ``generate(sampler="fused")`` on a tiny fp32 model."""
import pytest
import torch

from smdt_amd.models import generation as G
from smdt_amd.models.hf import HFCausalLM
from smdt_amd.ops import functional as SF

CFG = dict(model_type="llama", hidden_size=64, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
           intermediate_size=96, vocab_size=100, max_position_embeddings=64, rms_norm_eps=1e-6, rope_theta=10000.0,
           hidden_act="silu", tie_word_embeddings=False, bos_token_id=1, eos_token_id=2)
NEW = 12
_STATE = {}


def _model():
    if "m" not in _STATE:
        torch.manual_seed(0)
        _STATE["m"] = HFCausalLM(CFG, params_dtype=torch.float32).eval()
        _STATE["ids"] = torch.randint(3, 100, (2, 6), generator=torch.Generator().manual_seed(1))
        _STATE["greedy"] = _STATE["m"].generate(_STATE["ids"], max_new_tokens=NEW, eos_token_id=None)
    return _STATE["m"], _STATE["ids"], _STATE["greedy"]


@pytest.mark.parametrize("k,p", [(0, 1.0), (5, 1.0), (0, 0.8), (5, 0.8)])
def test_kept_set_is_filter_logits_on_tie_free_rows(k, p):
    x = torch.randn(4, 97, generator=torch.Generator().manual_seed(2))
    assert all(row.unique().numel() == 97 for row in x)
    keep, _ = SF.sample_filter_ref(x, 0.7, k, p)
    assert torch.equal(keep, torch.isfinite(G.filter_logits(x, 0.7, k, p)))


def test_equispaced_draws_follow_the_filtered_distribution():
    x = torch.tensor([[0.3, -1.2, 2.0, 0.9, -0.4, 1.4, -2.5, 0.1]])
    N = 4096
    u = ((torch.arange(N) + 0.5) / N).float()
    tok = SF.sample_tokens_ref(x.expand(N, 8), u, temperature=0.8, top_k=6, top_p=0.9)
    want = torch.softmax(G.filter_logits(x, 0.8, 6, 0.9).double(), dim=-1)[0]
    freq = torch.bincount(tok, minlength=8).double() / N
    assert (freq - want).abs().max().item() <= 2 / N


def test_tie_class_at_the_top_p_cut_is_kept_whole():
    # probabilities .4, .2, .2, .2 (the last three tied): the mass above the class is .4 < .5, so all three stay
    x = torch.tensor([[0.4, 0.2, 0.2, 0.2, 1e-9]]).log()
    keep, _ = SF.sample_filter_ref(x, 1.0, 0, 0.5)
    assert keep.tolist() == [[True, True, True, True, False]]
    keep, _ = SF.sample_filter_ref(x, 1.0, 0, 0.35)            # .4 is not < .35: only the most likely token
    assert keep.tolist() == [[True, False, False, False, False]]


def test_generate_fused_greedy_and_top_k_1_are_the_default_greedy_tokens():
    m, ids, greedy = _model()
    assert torch.equal(m.generate(ids, max_new_tokens=NEW, eos_token_id=None, sampler="fused"), greedy)
    out = m.generate(ids, max_new_tokens=NEW, eos_token_id=None, sampler="fused", do_sample=True, top_k=1,
                     temperature=0.7, generator=torch.Generator().manual_seed(5))
    assert torch.equal(out, greedy)


def test_generate_fused_pads_after_eos():
    m, ids, greedy = _model()
    new = greedy[:, 6:]
    row, t = next((r, t) for t in range(1, NEW - 1) for r in range(2)
                  if new[r, t] not in new[r, :t] and new[r, t] not in new[1 - r])
    eos, pad = int(new[row, t]), 1
    want = greedy.clone()
    want[row, 6 + t + 1:] = pad
    out = m.generate(ids, max_new_tokens=NEW, eos_token_id=eos, pad_token_id=pad, sampler="fused")
    assert torch.equal(out, want)
    assert torch.equal(out, m.generate(ids, max_new_tokens=NEW, eos_token_id=eos, pad_token_id=pad))


def test_refusals_name_the_cause():
    m, ids, _ = _model()
    with pytest.raises(ValueError, match="sampler must be"):
        m.generate(ids, max_new_tokens=2, sampler="topk")
    with pytest.raises(NotImplementedError, match="draft model"):
        m.generate(ids, max_new_tokens=2, sampler="fused", draft_model=m)
    x = torch.zeros(2, 8)
    for kw in (dict(temperature=0.0), dict(top_p=0.0), dict(top_p=1.5)):
        assert not SF.sample_tokens_supported(x, **kw)
        with pytest.raises(ValueError, match="sample_tokens needs"):
            SF.sample_tokens(x, torch.zeros(2), **kw)
    assert not SF.sample_tokens_supported(torch.zeros(2, 8).t())
    assert SF.sample_tokens_supported(torch.zeros(2, 16)[:, :8])
