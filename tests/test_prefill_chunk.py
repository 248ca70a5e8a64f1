"""Chunked / prefix-cached prefill on the CPU: the torch twins, ``forward_chunk`` and
``generate(prefill_chunk=..., cached_prefix=...)`` of fp32 models (the GPU kernels are judged in
test_prefill_chunk_gpu.py)."""
import pytest
import torch

from smdt_amd.models import generation as G
from smdt_amd.ops import functional as SF
from test_generation import KINDS, _model


def _ragged():
    ids = torch.randint(3, 100, (2, 10), generator=torch.Generator().manual_seed(4))
    mask = torch.ones(2, 10, dtype=torch.long)
    mask[0, 7:] = 0
    return ids, mask


@pytest.mark.parametrize("kind", KINDS)
def test_chunked_prefill_equals_forward_prefill(kind):
    """Pieces of 3 from a cached prefix of [2, 0] tokens: the logits and the cache rows below the
    prompt lengths are ``forward_prefill``'s. Every row the pieces must write holds NaN before."""
    m = _model(kind).model
    ids, mask = _ragged()
    plen, starts = mask.sum(1), [2, 0]
    with torch.no_grad():
        c0, c1 = (G.KVCache(m.cfg, 2, 12, torch.float32) for _ in range(2))
        want = m.forward_prefill(ids, plen, c0)
        m.forward_prefill(ids, plen, c1)
        for t in c1.k + c1.v:
            for b, p in enumerate(starts):
                t[b, p:] = float("nan")
        got = G._prefill_pieces(m, ids, plen, c1, 3, starts)
    torch.testing.assert_close(got, want)
    for a, w in zip(c1.k + c1.v, c0.k + c0.v):
        for b in range(2):
            torch.testing.assert_close(a[b, :plen[b]], w[b, :plen[b]])


@pytest.mark.parametrize("kw", [dict(prefill_chunk=3), dict(cached_prefix=[2, 4]),
                                dict(prefill_chunk=4, cached_prefix=1)], ids=["chunk", "prefix", "both"])
def test_generate_tokens_equal_the_plain_call(kw):
    m = _model("llama")
    ids, mask = _ragged()
    plain = m.generate(ids, mask, max_new_tokens=8, eos_token_id=None)
    if "cached_prefix" in kw:
        kw = dict(kw, cache=G.KVCache(m.model.cfg, 2, 18, torch.float32))
        m.generate(ids, mask, max_new_tokens=8, eos_token_id=None, cache=kw["cache"])
    assert torch.equal(m.generate(ids, mask, max_new_tokens=8, eos_token_id=None, **kw), plain)


def test_pos_lens_minus_t_is_the_multi_token_twin():
    g = torch.Generator().manual_seed(2)
    T, lens = 5, torch.tensor([5, 23, 40], dtype=torch.int32)
    q = torch.randn(3, T, 4, 16, generator=g)
    k, v = torch.randn(3, 40, 2, 16, generator=g), torch.randn(3, 40, 2, 16, generator=g)
    want = SF.decode_attention_multi_ref(q, k, v, lens, 0.25)
    assert torch.equal(SF.prefill_attention_ref(q, k, v, lens - T, lens, 0.25), want)
    assert torch.equal(SF.prefill_attention(q, k, v, lens - T, lens, 0.25), want)
