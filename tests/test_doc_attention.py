"""Per-document attention (``--reset-attention-mask``) on the CPU reference path: the ``doc_start``
descriptor against the dense left-to-right mask, ``attention_ref`` against attention run per
document, a packed GPT sample against its documents run alone, and the argument validation."""
import math

import pytest
import torch

from smdt_amd.ops import functional as SF
from smdt_amd.train.utils import document_ends, document_starts, get_ltor_masks_and_position_ids

EOD = 7


def _token_cases():
    g = torch.Generator().manual_seed(0)
    rnd = torch.randint(0, 12, (3, 48), generator=g)           # EOD = 7 about every 12th token
    assert (rnd == EOD).any(dim=1).all()
    base = torch.randint(8, 20, (5, 16), generator=g)          # no EOD ...
    base[0, 5] = base[0, 6] = EOD                              # two consecutive EODs
    base[1, 0] = EOD                                           # EOD at position 0
    base[2, 15] = EOD                                          # EOD at the last position
    base[3, 0] = base[3, 1] = base[3, 14] = base[3, 15] = EOD  # both ends, doubled
    return {"random": rnd, "edges": base, "no_eod": base[4:5]}


@pytest.mark.parametrize("case", ["random", "edges", "no_eod"])
def test_document_starts_matches_the_dense_reset_mask(case):
    """``k`` is visible to ``q`` iff ``doc_start[q] <= k <= q`` (and iff ``k <= q < doc_end[k]``):
    exactly the block structure of ``get_ltor_masks_and_position_ids(reset_attention_mask=True)``."""
    toks = _token_cases()[case]
    b, s = toks.shape
    dense, _, _ = get_ltor_masks_and_position_ids(toks, EOD, False, True, False)     # True = masked
    ds = document_starts(toks, EOD)
    de = document_ends(ds)
    assert ds.dtype == torch.int32 and ds.shape == (b, s) and de.dtype == torch.int32 and de.shape == (b, s)
    ar = torch.arange(s)
    q, k = ar[None, :, None], ar[None, None, :]
    vis_q = (k >= ds[:, :, None]) & (k <= q)
    vis_k = (k <= q) & (q < de[:, None, :])
    assert torch.equal(vis_q, ~dense[:, 0])
    assert torch.equal(vis_k, ~dense[:, 0])
    assert torch.equal(SF.document_mask(ds), dense)
    # the invariants the kernels rely on: both non-decreasing, start <= i < end
    assert (ds[:, 1:] >= ds[:, :-1]).all() and (de[:, 1:] >= de[:, :-1]).all()
    assert (ds <= ar).all() and (de > ar).all() and (de <= s).all()
    if case == "no_eod":
        assert (ds == 0).all() and (de == s).all()


def test_document_starts_values_at_the_edges():
    toks = _token_cases()["edges"]
    ds = document_starts(toks, EOD)
    assert ds[0].tolist() == [0] * 6 + [6] + [7] * 9          # the second EOD is a one-token document
    assert ds[1].tolist() == [0] + [1] * 15                    # EOD at 0 ends a one-token document
    assert ds[2].tolist() == [0] * 16                          # EOD at the end belongs to its document
    assert document_ends(ds)[0].tolist() == [6] * 6 + [7] + [16] * 9


@pytest.mark.parametrize("heads", [(4, 4), (4, 2)])
def test_attention_ref_doc_start_is_attention_per_document(heads):
    torch.manual_seed(1)
    B, S, D = 2, 40, 16
    H, Hkv = heads
    q = torch.randn(B, S, H, D)
    k, v = torch.randn(B, S, Hkv, D), torch.randn(B, S, Hkv, D)
    bounds = [[0, 7, 8, 23, 39, 40], [0, 40]]                  # row 0: a one-token document, the last token alone
    ds = torch.zeros(B, S, dtype=torch.int32)
    for bi, bd in enumerate(bounds):
        for a, e in zip(bd[:-1], bd[1:]):
            ds[bi, a:e] = a
    scale = 1 / math.sqrt(D)
    o = SF.attention_ref(q, k, v, scale, True, doc_start=ds)
    assert torch.isfinite(o).all()
    for bi, bd in enumerate(bounds):
        for a, e in zip(bd[:-1], bd[1:]):
            part = SF.attention_ref(q[bi:bi + 1, a:e], k[bi:bi + 1, a:e], v[bi:bi + 1, a:e], scale, True)
            torch.testing.assert_close(o[bi:bi + 1, a:e], part, atol=1e-5, rtol=1e-5)
    # the public entry points take the CPU tensors to the same reference
    torch.testing.assert_close(SF.flash_attention(q, k, v, scale, True, doc_start=ds), o)
    assert not torch.allclose(SF.flash_attention(q, k, v, scale, True), o)
    with pytest.raises(ValueError, match="causal"):
        SF.flash_attention(q, k, v, scale, False, doc_start=ds)
    with pytest.raises(ValueError, match="int32"):
        SF.flash_attention(q, k, v, scale, True, doc_start=ds.long())


def _tiny_gpt(**kw):
    from smdt_amd.models.gpt import GPTModel
    from smdt_amd.models.transformer import TransformerConfig
    from smdt_amd.parallel import state as ps
    ps.destroy_model_parallel()
    cfg = TransformerConfig(num_layers=2, hidden_size=64, num_attention_heads=4, max_position_embeddings=32,
                            padded_vocab_size=64, hidden_dropout=0.0, attention_dropout=0.0, seed=3,
                            params_dtype=torch.float32, **kw)
    return GPTModel(cfg).eval()


@pytest.mark.parametrize("flash", [True, False])
def test_gpt_packed_documents_match_documents_run_alone(flash):
    """Two documents packed into one sample, with reset attention mask and position ids: every
    token's loss equals the loss of its document run alone. Without ``doc_start`` the second
    document attends into the first and its losses differ. ``flash=False`` takes the unfused path
    (dense mask from ``doc_start`` into the masked softmax)."""
    model = _tiny_gpt(use_flash_attn=flash)
    g = torch.Generator().manual_seed(2)
    d1 = torch.cat([torch.randint(8, 60, (11,), generator=g), torch.tensor([EOD])])       # ends with its EOD
    d2 = torch.randint(8, 60, (13,), generator=g)
    packed = torch.cat([d1, d2]).unsqueeze(0)                                               # [1, 25]
    toks, labels = packed[:, :-1], packed[:, 1:]
    _, _, pos = get_ltor_masks_and_position_ids(toks, EOD, True, False, False, build_attention_mask=False)
    ds = document_starts(toks, EOD)
    n1 = d1.numel()
    assert ds[0].tolist() == [0] * n1 + [n1] * (toks.shape[1] - n1) and pos[0, n1] == 0
    with torch.no_grad():
        packed_loss = model(toks, pos, None, labels=labels, doc_start=ds)
        plain_loss = model(toks, pos, None, labels=labels)
        alone1 = model(d1[None, :], None, None, labels=torch.cat([d1[1:], d2[:1]])[None, :])
        alone2 = model(d2[None, :-1], None, None, labels=d2[None, 1:])
    assert torch.isfinite(packed_loss).all()
    torch.testing.assert_close(packed_loss[:, :n1], alone1, atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(packed_loss[:, n1:], alone2, atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(plain_loss[:, :n1], alone1, atol=1e-5, rtol=1e-5)          # causal: unaffected
    assert (plain_loss[:, n1 + 1:] - alone2[:, 1:]).abs().max() > 1e-3                     # leaks across the EOD


def test_gpt_doc_start_survives_full_recompute():
    """The value travels with the call: the recompute in backward re-enters the layers with the
    same ``doc_start`` (gradients equal the run without recompute)."""
    g = torch.Generator().manual_seed(4)
    toks = torch.randint(8, 60, (2, 25), generator=g)
    toks[0, 9] = toks[1, 17] = EOD
    ds = document_starts(toks[:, :-1], EOD)
    grads = []
    for kw in ({}, {"recompute_granularity": "full", "recompute_method": "uniform", "recompute_num_layers": 1}):
        model = _tiny_gpt(**kw).train()
        model(toks[:, :-1], None, None, labels=toks[:, 1:], doc_start=ds).mean().backward()
        grads.append([p.grad.clone() for p in model.parameters()])
    for a, b in zip(*grads):
        torch.testing.assert_close(a, b, atol=1e-6, rtol=1e-5)


def test_reset_attention_mask_rejects_context_parallel(monkeypatch):
    from smdt_amd.train import arguments as A
    base = ["--num-layers", "2", "--hidden-size", "64", "--num-attention-heads", "4", "--seq-length", "32",
            "--max-position-embeddings", "32", "--micro-batch-size", "1", "--global-batch-size", "2",
            "--train-iters", "1", "--lr", "0.001", "--mock-data", "--vocab-size", "64", "--tokenizer-type",
            "NullTokenizer", "--reset-attention-mask"]
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(AssertionError, match="reset-attention-mask"):
        A.validate_args(A.parse_args(argv=base + ["--context-parallel-size", "2"]))
    without = [a for a in base if a != "--reset-attention-mask"]
    A.validate_args(A.parse_args(argv=without + ["--context-parallel-size", "2"]))      # cp alone is fine
    args = A.parse_args(argv=base)
    A.validate_args(args)
    assert args.reset_attention_mask and args.context_parallel_size == 1
