"""--moe-router-topk, CPU side: the routing twin against a token-by-token construction, the fp32 layer
with k = 2 (per-expert loop and grouped twin) against a per-token composition, the flag's plumbing."""
import math

import pytest
import torch

from test_moe_grouped import _validate


def tied_logits(T, E, seed=0):
    """A grid of four values (ties in most rows), row 0 all equal; E = 8: nobody picks the last expert."""
    lg = torch.randint(0, 4, (T, E), generator=torch.Generator().manual_seed(seed)).float() * 0.5
    if E == 8:
        lg[:, -1] = -10.0
    lg[0, :E - (E == 8)] = 1.0
    return lg


def brute_force_topk(lg, k):
    T, E = lg.shape
    R = (T * k // 256 + E) * 256
    experts, probs = [], []
    for t in range(T):
        es = sorted(range(E), key=lambda i: (-float(lg[t, i]), i))[:k]
        w = [math.exp(float(lg[t, e]) - float(lg[t, es[0]])) for e in es]
        experts.append(es)
        probs.append([x / sum(w) for x in w])
    counts = [sum(es.count(e) for es in experts) for e in range(E)]
    rows = [-(-c // 256) * 256 for c in counts]
    start = [sum(rows[:e]) for e in range(E)]
    fill, row_of, tok_of, p_of = list(start), [], [-1] * R, [0.0] * R
    for t in range(T):
        row_of.append([fill[e] for e in experts[t]])
        for e, p in zip(experts[t], probs[t]):
            tok_of[fill[e]], p_of[fill[e]] = t, p
            fill[e] += 1
    tile = [-1] * (R // 256)
    for e in range(E):
        tile[start[e] // 256:(start[e] + rows[e]) // 256] = [e] * (rows[e] // 256)
    return probs, experts, row_of, tok_of, tile, [[start[e], rows[e]] for e in range(E)], counts, p_of


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("E", [2, 8])
@pytest.mark.parametrize("T", [1, 257])
def test_topk_routing_twin_matches_brute_force(T, E, k):
    from smdt_amd.ops import functional as SF
    k = min(k, E)
    lg = tied_logits(T, E)
    got = SF.moe_route_ref(lg, topk=k)
    want = brute_force_topk(lg, k)
    assert len(got) == 8 and got[3].numel() == SF.moe_rows(T * k, E)
    assert got[1][0].tolist() == list(range(k))                  # a tie goes to the lower index
    assert E == 2 or int(got[6][-1]) == 0                        # the expert nobody picks
    for i in range(8):
        if i in (0, 7):
            torch.testing.assert_close(got[i], torch.tensor(want[i]), rtol=1e-6, atol=0)
        else:
            assert got[i].tolist() == want[i] and got[i].dtype == (torch.int64 if i == 3 else torch.int32), i
    assert SF.moe_route(lg, topk=k)[2].tolist() == want[2] and len(SF.moe_route(lg)) == 7   # k = 1: today's tuple


@pytest.mark.parametrize("grouped", [False, True])
def test_switch_layer_top2_equals_per_token_composition_fp32(grouped):
    """Output, dx and every parameter gradient (router included; None for an unpicked expert), fp32 defaults."""
    from smdt_amd.models.transformer import SwitchMLP, TransformerConfig
    from smdt_amd.parallel import state as ps
    ps.destroy_model_parallel()
    E, k, h = 4, 2, 32
    m = SwitchMLP(TransformerConfig(num_layers=2, hidden_size=h, ffn_hidden_size=64, num_attention_heads=2,
                                    max_position_embeddings=32, padded_vocab_size=64, params_dtype=torch.float32,
                                    hidden_dropout=0.0, attention_dropout=0.0, num_experts=E, seed=2,
                                    moe_router_topk=k, moe_grouped_gemm=grouped), 1)
    with torch.no_grad():
        m.router.mul_(50)
        m.router_bias[3] = -1e4                                   # nobody picks expert 3
    x = torch.randn(30, 2, h, generator=torch.Generator().manual_seed(0))
    wgt = torch.linspace(-1, 1, x.numel()).view_as(x)
    xi = x.clone().requires_grad_(True)
    out, bias = m(xi)
    (out * wgt).sum().backward()
    got = [out.detach(), xi.grad] + [p.grad for p in m.parameters()]
    m.zero_grad(set_to_none=True)
    xr = x.clone().requires_grad_(True)
    flat = xr.reshape(-1, h)
    logits = torch.nn.functional.linear(flat, m.router, m.router_bias)
    rows, lg = [], logits.tolist()
    for t in range(flat.shape[0]):
        es = sorted(range(E), key=lambda i: (-lg[t][i], i))[:k]
        p = torch.softmax(logits[t, es], -1)
        ys = [m.experts[e](flat[t].view(1, 1, h)) for e in es]
        rows.append(sum(p[j] * (y + yb).view(h) for j, (y, yb) in enumerate(ys)))
    ref = torch.stack(rows).view_as(x)
    (ref * wgt).sum().backward()
    want = [ref.detach(), xr.grad] + [p.grad for p in m.parameters()]
    names = ["out", "dx"] + [n for n, _ in m.named_parameters()]
    for n, g, w in zip(names, got, want):
        if w is None:
            assert g is None and "experts.3." in n, n
        else:
            torch.testing.assert_close(g, w, msg=lambda s, n=n: f"{n}: {s}")


def test_moe_router_topk_flag_reaches_the_config_and_is_validated(monkeypatch):
    from smdt_amd.models.transformer import TransformerConfig
    from smdt_amd.train import arguments as A
    from smdt_amd.train.checkpointing import CHECKPOINT_ARGS
    cfgs = []
    for extra in ([], ["--moe-router-topk", "2"]):
        a = _validate(["--num-experts", "4"] + extra, monkeypatch)
        a.padded_vocab_size = 64
        cfgs.append(A.core_transformer_config_from_args(a))
    assert [c.moe_router_topk for c in cfgs] == [1, 2] and "moe_router_topk" in CHECKPOINT_ARGS
    with pytest.raises(ValueError, match="--num-experts"):
        _validate(["--moe-router-topk", "2"], monkeypatch)
    for e, k in (("4", "0"), ("4", "5"), ("16", "9")):
        with pytest.raises(ValueError, match="--moe-router-topk must be in 1"):
            _validate(["--num-experts", e, "--moe-router-topk", k], monkeypatch)
    for kw, msg in ((dict(num_experts=4, moe_router_topk=5), "moe_router_topk"), (dict(moe_router_topk=2), "num_experts")):
        with pytest.raises(ValueError, match=msg):
            TransformerConfig(**kw)
