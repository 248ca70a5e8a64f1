"""sample.hip against its float64 twin (``SF.sample_tokens_ref`` / ``sample_filter_ref``).

Every sampled case goes through ``_check``: the returned token is in the twin's kept set and sits
where the twin's CDF puts u, to eps = 1e-5 of the kept mass Z: fp32 argument rounding plus a 1-ulp
exp2 is a relative error of at most (|a| ln 2 + 1) 2^-23 per term with |a| <= 64 for any term that
matters (5.4e-6 of Z), and the 2^-40 fixed-point grid adds less than 1e-7."""
import functools

import pytest
import torch

from smdt_amd.ops import functional as SF

pytestmark = pytest.mark.gpu

EPS = 1e-5
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
IDS = ["bf16", "fp16", "fp32"]
# (V, row stride): one entry, below a vector, a ragged tail, an odd stride (rows off 16-byte alignment),
# a GPT-2 vocabulary (staged in LDS for 16-bit), and beyond the staged size
GEOMS = [(1, 1), (33, 33), (1000, 1024), (4097, 4097), (50257, 50304), (70001, 70016)]
U16 = torch.cat([torch.tensor([0.0, 1 - 2.0 ** -24]), torch.rand(14, generator=torch.Generator().manual_seed(4))])


def _on_gpu(x, stride, reps):
    """Every row of x [R, V] ``reps`` times, as the [:, :V] view of a [R reps, stride] buffer."""
    buf = torch.zeros(x.shape[0] * reps, stride, dtype=x.dtype, device="cuda")
    buf[:, :x.shape[1]] = x.repeat_interleave(reps, 0).cuda()
    return buf[:, :x.shape[1]]


def _check(x, stride, T, k, p, u=U16):
    """x [R, V] (CPU, already in the kernel's dtype): every row with every u. Returns tok [R, len(u)]."""
    R, n = x.shape[0], u.numel()
    tok = SF.sample_tokens(_on_gpu(x, stride, n), u.repeat(R).float().cuda(), T, k, p).cpu().view(R, n)
    keep, pr = SF.sample_filter_ref(x, T, k, p)
    cdf = (pr * keep).cumsum(-1)
    Z = cdf[:, -1:]
    assert keep.gather(1, tok).all(), "a token outside the kept set"
    lo = torch.cat([torch.zeros(R, 1, dtype=cdf.dtype), cdf], 1).gather(1, tok)
    uz = u.double()[None, :] * Z
    off = torch.maximum(lo - uz, uz - cdf.gather(1, tok)) / Z
    print(f"V {x.shape[1]} T {T} k {k} p {p}: worst CDF miss {off.max().item():.3e} of Z (<= 0 is inside)")
    assert (lo - EPS * Z <= uz).all() and (uz < cdf.gather(1, tok) + EPS * Z).all(), off.max().item()
    return tok


@functools.lru_cache(None)
def _gauss(dtype, V):
    return (3 * torch.randn(4, V, generator=torch.Generator().manual_seed(V))).to(dtype)


@pytest.mark.parametrize("top_k", ["0", "1", "2", "50", "V - 1", "V", "V + 7"])
@pytest.mark.parametrize("V,stride", GEOMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gaussian_rows_top_k(dtype, V, stride, top_k):
    k = eval(top_k, {"V": V})
    for T in (0.7, 1.0, 1.5):
        _check(_gauss(dtype, V), stride, T, k, 1.0)


@pytest.mark.parametrize("top_p", [0.4, 0.6, 0.75, 0.83, 0.95])
@pytest.mark.parametrize("V,stride", GEOMS[1:])          # a 6-token head and a tail need V >= 7
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_constructed_top_p_rows(dtype, V, stride, top_p):
    pos = [0, V - 1] + ([1023, 1024] if V > 1025 else [V // 3, V // 3 + 1]) + [V // 2, V // 2 + 2]
    prob = torch.full((V,), 0.1 / (V - 6), dtype=torch.float64)
    prob[pos] = torch.tensor([0.1, 0.5, 0.03, 0.2, 0.02, 0.05], dtype=torch.float64)
    x = prob.log().to(dtype)[None]
    keep, pr = SF.sample_filter_ref(x, 1.0, 0, top_p)
    # the cut's margin, a condition on the rounded inputs: no class's mass-above is within .01 of top_p Z
    srt = pr[0].sort(descending=True).values
    above = torch.cat([torch.zeros(1, dtype=srt.dtype), srt.cumsum(0)[:-1]]) / srt.sum()
    assert (above[:6] - top_p).abs().min() >= 0.01 and abs(above[6] - top_p) >= 0.01, above[:7]
    assert int(keep.sum()) == {0.4: 1, 0.6: 2, 0.75: 3, 0.83: 4, 0.95: V}[top_p]      # .95: the whole tail class
    _check(x, stride, 1.0, 0, top_p)
    _check(x, stride, 1.0, V - 3, top_p)                 # top-k first (drops nothing above its tie class)


@pytest.mark.parametrize("V,stride", GEOMS[1:])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_ties_at_the_kth_value_and_minus_inf(dtype, V, stride):
    g = torch.Generator().manual_seed(V + 1)
    x = torch.randn(1, V, generator=g).clamp(max=2.0).to(dtype)
    where = torch.randperm(V, generator=g)[:8]
    x[0, where[:3]], x[0, where[3:]] = 3.0, 2.5          # k = 5 lands inside the five tied at 2.5
    keep, pr = SF.sample_filter_ref(x, 1.0, 5, 1.0)
    assert sorted(keep[0].nonzero().flatten().tolist()) == sorted(where.tolist())
    cdf = (pr * keep).cumsum(-1)[0]
    mid = ((cdf[where] - pr[0, where] / 2) / cdf[-1]).float()          # one u in the middle of every kept token
    tok = _check(x, stride, 1.0, 5, 1.0, torch.cat([mid, U16[:8]]))
    assert set(where.tolist()) == set(tok.flatten().tolist())

    y = _gauss(dtype, V)[:1].clone()
    y[0, torch.randperm(V, generator=g)[:V // 2]] = float("-inf")
    y[0, [0, V - 1]] = float("-inf")
    for p in (1.0, 0.9):
        assert torch.isfinite(y[0, _check(y, stride, 1.0, 0, p).flatten()]).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_greedy_takes_the_lowest_index_of_a_duplicated_maximum(dtype):
    x = _gauss(dtype, 4097).repeat(4, 1).clone()
    for b in range(16):
        x[b, [17 + 251 * b, 4096 - 3 * b]] = 40.0
    tok = SF.sample_tokens(_on_gpu(x, 4097, 1), do_sample=False)
    assert tok.cpu().tolist() == [17 + 251 * b for b in range(16)] == x.float().argmax(-1).tolist()


def test_bookkeeping_matches_the_twin_exactly():
    x = _gauss(torch.bfloat16, 1000)[[0, 1, 2, 3, 0, 1]]
    eos, pad, t = int(x[2].float().argmax()), 7, 3
    state = lambda dev: dict(seq=torch.full((6, 12), pad, device=dev), plen=torch.tensor([1, 5, 2, 8, 4, 3], device=dev),
                             finished=torch.tensor([0, 1, 0, 0, 1, 0], dtype=torch.bool, device=dev))
    cpu, gpu = state("cpu"), state("cuda")
    want = SF.sample_tokens_ref(x, do_sample=False, t=t, eos=eos, pad=pad, **cpu)
    got = SF.sample_tokens(_on_gpu(x, 1024, 1), do_sample=False, t=t, eos=eos, pad=pad, **gpu)
    assert cpu["finished"].tolist() == [False, True, True, False, True, False] and want[1] == pad
    assert torch.equal(got.cpu(), want)
    assert torch.equal(gpu["seq"].cpu(), cpu["seq"]) and torch.equal(gpu["finished"].cpu(), cpu["finished"])


def test_two_calls_are_bitwise_equal():
    lg, u = _on_gpu(_gauss(torch.bfloat16, 50257), 50304, 16), U16.repeat(4).cuda()
    a, b = SF.sample_tokens(lg, u, 0.7, 50, 0.9), SF.sample_tokens(lg, u, 0.7, 50, 0.9)
    assert torch.equal(a, b) and a.unique().numel() > 8


def test_generate_fused_on_a_bf16_model(monkeypatch):
    from smdt_amd.models.generation import generate
    from smdt_amd.models.gpt import GPTModel
    from smdt_amd.models.transformer import TransformerConfig
    from smdt_amd.parallel import state as ps
    ps.destroy_model_parallel()
    m = GPTModel(TransformerConfig(num_layers=2, hidden_size=256, num_attention_heads=4, activation="relu",
                                   position_embedding_type="learned_absolute", max_position_embeddings=128,
                                   padded_vocab_size=512, hidden_dropout=0.0, attention_dropout=0.0, seed=3,
                                   params_dtype=torch.bfloat16), device="cuda").eval()
    m.loss_vocab_size = 500
    ids = torch.randint(3, 500, (2, 11), generator=torch.Generator().manual_seed(9)).cuda()
    gen = lambda: torch.Generator(device="cuda").manual_seed(21)
    kw = dict(max_new_tokens=20, eos_token_id=None)
    greedy = generate(m, ids, **kw)
    fused = SF.sample_tokens

    def no_tie(logits, *a, **k):           # greedy equality is only promised where the maximum is unique
        top = logits.float().topk(2, dim=-1).values
        assert (top[:, 0] > top[:, 1]).all()
        return fused(logits, *a, **k)

    monkeypatch.setattr(SF, "sample_tokens", no_tie)
    assert torch.equal(generate(m, ids, sampler="fused", **kw), greedy)
    assert torch.equal(generate(m, ids, sampler="fused", do_sample=True, top_k=1, temperature=0.7, generator=gen(), **kw),
                       greedy)
    monkeypatch.setattr(SF, "sample_tokens", fused)
    skw = dict(kw, sampler="fused", do_sample=True, temperature=0.9, top_k=50, top_p=0.95)
    eager = generate(m, ids, generator=gen(), **skw)
    assert torch.equal(generate(m, ids, generator=gen(), use_graph=True, **skw), eager)
    assert int(eager.max()) < 500 and not torch.equal(eager, greedy)
