"""Speculative decoding on the CPU (fp32, the torch twins of decode_attn_multi.hip): the twins
against brute force and against the single-token twins, ``speculative_accept`` on hand-made tables,
``forward_extend`` against successive ``forward_decode`` steps, speculative ``generate`` against
plain greedy ``generate`` token for token, and every refusal."""
import copy

import pytest
import torch

from smdt_amd.models import generation as G
from smdt_amd.models.hf import HFCausalLM
from smdt_amd.ops import functional as SF
from test_generation import CFGS, KINDS, NEW, _eos_case, _greedy, _model, _prompt

_DRAFTS = {}


def _draft(kind, how):
    """"seed": the same architecture from another seed. "swapped": a copy of the target whose output-
    embedding rows of a few token ids on its greedy paths are swapped in pairs, so it proposes the
    wrong token exactly where the target emits one of them: a deterministic mix of accepts and
    rejects that differs between the rows."""
    if (kind, how) not in _DRAFTS:
        if how == "seed":
            d = HFCausalLM(CFGS[kind], params_dtype=torch.float32, seed=7).eval()
        else:
            d = copy.deepcopy(_model(kind)).eval()
            new = _greedy(kind)[:, 6:]
            ids = [int(new[0, 3]), int(new[1, 5]), int(new[0, 9]), int(new[1, 12])]
            w = d.model.output_weight if d.model.output_weight is not None else d.model.embedding.weight
            with torch.no_grad():
                for t in dict.fromkeys(ids):
                    o = (t + 1) % 100
                    rows = w[[t, o]].clone()
                    w[t], w[o] = rows[1], rows[0]
        _DRAFTS[(kind, how)] = d
    return _DRAFTS[(kind, how)]


# ------------------------------------------------------------------------------- twins
def _brute(q, k, v, lens, scale):
    B, T, nh, D = q.shape
    nkv = k.shape[2]
    out = torch.zeros(B, T, nh, D, dtype=torch.float64)
    for b in range(B):
        for t in range(T):
            n = int(lens[b]) - T + t + 1
            for h in range(nh):
                if n > 0:
                    kk, vv = k[b, :n, h // (nh // nkv)].double(), v[b, :n, h // (nh // nkv)].double()
                    out[b, t, h] = torch.softmax(kk @ q[b, t, h].double() * scale, 0) @ vv
    return out


@pytest.mark.parametrize("nh,nkv", [(4, 4), (8, 2)])
@pytest.mark.parametrize("pattern", ["fresh", "full", "mixed"])
@pytest.mark.parametrize("T", [1, 2, 5, 8])
def test_decode_attention_multi_ref_against_float64(T, pattern, nh, nkv):
    torch.manual_seed(0)
    B, cap, D = 3, 20, 16
    lens = {"fresh": [T, T, T], "full": [20, 20, 20], "mixed": [T, 13, 20]}[pattern]
    q, k, v = torch.randn(B, T, nh, D), torch.randn(B, cap, nkv, D), torch.randn(B, cap, nkv, D)
    lens_t = torch.tensor(lens, dtype=torch.int32)
    want = _brute(q, k, v, lens_t, 0.25)
    for b in range(B):                      # the tail must not matter, whatever it holds
        k[b, lens[b]:] = float("nan")
        v[b, lens[b]:] = float("nan")
    got = SF.decode_attention_multi(q, k, v, lens_t, 0.25)
    assert got.dtype == q.dtype and got.shape == q.shape and torch.isfinite(got).all()
    torch.testing.assert_close(got.double(), want, rtol=1e-5, atol=1e-6)
    got64 = SF.decode_attention_multi_ref(q.double(), k.double(), v.double(), lens_t, 0.25)
    torch.testing.assert_close(got64, want, rtol=1e-12, atol=1e-12)
    # in fp32 the emulation's only extra rounding (P to fp32) is the identity: it is the same function
    emu = SF.decode_attention_multi_ref(q, k, v, lens_t, 0.25, emulate=True)
    torch.testing.assert_close(emu.double(), want, rtol=1e-5, atol=1e-6)


def test_emulation_rounds_p_per_chunk():
    """bf16 operands over three chunks: the emulation differs from the plain twin (it rounds P) and
    stays within a few bf16 ulps of it; NaN beyond ``lens`` does not reach it."""
    torch.manual_seed(1)
    C = SF.DECODE_CHUNK
    q = torch.randn(2, 3, 4, 16).bfloat16()
    k, v = torch.randn(2, 2 * C + 9, 2, 16).bfloat16(), torch.randn(2, 2 * C + 9, 2, 16).bfloat16()
    lens = torch.tensor([2 * C + 9, C + 1], dtype=torch.int32)
    k[1, C + 1:] = float("nan")
    v[1, C + 1:] = float("nan")
    plain = SF.decode_attention_multi_ref(q, k, v, lens, 0.25)
    emu = SF.decode_attention_multi_ref(q, k, v, lens, 0.25, emulate=True)
    assert torch.isfinite(emu).all() and not torch.equal(plain, emu)
    assert (plain.float() - emu.float()).abs().max() <= 4 * torch.finfo(torch.bfloat16).eps * plain.float().abs().max()


def test_t1_bits_equal_the_single_token_twin():
    torch.manual_seed(2)
    q, k, v = torch.randn(3, 1, 8, 16), torch.randn(3, 20, 2, 16), torch.randn(3, 20, 2, 16)
    lens = torch.tensor([1, 13, 20], dtype=torch.int32)
    a = SF.decode_attention_multi_ref(q, k, v, lens, 0.25)
    b = SF.decode_attention_ref(q[:, 0].contiguous(), k, v, lens, 0.25)
    assert torch.equal(a[:, 0], b)


@pytest.mark.parametrize("rot", [16, 8, None])
def test_decode_rope_append_multi_ref_equals_t_calls(rot):
    torch.manual_seed(0)
    B, T, cap, nh, nkv, hd = 3, 4, 12, 4, 2, 16
    qkv = torch.randn(T, B, (nh + 2 * nkv) * hd).transpose(0, 1)            # the model's layout
    pos = torch.tensor([0, 8, 4], dtype=torch.int32)
    k, v = torch.randn(B, cap, nkv, hd), torch.randn(B, cap, nkv, hd)
    k1, v1 = k.clone(), v.clone()
    rope = None
    if rot is not None:
        cos, sin = SF.rope_tables(cap, rot)
        rope = (cos, sin, rot)
    want = torch.stack([SF.decode_rope_append_ref(qkv[:, t], k1, v1, pos + t, nh, nkv, hd, rope) for t in range(T)], 1)
    got = SF.decode_rope_append_multi(qkv, k, v, pos, nh, nkv, hd, rope=rope)
    assert got.shape == (B, T, nh, hd) and torch.equal(got, want)
    assert torch.equal(k, k1) and torch.equal(v, v1)
    with pytest.raises(ValueError):
        SF.decode_rope_append_multi(torch.randn(B, 9, (nh + 2 * nkv) * hd), k, v, pos, nh, nkv, hd)


def test_supported_predicate():
    kc = torch.zeros(2, 32, 2, 64, dtype=torch.bfloat16)
    ok = torch.zeros(2, 5, 8, 64, dtype=torch.bfloat16)
    assert SF.decode_attention_multi_supported(ok, kc, kc)
    assert SF.decode_attention_multi_supported(ok[:, :1], kc, kc) and SF.DECODE_MULTI_MAX_T == 8
    assert not SF.decode_attention_multi_supported(torch.zeros(2, 9, 8, 64, dtype=torch.bfloat16), kc, kc)
    assert not SF.decode_attention_multi_supported(ok[:, :0], kc, kc)
    assert not SF.decode_attention_multi_supported(ok[:, 0], kc, kc)
    assert not SF.decode_attention_multi_supported(ok.float(), kc.float(), kc.float())
    assert not SF.decode_attention_multi_supported(torch.zeros(2, 5, 6, 64, dtype=torch.bfloat16), kc, kc)
    assert not SF.decode_attention_multi_supported(ok, kc.to(torch.float8_e4m3fn), kc.to(torch.float8_e4m3fn))


# ------------------------------------------------------------------------------- the accept step
def _accept(draft, target, remaining, finished, eos=None, pad=-1):
    out = G.speculative_accept(torch.tensor(draft), torch.tensor(target), torch.tensor(remaining),
                               torch.tensor(finished), eos, pad)
    return [o.tolist() for o in out]


def test_accept_prefix_lengths():
    # rows: n = 0 (first draft wrong), n = k (all right), n = 2 (a later match after a miss does not count)
    draft = [[9, 9, 9, 9], [1, 2, 3, 4], [1, 2, 9, 4]]
    target = [[1, 2, 3, 4, 5], [1, 2, 3, 4, 5], [1, 2, 3, 4, 5]]
    toks, count, done, n = _accept(draft, target, [10, 10, 10], [False] * 3)
    assert n == [0, 4, 2] and count == [1, 5, 3] and done == [False] * 3
    assert toks == [[1, -1, -1, -1, -1], [1, 2, 3, 4, 5], [1, 2, 3, -1, -1]]


def test_accept_cuts_at_eos_remaining_and_finished_rows():
    draft = [[1, 2, 3, 4]] * 5
    target = [[1, 2, 3, 4, 5]] * 5
    #            EOS inside   EOS is p_n   budget 2     budget cuts before the EOS   finished
    remaining = [10, 10, 2, 2, 10]
    finished = [False, False, False, False, True]
    toks, count, done, n = _accept(draft, target, remaining, finished, eos=3, pad=0)
    assert n == [4] * 5
    assert count == [3, 3, 2, 2, 0]
    assert done == [True, True, False, False, True]
    assert toks[0] == [1, 2, 3, 0, 0] and toks[2] == [1, 2, 0, 0, 0] and toks[4] == [0] * 5
    # EOS as the target's own token after a rejected draft
    toks, count, done, n = _accept([[1, 9, 9, 9]], [[1, 3, 7, 7, 7]], [10], [False], eos=3, pad=0)
    assert n == [1] and count == [2] and done == [True] and toks == [[1, 3, 0, 0, 0]]
    # a row with nothing left emits nothing and is not marked finished by an EOS it does not emit
    toks, count, done, n = _accept([[3, 3, 3, 3]], [[3, 3, 3, 3, 3]], [0], [False], eos=3, pad=0)
    assert count == [0] and done == [False] and toks == [[0] * 5]


# ------------------------------------------------------------------------------- the model hooks
@pytest.mark.parametrize("kind", KINDS)
def test_forward_extend_equals_successive_decode_steps(kind):
    """T tokens through one ``forward_extend`` against T ``forward_decode`` steps. The bound is twice
    the difference already present between ``forward_decode`` and the full forward on those tokens
    (two existing paths), measured here."""
    m = _model(kind).model
    seq = _greedy(kind)
    T = 5
    ids, plen = seq[:, :6], torch.full((2,), 6)
    with torch.no_grad():
        caches = [G.KVCache(m.cfg, 2, 6 + T, torch.float32) for _ in range(2)]
        for c in caches:
            m.forward_prefill(ids, plen, c)
            c.lens.copy_(plen)
        steps = []
        for t in range(T):
            caches[0].advance()
            steps.append(m.forward_decode(seq[:, 6 + t], caches[0]))
        steps = torch.stack(steps, 1)                                            # [2, T, V]
        caches[1].advance(T)
        ext = m.forward_extend(seq[:, 6:6 + T], caches[1])
        full = m(seq[:, :6 + T])[:, 6:]
    assert ext.shape == steps.shape
    assert torch.equal(caches[0].lens, caches[1].lens) and torch.equal(caches[1].pos, plen.int())
    for a, b in zip(caches[0].k + caches[0].v, caches[1].k + caches[1].v):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)
    base = (steps - full).abs().max().item()
    got = (ext - steps).abs().max().item()
    print(f"{kind}: |forward_extend - decode steps| {got:.3e}, |decode steps - full forward| {base:.3e}")
    assert base > 0 and got <= 2 * base


def test_forward_extend_refuses_an_mx_cache():
    m = _model("llama").model
    m64 = HFCausalLM(dict(CFGS["llama"], hidden_size=256), params_dtype=torch.float32).eval().model   # head dim 64
    cache = G.KVCache(m64.cfg, 2, 16, torch.float32, format="mxfp8")
    cache.advance(2)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="mxfp8"):
        m64.forward_extend(torch.zeros(2, 2, dtype=torch.long), cache)
    assert m is not m64


def test_advance_default_is_one_token():
    c = G.KVCache(_model("opt").cfg, 2, 8, torch.float32)
    c.lens.copy_(torch.tensor([3, 1]))
    c.advance()
    assert c.pos.tolist() == [3, 1] and c.lens.tolist() == [4, 2]
    c.advance(3)
    assert c.pos.tolist() == [4, 2] and c.lens.tolist() == [7, 5]


# ------------------------------------------------------------------------------- generation
@pytest.mark.parametrize("kind", KINDS)
def test_self_draft_returns_greedy_and_accepts_everything(kind):
    m, st = _model(kind), {}
    out = m.generate(_prompt(), max_new_tokens=NEW, eos_token_id=None, draft_model=m, num_draft_tokens=4, stats=st)
    assert torch.equal(out, _greedy(kind))
    assert st["drafted"] == st["accepted"] > 0 and st["rounds"] == 3           # 1 + 3 * 5 = 16 tokens


@pytest.mark.parametrize("how", ["seed", "swapped"])
@pytest.mark.parametrize("kind", KINDS)
def test_other_drafts_return_greedy(kind, how):
    m, st = _model(kind), {}
    out = m.generate(_prompt(), max_new_tokens=NEW, eos_token_id=None, draft_model=_draft(kind, how),
                     num_draft_tokens=4, stats=st)
    assert torch.equal(out, _greedy(kind)), st
    assert 0 <= st["accepted"] <= st["drafted"] and st["drafted"] % 4 == 0
    if how == "swapped":              # a mix of accepts and rejects
        assert 0 < st["accepted"] < st["drafted"], st


@pytest.mark.parametrize("k,new", [(1, 16), (7, 16), (4, 13), (3, 2), (4, 1)])
def test_draft_lengths_and_budgets(k, new):
    """k = 1 and k = 7, and budgets that are not a multiple of k + 1 (the last round is cut)."""
    m = _model("llama")
    for d in (m, _draft("llama", "swapped")):
        out = m.generate(_prompt(), max_new_tokens=new, eos_token_id=None, draft_model=d, num_draft_tokens=k)
        assert out.shape == (2, 6 + new) and torch.equal(out, _greedy("llama")[:, :6 + new])


@pytest.mark.parametrize("how", ["self", "swapped"])
def test_ragged_prompts(how):
    kind = "opt"
    m = _model(kind)
    g = torch.Generator().manual_seed(2)
    a, b = torch.randint(3, 100, (1, 3), generator=g), torch.randint(3, 100, (1, 9), generator=g)
    ids = torch.full((2, 9), 77)
    ids[0, :3], ids[1] = a[0], b[0]
    mask = torch.zeros(2, 9, dtype=torch.long)
    mask[0, :3], mask[1] = 1, 1
    want = m.generate(ids, mask, max_new_tokens=NEW, eos_token_id=None, pad_token_id=1)
    d = m if how == "self" else _draft(kind, "swapped")
    out = m.generate(ids, mask, max_new_tokens=NEW, eos_token_id=None, pad_token_id=1, draft_model=d,
                     num_draft_tokens=4)
    assert torch.equal(out, want)


@pytest.mark.parametrize("how", ["self", "swapped"])
def test_eos_row_pads_and_other_row_unaffected(how):
    kind, row, t, eos = _eos_case()
    m, pad = _model(kind), 1
    want = m.generate(_prompt(), max_new_tokens=NEW, eos_token_id=eos, pad_token_id=pad)
    assert (want[row, 6 + t + 1:] == pad).all() and int(want[row, 6 + t]) == eos
    d = m if how == "self" else _draft(kind, "swapped")
    out = m.generate(_prompt(), max_new_tokens=NEW, eos_token_id=eos, pad_token_id=pad, draft_model=d,
                     num_draft_tokens=4)
    assert torch.equal(out, want)


def test_loop_stops_once_all_rows_finished(monkeypatch):
    kind, row, t, eos = _eos_case()
    m = _model(kind)
    calls = []
    orig = m.model.forward_extend
    monkeypatch.setattr(m.model, "forward_extend", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    new = 50
    out = m.generate(_prompt()[row:row + 1], max_new_tokens=new, eos_token_id=eos, pad_token_id=1, draft_model=m,
                     num_draft_tokens=4)
    assert out.shape == (1, 6 + new)
    assert torch.equal(out[0, :6 + t + 1], _greedy(kind)[row, :6 + t + 1])
    assert torch.equal(out[0, 6 + t + 1:], torch.full((new - t - 1,), 1))
    assert len(calls) == -(-t // 5)                 # the rounds that reach new token t, and no more


def test_passed_cache_is_used():
    m = _model("llama")
    cache = G.KVCache(m.cfg, 2, 6 + 8 + 4, torch.float32)
    out = m.generate(_prompt(), max_new_tokens=8, eos_token_id=None, cache=cache, draft_model=m, num_draft_tokens=4)
    assert torch.equal(out, _greedy("llama")[:, :14])
    assert cache.lens.tolist() == [6 + 7, 6 + 7]            # every emitted token but the last is cached


# ------------------------------------------------------------------------------- refusals and state
def test_refusals_name_their_cause():
    m = _model("llama")
    ids = _prompt()
    with pytest.raises(NotImplementedError, match="do_sample"):
        m.generate(ids, max_new_tokens=4, do_sample=True, draft_model=m)
    with pytest.raises(NotImplementedError, match="kv_cache_format"):
        m.generate(ids, max_new_tokens=4, kv_cache_format="mxfp8", draft_model=m)
    for k in (0, 8, -1):
        with pytest.raises(ValueError, match="num_draft_tokens"):
            m.generate(ids, max_new_tokens=4, draft_model=m, num_draft_tokens=k)
    other_vocab = HFCausalLM(dict(CFGS["llama"], vocab_size=90), params_dtype=torch.float32).eval()
    with pytest.raises(ValueError, match="vocabulary"):
        m.generate(ids, max_new_tokens=4, draft_model=other_vocab)
    # 6 + 54 + 4 == 64 fits both; one more position does not; a shorter draft is named
    assert m.cfg.max_position_embeddings == 64
    m.generate(ids, max_new_tokens=54, eos_token_id=None, draft_model=m, num_draft_tokens=4)
    with pytest.raises(ValueError, match="num_draft_tokens 4 = 65 exceeds max_position_embeddings 64 of the target"):
        m.generate(ids, max_new_tokens=55, draft_model=m, num_draft_tokens=4)
    short = HFCausalLM(dict(CFGS["llama"], max_position_embeddings=32), params_dtype=torch.float32).eval()
    with pytest.raises(ValueError, match="of the draft model"):
        m.generate(ids, max_new_tokens=24, draft_model=short, num_draft_tokens=4)
    with pytest.raises(ValueError, match="the draft model is refused"):
        m.generate(ids, max_new_tokens=30, draft_model=short, num_draft_tokens=4)
    cache = G.KVCache(m.cfg, 2, 6 + 8 + 3, torch.float32)
    with pytest.raises(ValueError, match="KV cache"):
        m.generate(ids, max_new_tokens=8, cache=cache, draft_model=m, num_draft_tokens=4)


def test_draft_that_fails_refuse_is_named(monkeypatch):
    m, d = _model("llama"), _draft("llama", "seed")
    monkeypatch.setattr(d.model.cfg, "sequence_parallel", True)
    with pytest.raises(NotImplementedError, match="the draft model is refused.*sequence parallelism"):
        m.generate(_prompt(), max_new_tokens=2, draft_model=d)


def test_training_mode_of_both_models_is_restored():
    m, d = _model("gpt2"), _draft("gpt2", "seed")
    m.train()
    try:
        out = m.generate(_prompt(), max_new_tokens=NEW, eos_token_id=None, draft_model=d, num_draft_tokens=2)
        assert m.training and not d.training
        d.train()
        with pytest.raises(ValueError):
            m.generate(_prompt(), max_new_tokens=4, draft_model=d, num_draft_tokens=0)
        assert m.training and d.training
        m.eval()
        m.generate(_prompt(), max_new_tokens=4, eos_token_id=None, draft_model=d, num_draft_tokens=2)
        assert not m.training and d.training
    finally:
        m.eval()
        d.eval()
    assert torch.equal(out, _greedy("gpt2"))


# ------------------------------------------------------------------------------- recipe
def test_recipe_generate_with_a_draft_directory(tmp_path):
    import json
    import os
    import subprocess
    import sys
    from smdt_amd.data import sft
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    torch.manual_seed(0)
    m = HFCausalLM(dict(CFGS["opt"], vocab_size=50272, max_position_embeddings=128), params_dtype=torch.float32)
    d = str(tmp_path / "model")
    m.save_pretrained(d)
    sft.load_tokenizer("facebook/opt-125m").save_pretrained(d)
    script = os.path.join(root, "recipes", "4_training_alpaca_deepspeed", "generate.py")
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    base = [sys.executable, script, "--model_dir", d, "--instruction", "Name three colours.", "--max_new_tokens", "7"]
    recs = []
    for extra in ([], ["--draft_model_dir", d, "--num_draft_tokens", "3"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        recs.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))
    assert recs[1]["new_token_ids"] == recs[0]["new_token_ids"]
    assert recs[1]["rounds"] == 2 and recs[1]["accepted"] == recs[1]["drafted"] == 6 and "rounds" not in recs[0]
