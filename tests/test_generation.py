"""KV-cache text generation on the CPU (fp32, the torch twins of decode_attn.hip): greedy parity
with ``transformers``, cached == uncached, ragged batches, EOS, sampling, the twins against brute
force, every refusal, and the recipe script."""
import json
import math
import os
import subprocess
import sys
import tempfile

import pytest
import torch

from smdt_amd.models import generation as G
from smdt_amd.models import transformer as T
from smdt_amd.models.hf import HFCausalLM
from smdt_amd.ops import functional as SF
from smdt_amd.parallel import state as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the tiny configs of tests/test_hf_models.py
CFGS = {
    "opt": dict(model_type="opt", hidden_size=64, num_hidden_layers=2, num_attention_heads=4, ffn_dim=128,
                vocab_size=100, max_position_embeddings=64, activation_function="relu", do_layer_norm_before=True,
                enable_bias=True, word_embed_proj_dim=64, pad_token_id=1, bos_token_id=2, eos_token_id=2),
    "llama": dict(model_type="llama", hidden_size=64, num_hidden_layers=2, num_attention_heads=4,
                  num_key_value_heads=2, intermediate_size=96, vocab_size=100, max_position_embeddings=64,
                  rms_norm_eps=1e-6, rope_theta=10000.0, hidden_act="silu", tie_word_embeddings=False,
                  bos_token_id=1, eos_token_id=2),
    "gpt2": dict(model_type="gpt2", n_embd=64, n_layer=2, n_head=4, vocab_size=100, n_positions=64,
                 activation_function="gelu_new", bos_token_id=0, eos_token_id=0),
}
KINDS = sorted(CFGS)
NEW = 16

_MODELS = {}


def _model(kind):
    if kind not in _MODELS:
        torch.manual_seed(0)
        _MODELS[kind] = HFCausalLM(CFGS[kind], params_dtype=torch.float32).eval()
    return _MODELS[kind]


def _prompt():
    return torch.randint(3, 100, (2, 6), generator=torch.Generator().manual_seed(1))


_GREEDY = {}


def _greedy(kind):
    """The cached greedy path of the shared inputs, [2, 6 + NEW] (computed once, never modified)."""
    if kind not in _GREEDY:
        _GREEDY[kind] = _model(kind).generate(_prompt(), max_new_tokens=NEW, eos_token_id=None)
    return _GREEDY[kind]


# ------------------------------------------------------------------------------- greedy parity
@pytest.mark.parametrize("kind", KINDS)
def test_greedy_matches_transformers_token_for_token(kind):
    transformers = pytest.importorskip("transformers")
    m, ids = _model(kind), _prompt()
    with tempfile.TemporaryDirectory() as d:
        m.save_pretrained(d)
        ref = transformers.AutoModelForCausalLM.from_pretrained(d, dtype=torch.float32,
                                                                attn_implementation="eager").eval()
    with torch.no_grad():
        want = ref.generate(ids, attention_mask=torch.ones_like(ids), do_sample=False, max_new_tokens=NEW,
                            min_new_tokens=NEW, eos_token_id=None, pad_token_id=0)
    got = _greedy(kind)
    assert got.shape == (2, 6 + NEW)
    assert torch.equal(got, want), (got.tolist(), want.tolist())


@pytest.mark.parametrize("kind", KINDS)
def test_cached_equals_uncached(kind):
    m, seq = _model(kind), _prompt()
    with torch.no_grad():
        for _ in range(NEW):
            logits = m(seq)[1]                                   # full forward over the growing prefix
            seq = torch.cat([seq, logits[:, -1].argmax(-1, keepdim=True)], dim=1)
    assert torch.equal(_greedy(kind), seq)


# ------------------------------------------------------------------------------- ragged batch
@pytest.mark.parametrize("kind", KINDS)
def test_ragged_batch_rows_equal_rows_alone(kind):
    m = _model(kind)
    g = torch.Generator().manual_seed(2)
    a, b = torch.randint(3, 100, (1, 3), generator=g), torch.randint(3, 100, (1, 9), generator=g)
    pad = 1
    ids = torch.full((2, 9), 77)             # a real token id in the pad slots: the mask alone decides
    ids[0, :3], ids[1] = a[0], b[0]
    mask = torch.zeros(2, 9, dtype=torch.long)
    mask[0, :3], mask[1] = 1, 1
    out = m.generate(ids, mask, max_new_tokens=NEW, eos_token_id=None, pad_token_id=pad)
    alone_a = m.generate(a, max_new_tokens=NEW, eos_token_id=None, pad_token_id=pad)
    alone_b = m.generate(b, max_new_tokens=NEW, eos_token_id=None, pad_token_id=pad)
    assert out.shape == (2, 9 + NEW)
    # layout: prompt, new tokens immediately after, then pad
    assert torch.equal(out[0, :3 + NEW], alone_a[0])
    assert torch.equal(out[0, 3 + NEW:], torch.full((6,), pad))
    assert torch.equal(out[1], alone_b[0])


# ------------------------------------------------------------------------------- EOS
def _eos_case():
    """(kind, row, step, eos): a token one row of a greedy path emits mid-path and not earlier, and
    the other row never before it."""
    for kind in KINDS:
        new = _greedy(kind)[:, 6:]
        for row in (0, 1):
            for t in range(2, NEW - 2):
                eos = int(new[row, t])
                if eos not in new[row, :t].tolist() and eos not in new[1 - row].tolist():
                    return kind, row, t, eos
    raise AssertionError("no usable EOS token on the greedy paths")


def test_eos_row_pads_and_other_row_unaffected():
    kind, row, t, eos = _eos_case()
    m, pad = _model(kind), 1
    assert eos != pad
    out = m.generate(_prompt(), max_new_tokens=NEW, eos_token_id=eos, pad_token_id=pad)
    want = _greedy(kind).clone()
    want[row, 6 + t + 1:] = pad
    assert torch.equal(out, want)


def test_loop_stops_once_all_rows_finished(monkeypatch):
    kind, row, t, eos = _eos_case()
    m = _model(kind)
    calls = []
    orig = m.model.forward_decode
    monkeypatch.setattr(m.model, "forward_decode", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    new = 50
    out = m.generate(_prompt()[row:row + 1], max_new_tokens=new, eos_token_id=eos, pad_token_id=1)
    assert out.shape == (1, 6 + new)
    assert torch.equal(out[0, :6 + t + 1], _greedy(kind)[row, :6 + t + 1])
    assert torch.equal(out[0, 6 + t + 1:], torch.full((new - t - 1,), 1))
    # the host polls every EOS_POLL_STEPS steps: the first poll after the EOS ends the loop
    assert len(calls) == G.EOS_POLL_STEPS - 1 < new - 1


# ------------------------------------------------------------------------------- sampling
def test_top_k_1_equals_greedy():
    out = _model("llama").generate(_prompt(), max_new_tokens=NEW, eos_token_id=None, do_sample=True, top_k=1,
                                   temperature=0.7, generator=torch.Generator().manual_seed(5))
    assert torch.equal(out, _greedy("llama"))


def test_same_seed_same_tokens_and_real_vocab_only():
    m = _model("opt")
    assert m.cfg.padded_vocab_size == 128 and m.vocab_size == 100
    # the padding rows of the tied embedding get a large norm: their logits would win if they were sampled
    w = m.model.embedding.weight
    saved = w.data[100:].clone()
    try:
        w.data[100:] = 3.0
        kw = dict(max_new_tokens=NEW, eos_token_id=None, do_sample=True, temperature=1.5)
        a = m.generate(_prompt(), generator=torch.Generator().manual_seed(7), **kw)
        b = m.generate(_prompt(), generator=torch.Generator().manual_seed(7), **kw)
        c = m.generate(_prompt(), generator=torch.Generator().manual_seed(8), **kw)
        g = m.generate(_prompt(), max_new_tokens=NEW, eos_token_id=None)
    finally:
        w.data[100:] = saved
    assert torch.equal(a, b) and not torch.equal(a, c)
    for out in (a, c, g):
        assert int(out.max()) < 100 and int(out.min()) >= 0


def test_top_p_stays_inside_the_nucleus():
    torch.manual_seed(3)
    logits = torch.randn(4, 100) * 2.0
    p = 0.6
    kept = torch.isfinite(G.filter_logits(logits, top_p=p))
    probs = torch.softmax(logits, -1)
    for r in range(4):
        order = sorted(range(100), key=lambda i: -float(probs[r, i]))
        nucleus, mass = set(), 0.0
        for i in order:                       # the smallest set of most likely tokens reaching p
            nucleus.add(i)
            mass += float(probs[r, i])
            if mass >= p:
                break
        assert set(kept[r].nonzero().flatten().tolist()) == nucleus
    gen = torch.Generator().manual_seed(0)
    for _ in range(50):
        tok = G._pick(logits, True, 1.0, 0, p, gen)
        assert bool(kept[torch.arange(4), tok].all())


# ------------------------------------------------------------------------------- twins
def _brute(q, k, v, lens, scale):
    B, nh, D = q.shape
    nkv = k.shape[2]
    out = torch.zeros(B, nh, D, dtype=torch.float64)
    for b in range(B):
        n = int(lens[b])
        for h in range(nh):
            kk, vv = k[b, :n, h // (nh // nkv)].double(), v[b, :n, h // (nh // nkv)].double()
            out[b, h] = torch.softmax(kk @ q[b, h].double() * scale, 0) @ vv
    return out


@pytest.mark.parametrize("nh,nkv", [(4, 4), (8, 2)])
@pytest.mark.parametrize("lens", [[1, 1, 1], [20, 20, 20], [1, 13, 20]])
def test_decode_attention_ref_against_float64(nh, nkv, lens):
    torch.manual_seed(0)
    B, cap, D = 3, 20, 16
    q, k, v = torch.randn(B, nh, D), torch.randn(B, cap, nkv, D), torch.randn(B, cap, nkv, D)
    lens_t = torch.tensor(lens, dtype=torch.int32)
    want = _brute(q, k, v, lens_t, 0.25)
    for b in range(B):                      # the tail must not matter, whatever it holds
        k[b, lens[b]:] = float("nan")
        v[b, lens[b]:] = float("nan")
    got = SF.decode_attention(q, k, v, lens_t, 0.25)
    assert got.dtype == q.dtype and torch.isfinite(got).all()
    torch.testing.assert_close(got.double(), want, rtol=1e-5, atol=1e-6)
    got64 = SF.decode_attention_ref(q.double(), k.double(), v.double(), lens_t, 0.25)
    torch.testing.assert_close(got64, want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("rot", [16, 8, None])
def test_decode_rope_append_ref_reproduces_rope_ref(rot):
    torch.manual_seed(0)
    B, cap, nh, nkv, hd = 3, 10, 4, 2, 16
    qkv = torch.randn(B, (nh + 2 * nkv) * hd)
    pos = torch.tensor([0, 9, 4], dtype=torch.int32)
    k = torch.randn(B, cap, nkv, hd)
    v = torch.randn(B, cap, nkv, hd)
    k0, v0 = k.clone(), v.clone()
    rope = None
    if rot is not None:
        cos, sin = SF.rope_tables(cap, rot)
        rope = (cos, sin, rot)
    q = SF.decode_rope_append(qkv, k, v, pos, nh, nkv, hd, rope=rope)
    qin = qkv[:, :nh * hd].view(B, nh, hd)
    kin = qkv[:, nh * hd:(nh + nkv) * hd].view(B, nkv, hd)
    vin = qkv[:, (nh + nkv) * hd:].view(B, nkv, hd)
    if rope is not None:
        qin = SF._rope_ref(qin, cos, sin, rot, pos.long())
        kin = SF._rope_ref(kin, cos, sin, rot, pos.long())
    assert torch.equal(q, qin)
    for b in range(B):
        p = int(pos[b])
        assert torch.equal(k[b, p], kin[b]) and torch.equal(v[b, p], vin[b])
        k0[b, p], v0[b, p] = k[b, p], v[b, p]
    assert torch.equal(k, k0) and torch.equal(v, v0)          # no other row changed


def test_supported_predicate():
    q = torch.zeros(2, 8, 64, dtype=torch.bfloat16)
    kc = torch.zeros(2, 32, 2, 64, dtype=torch.bfloat16)
    assert SF.decode_attention_supported(q, kc, kc)
    assert not SF.decode_attention_supported(q.float(), kc.float(), kc.float())
    assert not SF.decode_attention_supported(torch.zeros(2, 8, 96, dtype=torch.bfloat16),
                                             torch.zeros(2, 32, 2, 96, dtype=torch.bfloat16))
    assert not SF.decode_attention_supported(torch.zeros(2, 6, 64, dtype=torch.bfloat16),
                                             torch.zeros(2, 32, 4, 64, dtype=torch.bfloat16))
    assert not SF.decode_attention_supported(q, kc.half(), kc.half())


# ------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("field", ["tp", "pp", "cp"])
def test_refuses_model_parallel(monkeypatch, field):
    m = _model("llama")
    st = ps.get_state()
    monkeypatch.setattr(st, field, 2)                 # a stubbed parallel state
    with pytest.raises(NotImplementedError, match="parallel"):
        m.generate(_prompt(), max_new_tokens=2)


def test_refuses_sequence_parallel(monkeypatch):
    m = _model("llama")
    monkeypatch.setattr(m.model.cfg, "sequence_parallel", True)
    with pytest.raises(NotImplementedError, match="sequence parallelism"):
        m.generate(_prompt(), max_new_tokens=2)


def test_refuses_active_pack_context():
    m = _model("llama")
    with T.packed_sequences(torch.arange(4), 2, 6):
        with pytest.raises(RuntimeError, match="packed_sequences"):
            m.generate(_prompt(), max_new_tokens=2)


def test_refuses_prompts_not_right_padded():
    m = _model("llama")
    mask = torch.ones(2, 6, dtype=torch.long)
    mask[0, 0] = 0                                    # left-padded
    with pytest.raises(ValueError, match="right-padded"):
        m.generate(_prompt(), mask, max_new_tokens=2)
    mask = torch.ones(2, 6, dtype=torch.long)
    mask[1, 2] = 0                                    # a hole
    with pytest.raises(ValueError, match="right-padded"):
        m.generate(_prompt(), mask, max_new_tokens=2)


def test_refuses_beyond_max_positions_and_capacity():
    m = _model("llama")
    assert m.cfg.max_position_embeddings == 64
    with pytest.raises(ValueError, match="max_position_embeddings"):
        m.generate(_prompt(), max_new_tokens=59)
    m.generate(_prompt(), max_new_tokens=58, eos_token_id=None)         # 6 + 58 == 64 fits
    cache = G.KVCache(m.cfg, 2, 10, torch.float32)
    with pytest.raises(ValueError, match="KV cache"):
        m.generate(_prompt(), max_new_tokens=5, cache=cache)
    out = m.generate(_prompt(), max_new_tokens=4, eos_token_id=None, cache=cache)
    assert torch.equal(out, _greedy("llama")[:, :10])


def test_training_mode_is_restored():
    m = _model("gpt2")
    m.train()
    try:
        out = m.generate(_prompt(), max_new_tokens=NEW, eos_token_id=None)
        assert m.training and m.model.decoder.layers[0].training
    finally:
        m.eval()
    assert torch.equal(out, _greedy("gpt2"))


# ------------------------------------------------------------------------------- recipe
def test_recipe_generate_prints_ids_with_the_offline_tokenizer(tmp_path):
    from smdt_amd.data import sft
    torch.manual_seed(0)
    hf = dict(CFGS["opt"], vocab_size=50272, max_position_embeddings=128)
    m = HFCausalLM(hf, params_dtype=torch.float32)
    d = str(tmp_path / "model")
    m.save_pretrained(d)
    sft.load_tokenizer("facebook/opt-125m").save_pretrained(d)
    script = os.path.join(ROOT, "recipes", "4_training_alpaca_deepspeed", "generate.py")
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, script, "--model_dir", d, "--instruction", "Name three colours.",
                        "--max_new_tokens", "5"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    rec = json.loads(lines[-1])
    assert 1 <= len(rec["new_token_ids"]) <= 5 and all(0 <= t < 50272 for t in rec["new_token_ids"])
    assert "cannot decode" in r.stdout
    assert math.isfinite(rec["prompt_tokens"]) and rec["prompt_tokens"] > 10
