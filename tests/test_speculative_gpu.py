"""The multi-token decode step on the MI355X (decode_attn_multi.hip) and speculative ``generate``.

The attention kernel is judged row by row as ``_numerics.flash_excess`` judges flash attention: its
error against float64 of the same 16-bit inputs may be at most 2 x the error, in the same row, of
the torch twin that places the kernel's rounding points (``decode_attention_multi_ref(emulate=
True)``), plus one ulp of the type at the row's maximum. The append is compared bit for bit with T
single-token calls and, as both run one kernel, with the ``rope_`` kernel. End to end, speculative tokens must equal the plain greedy
ones unless the fp32 model itself cannot separate the two tokens at the first difference."""
import math

import pytest
import torch

from _numerics import flash_excess
from smdt_amd.ops import _ext
from smdt_amd.ops import functional as SF
from test_generation_gpu import FORMS, _pair, _ragged_prompt

pytestmark = pytest.mark.gpu

C = SF.DECODE_CHUNK
DTYPES = [torch.bfloat16, torch.float16]
HEADS = [(4, 4), (8, 2), (8, 1), (4, 2)]
TS = [1, 2, 5, 8]
PATTERNS = {
    "fresh": (lambda T: [T, T, T], 2 * C),                   # query 0 sees one key
    "edge": (lambda T: [C, C + 1, C + T - 1], 2 * C),        # the T limits straddle the chunk edge
    "mixed": (lambda T: [T, 2 * C + 37, 4 * C], 4 * C),
}


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _operands(dtype, D, nh, nkv, T, lens, cap, seed, nan_tail=True):
    g = _gen(seed)
    q = torch.randn(3, T, nh, D, device="cuda", generator=g).to(dtype)
    k = torch.randn(3, cap, nkv, D, device="cuda", generator=g).to(dtype)
    v = torch.randn(3, cap, nkv, D, device="cuda", generator=g).to(dtype)
    if nan_tail:
        for b, n in enumerate(lens):
            k[b, n:] = float("nan")
            v[b, n:] = float("nan")
    return q, k, v, torch.tensor(lens, dtype=torch.int32, device="cuda")


def test_limits_exported():
    assert _ext.ext().decode_attn_multi_max_t() == SF.DECODE_MULTI_MAX_T


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("nh,nkv", HEADS)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_decode_attention_multi_against_float64(dtype, D, nh, nkv, T, pattern):
    mk, cap = PATTERNS[pattern]
    lens = mk(T)
    q, k, v, lens_t = _operands(dtype, D, nh, nkv, T, lens, cap, D + 7 * nh + 13 * nkv + 31 * T + len(pattern))
    scale = 1.0 / math.sqrt(D)
    ref = SF.decode_attention_multi_ref(q.double(), k.double(), v.double(), lens_t, scale)
    emu = SF.decode_attention_multi_ref(q, k, v, lens_t, scale, emulate=True)
    out = SF.decode_attention_multi(q, k, v, lens_t, scale)
    assert out.shape == q.shape and out.dtype == q.dtype
    ratio, e_k, e_e = flash_excess(out, emu, ref, dtype)
    print(f"decode_attention_multi row-relative err: kernel {e_k:.3e} emulation {e_e:.3e} kernel/bound {ratio:.3f}")
    assert ratio <= 1.0, (ratio, e_k, e_e)
    if pattern == "fresh":           # query 0 sees a lone key: its output is that v row exactly
        assert torch.equal(out[:, 0].view(3, nkv, nh // nkv, D), v[:, 0].unsqueeze(2).expand(3, nkv, nh // nkv, D))
    if max(lens) < cap:              # a grid bound below the capacity gives the same bits
        assert torch.equal(SF.decode_attention_multi(q, k, v, lens_t, scale, max_len=max(lens)), out)


def test_t1_is_the_single_token_op():
    """T = 1 has ``decode_attention``'s meaning: both kernels within the twin's error of float64."""
    lens = [1, 2 * C + 37, 4 * C]
    q, k, v, lens_t = _operands(torch.bfloat16, 128, 8, 2, 1, lens, 4 * C, 3)
    ref = SF.decode_attention_ref(q[:, 0].double(), k.double(), v.double(), lens_t, 0.1)
    one = SF.decode_attention(q[:, 0].contiguous(), k, v, lens_t, 0.1)
    multi = SF.decode_attention_multi(q, k, v, lens_t, 0.1)[:, 0]
    e1, em = (one.double() - ref).abs().max().item(), (multi.double() - ref).abs().max().item()
    print(f"T = 1: decode_attention {e1:.3e}, decode_attention_multi {em:.3e}")
    assert em <= 2 * e1 + torch.finfo(torch.bfloat16).eps * ref.abs().max().item()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_future_blind(dtype):
    """Other (finite) values in the cache rows of the new tokens after t leave query t's bits
    unchanged: those rows are multiplied by an exact zero."""
    T, D, nh, nkv = 5, 128, 8, 2
    lens = [C, C + 1, C + T - 1]
    q, k, v, lens_t = _operands(dtype, D, nh, nkv, T, lens, 2 * C, 17)
    out = SF.decode_attention_multi(q, k, v, lens_t, 0.09)
    g = _gen(18)
    for t in range(T - 1):
        k2, v2 = k.clone(), v.clone()
        for b, n in enumerate(lens):
            first = n - T + t + 1                                   # the row of new token t + 1
            k2[b, first:n] = (37.0 * torch.randn(n - first, nkv, D, device="cuda", generator=g)).to(dtype)
            v2[b, first:n] = (37.0 * torch.randn(n - first, nkv, D, device="cuda", generator=g)).to(dtype)
        again = SF.decode_attention_multi(q, k2, v2, lens_t, 0.09)
        assert torch.equal(again[:, :t + 1], out[:, :t + 1]), t
        assert not torch.equal(again[:, t + 1:], out[:, t + 1:])


def test_bitwise_repeatable():
    lens = [3 * C + 5, 7, C + 1]
    q, k, v, lens_t = _operands(torch.bfloat16, 128, 8, 2, 5, lens, 3 * C + 5, 5)
    a = SF.decode_attention_multi(q, k, v, lens_t, 0.1)
    b = SF.decode_attention_multi(q, k, v, lens_t, 0.1)
    assert torch.equal(a, b)


def test_query_without_keys_returns_zeros():
    """lens < T: the first T - lens queries see no key."""
    T = 5
    q, k, v, lens_t = _operands(torch.bfloat16, 64, 4, 2, T, [2, 0, 5], C, 9)
    out = SF.decode_attention_multi(q, k, v, lens_t, 0.1)
    assert torch.isfinite(out).all()
    assert out[0, :3].abs().max() == 0 and out[1].abs().max() == 0
    assert torch.equal(out[0, 3].view(2, 2, 64), v[0, 0].unsqueeze(1).expand(2, 2, 64))


@pytest.mark.parametrize("nh,nkv,D,rot", [(4, 2, 64, 64), (16, 4, 128, 128), (4, 4, 64, 32), (12, 12, 64, None)])
@pytest.mark.parametrize("seq_first", [False, True], ids=["bt", "tb"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_decode_rope_append_multi_bitwise(dtype, seq_first, nh, nkv, D, rot):
    """The bytes of T calls of ``decode_rope_append`` (q and both caches), from a [B, T, W] tensor
    and from the model's sequence-first [T, B, W] as a transposed view. Both sides run one kernel,
    so the transposed case is anchored independently as well: q / k of every token against the
    ``rope_`` kernel at position pos[b] + t, v against the source rows."""
    B, T, cap = 4, 5, 40
    g = _gen(7)
    W = (nh + 2 * nkv) * D
    if seq_first:
        qkv = torch.randn(T, B, W, device="cuda", generator=g).to(dtype).transpose(0, 1)
        assert not qkv.is_contiguous()
    else:
        qkv = torch.randn(B, T, W, device="cuda", generator=g).to(dtype)
    pos = torch.tensor([0, cap - T, 17, 5], dtype=torch.int32, device="cuda")
    kc = torch.randn(B, cap, nkv, D, device="cuda", generator=g).to(dtype)
    vc = torch.randn(B, cap, nkv, D, device="cuda", generator=g).to(dtype)
    k1, v1 = kc.clone(), vc.clone()
    rope = None
    if rot is not None:
        cos, sin = SF.rope_tables(cap, rot, device="cuda")
        rope = (cos, sin, rot)
    want = torch.stack([SF.decode_rope_append(qkv[:, t].contiguous(), k1, v1, pos + t, nh, nkv, D, rope=rope)
                        for t in range(T)], dim=1)
    got = SF.decode_rope_append_multi(qkv, kc, vc, pos, nh, nkv, D, rope=rope)
    assert got.shape == (B, T, nh, D) and torch.equal(got, want)
    assert torch.equal(kc, k1) and torch.equal(vc, v1)
    if not seq_first:
        return
    want_qk = qkv[:, :, :(nh + nkv) * D].reshape(B, T, nh + nkv, D).clone()
    if rot is not None:
        for b in range(B):           # the rope_ kernel on a [cap] sequence holding token t's row at pos[b] + t
            x = torch.zeros(cap, nh + nkv, D, device="cuda", dtype=dtype)
            x[int(pos[b]):int(pos[b]) + T] = want_qk[b]
            _ext.ext().rope_(x, cos, sin, rot, 1, cap, False)
            want_qk[b] = x[int(pos[b]):int(pos[b]) + T]
    want_v = qkv[:, :, (nh + nkv) * D:].reshape(B, T, nkv, D)
    assert torch.equal(got, want_qk[:, :, :nh])
    for b in range(B):
        p = int(pos[b])
        assert torch.equal(kc[b, p:p + T], want_qk[b, :, nh:])
        assert torch.equal(vc[b, p:p + T], want_v[b])


def test_refused_shapes_raise():
    def ops(nh, nkv, D, dtype, T):
        q = torch.zeros(2, T, nh, D, device="cuda", dtype=dtype)
        kc = torch.zeros(2, 16, nkv, D, device="cuda", dtype=dtype)
        return q, kc, kc.clone(), torch.full((2,), 8, dtype=torch.int32, device="cuda")
    code = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
    for nh, nkv, D, dtype, T in [(4, 4, 64, torch.bfloat16, 0), (4, 4, 64, torch.bfloat16, 9),
                                 (4, 4, 96, torch.bfloat16, 2), (6, 2, 64, torch.bfloat16, 2),
                                 (4, 4, 64, torch.float32, 2)]:
        q, kc, vc, lens = ops(nh, nkv, D, dtype, T)
        assert not SF.decode_attention_multi_supported(q, kc, vc)
        assert not _ext.ext().decode_attn_multi_supported(code[dtype], D, nh, nkv, T)
        with pytest.raises((RuntimeError, ValueError)):
            SF.decode_attention_multi(q, kc, vc, lens, 0.125)
    q, kc, vc, lens = ops(4, 4, 64, torch.bfloat16, 2)
    assert SF.decode_attention_multi_supported(q, kc, vc) and _ext.ext().decode_attn_multi_supported(1, 64, 4, 4, 2)
    with pytest.raises(ValueError):
        SF.decode_attention_multi(q, kc, vc, lens, 0.125, max_len=17)
    k8 = kc.to(torch.float8_e4m3fn)                                  # an MXFP8 cache's element tensors
    assert not SF.decode_attention_multi_supported(q, k8, k8.clone())
    with pytest.raises(RuntimeError):
        SF.decode_attention_multi(q, k8, k8.clone(), lens, 0.125)
    with pytest.raises((RuntimeError, ValueError)):
        SF.decode_rope_append_multi(torch.zeros(2, 9, 12 * 64, device="cuda", dtype=torch.bfloat16), kc, vc, lens,
                                    4, 4, 64)


# ------------------------------------------------------------------------------- the model hooks
@pytest.mark.parametrize("form", sorted(FORMS))
def test_forward_extend_as_close_to_fp32_as_decode_steps(form):
    """Teacher-forced on the fp32 model's greedy tokens: T = 5 tokens through one ``forward_extend``
    and through 5 ``forward_decode`` steps; the former's logits may be at most 2 x as far from the
    fp32 model's as the latter's."""
    from smdt_amd.models.generation import KVCache, generate
    ref, gpu = _pair(form)
    ids, mask = _ragged_prompt()
    T = 5
    seq = generate(ref, ids, mask, max_new_tokens=T + 1, eos_token_id=None)
    plen = mask.sum(1)
    toks = torch.stack([seq[b, plen[b]:plen[b] + T] for b in range(2)]).cuda()           # [2, T]
    with torch.no_grad():
        caches = [KVCache(gpu.cfg, 2, 11 + T, torch.bfloat16, "cuda") for _ in range(2)]
        for c in caches:
            gpu.forward_prefill(ids.cuda(), plen.cuda(), c)
            c.lens.copy_(plen)
        steps = []
        for t in range(T):
            caches[0].advance()
            steps.append(gpu.forward_decode(toks[:, t], caches[0]))
        steps = torch.stack(steps, 1).float().cpu()[..., :500]
        caches[1].advance(T)
        ext = gpu.forward_extend(toks, caches[1]).float().cpu()[..., :500]
        assert torch.equal(caches[0].lens, caches[1].lens)
        e_s = e_x = 0.0
        for b in range(2):
            n = int(plen[b])
            want = ref(seq[b:b + 1, :n + T])[0, n:, :500]                                 # [T, V] fp32
            e_s = max(e_s, (steps[b] - want).abs().max().item())
            e_x = max(e_x, (ext[b] - want).abs().max().item())
    print(f"{form}: max logit error vs fp32: forward_extend {e_x:.4e}, {T} forward_decode steps {e_s:.4e}")
    assert e_x <= 2 * e_s, (e_x, e_s)


def test_forward_extend_refuses_an_mx_cache():
    from smdt_amd.models.generation import KVCache
    _, gpu = _pair("llama")
    cache = KVCache(gpu.cfg, 2, 32, torch.bfloat16, "cuda", format="mxfp8")
    cache.advance(2)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="mxfp8"):
        gpu.forward_extend(torch.zeros(2, 2, dtype=torch.long, device="cuda"), cache)


# ------------------------------------------------------------------------------- end to end
_DRAFTS = {}


def _other_seed_draft():
    """A bf16 llama of another seed with the target's vocabulary."""
    if "d" not in _DRAFTS:
        from smdt_amd.models.gpt import GPTModel
        from smdt_amd.models.transformer import TransformerConfig
        _pair("llama")
        kw = dict(FORMS["llama"], max_position_embeddings=128, padded_vocab_size=512, hidden_dropout=0.0,
                  attention_dropout=0.0, seed=11)
        d = GPTModel(TransformerConfig(**kw, params_dtype=torch.bfloat16), device="cuda").eval()
        d.loss_vocab_size = 500
        _DRAFTS["d"] = d
    return _DRAFTS["d"]


def _assert_tokens_or_fp32_tie(spec, plain, ids, mask, what):
    """Equal tokens; otherwise, at the first difference of a row, the fp32 model teacher-forced on
    the common prefix may separate the two tokens' logits by at most twice the 16-bit path's
    measured logit error there."""
    if torch.equal(spec, plain):
        print(f"{what}: speculative tokens equal the plain greedy tokens")
        return
    ref, gpu = _pair("llama")
    plen = mask.sum(1)
    for b in range(spec.shape[0]):
        diff = (spec[b] != plain[b]).nonzero()
        if not len(diff):
            continue
        i = int(diff[0])
        assert i >= int(plen[b]), "the prompt was changed"
        prefix = plain[b:b + 1, :i].cpu()
        with torch.no_grad():
            want = ref(prefix)[0, -1, :500]
            have = gpu(prefix.cuda())[0, -1, :500].float().cpu()
        err = (have - want).abs().max().item()
        gap = abs(want[int(spec[b, i])] - want[int(plain[b, i])]).item()
        print(f"{what}: row {b} differs at {i}: fp32 logit gap {gap:.4e}, 16-bit logit error {err:.4e}")
        assert gap <= 2 * err, (b, i, gap, err)


@pytest.mark.parametrize("draft", ["self", "other"])
def test_speculative_generate_returns_the_greedy_tokens(draft):
    from smdt_amd.models.generation import generate
    _, gpu = _pair("llama")
    d = gpu if draft == "self" else _other_seed_draft()
    ids, mask = _ragged_prompt()
    ids, mask = ids.cuda(), mask.cuda()
    plain = generate(gpu, ids, mask, max_new_tokens=22, eos_token_id=None)
    st = {}
    spec = generate(gpu, ids, mask, max_new_tokens=22, eos_token_id=None, draft_model=d, num_draft_tokens=4, stats=st)
    print(f"{draft} draft: {st}")
    assert spec.shape == plain.shape and st["rounds"] >= 1 and 0 <= st["accepted"] <= st["drafted"]
    _assert_tokens_or_fp32_tie(spec, plain, ids, mask, f"{draft} draft")


def test_speculative_graph_replay_returns_the_eager_tokens():
    from smdt_amd.models.generation import generate
    _, gpu = _pair("llama")
    ids, mask = _ragged_prompt()
    ids, mask = ids.cuda(), mask.cuda()
    kw = dict(max_new_tokens=30, eos_token_id=None, draft_model=_other_seed_draft(), num_draft_tokens=4)
    s0, s1 = {}, {}
    eager = generate(gpu, ids, mask, stats=s0, **kw)
    graph = generate(gpu, ids, mask, use_graph=True, stats=s1, **kw)
    assert torch.equal(eager, graph) and s0 == s1 and s0["rounds"] >= 3


def test_speculative_weight_format_native():
    from smdt_amd.models.generation import generate
    _, gpu = _pair("llama")
    ids, mask = _ragged_prompt()
    ids, mask = ids.cuda(), mask.cuda()
    plain = generate(gpu, ids, mask, max_new_tokens=22, eos_token_id=None, weight_format="native")
    spec = generate(gpu, ids, mask, max_new_tokens=22, eos_token_id=None, weight_format="native", draft_model=gpu,
                    num_draft_tokens=4)
    _assert_tokens_or_fp32_tie(spec, plain, ids, mask, "weight_format native")


def test_rounds_do_not_synchronise():
    """After the first round (first use of every shape) further rounds run with host
    synchronisation made an error: a round reads nothing on the host; the caller's poll is the only
    read."""
    from smdt_amd.models.generation import SpeculativeState
    _, gpu = _pair("llama")
    ids, mask = _ragged_prompt()
    ids, mask = ids.cuda(), mask.cuda()
    with torch.no_grad():
        st = SpeculativeState(gpu, _other_seed_draft(), ids, mask, 40, 4, None, 0, None, None)
        x0 = st.round(st.x0)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for _ in range(4):
                x0 = st.round(x0)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert int(st.counters[0]) == 5 and 5 <= int(st.nout.min()) and not st.all_done()
