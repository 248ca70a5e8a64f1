"""KV-cache text generation for ``GPTModel`` (and ``HFCausalLM.generate`` on top of it).

Prefill: the right-padded prompt batch [B, Lmax] runs through the unchanged causal forward (flash
attention on the GPU); causality keeps a real token blind to the pads on its right. Every attention
layer copies its post-RoPE K and V into cache rows 0 .. Lmax - 1 (``transformer.kv_prefill``),
``lens`` is set to the prompt lengths and only the last real position of each row goes through the
LM head.

Decode step: one new token per sequence. ``ParallelAttention.forward_decode`` runs the QKV linear,
rotates q / k at ``pos = lens`` and appends k / v into that cache row (over the pad K / V the
prefill left there), then single-query attention over ``lens + 1`` keys (csrc/kernels/
decode_attn.hip). ``lens`` and ``pos`` live on the device and advance there once per step: no
kernel and no Python code of a step reads a length on the host, so with the static shapes
(``max_len = capacity``) a step can be captured in a graph (``use_graph=True``,
``train.graphs.CapturedStep``).

``kv_cache_format="mxfp8"`` stores the cache as MXFP8 (E4M3 elements and one E8M0 scale byte per 32,
51.6 % of the 16-bit bytes; ``ops.functional.KV_CACHE_FORMATS``): every row is the MX quantisation
of the 16-bit row the default cache would have held, written by the prefill store and by the
quantising append, and read by csrc/kernels/decode_attn_mx.hip. The prefill's own attention still
runs on the 16-bit K / V through flash attention.

Speculative decoding (``generate(draft_model=...)``, greedy): a round lets the draft model propose
``k = num_draft_tokens`` tokens in k + 1 single-token steps and the target check them all in ONE
multi-token step (``GPTModel.forward_extend``, csrc/kernels/decode_attn_multi.hip: its linears see
B (k + 1) rows of the same weight stream). ``speculative_accept`` keeps the longest prefix the
target agrees with plus the target's own next token, so the output is the plain greedy output.
A whole round stays on the device and can be captured in one graph.
"""
from __future__ import annotations

from typing import Optional

import torch

from ..ops import functional as SF
from ..parallel import state as ps
from ..parallel import decode_weights as dw
from ..parallel import tensor_parallel as tp
from . import transformer as _T
from .transformer import TransformerConfig

EOS_POLL_STEPS = 16     # the host asks whether every row has finished at most this often


def _check_kv_format(cfg: TransformerConfig, fmt, who: str):
    """Every refusal of a ``kv_cache_format``, naming the cause, before anything is allocated."""
    if fmt is None:
        return
    if fmt not in SF.KV_CACHE_FORMATS:
        raise ValueError(f"{who}: kv_cache_format must be None or one of {SF.KV_CACHE_FORMATS}, got {fmt!r}")
    D, nh, nkv = cfg.kv_channels, cfg.num_attention_heads, cfg.num_query_groups
    if D % SF.MX_BLOCK:
        raise ValueError(f"{who}: kv_cache_format {fmt!r} needs a head dimension that is a multiple of "
                         f"{SF.MX_BLOCK} (one scale per {SF.MX_BLOCK} elements), got {D}")
    if D not in (64, 128) or nh % nkv or nh // nkv not in (1, 2, 4, 8):
        raise ValueError(f"{who}: kv_cache_format {fmt!r} needs a head dimension in (64, 128) and "
                         f"num_attention_heads / num_query_groups in (1, 2, 4, 8) (the decode kernel's set), got "
                         f"head dimension {D} and {nh} / {nkv}")
    if nkv * D > SF._KV_MX_MAX_ROW:
        raise ValueError(f"{who}: kv_cache_format {fmt!r} needs num_query_groups * head dimension <= "
                         f"{SF._KV_MX_MAX_ROW} (the append kernel's staged row), got {nkv * D}")


class KVCache:
    """Per-layer K / V of shape [B, capacity, nkv, D], ``lens`` (int32 [B], device: the valid keys
    of each sequence) and ``pos`` (int32 [B]: the row the current step's token is written to).
    ``format="mxfp8"``: ``k`` / ``v`` hold float8_e4m3fn elements and ``k_scale`` / ``v_scale``
    [B, capacity, nkv, D / 32] their uint8 E8M0 scales (``dtype`` is then unused)."""

    def __init__(self, cfg: TransformerConfig, batch: int, capacity: int, dtype=None, device=None, format=None):
        if batch < 1 or capacity < 1:
            raise ValueError(f"KVCache: batch {batch} and capacity {capacity} must be positive")
        _check_kv_format(cfg, format, "KVCache")
        self.batch, self.capacity = int(batch), int(capacity)
        self.max_len = self.capacity          # bounds the decode kernel's grid (static: capturable)
        self.format = format
        dtype = dtype or cfg.params_dtype
        shape = (self.batch, self.capacity, cfg.num_query_groups, cfg.kv_channels)
        if format is not None:
            dtype = torch.float8_e4m3fn
            sshape = shape[:3] + (cfg.kv_channels // SF.MX_BLOCK,)
            # scale byte 127 is 2^0: an unwritten row reads as zeros, as in the 16-bit cache
            self.k_scale = [torch.full(sshape, 127, dtype=torch.uint8, device=device) for _ in range(cfg.num_layers)]
            self.v_scale = [torch.full(sshape, 127, dtype=torch.uint8, device=device) for _ in range(cfg.num_layers)]
        self.k = [torch.zeros(shape, dtype=dtype, device=device) for _ in range(cfg.num_layers)]
        self.v = [torch.zeros(shape, dtype=dtype, device=device) for _ in range(cfg.num_layers)]
        self.lens = torch.zeros(self.batch, dtype=torch.int32, device=device)
        self.pos = torch.zeros(self.batch, dtype=torch.int32, device=device)

    def store_prefill(self, attn, qkv):
        """Called by every attention layer under ``transformer.kv_prefill``: ``qkv`` [L, B, W] is the
        layer's fused projection output after RoPE."""
        L, B = qkv.shape[0], qkv.shape[1]
        if B != self.batch or L > self.capacity:
            raise RuntimeError(f"KVCache: a prompt batch [{B}, {L}] does not fit the cache "
                               f"[{self.batch}, capacity {self.capacity}]")
        _, k, v = SF._qkv_views(qkv, attn.nh, attn.nkv, attn.hd, True)            # [B, L, nkv, D]
        if self.format is not None:
            i = attn.layer_number
            return SF.kv_store_mx(k, v, self.k[i], self.k_scale[i], self.v[i], self.v_scale[i])
        self.k[attn.layer_number][:, :L].copy_(k)
        self.v[attn.layer_number][:, :L].copy_(v)

    def advance(self, n: int = 1):
        """Start a decode step of ``n`` new tokens per sequence: they go to rows ``pos = lens`` ..
        ``pos + n - 1`` and are ``n`` more keys."""
        self.pos.copy_(self.lens)
        self.lens.add_(n)


def _refuse(model, input_ids, attention_mask, max_new_tokens, cache, kv_cache_format=None):
    """Everything generation does not do raises here, naming the cause."""
    cfg = model.cfg
    st = ps.get_state()
    if st.tp > 1 or st.pp > 1 or st.cp > 1:
        raise NotImplementedError(f"generate: tensor / pipeline / context parallel models are not supported "
                                  f"(TP {st.tp}, PP {st.pp}, CP {st.cp}); generate from an unsharded model")
    if cfg.sequence_parallel:
        raise NotImplementedError("generate: sequence parallelism (sequence_parallel=True) is not supported")
    if _T._PACK["idx"] is not None:
        raise RuntimeError("generate: a padding-free packed_sequences context is active; generation takes the "
                           "padded [B, L] batch")
    if not (model.pre_process and model.post_process):
        raise NotImplementedError("generate: the model must own the embedding and the LM head (one pipeline stage)")
    if input_ids.dim() != 2 or input_ids.shape[1] < 1:
        raise ValueError(f"generate: input_ids must be [B, L] with L >= 1, got {tuple(input_ids.shape)}")
    if max_new_tokens < 1:
        raise ValueError(f"generate: max_new_tokens must be positive, got {max_new_tokens}")
    B, L = input_ids.shape
    if attention_mask is not None:
        if attention_mask.shape != input_ids.shape:
            raise ValueError(f"generate: attention_mask {tuple(attention_mask.shape)} does not match input_ids "
                             f"{tuple(input_ids.shape)}")
        m = attention_mask.bool().cpu()            # once per call, before the loop
        if not bool(m[:, 0].all()) or bool((m[:, 1:] & ~m[:, :-1]).any()):
            raise ValueError("generate: prompts must be right-padded (attention_mask rows of ones followed by zeros, "
                             "at least one token per row)")
    total = L + max_new_tokens
    if total > cfg.max_position_embeddings:
        raise ValueError(f"generate: prompt length {L} + max_new_tokens {max_new_tokens} = {total} exceeds "
                         f"max_position_embeddings {cfg.max_position_embeddings}")
    if cache is not None and (cache.batch != B or total > cache.capacity):
        raise ValueError(f"generate: prompt length {L} + max_new_tokens {max_new_tokens} = {total} for batch {B} "
                         f"exceeds the KV cache (batch {cache.batch}, capacity {cache.capacity})")
    _check_kv_format(cfg, kv_cache_format, "generate")
    if cache is not None and kv_cache_format is not None and cache.format != kv_cache_format:
        raise ValueError(f"generate: kv_cache_format {kv_cache_format!r} disagrees with the passed cache, whose format "
                         f"is {cache.format!r}")


def _decode_weights(model, weight_format):
    """The ``dw.DecodeWeights`` of a ``generate(weight_format=...)`` call (None for None): every
    refusal raises here, the quantised copies are made (or found in the cache) and the kernel's
    workspace and the dequantisation scratch are allocated, all before the first decode step."""
    if weight_format is None:
        return None
    if weight_format not in SF.DECODE_LINEAR_FORMATS:
        raise ValueError(f"generate: weight_format must be None or one of {SF.DECODE_LINEAR_FORMATS}, "
                         f"got {weight_format!r}")
    cfg = model.cfg
    if cfg.num_experts:
        raise NotImplementedError(f"generate(weight_format={weight_format!r}): Switch MLP models (num_experts "
                                  f"{cfg.num_experts}) are not supported")
    head = model.output_weight if model.output_weight is not None else model.embedding.weight
    linears = []
    for name, mod in model.decoder.named_modules():
        if isinstance(mod, (tp.ColumnParallelLinear, tp.RowParallelLinear)):
            if mod._fp8 is not None:
                raise RuntimeError(f"generate(weight_format={weight_format!r}): {name} carries _fp8 (an FP8 / MXFP8 "
                                   "training linear); weight formats are for models with plain 16-bit linears")
            linears.append((name, mod.weight, False))
    linears.append(("the LM head", head, True))
    state = dw.DecodeWeights(weight_format, head_weight=head)
    state.prepare(linears)
    return state


def filter_logits(logits, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0):
    """fp32 logits [B, V] -> the logits sampling draws from: divided by the temperature, all but
    the ``top_k`` largest and everything outside the ``top_p`` nucleus (the smallest set of most
    likely tokens whose probability reaches ``top_p``) set to -inf."""
    logits = logits.float()
    if temperature != 1.0:
        logits = logits / temperature
    if top_k and 0 < top_k < logits.shape[-1]:
        kth = logits.topk(top_k, dim=-1).values[:, -1:]
        logits = logits.masked_fill(logits < kth, float("-inf"))
    if top_p < 1.0:
        srt, idx = logits.sort(dim=-1, descending=True)
        probs = torch.softmax(srt, dim=-1)
        before = probs.cumsum(dim=-1) - probs            # mass of the more likely tokens
        drop = before >= top_p                           # never the most likely token (before = 0)
        logits = logits.masked_fill(torch.zeros_like(drop).scatter(1, idx, drop), float("-inf"))
    return logits


def _pick(logits, do_sample, temperature, top_k, top_p, generator):
    if not do_sample:
        return logits.argmax(dim=-1)
    probs = torch.softmax(filter_logits(logits, temperature, top_k, top_p), dim=-1)
    # exponential race (the draw torch.multinomial makes for one sample), without a host sync
    q = torch.empty_like(probs).exponential_(1.0, generator=generator)
    return (probs / q).argmax(dim=-1)


@torch.no_grad()
def generate(model, input_ids, attention_mask=None, max_new_tokens: int = 32, do_sample: bool = False,
             temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, eos_token_id: Optional[int] = None,
             pad_token_id: int = 0, generator: Optional[torch.Generator] = None, use_graph: bool = False,
             cache: Optional[KVCache] = None, weight_format: Optional[str] = None,
             kv_cache_format: Optional[str] = None, draft_model=None, num_draft_tokens: int = 4,
             stats: Optional[dict] = None):
    """Greedy or sampled continuation of the right-padded prompts ``input_ids`` [B, Lmax]
    (``attention_mask`` marks the real tokens; None: every row is Lmax long) with a KV cache.

    Returns ``sequences`` [B, Lmax + max_new_tokens]: row b holds its prompt, then its new tokens
    immediately after, then ``pad_token_id``. A row that has emitted ``eos_token_id`` emits pad from
    then on; the loop stops once every row has finished, which the host checks every
    ``EOS_POLL_STEPS`` steps (no per-step synchronisation). Sampling (``do_sample``) draws from
    ``filter_logits`` over the real vocabulary (``model.loss_vocab_size``), so vocab padding columns
    are never returned. ``use_graph=True`` (GPU) captures one decode step and replays it.
    ``cache``: a ``KVCache`` to reuse (its capacity must hold Lmax + max_new_tokens).

    ``weight_format``: None (the model's own linears), or how the layers' linears read their
    weights: "native" streams the 16-bit parameters through the decode GEMM kernel
    (csrc/kernels/decode_linear.hip) in steps of up to 16 sequences; "mxfp8" / "mxfp4" (bf16 models)
    stream a cached block-scaled copy instead, and the prefill and batches above 16 run the
    ordinary linear over the same dequantised values. The LM head always uses the native form; the
    16-bit parameters stay resident and ``state_dict`` is unchanged.

    ``kv_cache_format``: None (a cache in the model dtype) or "mxfp8": K and V are stored as MXFP8,
    the MX quantisation of the 16-bit rows, at 51.6 % of the bytes (head dimension 64 or 128,
    heads / kv heads in 1, 2, 4, 8; bf16 and fp16 models). A passed ``cache`` keeps its own format;
    naming a different one here raises. Independent of ``weight_format`` and ``use_graph``.

    ``draft_model``: a second model with the same vocabulary (``model`` itself is allowed: the
    self-draft upper bound) turns on greedy speculative decoding with ``num_draft_tokens`` = k
    drafted tokens per round, 1 <= k <= ``SF.DECODE_MULTI_MAX_T`` - 1. The tokens are those of the
    plain greedy call. Positions up to Lmax + max_new_tokens + k - 1 are touched (rejected drafts),
    so both models' ``max_position_embeddings`` and a passed ``cache`` must hold Lmax +
    max_new_tokens + k. ``weight_format`` applies to the target only; sampling and
    ``kv_cache_format`` are refused. ``use_graph=True`` captures one whole round. ``stats``, if a
    dict, receives ``rounds``, ``drafted`` and ``accepted`` (drafted tokens the target agreed with),
    both counted over the rows that were still generating."""
    if draft_model is not None:
        _refuse_speculative(model, draft_model, input_ids, attention_mask, max_new_tokens, cache, kv_cache_format,
                            do_sample, num_draft_tokens)
        state = _decode_weights(model, weight_format)
        modes = (model.training, draft_model.training)
        model.eval()
        draft_model.eval()
        try:
            return _generate_speculative(model, draft_model, input_ids, attention_mask, int(max_new_tokens),
                                         int(num_draft_tokens), eos_token_id, int(pad_token_id), use_graph, cache,
                                         state, stats)
        finally:
            draft_model.train(modes[1])
            model.train(modes[0])
    _refuse(model, input_ids, attention_mask, max_new_tokens, cache, kv_cache_format)
    state = _decode_weights(model, weight_format)
    if do_sample and temperature <= 0:
        raise ValueError(f"generate: temperature must be positive, got {temperature}")
    was_training = model.training
    model.eval()
    try:
        with dw.decode_weights(state):
            return _generate(model, input_ids, attention_mask, int(max_new_tokens), do_sample, float(temperature),
                             int(top_k), float(top_p), eos_token_id, int(pad_token_id), generator, use_graph, cache,
                             kv_cache_format)
    finally:
        model.train(was_training)


def _generate(model, input_ids, attention_mask, max_new, do_sample, temperature, top_k, top_p, eos, pad, generator,
              use_graph, cache, kv_cache_format=None):
    cfg = model.cfg
    dev = input_ids.device
    B, L = input_ids.shape
    vocab = int(model.loss_vocab_size or cfg.padded_vocab_size)
    if attention_mask is None:
        plen = torch.full((B,), L, dtype=torch.int64, device=dev)
    else:
        plen = attention_mask.to(dev).long().sum(dim=1)
    if cache is None:
        cache = KVCache(cfg, B, L + max_new, cfg.params_dtype, dev, format=kv_cache_format)

    seq = torch.full((B, L + max_new), pad, dtype=input_ids.dtype, device=dev)
    keep = torch.arange(L, device=dev)[None, :] < plen[:, None]
    seq[:, :L] = torch.where(keep, input_ids, seq[:, :L])
    finished = torch.zeros(B, dtype=torch.bool, device=dev)

    def emit(logits, t):
        tok = _pick(logits[:, :vocab], do_sample, temperature, top_k, top_p, generator)
        tok = torch.where(finished, torch.full_like(tok, pad), tok)
        seq.scatter_(1, (plen + t).unsqueeze(1), tok.unsqueeze(1).to(seq.dtype))
        if eos is not None:
            finished.logical_or_(tok == eos)
        return tok

    logits = model.forward_prefill(input_ids, plen, cache)
    cache.lens.copy_(plen)
    tok = emit(logits, 0)

    def step(tokens):
        cache.advance()
        return model.forward_decode(tokens, cache)

    captured = None
    if use_graph and dev.type == "cuda":
        # the first decode step runs eagerly (GEMM algorithm selection), the second is captured
        from ..train.graphs import CapturedStep
        step = captured = CapturedStep(step, warmup=1)
    for t in range(1, max_new):
        if eos is not None and t % EOS_POLL_STEPS == 0 and bool(finished.all()):
            break
        tok = emit(step(tok), t)
    if captured is not None and captured.note.startswith("capture failed"):
        raise RuntimeError(f"generate(use_graph=True): the decode step could not be captured ({captured.note})")
    return seq


# ------------------------------------------------------------------------------------------------
# Greedy speculative decoding


def _refuse_speculative(model, draft, input_ids, attention_mask, max_new_tokens, cache, kv_cache_format, do_sample,
                        k):
    """Every refusal of ``generate(draft_model=...)``, naming the cause, before anything is allocated."""
    if do_sample:
        raise NotImplementedError("generate(draft_model=...): verification is greedy; do_sample=True is not supported "
                                  "with a draft model")
    if kv_cache_format is not None or (cache is not None and cache.format is not None):
        raise NotImplementedError("generate(draft_model=...): kv_cache_format is not supported with a draft model "
                                  "(the multi-token verify step reads a 16-bit cache)")
    max_t = SF.DECODE_MULTI_MAX_T
    if isinstance(k, bool) or int(k) != k or not 1 <= k <= max_t - 1:
        raise ValueError(f"generate(draft_model=...): num_draft_tokens must be in 1 .. {max_t - 1} (the verify step "
                         f"takes up to {max_t} tokens), got {k!r}")
    _refuse(model, input_ids, attention_mask, max_new_tokens, None, None)
    try:
        _refuse(draft, input_ids, attention_mask, max_new_tokens, None, None)
    except (ValueError, NotImplementedError, RuntimeError) as e:
        raise type(e)(f"generate(draft_model=...): the draft model is refused: {e}") from e
    vt = int(model.loss_vocab_size or model.cfg.padded_vocab_size)
    vd = int(draft.loss_vocab_size or draft.cfg.padded_vocab_size)
    if vt != vd:
        raise ValueError(f"generate(draft_model=...): the draft model's vocabulary ({vd}) differs from the target's "
                         f"({vt})")
    B, L = input_ids.shape
    total = L + max_new_tokens + k
    for who, m in (("the target", model), ("the draft model", draft)):
        if total > m.cfg.max_position_embeddings:
            raise ValueError(f"generate(draft_model=...): prompt length {L} + max_new_tokens {max_new_tokens} + "
                             f"num_draft_tokens {k} = {total} exceeds max_position_embeddings "
                             f"{m.cfg.max_position_embeddings} of {who} (rejected drafts touch those positions)")
    if cache is not None and (cache.batch != B or total > cache.capacity):
        raise ValueError(f"generate(draft_model=...): prompt length {L} + max_new_tokens {max_new_tokens} + "
                         f"num_draft_tokens {k} = {total} for batch {B} exceeds the KV cache (batch {cache.batch}, "
                         f"capacity {cache.capacity})")


def speculative_accept(draft, target_argmax, remaining, finished, eos, pad):
    """The accept step of one round, per row, on the device (no host read).

    ``draft`` [B, k]: the proposed d1 .. dk; ``target_argmax`` [B, k + 1]: the target's greedy
    tokens p0 .. pk after x0, d1 .. dk; ``remaining`` [B]: tokens the row may still emit;
    ``finished`` [B] bool. n = the longest prefix with d_i == p_(i-1) (a cumulative product). The
    row emits d1 .. dn, p_n, which are p0 .. pn, cut at ``remaining`` and after the first ``eos``
    (None: no EOS); a finished row emits nothing.

    Returns (tokens [B, k + 1]: the emitted run, then ``pad``; count [B]: its length; finished [B]:
    the old flag or an emitted EOS; n [B]: the accepted drafts before any cut)."""
    k = draft.shape[1]
    match = (draft == target_argmax[:, :k]).long()
    n = match.cumprod(dim=1).sum(dim=1)                                         # [B], 0 .. k
    idx = torch.arange(k + 1, device=draft.device)[None, :]
    count = torch.minimum(n + 1, remaining.long().clamp(min=0))
    count = torch.where(finished, torch.zeros_like(count), count)
    done = finished
    if eos is not None:
        hit = (target_argmax == eos) & (idx < count[:, None])
        first = torch.where(hit, idx, torch.full_like(idx, k + 1)).amin(dim=1)  # k + 1: none
        count = torch.minimum(count, first + 1)
        done = finished | hit.any(dim=1)
    tokens = torch.where(idx < count[:, None], target_argmax, torch.full_like(target_argmax, pad))
    return tokens, count, done, n


class SpeculativeState:
    """What the rounds of one speculative ``generate`` call update in place (all on the device):
    ``seq`` [B, L + max_new + 1] (the last column takes the writes of tokens that are not emitted),
    ``plen`` / ``nout`` / ``remaining`` int64 [B], ``finished`` bool [B], ``counters`` int64 [3]
    (rounds, drafted, accepted) and the two caches."""

    def __init__(self, model, draft, input_ids, attention_mask, max_new, k, eos, pad, cache, dstate):
        cfg, dev = model.cfg, input_ids.device
        B, L = input_ids.shape
        self.model, self.draft, self.k, self.eos, self.pad, self.dstate = model, draft, k, eos, pad, dstate
        self.vocab = int(model.loss_vocab_size or cfg.padded_vocab_size)
        self.plen = (torch.full((B,), L, dtype=torch.int64, device=dev) if attention_mask is None
                     else attention_mask.to(dev).long().sum(dim=1))
        cap = L + max_new + k
        self.cache = cache if cache is not None else KVCache(cfg, B, cap, cfg.params_dtype, dev)
        # a self-draft still keeps a cache of its own: the draft steps run ahead of the target
        self.dcache = KVCache(draft.cfg, B, cap, draft.cfg.params_dtype, dev)
        self.seq = torch.full((B, L + max_new + 1), pad, dtype=input_ids.dtype, device=dev)
        keep = torch.arange(L, device=dev)[None, :] < self.plen[:, None]
        self.seq[:, :L] = torch.where(keep, input_ids, self.seq[:, :L])
        self.finished = torch.zeros(B, dtype=torch.bool, device=dev)
        self.counters = torch.zeros(3, dtype=torch.int64, device=dev)
        # prefill of both models; the target's logits give the first token x0
        with dw.decode_weights(dstate):
            logits = model.forward_prefill(input_ids, self.plen, self.cache)
        self.cache.lens.copy_(self.plen)
        draft.forward_prefill(input_ids, self.plen, self.dcache)
        self.dcache.lens.copy_(self.plen)
        x0 = logits[:, :self.vocab].argmax(dim=-1)
        self.seq.scatter_(1, self.plen.unsqueeze(1), x0.unsqueeze(1).to(self.seq.dtype))
        if eos is not None:
            self.finished.logical_or_(x0 == eos)
        self.nout = torch.ones(B, dtype=torch.int64, device=dev)
        self.remaining = torch.full((B,), max_new - 1, dtype=torch.int64, device=dev)
        self.x0 = x0

    def round(self, x0):
        """One round from the last emitted token ``x0`` [B] (in neither cache yet): k + 1 draft
        steps, one verify step, the accept step and every state update. Returns the new x0. Nothing
        here reads the device."""
        k, V = self.k, self.vocab
        cache, dcache = self.cache, self.dcache
        base = cache.lens.clone()
        tok, drafts = x0, []
        for i in range(k + 1):          # the last step only fills the draft's cache
            dcache.advance()
            lg = self.draft.forward_decode(tok, dcache)
            if i < k:
                tok = lg[:, :V].argmax(dim=-1)
                drafts.append(tok)
        d = torch.stack(drafts, dim=1)                                           # [B, k]
        cache.advance(k + 1)
        with dw.decode_weights(self.dstate):
            logits = self.model.forward_extend(torch.cat([x0.unsqueeze(1), d], dim=1), cache)
        p = logits[..., :V].argmax(dim=-1)                                       # [B, k + 1]
        active = ~self.finished & (self.remaining > 0)
        toks, count, done, n = speculative_accept(d, p, self.remaining, self.finished, self.eos, self.pad)
        idx = torch.arange(k + 1, device=x0.device)[None, :]
        col = torch.where(idx < count[:, None], (self.plen + self.nout)[:, None] + idx,
                          torch.full_like(idx, self.seq.shape[1] - 1))
        self.seq.scatter_(1, col, toks.to(self.seq.dtype))
        last = toks.gather(1, (count - 1).clamp(min=0).unsqueeze(1)).squeeze(1)
        x0 = torch.where(count > 0, last, x0)
        self.nout.add_(count)
        self.remaining.sub_(count)
        self.finished.copy_(done)
        new_lens = (base.long() + count).to(torch.int32)
        cache.lens.copy_(new_lens)
        dcache.lens.copy_(new_lens)
        self.counters.add_(torch.stack([torch.ones_like(n[0]), (active.long() * k).sum(), (active.long() * n).sum()]))
        return x0

    def all_done(self):
        """The one flag the host may read per round."""
        return bool((self.finished | (self.remaining <= 0)).all())


def _generate_speculative(model, draft, input_ids, attention_mask, max_new, k, eos, pad, use_graph, cache, dstate,
                          stats):
    st = SpeculativeState(model, draft, input_ids, attention_mask, max_new, k, eos, pad, cache, dstate)
    step, captured = st.round, None
    if use_graph and input_ids.device.type == "cuda":
        from ..train.graphs import CapturedStep
        step = captured = CapturedStep(st.round, warmup=1)     # round 1 eager, round 2 captured
    x0 = st.x0
    # a round emits at least one token per unfinished row and at most k + 1
    for r in range(max_new - 1):
        if (eos is not None or r * (k + 1) >= max_new - 1) and st.all_done():
            break
        x0 = step(x0)
    if captured is not None and captured.note.startswith("capture failed"):
        raise RuntimeError(f"generate(use_graph=True): the speculative round could not be captured ({captured.note})")
    if stats is not None:
        rounds, drafted, accepted = (int(v) for v in st.counters.tolist())
        stats.update(rounds=rounds, drafted=drafted, accepted=accepted)
    return st.seq[:, :-1].contiguous()
