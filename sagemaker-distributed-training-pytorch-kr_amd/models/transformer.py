"""Megatron-compatible parallel transformer (GPT / LLaMA families) on the gfx950 kernel library.

Covers the model side of the reference's Megatron recipe (`core_transformer_config_
from_args`, /root/reference/3_training_megatron-lm/megatron/arguments.py:419-446, GPTModel at
`pretrain_gpt.py:46-58`): pre-LN blocks, learned-absolute or RoPE positions, GeLU / SwiGLU /
squared-ReLU MLPs, MHA or GQA, hidden/attention dropout, TP + SP + activation recompute.

Activation layout is [s, b, h] (sequence-first, as Megatron) so sequence-parallel shards are
contiguous chunks and the TP collectives move contiguous buffers.

The residual stream is "deferred": a layer returns (branch_output, branch_bias) plus the
residual, and the NEXT layer's first LayerNorm consumes them through ONE fused kernel
(bias + dropout + residual-add + LayerNorm, K4+K6), so the residual stream is written once and
read once per sub-block. Layer 0 folds the embedding dropout into the same kernel.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, field
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops import _ext
from ..ops import functional as SF
from ..parallel import state as ps
from ..parallel import decode_weights as dw
from ..parallel import fp8_linear
from ..parallel import moe_experts
from ..parallel import tensor_parallel as tp
from ..parallel.random import checkpoint as rng_checkpoint, get_rng


@dataclass
class TransformerConfig:
    num_layers: int = 24
    hidden_size: int = 1024
    num_attention_heads: int = 16
    num_query_groups: Optional[int] = None       # GQA (None -> MHA)
    ffn_hidden_size: Optional[int] = None        # default 4h (GeLU) / 8h/3 rounded (SwiGLU)
    kv_channels: Optional[int] = None
    # uneven pipeline split (Megatron-core --decoder-first/last-pipeline-num-layers): the last
    # stage also runs the LM head + CE, so giving it fewer layers balances the pipeline
    decoder_first_pipeline_num_layers: Optional[int] = None
    decoder_last_pipeline_num_layers: Optional[int] = None
    hidden_dropout: float = 0.1
    attention_dropout: float = 0.1
    layernorm_epsilon: float = 1e-5
    layernorm_zero_centered_gamma: bool = False  # --apply-layernorm-1p: gamma stored as (gamma - 1)
    apply_residual_connection_post_layernorm: bool = False   # residual taken after the norm
    normalization: str = "LayerNorm"            # or "RMSNorm"
    activation: str = "gelu"                     # gelu | swiglu | squared_relu | gelu_erf
    num_experts: Optional[int] = None            # --num-experts: Switch MLP (top-1 routed experts)
    moe_grouped_gemm: bool = False               # --moe-grouped-gemm: device routing + grouped expert GEMMs
    add_bias_linear: bool = True
    position_embedding_type: str = "learned_absolute"   # or "rope"
    rotary_percent: float = 1.0
    rotary_base: float = 10000.0
    max_position_embeddings: int = 1024
    position_offset: int = 0                     # OPT's learned positions start at row 2
    padded_vocab_size: int = 50304
    untie_embeddings_and_output_weights: bool = False
    init_method_std: float = 0.02
    init_method: str = "normal"                  # or "xavier_uniform" (--init-method-xavier-uniform)
    perform_initialization: bool = True         # False: --no-initialization (weights left unset)
    use_cpu_initialization: bool = False        # --use-cpu-initialization: draw on the host
    params_dtype: torch.dtype = torch.bfloat16
    seed: int = 1234
    # parallelism
    sequence_parallel: bool = False
    async_tensor_model_parallel_allreduce: bool = True
    # fusions (Megatron --no-*-fusion flags turn these off)
    masked_softmax_fusion: bool = True
    bias_gelu_fusion: bool = True
    bias_dropout_fusion: bool = True
    use_flash_attn: bool = True
    apply_query_key_layer_scaling: bool = False
    # recompute (P9)
    recompute_granularity: Optional[str] = None  # "full" | "selective"
    recompute_method: Optional[str] = None       # "uniform" | "block"
    recompute_num_layers: Optional[int] = None
    distribute_saved_activations: bool = False   # full recompute: saved layer inputs split across TP
    # FP8 linears with delayed scaling (--fp8-e4m3 / --fp8-hybrid): QKV, proj, fc1, fc2 of every
    # layer run their forward and input-gradient GEMMs on FP8 operands (fp8_linear.FP8State)
    fp8: Optional[str] = None                    # None | "e4m3" | "hybrid" (dY in E5M2)
    fp8_wgrad: bool = False                      # --fp8-wgrad: the weight-gradient GEMM on FP8 operands too
    fp8_margin: int = 0
    fp8_interval: int = 1
    fp8_amax_history_len: int = 1
    fp8_amax_compute_algo: str = "most_recent"   # or "max"
    # --fp8-recipe: "delayed" (per-tensor delayed scaling, above) | "mxfp8" (OCP MX block scaling
    # on the scaled MFMA, tp.MXFP8Linear: no state, no table in the state dict)
    fp8_recipe: str = "delayed"

    def __post_init__(self):
        if self.fp8_recipe not in ("delayed", "mxfp8"):
            raise ValueError(f"fp8_recipe must be 'delayed' or 'mxfp8', got {self.fp8_recipe!r}")
        if self.fp8_recipe == "mxfp8" and not self.fp8:
            raise ValueError("fp8_recipe 'mxfp8' needs fp8 linears (fp8 = 'e4m3' or 'hybrid')")
        if self.fp8_recipe == "mxfp8" and self.fp8_wgrad:
            raise ValueError("fp8_recipe 'mxfp8' keeps the weight gradient in 16 bits: fp8_wgrad is not supported")
        if self.fp8 not in (None, "e4m3", "hybrid"):
            raise ValueError(f"fp8 must be None, 'e4m3' or 'hybrid', got {self.fp8!r}")
        if self.fp8_wgrad and not self.fp8:
            raise ValueError("fp8_wgrad needs fp8 linears (fp8 = 'e4m3' or 'hybrid')")
        if self.fp8 and self.params_dtype not in (torch.bfloat16, torch.float16):
            raise ValueError("fp8 linears need bf16 or fp16 parameters")
        if self.fp8 and self.num_experts:
            raise ValueError("fp8 linears with num_experts are not supported (per-expert row counts are not "
                             "multiples of 16)")
        if self.moe_grouped_gemm and not self.num_experts:
            raise ValueError("moe_grouped_gemm needs num_experts")
        if self.num_query_groups is None:
            self.num_query_groups = self.num_attention_heads
        if self.kv_channels is None:
            self.kv_channels = self.hidden_size // self.num_attention_heads
        if self.ffn_hidden_size is None:
            if self.activation == "swiglu":
                f = int(8 * self.hidden_size / 3)
                self.ffn_hidden_size = 256 * ((f + 255) // 256)
            else:
                self.ffn_hidden_size = 4 * self.hidden_size

    @property
    def rms(self) -> bool:
        return self.normalization.lower() == "rmsnorm"


def _gather_wait(mod, x):
    """Run ``mod``'s overlapped-ZeRO parameter all-gather wait (a forward pre-hook installed by
    parallel/distributed.py) for a module whose weights are read without calling ``mod(x)``
    (Norm.fused, the fused MLP paths). Without it the kernel could read weights whose async
    all-gather is still in flight. The wait is idempotent."""
    for hook in tuple(mod._forward_pre_hooks.values()):
        if getattr(hook, "_smdt_gather_wait", False):
            hook(mod, (x,))


class Norm(nn.Module):
    """LayerNorm / RMSNorm parameters; the math runs in the fused BDA+norm kernel."""

    def __init__(self, h, cfg: TransformerConfig, device=None):
        super().__init__()
        self.rms = cfg.rms
        self.eps = cfg.layernorm_epsilon
        # Sequence-parallel activations are sharded across TP: draw their dropout masks from the
        # per-TP-rank stream; replicated activations use the TP-identical default stream.
        self.rng_kind = "tp" if cfg.sequence_parallel and ps.get_state().tp > 1 else "default"
        # --apply-layernorm-1p: the stored gamma is centred on zero (so weight decay pulls the
        # scale toward 1) and the kernel reads 1 + weight
        self.one_p = bool(cfg.layernorm_zero_centered_gamma)
        init = torch.zeros if self.one_p else torch.ones
        self.weight = nn.Parameter(init(h, dtype=cfg.params_dtype, device=device))
        self.weight.sequence_parallel = cfg.sequence_parallel
        if not self.rms:
            self.bias = nn.Parameter(torch.zeros(h, dtype=cfg.params_dtype, device=device))
            self.bias.sequence_parallel = cfg.sequence_parallel
        else:
            self.register_parameter("bias", None)

    def fused(self, x, xbias, residual, p, training, gather=None):
        # called instead of forward() by the layers: wait for this module's overlapped ZeRO
        # parameter all-gather (see _gather_wait) before the kernel reads the weights
        _gather_wait(self, x)
        w = self.weight + 1 if self.one_p else self.weight
        return SF.bias_dropout_add_norm(x, xbias, residual, w, self.bias, p, training, self.eps, self.rms,
                                        rng=get_rng(self.rng_kind), gather=gather)

    def forward(self, x):
        return self.fused(x, None, None, 0.0, False)[0]


# ---------------------------------------------------------------------------------------------
# Padding-free ("unpadded") micro-batches. An SFT micro-batch is right-padded to its longest
# example; with causal attention a real token never sees a pad, so the pads only cost compute.
# Under ``packed_sequences`` every token-wise op (embeddings, GEMMs, norms, MLP, LM head + CE)
# runs on the T real tokens only ([T, 1, h]); attention alone scatters its fused QKV into the
# padded [L, b] layout (zeros in the pad rows), runs RoPE + the causal flash kernels there and
# gathers the T context rows back. Real-token outputs and all gradients equal the padded
# computation's (models/hf.py ``HFCausalLM.forward`` sets it up from the attention mask).
_PACK = {"idx": None, "b": 0, "L": 0, "inv": None, "groups": None}


class packed_sequences:
    """Context: ``idx`` (device int64 [T]) = seq-first flat positions s * b + bi of the real
    tokens of a right-padded [b, L] batch. ``groups`` (optional, ``length_groups``): the rows
    bucketed by their own length, for the length-grouped attention layout."""

    def __init__(self, idx, b: int, L: int, groups=None):
        self.state = {"idx": idx, "b": int(b), "L": int(L), "inv": None, "groups": groups}

    def __enter__(self):
        self.prev = dict(_PACK)
        _PACK.update(self.state)
        return self

    def __exit__(self, *exc):
        _PACK.update(self.prev)
        return False


_PACK_GATHER = os.environ.get("SMDT_PACK_GATHER", "1") == "1"     # A/B: 0 = torch index ops


def _inv_map():
    """[L * b] int64: the packed row of each padded position, -1 for pads (cached per context)."""
    inv = _PACK.get("inv")
    if inv is None:
        idx, b, L = _PACK["idx"], _PACK["b"], _PACK["L"]
        inv = torch.full((L * b,), -1, dtype=torch.int64, device=idx.device)
        inv[idx] = torch.arange(idx.numel(), device=idx.device)
        _PACK["inv"] = inv
    return inv


class _GatherRows(torch.autograd.Function):
    """out[r] = x[fwd_map[r]] (0 where fwd_map[r] < 0); the gradient is the gather with
    ``bwd_map``, the inverse row map (ops: gather_rows in transpose.hip — every output row
    written once: no zero fill of the padded buffer, no index_copy / index_add scatter)."""

    @staticmethod
    def forward(ctx, x, fwd_map, bwd_map):
        ctx.bwd_map = bwd_map
        ctx.nin = x.shape[0]
        return _ext.ext().gather_rows(x.contiguous(), fwd_map)

    @staticmethod
    def backward(ctx, g):
        return _ext.ext().gather_rows(g.contiguous(), ctx.bwd_map), None, None


# Length-grouped attention layout (SMDT_SFT_LENGTH_GROUPS, default on). The padded [L, b] layout
# pays attention (and the row gathers) for every row at the window's longest length L: an NB4
# window of 32 Alpaca rows (~135 tokens each, the longest a few hundred) spends most of its causal
# attention on pad rows. Rows are instead bucketed by their own length rounded up to 128 (the
# flash kernels' S granularity) into blocks [L_g, b_g], laid out one after another in ONE
# [sum_g L_g b_g, W] buffer: ONE row gather in, the causal flash kernels per block on views of
# it (no copies either way), ONE gather out. Real-token results equal the [L, b] layout's: a real
# token still sees exactly its own row's earlier tokens.
_LENGTH_GROUPS = os.environ.get("SMDT_SFT_LENGTH_GROUPS", "1") in ("1", "force")   # force: skip the cost gate
_LENGTH_GROUPS_FORCE = os.environ.get("SMDT_SFT_LENGTH_GROUPS", "1") == "force"
_GROUP_ALIGN = 128


# When the grouping pays: the attention work it saves is ~7 x (b L^2 saved) x hidden FLOPs per
# layer (forward + backward, at ~150 TFLOP/s for the padded causal kernels at these lengths);
# each extra block costs per layer its own launches and host work, calibrated at 250 us from the
# two NB4 models: OPT-125m (hidden 768) ran 11 % slower grouped, LLaMA-7B (4096) 6-7 % faster
# (profiles/r5_sft_groups/).
_GROUP_LAUNCH_S = 250e-6
_GROUP_FLOPS = 1.5e14


def length_groups(mask_cpu, idx_cpu, device, hidden: int = None):
    """Host-side (CPU, no device sync) plan of the length-grouped layout for a right-padded
    [b, L] CPU ``mask_cpu`` whose packed tokens are the seq-first positions ``idx_cpu``:
    ``{"blocks": [(row offset, L_g, b_g)], "inv": [P] packed index of each grouped position
    (-1 = pad), "pack": [T] grouped position of each packed token (-1: a trailing pad token
    beyond its row's block, whose attention output is then 0)}``, the maps on ``device``. None
    when, for a model of this ``hidden`` size, the attention work saved would not pay for the
    extra launches."""
    b, L = mask_cpu.shape
    lens = mask_cpu.sum(1).clamp(min=1)
    Lr = ((lens + _GROUP_ALIGN - 1) // _GROUP_ALIGN) * _GROUP_ALIGN          # per-row block length
    blocks, off = [], 0
    row_off = torch.empty(b, dtype=torch.int64)      # block offset of each row's block
    row_j = torch.empty(b, dtype=torch.int64)        # the row's index inside its block
    row_b = torch.empty(b, dtype=torch.int64)        # rows in the row's block
    row_L = torch.empty(b, dtype=torch.int64)
    for Lg in sorted(set(Lr.tolist())):
        rows = (Lr == Lg).nonzero().squeeze(1)
        bg = rows.numel()
        blocks.append((off, int(Lg), int(bg)))
        row_off[rows] = off
        row_j[rows] = torch.arange(bg)
        row_b[rows] = bg
        row_L[rows] = Lg
        off += int(Lg) * bg
    if hidden is not None:
        saved = b * L * L - sum(bg * Lg * Lg for _, Lg, bg in blocks)
        if 7.0 * saved * hidden / _GROUP_FLOPS < (len(blocks) - 1) * _GROUP_LAUNCH_S:
            return None
    s_t, i_t = idx_cpu // b, idx_cpu % b
    ok = s_t < row_L[i_t]
    pos = row_off[i_t] + s_t * row_b[i_t] + row_j[i_t]
    pack = torch.where(ok, pos, torch.full_like(pos, -1))
    inv = torch.full((off,), -1, dtype=torch.int64)
    inv[pos[ok]] = torch.arange(idx_cpu.numel())[ok]
    return {"blocks": blocks, "inv": inv.to(device, non_blocking=True),
            "pack": pack.to(device, non_blocking=True), "rows": off}


class _RopeQKVGroups(torch.autograd.Function):
    """RoPE (in place) on the q / k parts of the length-grouped [P, W] buffer: one launch per
    block, positions (row // b_g) within the block."""

    @staticmethod
    def forward(ctx, x, cos, sin, rot, nh, nkv, hd, blocks):
        ctx.mark_dirty(x)
        for o, Lg, bg in blocks:
            _ext.ext().rope_(x[o:o + Lg * bg, :(nh + nkv) * hd].view(Lg * bg, nh + nkv, hd), cos, sin, rot,
                             bg, Lg, False)
        ctx.save_for_backward(cos, sin)
        ctx.cfg = (rot, nh, nkv, hd, blocks)
        return x

    @staticmethod
    def backward(ctx, g):
        cos, sin = ctx.saved_tensors
        rot, nh, nkv, hd, blocks = ctx.cfg
        d = g if g.is_contiguous() else g.contiguous()
        for o, Lg, bg in blocks:
            _ext.ext().rope_(d[o:o + Lg * bg, :(nh + nkv) * hd].view(Lg * bg, nh + nkv, hd), cos, sin, rot,
                             bg, Lg, True)
        return d, None, None, None, None, None, None, None


class _FlashQKVGroups(torch.autograd.Function):
    """Causal flash attention of every block [L_g, b_g] of the length-grouped [P, W] fused-QKV
    buffer, reading q / k / v as strided views of it and writing the context [P, nh hd] and, in
    backward, d(qkv) [P, W] block by block in place (the kernels take strided views)."""

    @staticmethod
    def forward(ctx, qkv, nh, nkv, hd, scale, dropout_p, seeds, blocks):
        C = _ext.ext()
        P, W = qkv.shape
        out = qkv.new_empty(P, nh, hd)
        lses = []
        for (o, Lg, bg), (seed, off) in zip(blocks, seeds):
            q, k, v = SF._qkv_views(qkv[o:o + Lg * bg].view(Lg, bg, W), nh, nkv, hd, True)
            ov = out[o:o + Lg * bg].view(Lg, bg, nh, hd).transpose(0, 1)
            lses.append(C.flash_fwd(q, k, v, scale, True, ov, dropout_p, seed, off)[1])
        ctx.save_for_backward(qkv, out, *lses)
        ctx.cfg = (nh, nkv, hd, scale, dropout_p, seeds, blocks)
        return out.view(P, nh * hd)

    @staticmethod
    def backward(ctx, dout):
        qkv, out, *lses = ctx.saved_tensors
        nh, nkv, hd, scale, dropout_p, seeds, blocks = ctx.cfg
        C = _ext.ext()
        P, W = qkv.shape
        dqkv = torch.empty_like(qkv)
        do_all = dout.contiguous().view(P, nh, hd)
        for (o, Lg, bg), (seed, off), lse in zip(blocks, seeds, lses):
            sl = slice(o, o + Lg * bg)
            q, k, v = SF._qkv_views(qkv[sl].view(Lg, bg, W), nh, nkv, hd, True)
            dq, dk, dv = SF._qkv_views(dqkv[sl].view(Lg, bg, W), nh, nkv, hd, True)
            o_v = out[sl].view(Lg, bg, nh, hd).transpose(0, 1)
            do_v = do_all[sl].view(Lg, bg, nh, hd).transpose(0, 1)
            C.flash_bwd(q, k, v, o_v, do_v, lse, scale, True, dq, dk, dv, dropout_p, seed, off)
        return dqkv, None, None, None, None, None, None, None


def _unpack_rows(x):
    """[T, 1, W] -> [L, b, W] with zero pad rows (differentiable)."""
    idx, b, L = _PACK["idx"], _PACK["b"], _PACK["L"]
    W = x.shape[-1]
    if _PACK_GATHER and _ext.use_kernels(x) and (W * x.element_size()) % 16 == 0:
        return _GatherRows.apply(x.reshape(-1, W), _inv_map(), idx).view(L, b, W)
    return x.new_zeros(L * b, W).index_copy(0, idx, x.reshape(-1, W)).view(L, b, W)


def _pack_rows(x):
    """[L, b, C] -> [T, 1, C] (the real-token rows)."""
    C = x.shape[-1]
    if _PACK_GATHER and _ext.use_kernels(x) and (C * x.element_size()) % 16 == 0:
        return _GatherRows.apply(x.reshape(-1, C), _PACK["idx"], _inv_map()).unsqueeze(1)
    return x.reshape(-1, C).index_select(0, _PACK["idx"]).unsqueeze(1)


# Text generation (models/generation.py). During the prefill of a ``KVCache`` every attention layer
# copies its post-RoPE K and V into the cache on its way through the unchanged causal forward.
_KV_PREFILL = {"cache": None}


class kv_prefill:
    """Context: attention layers store their K / V rows into ``cache`` (``KVCache.store_prefill``)."""

    def __init__(self, cache):
        self.cache = cache

    def __enter__(self):
        self.prev = _KV_PREFILL["cache"]
        _KV_PREFILL["cache"] = self.cache
        return self

    def __exit__(self, *exc):
        _KV_PREFILL["cache"] = self.prev
        return False


class ParallelAttention(nn.Module):
    def __init__(self, cfg: TransformerConfig, layer_number: int, device=None):
        super().__init__()
        st = ps.get_state()
        self.cfg = cfg
        self.layer_number = layer_number
        tpn = st.tp
        assert cfg.num_attention_heads % tpn == 0 and cfg.num_query_groups % tpn == 0
        self.nh = cfg.num_attention_heads // tpn
        self.nkv = cfg.num_query_groups // tpn
        self.hd = cfg.kv_channels
        q_out = cfg.num_attention_heads * self.hd
        kv_out = cfg.num_query_groups * self.hd
        std = cfg.init_method_std
        out_std = std / math.sqrt(2.0 * cfg.num_layers)
        self.qkv = tp.ColumnParallelLinear(cfg.hidden_size, q_out + 2 * kv_out, bias=cfg.add_bias_linear,
                                           init_std=std, key=f"layers.{layer_number}.qkv", seed=cfg.seed,
                                           params_dtype=cfg.params_dtype, device=device,
                                           sequence_parallel=cfg.sequence_parallel,
                                           chunks=[q_out, kv_out, kv_out],
                                           async_tensor_model_parallel_allreduce=cfg.async_tensor_model_parallel_allreduce)
        self.proj = tp.RowParallelLinear(q_out, cfg.hidden_size, bias=cfg.add_bias_linear, init_std=out_std,
                                         key=f"layers.{layer_number}.proj", seed=cfg.seed,
                                         params_dtype=cfg.params_dtype, device=device,
                                         sequence_parallel=cfg.sequence_parallel, skip_bias_add=True)
        self.rope = None

    def set_rope(self, cos, sin, rot):
        self.rope = (cos, sin, rot)

    def core_attention_unfused(self, qkv, training, doc_start=None):
        """Megatron's unfused path: baddbmm -> fused causal softmax (K1) -> dropout -> bmm. With
        ``doc_start`` ([b, s], per-document attention) the [b, 1, s, s] left-to-right mask is built
        from it and the fused masked softmax (K2) runs instead."""
        s, b = qkv.shape[0], qkv.shape[1]
        q, k, v = SF._qkv_views(qkv, self.nh, self.nkv, self.hd, True)  # [b, s, h, d]
        if self.nkv != self.nh:
            rep = self.nh // self.nkv
            k = k.repeat_interleave(rep, dim=2)
            v = v.repeat_interleave(rep, dim=2)
        qh = q.permute(0, 2, 1, 3).reshape(b * self.nh, s, self.hd)
        kh = k.permute(0, 2, 3, 1).reshape(b * self.nh, self.hd, s)
        vh = v.permute(0, 2, 1, 3).reshape(b * self.nh, s, self.hd)
        scores = torch.bmm(qh, kh).view(b, self.nh, s, s)
        if doc_start is None:
            probs = SF.scaled_masked_softmax(scores, None, 1.0 / math.sqrt(self.hd), causal=True)
        else:
            probs = SF.scaled_masked_softmax(scores, SF.document_mask(doc_start), 1.0 / math.sqrt(self.hd))
        if training and self.cfg.attention_dropout > 0:
            probs = F.dropout(probs, p=self.cfg.attention_dropout, training=True)
        ctx = torch.bmm(probs.view(b * self.nh, s, s), vh)          # [b*nh, s, d]
        return ctx.view(b, self.nh, s, self.hd).permute(2, 0, 1, 3).reshape(s, b, self.nh * self.hd)

    def core_attention_context_parallel(self, qkv, training):
        """Context parallelism: ``qkv`` holds this CP rank's contiguous
        sequence chunk; two all-to-alls re-shard it to the FULL sequence for nh/cp heads around the
        unchanged causal flash kernel (parallel/context_parallel.py) and back."""
        from ..parallel.context_parallel import ulysses_attention
        st = ps.get_state()
        q, k, v = SF._qkv_views(qkv, self.nh, self.nkv, self.hd, False)   # [s/cp, b, heads, d]
        p = self.cfg.attention_dropout if training else 0.0
        if not self.cfg.use_flash_attn:
            raise NotImplementedError("context parallelism runs attention through the flash kernels "
                                      "(--use-flash-attn)")
        ctx = ulysses_attention(q, k, v, group=st.cp_group, causal=True, scale=1.0 / math.sqrt(self.hd),
                                dropout_p=p, rng=get_rng("tp"))
        return ctx.reshape(ctx.shape[0], ctx.shape[1], self.nh * self.hd)

    def _qkv_bias_from_attention(self, x):
        """The QKV bias Parameter if the flash attention backward is to make its gradient
        (``tp.bias_from_producer``), else None. Strict: d(qkv) of the linear must BE what the
        backward kernels write, so only the in-place fused-QKV flash path with nothing between the
        linear and attention (no RoPE, no padding-free repacking, no context parallelism, a plain
        16-bit linear) and a shape the kernels take as it is."""
        lin = self.qkv
        if (_PACK["idx"] is not None or self.rope is not None or not self.cfg.use_flash_attn
                or ps.get_state().cp != 1 or lin._fp8 is not None or dw.decode_quantised() or lin.sequence_parallel
                or lin.gather_output
                or lin.skip_bias_add or not torch.is_grad_enabled() or x.dim() != 3
                or lin.bias is None or lin.weight.dtype != x.dtype or lin.bias.dtype != x.dtype):
            return None
        W = (self.nh + 2 * self.nkv) * self.hd
        if self.hd not in (64, 128) or x.shape[0] % 128 or W % 8 or self.nh % self.nkv or lin.out_local != W:
            return None
        return lin.bias if tp.bias_from_producer(lin.bias, x) else None

    def forward(self, x, training=True, doc_start=None):
        qkv_bias = self._qkv_bias_from_attention(x)
        if qkv_bias is not None:
            qkv = self.qkv(x, bias_grad=False)
            p = self.cfg.attention_dropout if training else 0.0
            return self.proj(SF.flash_attention_qkv(qkv, self.nh, self.nkv, self.hd, seq_first=True, causal=True,
                                                    dropout_p=p, rng=get_rng("tp"), doc_start=doc_start,
                                                    bias_p=qkv_bias))
        qkv = self.qkv(x)                                        # [s, b, (nh + 2 nkv) d]
        if _PACK["idx"] is not None:                              # padding-free micro-batch
            if doc_start is not None:
                raise NotImplementedError("per-document attention (doc_start / --reset-attention-mask) is not "
                                          "supported in the padding-free length-grouped SFT layout")
            if self._groups_ok(qkv):
                return self.proj(self._attend_groups(qkv, training))
            return self.proj(_pack_rows(self._attend(_unpack_rows(qkv), training)))
        return self.proj(self._attend(qkv, training, doc_start))  # (out, bias)

    def forward_decode(self, x, cache, layer: int):
        """One new token per sequence, x [1, b, h], against ``cache`` (models/generation.KVCache):
        QKV linear, RoPE at ``cache.pos`` and the append of K / V into that row of layer ``layer``'s
        cache (decode_attn.hip), single-query attention over the ``cache.lens`` keys, projection.
        ``cache.format`` picks the op pair: the 16-bit one, or the MXFP8 one. Returns what
        ``forward`` returns."""
        qkv = self.qkv(x)                                        # [1, b, (nh + 2 nkv) d]
        b = qkv.shape[1]
        k, v = cache.k[layer], cache.v[layer]
        if cache.format is not None:                             # MXFP8 cache (decode_attn_mx.hip)
            ks, vs = cache.k_scale[layer], cache.v_scale[layer]
            q = SF.decode_rope_append_mx(qkv.view(b, -1), k, ks, v, vs, cache.pos, self.nh, self.nkv, self.hd,
                                         rope=self.rope)
            ctx = SF.decode_attention_mx(q, k, ks, v, vs, cache.lens, 1.0 / math.sqrt(self.hd),
                                         max_len=cache.max_len)
            return self.proj(ctx.view(1, b, self.nh * self.hd))
        q = SF.decode_rope_append(qkv.view(b, -1), k, v, cache.pos, self.nh, self.nkv, self.hd, rope=self.rope)
        ctx = SF.decode_attention(q, k, v, cache.lens, 1.0 / math.sqrt(self.hd), max_len=cache.max_len)
        return self.proj(ctx.view(1, b, self.nh * self.hd))

    def forward_extend(self, x, cache, layer: int):
        """T new tokens per sequence, x [T, b, h], against a 16-bit ``cache`` whose ``pos`` / ``lens``
        were advanced by T (``KVCache.advance(T)``): QKV linear over the T b rows, RoPE at
        ``cache.pos + t`` and the append of the T K / V rows, attention of query t over keys
        0 .. lens - T + t (decode_attn_multi.hip), projection. The sequence-first projection output
        goes to the append kernel as a transposed view, without a copy. Returns what ``forward``
        returns, [T, b, h]."""
        if cache.format is not None:
            raise NotImplementedError(f"forward_extend: the multi-token decode step reads a 16-bit K/V cache; this "
                                      f"cache's format is {cache.format!r}")
        qkv = self.qkv(x)                                        # [T, b, (nh + 2 nkv) d]
        T, b = qkv.shape[0], qkv.shape[1]
        k, v = cache.k[layer], cache.v[layer]
        q = SF.decode_rope_append_multi(qkv.transpose(0, 1), k, v, cache.pos, self.nh, self.nkv, self.hd,
                                        rope=self.rope)         # [b, T, nh, d]
        ctx = SF.decode_attention_multi(q, k, v, cache.lens, 1.0 / math.sqrt(self.hd), max_len=cache.max_len)
        return self.proj(ctx.transpose(0, 1).reshape(T, b, self.nh * self.hd))

    def _groups_ok(self, qkv) -> bool:
        g = _PACK.get("groups")
        W = qkv.shape[-1]
        return (g is not None and self.cfg.use_flash_attn and ps.get_state().cp == 1 and _ext.use_kernels(qkv)
                and self.hd in (64, 128) and qkv.dtype in (torch.bfloat16, torch.float16)
                and (W * qkv.element_size()) % 16 == 0 and W % 8 == 0)

    def _attend_groups(self, qkv, training):
        """Padding-free attention in the length-grouped layout (``length_groups``): [T, 1, W]
        packed QKV -> grouped blocks (one row gather) -> RoPE -> causal flash per block -> [T, 1,
        nh hd] (one row gather)."""
        g = _PACK["groups"]
        W = qkv.shape[-1]
        x = _GatherRows.apply(qkv.reshape(-1, W), g["inv"], g["pack"])           # [P, W]
        if self.rope is not None:
            cos, sin, rot = self.rope
            x = _RopeQKVGroups.apply(x, cos, sin, rot, self.nh, self.nkv, self.hd, g["blocks"])
        p = self.cfg.attention_dropout if training else 0.0
        seeds = [SF._rng(get_rng("tp")).next() if p > 0 else (0, 0) for _ in g["blocks"]]
        ctx = _FlashQKVGroups.apply(x, self.nh, self.nkv, self.hd, 1.0 / math.sqrt(self.hd), float(p), seeds,
                                    g["blocks"])
        return _GatherRows.apply(ctx, g["pack"], g["inv"]).unsqueeze(1)         # [T, 1, nh hd]

    def _attend(self, qkv, training, doc_start=None):
        cp = ps.get_state().cp
        if cp > 1 and doc_start is not None:
            raise NotImplementedError("per-document attention (doc_start / --reset-attention-mask) is not "
                                      "supported with context parallelism (--context-parallel-size > 1)")
        if self.rope is not None:
            cos, sin, rot = self.rope
            if cp > 1:  # this rank's positions: chunk cp_rank of the full sequence
                off = ps.get_state().cp_rank * qkv.shape[0]
                cos, sin = cos[off: off + qkv.shape[0]], sin[off: off + qkv.shape[0]]
            qkv = _RopeQKV.apply(qkv, cos, sin, rot, self.nh, self.nkv, self.hd)
        if _KV_PREFILL["cache"] is not None:
            _KV_PREFILL["cache"].store_prefill(self, qkv)
        if cp > 1:
            return self.core_attention_context_parallel(qkv, training)
        if self.cfg.use_flash_attn:
            # attention dropout runs inside the flash kernels; heads are TP-sharded, so the mask
            # comes from the per-TP-rank stream (Megatron forks the model-parallel tracker here)
            p = self.cfg.attention_dropout if training else 0.0
            ctx = SF.flash_attention_qkv(qkv, self.nh, self.nkv, self.hd, seq_first=True, causal=True,
                                         dropout_p=p, rng=get_rng("tp"), doc_start=doc_start)
        elif training and self.cfg.recompute_granularity == "selective" and torch.is_grad_enabled():
            # Megatron's selective recompute: only the [b, np, s, s] scores / probabilities /
            # dropout of the unfused core attention are dropped and recomputed in backward (the
            # flash kernels never store them, so with flash there is nothing to recompute)
            ctx = rng_checkpoint(lambda t: self.core_attention_unfused(t, training, doc_start), qkv)
        else:
            ctx = self.core_attention_unfused(qkv, training, doc_start)
        return ctx


class _RopeQKV(torch.autograd.Function):
    """RoPE on the q and k parts of a fused [s, b, W] QKV buffer (kernel: rope.hip), in place:
    the buffer is the QKV GEMM's own output (or the padding-free scatter's), which nothing else
    keeps, and its gradient comes straight from the attention backward — so neither direction
    pays a [tokens, W] copy (LLaMA-7B: 2 x 32 copies of 100-300 MB per step)."""

    @staticmethod
    def forward(ctx, qkv, cos, sin, rot, nh, nkv, hd):
        s, b, W = qkv.shape
        # a view (e.g. the [s, b, W] reshape of a TP linear's output under CP) cannot be marked
        # dirty inside a custom Function, so it takes the copy
        if qkv.is_contiguous() and qkv._base is None:
            out = qkv
            ctx.mark_dirty(qkv)
        else:
            out = qkv.contiguous()
        _apply_rope_parts(out.view(s * b, W), cos, sin, rot, nh, nkv, hd, b, s, False)
        ctx.save_for_backward(cos, sin)
        ctx.cfg = (rot, nh, nkv, hd, b, s)
        return out

    @staticmethod
    def backward(ctx, g):
        cos, sin = ctx.saved_tensors
        rot, nh, nkv, hd, b, s = ctx.cfg
        d = g if g.is_contiguous() else g.contiguous()
        _apply_rope_parts(d.view(s * b, -1), cos, sin, rot, nh, nkv, hd, b, s, True)
        return d, None, None, None, None, None, None


def _apply_rope_parts(flat, cos, sin, rot, nh, nkv, hd, b, s, inverse):
    q = flat[:, : nh * hd].view(s * b, nh, hd)
    k = flat[:, nh * hd:(nh + nkv) * hd].view(s * b, nkv, hd)
    from ..ops import _ext
    if _ext.use_kernels(flat):
        # q and k heads are adjacent in every row of the fused buffer and rotate identically:
        # ONE launch over the [tokens, nh + nkv, hd] view (row stride W)
        _ext.ext().rope_(flat[:, :(nh + nkv) * hd].view(s * b, nh + nkv, hd), cos, sin, rot, b, s, inverse)
    else:
        pos = torch.arange(s * b, device=flat.device) // b
        q.copy_(SF._rope_ref(q, cos.to(flat.device), sin.to(flat.device), rot, pos, inverse))
        k.copy_(SF._rope_ref(k, cos.to(flat.device), sin.to(flat.device), rot, pos, inverse))


class ParallelMLP(nn.Module):
    def __init__(self, cfg: TransformerConfig, layer_number: int, device=None, key: Optional[str] = None):
        super().__init__()
        self.cfg = cfg
        key = key or f"layers.{layer_number}"
        f = cfg.ffn_hidden_size
        std = cfg.init_method_std
        out_std = std / math.sqrt(2.0 * cfg.num_layers)
        self.gated = cfg.activation == "swiglu"
        fc1_out = 2 * f if self.gated else f
        self.fc1 = tp.ColumnParallelLinear(cfg.hidden_size, fc1_out, bias=cfg.add_bias_linear, init_std=std,
                                           key=f"{key}.fc1", seed=cfg.seed,
                                           params_dtype=cfg.params_dtype, device=device,
                                           sequence_parallel=cfg.sequence_parallel, skip_bias_add=True,
                                           chunks=[f, f] if self.gated else None,
                                           async_tensor_model_parallel_allreduce=cfg.async_tensor_model_parallel_allreduce,
                                           bias_grad_from_output=True)   # forward() only ever uses h + b
        self.fc2 = tp.RowParallelLinear(f, cfg.hidden_size, bias=cfg.add_bias_linear, init_std=out_std,
                                        key=f"{key}.fc2", seed=cfg.seed,
                                        params_dtype=cfg.params_dtype, device=device,
                                        sequence_parallel=cfg.sequence_parallel, skip_bias_add=True)

    def forward(self, x):
        act = self.cfg.activation
        # FP8 linears take the unfused route: FP8 GEMM, then the bias-activation kernel
        # (nor under a quantised generation weight format: the fused forms would read the 16-bit weights)
        fused = act == "gelu" and self.cfg.bias_gelu_fusion and not self.cfg.fp8 and not dw.decode_quantised()
        if fused:
            # the fused forms read fc1 / fc2 weights without calling fc1(x) / fc2(x)
            _gather_wait(self.fc1, x)
            _gather_wait(self.fc2, x)
        if fused and tp.sp_fused_gelu_mlp_ok(x, self):
            # TP > 1 + sequence parallelism: the GeLU halves inside the ring-chunk GEMMs
            return tp.SPFusedGeLUMLP.apply(x, self.fc1.weight, self.fc1.bias, self.fc2.weight), self.fc2.bias
        if fused and tp.linear_bias_gelu_ok(x, self.fc1):
            if tp.fused_gelu_mlp_ok(x, self):
                # both GeLU halves inside the GEMMs: fc1 + bias + GeLU forward, fc2 dgrad + GeLU
                # backward (gemm_tn.hip epilogues)
                y = tp.FusedGeLUMLP.apply(x, self.fc1.weight, self.fc1.bias, self.fc2.weight)
                return y, self.fc2.bias
            # fc1 GEMM + bias + GeLU in one launch (gemm_tn.hip's bias-GeLU epilogue)
            return self.fc2(tp.linear_bias_gelu(x, self.fc1))
        h, b = self.fc1(x)
        if act in ("gelu", "gelu_erf"):
            if self.cfg.bias_gelu_fusion:
                h = SF.bias_gelu(h, b, "tanh" if act == "gelu" else "none")
            else:
                h = F.gelu(h + b if b is not None else h, approximate="tanh" if act == "gelu" else "none")
        elif act == "swiglu":
            if b is not None:
                h = h + b
            h = SF.swiglu(h)
        elif act == "squared_relu":
            h = F.relu(h + b if b is not None else h).pow(2)
        elif act == "relu":  # OPT
            h = F.relu(h + b if b is not None else h)
        else:
            raise ValueError(f"unknown activation {act}")
        return self.fc2(h)


class SwitchMLP(nn.Module):
    """``--num-experts E``: Megatron's Switch MLP (top-1 routing; the flag at
    /root/reference/3_training_megatron-lm/megatron/arguments.py:610-611, no expert-parallel group
    there either). A router (h -> E, softmax in fp32) picks one expert per token; each expert is a
    full ``ParallelMLP`` (tensor-parallel like the dense MLP); the token's output is the expert's
    (output + bias) scaled by the router probability. Tokens are sorted by expert once, so each
    expert runs ONE contiguous GEMM chain on its slice (no per-expert masks or scatters), and one
    gather puts the rows back. The per-expert token counts are read on the host (one sync per layer),
    so an MoE step is not graph-captured.

    ``--moe-grouped-gemm`` (opt-in, TP = 1, bf16 / fp16, gelu, biases on): the router runs on the
    device (csrc/kernels/moe_route.hip) into an expert-sorted, tile-padded row buffer, and the
    experts' GEMMs are grouped launches that pick their weight per 256-row tile from device tables
    (gemm_tn.hip GROUPED, wgrad_gemm.hip's ranged kernel): no host sync, launch shapes independent
    of the routing, so the step can be captured (train/graphs.CapturedStep). Same parameters and
    checkpoint layout. Where a condition fails the layer raises; it never falls back."""

    def __init__(self, cfg: TransformerConfig, layer_number: int, device=None):
        super().__init__()
        if cfg.sequence_parallel and ps.get_state().tp > 1:
            # each TP rank would route a different sequence shard, so the experts' TP collectives
            # would not line up across the group
            raise NotImplementedError("--num-experts with --sequence-parallel")
        self.cfg = cfg
        e = int(cfg.num_experts)
        self.router = nn.Parameter(tp.init_full_then_shard(
            (e, cfg.hidden_size), cfg.init_method_std, f"layers.{layer_number}.router", cfg.seed,
            cfg.params_dtype, device, None, 0, 1))
        self.router_bias = nn.Parameter(torch.zeros(e, dtype=cfg.params_dtype, device=device))
        self.experts = nn.ModuleList(ParallelMLP(cfg, layer_number, device, key=f"layers.{layer_number}.experts.{i}")
                                     for i in range(e))
        self._tabs = None      # --moe-grouped-gemm: the experts' pointer tables, built at first use

    def route(self, flat):
        """(top-1 probability [n] fp32, expert index [n]) of each token row."""
        prob = torch.softmax(F.linear(flat, self.router, self.router_bias).float(), dim=-1)
        return prob.max(dim=-1)

    def _grouped_check(self, flat):
        """--moe-grouped-gemm asked for: raise, naming the condition, where the grouped path cannot
        run (it never falls back to the per-expert loop). Returns whether the kernels run."""
        cfg = self.cfg
        why = None
        if ps.get_state().tp > 1:
            why = "tensor parallel size 1"
        elif cfg.activation != "gelu":
            why = f"the gelu activation (got {cfg.activation})"
        elif not cfg.add_bias_linear:
            why = "linear biases (--disable-bias-linear is set)"
        elif cfg.fp8:
            why = "16-bit experts (fp8 is set)"
        kern = _ext.use_kernels(flat)
        if why is None and kern:
            T, h, f, E = flat.shape[0], cfg.hidden_size, cfg.ffn_hidden_size, len(self.experts)
            R = SF.moe_rows(T, E)
            C = _ext.ext()
            probe = self.experts[0]
            if flat.dtype not in (torch.bfloat16, torch.float16) or probe.fc1.weight.dtype != flat.dtype:
                why = f"bf16 or fp16 activations and weights (got {flat.dtype} / {probe.fc1.weight.dtype})"
            elif not (C.gemm_tn_shape_supported(R, f, h) and C.gemm_tn_shape_supported(R, h, f)):
                why = (f"gemm_tn shapes: hidden {h} and ffn {f} multiples of 256 (rows {R})")
            elif torch.is_grad_enabled() and any(
                    getattr(p, "main_grad", None) is None or p.main_grad.dtype != torch.float32
                    or isinstance(getattr(type(p), "main_grad", None), property)
                    for ex in self.experts for p in (ex.fc1.weight, ex.fc1.bias, ex.fc2.weight, ex.fc2.bias)):
                why = "a plain fp32 main_grad on every expert weight and bias (a DDP wrapper with fp32 gradients)"
        if why is not None:
            raise RuntimeError(f"--moe-grouped-gemm needs {why}")
        return kern

    def _forward_grouped(self, x):
        """--moe-grouped-gemm: device routing + grouped expert GEMMs (``moe_experts.GroupedSwitchExperts``):
        no host sync and no launch shape that depends on the routing."""
        s, b, h = x.shape
        flat = x.reshape(s * b, h)
        kern = self._grouped_check(flat)
        logits = F.linear(flat, self.router, self.router_bias)
        route = SF.moe_route(logits)
        self.last_counts = route[6]      # tokens per expert of the last call (device, int32)
        # the router's gradient: autograd through the softmax, at the expert the tables picked
        top_p = torch.softmax(logits.float(), dim=-1).gather(1, route[1].long().unsqueeze(1)).squeeze(1)
        ex = self.experts
        w1, b1 = [e.fc1.weight for e in ex], [e.fc1.bias for e in ex]
        w2, b2 = [e.fc2.weight for e in ex], [e.fc2.bias for e in ex]
        tabs = None
        if kern:
            key = tuple(p.data_ptr() for p in w1 + b1 + w2 + b2)
            if self._tabs is None or self._tabs[0] != key:      # built once per layer
                self._tabs = (key, (SF.moe_pointer_tables(w1, b1), SF.moe_pointer_tables(w2, b2)))
            tabs = self._tabs[1]
        out = moe_experts.GroupedSwitchExperts.apply(flat, top_p, route, tabs, len(ex), *w1, *b1, *w2, *b2)
        return out.view(s, b, h), None

    def forward(self, x):
        if self.cfg.moe_grouped_gemm:
            return self._forward_grouped(x)
        s, b, h = x.shape
        flat = x.reshape(s * b, h)
        top_p, top_e = self.route(flat)
        order = torch.argsort(top_e, stable=True)
        counts = torch.bincount(top_e, minlength=len(self.experts)).tolist()
        xs = flat.index_select(0, order)
        outs, o = [], 0
        for i, n in enumerate(counts):
            if n == 0:
                continue          # an expert with no tokens gets no gradient this step
            y, yb = self.experts[i](xs[o:o + n].unsqueeze(1))
            y = y.squeeze(1)
            outs.append(y + yb if yb is not None else y)
            o += n
        inv = torch.empty_like(order)
        inv[order] = torch.arange(order.numel(), device=order.device)
        out = torch.cat(outs).index_select(0, inv) * top_p.unsqueeze(-1).to(x.dtype)
        return out.view(s, b, h), None


def _sp_gather(cfg):
    """(tp, tp_rank) when sequence-parallel norms should write into all-gather slots."""
    if not cfg.sequence_parallel or _PACK["idx"] is not None:
        return None
    return tp.sp_gather_spec()


class ParallelTransformerLayer(nn.Module):
    def __init__(self, cfg: TransformerConfig, layer_number: int, device=None):
        super().__init__()
        self.cfg = cfg
        self.layer_number = layer_number
        self.input_norm = Norm(cfg.hidden_size, cfg, device)
        self.attention = ParallelAttention(cfg, layer_number, device)
        self.post_attention_norm = Norm(cfg.hidden_size, cfg, device)
        self.mlp = SwitchMLP(cfg, layer_number, device) if cfg.num_experts else ParallelMLP(cfg, layer_number, device)
        self.post_ln_residual = bool(cfg.apply_residual_connection_post_layernorm)
        if self.post_ln_residual and cfg.sequence_parallel and ps.get_state().tp > 1:
            # the SP norms hand their output to the all-gather, not back as a local residual
            raise NotImplementedError("--apply-residual-connection-post-layernorm with --sequence-parallel")

    def forward(self, x, xbias, residual, doc_start=None):
        training = self.training
        p = self.cfg.hidden_dropout
        # sequence parallelism: each norm's output is all-gathered by the next column-parallel
        # linear and (after a layer) its input gradient by the row-parallel linear that produced
        # x — both are written straight into their slot of the gather buffer (no local copy)
        g = _sp_gather(self.cfg)
        ln1, residual = self.input_norm.fused(x, xbias, residual, p, training,
                                              gather=None if g is None else g + (True, residual is not None))
        if self.post_ln_residual:           # Megatron's --apply-residual-connection-post-layernorm
            residual = ln1
        a, ab = self.attention(ln1, training, doc_start)
        ln2, residual = self.post_attention_norm.fused(a, ab, residual, p, training,
                                                       gather=None if g is None else g + (True, True))
        if self.post_ln_residual:
            residual = ln2
        m, mb = self.mlp(ln2)
        return m, mb, residual

    def forward_decode(self, x, xbias, residual, cache, layer: int):
        """``forward`` for one new token per sequence against a K/V cache (no sequence parallelism):
        the same norms and MLP, attention through ``ParallelAttention.forward_decode``."""
        training = self.training
        p = self.cfg.hidden_dropout
        ln1, residual = self.input_norm.fused(x, xbias, residual, p, training)
        if self.post_ln_residual:
            residual = ln1
        a, ab = self.attention.forward_decode(ln1, cache, layer)
        ln2, residual = self.post_attention_norm.fused(a, ab, residual, p, training)
        if self.post_ln_residual:
            residual = ln2
        m, mb = self.mlp(ln2)
        return m, mb, residual

    def forward_extend(self, x, xbias, residual, cache, layer: int):
        """``forward_decode`` for T new tokens per sequence, x [T, b, h]
        (``ParallelAttention.forward_extend``)."""
        training = self.training
        p = self.cfg.hidden_dropout
        ln1, residual = self.input_norm.fused(x, xbias, residual, p, training)
        if self.post_ln_residual:
            residual = ln1
        a, ab = self.attention.forward_extend(ln1, cache, layer)
        ln2, residual = self.post_attention_norm.fused(a, ab, residual, p, training)
        if self.post_ln_residual:
            residual = ln2
        m, mb = self.mlp(ln2)
        return m, mb, residual

    def forward_phases(self, st):
        """``forward`` cut at its four sequence-parallel exchanges for the sub-batch interleave
        (``ParallelTransformer._forward_subbatch``): each phase ends right after it STARTS an
        exchange (the norms' all-gathers by ``tp.ag_start``; the row-parallel linears' reduce-
        scatters are left in flight by ``rs_ring`` under ``tp.begin_subbatch``) and the next phase
        of this half begins by completing it. ``st`` holds this half's (x, xbias, residual) and its
        rows of ``doc_start`` (or None)."""
        training = self.training
        p = self.cfg.hidden_dropout
        g = _sp_gather(self.cfg)
        group = ps.get_state().tp_group
        x, residual = tp.rs_finish(st["x"]), st["residual"]
        ln1, residual = self.input_norm.fused(x, st["xbias"], residual, p, training,
                                              gather=None if g is None else g + (True, residual is not None))
        tp.ag_start(ln1, group)
        yield
        a, ab = self.attention(ln1, training, st.get("doc_start"))
        yield
        ln2, residual = self.post_attention_norm.fused(tp.rs_finish(a), ab, residual, p, training,
                                                       gather=None if g is None else g + (True, True))
        tp.ag_start(ln2, group)
        yield
        m, mb = self.mlp(ln2)
        st.update(x=m, xbias=mb, residual=residual)
        yield


# Sub-batch interleave of the sequence-parallel TP-pair exchanges (tp.begin_subbatch). "2": the
# two batch halves of a micro-batch alternate phase by phase; "0" (default) off.
_SUBBATCH = int(os.environ.get("SMDT_SP_SUBBATCH", "0") or 0)


class ParallelTransformer(nn.Module):
    """A stack of layers [first, first + n) of the full model (pipeline stages own a slice)."""

    def __init__(self, cfg: TransformerConfig, first_layer: int, num_layers: int, post_norm: bool, device=None):
        super().__init__()
        self.cfg = cfg
        self.layers = nn.ModuleList([ParallelTransformerLayer(cfg, first_layer + i, device) for i in range(num_layers)])
        self.final_norm = Norm(cfg.hidden_size, cfg, device) if post_norm else None
        if cfg.fp8 and num_layers > 0:
            # QKV, projection, fc1 and fc2 of every layer; registered only with FP8 on, so the state
            # dict of a 16-bit model keeps its keys
            lins = [m for l in self.layers for m in (l.attention.qkv, l.attention.proj, l.mlp.fc1, l.mlp.fc2)]
            if cfg.fp8_recipe == "mxfp8":      # stateless: no module, no buffer, nothing in the state dict
                fp8_linear.attach_mxfp8(lins, fp8_linear.MXFP8Recipe(cfg.fp8))
                return
            self.fp8_state = fp8_linear.FP8State(len(lins), cfg.fp8, cfg.fp8_margin, cfg.fp8_interval,
                                                 cfg.fp8_amax_history_len, cfg.fp8_amax_compute_algo, device,
                                                 fp8_wgrad=cfg.fp8_wgrad)
            fp8_linear.attach_fp8(lins, self.fp8_state)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        if self.cfg.fp8 and self.cfg.fp8_recipe == "mxfp8":
            # a delayed-scaling checkpoint: its table has no meaning for block scaling
            table = [k for k in state_dict if k.startswith(prefix + "fp8_state.")]
            for k in table:
                del state_dict[k]
            if table and (not torch.distributed.is_initialized() or torch.distributed.get_rank() == 0):
                print(f"FP8: --fp8-recipe mxfp8 keeps no scaling state: dropped the checkpoint's delayed-scaling "
                      f"table ({prefix}fp8_state.*)", flush=True)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                                      error_msgs)

    def _run(self, i, x, xb, res, doc_start=None):
        layer = self.layers[i]
        cfg = self.cfg
        if self.training and cfg.recompute_granularity == "full":
            n = cfg.recompute_num_layers or len(self.layers)
            if cfg.recompute_method == "block" and i >= n:
                return layer(x, xb, res, doc_start)
            # doc_start (an integer tensor, no gradient) travels with the call: the closures bind
            # THIS call's value, so the recompute in backward sees it whatever ran in between
            if cfg.distribute_saved_activations and ps.get_state().tp > 1 and not cfg.sequence_parallel:
                from ..parallel.random import distributed_checkpoint
                if res is None:
                    return distributed_checkpoint(lambda a, b_: layer(a, b_, None, doc_start), x, xb)
                return distributed_checkpoint(lambda a, b_, r: layer(a, b_, r, doc_start), x, xb, res)
            if xb is None:
                return rng_checkpoint(lambda a, r: layer(a, None, r, doc_start), x, res)
            return rng_checkpoint(lambda a, b_, r: layer(a, b_, r, doc_start), x, xb, res)
        return layer(x, xb, res, doc_start)

    def _subbatch_ok(self, x) -> bool:
        cfg = self.cfg
        st = ps.get_state()
        return (_SUBBATCH == 2 and self.training and torch.is_grad_enabled() and cfg.sequence_parallel
                and st.cp == 1 and cfg.recompute_granularity != "full" and _PACK["idx"] is None
                and tp.subbatch_capable(st) and x.dim() == 3 and x.shape[1] % 2 == 0
                and len(self.layers) > 0)

    def _forward_subbatch(self, x, xbias, residual, doc_start=None):
        """The layer stack on the two batch halves of the micro-batch, phase by phase alternately
        (see ``ParallelTransformerLayer.forward_phases``): half b's GEMMs / attention run while half
        a's exchange is in flight and vice versa. The halves meet again (one concat each) before
        the final norm / the pipeline send. Same math as ``forward`` per half; with dropout, the
        masks are drawn in the interleaved order."""
        hb = x.shape[1] // 2
        if x.requires_grad:
            x = tp.WgradMergeScope.apply(x, False)
        halves = []
        for i in range(2):
            sl = slice(i * hb, (i + 1) * hb)
            halves.append({"x": x[:, sl].contiguous(), "xbias": xbias,
                           "residual": None if residual is None else residual[:, sl].contiguous(),
                           "doc_start": None if doc_start is None else doc_start[sl].contiguous()})
        tp.begin_subbatch()
        try:
            for layer in self.layers:
                gens = [layer.forward_phases(h) for h in halves]
                for _ in range(4):
                    for gen in gens:
                        next(gen)
            for h in halves:
                tp.rs_finish(h["x"])
        finally:
            tp.end_subbatch()
        x = torch.cat([h["x"] for h in halves], dim=1)
        if x.requires_grad:
            x = tp.WgradMergeScope.apply(x, True)
        xbias = halves[0]["xbias"]
        residual = torch.cat([h["residual"] for h in halves], dim=1)
        return x, xbias, residual

    def forward_decode(self, x, cache):
        """The whole stack (it must own the final norm) on one new token per sequence, x [1, b, h],
        against ``cache``: the normalised output [1, b, h]."""
        xbias = residual = None
        for i, layer in enumerate(self.layers):
            x, xbias, residual = layer.forward_decode(x, xbias, residual, cache, i)
        return self.final_norm.fused(x, xbias, residual, self.cfg.hidden_dropout, self.training)[0]

    def forward_extend(self, x, cache):
        """``forward_decode`` for T new tokens per sequence, x [T, b, h]: the normalised output
        [T, b, h]."""
        xbias = residual = None
        for i, layer in enumerate(self.layers):
            x, xbias, residual = layer.forward_extend(x, xbias, residual, cache, i)
        return self.final_norm.fused(x, xbias, residual, self.cfg.hidden_dropout, self.training)[0]

    def forward(self, x, xbias=None, residual=None, doc_start=None):
        """Returns (pending_x, pending_bias, residual) or, with ``final_norm``, the normalised
        output (the pending branch folded into the residual first). ``doc_start`` (int32 [b, s],
        ``ops.functional.document_starts``) restricts every layer's attention to each token's own
        document."""
        if self._subbatch_ok(x):
            x, xbias, residual = self._forward_subbatch(x, xbias, residual, doc_start)
        elif self.cfg.recompute_granularity != "full" and not tp.foreign_hooks(self):
            # every row-parallel output of the stack is consumed by the next fused norm (the
            # layers' own, or the final one): the ring reduce-scatters leave their combine to it.
            # Not with user hooks on the stack (they would read a tensor missing the peer's
            # partial); the ledger (tp.check_pending_adds) catches any other consumer.
            if x.requires_grad and torch.is_grad_enabled():
                x = tp.PendingAddCheck.apply(x)
            with tp.defer_rs_add():
                for i in range(len(self.layers)):
                    x, xbias, residual = self._run(i, x, xbias, residual, doc_start)
        else:
            for i in range(len(self.layers)):
                x, xbias, residual = self._run(i, x, xbias, residual, doc_start)
        if self.final_norm is not None:
            g = _sp_gather(self.cfg)          # y feeds the LM head's column-parallel all-gather
            y, _ = self.final_norm.fused(x, xbias, residual, self.cfg.hidden_dropout, self.training,
                                         gather=None if g is None else g + (True, residual is not None))
            tp.check_pending_adds("the end of the layer stack's forward")
            return y
        x = tp.materialize_add(x)      # leaves the stage: no pending summand
        tp.check_pending_adds("the end of the layer stack's forward")
        return x, xbias, residual
