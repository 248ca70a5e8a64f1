"""Autograd-aware fused ops backed by the gfx950 kernel library.

Every op has two paths:
  * GPU tensors -> the HIP kernels in ``smdt_amd/_C.so`` (no silent fallback: see ``_ext``);
  * CPU tensors -> a plain PyTorch reference with identical semantics (tests, gloo runs).

Reference-parity notes: these cover Megatron's fused kernels K1-K6, K12, K15,
K16 (`megatron/arguments.py:814-854` in /root/reference/3_training_megatron-lm) with the same
enable/disable flags wired up in ``smdt_amd.models.transformer``.
"""
from __future__ import annotations

import math
import os
from typing import Optional

import torch
import torch.nn.functional as F

from . import _ext

# --------------------------------------------------------------------------------------------
# Dropout RNG: stateless Philox (seed, offset) pairs. The forward call records its pair in the
# autograd context and the backward kernel regenerates the identical mask.


class PhiloxState:
    """Per-process (seed, offset) source for the fused dropout kernels.

    ``offset`` advances by one per kernel call, so successive calls draw independent streams.
    Tensor-parallel-aware seeding lives in ``smdt_amd.parallel.random``.
    """

    def __init__(self, seed: int = 1234):
        self.seed = int(seed)
        self.offset = 0

    def next(self):
        self.offset += 1
        return self.seed, self.offset

    def state_dict(self):
        return {"seed": self.seed, "offset": self.offset}

    def load_state_dict(self, d):
        self.seed, self.offset = int(d["seed"]), int(d["offset"])


_DEFAULT_RNG = PhiloxState()


def default_rng() -> PhiloxState:
    return _DEFAULT_RNG


def _rng(rng: Optional[PhiloxState]) -> PhiloxState:
    return rng if rng is not None else _DEFAULT_RNG


# --------------------------------------------------------------------------------------------
# Fused (bias + dropout + residual) -> LayerNorm / RMSNorm


def _ln_ref(s, gamma, beta, eps, rms):
    sf = s.float()
    if rms:
        y = sf * torch.rsqrt(sf.pow(2).mean(-1, keepdim=True) + eps) * gamma.float()
    else:
        y = F.layer_norm(sf, (s.shape[-1],), gamma.float(), None if beta is None else beta.float(), eps)
    return y.to(s.dtype)


def grad_accumulate_target(t):
    """The fp32 DDP ``main_grad`` of parameter ``t`` if a kernel may accumulate the parameter's
    gradient straight into it (then the kernel owner calls ``t._smdt_grad_ready``), else None."""
    if t is None or not isinstance(t, torch.nn.Parameter):
        return None
    mg = getattr(t, "main_grad", None)
    if (mg is None or mg.dtype != torch.float32 or not mg.is_cuda or not mg.is_contiguous()
            or getattr(t, "_smdt_grad_ready", None) is None):
        return None
    return mg


def _mark_ready(*params):
    for t in params:
        if t is not None:
            t._smdt_grad_ready(t)


def gather_slot(t, world: int, rank: int):
    """A [world * n, ...] buffer (uninitialised) and its rank-th row block, the slot ``t``'s
    producer writes into so that a sequence-parallel all-gather of it needs no local copy
    (``tensor_parallel.ag_ring`` takes the buffer, marked on the slot as ``_smdt_gather``)."""
    n = t.shape[0]
    buf = t.new_empty((world * n,) + tuple(t.shape[1:]))
    return buf, buf[rank * n:(rank + 1) * n]


def _mark_gather(t, buf, rank):
    t._smdt_gather = (buf, rank)
    return t


class _BDALayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias, residual, gamma, beta, p, eps, rms, seed, offset, gather=None, x2=None):
        """``gather`` = (world, rank, y_into_gather, dx_into_gather) under sequence parallelism:
        the normalised output (consumed by a column-parallel ring all-gather) and / or the input
        gradient (consumed by a row-parallel linear's backward all-gather) are written into their
        rank's slot of a gather buffer. ``x2`` (no gradient): a second summand of x, added in the
        kernel (a reduce-scatter's incoming partial, see ``tensor_parallel.rs_ring``); x's
        gradient is also x + x2's."""
        C = _ext.ext()
        x = x.contiguous()
        buf = out_y = None
        if gather is not None and gather[2]:
            buf, out_y = gather_slot(x, gather[0], gather[1])
        y, s, mean, rstd = C.layernorm_fwd(x, None if residual is None else residual.contiguous(),
                                           bias, gamma, beta, eps, p, seed, offset, rms, True, out_y,
                                           None if x2 is None else x2.contiguous())
        if buf is not None:
            _mark_gather(y, buf, gather[1])
        ctx.save_for_backward(s, gamma, mean, rstd)
        ctx.pref = (bias, gamma, beta)  # parameter objects: their main_grad / readiness hooks
        ctx.cfg = (p, seed, offset, rms, bias is not None, residual is not None, beta is not None,
                   gamma.dtype, None if bias is None else bias.dtype)
        ctx.gather = gather
        return y, s

    @staticmethod
    def backward(ctx, dy, ds):
        s, gamma, mean, rstd = ctx.saved_tensors
        p, seed, offset, rms, has_bias, has_res, has_beta, gdt, bdt = ctx.cfg
        C = _ext.ext()
        # the consuming column-parallel linear's backward reduce-scatter may leave its peer's
        # partial as a pending summand of dy (tensor_parallel.rs_ring, defer_add): added in-kernel
        from ..parallel.tensor_parallel import take_pending_add
        dy2 = take_pending_add(dy)
        dy = dy.contiguous()
        ds = None if ds is None else ds.contiguous()
        bias_p, gamma_p, beta_p = ctx.pref
        # bias / gamma / beta gradients go straight into fp32 main_grad when DDP owns them
        ta = grad_accumulate_target(gamma_p)
        tb = grad_accumulate_target(beta_p) if has_beta else None
        tc = grad_accumulate_target(bias_p) if has_bias else None
        gbuf = out_dx = None
        if ctx.gather is not None and ctx.gather[3]:
            gbuf, out_dx = gather_slot(s, ctx.gather[0], ctx.gather[1])
        d_s, dx, dgamma, dbeta, dbias = C.layernorm_bwd(dy, ds, s, gamma, mean, rstd, p, seed, offset, rms,
                                                        True, has_bias, ta, tb, tc, out_dx,
                                                        None if dy2 is None else dy2.contiguous())
        if gbuf is not None:
            _mark_gather(dx, gbuf, ctx.gather[1])
        _mark_ready(gamma_p if ta is not None else None, beta_p if tb is not None else None,
                    bias_p if tc is not None else None)
        g_gamma = None if ta is not None else dgamma.to(gdt)
        g_beta = None if (not has_beta or tb is not None) else dbeta.to(gdt)
        g_bias = None if (not has_bias or tc is not None) else dbias.to(bdt)
        return (dx, g_bias, d_s if has_res else None, g_gamma, g_beta, None, None, None, None, None, None, None)


def bias_dropout_add_norm(x, bias, residual, gamma, beta, p: float, training: bool, eps: float = 1e-5,
                          rms: bool = False, rng: Optional[PhiloxState] = None, gather=None):
    """Returns ``(norm(s), s)`` with ``s = residual + dropout(x + bias)``.

    ``bias``, ``residual`` may be None; ``beta`` is ignored for RMSNorm. This is the
    residual-stream step of a pre-LN transformer fused with the following LayerNorm.
    ``gather`` (world, rank, y, dx): see ``_BDALayerNorm.forward`` (kernel path only).
    """
    p = float(p) if training else 0.0
    # a row-parallel output whose reduce-scatter left its peer's partial as a pending summand
    # (tensor_parallel.rs_ring under defer_rs_add): x + x2 is the value, added in the kernel
    from ..parallel.tensor_parallel import plain, take_pending_add
    x2 = take_pending_add(x)
    x = plain(x)
    if _ext.use_kernels(x):
        seed, offset = _rng(rng).next() if p > 0 else (0, 0)
        return _BDALayerNorm.apply(x, bias, residual, gamma, None if rms else beta, p, float(eps), bool(rms),
                                   int(seed), int(offset), gather, x2)
    if x2 is not None:
        x = x + x2
    h = x if bias is None else x + bias
    if p > 0:
        h = F.dropout(h, p=p, training=True)
    s = h if residual is None else residual + h
    if rms:
        sf = s.float()
        y = (sf * torch.rsqrt(sf.pow(2).mean(-1, keepdim=True) + eps) * gamma.float()).to(s.dtype)
    else:
        y = F.layer_norm(s.float(), (s.shape[-1],), gamma.float(), None if beta is None else beta.float(),
                         eps).to(s.dtype)
    return y, s


def layer_norm(x, gamma, beta, eps: float = 1e-5):
    return bias_dropout_add_norm(x, None, None, gamma, beta, 0.0, False, eps, False)[0]


def rms_norm(x, gamma, eps: float = 1e-6):
    return bias_dropout_add_norm(x, None, None, gamma, None, 0.0, False, eps, True)[0]


def bias_dropout_add(x, bias, residual, p: float, training: bool):
    """Unfused residual step (pipeline-stage boundaries only)."""
    h = x if bias is None else x + bias
    if training and p > 0:
        h = F.dropout(h, p=p, training=True)
    return h if residual is None else residual + h


# --------------------------------------------------------------------------------------------
# bias + GeLU / SwiGLU

_ACT_CODES = {"gelu": 0, "gelu_tanh": 0, "gelu_erf": 1}


class _BiasAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias, act):
        C = _ext.ext()
        x = x.contiguous()
        y = C.bias_act_fwd(x, bias, act)
        ctx.save_for_backward(x, bias)
        ctx.bias_p = bias
        ctx.act = act
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, bias = ctx.saved_tensors
        C = _ext.ext()
        # a detached bias (ColumnParallelLinear(bias_grad_from_output=True): the linear produces
        # the bias gradient with its weight gradient) needs no column sums here
        want_db = ctx.has_bias and ctx.needs_input_grad[1]
        tgt = grad_accumulate_target(ctx.bias_p) if want_db else None
        dx, dbias = C.bias_act_bwd(dy.contiguous(), x, bias, ctx.act, want_db, tgt)
        if tgt is not None:
            _mark_ready(ctx.bias_p)
            return dx, None, None
        return dx, (dbias.to(bias.dtype) if want_db else None), None


def bias_gelu(x, bias=None, approximate: str = "tanh"):
    """GeLU(x + bias); ``approximate='tanh'`` is Megatron's bias_gelu, 'none' the erf form."""
    act = 0 if approximate == "tanh" else 1
    if _ext.use_kernels(x):
        return _BiasAct.apply(x, bias, act)
    h = x if bias is None else x + bias
    return F.gelu(h.float(), approximate="tanh" if act == 0 else "none").to(x.dtype)


class _SwiGLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        C = _ext.ext()
        x = x.contiguous()
        ctx.save_for_backward(x)
        return C.swiglu_fwd(x)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return _ext.ext().swiglu_bwd(dy.contiguous(), x)


def swiglu(x):
    """x = [gate | up] on the last dim -> silu(gate) * up."""
    if _ext.use_kernels(x):
        return _SwiGLU.apply(x)
    g, u = x.chunk(2, dim=-1)
    return (F.silu(g.float()) * u.float()).to(x.dtype)


# --------------------------------------------------------------------------------------------
# Scaled masked softmax (Megatron K1-K3)


class _ScaledSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask, mode, scale):
        C = _ext.ext()
        y = C.softmax_fwd(x.contiguous(), mask, mode, scale)
        ctx.save_for_backward(y)
        ctx.mode, ctx.scale = mode, scale
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return _ext.ext().softmax_bwd(dy.contiguous(), y, ctx.mode, ctx.scale), None, None, None


def scaled_masked_softmax(x, mask=None, scale: float = 1.0, causal: bool = False):
    """softmax(scale * x) over the last dim of [b, np, sq, sk].

    ``causal`` masks key j > query i (Megatron's upper-triangular mask) for any sq, sk: the
    triangle is aligned to the top-left corner, on the kernel path and the PyTorch path alike (for
    sq != sk this is NOT the bottom-right alignment of a decoding step). Otherwise ``mask``
    ([b, 1, sq, sk] or [1, 1, sq, sk] bool, True = masked) is applied if given; a fully masked
    row gives zeros.
    """
    mode = 1 if causal else (2 if mask is not None else 0)
    if _ext.use_kernels(x) and x.shape[-1] <= 4096 and x.shape[-1] % 8 == 0:
        m = None
        if mode == 2:
            m = mask.expand(x.shape[0], 1, x.shape[2], x.shape[3]).contiguous().to(torch.uint8)
        return _ScaledSoftmax.apply(x, m, mode, float(scale))
    xf = x.float() * scale
    if mode == 1:
        sq, sk = x.shape[-2], x.shape[-1]
        cm = torch.ones(sq, sk, dtype=torch.bool, device=x.device).triu(1)
        xf = xf.masked_fill(cm, float("-inf"))
    elif mode == 2:
        xf = xf.masked_fill(mask, float("-inf"))
    y = torch.softmax(xf, dim=-1)
    y = torch.nan_to_num(y, nan=0.0)
    return y.to(x.dtype)


# --------------------------------------------------------------------------------------------
# Flash attention


def _qkv_views(qkv, nh, nkv, hd, seq_first):
    """[S, B, W] (seq_first) or [B, S, W] fused projection output -> q, k, v as [B, S, H, D]
    views with W = (nh + 2 nkv) hd laid out as [q heads | k heads | v heads]."""
    if seq_first:
        x = qkv.transpose(0, 1)
    else:
        x = qkv
    q = x[..., : nh * hd].unflatten(-1, (nh, hd))
    k = x[..., nh * hd:(nh + nkv) * hd].unflatten(-1, (nkv, hd))
    v = x[..., (nh + nkv) * hd:].unflatten(-1, (nkv, hd))
    return q, k, v


def document_ends(doc_start):
    """The key-side twin of ``doc_start`` (int32 [B, S], the index of the first token of each
    token's document): ``doc_end[b, k]`` is one past the last token of ``k``'s document, so query
    ``q`` attends key ``k`` iff ``k <= q < doc_end[k]``  (<=> ``doc_start[q] <= k <= q``). The dK / dV
    kernel reads it. Device ops only (no host sync, capturable); the result is kept on the
    ``doc_start`` tensor object, so the layers of a model derive it once per batch — do not write
    into a ``doc_start`` after it was used."""
    de = getattr(doc_start, "_smdt_doc_end", None)
    if de is None:
        S = doc_start.shape[1]
        ar = torch.arange(S, dtype=torch.int32, device=doc_start.device)
        first = torch.where(doc_start == ar, ar, ar.new_full((), S))        # index of each first token, else S
        nxt = torch.cat([first[:, 1:], first.new_full((first.shape[0], 1), S)], dim=1)   # ... of tokens > k
        de = nxt.flip(1).cummin(dim=1).values.flip(1).to(torch.int32).contiguous()
        doc_start._smdt_doc_end = de
    return de


def document_mask(doc_start):
    """[B, 1, S, S] bool, True = masked: the left-to-right mask with per-document blocks (key after
    the query, or before the query's document) for the unfused softmax path."""
    S = doc_start.shape[1]
    ar = torch.arange(S, device=doc_start.device)
    m = (ar[None, None, :] > ar[None, :, None]) | (ar[None, None, :] < doc_start[:, :, None])
    return m.unsqueeze(1)


def _doc_check(doc_start, B, S, causal):
    if not causal:
        raise ValueError("doc_start (per-document attention) needs causal=True")
    if doc_start.dtype != torch.int32 or tuple(doc_start.shape) != (B, S):
        raise ValueError(f"doc_start must be int32 [B, S] = [{B}, {S}], got {doc_start.dtype} "
                         f"{tuple(doc_start.shape)}")


class _FlashAttnQKV(torch.autograd.Function):
    """``bias_p`` (the bias Parameter of the QKV projection whose output ``qkv`` is, or None): the
    backward kernels also emit the token sums of the fp32 dQ | dK | dV (flash_attn.hip SUMS), and
    their fixed-order reduction goes straight into the bias' fp32 ``main_grad`` — the projection
    then queues its weight gradient without bias tiles (tensor_parallel.bias_from_producer)."""

    @staticmethod
    def forward(ctx, qkv, nh, nkv, hd, seq_first, scale, causal, dropout_p=0.0, seed=0, offset=0,
                doc_start=None, doc_end=None, bias_p=None):
        ctx.bias_p = bias_p
        C = _ext.ext()
        q, k, v = _qkv_views(qkv, nh, nkv, hd, seq_first)
        if seq_first:
            S, B = qkv.shape[0], qkv.shape[1]
            out = qkv.new_empty(S, B, nh, hd)
            ov = out.transpose(0, 1)
        else:
            B, S = qkv.shape[0], qkv.shape[1]
            out = qkv.new_empty(B, S, nh, hd)
            ov = out
        _, lse = C.flash_fwd(q, k, v, scale, causal, ov, dropout_p, seed, offset, doc_start)
        ctx.save_for_backward(qkv, out, lse)
        ctx.cfg = (nh, nkv, hd, seq_first, scale, causal, dropout_p, seed, offset)
        ctx.doc = (doc_start, doc_end)      # integer descriptors: no gradient, no version tracking needed
        return out.flatten(-2)

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        nh, nkv, hd, seq_first, scale, causal, dropout_p, seed, offset = ctx.cfg
        C = _ext.ext()
        q, k, v = _qkv_views(qkv, nh, nkv, hd, seq_first)
        dqkv = torch.empty_like(qkv)
        dq, dk, dv = _qkv_views(dqkv, nh, nkv, hd, seq_first)
        do = dout.unflatten(-1, (nh, hd))
        o = out
        if seq_first:
            do = do.transpose(0, 1)
            o = o.transpose(0, 1)
        bias_p = ctx.bias_p
        if bias_p is None:
            C.flash_bwd(q, k, v, o, do, lse, scale, causal, dq, dk, dv, dropout_p, seed, offset, *ctx.doc)
        else:
            tgt = grad_accumulate_target(bias_p)
            if tgt is None or tgt.numel() != qkv.shape[-1]:
                raise RuntimeError("flash attention: the QKV bias gradient was left to the attention backward but "
                                   "the bias has no fp32 main_grad to receive it")
            C.flash_bwd_dbias(q, k, v, o, do, lse, scale, causal, tgt, True, dq, dk, dv, dropout_p, seed, offset,
                              *ctx.doc)
            bias_p._smdt_grad_ready(bias_p)
        return dqkv, None, None, None, None, None, None, None, None, None, None, None, None


class _FlashAttn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, scale, causal, dropout_p=0.0, seed=0, offset=0, doc_start=None, doc_end=None):
        C = _ext.ext()
        o, lse = C.flash_fwd(q, k, v, scale, causal, None, dropout_p, seed, offset, doc_start)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.cfg = (scale, causal, dropout_p, seed, offset)
        ctx.doc = (doc_start, doc_end)
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        scale, causal, p, seed, offset = ctx.cfg
        dq, dk, dv = _ext.ext().flash_bwd(q, k, v, o, do, lse, scale, causal, None, None, None, p, seed, offset,
                                          *ctx.doc)
        return dq, dk, dv, None, None, None, None, None, None, None


_M32 = 0xFFFFFFFF


def _fmix32_t(x):
    x = x ^ (x >> 16)
    x = (x * 0x85EBCA6B) & _M32
    x = x ^ (x >> 13)
    x = (x * 0xC2B2AE35) & _M32
    return x ^ (x >> 16)


def _fmix32_i(x: int) -> int:
    x &= _M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & _M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & _M32
    return x ^ (x >> 16)


def flash_dropout_thr(p: float):
    """(7-bit threshold, keep scale) the kernels use for drop probability ``p``: the realised drop
    rate is round(p * 128) / 128 (the kernels test the low 7 bits of each random byte with one
    SWAR add per 4 bytes; FlashAttention-2 thresholds random bytes too)."""
    thr = min(int(p * 128.0 + 0.5), 127)
    return thr, 128.0 / (128.0 - thr)


# Graph-safe dropout RNG. The fused dropout kernels take a (seed, offset) pair per call from the
# host (``_Rng``); inside a captured HIP graph those values are baked into the kernel arguments
# and every replay would redraw the same masks. With a device step counter registered, every
# dropout kernel mixes the counter's value into its key at run time (flash_attn.hip drop_key,
# layernorm.hip ln_drop_key); ``advance_graph_rng`` (a device add, captured with the step)
# moves it once per training step — after the backward, so forward and backward of a step see
# the same masks.
_GRAPH_RNG = {"counter": None}


def enable_graph_rng(device=None) -> torch.Tensor:
    c = _GRAPH_RNG["counter"]
    if c is None:
        c = torch.zeros(1, dtype=torch.int32, device=device or torch.device("cuda", torch.cuda.current_device()))
        _ext.ext().set_rng_step(c)
        _GRAPH_RNG["counter"] = c
    return c


def disable_graph_rng():
    if _GRAPH_RNG["counter"] is not None:
        _ext.ext().set_rng_step(None)
        _GRAPH_RNG["counter"] = None


def advance_graph_rng():
    c = _GRAPH_RNG["counter"]
    if c is not None:
        c.add_(1)


def flash_dropout_keep_mask(B: int, H: int, S: int, p: float, seed: int, offset: int, device=None,
                            step: Optional[int] = None):
    """Bit-exact twin of the flash kernels' dropout mask: bool [B, H, S(q), S(k)], True = kept
    (see ``drop_hash`` in flash_attn.hip): each 2x2 (query, key) block shares one hash, byte
    2 (q & 1) + (k & 1) decides the element (kept iff its low 7 bits >= the threshold).
    ``step``: the graph-safe RNG counter value the kernels read (``enable_graph_rng``)."""
    thr, _ = flash_dropout_thr(p)
    key0 = _fmix32_i((seed & _M32) ^ _fmix32_i(((seed >> 32) + 0x9E3779B9) & _M32))
    key1 = _fmix32_i((((offset & _M32) * 0x27D4EB2F) & _M32) ^ _fmix32_i(((offset >> 32) + 0x165667B1) & _M32))
    if step is not None:
        key1 ^= _fmix32_i(((step & _M32) * 0x9E3779B1 + 0x85EBCA77) & _M32)
    bh = torch.arange(B * H, dtype=torch.int64, device=device)
    kbh = _fmix32_t((key0 + bh * 0x632BE5AB) & _M32) ^ key1                          # [BH]
    half = S // 2
    blk = (torch.arange(half, dtype=torch.int64, device=device)[:, None] * half
           + torch.arange(half, dtype=torch.int64, device=device)[None, :])            # [S/2, S/2]
    x = blk[None] ^ kbh[:, None, None]
    x = (((x ^ (x >> 16)) & 0xFFFFFF) * 0x45D9F3) & _M32   # v_mul_u32_u24
    x = (((x ^ (x >> 16)) & 0xFFFFFF) * 0x45D9F3) & _M32
    x = x ^ (x >> 16)
    by = torch.stack([(x >> (8 * i)) & 0x7F for i in range(4)], dim=-1) >= thr           # [BH, S/2, S/2, 4]
    # byte 2 qb + kb -> [BH, S/2, S/2, 2(q), 2(k)] -> [BH, S/2, 2, S/2, 2]
    keep = by.view(B * H, half, half, 2, 2).permute(0, 1, 3, 2, 4)
    return keep.reshape(B, H, S, S)


def attention_ref(q, k, v, scale, causal, dropout_p: float = 0.0, keep=None, doc_start=None):
    """Reference attention on [B, S, H, D] (GQA by head repetition), fp32 math (float64 for float64
    inputs). ``keep``
    ([B, H, S, S] bool) is the dropout keep-mask (``flash_dropout_keep_mask``). ``doc_start``
    (int32 [B, S], causal only) also masks keys before the query's document: block-diagonal causal."""
    if q.is_cuda and os.environ.get("SMDT_ASSERT_FLASH") == "1":
        raise RuntimeError("SMDT_ASSERT_FLASH=1: reference attention reached on the GPU")
    B, S, H, D = q.shape
    Hkv = k.shape[2]
    if Hkv != H:
        k = k.repeat_interleave(H // Hkv, dim=2)
        v = v.repeat_interleave(H // Hkv, dim=2)
    wd = torch.float64 if q.dtype == torch.float64 else torch.float32   # float64 in, float64 math (tests)
    qf, kf, vf = (t.to(wd).transpose(1, 2) for t in (q, k, v))
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale
    if causal:
        cm = torch.ones(S, S, dtype=torch.bool, device=q.device).triu(1)
        s = s.masked_fill(cm, float("-inf"))
    if doc_start is not None:
        _doc_check(doc_start, B, S, causal)
        ar = torch.arange(S, device=q.device)
        s = s.masked_fill((ar[None, None, :] < doc_start[:, :, None]).unsqueeze(1), float("-inf"))
    p = torch.softmax(s, dim=-1)
    if dropout_p > 0:
        if keep is None:
            p = torch.nn.functional.dropout(p, dropout_p, training=True)
        else:
            p = p * keep * flash_dropout_thr(dropout_p)[1]
    o = torch.matmul(p, vf).transpose(1, 2)
    return o.to(q.dtype)


def flash_supported(q, k) -> bool:
    """True when the kernels take q / k exactly as they are (no padding)."""
    B, S, H, D = q.shape
    return (q.dtype in (torch.bfloat16, torch.float16) and D in (64, 128) and S % 128 == 0
            and H % k.shape[2] == 0 and q.stride(-1) == 1 and k.stride(-1) == 1)


def _flash_plan(q, k, causal: bool):
    """(S_pad, D_pad) the gfx950 kernels run this attention at, or raise — a GPU tensor never
    drops to the materialised S x S reference (ops/_ext.py policy).

    Padding is exact where it is used: head dims below 64 / 128 are zero-padded (zero q / k
    columns add nothing to q.k, zero v columns produce output columns that are sliced off, and
    the softmax scale stays 1 / sqrt(D_orig)); a causal sequence is padded at its END (no real
    query attends to a later key). A non-causal sequence that is not a multiple of 128 would
    need key masking and is rejected."""
    B, S, H, D = q.shape
    if q.dtype not in (torch.bfloat16, torch.float16):
        raise RuntimeError(f"flash attention on the GPU runs bf16 / fp16, got {q.dtype}; cast the model "
                           "(--bf16 / --fp16) or disable flash attention (--no-flash-attn)")
    if H % k.shape[2]:
        raise RuntimeError(f"flash attention: {H} query heads are not a multiple of {k.shape[2]} kv heads")
    if D > 128:
        raise RuntimeError(f"flash attention: head dim {D} > 128 is not supported by the gfx950 kernels")
    Dp = 64 if D <= 64 else 128
    Sp = -(-S // 128) * 128
    if Sp != S and not causal:
        raise RuntimeError(f"flash attention: non-causal sequence length {S} must be a multiple of 128")
    return Sp, Dp


def _pad_bshd(t, Sp, Dp):
    S, D = t.shape[1], t.shape[3]
    if Sp == S and Dp == D:
        return t
    return torch.nn.functional.pad(t, (0, Dp - D, 0, 0, 0, Sp - S))


def _doc_args(doc_start, S, Sp):
    """(doc_start, doc_end) as the kernels take them at the padded length ``Sp``: the pad rows
    S .. Sp - 1 form a document of their own, so no real token's bounds move."""
    if doc_start is None:
        return None, None
    if Sp != S:
        pad = doc_start.new_full((doc_start.shape[0], Sp - S), S)
        doc_start = torch.cat([doc_start, pad], dim=1)
    doc_start = doc_start.contiguous()
    return doc_start, document_ends(doc_start)


def flash_attention(q, k, v, scale: Optional[float] = None, causal: bool = True, dropout_p: float = 0.0,
                    rng: Optional[PhiloxState] = None, doc_start=None):
    """Attention over [B, S, H, D] tensors (any batch/seq/head strides, unit last stride);
    ``k``/``v`` may have fewer heads (GQA). ``doc_start`` (int32 [B, S], non-decreasing along S,
    ``doc_start[b, i] <= i``; causal only): per-document attention of packed samples, query ``q``
    attends key ``k`` iff ``doc_start[b, q] <= k <= q``."""
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    if doc_start is not None:
        _doc_check(doc_start, q.shape[0], q.shape[1], causal)
    seed, off = _rng(rng).next() if dropout_p > 0 else (0, 0)
    if _ext.use_kernels(q):
        S, D = q.shape[1], q.shape[3]
        Sp, Dp = _flash_plan(q, k, causal)
        ds, de = _doc_args(doc_start, S, Sp)
        if (Sp, Dp) == (S, D) and flash_supported(q, k):
            return _FlashAttn.apply(q, k, v, float(scale), bool(causal), float(dropout_p), int(seed), int(off),
                                    ds, de)
        qp, kp, vp = (_pad_bshd(t.contiguous() if t.stride(-1) != 1 else t, Sp, Dp) for t in (q, k, v))
        o = _FlashAttn.apply(qp, kp, vp, float(scale), bool(causal), float(dropout_p), int(seed), int(off), ds, de)
        return o[:, :S, :, :D]
    keep = flash_dropout_keep_mask(q.shape[0], q.shape[2], q.shape[1], dropout_p, seed, off, q.device) \
        if dropout_p > 0 else None
    return attention_ref(q, k, v, scale, causal, dropout_p, keep, doc_start)


def flash_attention_qkv(qkv, nh: int, nkv: int, hd: int, seq_first: bool = True, causal: bool = True,
                        scale: Optional[float] = None, dropout_p: float = 0.0, rng: Optional[PhiloxState] = None,
                        doc_start=None, bias_p=None):
    """Attention straight off a fused QKV projection output.

    ``qkv`` is [S, B, (nh + 2 nkv) hd] (``seq_first``) or [B, S, ...]; returns [S, B, nh hd]
    (resp. [B, S, nh hd]). Backward produces ONE fused d(qkv) buffer. ``dropout_p`` > 0 applies
    attention-probability dropout inside the kernels (mask re-derived from ``rng``'s
    (seed, offset) in backward — nothing is stored). Shapes the kernels cannot read in place
    (S % 128 != 0, head dim not 64 / 128) go through the padded separate-q/k/v path.
    ``doc_start`` (int32 [B, S], batch-first whatever ``seq_first``): per-document attention, see
    ``flash_attention``. ``bias_p``: see ``_FlashAttnQKV``; the caller has left the QKV bias
    gradient to this call, so a shape that misses the in-place kernels is an error.
    """
    if scale is None:
        scale = 1.0 / math.sqrt(hd)
    q, k, v = _qkv_views(qkv, nh, nkv, hd, seq_first)
    if doc_start is not None:
        _doc_check(doc_start, q.shape[0], q.shape[1], causal)
    fused = (_ext.use_kernels(qkv) and qkv.is_contiguous() and flash_supported(q, k)
             and (nh + 2 * nkv) * hd % 8 == 0)
    if bias_p is not None and not fused:
        raise RuntimeError("flash_attention_qkv: the QKV bias gradient was left to the attention backward, but "
                           "this call does not run the in-place flash kernels")
    if _ext.use_kernels(qkv):
        if fused:
            seed, off = _rng(rng).next() if dropout_p > 0 else (0, 0)
            ds, de = _doc_args(doc_start, q.shape[1], q.shape[1])
            return _FlashAttnQKV.apply(qkv, nh, nkv, hd, bool(seq_first), float(scale), bool(causal),
                                       float(dropout_p), int(seed), int(off), ds, de, bias_p)
        o = flash_attention(q, k, v, scale, causal, dropout_p, rng, doc_start)          # [B, S, H, D]
    else:
        seed, off = _rng(rng).next() if dropout_p > 0 else (0, 0)
        keep = None
        if dropout_p > 0:
            keep = flash_dropout_keep_mask(q.shape[0], nh, q.shape[1], dropout_p, seed, off, qkv.device)
        o = attention_ref(q, k, v, scale, causal, dropout_p, keep, doc_start)  # [B, S, H, D]
    if seq_first:
        o = o.transpose(0, 1)
    return o.flatten(-2).contiguous()


# --------------------------------------------------------------------------------------------
# Swin shifted-window attention on the qkv linear's output over the padded, unrolled grid.
#
# Window (wy, wx) token (iy, ix) is rolled coordinate (y, x) = (wy ws + iy, wx ws + ix); it is read
# from and written to source coordinate ((y + shift) mod ph, (x + shift) mod pw). The shift mask's
# region of a rolled coordinate is 0 for y < ph - ws, 1 for y < ph - shift, else 2 (same in x), id
# 3 ry + rx: the image ShiftedWindowAttention._bias paints. window_attn.hip computes the same
# mapping as address arithmetic; window_attention_ref is its statement in torch ops.


def window_attention_map(ph: int, pw: int, window: int, shift: int, device=None):
    """(src, region), both int64 [nW, N]: the flat index into the [ph * pw] token grid of every
    window token, and its shift-mask region id."""
    ws = window
    ar = lambda n, *shape: torch.arange(n, device=device).view(*shape)  # noqa: E731
    y = (ar(ph // ws, -1, 1, 1, 1) * ws + ar(ws, 1, 1, -1, 1)).expand(ph // ws, pw // ws, ws, ws)
    x = (ar(pw // ws, 1, -1, 1, 1) * ws + ar(ws, 1, 1, 1, -1)).expand(ph // ws, pw // ws, ws, ws)
    src = ((y + shift) % ph) * pw + (x + shift) % pw
    ry = (y >= ph - ws).long() + (y >= ph - shift).long()
    rx = (x >= pw - ws).long() + (x >= pw - shift).long()
    return src.reshape(-1, ws * ws), (3 * ry + rx).reshape(-1, ws * ws)


def window_attention_ref(qkv, table, window: int, shift: int, num_heads: int):
    """Torch twin of the fused kernel: qkv [B, ph, pw, 3 C] read as (3, heads, d), table
    [(2 ws - 1)^2, heads] -> [B, ph, pw, C] at the unrolled positions. Gather by computed source
    coordinates, scores and softmax in fp32 (float64 for float64 operands)."""
    B, ph, pw, C3 = qkv.shape
    ws, N, C = window, window * window, C3 // 3
    d = C // num_heads
    if ph % ws or pw % ws or C3 != 3 * num_heads * d or not 0 <= shift < ws:
        raise ValueError(f"window_attention: grid {ph} x {pw}, window {ws}, shift {shift}, last dim {C3}, "
                         f"heads {num_heads} do not fit")
    ct = torch.float64 if qkv.dtype == torch.float64 else torch.float32
    src, region = window_attention_map(ph, pw, ws, shift, qkv.device)
    nW = src.shape[0]
    x = qkv.reshape(B, ph * pw, 3, num_heads, d)[:, src.flatten()].view(B, nW, N, 3, num_heads, d)
    q, k, v = (t.permute(0, 1, 3, 2, 4).to(ct) for t in x.unbind(3))                # [B, nW, h, N, d]
    t = torch.arange(N, device=qkv.device)
    c = (t // ws) * (2 * ws - 1) + t % ws
    idx = c[:, None] - c[None, :] + 2 * ws * (ws - 1)
    s = q.matmul(k.transpose(-2, -1)) * d ** -0.5 + table.to(ct)[idx].permute(2, 0, 1)
    if shift > 0:
        s = s + (region[:, :, None] != region[:, None, :]).to(ct).mul(-100.0)[None, :, None]
    o = torch.softmax(s, dim=-1).matmul(v).permute(0, 1, 3, 2, 4).reshape(B, nW * N, C).to(qkv.dtype)
    return o[:, torch.argsort(src.flatten())].view(B, ph, pw, C)


def window_attention_supported(qkv, window: int, shift: int, num_heads: int) -> bool:
    """The shapes window_attn.hip takes (smdt_window_attn_supported in launchers.h)."""
    if qkv.dim() != 4 or qkv.dtype not in (torch.bfloat16, torch.float16) or num_heads <= 0:
        return False
    B, ph, pw, C3 = qkv.shape
    if not (C3 == 96 * num_heads and 1 <= window <= 8 and ph >= window and pw >= window and ph % window == 0
            and pw % window == 0 and 0 <= shift < window and qkv.numel() > 0):
        return False
    # the binding's and the launcher's size limits: grid sides below 2^20, at most 2^30 (window, head) waves
    return ph < 2 ** 20 and pw < 2 ** 20 and B * (ph // window) * (pw // window) * num_heads <= 2 ** 30


class _WindowAttn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, table, window, shift, heads):
        tf = table.detach().float().contiguous()
        qkv = qkv.contiguous()
        out, lse = _ext.ext().window_attn_fwd(qkv, tf, window, shift, heads)
        ctx.save_for_backward(qkv, tf, lse)
        ctx.args = (window, shift, heads, table.dtype)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, tf, lse = ctx.saved_tensors
        window, shift, heads, tdtype = ctx.args
        dqkv, dtable = _ext.ext().window_attn_bwd(qkv, tf, lse, dout.contiguous(), window, shift, heads)
        return dqkv, dtable.to(tdtype), None, None, None


def window_attention(qkv, table, window: int, shift: int, num_heads: int):
    """Shifted-window attention core of a Swin block (no dropout): see window_attention_ref for the
    semantics. bf16 / fp16 GPU operands of a supported shape run the fused HIP kernels (under
    autocast an fp32 qkv is cast to the autocast dtype first); the CPU, SMDT_DISABLE_KERNELS=1 and
    every other dtype or shape run the torch twin."""
    if qkv.is_cuda and qkv.dtype == torch.float32 and torch.is_autocast_enabled():
        qkv = qkv.to(torch.get_autocast_gpu_dtype())
    if window_attention_supported(qkv, window, shift, num_heads) and _ext.use_kernels(qkv):
        return _WindowAttn.apply(qkv, table, window, shift, num_heads)
    return window_attention_ref(qkv, table, window, shift, num_heads)


# --------------------------------------------------------------------------------------------
# Rotary embedding


def rope_tables(max_pos: int, rot_dim: int, base: float = 10000.0, device=None):
    inv = 1.0 / (base ** (torch.arange(0, rot_dim, 2, dtype=torch.float64) / rot_dim))
    t = torch.arange(max_pos, dtype=torch.float64)
    f = torch.outer(t, inv)
    return f.cos().float().to(device), f.sin().float().to(device)


def _rope_ref(x, cos, sin, rot, pos, inverse=False):
    # x [ntok, nh, d]; pos [ntok]
    xr = x[..., :rot].float()
    x1, x2 = xr[..., : rot // 2], xr[..., rot // 2:]
    c = cos[pos].unsqueeze(1)
    s = sin[pos].unsqueeze(1)
    if inverse:
        s = -s
    out = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).to(x.dtype)
    return torch.cat([out, x[..., rot:]], dim=-1) if rot < x.shape[-1] else out


class _Rope(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cos, sin, rot, pos_div, pos_mod):
        y = x.clone()
        _ext.ext().rope_(y, cos, sin, rot, pos_div, pos_mod, False)
        ctx.save_for_backward(cos, sin)
        ctx.cfg = (rot, pos_div, pos_mod)
        return y

    @staticmethod
    def backward(ctx, dy):
        cos, sin = ctx.saved_tensors
        rot, pos_div, pos_mod = ctx.cfg
        dx = dy.contiguous().clone()
        _ext.ext().rope_(dx, cos, sin, rot, pos_div, pos_mod, True)
        return dx, None, None, None, None, None


def apply_rope(x, cos, sin, pos_div: int, pos_mod: int, rot: Optional[int] = None):
    """Rotate-half RoPE on x [ntok, nh, d]; token t has position (t // pos_div) % pos_mod."""
    rot = rot or x.shape[-1]
    if _ext.use_kernels(x) and rot % 16 == 0:
        xx = x if x.stride(-1) == 1 and x.stride(0) % 8 == 0 and x.stride(1) % 8 == 0 else x.contiguous()
        return _Rope.apply(xx, cos, sin, rot, pos_div, pos_mod)
    pos = (torch.arange(x.shape[0], device=x.device) // pos_div) % pos_mod
    return _rope_ref(x, cos.to(x.device), sin.to(x.device), rot, pos)


# --------------------------------------------------------------------------------------------
# Incremental decoding (csrc/kernels/decode_attn.hip; decode_common.h holds what it shares with
# the MXFP8 and multi-token files below): one new token per sequence against a K/V cache [B, cap,
# nkv, D]. Lengths and positions are device int32 [B] tensors and are never read on the host, so a
# decode step has static shapes and can be captured in a graph.

DECODE_CHUNK = 256      # keys per workgroup of the split-KV kernel (smdt_decode_attn_chunk)


def _decode_max_len(name, max_len, cap):
    """The grid bound an attention wrapper hands its kernel: ``max_len`` (None: the capacity), in 1 .. cap."""
    max_len = cap if max_len is None else int(max_len)
    if not 0 < max_len <= cap:
        raise ValueError(f"{name}: max_len {max_len} must be in 1 .. the capacity {cap}")
    return max_len


def _decode_check_qkv(name, qkv, nh, nkv, hd, lead="B"):
    """qkv is [B, W] (``lead`` "B") or [B, T, W] ("B, T") with W = (nh + 2 nkv) hd."""
    W = (nh + 2 * nkv) * hd
    if qkv.dim() != lead.count(",") + 2 or qkv.shape[-1] != W:
        raise ValueError(f"{name}: qkv {tuple(qkv.shape)} is not [{lead}, (nh + 2 nkv) hd] = [{lead}, {W}]")


def _decode_check_caches(name, qkv, k_cache, v_cache, nkv, hd):
    if tuple(k_cache.shape[2:]) != (nkv, hd) or k_cache.shape != v_cache.shape or k_cache.shape[0] != qkv.shape[0]:
        raise ValueError(f"{name}: caches {tuple(k_cache.shape)} / {tuple(v_cache.shape)} are not "
                         f"[B, cap, {nkv}, {hd}]")


def _decode_check_append_gpu(name, qkv, k_cache, v_cache, hd, rope):
    """What the 16-bit append kernel takes of GPU operands."""
    if qkv.dtype not in (torch.bfloat16, torch.float16) or k_cache.dtype != qkv.dtype or v_cache.dtype != qkv.dtype \
            or hd % 8 or (rope is not None and rope[2] % 16):
        raise RuntimeError(f"{name} on the GPU needs bf16 / fp16 qkv and caches of one dtype, hd % 8 == 0 "
                           f"and a rotary dim % 16 == 0; got {qkv.dtype} / {k_cache.dtype} / {v_cache.dtype}, hd {hd}")


def _rope_args(rope):
    """The append bindings' trailing arguments: (cos, sin, rot) of the model's tables, nothing without RoPE."""
    if rope is None:
        return ()
    cos, sin, rot = rope
    return cos, sin, int(rot)


def decode_attention_supported(q, k_cache, v_cache=None) -> bool:
    """The operands decode_attn.hip takes (smdt_decode_attn_supported in launchers.h): q [B, nh, D]
    and caches [B, cap, nkv, D] of one 16-bit dtype, D in {64, 128}, nh / nkv in {1, 2, 4, 8}."""
    if q.dim() != 3 or k_cache.dim() != 4 or q.dtype not in (torch.bfloat16, torch.float16):
        return False
    if k_cache.dtype != q.dtype or (v_cache is not None and (v_cache.dtype != q.dtype or v_cache.shape != k_cache.shape)):
        return False
    (B, nh, D), (Bk, cap, nkv, Dk) = q.shape, k_cache.shape
    if B != Bk or D != Dk or D not in (64, 128) or B < 1 or cap < 1 or nkv < 1 or nh % nkv:
        return False
    return nh // nkv in (1, 2, 4, 8) and B <= 65535 and nkv <= 65535


def decode_attention_ref(q, k_cache, v_cache, lens, scale, max_len=None):
    """Torch twin of the kernel: softmax(scale q . K[:lens[b]]) V[:lens[b]] per sequence and head,
    kv head h // (nh / nkv) serving query head h. fp32 math (float64 for float64 operands), one
    rounding at the output. Rows at or beyond ``lens[b]`` are selected out before any arithmetic,
    so NaN / Inf there cannot reach the result. ``max_len`` only bounds the kernel's grid."""
    B, nh, D = q.shape
    cap, nkv = k_cache.shape[1], k_cache.shape[2]
    if nh % nkv:
        raise ValueError(f"decode_attention: {nh} query heads are not a multiple of {nkv} kv heads")
    ct = torch.float64 if q.dtype == torch.float64 else torch.float32
    valid = torch.arange(cap, device=q.device)[None, :] < lens[:, None]                       # [B, cap]
    zero = torch.zeros((), dtype=ct, device=q.device)
    kk = torch.where(valid[:, :, None, None], k_cache.to(ct), zero)
    vv = torch.where(valid[:, :, None, None], v_cache.to(ct), zero)
    qg = q.to(ct).view(B, nkv, nh // nkv, D)
    s = torch.einsum("bkgd,bckd->bkgc", qg, kk) * scale
    s = s.masked_fill(~valid[:, None, None, :], float("-inf"))
    o = torch.einsum("bkgc,bckd->bkgd", torch.softmax(s, dim=-1), vv)
    return o.reshape(B, nh, D).to(q.dtype)


def decode_attention(q, k_cache, v_cache, lens, scale, max_len=None):
    """Attention of one new query per sequence, q [B, nh, D], against the caches [B, cap, nkv, D]:
    keys 0 .. lens[b] - 1 (``lens`` int32 [B] on q's device, the new token included). ``max_len``
    (host int <= cap, default cap) only bounds the kernel's grid: every lens[b] must be <= it.
    GPU operands run decode_attn.hip or raise (``decode_attention_supported``); CPU operands run
    the torch twin."""
    if not _ext.use_kernels(q, k_cache, v_cache):
        return decode_attention_ref(q, k_cache, v_cache, lens, scale, max_len)
    if not decode_attention_supported(q, k_cache, v_cache):
        raise RuntimeError(f"decode_attention on the GPU needs bf16 / fp16 q [B, nh, D] and caches [B, cap, nkv, D] "
                           f"of one dtype, D in (64, 128) and nh / nkv in (1, 2, 4, 8); got q {tuple(q.shape)} "
                           f"{q.dtype}, k_cache {tuple(k_cache.shape)} {k_cache.dtype}, v_cache "
                           f"{tuple(v_cache.shape)} {v_cache.dtype}")
    max_len = _decode_max_len("decode_attention", max_len, k_cache.shape[1])
    return _ext.ext().decode_attn(q.contiguous(), k_cache, v_cache, lens, float(scale), max_len)


def _decode_rope_rows(qkv, pos, nh, nkv, hd, rope):
    """q [B, nh, hd], k and v [B, nkv, hd] of the new tokens, q / k rotated at pos[b] (``_rope_ref``)."""
    B = qkv.shape[0]
    q = qkv[:, : nh * hd].reshape(B, nh, hd)
    k = qkv[:, nh * hd:(nh + nkv) * hd].reshape(B, nkv, hd)
    v = qkv[:, (nh + nkv) * hd:].reshape(B, nkv, hd)
    if rope is not None:
        cos, sin, rot = rope
        q = _rope_ref(q, cos.to(qkv.device), sin.to(qkv.device), rot, pos.long())
        k = _rope_ref(k, cos.to(qkv.device), sin.to(qkv.device), rot, pos.long())
    return q, k, v


def decode_rope_append_ref(qkv, k_cache, v_cache, pos, nh, nkv, hd, rope=None):
    """Torch twin of ``decode_rope_append`` (``_rope_ref`` at position pos[b], index writes)."""
    q, k, v = _decode_rope_rows(qkv, pos, nh, nkv, hd, rope)
    rows = torch.arange(qkv.shape[0], device=qkv.device)
    k_cache[rows, pos.long()] = k.to(k_cache.dtype)
    v_cache[rows, pos.long()] = v.to(v_cache.dtype)
    return q.contiguous()


def decode_rope_append(qkv, k_cache, v_cache, pos, nh, nkv, hd, rope=None):
    """One new token per sequence: ``qkv`` [B, (nh + 2 nkv) hd] is the QKV projection's output,
    ``pos`` int32 [B] (device) each token's position. q and k are rotated at pos[b] (``rope`` =
    (cos, sin, rot) tables of the model, None: no RoPE), k and v are written into row pos[b] of the
    caches [B, cap, nkv, hd] and q [B, nh, hd] is returned. The rotation is bit for bit what the
    ``rope_`` kernel writes for the same row at the same position. GPU operands run the kernel or
    raise; CPU operands run the torch twin."""
    _decode_check_qkv("decode_rope_append", qkv, nh, nkv, hd)
    _decode_check_caches("decode_rope_append", qkv, k_cache, v_cache, nkv, hd)
    if not _ext.use_kernels(qkv, k_cache, v_cache):
        return decode_rope_append_ref(qkv, k_cache, v_cache, pos, nh, nkv, hd, rope)
    _decode_check_append_gpu("decode_rope_append", qkv, k_cache, v_cache, hd, rope)
    return _ext.ext().decode_rope_append(qkv.contiguous(), k_cache, v_cache, pos, nh, *_rope_args(rope))


# --------------------------------------------------------------------------------------------
# Multi-token decode step (csrc/kernels/decode_attn_multi.hip): T new tokens per sequence in one
# pass, the verify step of speculative decoding. q is [B, T, nh, D]; ``lens`` counts the keys with
# all T new tokens appended and query t sees keys 0 .. lens[b] - T + t (the old keys, the new tokens
# before it, itself). T = 1 is ``decode_attention``'s meaning.

DECODE_MULTI_MAX_T = 8      # smdt_decode_attn_multi_max_t(): T * (nh / nkv) <= 64 query rows per kv head


def decode_attention_multi_supported(q, k_cache, v_cache=None) -> bool:
    """The operands decode_attn_multi.hip takes (smdt_decode_attn_multi_supported): q [B, T, nh, D]
    with 1 <= T <= ``DECODE_MULTI_MAX_T`` and otherwise ``decode_attention_supported``'s set."""
    if q.dim() != 4 or not 1 <= q.shape[1] <= DECODE_MULTI_MAX_T or q.shape[1] * q.shape[2] > 65535:
        return False
    return decode_attention_supported(q[:, 0], k_cache, v_cache)


def _multi_limits(lens, T):
    """[B, T]: the number of keys query t of sequence b sees, lens[b] - T + t + 1 (not below 0)."""
    return (lens.long()[:, None] - T + 1 + torch.arange(T, device=lens.device)[None, :]).clamp_(min=0)


def decode_attention_multi_ref(q, k_cache, v_cache, lens, scale, max_len=None, emulate: bool = False):
    """Torch twin of ``decode_attention_multi``. Default: ``decode_attention_ref`` of every query t
    over its own lens[b] - T + t + 1 keys (fp32 math, float64 for float64 operands, one rounding at
    the output; the bits of ``decode_attention_ref`` at T = 1); a query that sees no key returns
    zeros. Keys at or beyond a query's limit are selected out before any arithmetic.

    ``emulate=True`` places the kernel's rounding points instead: per chunk of ``DECODE_CHUNK`` keys
    the probabilities exp(s - chunk maximum) are rounded to q's dtype before the P V product
    (their sum l stays unrounded fp32), the product accumulates in fp32, the chunks are combined in
    fp32 as the combine kernel does, and the output is rounded once."""
    B, T, nh, D = q.shape
    lim = _multi_limits(lens, T)
    if not emulate:
        out = torch.empty_like(q)
        for t in range(T):
            o = decode_attention_ref(q[:, t].contiguous(), k_cache, v_cache, lim[:, t], scale)
            out[:, t] = torch.where((lim[:, t] > 0)[:, None, None], o, torch.zeros((), dtype=q.dtype, device=q.device))
        return out
    cap, nkv = k_cache.shape[1], k_cache.shape[2]
    if nh % nkv:
        raise ValueError(f"decode_attention_multi: {nh} query heads are not a multiple of {nkv} kv heads")
    C = DECODE_CHUNK
    nc = (cap + C - 1) // C
    f32 = torch.float32
    valid = torch.arange(cap, device=q.device)[None, None, :] < lim[:, :, None]             # [B, T, cap]
    used = valid.any(dim=1)                                                                  # [B, cap]
    zero = torch.zeros((), dtype=f32, device=q.device)
    kk = torch.where(used[:, :, None, None], k_cache.to(f32), zero)
    vv = torch.where(used[:, :, None, None], v_cache.to(f32), zero)
    qg = q.to(f32).reshape(B, T, nkv, nh // nkv, D)
    s = torch.einsum("btkgd,bckd->btkgc", qg, kk) * scale
    s = s.masked_fill(~valid[:, :, None, None, :], float("-inf"))
    pad = nc * C - cap
    if pad:
        s = torch.nn.functional.pad(s, (0, pad), value=float("-inf"))
        vv = torch.nn.functional.pad(vv, (0, 0, 0, 0, 0, pad))
    s = s.view(B, T, nkv, nh // nkv, nc, C)
    m = s.amax(dim=-1)                                                                       # [B, T, k, g, nc]
    p = torch.where(s == float("-inf"), zero, torch.exp(s - m.unsqueeze(-1).clamp(min=-3.0e38)))
    l = p.sum(dim=-1)
    acc = torch.einsum("btkgnc,bnckd->btkgnd", p.to(q.dtype).to(f32), vv.view(B, nc, C, nkv, D))
    has = l > 0
    M = torch.where(has, m, torch.full_like(m, float("-inf"))).amax(dim=-1, keepdim=True)
    w = torch.where(has, torch.exp(m - M.clamp(min=-3.0e38)), zero)
    num = (w.unsqueeze(-1) * acc).sum(dim=-2)
    den = (w * l).sum(dim=-1, keepdim=True)
    o = torch.where(den > 0, num / den.clamp(min=1e-38), zero)
    return o.reshape(B, T, nh, D).to(q.dtype)


def decode_attention_multi(q, k_cache, v_cache, lens, scale, max_len=None):
    """Attention of T new queries per sequence, q [B, T, nh, D], against the caches [B, cap, nkv, D]
    that already hold the T new tokens' keys: ``lens`` (int32 [B] on q's device) counts the keys
    with all T appended and query t sees keys 0 .. lens[b] - T + t. Returns [B, T, nh, D]; a query
    that sees no key returns zeros. ``max_len`` (host int <= cap, default cap) only bounds the
    kernel's grid. GPU operands run decode_attn_multi.hip (scores and P V on the 16x16x32 MFMA) or
    raise (``decode_attention_multi_supported``); CPU operands run the torch twin."""
    if q.dim() != 4:
        raise ValueError(f"decode_attention_multi: q must be [B, T, nh, D], got {tuple(q.shape)}")
    if not _ext.use_kernels(q, k_cache, v_cache):
        if q.shape[1] < 1:
            raise ValueError("decode_attention_multi: T must be at least 1")
        return decode_attention_multi_ref(q, k_cache, v_cache, lens, scale, max_len)
    if not decode_attention_multi_supported(q, k_cache, v_cache):
        raise RuntimeError(f"decode_attention_multi on the GPU needs bf16 / fp16 q [B, T, nh, D] with 1 <= T <= "
                           f"{DECODE_MULTI_MAX_T} and 16-bit caches [B, cap, nkv, D] of q's dtype (not an MXFP8 cache), "
                           f"D in (64, 128) and nh / nkv in (1, 2, 4, 8); got q {tuple(q.shape)} {q.dtype}, k_cache "
                           f"{tuple(k_cache.shape)} {k_cache.dtype}, v_cache {tuple(v_cache.shape)} {v_cache.dtype}")
    max_len = _decode_max_len("decode_attention_multi", max_len, k_cache.shape[1])
    return _ext.ext().decode_attn_multi(q.contiguous(), k_cache, v_cache, lens, float(scale), max_len)


def decode_rope_append_multi_ref(qkv, k_cache, v_cache, pos, nh, nkv, hd, rope=None):
    """Torch twin of ``decode_rope_append_multi``: T calls of ``decode_rope_append_ref``, token t at
    position pos[b] + t."""
    T = qkv.shape[1]
    return torch.stack([decode_rope_append_ref(qkv[:, t], k_cache, v_cache, pos + t, nh, nkv, hd, rope)
                        for t in range(T)], dim=1)


def decode_rope_append_multi(qkv, k_cache, v_cache, pos, nh, nkv, hd, rope=None):
    """T new tokens per sequence: ``qkv`` [B, T, (nh + 2 nkv) hd]. Token t of sequence b is rotated
    at position pos[b] + t (``pos`` int32 [B], device) and its k / v are written into cache row
    pos[b] + t; q [B, T, nh, hd] is returned. The bytes are those of T calls of
    ``decode_rope_append``. The kernel takes the batch and token strides as they are (rows of W
    contiguous elements, strides multiples of 8 elements), so the model passes its sequence-first
    [T, B, W] projection as ``qkv.transpose(0, 1)`` and no copy is made; anything else is copied
    here. GPU operands run the kernel or raise; CPU operands run the torch twin."""
    _decode_check_qkv("decode_rope_append_multi", qkv, nh, nkv, hd, lead="B, T")
    if not 1 <= qkv.shape[1] <= DECODE_MULTI_MAX_T:
        raise ValueError(f"decode_rope_append_multi: T = {qkv.shape[1]} is outside 1 .. {DECODE_MULTI_MAX_T}")
    _decode_check_caches("decode_rope_append_multi", qkv, k_cache, v_cache, nkv, hd)
    if not _ext.use_kernels(qkv, k_cache, v_cache):
        return decode_rope_append_multi_ref(qkv, k_cache, v_cache, pos, nh, nkv, hd, rope)
    _decode_check_append_gpu("decode_rope_append_multi", qkv, k_cache, v_cache, hd, rope)
    if qkv.stride(2) != 1 or qkv.stride(0) % 8 or qkv.stride(1) % 8 or qkv.data_ptr() % 16:
        qkv = qkv.contiguous()
    return _ext.ext().decode_rope_append(qkv, k_cache, v_cache, pos, nh, *_rope_args(rope))     # 3-D: the T-token form


# --------------------------------------------------------------------------------------------
# MXFP8 K/V cache (csrc/kernels/decode_attn_mx.hip, generate(kv_cache_format="mxfp8")). K and V of
# a layer are each stored as q [B, cap, nkv, D] float8_e4m3fn and s [B, cap, nkv, D / 32] uint8
# (E8M0, bias 127): a (sequence, position, kv head) row of D elements is D / 32 MX blocks and its
# bytes are ``mx_quantize_ref(row, "e4m3")`` of the row a 16-bit cache would have stored (the
# post-RoPE K, and V, in the model dtype). A value is q * 2^(s - 127) (``_e8m0_to_f32``). No
# calibration and no state: a row's bytes depend on that row alone, so the prefill and the decode
# step write the same bytes for the same token. (D + D / 32) / 2 D = 51.6 % of the 16-bit cache.

KV_CACHE_FORMATS = ("mxfp8",)
_KV_MX_MAX_ROW = 8192        # nkv * D the append kernel stages in LDS (smdt_decode_rope_append_mx)


def _kv_mx_shapes(kq, ks, vq, vs, name):
    """(B, cap, nkv, D) of an MXFP8 cache after checking the four tensors against each other."""
    if kq.dim() != 4 or kq.shape[3] % MX_BLOCK or kq.shape[3] < MX_BLOCK:
        raise ValueError(f"{name}: the cache elements {tuple(kq.shape)} are not [B, cap, nkv, D] with D a multiple "
                         f"of {MX_BLOCK}")
    B, cap, nkv, D = kq.shape
    if vq.shape != kq.shape or tuple(ks.shape) != (B, cap, nkv, D // MX_BLOCK) or vs.shape != ks.shape:
        raise ValueError(f"{name}: k / v elements {tuple(kq.shape)} / {tuple(vq.shape)} and scales {tuple(ks.shape)} / "
                         f"{tuple(vs.shape)} are not [B, cap, nkv, D] and [B, cap, nkv, D / {MX_BLOCK}]")
    if kq.dtype != torch.float8_e4m3fn or vq.dtype != torch.float8_e4m3fn or ks.dtype != torch.uint8 \
            or vs.dtype != torch.uint8:
        raise ValueError(f"{name}: an MXFP8 cache is float8_e4m3fn elements and uint8 scales, got {kq.dtype} / "
                         f"{vq.dtype} and {ks.dtype} / {vs.dtype}")
    return B, cap, nkv, D


def kv_dequantize_mx(q, s):
    """fp32 [..., D] of MXFP8 cache rows (q [..., D] E4M3, s [..., D / 32] E8M0): q * 2^(s - 127), exact."""
    D = q.shape[-1]
    v = q.float().unflatten(-1, (D // MX_BLOCK, MX_BLOCK)) * _e8m0_to_f32(s).unsqueeze(-1)
    return v.flatten(-2)


def _kv_quantize_rows(x):
    """``mx_quantize_ref`` of rows x [..., D]: (uint8 view of the E4M3 bytes [..., D], scales [..., D / 32])."""
    D = x.shape[-1]
    q, s = mx_quantize_ref(x.reshape(-1, D), "e4m3")
    return q.view(torch.uint8).reshape(x.shape), s.reshape(*x.shape[:-1], D // MX_BLOCK)


def decode_attention_mx_supported(q, kq, ks, vq, vs) -> bool:
    """The operands decode_attn_mx.hip takes: q [B, nh, D] bf16 / fp16 against an MXFP8 cache
    (elements [B, cap, nkv, D], scales [B, cap, nkv, D / 32]), D in {64, 128}, nh / nkv in
    {1, 2, 4, 8}: the limits of ``decode_attention_supported``."""
    if q.dim() != 3 or q.dtype not in (torch.bfloat16, torch.float16):
        return False
    try:
        Bk, cap, nkv, Dk = _kv_mx_shapes(kq, ks, vq, vs, "decode_attention_mx")
    except ValueError:
        return False
    B, nh, D = q.shape
    if B != Bk or D != Dk or D not in (64, 128) or B < 1 or cap < 1 or nkv < 1 or nh % nkv:
        return False
    return nh // nkv in (1, 2, 4, 8) and B <= 65535 and nkv <= 65535


def decode_attention_mx_ref(q, kq, ks, vq, vs, lens, scale, max_len=None):
    """Torch twin of ``decode_attention_mx`` and its definition: ``decode_attention_ref`` on the
    dequantised cache (fp32, exact). Rows at or beyond ``lens[b]`` are selected out there, elements
    and scales alike."""
    _kv_mx_shapes(kq, ks, vq, vs, "decode_attention_mx")
    return decode_attention_ref(q, kv_dequantize_mx(kq, ks), kv_dequantize_mx(vq, vs), lens, scale, max_len)


def decode_attention_mx(q, kq, ks, vq, vs, lens, scale, max_len=None):
    """``decode_attention`` against an MXFP8 cache: q [B, nh, D] (bf16 / fp16), K as ``kq``
    [B, cap, nkv, D] float8_e4m3fn with ``ks`` [B, cap, nkv, D / 32] uint8, V likewise; ``lens`` and
    ``max_len`` as there. The cache is dequantised in fp32 in registers, so fp16 models are served
    too. GPU operands run decode_attn_mx.hip or raise (``decode_attention_mx_supported``); CPU
    operands run the torch twin."""
    if not _ext.use_kernels(q, kq, vq):
        return decode_attention_mx_ref(q, kq, ks, vq, vs, lens, scale, max_len)
    _kv_mx_shapes(kq, ks, vq, vs, "decode_attention_mx")
    if not decode_attention_mx_supported(q, kq, ks, vq, vs):
        raise RuntimeError(f"decode_attention_mx on the GPU needs bf16 / fp16 q [B, nh, D], an MXFP8 cache "
                           f"[B, cap, nkv, D], D in (64, 128) and nh / nkv in (1, 2, 4, 8); got q {tuple(q.shape)} "
                           f"{q.dtype}, cache {tuple(kq.shape)}")
    max_len = _decode_max_len("decode_attention_mx", max_len, kq.shape[1])
    return _ext.ext().decode_attn_mx(q.contiguous(), kq, ks, vq, vs, lens, float(scale), max_len)


def decode_rope_append_mx_ref(qkv, kq, ks, vq, vs, pos, nh, nkv, hd, rope=None):
    """Torch twin of ``decode_rope_append_mx`` and its definition: ``decode_rope_append_ref``'s q, and
    ``mx_quantize_ref`` of the k / v rows it stores (in qkv's dtype) into row pos[b]."""
    q, k, v = _decode_rope_rows(qkv, pos, nh, nkv, hd, rope)
    rows = torch.arange(qkv.shape[0], device=qkv.device)
    for x, qc, sc in ((k.to(qkv.dtype), kq, ks), (v, vq, vs)):
        qb, sb = _kv_quantize_rows(x)
        qc.view(torch.uint8)[rows, pos.long()] = qb
        sc[rows, pos.long()] = sb
    return q.contiguous()


def decode_rope_append_mx(qkv, kq, ks, vq, vs, pos, nh, nkv, hd, rope=None):
    """``decode_rope_append`` into an MXFP8 cache: q [B, nh, hd] comes back in qkv's dtype with the
    bytes ``decode_rope_append`` returns; k (rotated) and v are rounded to qkv's dtype, quantised per
    32-block (``mx_quantize_ref``) and written, elements and scale bytes, into row pos[b]. A position
    outside the cache writes nothing. GPU operands run decode_attn_mx.hip or raise; CPU operands
    run the torch twin."""
    _decode_check_qkv("decode_rope_append_mx", qkv, nh, nkv, hd)
    B, cap, ckv, D = _kv_mx_shapes(kq, ks, vq, vs, "decode_rope_append_mx")
    if (ckv, D) != (nkv, hd) or B != qkv.shape[0]:
        raise ValueError(f"decode_rope_append_mx: the cache {tuple(kq.shape)} is not [{qkv.shape[0]}, cap, {nkv}, {hd}]")
    if not _ext.use_kernels(qkv, kq, vq):
        return decode_rope_append_mx_ref(qkv, kq, ks, vq, vs, pos, nh, nkv, hd, rope)
    if qkv.dtype not in (torch.bfloat16, torch.float16) or (rope is not None and rope[2] % 16):
        raise RuntimeError(f"decode_rope_append_mx on the GPU needs bf16 / fp16 qkv and a rotary dim % 16 == 0; got "
                           f"{qkv.dtype}, rotary dim {None if rope is None else rope[2]}")
    if nkv * hd > _KV_MX_MAX_ROW:
        raise RuntimeError(f"decode_rope_append_mx: nkv * hd = {nkv * hd} exceeds {_KV_MX_MAX_ROW}, the k / v row the "
                           "kernel stages in LDS")
    return _ext.ext().decode_rope_append_mx(qkv.contiguous(), kq, ks, vq, vs, pos, nh, *_rope_args(rope))


def kv_store_mx_ref(k, v, kq, ks, vq, vs):
    """Torch twin of ``kv_store_mx``: ``mx_quantize_ref`` of every row."""
    L = k.shape[1]
    for x, qc, sc in ((k, kq, ks), (v, vq, vs)):
        qb, sb = _kv_quantize_rows(x)
        qc.view(torch.uint8)[:, :L] = qb
        sc[:, :L] = sb


def kv_store_mx(k, v, kq, ks, vq, vs):
    """The prefill store: k / v [B, L, nkv, D] (views of the post-RoPE QKV, model dtype) quantised
    row by row into rows 0 .. L - 1 of an MXFP8 cache. Not a hot path: GPU operands go through the
    ``mx_quantize`` kernel on a contiguous [B L nkv, D] copy and two strided copies per tensor; its
    bytes are the twin's."""
    B, cap, nkv, D = _kv_mx_shapes(kq, ks, vq, vs, "kv_store_mx")
    if k.dim() != 4 or k.shape != v.shape or (k.shape[0], k.shape[2], k.shape[3]) != (B, nkv, D) or k.shape[1] > cap:
        raise ValueError(f"kv_store_mx: k / v {tuple(k.shape)} / {tuple(v.shape)} do not fit the cache {tuple(kq.shape)}")
    if not _ext.use_kernels(k, v, kq):
        return kv_store_mx_ref(k, v, kq, ks, vq, vs)
    if k.dtype not in (torch.bfloat16, torch.float16) or v.dtype != k.dtype:
        raise RuntimeError(f"kv_store_mx on the GPU needs bf16 / fp16 k and v of one dtype, got {k.dtype} / {v.dtype}")
    L = k.shape[1]
    for x, qc, sc in ((k, kq, ks), (v, vq, vs)):
        qb, sb = mx_quantize(x.reshape(B * L * nkv, D), "e4m3")
        qc.view(torch.uint8)[:, :L].copy_(qb.view(torch.uint8).view(B, L, nkv, D))
        sc[:, :L].copy_(sb.view(B, L, nkv, D // MX_BLOCK))


# --------------------------------------------------------------------------------------------
# (Vocab-parallel) cross entropy


class _FusedCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, vstart, group, ignore_index, inplace_grad, vvalid):
        C = _ext.ext()
        lg = logits.contiguous()
        t = target.contiguous().view(-1)
        mx, se, tg = C.ce_stats(lg.view(-1, lg.shape[-1]), t, vstart, vvalid)
        if group is not None and torch.distributed.get_world_size(group) > 1:
            from ..comm import stats as _cs
            gmax = mx.clone()
            with _cs.blocking("all_reduce", group, 3 * gmax.numel() * gmax.element_size()):
                torch.distributed.all_reduce(gmax, op=torch.distributed.ReduceOp.MAX, group=group)
                se = se * torch.exp(mx - gmax)
                torch.distributed.all_reduce(se, group=group)
                torch.distributed.all_reduce(tg, group=group)
            mx = gmax
        loss = torch.log(se) + mx - tg
        loss = torch.where(t == ignore_index, torch.zeros_like(loss), loss)
        ctx.save_for_backward(lg, t, mx, se)
        ctx.cfg = (vstart, ignore_index, inplace_grad, vvalid)
        return loss.view(target.shape)

    @staticmethod
    def backward(ctx, dloss):
        lg, t, mx, se = ctx.saved_tensors
        vstart, ignore_index, inplace_grad, vvalid = ctx.cfg
        C = _ext.ext()
        out = lg if inplace_grad else torch.empty_like(lg)
        C.ce_bwd(lg.view(-1, lg.shape[-1]), t, mx, se, dloss.contiguous().view(-1).float(),
                 out.view(-1, lg.shape[-1]), vstart, ignore_index, vvalid)
        return out, None, None, None, None, None, None


def cross_entropy(logits, target, vocab_start: int = 0, group=None, ignore_index: int = -100,
                  inplace_grad: bool = False, vocab_size: int = 0):
    """Per-token CE loss (fp32) for logits [..., V_local] holding vocab slice
    [vocab_start, vocab_start + V_local). With ``group`` the logits are vocab-parallel and the
    three per-row statistics are all-reduced (MAX, SUM, SUM) across it.

    ``inplace_grad=True`` writes dlogits over the logits buffer (saves a [tokens, V] tensor);
    only valid when nothing else reads the logits after the loss.
    ``vocab_size`` > 0 marks global columns >= vocab_size as padding (excluded from the softmax,
    zero gradient) — HF semantics for a vocab padded to a multiple of 128.
    """
    vvalid = 0
    if vocab_size > 0:
        vvalid = min(max(int(vocab_size) - int(vocab_start), 0), logits.shape[-1])
        assert vvalid > 0, "a vocab shard holds only padding; use a smaller padding multiple"
        if vvalid == logits.shape[-1]:
            vvalid = 0
    if _ext.use_kernels(logits) and logits.shape[-1] % 8 == 0:
        return _FusedCE.apply(logits, target, int(vocab_start), group, int(ignore_index), bool(inplace_grad),
                              vvalid)
    return _ce_ref(logits, target, vocab_start, group, ignore_index, vvalid)


class _CERef(torch.autograd.Function):
    """Vocab-parallel CE in plain PyTorch (CPU path), same math as the fused kernel."""

    @staticmethod
    def forward(ctx, logits, target, vstart, group, ignore_index, vvalid=0):
        lf = logits.float()
        V = lf.shape[-1]
        if vvalid:
            lf = lf.clone()
            lf[..., vvalid:] = float("-inf")
        mx = lf.max(-1).values
        ws = 1
        if group is not None:
            ws = torch.distributed.get_world_size(group)
        if ws > 1:
            torch.distributed.all_reduce(mx, op=torch.distributed.ReduceOp.MAX, group=group)
        ex = torch.exp(lf - mx.unsqueeze(-1))
        se = ex.sum(-1)
        local = target - vstart
        inr = (local >= 0) & (local < V)
        idx = local.clamp(0, V - 1)
        tg = torch.gather(lf, -1, idx.unsqueeze(-1)).squeeze(-1) * inr
        if ws > 1:
            torch.distributed.all_reduce(se, group=group)
            torch.distributed.all_reduce(tg, group=group)
        loss = torch.log(se) + mx - tg
        ign = target == ignore_index
        loss = loss.masked_fill(ign, 0.0)
        ctx.save_for_backward(ex, se, idx, inr, ign)
        ctx.dtype = logits.dtype
        return loss

    @staticmethod
    def backward(ctx, g):
        ex, se, idx, inr, ign = ctx.saved_tensors
        p = ex / se.unsqueeze(-1)
        oh = torch.zeros_like(p).scatter_(-1, idx.unsqueeze(-1), inr.unsqueeze(-1).float())
        d = (p - oh) * g.masked_fill(ign, 0.0).unsqueeze(-1)
        return d.to(ctx.dtype), None, None, None, None, None


def _ce_ref(logits, target, vocab_start, group, ignore_index, vvalid=0):
    return _CERef.apply(logits, target, int(vocab_start), group, int(ignore_index), int(vvalid))


# --------------------------------------------------------------------------------------------
# FP8 with delayed per-tensor scaling (csrc/kernels/fp8_quant.hip). gfx950 uses the OCP encodings,
# which are torch.float8_e4m3fn / torch.float8_e5m2. Every op has a pure-torch twin (``*_ref``)
# that runs on the CPU and under SMDT_DISABLE_KERNELS=1 and is the reference of the GPU tests.

FP8_MAX = {"e4m3": 448.0, "e5m2": 57344.0}
FP8_DTYPE = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}


def fp8_quantize_ref(x, scale, amax, fmt: str, transpose: bool = False):
    xf = x.float()
    amax.copy_(torch.maximum(amax, xf.abs().max().reshape(amax.shape)))   # NaN / inf propagate
    mx = FP8_MAX[fmt]
    q = (xf * scale).clamp(-mx, mx).to(FP8_DTYPE[fmt])                    # clamp keeps NaN
    if transpose:
        return q, q.t().contiguous()
    return q


def fp8_quantize(x, scale, amax, fmt: str, transpose: bool = False):
    """q = fp8(clamp(float(x) * scale, +-max)) for x [M, K] bf16 / fp16, round-to-nearest-even, in
    ``fmt`` ("e4m3" | "e5m2"); with ``transpose`` also qt [K, M], the same bytes transposed.
    ``scale`` and ``amax`` are one-element fp32 tensors on x's device; ``amax`` is updated in place
    to max(amax, max |x|) (before scaling; a NaN / inf input leaves it non-finite)."""
    if fmt not in FP8_MAX:
        raise ValueError(f"fp8_quantize: fmt must be 'e4m3' or 'e5m2', got {fmt!r}")
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 16 or x.shape[1] % 16:
        raise ValueError(f"fp8_quantize: need x [M >= 1, K multiple of 16], got {tuple(x.shape)}")
    if x.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError(f"fp8_quantize: bf16 / fp16 input only, got {x.dtype}")
    if not _ext.use_kernels(x):
        return fp8_quantize_ref(x, scale, amax, fmt, transpose)
    out = _ext.ext().fp8_quantize(x.contiguous(), scale, amax, 0 if fmt == "e4m3" else 1, bool(transpose))
    return (out[0], out[1]) if transpose else out[0]


def fp8_update_scales_ref(scale, amax_history, amax, fmt_max, margin: int, algo: str):
    amax_history[:, 1:] = amax_history[:, :-1].clone()
    amax_history[:, 0] = amax
    amax.zero_()
    red = amax_history[:, 0] if algo == "most_recent" else amax_history.max(dim=1).values
    new = (fmt_max / red) / float(2 ** margin)
    ok = torch.isfinite(red) & (red > 0) & torch.isfinite(new)
    scale.copy_(torch.where(ok, new, scale))


def fp8_update_scales(scale, amax_history, amax, fmt_max, margin: int = 0, algo: str = "most_recent"):
    """One delayed-scaling update of a table of T FP8 tensors, in place and without a host sync:
    roll ``amax_history`` [T, H], write ``amax`` [T] into column 0 and zero it, reduce the history
    (``most_recent`` | ``max``) and set ``scale`` [T] = (fmt_max / amax) / 2^margin. A reduced amax
    of 0 or a non-finite one keeps the previous scale."""
    if algo not in ("most_recent", "max"):
        raise ValueError(f"fp8_update_scales: algo must be 'most_recent' or 'max', got {algo!r}")
    if not _ext.use_kernels(scale):
        return fp8_update_scales_ref(scale, amax_history, amax, fmt_max, int(margin), algo)
    _ext.ext().fp8_update_scales(scale, amax_history, amax, fmt_max, int(margin), algo == "max")


def fp8_gemm_ref(a, b, inv_a, inv_b, bias, out_dtype):
    acc = a.float().matmul(b.float().t()) * (inv_a * inv_b)
    if bias is not None:
        acc = acc + bias.float()
    return acc.to(out_dtype)


def fp8_gemm(a, b, inv_a, inv_b, bias=None, out_dtype=torch.bfloat16):
    """out [M, N] = (a [M, K] · b [N, K]^T) * inv_a * inv_b (+ bias), FP8 operands (E4M3 or E5M2,
    row-major), fp32 accumulation, through hipBLASLt's per-tensor-scaled FP8 GEMM
    (``torch._scaled_mm``). ``inv_a`` / ``inv_b``: one-element fp32 dequantisation factors on the
    device. A shape the library refuses raises with the shape; there is no 16-bit fallback."""
    if not _ext.use_kernels(a):
        return fp8_gemm_ref(a, b, inv_a, inv_b, bias, out_dtype)
    try:
        return torch._scaled_mm(a, b.t(), scale_a=inv_a, scale_b=inv_b, bias=bias, out_dtype=out_dtype)
    except RuntimeError as e:
        raise RuntimeError(f"fp8_gemm: the library refused M x N x K = {a.shape[0]} x {b.shape[0]} x {a.shape[1]} "
                           f"({a.dtype} x {b.dtype} -> {out_dtype}): {e}") from e


def fp8_wgrad_ref(mg, qdy, qx, inv_dy, inv_x, overwrite: bool = False):
    """Torch twin of ``fp8_wgrad``: the fp32 matmul of the dequantised operands."""
    prod = (qdy.float() * inv_dy).t().matmul(qx.float() * inv_x).view_as(mg)
    if overwrite:
        mg.copy_(prod)
    else:
        mg.add_(prod)
    return mg


def fp8_wgrad_supported(M: int, N: int, K: int) -> bool:
    """Whether the FP8 wgrad kernel takes dY [M, N] x [M, K] (M a multiple of its 64-row stage)."""
    return M > 0 and M % 64 == 0 and N >= 16 and K >= 16 and N % 16 == 0 and K % 16 == 0 and N * K < 2 ** 31


def fp8_wgrad(mg, qdy, qx, inv_dy, inv_x, overwrite: bool = False):
    """mg [N, K] fp32 (+)= (inv_dy * inv_x) * qdy [M, N]^T · qx [M, K] on FP8 bytes (qdy E5M2 or
    E4M3, qx E4M3; csrc/kernels/wgrad_fp8.hip), fp32 accumulation; ``overwrite`` stores instead of
    adding. ``inv_dy`` / ``inv_x``: one-element fp32 dequantisation factors on the device, read by
    the kernel. A shape the kernel refuses raises; there is no 16-bit fallback."""
    if not _ext.use_kernels(qdy):
        return fp8_wgrad_ref(mg, qdy, qx, inv_dy, inv_x, overwrite)
    if not _ext.ext().wgrad_fp8_grouped([mg], [qdy], [qx], [inv_dy], [inv_x], [bool(overwrite)]):
        raise RuntimeError(f"fp8_wgrad: the kernel refused M x N x K = {qdy.shape[0]} x {qdy.shape[1]} x "
                           f"{qx.shape[1]} ({qdy.dtype} x {qx.dtype} -> {mg.dtype}, M must be a multiple of 64, "
                           "N and K of 16, contiguous operands, fp32 contiguous target)")
    return mg


# --------------------------------------------------------------------------------------------
# MXFP8 (--fp8-recipe mxfp8): OCP MX block scaling, one E8M0 scale byte (bias 127) per 32 elements
# along the contraction dimension (csrc/kernels/mx_quant.hip, gemm_mx.hip). No amax table, no
# delayed scale: a block's scale comes from the block itself.

MX_BLOCK = 32
MX_EMAX = {"e4m3": 8, "e5m2": 15}    # exponent of the format's largest power of two


def _mx_check(x, fmt, columnwise, name):
    if fmt not in FP8_MAX:
        raise ValueError(f"{name}: fmt must be 'e4m3' or 'e5m2', got {fmt!r}")
    if x.dim() != 2 or x.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError(f"{name}: need a 2-D bf16 / fp16 tensor, got {tuple(x.shape)} {x.dtype}")
    R, C = x.shape
    if columnwise:
        if R < 32 or R % 32 or C < 16 or C % 16:
            raise ValueError(f"{name}: the column form needs [R multiple of 32, C multiple of 16], got {tuple(x.shape)}")
    elif R < 1 or C < 32 or C % 32:
        raise ValueError(f"{name}: the row form needs [M >= 1, K multiple of 32], got {tuple(x.shape)}")


def mx_quantize_ref(x, fmt: str, columnwise: bool = False):
    """Torch twin of ``mx_quantize`` and its definition. Per block of 32 along the last dimension
    (of x^T with ``columnwise``): a = max |v| over the finite values, e = clamp(floor(log2 a) -
    emax, -127, 127) (0 when a == 0), s = e + 127, q = fp8(clamp(v * 2^-e, +-max)), round to
    nearest even; NaN stays NaN, +-inf saturates."""
    xf = x.float()
    if columnwise:
        xf = xf.t()
    M, K = xf.shape
    b = xf.reshape(M, K // MX_BLOCK, MX_BLOCK)
    a = torch.where(torch.isfinite(b), b.abs(), torch.zeros_like(b)).amax(dim=-1)
    ex = (a.contiguous().view(torch.int32) >> 23) & 0xFF          # floor(log2 a) + 127 (0 for an fp32 subnormal)
    e = (ex - 127 - MX_EMAX[fmt]).clamp(-127, 127)
    e = torch.where(a == 0, torch.zeros_like(e), e)
    mult = ((127 - e) << 23).to(torch.int32).view(torch.float32)   # 2^-e, exact
    mx = FP8_MAX[fmt]
    q = (b * mult.unsqueeze(-1)).clamp(-mx, mx).to(FP8_DTYPE[fmt]).reshape(M, K)   # clamp keeps NaN
    return q.contiguous(), (e + 127).to(torch.uint8)


def mx_quantize(x, fmt: str, columnwise: bool = False):
    """MX quantisation of x [M, K] bf16 / fp16 (K % 32 == 0): (q [M, K] in ``fmt`` ("e4m3" |
    "e5m2"), s [M, K / 32] uint8 E8M0). With ``columnwise`` x is [R, C] (R % 32 == 0, C % 16 == 0)
    and the result is the quantisation of x^T: (qT [C, R], sT [C, R / 32]), blocks along R."""
    _mx_check(x, fmt, columnwise, "mx_quantize")
    if not _ext.use_kernels(x):
        return mx_quantize_ref(x, fmt, columnwise)
    out = _ext.ext().mx_quantize(x.contiguous(), 0 if fmt == "e4m3" else 1, not columnwise, bool(columnwise))
    return out[0], out[1]


def mx_quantize_weight_ref(w, fmt: str = "e4m3"):
    return mx_quantize_ref(w, fmt) + mx_quantize_ref(w, fmt, True)


def mx_quantize_weight(w, fmt: str = "e4m3"):
    """Both forms of a weight w [N, K] (N, K multiples of 32) from one read of it: (q [N, K],
    s [N, K / 32], qT [K, N], sT [K, N / 32]), the operands of the forward and the dgrad GEMM."""
    _mx_check(w, fmt, False, "mx_quantize_weight")
    _mx_check(w, fmt, True, "mx_quantize_weight")
    if not _ext.use_kernels(w):
        return mx_quantize_weight_ref(w, fmt)
    return tuple(_ext.ext().mx_quantize(w.contiguous(), 0 if fmt == "e4m3" else 1, True, True))


def mx_dequantize_ref(q, s):
    M, K = q.shape
    scale = torch.ldexp(torch.ones((), dtype=torch.float32, device=q.device), s.to(torch.int32) - 127)
    return (q.float().reshape(M, K // MX_BLOCK, MX_BLOCK) * scale.unsqueeze(-1)).reshape(M, K)


def mx_dequantize(q, s):
    """fp32 [M, K] = q * 2^(s - 127) per block of 32 (plain torch on every device: tests and
    references only, nothing on the training path calls it)."""
    return mx_dequantize_ref(q, s)


def gemm_mx_ref(a, sa, b, sb, bias=None, out_dtype=torch.bfloat16):
    """Torch twin of ``gemm_mx``: the fp32 matmul of the dequantised operands."""
    acc = mx_dequantize_ref(a, sa).matmul(mx_dequantize_ref(b, sb).t())
    if bias is not None:
        acc = acc + bias.float()
    return acc.to(out_dtype)


def gemm_mx_supported(M: int, N: int, K: int) -> bool:
    """Whether the block-scaled GEMM takes [M, K] x [N, K]: every extent a multiple of 128."""
    return (M > 0 and N > 0 and K > 0 and M % 128 == 0 and N % 128 == 0 and K % 128 == 0
            and M * K < 2 ** 31 and N * K < 2 ** 31 and M * N < 2 ** 31)


def gemm_mx(a, sa, b, sb, bias=None, out_dtype=torch.bfloat16, max_blocks: int = 0):
    """out [M, N] = sum_k a[m, k] 2^(sa[m, k / 32] - 127) * b[n, k] 2^(sb[n, k / 32] - 127) (+ bias)
    on gfx950's block-scaled MFMA (csrc/kernels/gemm_mx.hip): a [M, K] E4M3 or E5M2, b [N, K] E4M3,
    uint8 E8M0 scales, fp32 accumulation, bf16 / fp16 output. M, N and K must be multiples of 128
    and the operands contiguous: anything else raises with the shape; there is no fallback.
    ``max_blocks`` > 0 caps the persistent grid (tests)."""
    M, K = a.shape
    N = b.shape[0]
    shape = f"M x N x K = {M} x {N} x {K}"
    if b.shape[1] != K or not gemm_mx_supported(M, N, K):
        raise ValueError(f"gemm_mx: {shape} refused (b is {tuple(b.shape)}): M, N and K must be multiples of 128")
    if tuple(sa.shape) != (M, K // 32) or tuple(sb.shape) != (N, K // 32) or sa.dtype != torch.uint8 or sb.dtype != torch.uint8:
        raise ValueError(f"gemm_mx: {shape}: scales must be uint8 [rows, K / 32], got {tuple(sa.shape)} and {tuple(sb.shape)}")
    if not (a.is_contiguous() and b.is_contiguous() and sa.is_contiguous() and sb.is_contiguous()):
        raise ValueError(f"gemm_mx: {shape}: operands and scales must be contiguous")
    if a.dtype not in (torch.float8_e4m3fn, torch.float8_e5m2) or b.dtype != torch.float8_e4m3fn:
        raise ValueError(f"gemm_mx: {shape}: a must be E4M3 or E5M2 and b E4M3, got {a.dtype} and {b.dtype}")
    if out_dtype not in (torch.bfloat16, torch.float16):
        raise ValueError(f"gemm_mx: bf16 / fp16 output only, got {out_dtype}")
    if not _ext.use_kernels(a):
        return gemm_mx_ref(a, sa, b, sb, bias, out_dtype)
    return _ext.ext().gemm_mx(a, sa, b, sb, bias, 1 if out_dtype == torch.bfloat16 else 2, int(max_blocks))


# --------------------------------------------------------------------------------------------
# Decode linear (csrc/kernels/decode_linear.hip): y = x W^T (+ b) for the M <= 16 rows of a decode
# step, streaming W once in one of three forms: "native" (the 16-bit parameter), "mxfp8" (the row
# form of ``mx_quantize(w, "e4m3")``) and "mxfp4" (E2M1 nibbles [N, K / 2], element 2 j in the low
# nibble of byte j, E8M0 scales [N, K / 32]). The quantised forms dequantise exactly to bf16, so the
# kernel computes a bf16 linear over dequant(quant(W)) up to the summation order.

DECODE_LINEAR_FORMATS = ("native", "mxfp8", "mxfp4")
_DL_FMT = {"native": 0, "mxfp8": 1, "mxfp4": 2}
FP4_EMAX = 2                 # exponent of E2M1's largest power of two (4; the largest value is 6)
FP4_MAX = 6.0
_FP4_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def _dl_fmt(fmt):
    if fmt not in _DL_FMT:
        raise ValueError(f"decode_linear: the weight format must be one of {DECODE_LINEAR_FORMATS}, got {fmt!r}")
    return _DL_FMT[fmt]


def mx4_quantize_ref(w, name: str = "the weight"):
    """MXFP4 of w [N, K] (K % 32 == 0), the rule of ``mx_quantize_ref`` with E2M1 elements: per block
    of 32 along K, a = max |v|, e = clamp(floor(log2 a) - 2, -127, 127) (0 when a == 0), s = e + 127,
    element = RNE(v * 2^-e) on {0, .5, 1, 1.5, 2, 3, 4, 6} saturating at +-6 (ties to the even code).
    Returns (q uint8 [N, K / 2], element 2 j in the low nibble of byte j; s uint8 [N, K / 32]).
    FP4 has no NaN or Inf: a non-finite weight raises, naming ``name``. Runs on either device."""
    if w.dim() != 2 or w.shape[1] < MX_BLOCK or w.shape[1] % MX_BLOCK:
        raise ValueError(f"mx4_quantize: {name} must be [N, K multiple of 32], got {tuple(w.shape)}")
    wf = w.detach().float()
    if not bool(torch.isfinite(wf).all()):
        raise ValueError(f"mx4_quantize: {name} holds NaN or Inf, which MXFP4 (E2M1) cannot represent")
    N, K = wf.shape
    b = wf.reshape(N, K // MX_BLOCK, MX_BLOCK)
    a = b.abs().amax(dim=-1)
    ex = (a.contiguous().view(torch.int32) >> 23) & 0xFF          # floor(log2 a) + 127
    e = (ex - 127 - FP4_EMAX).clamp(-127, 127)
    e = torch.where(a == 0, torch.zeros_like(e), e)
    mult = ((127 - e) << 23).to(torch.int32).view(torch.float32)   # 2^-e, exact
    v = (b * mult.unsqueeze(-1)).abs().clamp(max=FP4_MAX)
    # torch.round is round-half-to-even; on each binade's grid an even multiple is an even code
    code = torch.where(v < 2, torch.round(v * 2), torch.where(v < 4, torch.round(v) + 2, torch.round(v / 2) + 4))
    code = code.to(torch.uint8) | (torch.signbit(b).to(torch.uint8) << 3)      # -0.0 keeps its sign
    code = code.reshape(N, K // 2, 2)
    q = code[..., 0] | (code[..., 1] << 4)
    return q.contiguous(), (e + 127).to(torch.uint8)


def _e8m0_to_f32(s):
    """2^(s - 127) of E8M0 bytes, built from the exponent field (exact on every device; 0 is the
    fp32 subnormal 2^-127, 255 the E8M0 NaN)."""
    si = s.to(torch.int32)
    bits = torch.where(si == 0, torch.full_like(si, 0x00400000), si << 23)
    bits = torch.where(si == 255, torch.full_like(si, 0x7FC00000), bits)
    return bits.view(torch.float32)


def mx4_dequantize_ref(q, s):
    """fp32 [N, K] of MXFP4 (q uint8 [N, K / 2], s uint8 [N, K / 32]): value(code) * 2^(s - 127)."""
    N, K2 = q.shape
    lut = torch.tensor(_FP4_VALUES + tuple(-x for x in _FP4_VALUES), dtype=torch.float32, device=q.device)
    codes = torch.stack((q & 0xF, q >> 4), dim=-1).reshape(N, 2 * K2)
    scale = _e8m0_to_f32(s)
    return (lut[codes.long()].reshape(N, 2 * K2 // MX_BLOCK, MX_BLOCK) * scale.unsqueeze(-1)).reshape(N, 2 * K2)


def decode_weight_quantize(w, fmt: str, name: str = "the weight"):
    """(q, scales) of a weight [N, K] in the decode format ``fmt`` ("mxfp8" | "mxfp4"). mxfp8 uses the
    ``mx_quantize`` kernel where it takes the weight and its torch twin (same bytes) elsewhere."""
    if _dl_fmt(fmt) == 0:
        raise ValueError("decode_weight_quantize: the native format has no quantised copy")
    if w.dim() != 2 or w.shape[1] < MX_BLOCK or w.shape[1] % MX_BLOCK:
        raise ValueError(f"decode_linear: {name} [{', '.join(map(str, w.shape))}] cannot take the {fmt} format: "
                         f"the input size must be a multiple of {MX_BLOCK}")
    if fmt == "mxfp4":
        return mx4_quantize_ref(w, name)
    w = w.detach()
    if _ext.use_kernels(w) and w.dtype in (torch.bfloat16, torch.float16):
        return mx_quantize(w, "e4m3")
    return mx_quantize_ref(w, "e4m3")


def decode_weight_dequantize_into(out, q, s, fmt: str):
    """``out`` [N, K] (bf16, or fp32) = the dequantised weight, computed in ``out`` itself: every
    value is exact in bf16 (a 1- or 3-bit mantissa times a power of two), so each step below is exact
    and the result equals ``decode_weight_dequantize`` cast to ``out``'s dtype. No fp32 or index
    tensor of the weight's size is built."""
    N, K = out.shape
    if fmt == "mxfp4":
        for half in (0, 1):                          # element 2 j: low nibble of byte j
            c = (q >> 4) if half else (q & 0xF)
            mag, odd = c & 7, (c & 1).to(out.dtype)
            # codes 0, 1: 0 and 0.5; codes 2 .. 7: (2 + odd) * {0.5, 1, 2}
            v = torch.where(mag < 2, odd * 0.5,
                            (2 + odd) * torch.where(mag < 4, 0.5, torch.where(mag < 6, 1.0, 2.0)).to(out.dtype))
            out[:, half::2] = torch.where(c >= 8, -v, v)
    else:
        out.copy_(q)
    out.view(N, K // MX_BLOCK, MX_BLOCK).mul_(_e8m0_to_f32(s).to(out.dtype).unsqueeze(-1))
    return out


def decode_weight_dequantize(q, s, fmt: str):
    """fp32 [N, K] of a quantised decode weight."""
    if fmt == "mxfp4":
        return mx4_dequantize_ref(q, s)
    N, K = q.shape
    return (q.float().reshape(N, K // MX_BLOCK, MX_BLOCK) * _e8m0_to_f32(s).unsqueeze(-1)).reshape(N, K)


def decode_linear_supported(M: int, N: int, K: int, dtype, fmt: str) -> bool:
    """Whether decode_linear.hip takes x [M, K] of ``dtype`` against a weight [N, K] in ``fmt``:
    the limits live in the kernel file alone (smdt_decode_linear_supported) and this asks it."""
    code = {torch.bfloat16: 1, torch.float16: 2}.get(dtype)
    if code is None or fmt not in _DL_FMT or not _ext.available():
        return False
    return bool(_ext.ext().decode_linear_supported(code, _DL_FMT[fmt], int(M), int(N), int(K)))


def decode_linear_max_m() -> int:
    """The largest M the kernel takes (0 without the extension: nothing runs on the kernel)."""
    return int(_ext.ext().decode_linear_constants()[1]) if _ext.available() else 0


def decode_linear_constants() -> dict:
    """The kernel's tiling constants: rows of W per workgroup, the largest M, the workgroup count
    below which K is split, and per format the k a workgroup covers per step and the steps per
    unrolled iteration."""
    c = [int(v) for v in _ext.ext().decode_linear_constants()]
    return {"rows": c[0], "max_m": c[1], "split_below": c[2],
            "step_k": dict(zip(DECODE_LINEAR_FORMATS, c[3:6])), "unroll": dict(zip(DECODE_LINEAR_FORMATS, c[6:9]))}


def decode_linear_plan(N: int, K: int, fmt: str):
    """(splits, slice length) of the kernel's K split for a weight [N, K]."""
    s, sl = _ext.ext().decode_linear_plan(_dl_fmt(fmt), int(N), int(K))
    return int(s), int(sl)


def decode_linear_workspace_numel(M: int, N: int, K: int, fmt: str) -> int:
    """fp32 elements of workspace ``decode_linear`` needs for this shape (0: no split)."""
    s, _ = decode_linear_plan(N, K, fmt)
    return s * int(M) * int(N) if s > 1 else 0


def decode_linear_ref(x, w, scales=None, bias=None, fmt: str = "native"):
    """Torch twin: the linear of x's dtype over the dequantised weight."""
    if _dl_fmt(fmt) != 0:
        w = decode_weight_dequantize(w, scales, fmt).to(x.dtype)
    return F.linear(x, w, bias)


def decode_linear(x, w, scales=None, bias=None, fmt: str = "native", workspace=None, out=None):
    """y [..., N] = x [..., K] W^T (+ bias) with W in ``fmt`` (see the section comment; ``scales`` for
    the quantised formats). GPU operands run decode_linear.hip or raise
    (``decode_linear_supported``); ``workspace``: fp32, at least ``decode_linear_workspace_numel``
    elements, needed when the kernel splits K; ``out``: a [M, N] tensor to write (default: a new
    one). CPU operands run the torch twin."""
    f = _dl_fmt(fmt)
    if f != 0 and scales is None:
        raise ValueError(f"decode_linear: the {fmt} format needs its scales")
    if not _ext.use_kernels(x, w):
        y = decode_linear_ref(x, w, scales, bias, fmt)
        return y if out is None else out.copy_(y.view(out.shape))
    if f != 0 and x.dtype == torch.float16:
        raise ValueError(f"decode_linear: the {fmt} format is for bf16 models: its blocks dequantise to bf16, and "
                         "fp16 cannot hold the small ones")
    K = x.shape[-1]
    M = x.numel() // K
    N = w.shape[0]
    if not decode_linear_supported(M, N, K, x.dtype, fmt):
        raise RuntimeError(f"decode_linear: the kernel does not take M x N x K = {M} x {N} x {K}, {x.dtype}, {fmt} "
                           f"(decode_linear_supported; the largest M is {decode_linear_max_m()})")
    x2 = x.reshape(M, K)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    y = _ext.ext().decode_linear(x2, w, scales, bias, f, workspace, out)
    return y.view(tuple(x.shape[:-1]) + (N,))


# --------------------------------------------------------------------------------------------
# Switch MLP without host syncs (--moe-grouped-gemm): device routing into an expert-sorted,
# tile-padded row layout, and expert GEMMs that pick their weight per 256-row tile on the device
# (csrc/kernels/moe_route.hip, gemm_tn.hip GROUPED, wgrad_gemm.hip wgrad_ranged_kernel).

MOE_TILE = 256


def moe_rows(T: int, E: int) -> int:
    """Rows of the padded layout: every expert's segment is rounded up to whole 256-row tiles."""
    return (T // MOE_TILE + E) * MOE_TILE


def moe_route_ref(logits):
    """Torch twin of ``moe_route``: the identical tables (it reads the counts on the host)."""
    T, E = logits.shape
    dev = logits.device
    R = moe_rows(T, E)
    lf = logits.float()
    top_p = torch.softmax(lf, dim=-1).max(dim=-1).values
    ar = torch.arange(E, device=dev).expand(T, E)
    top_e = torch.where(lf == lf.max(dim=-1, keepdim=True).values, ar, E).min(dim=-1).values   # lowest index of a tie
    counts = torch.bincount(top_e, minlength=E)
    rows = (counts + MOE_TILE - 1) // MOE_TILE * MOE_TILE
    start = torch.cumsum(rows, 0) - rows
    order = torch.argsort(top_e, stable=True)
    first = torch.cumsum(counts, 0) - counts                       # first sorted position of each expert
    se = top_e[order]
    dest = start[se] + (torch.arange(T, device=dev) - first[se])   # row of the i-th sorted token
    row_of_token = torch.empty(T, dtype=torch.long, device=dev)
    row_of_token[order] = dest
    token_of_row = torch.full((R,), -1, dtype=torch.long, device=dev)
    token_of_row[dest] = order
    tile_expert = torch.full((R // MOE_TILE,), -1, dtype=torch.int32, device=dev)
    for e, (s, r) in enumerate(zip(start.tolist(), rows.tolist())):
        tile_expert[s // MOE_TILE:(s + r) // MOE_TILE] = e
    seg = torch.stack([start, rows], dim=1).to(torch.int32)
    return (top_p, top_e.to(torch.int32), row_of_token.to(torch.int32), token_of_row, tile_expert, seg,
            counts.to(torch.int32))


def moe_route(logits):
    """Top-1 routing of router logits [T, E] (E <= 64) into the expert-sorted, tile-padded layout of
    ``moe_rows(T, E)`` rows, with no host sync on the kernel path. Returns (top_p fp32 [T],
    expert_of_token int32 [T], row_of_token int32 [T], token_of_row int64 [R] with -1 on pad rows,
    tile_expert int32 [R / 256] with -1 on unused tail tiles, seg int32 [E, 2] = (start, rows),
    counts int32 [E]). Tokens keep their order inside a segment; a tie goes to the lowest index.
    Not differentiable: the router's gradient flows through the caller's own softmax."""
    logits = logits.detach()
    if logits.dim() != 2 or logits.shape[1] > 64:
        raise ValueError("moe_route: logits must be [tokens, experts] with at most 64 experts")
    if not _ext.use_kernels(logits):
        return moe_route_ref(logits)
    return tuple(_ext.ext().moe_route(logits.contiguous()))


def gelu_tanh_grad_ref(z):
    """d gelu_tanh(z) / dz in fp32."""
    with torch.enable_grad():      # torch's own derivative: what autograd gives the unfused path
        zz = z.detach().float().requires_grad_(True)
        return torch.autograd.grad(F.gelu(zz, approximate="tanh").sum(), zz)[0]


def gemm_tn_grouped_ref(a, weights, tile_expert, epi=0, biases=None, aux=None, sums=False):
    """Torch twin of ``gemm_tn_grouped``, tile by tile (it reads tile_expert on the host). Unused
    tail tiles are zero here; the kernel leaves padding there that nothing reads."""
    M = a.shape[0]
    N = weights[0].shape[0]
    outs = [a.new_zeros(M, N) for _ in range(2 if epi == 2 else 1)]
    part = torch.zeros(M // 128, N, dtype=torch.float32, device=a.device) if sums else None
    for i, e in enumerate(tile_expert.tolist()):
        if e < 0:
            continue
        r = slice(i * MOE_TILE, (i + 1) * MOE_TILE)
        acc = F.linear(a[r], weights[e])
        if epi == 0:
            outs[0][r] = acc
        elif epi == 1:
            outs[0][r] = (acc.float() + biases[e].float()).to(a.dtype)
        elif epi == 2:
            outs[0][r] = acc
            outs[1][r] = F.gelu(acc.float() + biases[e].float(), approximate="tanh").to(a.dtype)
        else:
            v = acc.float() * gelu_tanh_grad_ref(aux[r].float() + biases[e].float())
            outs[0][r] = v.to(a.dtype)
            if sums:
                part[2 * i] = v[:128].sum(0)
                part[2 * i + 1] = v[128:].sum(0)
    return outs + ([part] if sums else [])


def moe_pointer_tables(weights, biases=None):
    """(btab, biastab): device tables of the experts' base pointers for ``gemm_tn_grouped``. The
    caller keeps the tensors alive and rebuilds the tables when one of them is reallocated."""
    C = _ext.ext()
    return C.ptr_table([w.detach() for w in weights]), (C.ptr_table([b.detach() for b in biases])
                                                       if biases is not None else None)


def gemm_tn_grouped(a, weights, tile_expert, epi: int = 0, biases=None, aux=None, sums: bool = False, tables=None):
    """Per 256-row tile i of a [R, K]: a_i · weights[tile_expert[i]]^T ([N, K] each) with gemm_tn's
    epilogues (0 none, 1 + bias, 2 (pre-activation, gelu_tanh(pre + bias)), 3 product *
    gelu_tanh'(aux + bias); ``sums`` with 3: also the fp32 [R / 128, N] column sums per half tile).
    The expert of a tile is read on the device; ``tables`` = ``moe_pointer_tables(weights, biases)``
    made once by the caller (built per call when None). Returns a list like ``gemm_tn``. A shape
    the kernel does not take raises."""
    if epi >= 1 and biases is None:
        raise ValueError("gemm_tn_grouped: the epilogue needs the experts' biases")
    if not _ext.use_kernels(a):
        return gemm_tn_grouped_ref(a, weights, tile_expert, epi, biases, aux, sums)
    if tables is None:
        tables = moe_pointer_tables(weights, biases)
    return _ext.ext().gemm_tn_grouped(a.contiguous(), tables[0], weights[0].shape[0], tile_expert, epi,
                                      tables[1] if epi >= 1 else None, aux, sums, 0)


def wgrad_ranged_ref(mg, dy, x, seg, expert: int, bias_grad=None, overwrite: bool = False):
    """Torch twin of the ranged wgrad: mg (+)= dy[s:s + r]^T x[s:s + r] over expert's segment
    (s, r) = seg[expert] (read on the host); an empty segment leaves mg as it is (zeros with
    ``overwrite``). Returns whether the segment held rows."""
    s, r = (int(v) for v in seg[expert].tolist())
    if r == 0:
        if overwrite:
            mg.zero_()
        return False
    prod = dy[s:s + r].t().matmul(x[s:s + r]).view_as(mg)
    if overwrite:
        mg.copy_(prod)
    else:
        mg.add_(prod)
    if bias_grad is not None:
        bias_grad.add_(dy[s:s + r].float().sum(0))
    return True


def wgrad_ranged(mg, dy, x, seg, expert: int, bias_grad=None, overwrite: bool = False):
    """mg [N, K] fp32 (+)= dy[s:s + r]^T x[s:s + r] now, (s, r) = seg[expert] read on the device
    (wgrad_gemm.hip's ranged kernel; ``bias_grad`` fp32 [N] += the column sums of that dy range).
    The queued form is ``DeferredWgrad.push(..., mrange=(seg, expert))``."""
    if not _ext.use_kernels(dy):
        wgrad_ranged_ref(mg, dy, x, seg, expert, bias_grad, overwrite)
        return mg
    bt = bias_grad if bias_grad is not None else torch.empty(0, dtype=torch.float32, device=mg.device)
    if not _ext.ext().wgrad_grouped([mg], [dy], [x], [bt], [bool(overwrite)], 0, [seg], [int(expert)]):
        raise RuntimeError(f"wgrad_ranged: the kernel refused dY {tuple(dy.shape)} x X {tuple(x.shape)} -> "
                           f"{tuple(mg.shape)} (rows a multiple of 256, 16-bit contiguous operands, fp32 target)")
    return mg
