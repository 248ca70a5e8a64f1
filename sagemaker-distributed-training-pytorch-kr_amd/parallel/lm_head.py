"""The LM head and the cross entropy as one op for an unsplit vocabulary (``LMHeadCrossEntropy``),
and the per-slice pieces the vocab-parallel form is built from (``ce_local_pass``,
``combine_ce_stats``, ``subtract_onehot_``). Owns the SMDT_LM_HEAD_CE switch.

Feature layer: built on ``dense``, no collectives. The vocab-parallel op, which all-gathers the
slice statistics over the TP group and runs on the ring linears, lives in tensor_parallel.
"""
from __future__ import annotations

import os

import torch

from .dense import _dgrad_weight_t, _wgrad, dgrad, linear_rows


class LMHeadCrossEntropy(torch.autograd.Function):
    """Per-token CE of ``h W^T`` for an unsplit vocab (TP = 1), the LM head and the loss as ONE op.

    The forward runs the logits GEMM, then ``ce_fused`` reads each logits row once and overwrites
    it with softmax - onehot (cross_entropy.hip). The backward applies the per-row dloss on the
    [tokens, hidden] side instead of the [tokens, vocab] side: dX = diag(dloss) (D W) and
    dW = D^T (diag(dloss) X), so no pass over the logits remains in the backward. Against the
    separate ce_stats / ce_bwd kernels this removes one full read of the logits per step. Same
    math as Megatron's LM head + vocab-parallel CE at TP = 1 (SURVEY K12 / K13;
    /root/reference/3_training_megatron-lm/pretrain_gpt.py:51-57).
    """

    @staticmethod
    def forward(ctx, h, weight, target, ignore_index, vvalid):
        logits = linear_rows(h, weight)
        loss = _ext_mod().ce_fused(logits.view(-1, logits.shape[-1]), target.contiguous().view(-1),
                                   int(ignore_index), int(vvalid))
        ctx.save_for_backward(h, weight, logits)
        return loss.view(target.shape)

    @staticmethod
    def backward(ctx, dloss):
        h, weight, d = ctx.saved_tensors
        dl = dloss.contiguous().view(-1, 1).float()
        gi = dgrad(d, weight, _dgrad_weight_t(weight))
        gi.view(-1, gi.shape[-1]).mul_(dl)
        hs = torch.mul(h.reshape(-1, h.shape[-1]), dl).to(h.dtype)
        dw = _wgrad(weight, d.view(-1, d.shape[-1]), hs)
        return gi, dw, None, None, None


def ce_local_pass(logits2d, target, vstart: int, vvalid: int):
    """One pass over this rank's vocab slice of the logits: overwrite them with e = exp(x - m_local)
    (0 on padding columns >= vvalid) and return the row statistics [3, rows] fp32 = (m_local,
    sum e, target logit if the target is in [vstart, vstart + vvalid) else 0). HIP kernel
    (cross_entropy.hip ce_fused_kernel<LOCAL>) on the GPU, the same math in PyTorch on the CPU."""
    if logits2d.is_cuda:
        return _ext_mod().ce_fused_local(logits2d, target, int(vstart), int(vvalid))
    V = logits2d.shape[-1]
    nv = vvalid or V
    z = logits2d.float()[:, :nv]
    m = z.max(-1).values
    e = torch.exp(z - m[:, None])
    loc = target - vstart
    inr = (loc >= 0) & (loc < nv)
    t = torch.where(inr, z.gather(1, loc.clamp(0, nv - 1)[:, None])[:, 0], torch.zeros_like(m))
    out = torch.zeros(logits2d.shape, dtype=torch.float32, device=logits2d.device)
    out[:, :nv] = e
    logits2d.copy_(out.to(logits2d.dtype))
    return torch.stack([m, e.sum(-1), t])


def combine_ce_stats(allst, st, t, ignore_index):
    """Per-row loss and softmax scale c from every rank's ``ce_local_pass`` statistics
    ``allst`` [ranks, 3, rows] (this rank's: ``st``): M = max m_r, S = sum s_r exp(m_r - M),
    loss = log S + M - x_t, c = exp(m_mine - M) / S (0 for ignored rows)."""
    M = allst[:, 0].max(0).values
    S = (allst[:, 1] * torch.exp(allst[:, 0] - M)).sum(0)
    ign = t == ignore_index
    loss = torch.where(ign, torch.zeros_like(S), torch.log(S) + M - allst[:, 2].sum(0))
    c = torch.where(ign, torch.zeros_like(S), torch.exp(st[0] - M) / S)
    return loss, c


def subtract_onehot_(l2, t, c, vstart, vvalid, ignore_index):
    """The one-hot at ONE element per row whose target lies in this slice: e[t] -= 1 / c, so that
    c e = softmax - onehot. No host sync (every row writes its clamped position; rows without an
    in-slice target write their own value back)."""
    V = l2.shape[-1]
    loc = t - vstart
    inr = (loc >= 0) & (loc < (vvalid or V)) & (t != ignore_index)
    lin = torch.arange(l2.shape[0], device=l2.device) * V + loc.clamp(0, V - 1)
    flat = l2.view(-1)
    cur = flat[lin].float()
    flat[lin] = torch.where(inr, cur - 1.0 / c, cur).to(flat.dtype)


def _ext_mod():
    from ..ops import _ext
    return _ext.ext()


def lm_head_ce_ok(h, weight, tp: int) -> bool:
    """Whether ``LMHeadCrossEntropy`` applies: HIP kernels on, TP = 1, bf16 operands, a vocab
    whose row fits one block's registers (V % 8 == 0, V <= 65536). SMDT_LM_HEAD_CE=0 disables.

    bf16 only: the backward scales the hidden rows by the per-token dloss (``h * dl`` stored in
    the 16-bit type). Under an fp16 loss scale dl ~ scale / tokens, and |h| > 1 would overflow
    fp16 at loss scales the separate CE path (dl times softmax - onehot, |.| <= 1) still takes."""
    from ..ops import _ext
    return (_LM_HEAD_CE and tp == 1 and _ext.use_kernels(h) and h.dtype == torch.bfloat16
            and weight.dtype == h.dtype and weight.shape[0] % 8 == 0 and weight.shape[0] <= 65536)


_LM_HEAD_CE = os.environ.get("SMDT_LM_HEAD_CE", "1") == "1"
