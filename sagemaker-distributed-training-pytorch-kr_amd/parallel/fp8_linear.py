"""FP8 training linears at TP = 1: delayed per-tensor scaling (``FP8State`` / ``FP8Linear``, with the
FP8 weight-gradient GEMM under --fp8-wgrad) and the block-scaled MXFP8 recipe (``MXFP8Linear``).

Owns the scaling tables and both q(W) caches (``FP8State._wq``, ``_MX_WQ``), which it registers
with ``dense.register_weight_cache``. Feature layer: built on ``dense``; it reads the parallel state
(for the amax group) and is dispatched to by tensor_parallel, which it does not import.
"""
from __future__ import annotations

import weakref

import torch
import torch.distributed as dist
import torch.nn as nn

from ..comm import loopback as _lb
from ..ops import functional as SF
from . import dense
from . import state as ps
from .dense import _bias_grad, _fire, _wgrad_and_bias, _wgrad_target

# --------------------------------------------------------------------------------------------
# FP8 linears with delayed scaling (--fp8-e4m3 / --fp8-hybrid). The forward and input-gradient
# GEMMs of a transformer layer's four linears take FP8 operands with one scale per tensor:
#   y  = dequant(q(x) · q(W)^T) + b         x, W in E4M3
#   dX = dequant(q(dY) · q(W))              dY in E5M2 (hybrid) or E4M3
# The operands are quantised by fp8_quant.hip, the GEMM is hipBLASLt's per-tensor-scaled FP8 GEMM.
# The weight gradient is what it is without FP8: the 16-bit x and dY through ``_wgrad_and_bias``
# into the fp32 main_grad. With ``FP8State.fp8_wgrad`` (--fp8-wgrad, opt-in) it takes the FP8
# operands as well:
#   dW += dequant(q(dY)^T · q(x))           wgrad_fp8.hip, fp32 accumulation into main_grad
# The forward then saves q(x) instead of the 16-bit x (scales move only after the optimizer step,
# so the saved bytes are what a re-quantise in the backward would give), the backward's one q(dY)
# feeds both the dgrad and the wgrad, and the bias gradient still comes from the 16-bit dY.
# Scales are "delayed": a quantise uses the scale the last update derived
# from earlier amax values and records its own amax for the next update, so no tensor is read
# twice and nothing syncs with the host. TP = 1 only.

_FP8_STATES: "weakref.WeakSet" = weakref.WeakSet()
_FP8_SLOTS = 3          # per linear: input, weight, output gradient


class FP8State(nn.Module):
    """The FP8 tensors of one layer stack as one table: ``scale`` [T], ``amax_history`` [T, H] and
    the current ``amax`` [T] slots, T = 3 per linear (x, W, dY). All three (and the step count the
    update interval runs on) are persistent buffers, so they travel with the model's state dict; a
    state dict without them loads as a fresh table (scales 1) with a notice.

    Scales change only in ``after_optimizer_step`` (called by the optimizer at the end of its
    step, through ``fp8_after_optimizer_step``): one ``fp8_update_scales`` launch every
    ``interval`` steps. Every micro-batch of a step and every recomputed forward therefore sees the
    same scales, and amax merges by max, so a recompute leaves the table unchanged. q(W) and
    q(W)^T are made once per optimizer step and dropped by ``params_changed()`` like the cached
    W^T of the 16-bit dgrad.

    Data parallelism: before an update the amax slots are max-reduced over the data-parallel
    (x context-parallel) group, so every replica of a weight derives the same scales from the
    global batch, the tables stay identical across ranks, and the one table a checkpoint holds is
    every rank's.

    Captured steps: the update interval is counted on the host, which a graph replay does not
    run. With ``interval`` 1 a captured step carries its own update and advances its scales on
    every replay; ``interval`` > 1 inside a capture is refused. ``step_count`` counts the eager
    calls only; it matters to the interval alone, so a replayed step loses nothing by it."""

    def __init__(self, num_linears: int, fmt: str, margin: int = 0, interval: int = 1, history_len: int = 1,
                 algo: str = "most_recent", device=None, fp8_wgrad: bool = False):
        super().__init__()
        self.fp8_wgrad = bool(fp8_wgrad)     # the weight-gradient GEMM on q(dY) / q(x) too
        if fmt not in ("e4m3", "hybrid"):
            raise ValueError(f"FP8State: fmt must be 'e4m3' or 'hybrid', got {fmt!r}")
        if algo not in ("most_recent", "max"):
            raise ValueError(f"FP8State: unknown amax algorithm {algo!r}")
        if ps.get_state().tp > 1:
            raise NotImplementedError("FP8 linears (--fp8-e4m3 / --fp8-hybrid) with --tensor-model-parallel-size > 1")
        self.fmt, self.margin, self.interval, self.algo = fmt, int(margin), max(int(interval), 1), algo
        self.grad_fmt = "e5m2" if fmt == "hybrid" else "e4m3"
        T = _FP8_SLOTS * int(num_linears)
        f32 = dict(dtype=torch.float32, device=device)
        self.register_buffer("scale", torch.ones(T, **f32))
        self.register_buffer("amax_history", torch.zeros(T, max(int(history_len), 1), **f32))
        self.register_buffer("amax", torch.zeros(T, **f32))
        self.register_buffer("step_count", torch.zeros(1, dtype=torch.int64, device=device))
        fm = torch.full((T,), SF.FP8_MAX["e4m3"], **f32)
        fm[2::_FP8_SLOTS] = SF.FP8_MAX[self.grad_fmt]
        self.register_buffer("fmt_max", fm, persistent=False)
        self.register_buffer("scale_inv", torch.ones(T, **f32), persistent=False)
        self._step = 0
        self._epoch = 0          # bumped whenever the scales may have changed: keys the q(W) cache
        self._wq: dict = {}
        _FP8_STATES.add(self)

    def _apply(self, fn, recurse=True):
        # model.to(dtype=bf16) / .half() must not touch the tables: scales and amax stay fp32
        # (the kernels take fp32 slots, and a 16-bit scale would differ from the saved one)
        keep = {n: b for n, b in self._buffers.items() if b is not None and b.dtype == torch.float32}
        super()._apply(fn, recurse)
        for n, old in keep.items():
            new = self._buffers[n]
            if new.dtype != torch.float32:
                self._buffers[n] = old.to(new.device)
        self._scales_changed()
        return self

    def reset(self):
        self.scale.fill_(1.0)
        self.scale_inv.fill_(1.0)
        self.amax_history.zero_()
        self.amax.zero_()
        self.step_count.zero_()
        self._step = 0
        self._scales_changed()

    def _scales_changed(self):
        self._epoch += 1
        self._wq.clear()

    @torch.no_grad()
    def after_optimizer_step(self):
        if self.interval > 1 and self.scale.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("FP8: --fp8-interval > 1 cannot be captured in a graph (the interval is counted on "
                               "the host and a replay would update on every step or on none); use --fp8-interval 1 "
                               "or run the step eagerly")
        self._step += 1
        if self._step % self.interval:
            return
        group = _fp8_amax_group()
        if group is not None:
            dist.all_reduce(self.amax, op=dist.ReduceOp.MAX, group=group)
        SF.fp8_update_scales(self.scale, self.amax_history, self.amax, self.fmt_max, self.margin, self.algo)
        torch.reciprocal(self.scale, out=self.scale_inv)
        self._scales_changed()

    def slot(self, t: int):
        """(scale, amax, 1 / scale) one-element views of table row ``t``."""
        return self.scale[t:t + 1], self.amax[t:t + 1], self.scale_inv[t:t + 1]

    def weight_q(self, weight, t: int):
        """(q(W) [out, in], q(W)^T [in, out]) in E4M3, made once per optimizer step."""
        key = (weight.data_ptr(), weight._version, tuple(weight.shape), weight.dtype, self._epoch)
        hit = self._wq.get(id(weight))
        if hit is not None and hit[0] == key:
            return hit[1], hit[2]
        scale, amax, _ = self.slot(t)
        with torch.no_grad():
            q, qt = SF.fp8_quantize(weight.detach(), scale, amax, "e4m3", transpose=True)
        self._wq[id(weight)] = (key, q, qt)
        return q, qt

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        self.step_count.fill_(self._step)
        super()._save_to_state_dict(destination, prefix, keep_vars)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        names = ("scale", "amax_history", "amax", "step_count")
        if not any(prefix + n in state_dict for n in names):
            if not dist.is_initialized() or dist.get_rank() == 0:
                print(f"FP8: the checkpoint holds no scaling state ({prefix}*): starting from scales 1", flush=True)
            with torch.no_grad():
                self.reset()
            return
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                                      error_msgs)
        with torch.no_grad():
            torch.reciprocal(self.scale, out=self.scale_inv)
        self._step = int(self.step_count.item())
        self._scales_changed()


def _fp8_amax_group():
    """The group over which replicas of one weight see different data (dp x cp), or None when
    there is a single replica."""
    if not dist.is_initialized():
        return None
    st = ps.get_state()
    group = getattr(st, "dp_cp_group", None) or getattr(st, "dp_group", None)
    if group is None or isinstance(group, _lb.LoopbackGroup) or dist.get_world_size(group) <= 1:
        return None
    return group


def fp8_after_optimizer_step(model):
    """Advance the FP8 tables of ``model`` (a module or a list of model chunks) by one optimizer
    step; a no-op for a model without FP8 linears."""
    if not _FP8_STATES:
        return
    for chunk in (model if isinstance(model, (list, tuple)) else [model]):
        for m in chunk.modules():
            if isinstance(m, FP8State):
                m.after_optimizer_step()


def _fp8_rows(t, what):
    t2 = t.reshape(-1, t.shape[-1])
    if not t2.is_contiguous():
        t2 = t2.contiguous()
    if t2.shape[0] % 16 or t2.shape[1] % 16:
        raise ValueError(f"FP8 linear: {what} has {t2.shape[0]} rows x {t2.shape[1]} columns; the FP8 GEMM needs "
                         "multiples of 16 in every dimension")
    return t2


class FP8Linear(torch.autograd.Function):
    """y = x W^T (+ b) at TP = 1 with FP8 forward and dgrad GEMMs (see the section comment).
    ``slot0`` is the row of x in ``state``'s table (W: + 1, dY: + 2). ``bias`` always gets its
    gradient; ``add_bias`` False leaves the addition to the caller (skip_bias_add)."""

    @staticmethod
    def forward(ctx, x, weight, bias, add_bias, state, slot0):
        ctx.state, ctx.slot0 = state, slot0
        ctx.has_bias = bias is not None
        ctx.bias_p = bias
        ctx.x_shape = x.shape
        x2 = _fp8_rows(x, "the input")
        sx, ax, ix = state.slot(slot0)
        qx = SF.fp8_quantize(x2, sx, ax, "e4m3")
        ctx.fp8_wgrad = state.fp8_wgrad
        ctx.save_for_backward(qx if state.fp8_wgrad else x, weight)
        qw, _ = state.weight_q(weight, slot0 + 1)
        y = SF.fp8_gemm(qx, qw, ix, state.slot(slot0 + 1)[2], bias if (add_bias and bias is not None) else None,
                        weight.dtype)
        return y.view(tuple(x.shape[:-1]) + (weight.shape[0],))

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        state, slot0 = ctx.state, ctx.slot0
        g2 = _fp8_rows(g, "the output gradient")
        sg, ag, ig = state.slot(slot0 + 2)
        qg = SF.fp8_quantize(g2, sg, ag, state.grad_fmt)
        _, qwt = state.weight_q(weight, slot0 + 1)
        gi = SF.fp8_gemm(qg, qwt, ig, state.slot(slot0 + 1)[2], None, weight.dtype).view(ctx.x_shape)
        bias_p = ctx.bias_p if ctx.has_bias else None
        if ctx.fp8_wgrad:        # x is q(x): the wgrad on the FP8 operands, the bias from the 16-bit dY
            dw = _fp8_wgrad(weight, qg, x, ig, state.slot(slot0)[2])
            return gi, dw, _bias_grad(bias_p, g2), None, None, None
        t2 = x.reshape(-1, x.shape[-1])
        dw, db = _wgrad_and_bias(weight, bias_p, g2, t2)
        return gi, dw, db, None, None, None


def _fp8_wgrad(weight, qg, qx, inv_dy, inv_x):
    """dW = dequant(q(dY)^T q(x)) as ``_wgrad`` does it for 16-bit operands: queued for the FP8
    grouped launch, or one launch into ``main_grad`` now, or (no main_grad) returned to autograd."""
    mg, claim = _wgrad_target(weight)
    if mg is None:
        dw = torch.empty(qg.shape[1], qx.shape[1], dtype=torch.float32, device=qg.device)
        return SF.fp8_wgrad(dw, qg, qx, inv_dy, inv_x, overwrite=True).to(weight.dtype)
    if dense.DEFERRED_WGRAD.eligible(mg, qg, qx):
        dense.DEFERRED_WGRAD.push(weight, mg, qg, qx, fresh=claim(), scales=(inv_dy, inv_x))
        return None
    SF.fp8_wgrad(weight.main_grad.view(qg.shape[1], qx.shape[1]), qg, qx, inv_dy, inv_x)
    _fire((weight,))
    return None


def attach_fp8(linears, state: FP8State):
    """Give each linear (Column / RowParallelLinear) its three rows of ``state``'s table."""
    for i, lin in enumerate(linears):
        object.__setattr__(lin, "_fp8", (state, _FP8_SLOTS * i))    # a reference, not a submodule


# --------------------------------------------------------------------------------------------
# MXFP8 linears (--fp8-recipe mxfp8): the same two GEMMs on OCP MX operands, one E8M0 scale per 32
# elements along the contraction dimension, dequantised by the matrix core (gemm_mx.hip):
#   y  = q_row(x) · q_row(W)^T + b          x, W in E4M3, blocks along `in`
#   dX = q_row(dY) · q_col(W)^T             dY in E5M2 (hybrid) or E4M3, blocks along `out`
# A block's scale comes from the block itself, so there is no table, no amax all-reduce, nothing
# after the optimizer step and nothing in the state dict; no call reads the host, so a step
# captures with no caveat. The weight gradient is the 16-bit one (``_wgrad_and_bias``), x is saved
# in 16 bits. Both forms of q(W) are made by one launch per optimizer step and dropped by
# ``params_changed()`` like the cached W^T. TP = 1 only; every extent a multiple of 128.

_MX_WQ: dict = {}


class MXFP8Recipe:
    """What ``attach_mxfp8`` hangs on a linear: the gradient format alone ("hybrid": dY in E5M2)."""

    def __init__(self, fmt: str):
        if fmt not in ("e4m3", "hybrid"):
            raise ValueError(f"MXFP8Recipe: fmt must be 'e4m3' or 'hybrid', got {fmt!r}")
        if ps.get_state().tp > 1:
            raise NotImplementedError("MXFP8 linears (--fp8-recipe mxfp8) with --tensor-model-parallel-size > 1")
        self.fmt = fmt
        self.grad_fmt = "e5m2" if fmt == "hybrid" else "e4m3"


def mx_weight_q(weight):
    """(q [out, in], s [out, in / 32], qT [in, out], sT [in, out / 32]) of W in E4M3, made once per
    optimizer step (keyed like ``FP8State.weight_q``)."""
    key = (weight.data_ptr(), weight._version, tuple(weight.shape), weight.dtype, dense.WEIGHTS_EPOCH[0])
    hit = _MX_WQ.get(id(weight))
    if hit is not None and hit[0] == key:
        return hit[1]
    with torch.no_grad():
        forms = SF.mx_quantize_weight(weight.detach())
    _MX_WQ[id(weight)] = (key, forms)
    return forms


def _mx_rows(t, what, n_other):
    t2 = t.reshape(-1, t.shape[-1])
    if not t2.is_contiguous():
        t2 = t2.contiguous()
    if not SF.gemm_mx_supported(t2.shape[0], n_other, t2.shape[1]):
        raise ValueError(f"MXFP8 linear: {what} has {t2.shape[0]} rows x {t2.shape[1]} columns against {n_other} "
                         "on the other side; the block-scaled GEMM needs multiples of 128 in every dimension")
    return t2


class MXFP8Linear(torch.autograd.Function):
    """y = x W^T (+ b) at TP = 1 with MXFP8 forward and dgrad GEMMs (see the section comment).
    ``grad_fmt``: "e5m2" | "e4m3" for dY. ``bias`` always gets its gradient; ``add_bias`` False
    leaves the addition to the caller (skip_bias_add)."""

    @staticmethod
    def forward(ctx, x, weight, bias, add_bias, grad_fmt):
        ctx.grad_fmt = grad_fmt
        ctx.has_bias = bias is not None
        ctx.bias_p = bias
        ctx.x_shape = x.shape
        x2 = _mx_rows(x, "the input", weight.shape[0])
        qx, sx = SF.mx_quantize(x2, "e4m3")
        ctx.save_for_backward(x, weight)
        qw, sw, _, _ = mx_weight_q(weight)
        y = SF.gemm_mx(qx, sx, qw, sw, bias if (add_bias and bias is not None) else None, weight.dtype)
        return y.view(tuple(x.shape[:-1]) + (weight.shape[0],))

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        g2 = _mx_rows(g, "the output gradient", weight.shape[1])
        qg, sg = SF.mx_quantize(g2, ctx.grad_fmt)
        _, _, qwt, swt = mx_weight_q(weight)
        gi = SF.gemm_mx(qg, sg, qwt, swt, None, weight.dtype).view(ctx.x_shape)
        dw, db = _wgrad_and_bias(weight, ctx.bias_p if ctx.has_bias else None, g2, x.reshape(-1, x.shape[-1]))
        return gi, dw, db, None, None


def attach_mxfp8(linears, recipe: MXFP8Recipe):
    """Make each linear (Column / RowParallelLinear) an MXFP8 linear."""
    for lin in linears:
        object.__setattr__(lin, "_fp8", (recipe, 0))


def _drop_all_q():
    for s in list(_FP8_STATES):
        s._wq.clear()
    _MX_WQ.clear()


def _drop_one_q(p):
    for s in list(_FP8_STATES):
        s._wq.pop(id(p), None)
    _MX_WQ.pop(id(p), None)


dense.register_weight_cache(_drop_all_q, _drop_one_q)
