"""Megatron-style tensor and sequence parallelism over RCCL.

Equivalent of ``megatron.core.tensor_parallel`` as exercised by the reference recipe (SURVEY P4,
P6, K7, K13, U4: Column/RowParallelLinear, VocabParallelEmbedding, broadcast_data, the async
TP all-reduce `megatron/arguments.py:837-842`, sequence parallelism `:848-849` and gradient
accumulation fusion `:850-854` in /root/reference/3_training_megatron-lm).

Design notes (MI355X-first):
  * Weight gradients are accumulated straight into the fp32 ``param.main_grad`` view of the
    contiguous DDP buffer (K7), after which the layer tells the DDP reducer the parameter is
    ready, so the bucket's RCCL all-reduce / reduce-scatter launches while backward continues.
  * The input-gradient collective (TP all-reduce, or the SP reduce-scatter) is issued
    asynchronously and overlapped with the weight-gradient GEMM.
  * Weights are initialised from a TP-invariant generator (full tensor, then this rank's shard)
    so a TP=k model starts bit-identical to the TP=1 model: this is what the parallel-equivalence
    tests rely on.
"""
from __future__ import annotations

import contextlib
import hashlib
import math
import os
from typing import Optional

import torch
import torch.distributed as dist
import torch.nn as nn
import torch.nn.functional as F

from ..comm import loopback as _lb
from ..comm import relay as _relay
from ..comm import stats as _cs
from ..ops import _ext
from ..ops import functional as SF
from . import dense
from . import lm_head as _lmh
from . import state as ps
# Layering: dense (no collectives) <- fp8_linear / decode_weights / moe_experts / lm_head <- this
# module. What moved there is re-exported by name for callers that only use it. Flags and caches are
# NOT re-exported (a rebind of a copy would change nothing): code here reads them as
# ``dense.<name>`` at call time, the wgrad queue included, so one patch of ``dense`` reaches it.
from .dense import (DEFERRED_WGRAD, DeferredWgrad, _dgrad_weight_t, _fire, _nbytes, _row_blocks,  # noqa: F401
                    _wgrad, _wgrad_and_bias, dgrad, drop_cached_weight_t, flush_deferred_wgrad,
                    gemm_tn_blocks, linear_rows, mm_rows, params_changed)
# (fp8_linear before decode_weights: the order their caches are registered and so dropped in)
from .fp8_linear import (FP8Linear, FP8State, MXFP8Linear, MXFP8Recipe, attach_fp8, attach_mxfp8,  # noqa: F401
                         mx_weight_q)
from . import decode_weights as _dw
from .decode_weights import DecodeWeights, decode_weights  # noqa: F401
from .lm_head import (LMHeadCrossEntropy, ce_local_pass, combine_ce_stats, lm_head_ce_ok,  # noqa: F401
                      subtract_onehot_)
from .moe_experts import GroupedSwitchExperts  # noqa: F401

# --------------------------------------------------------------------------------------------
# collectives helpers


def _tp_size():
    return ps.get_state().tp


def _tp_group():
    return ps.get_state().tp_group


def _all_reduce(x, group, async_op=False):
    if dist.get_world_size(group) == 1:
        return None
    if not async_op:
        eng = ps.xgmi_engine(group)  # xGMI IPC all-reduce (comm/xgmi.py) when enabled for the group
        if eng is not None and eng.use["all_reduce"] and eng.fits(x):
            with _cs.blocking("all_reduce", group, _nbytes(x), "xgmi"):
                done = eng.all_reduce(x)
            if done:
                return None
        with _cs.blocking("all_reduce", group, _nbytes(x)):
            return dist.all_reduce(x, group=group)
    h = dist.all_reduce(x, group=group, async_op=True)
    _cs.collective("all_reduce", group, _nbytes(x), work=h)
    return h


def _gather_dim0(x, group):
    ws = dist.get_world_size(group)
    if ws == 1:
        return x
    out = torch.empty((x.shape[0] * ws,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    with _cs.blocking("all_gather", group, _nbytes(out)):
        dist.all_gather_into_tensor(out, x.contiguous(), group=group)
    return out


def _reduce_scatter_dim0(x, group, async_op=False):
    ws = dist.get_world_size(group)
    if ws == 1:
        return x, None
    assert x.shape[0] % ws == 0, "sequence length must divide the TP size"
    out = torch.empty((x.shape[0] // ws,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    if not async_op:
        with _cs.blocking("reduce_scatter", group, _nbytes(x)):
            dist.reduce_scatter_tensor(out, x.contiguous(), group=group)
        return out, None
    h = dist.reduce_scatter_tensor(out, x.contiguous(), group=group, async_op=True)
    _cs.collective("reduce_scatter", group, _nbytes(x), work=h)
    return out, h


# SMDT_EXCHANGE_CU_RESERVE (dense._CU_HELD): an exchange in flight books the CUs its kernel occupies
_CU_RESERVE_ON = os.environ.get("SMDT_EXCHANGE_CU_RESERVE", "1") == "1"


def _hold_cus(works, blocks):
    if _CU_RESERVE_ON and blocks > 0:
        for w in works:
            dense._CU_HELD[id(w)] = int(blocks)


def _wait_works(works, group):
    """Wait (on the current stream) for in-flight works of ``group``'s collectives."""
    for w in works:
        dense._CU_HELD.pop(id(w), None)
    if not _cs._ON:
        for w in works:
            w.wait()
        return
    with _cs.waiting(_cs.axis_of(group)):
        for w in works:
            w.wait()


def _split_dim(x, dim, group):
    ws = dist.get_world_size(group)
    if ws == 1:
        return x
    r = dist.get_rank(group)
    return x.chunk(ws, dim=dim)[r].contiguous()


def _gather_dim(x, dim, group):
    ws = dist.get_world_size(group)
    if ws == 1:
        return x
    if dim == 0:
        return _gather_dim0(x, group)
    parts = [torch.empty_like(x) for _ in range(ws)]
    dist.all_gather(parts, x.contiguous(), group=group)
    return torch.cat(parts, dim=dim)


class _CopyToTP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        _all_reduce(g, _tp_group())
        return g


class _ReduceFromTP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        _all_reduce(x, _tp_group())
        return x

    @staticmethod
    def backward(ctx, g):
        return g


class _ScatterToTP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return _split_dim(x, -1, _tp_group())

    @staticmethod
    def backward(ctx, g):
        return _gather_dim(g, -1, _tp_group())


class _GatherFromTP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return _gather_dim(x, -1, _tp_group())

    @staticmethod
    def backward(ctx, g):
        return _split_dim(g, -1, _tp_group())


class _ScatterToSP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return _split_dim(x, 0, _tp_group())

    @staticmethod
    def backward(ctx, g):
        return _gather_dim0(g, _tp_group())


class _GatherFromSP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, tp_output_grad):
        ctx.tp_output_grad = tp_output_grad
        return _gather_dim0(x, _tp_group())

    @staticmethod
    def backward(ctx, g):
        if ctx.tp_output_grad:
            return _reduce_scatter_dim0(g, _tp_group())[0], None
        return _split_dim(g, 0, _tp_group()), None


class _ReduceScatterToSP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return _reduce_scatter_dim0(x, _tp_group())[0]

    @staticmethod
    def backward(ctx, g):
        return _gather_dim0(g, _tp_group())


def copy_to_tensor_model_parallel_region(x):
    return _CopyToTP.apply(x) if _tp_size() > 1 else x


def reduce_from_tensor_model_parallel_region(x):
    return _ReduceFromTP.apply(x) if _tp_size() > 1 else x


def scatter_to_tensor_model_parallel_region(x):
    return _ScatterToTP.apply(x) if _tp_size() > 1 else x


def gather_from_tensor_model_parallel_region(x):
    return _GatherFromTP.apply(x) if _tp_size() > 1 else x


def scatter_to_sequence_parallel_region(x):
    return _ScatterToSP.apply(x) if _tp_size() > 1 else x


def gather_from_sequence_parallel_region(x, tensor_parallel_output_grad=True):
    return _GatherFromSP.apply(x, tensor_parallel_output_grad) if _tp_size() > 1 else x


def reduce_scatter_to_sequence_parallel_region(x):
    return _ReduceScatterToSP.apply(x) if _tp_size() > 1 else x


# Exchange-wait fillers (SMDT_W_FILL=1, split-backward pipeline schedules): the W GEMMs of the last
# backward pass stay queued into the next forward, whose TP-exchange waits each issue one of them
# (``fill_exchange_wait``) beside the in-flight transfer, on the CUs the transfer leaves; the rest
# is flushed when that forward ends (train/schedules.py). VERDICT r5 item 1, "split-K W fillers".
W_FILL = os.environ.get("SMDT_W_FILL", "0") == "1"
# W GEMM time offered to one exchange wait (us): ~ the relay's 131 us per 33.6 MB chunk less the
# chunk GEMM beside it; fillers are priced at dense._FILL_PFLOPS over the CUs the exchange leaves
_FILL_STREAM_ON = os.environ.get("SMDT_W_FILL_STREAM", "1") == "1"
# on the filler stream a filler may outlast its exchange without delaying the next one: 250 us
# measured best there (profiles/r6_fill3/: 110 / 250 / 500 us), 110 us on the compute stream
_FILL_US = float(os.environ.get("SMDT_W_FILL_US", "250" if _FILL_STREAM_ON else "110"))
_FILL = {"on": False}


# SMDT_W_FILL_STREAM (default 1, above): the fillers go to a stream of their own (joined at the end
# of each pass), so a filler that outlasts its exchange no longer holds up the next exchange's start
_FILL_STREAMS = {}


def _fill_stream(dev):
    s = _FILL_STREAMS.get(dev)
    if s is None:
        s = _FILL_STREAMS[dev] = torch.cuda.Stream(dev)
    return s


def fill_exchange_wait():
    """Before a ring exchange's wait (forward or backward): issue queued W GEMMs beside the
    transfer, oldest first, up to ~_FILL_US of estimated GEMM time."""
    if not (_FILL["on"] and dense.DEFERRED_WGRAD.items):
        return
    cus = gemm_tn_blocks()
    it0 = dense.DEFERRED_WGRAD.next_fillable()
    if it0 is not None and it0.one_cuda_segment:
        if _FILL_STREAM_ON:
            dev = it0.main_grad.device
            fs = _fill_stream(dev)
            fs.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(fs):
                dense.DEFERRED_WGRAD.fill_many(_FILL_US, cus, stream=fs)
        else:
            dense.DEFERRED_WGRAD.fill_many(_FILL_US, cus)
        return
    spent = 0.0
    while spent < _FILL_US:
        it = dense.DEFERRED_WGRAD.next_fillable()
        if it is None:
            return
        spent += it.est_us(cus)
        dense.DEFERRED_WGRAD.fill_one(cus)


def join_fill_stream():
    """The compute stream waits for the filler stream; then the filled items report readiness."""
    if _FILL_STREAMS:
        for dev, fs in _FILL_STREAMS.items():
            torch.cuda.current_stream(dev).wait_stream(fs)
    if dense.DEFERRED_WGRAD.ready_after_join:
        dense.DEFERRED_WGRAD.fire_ready()


class forward_fill:
    """Context for one pass (``flush_end``: a forward) of a split-backward schedule under
    SMDT_W_FILL: exchange waits take W fillers; after a forward, whatever is left unheld is
    flushed (a backward leaves its own W queued for the next forward)."""

    def __init__(self, flush_end: bool = True):
        self.flush_end = flush_end

    def __enter__(self):
        self.prev = _FILL["on"]
        _FILL["on"] = W_FILL
        return self

    def __exit__(self, *exc):
        _FILL["on"] = self.prev
        if W_FILL:
            join_fill_stream()
            if self.flush_end:
                dense.DEFERRED_WGRAD.flush_unheld()
        return False


def accumulation_window_ok(ddps, default: bool = True) -> bool:
    """Whether gradient accumulation over these DDP wrappers may hold + merge the micro-batches'
    deferred wgrad GEMMs (DeferredWgrad.hold): the no_sync micro-batches must report no readiness
    (stage 0 / 1, or stage 2 writing its single DP rank's gradient store in place), no ZeRO-3
    partitioner, no pipeline. SMDT_WGRAD_MERGE_ACCUM=1 / 0 forces it on / off; otherwise
    ``default`` decides. It pays for small micro-batches, where every micro-batch's wgrad is a
    short K-loop plus a full fp32 main_grad read-modify-write (LLaMA-7B at ~500 tokens: +12 %,
    profiles/r3_merge/), and costs for large ones, where the segment concatenation outweighs the
    saved main_grad traffic (GPT-2 small at 12,288 tokens per micro-batch: 75.5 vs 63.2 ms,
    profiles/r3_l4l/) — so the SFT engine defaults it on and the Megatron schedule off."""
    env = os.environ.get("SMDT_WGRAD_MERGE_ACCUM")
    if (env == "0" or (env is None and not default)) or not dense.DEFERRED_WGRAD.enabled:
        return False
    if ps.get_state().pp != 1:
        return False
    for d in ddps:
        if getattr(d, "zero3", None) is not None:
            return False
        if getattr(d, "zero_stage", 0) >= 2 and not getattr(d, "_direct", False):
            return False
    return True


# The QKV and fc1 bias gradients from the kernels that PRODUCE those linears' dY: the flash
# attention backward (flash_attn.hip SUMS: token sums of the fp32 dQ | dK | dV) and the fc2 dgrad's
# GeLU-backward epilogue (gemm_tn.hip SUMS), each followed by the fixed-order column-sum kernel
# straight into the bias' fp32 main_grad. SMDT_BIAS_FROM_PRODUCER=0 restores the wgrad bias tiles.
_BIAS_FROM_PRODUCER = os.environ.get("SMDT_BIAS_FROM_PRODUCER", "1") == "1"


def bias_from_producer(bias_p, like) -> bool:
    """Whether the kernel that writes a linear's dY (16-bit ``like``-typed, on its device) may
    also make the linear's bias gradient: TP = 1 without sequence parallelism, a bias with a plain
    fp32 ``main_grad`` and a readiness callback (not the lazily zeroed ZeRO-2 slices, whose first
    write is a store the wgrad queue owns), and no accumulation window / sub-batch merge / split
    backward of the wgrad queue (those report a parameter's readiness once per window). The caller
    checks that its producer kernel really runs."""
    if not _BIAS_FROM_PRODUCER or bias_p is None or not like.is_cuda or not _ext.use_kernels(like):
        return False
    if like.dtype not in (torch.bfloat16, torch.float16):
        return False
    if _tp_size() != 1 or isinstance(getattr(type(bias_p), "main_grad", None), property):
        return False
    q = dense.DEFERRED_WGRAD
    if q.hold or q.merge_repeats or q.defer:
        return False
    tgt = SF.grad_accumulate_target(bias_p)
    return tgt is not None and tgt.device == like.device and tgt.numel() == bias_p.numel()


def dgrad_into(dst, g, weight, wt=None):
    """dst[...] = g @ weight written in place."""
    if wt is None:
        torch.matmul(g, weight, out=dst)
    else:
        _mm_into(dst, g, wt)


# --------------------------------------------------------------------------------------------
# Linear with async grad communication + fused fp32 wgrad accumulation (K7, dense.py)


class LinearWithGradAccumulationAndAsyncCommunication(torch.autograd.Function):
    """y = x W^T (+ b) with Megatron's backward schedule:

    dgrad GEMM -> launch (async) TP all-reduce or SP reduce-scatter of dgrad -> wgrad GEMM into
    fp32 main_grad -> wait. With ``sequence_parallel`` the input is all-gathered along the
    sequence dim in forward (and re-gathered in backward, saving memory).
    """

    @staticmethod
    def forward(ctx, x, weight, bias, sequence_parallel, async_grad_allreduce, add_bias=True, bias_grad=True):
        ctx.sp = sequence_parallel
        ctx.async_ar = async_grad_allreduce
        # bias_grad False: the consumer of this linear's output makes the bias gradient
        # (``bias_from_producer``); the backward then produces the weight gradient alone
        ctx.has_bias = bias is not None and bias_grad
        ctx.bias_p = bias
        ctx.save_for_backward(x, weight)
        total = _gather_dim0(x, _tp_group()) if sequence_parallel else x
        # add_bias False: the caller adds the bias later (skip_bias_add) and this function only
        # produces its gradient (the column sums of dY) beside the weight gradient
        return linear_rows(total, weight, bias if add_bias else None)

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        gi_out, dw, db = _linear_backward(ctx, g, x, weight)
        return gi_out, dw, db, None, None, None, None


def _linear_backward(ctx, g, x, weight):
    """dgrad -> async TP all-reduce / SP reduce-scatter of it -> wgrad (+ bias grad) into the fp32
    main_grad -> wait: the backward of ``LinearWithGradAccumulationAndAsyncCommunication`` (ctx
    carries sp, async_ar, has_bias, bias_p)."""
    group = _tp_group()
    tp = dist.get_world_size(group) if group is not None else 1
    total = _gather_dim0(x, group) if (ctx.sp and tp > 1) else x
    g = g.contiguous()
    gi = dgrad(g, weight, _dgrad_weight_t(weight))
    handle = None
    if ctx.sp and tp > 1:
        gi_out, handle = _reduce_scatter_dim0(gi, group, async_op=True)
    else:
        gi_out = gi
        if ctx.async_ar and tp > 1:
            handle = _all_reduce(gi_out, group, async_op=True)
    g2 = g.reshape(-1, g.shape[-1])
    t2 = total.reshape(-1, total.shape[-1])
    dw, db = _wgrad_and_bias(weight, ctx.bias_p if ctx.has_bias else None, g2, t2)
    if handle is not None:
        # the collective is in flight: run the queued weight-gradient GEMMs beside it
        dense.DEFERRED_WGRAD.flush_opportunistic()
        _wait_works([handle], group)
    return gi_out, dw, db


# fc1 + bias + GeLU(tanh) as ONE GEMM launch (gemm_tn.hip EPI_BIAS_GELU): the epilogue writes the
# pre-activation (kept for the backward) and the activation; the separate bias_act_fwd pass over
# the [tokens, 4h] tensor is gone (Megatron's bias_gelu_fusion,
# /root/reference/3_training_megatron-lm/megatron/arguments.py:819-821); at TP = 1 the backward's
# GeLU half goes into the fc2 dgrad's epilogue as well (FusedGeLUMLP). On by default: the GPT-2
# 345M step measured 160.45 / 161.06 / 160.64 ms against 160.67 / 160.68 / 161.01 ms unfused (one
# box, interleaved; profiles/r5_gemm_tn/) — the fused ops are 1.02x / 1.05x the library GEMM +
# elementwise pass, the hand-written GEMM itself 0.85-0.92x hipBLASLt. SMDT_FUSED_BIAS_GELU=0 off.
_FUSED_BIAS_GELU = os.environ.get("SMDT_FUSED_BIAS_GELU", "1") == "1"


class LinearBiasGeLU(torch.autograd.Function):
    """act = gelu_tanh(x W^T + b) for a column-parallel fc1 without sequence parallelism. Backward:
    d(pre) = bias_act_bwd(d(act), pre) (the bias gradient comes from the wgrad launch, as for
    ``ColumnParallelLinear(bias_grad_from_output=True)``), then the linear's own backward."""

    @staticmethod
    def forward(ctx, x, weight, bias, async_grad_allreduce):
        ctx.sp = False
        ctx.async_ar = async_grad_allreduce
        ctx.has_bias = True
        ctx.bias_p = bias
        x2 = x.reshape(-1, x.shape[-1])
        pre, act = _ext.ext().gemm_tn(x2, weight, 2, bias)
        ctx.save_for_backward(x, weight, pre)
        shape = tuple(x.shape[:-1]) + (weight.shape[0],)
        return act.view(shape)

    @staticmethod
    def backward(ctx, dact):
        x, weight, pre = ctx.saved_tensors
        d2 = dact.reshape(-1, dact.shape[-1]).contiguous()
        dpre = _ext.ext().bias_act_bwd(d2, pre, ctx.bias_p.detach(), 0, False, None)[0]
        gi, dw, db = _linear_backward(ctx, dpre.view(tuple(x.shape[:-1]) + (weight.shape[0],)), x, weight)
        return gi, dw, db, None


class FusedGeLUMLP(torch.autograd.Function):
    """fc2(gelu_tanh(fc1(x) + b1)) at TP = 1 with both GeLU halves inside the GEMMs (gemm_tn.hip):
    forward fc1 + bias + GeLU in one launch (EPI_BIAS_GELU), backward fc2's dgrad with the GeLU
    backward in its epilogue (EPI_DGELU: d(pre) = (dY W2) * gelu'(pre + b1), the [tokens, 4h]
    d(activation) is never written). Saves x, pre and act — what the unfused path saves. fc2's bias
    is added by the caller (skip_bias_add), as in ``ParallelMLP``. Same math as Megatron's
    ParallelMLP with bias_gelu_fusion (/root/reference/3_training_megatron-lm/megatron/
    arguments.py:819-821)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2):
        C = _ext.ext()
        x2 = x.reshape(-1, x.shape[-1])
        pre, act = C.gemm_tn(x2, w1, 2, b1)
        y = linear_rows(act, w2)
        ctx.save_for_backward(x, w1, w2, pre, act)
        ctx.b1 = b1
        return y.view(tuple(x.shape[:-1]) + (w2.shape[0],))

    @staticmethod
    def backward(ctx, dy):
        x, w1, w2, pre, act = ctx.saved_tensors
        C = _ext.ext()
        b1 = ctx.b1
        dy2 = dy.reshape(-1, dy.shape[-1]).contiguous()
        w2t = _dgrad_weight_t(w2)
        b1_grad = b1      # who still owes fc1's bias gradient: the wgrad launch, unless the epilogue makes it
        if w2t is not None and C.gemm_tn_supported(dy2, w2t):
            if bias_from_producer(b1, dy2):
                # d(pre) and its column sums (fc1's bias gradient, straight into main_grad) from
                # the one epilogue; fc1's weight gradient is then queued without bias tiles
                dz = C.gemm_tn_dgelu_dbias(dy2, w2t, b1.detach(), pre, SF.grad_accumulate_target(b1), True)
                b1._smdt_grad_ready(b1)
                b1_grad = None
            else:
                dz = C.gemm_tn(dy2, w2t, 3, b1.detach(), None, None, 0, 0, pre)[0]
        else:
            dz = C.bias_act_bwd(dgrad(dy2, w2, w2t).contiguous(), pre, b1.detach(), 0, False, None)[0]
        dw2, _ = _wgrad_and_bias(w2, None, dy2, act)
        x2 = x.reshape(-1, x.shape[-1])
        dx = dgrad(dz, w1, _dgrad_weight_t(w1))
        dw1, db1 = _wgrad_and_bias(w1, b1_grad, dz, x2)
        return dx.view(x.shape), dw1, db1, dw2


def fused_gelu_mlp_ok(x, mlp) -> bool:
    """``FusedGeLUMLP`` applies: the fc1 + bias-GeLU conditions, TP = 1, fc2 without sequence
    parallelism and with its bias left to the caller."""
    return (_tp_size() == 1 and linear_bias_gelu_ok(x, mlp.fc1) and mlp.fc2.skip_bias_add
            and not mlp.fc2.sequence_parallel and mlp.fc2.weight.dtype == x.dtype)


class SPFusedGeLUMLP(torch.autograd.Function):
    """The sequence-parallel MLP of a TP > 1 rank with both GeLU halves inside the ring-chunk GEMMs
    (the TP form of ``FusedGeLUMLP``; BASELINE config 3's tp2 + SP layers):

      forward   fc1: ring all-gather of the SP chunks of x, each chunk's GEMM with the bias-GeLU
                epilogue (gemm_tn EPI_BIAS_GELU) writing its rows of the pre-activation and the
                activation; fc2: per-chunk GEMMs fused with the ring reduce-scatter (as
                ``_RowSPLinear``);
      backward  fc2: ring all-gather of dY, each chunk's dgrad with the GeLU backward in its
                epilogue (EPI_DGELU) writing d(pre) directly — the [tokens, 4h / tp] d(activation)
                and the separate bias_act_bwd pass are gone; fc1: dgrad chunks fused with the ring
                reduce-scatter, the fc1 weight and bias gradients (one grouped-wgrad pass over
                d(pre)) drained while the last chunk is in flight (as ``_ColumnSPLinear``).

    The collectives, their order and the saved tensors (gathered x, pre, act) are those of the
    unfused column / row SP linears, so a TP group whose ranks disagree on the gate could not
    deadlock on the exchanges either (the gate depends on shapes and dtypes only). Megatron's
    ParallelMLP with bias_gelu_fusion + sequence_parallel (/root/reference/3_training_megatron-lm/
    megatron/arguments.py:819-821, 848-849)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2):
        C = _ext.ext()
        group = _tp_group()
        x = x.contiguous()
        n = x.shape[0]
        ws = dist.get_world_size(group)
        lead = (n * ws,) + tuple(x.shape[1:-1])
        f = w1.shape[0]
        pre = x.new_empty(lead + (f,))
        act = x.new_empty(lead + (f,))

        def fc1_chunk(lo, ch):
            m = ch.shape[0]
            C.gemm_tn(ch.reshape(-1, ch.shape[-1]), w1, 2, b1, pre[lo:lo + m].view(-1, f),
                      act[lo:lo + m].view(-1, f), gemm_tn_blocks())
        total = ag_ring(x, group, fc1_chunk)
        y = rs_ring(lambda lo, m, o: _linear_into(act[lo:lo + m], w2, o), group, lead + (w2.shape[0],), act)
        ctx.save_for_backward(total, w1, w2, pre, act)
        ctx.b1 = b1
        ctx.bulk = _SPLIT["on"]     # a sub-batch half: bulk rings in backward
        ctx.defer_add = _bwd_add_to_norm(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        total, w1, w2, pre, act = ctx.saved_tensors
        C = _ext.ext()
        group = _tp_group()
        b1 = ctx.b1
        dy = dy.contiguous()
        f = w1.shape[0]
        dz = pre.new_empty(pre.shape)
        d2 = dz.view(-1, f)
        w2t = _dgrad_weight_t(w2)
        bd = b1.detach()

        def fc2_dgrad_chunk(lo, ch):
            m = ch.shape[0]
            C.gemm_tn(ch.reshape(-1, ch.shape[-1]), w2t, 3, bd, dz[lo:lo + m].view(-1, f), None,
                      gemm_tn_blocks(), 0, pre[lo:lo + m].view(-1, f))
        gfull = ag_ring(dy, group, fc2_dgrad_chunk, before_last_wait=_flush_wgrad, bulk=ctx.bulk)
        dw2 = _wgrad(w2, gfull.reshape(-1, gfull.shape[-1]), act.reshape(-1, f))
        res = {}

        def wgrad():
            res["dw"], res["db"] = _wgrad_and_bias(w1, b1, d2, total.reshape(-1, total.shape[-1]))
            _flush_wgrad()
        w1t = _dgrad_weight_t(w1)
        dx = rs_ring(lambda lo, m, o: _dgrad_rows(dz[lo:lo + m], w1, w1t, o), group,
                     dz.shape[:-1] + (w1.shape[1],), dz, wgrad, bulk=ctx.bulk, defer_add=ctx.defer_add)
        if "dw" not in res:
            wgrad()
        return dx, res["dw"], res["db"], dw2


def sp_fused_gelu_mlp_ok(x, mlp) -> bool:
    """``SPFusedGeLUMLP`` applies: TP > 1 with the ring collective-matmul sequence-parallel linears,
    fc1 with a bias and fc2 with its bias left to the caller, 16-bit CUDA operands, and every chunk
    GEMM on a gemm_tn shape (SP-chunk rows and the local 4h a multiple of 256, h of 128).
    Depends on shapes / dtypes / flags only, so every rank of the TP group decides alike."""
    fc1, fc2 = mlp.fc1, mlp.fc2
    if not (_FUSED_BIAS_GELU and _TP_OVERLAP and _tp_size() > 1 and x.is_cuda and fc1.sequence_parallel
            and fc2.sequence_parallel and fc1.bias is not None and fc1.bias_grad_from_output
            and fc2.skip_bias_add and not fc1.gather_output and x.dtype in (torch.bfloat16, torch.float16)
            and fc1.weight.dtype == x.dtype and fc2.weight.dtype == x.dtype and fc1.bias.dtype == x.dtype
            and _ext.use_kernels(x)):
        return False
    if _direct(_tp_group()) is not None:   # the direct TP4 / TP8 engine hands over row pieces
        return False
    rows = x.numel() // x.shape[-1]
    f, h = fc1.weight.shape
    return (rows % 256 == 0 and f % 256 == 0 and h % 128 == 0 and fc2.weight.shape == (h, f)
            and _fills_chip(rows, f) and bool(_ext.ext().gemm_tn_supported(x.reshape(rows, h), fc1.weight)))


def _fills_chip(rows: int, n: int) -> bool:
    """A chunk GEMM of rows x n has at least one 256 x 256 output tile per CU: gemm_tn's
    persistent grid is one workgroup per tile up to the CU count, so fewer tiles leave CUs idle
    (GPT-3 6.7B tp4 + SP: 2048-row chunks x 4096 = 128 tiles -> the stage rank 426 ms with the
    fused MLP vs 394 ms on hipBLASLt, profiles/r6_ab/)."""
    if not dense._NUM_CUS:
        dense._NUM_CUS.append(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)
    return (rows // 256) * (n // 256) >= dense._NUM_CUS[0]


def linear_bias_gelu_ok(x, layer) -> bool:
    """The fused fc1 + bias + GeLU path applies: CUDA, 16-bit, no sequence parallelism, a bias, and
    a shape gemm_tn supports."""
    if not (_FUSED_BIAS_GELU and x.is_cuda and layer.bias is not None and not layer.sequence_parallel
            and x.dtype in (torch.bfloat16, torch.float16) and layer.weight.dtype == x.dtype
            and layer.bias.dtype == x.dtype and x.is_contiguous() and not layer.gather_output
            and _ext.use_kernels(x)):
        return False
    x2 = x.view(-1, x.shape[-1])
    return _fills_chip(x2.shape[0], layer.weight.shape[0]) and bool(_ext.ext().gemm_tn_supported(x2, layer.weight))


def linear_bias_gelu(x, layer):
    """gelu_tanh(fc1(x) + b) through ``LinearBiasGeLU`` (call only when ``linear_bias_gelu_ok``)."""
    if not layer.async_ar:
        x = copy_to_tensor_model_parallel_region(x)
    return LinearBiasGeLU.apply(x, layer.weight, layer.bias, layer.async_ar)


class VocabParallelLMHeadCE(torch.autograd.Function):
    """LM head + CE for a vocabulary split over the TP group (TP > 1), the LM-head GEMM and the loss
    as ONE op with a single pass over this rank's [tokens, V / tp] logits (the
    TP = 1 form is ``LMHeadCrossEntropy``). Same math as Megatron's parallel_lm_logits +
    vocab-parallel CE (/root/reference/3_training_megatron-lm/pretrain_gpt.py:51-57;
    megatron/arguments.py:992-994):

    * logits = X W_r^T — with sequence parallelism through the ring all-gather collective-matmul
      (``_ColumnSPLinear``'s forward);
    * ``ce_local_pass`` overwrites them with e = exp(x - m_r) and returns (m_r, s_r, x_t) per row;
    * ONE all-gather of those [3, tokens] statistics replaces the three all-reduces (MAX, SUM,
      SUM): M = max m_r, S = sum s_r exp(m_r - M), loss = log S + M - x_t;
    * with the row scale c = exp(m_r - M) / S, softmax = c e, so the one-hot is subtracted at ONE
      element per row: e[t] -= 1 / c (no second pass);
    * backward: D = c e - onehot never exists — the per-row c dloss goes on the [tokens, hidden]
      side: dX = diag(c dl) (E W) (reduce-scattered along the sequence by the ring, or all-reduced
      without SP) and dW = E^T diag(c dl) X.

    Against logits -> separate stats kernel -> 3 all-reduces -> backward kernel over the logits,
    this drops one full read of the logits per micro-batch on the last pipeline stage.
    bf16 only (the hidden-side scaling, see ``lm_head_ce_ok``)."""

    @staticmethod
    def forward(ctx, x, weight, target, ignore_index, vstart, vvalid, sp):
        group = _tp_group()
        ws = dist.get_world_size(group)
        x = x.contiguous()
        if sp:
            n = x.shape[0]
            logits = x.new_empty((n * ws,) + tuple(x.shape[1:-1]) + (weight.shape[0],))
            total = ag_ring(x, group, lambda lo, ch: _mm_into(logits[lo:lo + ch.shape[0]], ch, weight))
        else:
            n = x.shape[0] // ws
            total = x
            logits = linear_rows(x, weight)
        V = logits.shape[-1]
        l2 = logits.view(-1, V)
        t = target.contiguous().view(-1)
        st = ce_local_pass(l2, t, vstart, vvalid).contiguous()
        allst = st.new_empty((ws,) + tuple(st.shape))
        if ws > 1:
            from ..comm import stats as _cs
            with _cs.blocking("all_gather", group, allst.numel() * allst.element_size()):
                dist.all_gather_into_tensor(allst.view(-1), st.view(-1), group=group)
        else:
            allst[0].copy_(st)
        loss, c = combine_ce_stats(allst, st, t, ignore_index)
        subtract_onehot_(l2, t, c, vstart, vvalid, ignore_index)
        ctx.save_for_backward(total, weight, logits, c)
        ctx.sp, ctx.n = sp, n
        return loss.view(target.shape)

    @staticmethod
    def backward(ctx, dloss):
        total, weight, e, c = ctx.saved_tensors
        group = _tp_group()
        n = ctx.n
        r = dloss.contiguous().view(-1).float() * c          # per-row scale of E = c dl
        r3 = r.view(e.shape[:-1] + (1,))
        wt = _dgrad_weight_t(weight)
        res = {}

        def wgrad():
            H = total.shape[-1]
            hs = torch.mul(total.reshape(-1, H), r.view(-1, 1)).to(total.dtype)
            res["dw"] = _wgrad(weight, e.view(-1, e.shape[-1]), hs)
            _flush_wgrad()

        def part(lo, m, o):
            g = _dgrad_rows(e[lo:lo + m], weight, wt, o)
            g.mul_(r3[lo:lo + m])
            return g
        if ctx.sp:
            gi = rs_ring(part, group, e.shape[:-1] + (weight.shape[1],), e, wgrad)
        else:
            gi = dgrad(e, weight, wt)
            gi.mul_(r3)
            h = dist.all_reduce(gi, group=group, async_op=True) if dist.get_world_size(group) > 1 else None
            wgrad()
            if h is not None:
                h.wait()
        if "dw" not in res:
            wgrad()
        return gi, res["dw"], None, None, None, None, None


def vp_lm_head_ce_ok(h, weight, tp: int) -> bool:
    """Whether ``VocabParallelLMHeadCE`` applies: TP > 1, HIP kernels on and bf16 operands (or the
    CPU reference with SMDT_LM_HEAD_CE_CPU=1, for the Gloo equivalence tests), a vocab slice whose
    row fits one block's registers (V / tp % 8 == 0, <= 65536). SMDT_LM_HEAD_CE=0 disables."""
    from ..ops import _ext
    if not (_lmh._LM_HEAD_CE and tp > 1 and weight.shape[0] % 8 == 0 and weight.shape[0] <= 65536
            and weight.dtype == h.dtype):
        return False
    if h.is_cuda:
        return _ext.use_kernels(h) and h.dtype == torch.bfloat16
    return os.environ.get("SMDT_LM_HEAD_CE_CPU", "0") == "1"


def linear_with_grad_accumulation_and_async_allreduce(x, weight, bias, sequence_parallel=False,
                                                      async_grad_allreduce=False, add_bias=True, fp8=None,
                                                      bias_grad=True):
    if _dw._DECODE["state"] is not None:    # generate(weight_format=...): unsharded, no gradients
        return _dw._decode_route(_dw._DECODE["state"], x, weight, bias, add_bias, fp8)
    if not bias_grad and (fp8 is not None or sequence_parallel):
        raise RuntimeError("bias_grad=False (the bias gradient from the consumer's kernel) is for the plain "
                           "16-bit linear at TP = 1")
    if fp8 is not None and isinstance(fp8[0], MXFP8Recipe):     # from attach_mxfp8; TP = 1
        return MXFP8Linear.apply(x, weight, bias, add_bias, fp8[0].grad_fmt)
    if fp8 is not None:                 # (FP8State, first table row) from attach_fp8; TP = 1
        return FP8Linear.apply(x, weight, bias, add_bias, fp8[0], fp8[1])
    if sequence_parallel and _TP_OVERLAP and _tp_size() > 1:
        return _ColumnSPLinear.apply(x, weight, bias, add_bias)
    return LinearWithGradAccumulationAndAsyncCommunication.apply(x, weight, bias, sequence_parallel,
                                                                 async_grad_allreduce, add_bias, bias_grad)


# --------------------------------------------------------------------------------------------
# Sequence-parallel linears with the TP collective fused into the GEMM as a ring (collective
# matmul): the all-gather / reduce-scatter moves one sequence chunk per step over RCCL p2p while
# the GEMM of the previous / next chunk runs, instead of a monolithic collective followed by a
# monolithic GEMM. On MI355X the TP pair talks over ONE xGMI link (~64-77 GB/s per direction),
# which at GPT-2 345M shapes moves a layer's activations slower than the MFMA cores consume them,
# so every byte in flight must have a GEMM beside it. Backward collectives additionally drain the
# deferred weight-gradient queue before they are waited for (Megatron's "launch dgrad collective
# -> wgrad GEMM -> wait", arguments.py:837-842, with the grouped MFMA wgrad as the overlapped work).

_TP_OVERLAP = os.environ.get("SMDT_TP_OVERLAP", "1") == "1"
_LB_RING_ASYNC = os.environ.get("SMDT_LOOPBACK_RING_ASYNC", "0") == "1"


def _ring(group):
    ws = dist.get_world_size(group)
    r = dist.get_rank(group)
    ranks = dist.get_process_group_ranks(group)
    return ws, r, ranks[(r + 1) % ws], ranks[(r - 1) % ws]


def _exchange(send, recv, nxt, prv, group):
    """One ring step: send to next and receive from prev in ONE p2p group (matched per peer in
    issue order, so a 2-rank ring with next == prev cannot deadlock). A 2-rank ring on an
    MI355X node goes over every xGMI link through the relay engine (comm/relay.py) when one was
    built for ``group`` and measured faster than RCCL's single-link p2p."""
    if _lb.is_loopback(group):
        # single-process TP emulation: the transfer as a local copy on the compute stream (issuing
        # it on the loopback side stream, as the real exchange runs beside the chunk GEMM, measured
        # SLOWER: 202.4 -> 219.7 ms per stage-1 rank, the per-exchange stream hand-offs cost more
        # than the overlap gains; profiles/r4_loopback_ring_async_neg/). SMDT_LOOPBACK_RING_ASYNC=1
        # re-runs that arm (the side stream is now a high-priority one).
        standin = _lb.link_standin() if send.is_cuda else None
        if standin is not None:
            # paced link stand-in (SMDT_LINK_STANDIN): the modelled link time and the relay's CU
            # footprint, on the side stream beside the rank's compute, waited for like the relay
            gbps, blocks = standin
            ns = int(_nbytes(send) / gbps)          # bytes / (GB/s) = ns
            C = _ext.ext()
            SPLIT_STATS["standin_exchanges"] = SPLIT_STATS.get("standin_exchanges", 0) + 1
            works = [group._issue([send, recv], lambda: C.paced_copy(recv, send, blocks, ns), [recv])]
            _hold_cus(works, blocks)
            return works
        if _LB_RING_ASYNC and send.is_cuda:
            return [group._issue([send, recv], lambda: recv.copy_(send), [recv])]
        recv.copy_(send)
        return []
    if nxt == prv:
        eng = _relay.engine_for(group)
        if eng is not None:
            h = eng.exchange_async(send, recv)
            if h is not None:
                _cs.collective("p2p", group, _nbytes(send), transport="relay", events=h.timing())
                _hold_cus([h], eng.cu_blocks())
                return [h]
    if send.is_cuda and dist.get_backend(group) == "gloo":
        # Gloo rehearsals with CUDA tensors (several ranks on one GPU, SMDT_BENCH_BACKEND=gloo):
        # a rank that sends to and receives from the same peer at once never completes its
        # receive (both ranks of a tp2 ring stalled in the first wait, profiles/r4_rehearse_tp2/);
        # the exchange goes through host buffers, synchronously. RCCL runs never take this path.
        s_cpu = send.detach().cpu()
        r_cpu = torch.empty(recv.shape, dtype=recv.dtype)
        for w in dist.batch_isend_irecv([dist.P2POp(dist.isend, s_cpu, nxt, group),
                                         dist.P2POp(dist.irecv, r_cpu, prv, group)]):
            w.wait()
        recv.copy_(r_cpu)
        return []
    works = dist.batch_isend_irecv([dist.P2POp(dist.isend, send, nxt, group),
                                    dist.P2POp(dist.irecv, recv, prv, group)])
    _cs.collective("p2p", group, _nbytes(send), work=works[0] if len(works) == 1 else None)
    return works


def _linear_into(x, w, out=None):
    """x W^T into ``out`` (returned) when given, else a new tensor (``rs_ring`` partials)."""
    if out is None and _RING_GEMM_TN and dense._CU_HELD and x.is_cuda:
        out = x.new_empty(tuple(x.shape[:-1]) + (w.shape[0],))
    if out is None:
        return torch.nn.functional.linear(x, w)
    _mm_into(out, x, w)
    return out


def _dgrad_rows(g, weight, wt, out=None):
    """dX = g @ weight into ``out`` (returned) when given, else a new tensor."""
    if out is None:
        return dgrad(g, weight, wt)
    dgrad_into(out, g, weight, wt)
    return out


# SMDT_RING_GEMM_TN=1: ring-chunk GEMMs issued while an exchange holds CUs run on gemm_tn with
# the leftover grid (gemm_tn_blocks) instead of hipBLASLt, whose full-chip grid races the exchange
_RING_GEMM_TN = os.environ.get("SMDT_RING_GEMM_TN", "0") == "1"


def _mm_into(dst, a, w, bias=None):
    """dst[..., o] = a[..., k] @ w[o, k]^T (+ bias) written in place (hipBLASLt out= GEMM)."""
    a2 = a.reshape(-1, a.shape[-1])
    d2 = dst.view(-1, dst.shape[-1])
    if _RING_GEMM_TN and dense._CU_HELD and a2.is_cuda and a2.is_contiguous() and d2.is_contiguous() \
            and a2.dtype in (torch.bfloat16, torch.float16) and w.dtype == a2.dtype \
            and (bias is None or bias.dtype == a2.dtype) and _ext.ext().gemm_tn_supported(a2, w) \
            and (a2.shape[0] // 256) * (w.shape[0] // 256) >= gemm_tn_blocks():
        # (only when the GEMM has a tile for every CU it may use: GPT-3 tp4's 2,048-row chunks have
        # 128 and stay on hipBLASLt, profiles/r6_mix/)
        _ext.ext().gemm_tn(a2, w, 1 if bias is not None else 0, bias, d2, None, gemm_tn_blocks())
        return
    if bias is not None:
        torch.addmm(bias, a2, w.t(), out=d2)
    else:
        torch.mm(a2, w.t(), out=d2)


def _direct(group):
    """The multi-link TP exchange engine (comm/tp_direct.py) bound to ``group``, or None."""
    st = ps.get_state()
    td = getattr(st, "tp_direct", None)
    return td if (td is not None and group is st.tp_group and td.active) else None


_SP_GATHER_SLOTS = os.environ.get("SMDT_SP_GATHER_SLOTS", "1") == "1"   # A/B switch
# ring all-gathers whose local block was already in place (written by its producer) vs copied
AG_RING_STATS = {"in_place": 0, "copied": 0}


def _gather_buffer(x, ws, r):
    """The [n * ws, ...] all-gather buffer of ``x`` with x in slot r: the buffer x's producer wrote
    it into (the norm's gather slot, no copy) or a new one with x copied in."""
    n = x.shape[0]
    mark = getattr(x, "_smdt_gather", None)
    if (mark is not None and mark[1] == r and mark[0].shape[0] == n * ws and mark[0].shape[1:] == x.shape[1:]
            and mark[0].is_contiguous() and x.is_contiguous() and x.data_ptr() == mark[0][r * n].data_ptr()):
        AG_RING_STATS["in_place"] += 1
        return mark[0]
    total = x.new_empty((n * ws,) + tuple(x.shape[1:]))
    total[r * n:(r + 1) * n].copy_(x)
    AG_RING_STATS["copied"] += 1
    return total


# Sub-batch interleave (``models/transformer.ParallelTransformer``, SMDT_SP_SUBBATCH): the two
# halves of a micro-batch run each layer phase by phase, alternately, so one half's TP-pair
# exchange travels beside the other half's GEMMs / attention instead of beside half of its own
# GEMM only (a 2-rank ring's sole overlap partner in forward: profiles/r5_predict_tp2x/). The
# issue order of the exchanges stays a pure function of the layer stack on both partners, which
# the relay's per-call epochs need. Forward only: the backward's exchanges already overlap the
# drained weight-gradient GEMMs.
_SPLIT = {"on": False}
# Forward reduce-scatters whose consumer is a fused norm (``defer_rs_add``, set by the layer
# stack): the 2-rank ring's combine (own partial + the peer's) is left to the norm kernel, which
# reads both summands (ops/functional.bias_dropout_add_norm, x2) instead of a separate add pass.
_DEFER_ADD = {"on": False}
_DEFER_RS_ADD = os.environ.get("SMDT_DEFER_RS_ADD", "1") == "1"


class defer_rs_add:
    """Context: forward ring reduce-scatters leave their combine to the consuming fused norm."""

    def __enter__(self):
        self.prev = _DEFER_ADD["on"]
        _DEFER_ADD["on"] = _DEFER_RS_ADD
        return self

    def __exit__(self, *exc):
        _DEFER_ADD["on"] = self.prev
        return False


def _bwd_add_to_norm(x) -> bool:
    """Whether a column SP linear's backward reduce-scatter may leave its combine to x's producer:
    inside the layer stack (``defer_rs_add``), x written by the fused norm kernel into its
    all-gather slot (``_smdt_gather``: the norm's autograd node receives the gradient as is) and on
    the kernel path (the norm backward that reads the pending summand)."""
    return (_DEFER_ADD["on"] and not _SPLIT["on"] and getattr(x, "_smdt_gather", None) is not None
            and _ext.use_kernels(x))


# Ledger of the pending summands: every summand hung on a tensor by
# ``set_pending_add`` must be taken by ``take_pending_add`` (the fused norm, forward or backward,
# or ``materialize_add``). A consumer that reads the tensor some other way would silently miss the
# peer's half, so anything left over at a check point raises instead: the end of the layer
# stack's forward and the end of its backward (models/transformer.ParallelTransformer), and
# DistributedDataParallel.finish_grad_sync.
_ADD_LEDGER = {"issued": 0, "consumed": 0, "live": {}}


# Forward guard (SMDT_DEFER_RS_GUARD, default on): a row-parallel output whose combine is deferred
# becomes a ``PendingPartial`` — its class is swapped in place (0.5 us; an ``as_subclass`` alias
# cost 6 us, +1.5 ms per emulated N = 8 stage step, profiles/r6_guard/) to a tensor subclass
# whose every torch operation raises, apart from metadata reads — until its fused norm takes the
# summand (``take_pending_add``) and turns it back into a plain tensor (``plain``). A consumer
# that reads it before that (a forward hook, a model variant reading the output twice or through
# a non-fused norm) fails at its first read instead of seeing a partial sum.
_GUARD = os.environ.get("SMDT_DEFER_RS_GUARD", "1") == "1"


def _meta_funcs():
    T = torch.Tensor
    out = {T.as_subclass, T.data_ptr, T.dim, T.size, T.numel, T.element_size, T.stride, T.is_contiguous,
           T.__len__, T.__hash__}
    for name in ("shape", "dtype", "device", "is_cuda", "requires_grad", "grad_fn", "ndim", "layout",
                 "is_leaf", "_version", "names"):
        prop = getattr(T, name, None)
        if prop is not None and hasattr(prop, "__get__"):
            out.add(prop.__get__)
    return out


class PendingPartial(torch.Tensor):
    """See _GUARD. Only metadata reads and ``as_subclass`` pass."""

    _META = None

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        if cls._META is None:
            cls._META = _meta_funcs()
        if func in cls._META:
            with torch._C.DisableTorchFunctionSubclass():
                return func(*args, **(kwargs or {}))
        name = getattr(func, "__name__", str(func))
        raise RuntimeError(
            f"a row-parallel output whose reduce-scatter combine was deferred to its fused norm was "
            f"read by another consumer ({name}) — it holds only this rank's partial sum. Run with "
            "SMDT_DEFER_RS_ADD=0, or keep the fused norm as the only consumer.")


def plain(t):
    """``t`` as a plain tensor again (a ``PendingPartial``'s class is swapped back in place)."""
    if type(t) is PendingPartial:
        t.__class__ = torch.Tensor
    return t


def set_pending_add(t, x2, where: str):
    """Hang ``x2`` on ``t`` for its consumer; returns t (forward outputs: turned into a
    ``PendingPartial`` in place under the guard)."""
    if _GUARD and where == "forward output" and type(t) is torch.Tensor:
        t.__class__ = PendingPartial
    t._smdt_add = x2
    _ADD_LEDGER["issued"] += 1
    _ADD_LEDGER["live"][id(t)] = where
    return t


def take_pending_add(t):
    """The pending summand of ``t`` (removed from it and from the ledger), or None. The caller
    then reads ``plain(t)``."""
    x2 = getattr(t, "_smdt_add", None)
    if x2 is not None:
        del t._smdt_add
        _ADD_LEDGER["consumed"] += 1
        _ADD_LEDGER["live"].pop(id(t), None)
    return x2


def check_pending_adds(where: str):
    """Raise if a deferred reduce-scatter summand was issued but never consumed. (Also drops any CU
    hold left by an exchange no ring waited for: every TP exchange of a layer-stack pass is
    complete at these check points.)"""
    dense._CU_HELD.clear()
    live = _ADD_LEDGER["live"]
    if live:
        kinds = sorted(set(live.values()))
        n = len(live)
        live.clear()
        raise RuntimeError(
            f"{n} deferred reduce-scatter summand(s) ({', '.join(kinds)}) were never added by their "
            f"consumer (checked at {where}): a hook, a second consumer or a non-fused norm read a "
            "row-parallel output / column-parallel input gradient without the peer's partial. Run "
            "with SMDT_DEFER_RS_ADD=0 or keep the fused norm as the only consumer.")


def foreign_hooks(module) -> bool:
    """Whether any hook other than the framework's own parameter-wait pre-hooks (marked
    ``_smdt_internal``) could see the layer stack's activations or gradients: global module hooks,
    or forward / backward hooks on ``module`` or a submodule. Deferring the reduce-scatter combine
    is only safe without them (a hook would read a tensor missing the peer's partial)."""
    from torch.nn.modules import module as _M
    for name in ("_global_forward_hooks", "_global_forward_pre_hooks", "_global_backward_hooks",
                 "_global_backward_pre_hooks"):
        if getattr(_M, name, None):
            return True
    for m in module.modules():
        if m._forward_hooks or m._backward_hooks or getattr(m, "_backward_pre_hooks", None):
            return True
        for h in m._forward_pre_hooks.values():
            if not getattr(h, "_smdt_internal", False):
                return True
    return False


def materialize_add(t):
    """Apply a pending reduce-scatter summand (``defer_rs_add``) in place; returns the plain t."""
    x2 = take_pending_add(t)
    t = plain(t)
    if x2 is not None:
        t.data.add_(x2)
    return t
_AG_PENDING = {}      # (data_ptr, shape) of a started all-gather's input -> (total, works, rank, n)
_RS_PENDING = []      # outputs whose reduce-scatter was started but not yet combined
SPLIT_STATS = {"ag_started": 0, "rs_deferred": 0, "rs_add_to_norm": 0, "bwd_add_to_norm": 0}


def _pending_key(x):
    return (x.data_ptr(), tuple(x.shape)) if _AG_PENDING else None


def subbatch_capable(st) -> bool:
    """Whether the TP exchanges can be started / left in flight for the sub-batch interleave: a
    2-rank ring writing into producer-filled gather slots, or a TP4 / TP8 direct engine."""
    if st.tp == 2:
        return sp_gather_spec() is not None
    return st.tp in (4, 8) and _direct(st.tp_group) is not None


def ag_start(x, group):
    """Issue the 2-rank ring all-gather of ``x`` now (TP4 / TP8: the direct engine's whole-chunk
    gather); the ``ag_ring`` call of x's consumer then waits and runs ONE GEMM over all chunks
    (the ring: its local chunk's GEMM, the wait, the peer's chunk)."""
    td = _direct(group)
    if td is not None:
        started = td.start_all_gather(x)
        if started is not None:     # (world-uniform: else the consumer's ag_ring gathers as usual)
            total, hs = started
            _AG_PENDING[(x.data_ptr(), tuple(x.shape))] = (total, hs, td.rank, x.shape[0])
            SPLIT_STATS["ag_started"] += 1
        return x
    ws, r, nxt, prv = _ring(group)
    assert ws == 2, "ag_start: 2-rank rings only"
    x = x.contiguous()
    n = x.shape[0]
    total = _gather_buffer(x, ws, r)
    peer = 1 - r
    # the receive goes through ``.data`` (same storage, own version counter): x is usually a view
    # of ``total`` returned by the fused norm (a multi-output autograd node), and an in-place write
    # into its base seen by autograd before x's consumer is applied would be refused
    raw = total.data
    works = _exchange(raw[r * n:(r + 1) * n], raw[peer * n:(peer + 1) * n], nxt, prv, group)
    _AG_PENDING[(x.data_ptr(), tuple(x.shape))] = (total, works, r, n)
    SPLIT_STATS["ag_started"] += 1
    return x


def rs_finish(t):
    """Complete a reduce-scatter ``rs_ring`` left in flight under the sub-batch interleave: wait for
    the peer's partial of this rank's chunk and add it into ``t`` (in place, outside autograd: the
    gradient of the sum is the gradient of t). Returns t; a no-op for any other tensor."""
    pend = getattr(t, "_smdt_rs_pending", None)
    if pend is None:
        return t
    del t._smdt_rs_pending
    works, incoming, _keep, group = pend
    _wait_works(works, group)
    if incoming is not None:     # the ring's combine (the direct engine's output is the sum)
        t.data.add_(incoming)    # outside autograd (t may be a view output of the linear's Function)
    try:
        _RS_PENDING.remove(t)
    except ValueError:
        pass
    return t


def begin_subbatch():
    _SPLIT["on"] = True


class PendingAddCheck(torch.autograd.Function):
    """Identity on the layer stack's input whose backward (the last node of the stack's backward)
    checks that every deferred summand of that backward was consumed (``check_pending_adds``)."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        check_pending_adds("the end of the layer stack's backward")
        return g


class WgradMergeScope(torch.autograd.Function):
    """Identity whose backward sets ``dense.DEFERRED_WGRAD.merge_repeats`` to ``on``. The sub-batch
    interleave wraps its output with on=True (the first node of the pass's backward) and its
    input with on=False (the last), so the merge of the two halves' pushes is scoped to that
    backward and every later pass flushes repeated pushes in order again."""

    @staticmethod
    def forward(ctx, x, on):
        ctx.on = bool(on)
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        dense.DEFERRED_WGRAD.merge_repeats = ctx.on
        return g, None


def end_subbatch():
    """Leave the interleave: any exchange still in flight is completed (a consumer that never came
    would otherwise leave the relay's epochs of the two partners apart)."""
    _SPLIT["on"] = False
    for t in list(_RS_PENDING):
        rs_finish(t)
    _RS_PENDING.clear()
    for total, works, _r, _n in list(_AG_PENDING.values()):
        for w in works:
            w.wait()
    _AG_PENDING.clear()
    dense._CU_HELD.clear()


# SMDT_RING_PIECES=k (2-rank rings): each exchange goes out in k row pieces, so the peer chunk's
# GEMM starts on the first piece (all-gather) and the first partial piece leaves before the whole
# partial exists (reduce-scatter); pieces keep whole 256-row GEMM blocks (else one piece)
_RING_PIECES = int(os.environ.get("SMDT_RING_PIECES", "1") or 1)


def _row_pieces(n: int, rows_per: int, k: int, align: int = 256):
    """[(a, b)) bounds of k row pieces of an n-row chunk (dim 0) whose GEMM rows (x rows_per) stay
    multiples of ``align`` (256 on the GPU: gemm_tn's row blocks); [(0, n)] when impossible."""
    if k <= 1 or n % k:
        return [(0, n)]
    step = n // k
    if (step * rows_per) % align:
        return [(0, n)]
    return [(i * step, (i + 1) * step) for i in range(k)]


def ag_ring(x, group, chunk_fn=None, before_last_wait=None, _skip_direct=False, bulk=False):
    """All-gather ``x`` along dim 0 over ``group`` as a ring; ``chunk_fn(lo, rows)`` runs on the
    gathered rows [lo, lo + rows.shape[0]) (dim 0) as soon as they are resident, while the next
    chunk is in flight: the ring hands over whole chunks (lo = c * n). Returns the gathered tensor.
    TP groups of 4 / 8 with a direct engine (comm/tp_direct.py) gather over all of the group's
    links at once instead, in row pieces: the local chunk's GEMM beside the first piece, every
    peer's rows of piece j as soon as piece j has landed."""
    pend = _AG_PENDING.pop(_pending_key(x), None)
    if pend is not None:
        # started earlier by ``ag_start`` (sub-batch interleave): the other half's phase ran beside
        # the transfer, so the consumer waits and runs ONE GEMM over both chunks (16,384 rows at
        # the BASELINE point instead of two 8,192-row chunk GEMMs)
        total, works, r, n = pend
        if before_last_wait is not None:
            before_last_wait()
        _wait_works(works, group)
        if chunk_fn is not None:
            chunk_fn(0, total)
        return total
    td = None if _skip_direct else _direct(group)
    if td is not None:
        out = td.all_gather(x, chunk_fn, before_last_wait)
        if out is not None:
            _cs.collective("all_gather", group, _nbytes(out), transport="xgmi")
            return out
    ws, r, nxt, prv = _ring(group)
    n = x.shape[0]
    total = _gather_buffer(x, ws, r)
    if bulk and ws == 2:
        # a sub-batch half's backward (``bulk``): the exchange beside the drained weight-gradient
        # GEMMs, then ONE GEMM over both chunks (half-size chunk GEMMs measured slow)
        peer = 1 - r
        works = _exchange(total[r * n:(r + 1) * n], total[peer * n:(peer + 1) * n], nxt, prv, group)
        if before_last_wait is not None:
            before_last_wait()
        _wait_works(works, group)
        if chunk_fn is not None:
            chunk_fn(0, total)
        return total
    rows_per = x.numel() // max(x.shape[0], 1) // max(x.shape[-1], 1)
    bounds = _row_pieces(n, rows_per, _RING_PIECES, 256 if x.is_cuda else 1) if ws == 2 else [(0, n)]
    if len(bounds) > 1:
        # 2-rank ring in row pieces: every piece of this rank's chunk goes out at once (the
        # engine's stream runs them in order), the local chunk's GEMM runs beside them, then each
        # peer piece's GEMM as soon as that piece has landed
        peer = 1 - r
        works_j = [_exchange(total[r * n + a:r * n + b], total[peer * n + a:peer * n + b], nxt, prv, group)
                   for a, b in bounds]
        SPLIT_STATS["ring_pieces"] = SPLIT_STATS.get("ring_pieces", 0) + len(bounds)
        if chunk_fn is not None:
            chunk_fn(r * n, x)
        for j, (a, b) in enumerate(bounds):
            if j == len(bounds) - 1 and before_last_wait is not None:
                before_last_wait()
            fill_exchange_wait()
            _wait_works(works_j[j], group)
            if chunk_fn is not None:
                chunk_fn(peer * n + a, total[peer * n + a:peer * n + b])
        return total
    for s in range(ws):
        c = (r - s) % ws
        works = None
        if s < ws - 1:
            nc = (c - 1) % ws
            works = _exchange(total[c * n:(c + 1) * n], total[nc * n:(nc + 1) * n], nxt, prv, group)
        if chunk_fn is not None:
            chunk_fn(c * n, x if s == 0 else total[c * n:(c + 1) * n])
        if works is not None:
            if s == ws - 2 and before_last_wait is not None:
                before_last_wait()
            fill_exchange_wait()
            _wait_works(works, group)
    return total


def rs_ring(partial_fn, group, full_shape, ref, before_last_wait=None, bulk=False, defer_add=False):
    """Reduce-scatter along dim 0 over ``group`` as a ring. The tensor being reduced (``full_shape``,
    ``ref``'s dtype / device) is produced on demand: ``partial_fn(lo, rows, out)`` computes its rows
    [lo, lo + rows) — a GEMM on those rows — into ``out`` when given (and returns it), else into a
    new tensor. Ring step s computes the next chunk's partial while the previous one is in flight.
    Returns this rank's reduced chunk. TP groups of 4 / 8 with a direct engine write the partials
    straight into the engine's input buffer in row pieces, each piece reduce-scattered over every
    link of the group while the next piece's GEMMs run."""
    td = _direct(group)
    if td is not None and _SPLIT["on"] and before_last_wait is None:
        # sub-batch interleave: every chunk's partial in ONE GEMM, the reduce-scatter left in
        # flight (``rs_finish`` waits) while the other half's phase runs
        n = full_shape[0] // td.world
        full = partial_fn(0, td.world * n, None)
        started = td.start_reduce_scatter(full)
        if started is None:
            out = full.new_empty((n,) + tuple(full.shape[1:]))
            dist.reduce_scatter_tensor(out, full.contiguous(), group=group)
            return out
        out, hs = started
        out._smdt_rs_pending = (hs, None, full, group)
        _RS_PENDING.append(out)
        SPLIT_STATS["rs_deferred"] += 1
        _cs.collective("reduce_scatter", group, _nbytes(out) * td.world, transport="xgmi")
        return out
    if td is not None:
        out = td.reduce_scatter(partial_fn, full_shape, ref, before_last_wait)
        _cs.collective("reduce_scatter", group, _nbytes(out) * td.world, transport="xgmi")
        return out
    ws, r, nxt, prv = _ring(group)
    n = full_shape[0] // ws
    if _SPLIT["on"] and ws == 2 and before_last_wait is None:
        # sub-batch interleave: the peer's partial, its exchange, this rank's partial; the combine
        # is left to ``rs_finish`` so the other half's work runs while the partial travels
        # (one GEMM over both chunks, then the peer's half goes out; ``own`` is a view of it)
        peer = 1 - r
        full = partial_fn(0, 2 * n, None)
        part = full[peer * n:(peer + 1) * n]
        incoming = torch.empty_like(part)
        works = _exchange(part, incoming, nxt, prv, group)
        own = full[r * n:(r + 1) * n]
        own._smdt_rs_pending = (works, incoming, full, group)
        _RS_PENDING.append(own)
        SPLIT_STATS["rs_deferred"] += 1
        return own
    if bulk and ws == 2:
        # a sub-batch half's backward: one GEMM over both chunks, the peer's half out beside the
        # drained weight-gradient GEMMs, then the combine
        peer = 1 - r
        full = partial_fn(0, 2 * n, None)
        incoming = torch.empty_like(full[:n])
        works = _exchange(full[peer * n:(peer + 1) * n], incoming, nxt, prv, group)
        if before_last_wait is not None:
            before_last_wait()
        _wait_works(works, group)
        return full[r * n:(r + 1) * n].add_(incoming)
    rows_per = 1
    for d in full_shape[1:-1]:
        rows_per *= d
    bounds = _row_pieces(n, rows_per, _RING_PIECES, 256 if ref.is_cuda else 1) if ws == 2 else [(0, n)]
    if len(bounds) > 1:
        # 2-rank ring in row pieces: the peer's partial piece by piece, each piece out as soon as
        # it exists, then this rank's own partial beside the transfers, then the combine
        peer = 1 - r
        incoming = None
        works_j, keep = [], []
        for a, b in bounds:
            part = partial_fn(peer * n + a, b - a, None)
            if incoming is None:
                incoming = torch.empty((n,) + tuple(part.shape[1:]), dtype=part.dtype, device=part.device)
            keep.append(part)
            works_j.append(_exchange(part, incoming[a:b], nxt, prv, group))
        SPLIT_STATS["ring_pieces"] = SPLIT_STATS.get("ring_pieces", 0) + len(bounds)
        own = partial_fn(r * n, n, None)
        for j in range(len(bounds)):
            if j == len(bounds) - 1 and before_last_wait is not None:
                before_last_wait()
            fill_exchange_wait()
            _wait_works(works_j[j], group)
        if (_DEFER_ADD["on"] and before_last_wait is None) or defer_add:
            own = set_pending_add(own, incoming, "backward dgrad" if defer_add else "forward output")
            SPLIT_STATS["bwd_add_to_norm" if defer_add else "rs_add_to_norm"] += 1
            return own
        return own.add_(incoming)
    works, incoming, keep = None, None, []
    for s in range(ws):
        c = (r - s - 1) % ws
        part = partial_fn(c * n, n, None)
        if works is not None:
            if s == ws - 1 and before_last_wait is not None:
                before_last_wait()
            fill_exchange_wait()
            _wait_works(works, group)
            if s == ws - 1 and ws == 2 and ((_DEFER_ADD["on"] and before_last_wait is None) or defer_add):
                # the consuming norm adds it (see _DEFER_ADD)
                part = set_pending_add(part, incoming, "backward dgrad" if defer_add else "forward output")
                SPLIT_STATS["bwd_add_to_norm" if defer_add else "rs_add_to_norm"] += 1
                return part
            part = part.add_(incoming)
        if s == ws - 1:
            return part
        incoming = torch.empty_like(part)
        keep.append(part)
        works = _exchange(part, incoming, nxt, prv, group)
    return None  # unreachable


def sp_gather_spec():
    """(world, rank) of the TP group when sequence-parallel linears run the ring collective-matmul
    (``ag_ring`` can take a producer-filled gather buffer), else None. The multi-link direct
    engine allocates its own buffers."""
    st = ps.get_state()
    if not _TP_OVERLAP or not _SP_GATHER_SLOTS or st.tp <= 1 or st.tp_group is None:
        return None
    td = getattr(st, "tp_direct", None)
    if td is not None and td.active:
        return None
    return st.tp, st.tp_rank


def _flush_wgrad():
    dense.DEFERRED_WGRAD.flush_opportunistic()


class _ColumnSPLinear(torch.autograd.Function):
    """Column-parallel linear on a sequence-parallel input: forward = ring all-gather fused with
    the GEMM (the gathered input is kept for the weight gradient: 288 GB of HBM makes the
    backward re-gather unnecessary); backward = dgrad GEMM fused with a ring reduce-scatter, the
    weight gradient queued and drained while the last chunk is in flight."""

    @staticmethod
    def forward(ctx, x, weight, bias, add_bias=True):
        group = _tp_group()
        x = x.contiguous()
        n = x.shape[0]
        ws = dist.get_world_size(group)
        out = x.new_empty((n * ws,) + tuple(x.shape[1:-1]) + (weight.shape[0],))
        fb = bias if add_bias else None
        total = ag_ring(x, group, lambda lo, ch: _mm_into(out[lo:lo + ch.shape[0]], ch, weight, fb))
        ctx.save_for_backward(total, weight)
        ctx.bias_p = bias
        ctx.n = n
        ctx.bulk = _SPLIT["on"]
        ctx.defer_add = _bwd_add_to_norm(x)
        return out

    @staticmethod
    def backward(ctx, g):
        total, weight = ctx.saved_tensors
        group = _tp_group()
        g = g.contiguous()
        n = ctx.n
        res = {}

        def wgrad():
            g2 = g.reshape(-1, g.shape[-1])
            res["dw"], res["db"] = _wgrad_and_bias(weight, ctx.bias_p, g2, total.reshape(-1, total.shape[-1]))
            _flush_wgrad()
        wt = _dgrad_weight_t(weight)
        gi = rs_ring(lambda lo, m, o: _dgrad_rows(g[lo:lo + m], weight, wt, o), group,
                     g.shape[:-1] + (weight.shape[1],), g, wgrad, bulk=ctx.bulk, defer_add=ctx.defer_add)
        if "dw" not in res:   # world 1 ring: no wait happened
            wgrad()
        return gi, res["dw"], res["db"], None


class _RowSPLinear(torch.autograd.Function):
    """Row-parallel linear whose output is reduce-scattered along the sequence: forward = per-chunk
    GEMMs fused with a ring reduce-scatter; backward = ring all-gather of the output gradient
    fused with the dgrad GEMM (queued weight gradients drained while the last chunk travels)."""

    @staticmethod
    def forward(ctx, x, weight):
        group = _tp_group()
        x = x.contiguous()
        ws = dist.get_world_size(group)
        assert x.shape[0] % ws == 0, "sequence length must divide the TP size"
        n = x.shape[0] // ws
        y = rs_ring(lambda lo, m, o: _linear_into(x[lo:lo + m], weight, o), group,
                    x.shape[:-1] + (weight.shape[0],), x)
        ctx.save_for_backward(x, weight)
        ctx.n = n
        ctx.bulk = _SPLIT["on"]
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        group = _tp_group()
        g = g.contiguous()
        n = ctx.n
        gi = x.new_empty(x.shape)
        wt = _dgrad_weight_t(weight)
        gfull = ag_ring(g, group, lambda lo, ch: dgrad_into(gi[lo:lo + ch.shape[0]], ch, weight, wt),
                        before_last_wait=_flush_wgrad, bulk=ctx.bulk)
        dw = _wgrad(weight, gfull.reshape(-1, gfull.shape[-1]), x.reshape(-1, x.shape[-1]))
        return gi, dw


def column_sp_linear(x, weight, bias):
    return _ColumnSPLinear.apply(x, weight, bias)


def row_sp_linear(x, weight):
    return _RowSPLinear.apply(x, weight)


# --------------------------------------------------------------------------------------------
# TP-invariant initialisation


def _key_seed(base_seed: int, key: str) -> int:
    h = hashlib.sha1(f"{base_seed}:{key}".encode()).digest()
    return int.from_bytes(h[:8], "little") & ((1 << 62) - 1)


_INIT = {"method": "normal", "perform": True, "cpu": False}


@contextlib.contextmanager
def weight_init(method: str = "normal", perform: bool = True, cpu: bool = False):
    """The init rule of the weights built inside (Megatron's ``--init-method-xavier-uniform`` /
    ``--no-initialization``, /root/reference/3_training_megatron-lm/megatron/arguments.py):
    ``"normal"`` draws N(0, std); ``"xavier_uniform"`` draws U(-a, a), a = sqrt(6 / (fan_in +
    fan_out)) of the FULL 2-D weight (so the values do not depend on the TP degree), for every
    weight, the scaled output layers included; ``perform=False`` leaves weights unset (they are
    about to be loaded from a checkpoint) and skips the full-tensor draw; ``cpu=True``
    (``--use-cpu-initialization``) draws on the host generator and moves the shard to the device,
    so a GPU model starts from exactly the CPU model's weights."""
    assert method in ("normal", "xavier_uniform"), method
    old = dict(_INIT)
    _INIT.update(method=method, perform=bool(perform), cpu=bool(cpu))
    try:
        yield
    finally:
        _INIT.update(old)


@torch.no_grad()
def init_full_then_shard(shape, std: float, key: str, base_seed: int, dtype, device, shard_dim: Optional[int],
                         rank: int, world: int, chunks=None):
    """Normal(0, std) init of the FULL tensor from a deterministic generator, then return this
    rank's shard along ``shard_dim``. ``chunks`` (a list of sizes along shard_dim) shards each
    chunk separately (fused QKV / gate-up weights keep per-rank [q|k|v] groups). ``weight_init``
    switches the rule (Xavier-uniform, or no initialization)."""
    dev = torch.device(device) if device is not None else torch.device("cpu")
    if not _INIT["perform"]:
        sh = list(shape)
        if shard_dim is not None and world > 1:
            sh[shard_dim] //= world
        return torch.empty(sh, dtype=dtype, device=dev)
    if _INIT["cpu"] and dev.type != "cpu":
        with weight_init(_INIT["method"], True, False):
            return init_full_then_shard(shape, std, key, base_seed, dtype, None, shard_dim, rank, world,
                                        chunks).to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(_key_seed(base_seed, key))
    full = torch.empty(shape, dtype=torch.float32, device=dev)
    if std == 0:
        full.zero_()
    elif _INIT["method"] == "xavier_uniform" and len(shape) == 2:
        a = math.sqrt(6.0 / (shape[0] + shape[1]))
        full.uniform_(-a, a, generator=gen)
    else:
        full.normal_(0.0, std, generator=gen)
    if shard_dim is None or world == 1:
        return full.to(dtype)
    if chunks is None:
        return full.chunk(world, dim=shard_dim)[rank].contiguous().to(dtype)
    parts = torch.split(full, chunks, dim=shard_dim)
    return torch.cat([p.chunk(world, dim=shard_dim)[rank] for p in parts], dim=shard_dim).contiguous().to(dtype)


class ColumnParallelLinear(nn.Module):
    """Y = X A with A split along its output dim: rank holds A[:, rank-slice]."""

    _fp8 = None     # (FP8State, table row) once attach_fp8 made this an FP8 linear

    def __init__(self, input_size, output_size, bias=True, gather_output=False, init_std=0.02, key="col",
                 seed=1234, params_dtype=torch.float32, device=None, sequence_parallel=False,
                 skip_bias_add=False, chunks=None, async_tensor_model_parallel_allreduce=True,
                 bias_grad_from_output=False):
        super().__init__()
        st = ps.get_state()
        self.tp, self.rank = st.tp, st.tp_rank
        assert output_size % self.tp == 0, f"{output_size} not divisible by TP {self.tp}"
        self.input_size, self.output_size = input_size, output_size
        self.out_local = output_size // self.tp
        self.gather_output = gather_output
        self.sequence_parallel = sequence_parallel and self.tp > 1
        self.skip_bias_add = skip_bias_add
        # skip_bias_add and the caller only ever adds the returned bias to the output (h + b, e.g.
        # the fused bias-GeLU): the bias gradient equals the column sums of this linear's output
        # gradient, so the linear produces it with its weight gradient (one pass over dY) and the
        # returned bias is detached
        self.bias_grad_from_output = bool(bias_grad_from_output and skip_bias_add and bias)
        self.async_ar = async_tensor_model_parallel_allreduce and self.tp > 1 and not self.sequence_parallel
        w = init_full_then_shard((output_size, input_size), init_std, key + ".weight", seed, params_dtype, device, 0,
                                 self.rank, self.tp, chunks)
        self.weight = nn.Parameter(w)
        self.weight.tensor_model_parallel = True
        self.weight.partition_dim = 0
        if bias:
            self.bias = nn.Parameter(torch.zeros(self.out_local, dtype=params_dtype, device=device))
            self.bias.tensor_model_parallel = True
            self.bias.partition_dim = 0
        else:
            self.register_parameter("bias", None)

    def forward(self, x, bias_grad=True):
        """``bias_grad`` False: the caller's next kernel makes this linear's bias gradient
        (``bias_from_producer``), the backward here makes the weight gradient alone."""
        if not (self.async_ar or self.sequence_parallel):
            x = copy_to_tensor_model_parallel_region(x)
        if not bias_grad:       # only the plain linear that adds its bias (the fused-QKV projection)
            assert not self.bias_grad_from_output and not self.skip_bias_add
            y = linear_with_grad_accumulation_and_async_allreduce(x, self.weight, self.bias, self.sequence_parallel,
                                                                  self.async_ar, fp8=self._fp8, bias_grad=False)
        elif self.bias_grad_from_output:
            y = linear_with_grad_accumulation_and_async_allreduce(x, self.weight, self.bias, self.sequence_parallel,
                                                                  self.async_ar, add_bias=False, fp8=self._fp8)
        else:
            b = None if self.skip_bias_add else self.bias
            y = linear_with_grad_accumulation_and_async_allreduce(x, self.weight, b, self.sequence_parallel,
                                                                  self.async_ar, fp8=self._fp8)
        if self.gather_output:
            y = gather_from_tensor_model_parallel_region(y)
        if self.skip_bias_add:
            return y, (self.bias.detach() if self.bias_grad_from_output else self.bias)
        return y


class RowParallelLinear(nn.Module):
    """Y = X A with A split along its input dim; partial outputs are all-reduced (or
    reduce-scattered along the sequence with sequence parallelism)."""

    _fp8 = None     # (FP8State, table row) once attach_fp8 made this an FP8 linear

    def __init__(self, input_size, output_size, bias=True, input_is_parallel=True, init_std=0.02, key="row",
                 seed=1234, params_dtype=torch.float32, device=None, sequence_parallel=False,
                 skip_bias_add=False):
        super().__init__()
        st = ps.get_state()
        self.tp, self.rank = st.tp, st.tp_rank
        assert input_size % self.tp == 0
        self.input_size, self.output_size = input_size, output_size
        self.in_local = input_size // self.tp
        self.input_is_parallel = input_is_parallel
        self.sequence_parallel = sequence_parallel and self.tp > 1
        self.skip_bias_add = skip_bias_add
        w = init_full_then_shard((output_size, input_size), init_std, key + ".weight", seed, params_dtype, device, 1,
                                 self.rank, self.tp)
        self.weight = nn.Parameter(w)
        self.weight.tensor_model_parallel = True
        self.weight.partition_dim = 1
        if bias:
            self.bias = nn.Parameter(torch.zeros(output_size, dtype=params_dtype, device=device))
            self.bias.sequence_parallel = self.sequence_parallel
        else:
            self.register_parameter("bias", None)

    def forward(self, x):
        if not self.input_is_parallel:
            x = scatter_to_tensor_model_parallel_region(x)
        if self.sequence_parallel and _TP_OVERLAP:
            y = _RowSPLinear.apply(x, self.weight)
        elif self.sequence_parallel:
            y = linear_with_grad_accumulation_and_async_allreduce(x, self.weight, None, False, False)
            y = reduce_scatter_to_sequence_parallel_region(y)
        else:
            y = linear_with_grad_accumulation_and_async_allreduce(x, self.weight, None, False, False, fp8=self._fp8)
            y = reduce_from_tensor_model_parallel_region(y)
        if self.skip_bias_add:
            return y, self.bias
        return y + self.bias if self.bias is not None else y


class _EmbeddingLookup(torch.autograd.Function):
    """out = weight[ids]. Backward scatters the rows with ``index_add_`` (device atomics, no host
    synchronisation — torch's sort-based embedding backward stalls the CPU on the GPU and leaves
    the tail of every backward launch-bound), straight into the fp32 DDP ``main_grad`` when the
    weight has one (K7-style fusion: no dense bf16 [V, H] gradient, no cast pass)."""

    @staticmethod
    def forward(ctx, ids, weight):
        ctx.save_for_backward(ids)
        ctx.weight = weight
        return F.embedding(ids, weight)

    @staticmethod
    def backward(ctx, g):
        (ids,) = ctx.saved_tensors
        w = ctx.weight
        flat = ids.reshape(-1)
        g2 = g.reshape(-1, g.shape[-1]).float()
        mg = getattr(w, "main_grad", None)
        if mg is not None and mg.dtype == torch.float32:
            mg.index_add_(0, flat, g2)
            _fire((w,))
            return None, None
        dw = torch.zeros(w.shape, dtype=torch.float32, device=g.device)
        dw.index_add_(0, flat, g2)
        return None, dw.to(w.dtype)


class _AddPositionSlice(torch.autograd.Function):
    """e [s, b, h] + weight[start:start + s] broadcast over b. Backward: de = g, and the table's
    gradient is the batch sum of g (one reduction) added to rows start..start + s of the fp32
    ``main_grad`` (torch's embedding backward would scatter s * b rows with atomics)."""

    @staticmethod
    def forward(ctx, e, weight, start):
        s = e.shape[0]
        ctx.weight, ctx.start = weight, start
        return e + weight[start:start + s].unsqueeze(1)

    @staticmethod
    def backward(ctx, g):
        w, start = ctx.weight, ctx.start
        s = g.shape[0]
        gs = g.sum(1, dtype=torch.float32)                          # [s, h]
        mg = getattr(w, "main_grad", None)
        if mg is not None and mg.dtype == torch.float32:
            mg[start:start + s].add_(gs)
            _fire((w,))
            return g, None, None
        dw = torch.zeros(w.shape, dtype=torch.float32, device=g.device)
        dw[start:start + s] = gs
        return g, dw.to(w.dtype), None


def add_position_slice(e, weight, start: int):
    """e + weight[start:start + e.shape[0]] (learned absolute positions shared by every sequence)."""
    assert start + e.shape[0] <= weight.shape[0], "sequence longer than the position table"
    if not torch.is_grad_enabled() or not weight.requires_grad:
        return e + weight[start:start + e.shape[0]].unsqueeze(1)
    return _AddPositionSlice.apply(e, weight, int(start))


def embedding_lookup(ids, weight):
    """weight[ids] with the synchronisation-free backward above (torch's own path when
    deterministic algorithms are requested: atomics make the fp32 sum order run-dependent)."""
    if torch.are_deterministic_algorithms_enabled() or not torch.is_grad_enabled() or not weight.requires_grad:
        return F.embedding(ids, weight)
    return _EmbeddingLookup.apply(ids, weight)


class VocabParallelEmbedding(nn.Module):
    """Embedding table split along the vocab dim; out-of-range rows contribute zeros and the
    partial lookups are summed across TP (all-reduce, or reduce-scatter with SP)."""

    def __init__(self, num_embeddings, embedding_dim, init_std=0.02, key="embedding", seed=1234,
                 params_dtype=torch.float32, device=None):
        super().__init__()
        st = ps.get_state()
        self.tp, self.rank = st.tp, st.tp_rank
        assert num_embeddings % self.tp == 0, "pad the vocab to a multiple of TP (make-vocab-size-divisible-by)"
        self.num_embeddings = num_embeddings
        self.per = num_embeddings // self.tp
        self.vocab_start = self.rank * self.per
        self.vocab_end = self.vocab_start + self.per
        w = init_full_then_shard((num_embeddings, embedding_dim), init_std, key + ".weight", seed, params_dtype,
                                 device, 0, self.rank, self.tp)
        self.weight = nn.Parameter(w)
        self.weight.tensor_model_parallel = True
        self.weight.partition_dim = 0

    def forward(self, ids, reduce=True):
        if self.tp > 1:
            mask = (ids < self.vocab_start) | (ids >= self.vocab_end)
            local = (ids - self.vocab_start).masked_fill(mask, 0)
            out = embedding_lookup(local, self.weight)
            out = out.masked_fill(mask.unsqueeze(-1), 0.0)
            if reduce:
                out = reduce_from_tensor_model_parallel_region(out)
            return out
        return embedding_lookup(ids, self.weight)


# --------------------------------------------------------------------------------------------
# data broadcast within TP (U4)


def broadcast_data(keys, data, datatype, src_rank=None):
    """Broadcast {key: int tensor} from TP rank 0 to the TP group (sizes first, then a flat
    buffer), like Megatron's ``tensor_parallel.broadcast_data`` (`pretrain_gpt.py:75`)."""
    st = ps.get_state()
    if st.tp == 1 or st.tp_group is None:
        return {k: data[k].to(datatype) for k in keys}
    src = st.tp_ranks[0] if src_rank is None else src_rank
    dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    if st.tp_rank == 0:
        sizes = []
        for k in keys:
            s = list(data[k].shape)
            sizes.append(len(s))
            sizes += s
        sz = torch.tensor(sizes + [0] * (32 * len(keys) - len(sizes)), dtype=torch.long, device=dev)
    else:
        sz = torch.zeros(32 * len(keys), dtype=torch.long, device=dev)
    dist.broadcast(sz, src, group=st.tp_group)
    shapes, i = [], 0
    szl = sz.tolist()
    for _ in keys:
        nd = szl[i]
        shapes.append(szl[i + 1:i + 1 + nd])
        i += 1 + nd
    total = sum(math.prod(s) for s in shapes)
    if st.tp_rank == 0:
        flat = torch.cat([data[k].to(dev).contiguous().view(-1).to(datatype) for k in keys])
    else:
        flat = torch.empty(total, dtype=datatype, device=dev)
    dist.broadcast(flat, src, group=st.tp_group)
    out, off = {}, 0
    for k, s in zip(keys, shapes):
        n = math.prod(s)
        out[k] = flat[off:off + n].view(s)
        off += n
    return out
