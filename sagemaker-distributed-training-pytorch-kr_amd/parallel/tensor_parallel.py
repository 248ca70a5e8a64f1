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
import weakref
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
from . import state as ps

# --------------------------------------------------------------------------------------------
# collectives helpers


def _tp_size():
    return ps.get_state().tp


def _tp_group():
    return ps.get_state().tp_group


def _nbytes(t):
    return t.numel() * t.element_size()


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


# CUs held by in-flight exchanges (id(work) -> workgroups): the relay engine's kernel (and its
# paced single-GPU stand-in) keeps 2 x world x sub workgroups resident for the whole transfer, one
# per CU (a GEMM workgroup fills a CU's register file, so neither can share a CU). A persistent
# GEMM launched beside it with one workgroup per CU (gemm_tn) would leave that many of its
# workgroups waiting for the transfer to end — or, launched first, keep the transfer from starting
# until the GEMM's tail: measured with the paced stand-in as ~every exchange fully exposed
# (profiles/r6_standin/). Chunk GEMMs issued while an exchange is in flight size their grid to
# the CUs left over (``gemm_tn_blocks``). SMDT_EXCHANGE_CU_RESERVE=0 turns this off.
_CU_HELD = {}
_CU_RESERVE_ON = os.environ.get("SMDT_EXCHANGE_CU_RESERVE", "1") == "1"
_NUM_CUS = []


def _hold_cus(works, blocks):
    if _CU_RESERVE_ON and blocks > 0:
        for w in works:
            _CU_HELD[id(w)] = int(blocks)


def gemm_tn_blocks() -> int:
    """max_blocks for a persistent gemm_tn launch now: 0 (every CU) unless exchanges in flight hold
    CUs, then the CUs they leave."""
    if not _CU_HELD:
        return 0
    if not _NUM_CUS:
        _NUM_CUS.append(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)
    # max, not sum: the exchanges in flight run one after another on their engine's stream
    return max(_NUM_CUS[0] - max(_CU_HELD.values()), _NUM_CUS[0] // 2)


def _wait_works(works, group):
    """Wait (on the current stream) for in-flight works of ``group``'s collectives."""
    for w in works:
        _CU_HELD.pop(id(w), None)
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


# --------------------------------------------------------------------------------------------
# Linear with async grad communication + fused fp32 wgrad accumulation (K7)


_FUSED_WGRAD = os.environ.get("SMDT_FUSED_WGRAD", "1") == "1"
# Which fused fp32-accumulate wgrad GEMM runs: "mfma" (hand-written gfx950 kernel,
# csrc/kernels/wgrad_gemm.hip), "blaslt" (hipBLASLt beta = 1) or "auto" (time both once per shape
# on scratch buffers and keep the faster). The MFMA kernel measured faster than hipBLASLt on every
# GPT-2 345M shape (BENCHMARKS.md), so it is the default.
_WGRAD_IMPL = os.environ.get("SMDT_WGRAD_IMPL", "mfma")
_WGRAD_CHOICE = {}


def _time_us(fn, reps=3):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / reps


def _wgrad_impl(C, mg, g2, t2):
    if _WGRAD_IMPL != "auto" or g2.dtype not in (torch.bfloat16, torch.float16):
        return _WGRAD_IMPL if g2.dtype in (torch.bfloat16, torch.float16) else "blaslt"
    key = (g2.shape[0], g2.shape[1], t2.shape[1], g2.device.index)
    impl = _WGRAD_CHOICE.get(key)
    if impl is None:
        scratch = torch.zeros_like(mg)
        impl = "blaslt"
        if C.wgrad_mfma(scratch, g2, t2, 0):
            tm = _time_us(lambda: C.wgrad_mfma(scratch, g2, t2, 0))
            tb = _time_us(lambda: C.wgrad_accumulate(scratch, g2, t2))
            impl = "mfma" if tm < tb else "blaslt"
        _WGRAD_CHOICE[key] = impl
    return impl


_FP8_DTYPES = (torch.float8_e5m2, torch.float8_e4m3fn)


def _cat_rows(ts):
    """torch.cat along the rows; FP8 segments are concatenated as bytes."""
    if ts[0].dtype in _FP8_DTYPES:
        return torch.cat([t.view(torch.uint8) for t in ts]).view(ts[0].dtype)
    return torch.cat(ts)


def _fire(params):
    """Report to DDP that the gradients of ``params`` (entries may be None) are in their main_grad."""
    for p in params:
        cb = getattr(p, "_smdt_grad_ready", None) if p is not None else None
        if cb is not None:
            cb(p)


def _wgrad_torch(mg, g2, t2, overwrite=False, bias_mg=None):
    """One wgrad problem in torch (CPU, or no kernel took it): mg (+)= g2^T t2 and, with a bias
    target, bias_mg += the column sums of g2."""
    prod = g2.t().matmul(t2).view_as(mg)
    (mg.copy_ if overwrite else mg.add_)(prod)
    if bias_mg is not None:
        bias_mg.add_(g2.float().sum(0))


class _WgradItem:
    """One queued weight gradient of ``DeferredWgrad``: main_grad (+)= g2^T t2 over its segments."""

    __slots__ = ("weight", "main_grad", "bias", "segments", "held", "complete", "fresh", "scales", "mrange", "nbytes")

    def __init__(self, weight, main_grad, bias, held, complete, fresh, scales, mrange):
        self.weight = weight
        self.main_grad = main_grad
        self.bias = bias            # bias Parameter whose gradient comes out of the same launch, or None
        self.segments = []          # one (g2, t2, g2._version, t2._version) per push, in push order
        self.nbytes = 0             # dY / X bytes the segments keep alive
        self.held = held            # created inside an accumulation window
        self.complete = complete    # has its segment of the synchronising pass
        self.fresh = fresh          # main_grad unwritten: the first GEMM into it stores
        self.scales = scales        # FP8 item: (1 / scale of dY, 1 / scale of x), else None
        self.mrange = mrange        # ranged item: (seg table, expert), else None

    @property
    def tiles(self):
        """256 x 256 output tiles of the weight (what ``flush_tiles`` counts)."""
        g2, t2 = self.segments[0][:2]
        return -(-g2.shape[1] // 256) * -(-t2.shape[1] // 256)

    def add(self, seg) -> int:
        """Append a segment; returns its bytes."""
        n = _nbytes(seg[0]) + _nbytes(seg[1])
        self.segments.append(seg)
        self.nbytes += n
        return n

    @property
    def kind(self):
        return "ranged" if self.mrange is not None else "fp8" if self.scales is not None else "16bit"

    @property
    def fillable(self):
        """Whether an exchange-wait filler may issue the item: complete, not held for a later pass,
        and 16-bit (FP8 and ranged items exist at TP = 1 only, so never beside a TP exchange)."""
        return self.complete and not self.held and self.scales is None and self.mrange is None

    @property
    def one_cuda_segment(self):
        """What the grouped filler (``fill_many``) asks on top of ``fillable``."""
        return len(self.segments) == 1 and self.main_grad.is_cuda

    def est_us(self, cus):
        """Estimated GEMM time on ``cus`` CUs (0: the whole chip) at _FILL_PFLOPS, for the filler budget."""
        g2, t2 = self.segments[0][:2]
        fl = 2.0 * g2.shape[0] * g2.shape[1] * t2.shape[1] * len(self.segments)
        return fl / (_FILL_PFLOPS * 1e9 * max(cus or 256, 1) / 256.0)

    def check_versions(self):
        for g2, t2, vg, vt in self.segments:
            if g2._version != vg or t2._version != vt:
                raise RuntimeError("deferred wgrad: a queued dY / X tensor was modified in place before the "
                                   "flush; disable with SMDT_DEFER_WGRAD=0 and report the op that did it")


class DeferredWgrad:
    """Deferred, grouped weight-gradient GEMMs.

    Backward produces one wgrad GEMM per linear layer; on their own the small ones (the 1024 x
    1024 attention projection, the QKV GEMM) cannot fill 256 CUs without split-K, and split-K
    pays fp32 atomics (~1.3 TB/s chip-wide). Instead ``_wgrad`` queues (main_grad, dY, X) and
    the queue is flushed as ONE grouped launch of the gfx950 MFMA kernel
    (csrc/kernels/wgrad_gemm.hip, ``smdt_wgrad_grouped``): every tile runs over the full token
    range, no atomics, deterministic. The queue holds dY / X alive until the flush (a few hundred
    MB per layer at GPT-2 345M scale: trivial next to 288 GB of HBM), flushes once it holds
    ``flush_tiles`` output tiles (several layers, so gradient buckets still become ready while
    backward runs and DDP overlaps their RCCL reduction), and is drained by DDP's
    ``start/finish_grad_sync`` before any gradient is read. A weight is reported ready to DDP
    only when its GEMM has been issued. Tensors are version-checked at flush time: an in-place
    write into a queued dY or X raises instead of producing a wrong gradient.

    FP8 items (``push(..., scales=)``, the FP8 linears under --fp8-wgrad) hold q(dY) / q(x) bytes
    and their two dequantisation factors; a flush round issues them as their own grouped launch of
    the FP8 kernel (csrc/kernels/wgrad_fp8.hip) beside the launch of the round's 16-bit items.
    Everything else (version checks, fresh / overwrite, segment rounds, hold / merge, readiness,
    defer) treats them like 16-bit items; the TP exchange fillers pass over them.

    Ranged items (``push(..., mrange=(seg, e))``, the Switch experts under --moe-grouped-gemm): g2 /
    t2 are the whole expert-sorted, tile-padded buffers and the GEMM runs over expert e's segment,
    which the kernel reads from the device table ``seg`` (wgrad_gemm.hip's ranged kernel: a launch
    of their own inside the same grouped call, never tail-split). They are never merged with a
    later push; the TP exchange fillers pass over them too.
    """

    def __init__(self):
        self.enabled = os.environ.get("SMDT_DEFER_WGRAD", "1") == "1"
        self.flush_tiles = int(os.environ.get("SMDT_DEFER_WGRAD_TILES", "1024"))
        # Gradient-accumulation window (set by the ZeRO engine, train/zero.py): while ``hold`` is
        # on, nothing flushes on size and DDP's sync re-enable does not drain the queue, so the
        # GEMMs of ALL micro-batches of a window meet in the queue. A weight queued again is
        # MERGED (its dY / X segments are concatenated along the token dim at flush time): one
        # GEMM over the window's tokens and ONE read-modify-write of the fp32 main_grad instead of
        # one per micro-batch (LLaMA-7B: 54 GB of main_grad traffic per pass). Held dY / X are
        # capped at SMDT_WGRAD_HOLD_GB, by default a quarter of the device memory free at the
        # first push (then the queue flushes as usual).
        self.hold = False
        self.hold_bytes_cap = None      # set at the first push (_hold_cap)
        self.allow_cpu = False          # tests: exercise the queue logic with a torch fallback
        # Split backward (the zero-bubble pipeline schedules, train/schedules.py): while ``defer``
        # is on, nothing flushes on size and the opportunistic flushes inside backward (beside an
        # in-flight TP collective) are skipped, so a stage's whole backward pass is B (the input
        # gradient chain) and its weight-gradient GEMMs (W) run only when the schedule flushes,
        # after the input gradient was sent to the previous stage.
        self.defer = False
        # Merged items of a held window: concatenate the segments (one GEMM over all tokens, one
        # main_grad read-modify-write: the SFT engine's small micro-batches) or issue one grouped
        # launch per segment round (large pipeline micro-batches: no concatenation copy).
        self.concat_segments = True
        # the sub-batch interleave (models/transformer._forward_subbatch) pushes every weight twice
        # per pass (once per batch half): merge the second push instead of flushing, the segments
        # issued as rounds (no concatenation copy)
        self.merge_repeats = False
        self.ready_after_join = []      # filler-stream items waiting for their readiness report
        self.stats = {"flushes": 0, "items": 0, "max_segments": 0, "stores": 0}
        # membership: written by _add and _take only
        self.items = []                 # _WgradItem, oldest first
        self.by_key = {}                # main_grad.data_ptr() -> item
        self.tiles = 0                  # sum of the items' tiles
        self.held_bytes = 0             # sum of the items' nbytes

    @property
    def targets(self):
        return set(self.by_key)

    def eligible(self, mg, g2, t2):
        if not self.enabled or mg.dtype != torch.float32 or not mg.is_contiguous():
            return False
        if g2.dim() != 2 or t2.dim() != 2:
            return False
        M, N, K = g2.shape[0], g2.shape[1], t2.shape[1]
        if M % 32 or N % 8 or K % 8 or mg.numel() != N * K:
            return False
        if g2.dtype in _FP8_DTYPES:      # an FP8 item (push(..., scales=...)): the FP8 grouped launch
            if t2.dtype != torch.float8_e4m3fn or not SF.fp8_wgrad_supported(M, N, K):
                return False
            return (_FUSED_WGRAD and _ext.use_kernels(g2)) if g2.is_cuda else self.allow_cpu
        if g2.is_cuda:
            return (_FUSED_WGRAD and g2.dtype in (torch.bfloat16, torch.float16) and t2.dtype == g2.dtype
                    and _ext.use_kernels(g2))
        return self.allow_cpu

    def _hold_cap(self, dev) -> int:
        env = os.environ.get("SMDT_WGRAD_HOLD_GB")
        if env is not None:
            return int(float(env) * 2 ** 30)
        if dev.type == "cuda":
            return int(0.25 * torch.cuda.mem_get_info(dev)[0])
        return 64 * 2 ** 30

    def _add(self, it, seg):
        """The one way in: a new item with its first segment, or one more segment of a queued item."""
        self.held_bytes += it.add(seg)
        if len(it.segments) == 1:
            self.items.append(it)
            self.by_key[it.main_grad.data_ptr()] = it
            self.tiles += it.tiles

    def _take(self, picks):
        """The one way out: remove ``picks`` (queued items) from the queue and return them."""
        ids ={id(it) for it in picks}
        self.items = [it for it in self.items if id(it) not in ids]
        for it in picks:
            del self.by_key[it.main_grad.data_ptr()]
            self.tiles -= it.tiles
            self.held_bytes -= it.nbytes
        return picks

    def push(self, weight, mg, g2, t2, bias=None, fresh=False, scales=None, mrange=None):
        """Queue mg += g2^T t2; ``bias`` (a bias Parameter with an fp32 main_grad, or None): its
        gradient, the column sums of g2, comes out of the same grouped launch. ``fresh``: mg holds
        no data yet (a lazily zeroed ZeRO-2 gradient buffer) — the first GEMM into it stores
        instead of adding. ``scales`` = (inv_dy, inv_x), one-element fp32 tensors: g2 / t2 are FP8
        bytes (--fp8-wgrad) and the item goes to the FP8 grouped launch, without a bias (a bias
        gradient is never summed from FP8 bytes). The scales of one weight are the same for every
        segment of a step, so merged segments keep the first pair. ``mrange`` = (seg, e): a ranged
        item, the GEMM over rows [seg[e, 0], + seg[e, 1]) of g2 / t2, read on the device."""
        if mrange is not None and (scales is not None or fresh):
            raise ValueError("deferred wgrad: a ranged item takes 16-bit operands and an accumulating target")
        if (scales is not None) != (g2.dtype in _FP8_DTYPES) or (scales is not None and bias is not None):
            raise ValueError("deferred wgrad: FP8 operands come with scales=(inv_dy, inv_x) and no bias, "
                             "16-bit operands without scales")
        if self.hold_bytes_cap is None:
            self.hold_bytes_cap = self._hold_cap(g2.device)
        g2, t2 = g2.contiguous(), t2.contiguous()
        it = self.by_key.get(mg.data_ptr())
        if it is not None and (mrange is not None or it.mrange is not None):
            self.flush()            # ranged items never merge: the earlier gradient is issued first
            it = None
        if it is not None and (it.held or self.hold or self.merge_repeats):
            # the same main_grad again inside an accumulation window: merge (the sum over the
            # concatenated token range is the same accumulation; one readiness report)
            it.complete = it.complete or not self.hold
        else:
            if it is not None:          # same main_grad twice outside a window: keep order
                self.flush()
            it = _WgradItem(weight, mg, bias, held=self.hold and mrange is None, fresh=bool(fresh), scales=scales,
                            mrange=mrange, complete=not self.hold or mrange is not None)
        self._add(it, (g2, t2, g2._version, t2._version))
        if self.held_bytes > self.hold_bytes_cap:
            self.flush()
        elif not self.hold and not self.defer:
            # size trigger on what a flush would issue now (the complete items): held items still
            # waiting for this pass's gradient neither count nor flush
            ready = [x for x in self.items if x.complete]
            if len(ready) >= 32 or sum(x.tiles for x in ready) >= self.flush_tiles:
                self.flush(complete_only=True)

    def flush_opportunistic(self):
        """A flush placed beside an in-flight collective to overlap it; skipped while ``defer``."""
        if not self.defer:
            self.flush()

    def flush(self, complete_only: bool = False):
        """Issue the queued GEMMs (one grouped launch) and report readiness. ``complete_only`` (the
        size-triggered flush of a synchronising pass): items of a held window whose weight has
        not yet received this pass's gradient stay queued to merge with it. A held item flushed
        without that gradient (a forced flush) accumulates but reports no readiness: the pass's
        own item for the weight does."""
        self._flush([it for it in self.items if it.complete] if complete_only else self.items)

    def flush_unheld(self):
        """Issue every queued item that is not held for a later synchronising pass."""
        self._flush([it for it in self.items if not it.held])

    @torch.no_grad()
    def _flush(self, items):
        if not items:
            return
        for it in self._take(items):        # a failed version check has dropped what was taken
            it.check_versions()
            if len(it.segments) > 1 and self.concat_segments and it.held:
                g2, t2 = _cat_rows([sg[0] for sg in it.segments]), _cat_rows([sg[1] for sg in it.segments])
                it.segments = [(g2, t2, g2._version, t2._version)]
        rounds = max(len(it.segments) for it in items)
        self.stats["flushes"] += 1
        self.stats["items"] += len(items)
        self.stats["max_segments"] = max(self.stats["max_segments"], rounds)
        # round i issues the i-th segment of every item: one grouped launch per round, so two
        # segments of one main_grad never run in the same launch (no write race, no atomics);
        # round 0 of an unwritten main_grad stores (overwrite), later rounds add
        for i in range(rounds):
            rnd = [(it, i, it.fresh and i == 0) for it in items if len(it.segments) > i]
            self.stats["stores"] += sum(1 for r in rnd if r[2])
            self._issue(rnd)
        _fire(p for it in items if it.complete for p in (it.weight, it.bias))

    @torch.no_grad()
    def _issue(self, rnd, cus: int = 0, filler=None):
        """Issue one round: ``rnd`` lists (item, segment index, overwrite), each item once, and the
        launches are sized for ``cus`` CUs (0: the whole chip). ``filler``: None for a flush, where
        torch takes over 16-bit problems that the grouped kernel declines; "grouped" / "blaslt" for
        an exchange-wait filler (16-bit items only), where a declined launch is an error."""
        ops = [(it, it.segments[i][0], it.segments[i][1], ow) for it, i, ow in rnd]
        cuda = [op for op in ops if op[1].is_cuda]
        # one launch for the round's 16-bit items, ranged ones included, and one for its FP8 items
        c16 = [op for op in cuda if op[0].kind != "fp8"]
        done = False
        if c16 and filler == "blaslt":
            # hipBLASLt beta = 1 into main_grad (its own non-persistent tiling shares the CUs
            # with the transfer without a tail split) + the bias column sums
            C = _ext.ext()
            for it, g2, t2, ow in c16:
                if ow:
                    it.main_grad.zero_()
                if not C.wgrad_accumulate(it.main_grad, g2, t2):
                    raise RuntimeError("deferred wgrad filler: hipBLASLt wgrad refused")
                if it.bias is not None:
                    C.bias_grad(g2, it.bias.main_grad, True)
            done = True
        elif c16:
            its, g2s, t2s, ows = map(list, zip(*c16))
            dev = g2s[0].device
            args = [[it.main_grad for it in its], g2s, t2s,
                    [it.bias.main_grad if it.bias is not None else _NO_BIAS.get(dev) for it in its], ows, int(cus)]
            ranged = any(it.mrange is not None for it in its)
            if ranged:      # ranged items: their own launch inside the call
                none = torch.empty(0, dtype=torch.int32, device=dev)
                args += [[it.mrange[0] if it.mrange is not None else none for it in its],
                         [int(it.mrange[1]) if it.mrange is not None else 0 for it in its]]
            done = _ext.ext().wgrad_grouped(*args)
            if not done and ranged:
                raise RuntimeError("deferred wgrad: the grouped launch refused a queued ranged item")
            if not done and filler:
                raise RuntimeError("deferred wgrad filler: grouped launch refused")
        for fmt in _FP8_DTYPES:      # one MFMA opcode per launch: E5M2 and E4M3 dY apart
            f8 = [op for op in cuda if op[0].kind == "fp8" and op[1].dtype == fmt]
            if f8:
                its, g2s, t2s, ows = map(list, zip(*f8))
                if not _ext.ext().wgrad_fp8_grouped([it.main_grad for it in its], g2s, t2s, [it.scales[0] for it in its],
                                                    [it.scales[1] for it in its], ows):
                    raise RuntimeError("deferred wgrad: the FP8 grouped launch refused a queued item")
        for it, g2, t2, ow in ops:
            if g2.is_cuda and (done or it.kind == "fp8"):
                continue
            # CPU (tests: allow_cpu), or kernels disabled: the twins and torch
            bias_mg = it.bias.main_grad if it.bias is not None else None
            if it.kind == "ranged":
                SF.wgrad_ranged_ref(it.main_grad, g2, t2, it.mrange[0], it.mrange[1], bias_mg, ow)
            elif it.kind == "fp8":
                SF.fp8_wgrad_ref(it.main_grad, g2, t2, it.scales[0], it.scales[1], ow)
            else:
                _wgrad_torch(it.main_grad, g2, t2, ow, bias_mg)

    def next_fillable(self):
        """The oldest item an exchange-wait filler may issue, or None."""
        return next((it for it in self.items if it.fillable), None)

    def fill_one(self, cus: int = 0) -> bool:
        """Exchange-wait filler (``fill``): issue the oldest queued, complete and not held item —
        ONE weight's gradient GEMM — as its own grouped launch sized for ``cus`` CUs (the ones an
        in-flight TP exchange leaves; its tail split into pieces that fill them), and report its
        readiness. Returns False when there was nothing to issue."""
        pick = self.next_fillable()
        if pick is None:
            return False
        self._take([pick])
        pick.check_versions()
        for i in range(len(pick.segments)):      # segments in order: round 0 may store
            self._issue([(pick, i, pick.fresh and i == 0)], cus, "blaslt" if _FILL_IMPL == "blaslt" else "grouped")
        self.stats["fills"] = self.stats.get("fills", 0) + 1
        _fire((pick.weight, pick.bias))
        return True

    def fill_many(self, budget_us: float, cus: int = 0, stream=None) -> int:
        """Exchange-wait filler, grouped form: the oldest queued, complete, not held, single-segment
        CUDA items up to ~``budget_us`` of estimated GEMM time (at least one) as ONE grouped launch
        sized for ``cus`` CUs. ``stream``: issue it there (the filler stream: it then never delays
        the next exchange, which waits only for the compute stream) — the caller joins that stream
        and ``fire_ready`` reports the items' readiness afterwards. Returns the items issued."""
        picks, spent = [], 0.0
        for it in self.items:
            if not (it.fillable and it.one_cuda_segment):
                continue
            us = it.est_us(cus)
            if picks and spent + us > budget_us:
                break
            picks.append(it)
            spent += us
            if spent >= budget_us:
                break
        if not picks:
            return 0
        for it in self._take(picks):
            it.check_versions()
            if stream is not None:      # the queue drops them before the filler stream ran
                it.segments[0][0].record_stream(stream)
                it.segments[0][1].record_stream(stream)
        self._issue([(it, 0, it.fresh) for it in picks], cus, "grouped")
        self.stats["fills"] = self.stats.get("fills", 0) + len(picks)
        ready = [p for it in picks for p in (it.weight, it.bias) if p is not None]
        if stream is None:
            _fire(ready)
        else:
            self.ready_after_join.extend(ready)
        return len(picks)

    def fire_ready(self):
        """Readiness of the items issued on the filler stream (after the caller joined it)."""
        ready, self.ready_after_join = self.ready_after_join, []
        _fire(ready)


DEFERRED_WGRAD = DeferredWgrad()
# Exchange-wait fillers (SMDT_W_FILL=1, split-backward pipeline schedules): the W GEMMs of the last
# backward pass stay queued into the next forward, whose TP-exchange waits each issue one of them
# (``fill_exchange_wait``) beside the in-flight transfer, on the CUs the transfer leaves; the rest
# is flushed when that forward ends (train/schedules.py). VERDICT r5 item 1, "split-K W fillers".
W_FILL = os.environ.get("SMDT_W_FILL", "0") == "1"
# W GEMM time offered to one exchange wait (us): ~ the relay's 131 us per 33.6 MB chunk less the
# chunk GEMM beside it; fillers are priced at _FILL_PFLOPS over the CUs the exchange leaves
_FILL_STREAM_ON = os.environ.get("SMDT_W_FILL_STREAM", "1") == "1"
# on the filler stream a filler may outlast its exchange without delaying the next one: 250 us
# measured best there (profiles/r6_fill3/: 110 / 250 / 500 us), 110 us on the compute stream
_FILL_US = float(os.environ.get("SMDT_W_FILL_US", "250" if _FILL_STREAM_ON else "110"))
_FILL_PFLOPS = 1.0
_FILL_IMPL = os.environ.get("SMDT_W_FILL_IMPL", "grouped")     # "grouped" (MFMA, split tail) / "blaslt"
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
    if not (_FILL["on"] and DEFERRED_WGRAD.items):
        return
    cus = gemm_tn_blocks()
    it0 = DEFERRED_WGRAD.next_fillable()
    if it0 is not None and it0.one_cuda_segment:
        if _FILL_STREAM_ON:
            dev = it0.main_grad.device
            fs = _fill_stream(dev)
            fs.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(fs):
                DEFERRED_WGRAD.fill_many(_FILL_US, cus, stream=fs)
        else:
            DEFERRED_WGRAD.fill_many(_FILL_US, cus)
        return
    spent = 0.0
    while spent < _FILL_US:
        it = DEFERRED_WGRAD.next_fillable()
        if it is None:
            return
        spent += it.est_us(cus)
        DEFERRED_WGRAD.fill_one(cus)


def join_fill_stream():
    """The compute stream waits for the filler stream; then the filled items report readiness."""
    if _FILL_STREAMS:
        for dev, fs in _FILL_STREAMS.items():
            torch.cuda.current_stream(dev).wait_stream(fs)
    if DEFERRED_WGRAD.ready_after_join:
        DEFERRED_WGRAD.fire_ready()


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
                DEFERRED_WGRAD.flush_unheld()
        return False


class _NoBias(dict):
    """Per-device empty fp32 tensor: 'no bias target' in a grouped wgrad launch's bias list."""

    def get(self, dev):
        t = super().get(dev)
        if t is None:
            t = self[dev] = torch.empty(0, dtype=torch.float32, device=dev)
        return t


_NO_BIAS = _NoBias()


def flush_deferred_wgrad():
    DEFERRED_WGRAD.flush()


def reset_wgrad_window():
    """Leave hold mode and issue whatever is queued (end of a training loop, or one that stopped
    inside an accumulation window)."""
    DEFERRED_WGRAD.hold = False
    DEFERRED_WGRAD.flush()


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
    if (env == "0" or (env is None and not default)) or not DEFERRED_WGRAD.enabled:
        return False
    if ps.get_state().pp != 1:
        return False
    for d in ddps:
        if getattr(d, "zero3", None) is not None:
            return False
        if getattr(d, "zero_stage", 0) >= 2 and not getattr(d, "_direct", False):
            return False
    return True


def accumulate_wgrad(mg, g2, t2):
    """mg (fp32 [N, K]) += g2^T t2 now: the MFMA wgrad kernel or hipBLASLt beta = 1, whichever the
    per-shape timing picked (no deferral, no readiness callback)."""
    done = False
    if (_FUSED_WGRAD and mg.dtype == torch.float32 and g2.dtype in (torch.bfloat16, torch.float16)
            and g2.is_cuda and mg.is_contiguous()):
        C = _ext.ext()
        g2, t2 = g2.contiguous(), t2.contiguous()
        if _wgrad_impl(C, mg, g2, t2) == "mfma":
            done = C.wgrad_mfma(mg, g2, t2, 0)
        if not done:
            done = C.wgrad_accumulate(mg, g2, t2)
    if not done:
        _wgrad_torch(mg, g2, t2)


def _wgrad_target(weight):
    """(mg, claim) for a weight's gradient GEMM: ``mg`` its fp32 main_grad or None, ``claim()``
    whether the first GEMM into mg stores — call it only when the item is pushed. Of a lazily
    zeroed ZeRO-2 buffer (distributed.py) mg is the raw slice, which ``claim`` may find still
    unwritten; a GEMM that runs now goes to ``weight.main_grad`` instead, which zeroes it."""
    raw = getattr(weight, "_smdt_mg_raw", None)
    if raw is not None:
        return raw(), weight._smdt_mg_claim
    return getattr(weight, "main_grad", None), bool      # bool() is False: nothing to claim


def _wgrad(weight, g2, t2):
    """dW = g2^T t2. With a DDP ``main_grad`` the product is accumulated straight into the fp32
    buffer (K7 gradient-accumulation fusion): queued for the grouped MFMA launch
    (``DeferredWgrad``), or ONE GEMM now (the MFMA kernel or hipBLASLt with beta = 1) instead of a
    bf16 GEMM + a separate fp32 add pass. Returns the gradient to hand back to autograd (None
    when it goes to ``main_grad``)."""
    mg, claim = _wgrad_target(weight)
    if mg is None:
        return g2.t().matmul(t2)
    if DEFERRED_WGRAD.eligible(mg, g2, t2):
        DEFERRED_WGRAD.push(weight, mg, g2, t2, fresh=claim())
        return None
    accumulate_wgrad(weight.main_grad, g2, t2)
    _fire((weight,))
    return None


# The bias gradient of a column-parallel linear (the column sums of dY) comes out of the grouped
# wgrad launch that reads dY anyway (csrc/kernels/wgrad_gemm.hip ``bias``) instead of a separate
# pass over dY; SMDT_WGRAD_BIAS=0 keeps the separate column-sum kernel. Where dY is written by a
# kernel of ours with nothing in between, that kernel makes the sums instead (below) and the
# linear queues its weight gradient without a bias: the wgrad's bias tiles are the slow tile of
# every round of 256 (profiles/bias_from_producer/).
_WGRAD_BIAS = os.environ.get("SMDT_WGRAD_BIAS", "1") == "1"

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
    q = DEFERRED_WGRAD
    if q.hold or q.merge_repeats or q.defer:
        return False
    tgt = SF.grad_accumulate_target(bias_p)
    return tgt is not None and tgt.device == like.device and tgt.numel() == bias_p.numel()


def _wgrad_and_bias(weight, bias_p, g2, t2):
    """(dW, db) for autograd: dW = g2^T t2 and db = sum_rows g2, each None when it went straight
    into the parameter's fp32 main_grad (queued, or by a kernel now)."""
    if bias_p is not None and _WGRAD_BIAS and g2.is_cuda:
        mg, claim = _wgrad_target(weight)
        tgt = SF.grad_accumulate_target(bias_p)
        if mg is not None and tgt is not None and tgt.numel() == g2.shape[-1] and DEFERRED_WGRAD.eligible(mg, g2, t2):
            DEFERRED_WGRAD.push(weight, mg, g2, t2, bias=bias_p, fresh=claim())
            return None, None
    dw = _wgrad(weight, g2, t2)
    return dw, (_bias_grad(bias_p, g2) if bias_p is not None else None)


# dgrad layout: dX = dY W with W [out, in] row-major is hipBLASLt's "NN" GEMM on this ROCm build,
# 14-24 % slower than the "TN" GEMM the forward runs in (F.linear, W^T read K-contiguous). A
# contiguous W^T made by the LDS tile-transpose kernel (ops: transpose2d, ~25 us per GPT-2 345M
# layer) turns every dgrad into F.linear(dY, W^T): 42.5 -> 37.4 ms of dgrad per step at 64 x 1024
# tokens (benchmarks/bench_dgrad.py, profiles/r2_dgrad_tn/). The copy is made per backward call
# (no cache to invalidate when the optimizer or a checkpoint load rewrites the weight).
_DGRAD_TN = os.environ.get("SMDT_DGRAD_TN", "1") == "1"


# W^T is kept from the first backward that needs it until the parameters next change, so gradient
# accumulation (NB4: 8 micro-batches per step) and pipeline micro-batches transpose each weight
# once per optimizer step instead of once per micro-batch (LLaMA-7B: 27 GB of transpose traffic
# per micro-batch). Entries are keyed on the weight's storage and version counter, and the whole
# cache is dropped by ``params_changed()``, which every optimizer step / parameter repair / master
# reload calls before it writes parameters (those writes go through raw kernels that do not bump
# version counters). SMDT_DGRAD_WT_CACHE=0 transposes per call.
_WT_CACHE_ON = os.environ.get("SMDT_DGRAD_WT_CACHE", "1") == "1"
_WT_CACHE: dict = {}


def params_changed():
    """Invalidate every cached W^T and FP8 q(W) (call before any out-of-autograd parameter write)."""
    _WT_CACHE.clear()
    _PARAMS_EPOCH[0] += 1           # the Switch experts' W^T buffers (moe_weight_t_tables) refill
    for s in list(_FP8_STATES):
        s._wq.clear()
    _MX_WQ.clear()
    _DECODE_WQ.clear()


def drop_cached_weight_t(params):
    """Forget the W^T of these parameters (ZeRO-3 frees a gathered bucket: its transposes must go
    with it, or the cache would end up holding a full bf16 copy of the model on every rank)."""
    _PARAMS_EPOCH[0] += 1
    for p in params:
        _WT_CACHE.pop(id(p), None)
        for s in list(_FP8_STATES):
            s._wq.pop(id(p), None)      # q(W) and q(W)^T go with the gathered weight too
        _MX_WQ.pop(id(p), None)
        _DECODE_WQ.pop(id(p), None)


def mm_rows(g, w):
    """g @ w (NN), row-split like ``linear_rows`` (the dgrad form when no W^T is made)."""
    M = g.numel() // g.shape[-1]
    bl = _row_blocks(M) if g.is_cuda else None
    if bl is None:
        return g.matmul(w)
    g2 = g.reshape(M, g.shape[-1])
    out = g.new_empty(tuple(g.shape[:-1]) + (w.shape[1],))
    o2 = out.view(M, w.shape[1])
    for a, b in bl:
        torch.mm(g2[a:b], w, out=o2[a:b])
    return out


def _dgrad_weight_t(weight):
    """W^T [in, out] contiguous for the TN dgrad, or None to use dY @ W directly. (A per-shape
    timed NN-vs-TN pick for few-token backward passes measured neutral on the SFT recipe,
    profiles/r4_sft_dgrad_tn/: TN stays.)"""
    if (_DGRAD_TN and weight.is_cuda and weight.dim() == 2 and weight.is_contiguous()
            and weight.dtype in (torch.bfloat16, torch.float16)
            and weight.shape[0] % 8 == 0 and weight.shape[1] % 8 == 0
            and _ext.use_kernels(weight)):   # raises on a GPU box without the extension
        if not _WT_CACHE_ON:
            return _ext.ext().transpose2d(weight)
        key = (weight.data_ptr(), weight._version, tuple(weight.shape), weight.dtype)
        hit = _WT_CACHE.get(id(weight))
        if hit is not None and hit[0] == key:
            return hit[1]
        wt = _ext.ext().transpose2d(weight)
        _WT_CACHE[id(weight)] = (key, wt)
        return wt
    return None


# Row-split GEMMs. hipBLASLt's heuristic picks poor kernels for token counts just above a multiple
# of 4096 (the SFT recipe's packed windows: M ~ 4.3 k varies every step, so no per-shape tuning
# applies): LLaMA-7B layer GEMMs at M = 4300 run at 845 TF/s whole and 1207 TF/s as 4096 rows +
# the remainder (4608: 927 -> 1206, 8600: 1087 -> 1309; at 5000 / 6100 the whole GEMM is as fast
# or faster; benchmarks/bench_sft_gemm_split.py, profiles/r4_sft_gemm_split/). So a GEMM whose
# M exceeds a multiple of SMDT_GEMM_ROW_SPLIT (4096; 0 = off) by at most a sixth of it is issued
# as two row blocks into one output.
_ROW_SPLIT = int(os.environ.get("SMDT_GEMM_ROW_SPLIT", "4096"))


def _row_blocks(M: int):
    q = _ROW_SPLIT
    if q <= 0 or M <= q:
        return None
    r = M % q
    if r == 0 or r > q // 6:
        return None
    return ((0, M - r), (M - r, M))


# Hand-written MFMA GEMM (csrc/kernels/gemm_tn.hip: persistent 256 x 256 tiles, LDS-DMA stage
# ring, trickled epilogue stores) for out = x W^T where it beats hipBLASLt. SMDT_GEMM_TN: "0" off,
# "1" every supported shape, a comma list of "N:K" pairs (e.g. "4096:1024,1024:4096") for those
# shapes only. The fused fc1 + bias-GeLU op (``linear_bias_gelu``) is governed separately by
# SMDT_FUSED_BIAS_GELU.
_GEMM_TN = os.environ.get("SMDT_GEMM_TN", "0")


def _gemm_tn_shapes():
    if _GEMM_TN in ("0", "", "1"):
        return None
    out = set()
    for item in _GEMM_TN.split(","):
        n, k = item.split(":")
        out.add((int(n), int(k)))
    return out


_GEMM_TN_SHAPES = _gemm_tn_shapes()


def _gemm_tn_ok(x2, w, bias):
    if _GEMM_TN == "0" or not x2.is_cuda or w.dim() != 2:
        return False
    if bias is not None and (bias.dtype != x2.dtype or not bias.is_contiguous()):
        return False
    if _GEMM_TN_SHAPES is not None and (w.shape[0], w.shape[1]) not in _GEMM_TN_SHAPES:
        return False
    return _ext.ext().gemm_tn_supported(x2, w)


def linear_rows(x, w, bias=None):
    """F.linear(x, w, bias), split into row blocks when ``_row_blocks`` says the whole GEMM would
    take a slow hipBLASLt kernel (CUDA only; identical results: each row's dot products are the
    same); the hand-written gemm_tn where SMDT_GEMM_TN selects it."""
    if x.is_cuda and x.dim() >= 2:
        M = x.numel() // x.shape[-1]
        if x.is_contiguous():
            x2 = x.view(M, x.shape[-1])
            if _gemm_tn_ok(x2, w, bias):
                y = _ext.ext().gemm_tn(x2, w, 1 if bias is not None else 0, bias)[0]
                return y.view(tuple(x.shape[:-1]) + (w.shape[0],))
        bl = _row_blocks(M)
        if bl is not None:
            x2 = x.reshape(M, x.shape[-1])
            out = x.new_empty(tuple(x.shape[:-1]) + (w.shape[0],))
            o2 = out.view(M, w.shape[0])
            for a, b in bl:
                if bias is not None:
                    torch.addmm(bias, x2[a:b], w.t(), out=o2[a:b])
                else:
                    torch.mm(x2[a:b], w.t(), out=o2[a:b])
            return out
    return F.linear(x, w, bias)


def dgrad(g, weight, wt=None):
    """dX = g @ weight (g [..., out], weight [out, in]); ``wt`` = weight^T from _dgrad_weight_t."""
    if wt is None:
        return mm_rows(g, weight)
    return linear_rows(g, wt)


def dgrad_into(dst, g, weight, wt=None):
    """dst[...] = g @ weight written in place."""
    if wt is None:
        torch.matmul(g, weight, out=dst)
    else:
        _mm_into(dst, g, wt)


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
        DEFERRED_WGRAD.flush_opportunistic()
        _wait_works([handle], group)
    return gi_out, dw, db


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
        if _tp_size() > 1:
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
    if DEFERRED_WGRAD.eligible(mg, qg, qx):
        DEFERRED_WGRAD.push(weight, mg, qg, qx, fresh=claim(), scales=(inv_dy, inv_x))
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
        if _tp_size() > 1:
            raise NotImplementedError("MXFP8 linears (--fp8-recipe mxfp8) with --tensor-model-parallel-size > 1")
        self.fmt = fmt
        self.grad_fmt = "e5m2" if fmt == "hybrid" else "e4m3"


def mx_weight_q(weight):
    """(q [out, in], s [out, in / 32], qT [in, out], sT [in, out / 32]) of W in E4M3, made once per
    optimizer step (keyed like ``FP8State.weight_q``)."""
    key = (weight.data_ptr(), weight._version, tuple(weight.shape), weight.dtype, _PARAMS_EPOCH[0])
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


# --------------------------------------------------------------------------------------------
# Weight formats for text generation (``generate(weight_format=...)``): inside ``decode_weights``
# every Column / RowParallelLinear and the LM head go through ``_decode_route``. Decode steps
# (M <= 16 rows) run the weight-streaming kernel (csrc/kernels/decode_linear.hip) on the 16-bit
# parameter ("native") or on a cached MXFP8 / MXFP4 copy of it; larger M (the prefill, big batches)
# under a quantised format dequantise the copy into one reused scratch buffer and run the existing
# linear on it, so prefill and decode see the same weight values. The copies are plain tensors in
# a side table: not parameters, not buffers, in no state_dict.

_DECODE = {"state": None}
_DECODE_WQ: dict = {}


class DecodeWeights:
    """What a ``decode_weights`` context carries: the format, the LM-head weight (always streamed
    in its native form: it is tied to the embedding in OPT / GPT-2 and is the accuracy-sensitive
    linear), the kernel's split-K workspace and the dequantisation scratch. ``prepare`` sizes both
    buffers for a model, so no decode step allocates them."""

    def __init__(self, fmt: str, head_weight=None):
        if fmt not in SF.DECODE_LINEAR_FORMATS:
            raise ValueError(f"weight_format must be None or one of {SF.DECODE_LINEAR_FORMATS}, got {fmt!r}")
        self.fmt = fmt
        self.head_weight = head_weight
        self.workspace = None
        self.scratch = None

    def format_of(self, weight) -> str:
        return "native" if weight is self.head_weight else self.fmt

    def prepare(self, linears):
        """``linears``: (name, weight, is_head) of every linear that will be routed. Quantises each
        once (raising for a weight the format cannot take) and allocates the buffers."""
        ws = scr = 0
        dev = dtype = None
        # a decode step has ``batch`` rows, but a short prompt's prefill (rows = batch * length) can
        # take the kernel too: the workspace is sized for the largest M the kernel takes
        max_m = SF.decode_linear_max_m()
        for name, w, _ in linears:
            fmt = self.format_of(w)
            N, K = w.shape
            if fmt != "native":
                if w.dtype == torch.float16:
                    raise ValueError(f"generate(weight_format={self.fmt!r}): {name} is fp16; the quantised formats are "
                                     "for bf16 models (their blocks dequantise to bf16, fp16 cannot hold the small ones)")
                decode_weight_q(w, fmt, name)
                scr = max(scr, w.numel())
            if w.is_cuda and SF.decode_linear_supported(max_m, N, K, w.dtype, fmt):
                ws = max(ws, SF.decode_linear_workspace_numel(max_m, N, K, fmt))
            dev, dtype = w.device, w.dtype
        if ws:
            self.workspace = torch.empty(ws, dtype=torch.float32, device=dev)
        if scr:
            self.scratch = torch.empty(scr, dtype=dtype, device=dev)

    def workspace_for(self, M, N, K, fmt):
        """The split-K workspace for this call (None: no split). ``prepare`` has sized it for every
        shape of its model; a linear it has not seen grows it here."""
        need = SF.decode_linear_workspace_numel(M, N, K, fmt)
        if not need:
            return None
        if self.workspace is None or self.workspace.numel() < need:
            self.workspace = torch.empty(need, dtype=torch.float32, device=torch.device("cuda", torch.cuda.current_device()))
        return self.workspace

    def dequantised(self, weight, q, s, fmt):
        """dequant(q, s) in the weight's dtype, made in the shared scratch buffer itself (exact in
        bf16, so no fp32 copy of the weight is ever built)."""
        if self.scratch is None or self.scratch.numel() < weight.numel() or self.scratch.dtype != weight.dtype:
            self.scratch = torch.empty(weight.numel(), dtype=weight.dtype, device=weight.device)
        return SF.decode_weight_dequantize_into(self.scratch[:weight.numel()].view(weight.shape), q, s, fmt)


class decode_weights:
    """Context: linears are routed by ``state`` (a ``DecodeWeights``); None leaves them alone."""

    def __init__(self, state: Optional[DecodeWeights]):
        self.state = state

    def __enter__(self):
        self.prev = _DECODE["state"]
        _DECODE["state"] = self.state
        return self.state

    def __exit__(self, *exc):
        _DECODE["state"] = self.prev
        return False


def decode_quantised() -> bool:
    """A quantised weight format is active: paths that read ``layer.weight`` themselves (the fused
    GeLU MLP forms, the QKV bias hand-off) must stand back, or they would use the 16-bit weights."""
    st = _DECODE["state"]
    return st is not None and st.fmt != "native"


def decode_weight_q(weight, fmt: str, name: str = "the weight"):
    """(q, scales) of ``weight`` in ``fmt`` ("mxfp8" | "mxfp4"), made once per set of parameter
    values: keyed exactly like ``mx_weight_q``, so a training step or an in-place edit
    re-quantises. One copy per weight: asking for another format replaces it. ``params_changed``
    and ``drop_cached_weight_t`` drop the copies with the other cached weight forms."""
    key = (weight.data_ptr(), weight._version, tuple(weight.shape), weight.dtype, _PARAMS_EPOCH[0], fmt)
    hit = _DECODE_WQ.get(id(weight))
    if hit is not None and hit[0] == key:
        return hit[1]
    with torch.no_grad():
        forms = SF.decode_weight_quantize(weight.detach(), fmt, name)
    if hit is None:         # the copy goes when its weight does (a deleted model frees its copies)
        weakref.finalize(weight, _DECODE_WQ.pop, id(weight), None)
    _DECODE_WQ[id(weight)] = (key, forms)
    return forms


def _decode_route(st: DecodeWeights, x, weight, bias, add_bias, fp8):
    if fp8 is not None:
        raise RuntimeError("generate(weight_format=...): this linear carries _fp8 (an FP8 / MXFP8 training linear); "
                           "weight formats are for models with plain 16-bit linears")
    fmt = st.format_of(weight)
    b = bias if add_bias else None
    N, K = weight.shape
    M = x.numel() // K
    kernel = x.is_cuda and weight.dtype == x.dtype and SF.decode_linear_supported(M, N, K, x.dtype, fmt)
    if fmt == "native":
        if kernel:
            return SF.decode_linear(x, weight.detach(), None, b, "native", st.workspace_for(M, N, K, fmt))
        return linear_rows(x, weight, b)
    if x.dtype == torch.float16:
        raise ValueError(f"generate(weight_format={fmt!r}): fp16 activations; the quantised formats are for bf16 models "
                         "(their blocks dequantise to bf16, fp16 cannot hold the small ones)")
    q, s = decode_weight_q(weight, fmt)
    if kernel:
        return SF.decode_linear(x, q, s, b, fmt, st.workspace_for(M, N, K, fmt))
    return linear_rows(x, st.dequantised(weight, q, s, fmt), b)


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


class GroupedSwitchExperts(torch.autograd.Function):
    """The experts of a Switch MLP at TP = 1 on the expert-sorted, tile-padded rows that
    ``SF.moe_route`` laid out (--moe-grouped-gemm): no host sync, no launch shape that depends on
    the per-expert counts, so the layer can be captured in a HIP graph.

    Forward: gather the tokens into the padded buffer (pad rows zero), grouped fc1 + bias + GeLU
    (keeps the pre-activation, as ``FusedGeLUMLP``), grouped fc2 + bias, gather back by
    ``row_of_token``, times ``top_p``. Backward: d(top_p) = rowwise dot of dOut with the unscaled
    expert output; the scaled dOut gathered into the padded layout, fc2 dgrad with the GeLU
    backward in its epilogue on the per-expert W2^T, fc1 dgrad on the per-expert W1^T, gather back.
    The 2 E weight gradients (and the bias gradients, from their bias tiles) are ranged items of
    ``DeferredWgrad`` when the parameters have an fp32 ``main_grad`` — the kernel path requires
    one; the torch twin (CPU, or SMDT_DISABLE_KERNELS=1) hands them to autograd otherwise, None for
    an expert without tokens.

    ``apply(x [T, h], top_p [T], route, tabs, E, *w1, *b1, *w2, *b2)``: ``route`` the tuple
    ``SF.moe_route`` returned, ``tabs`` = (fc1 tables, fc2 tables) for the forward or None."""

    @staticmethod
    def forward(ctx, x, top_p, route, tabs, E, *params):
        w1, b1, w2, b2 = (list(params[i * E:(i + 1) * E]) for i in range(4))
        _, _, row_of_token, token_of_row, tile_expert, seg, _ = route
        kern = _ext.use_kernels(x)
        if kern:
            xs = _ext.ext().gather_rows(x.contiguous(), token_of_row)
        else:
            xs = x.index_select(0, token_of_row.clamp_min(0)) * (token_of_row >= 0).unsqueeze(-1).to(x.dtype)
        pre, act = SF.gemm_tn_grouped(xs, w1, tile_expert, 2, b1, tables=tabs[0] if tabs else None)
        y = SF.gemm_tn_grouped(act, w2, tile_expert, 1, b2, tables=tabs[1] if tabs else None)[0]
        u = y.index_select(0, row_of_token)                  # the unscaled expert output per token
        ctx.save_for_backward(xs, pre, act, u, top_p, row_of_token, token_of_row, tile_expert, seg)
        ctx.params = (w1, b1, w2, b2)
        ctx.kern = kern
        return u * top_p.unsqueeze(-1).to(x.dtype)

    @staticmethod
    def backward(ctx, dout):
        xs, pre, act, u, top_p, row_of_token, token_of_row, tile_expert, seg = ctx.saved_tensors
        w1, b1, w2, b2 = ctx.params
        E = len(w1)
        dprob = (dout * u).sum(-1).to(top_p.dtype)
        du = (dout * top_p.unsqueeze(-1).to(dout.dtype)).contiguous()
        if ctx.kern:
            dys = _ext.ext().gather_rows(du, token_of_row)
            w2t, w1t = moe_weight_t_tables(w2, b1), moe_weight_t_tables(w1, None)
        else:
            dys = du.index_select(0, token_of_row.clamp_min(0)) * (token_of_row >= 0).unsqueeze(-1).to(du.dtype)
            w2t = w1t = None
        b1d = [b.detach() for b in b1]
        dz = SF.gemm_tn_grouped(dys, w2t[0] if w2t else [w.detach().t().contiguous() for w in w2], tile_expert, 3, b1d,
                                aux=pre, tables=w2t[1] if w2t else None)[0]
        dxs = SF.gemm_tn_grouped(dz, w1t[0] if w1t else [w.detach().t().contiguous() for w in w1], tile_expert, 0,
                                 tables=w1t[1] if w1t else None)[0]
        dx = dxs.index_select(0, row_of_token)
        grads = []
        for ws, bs, g2, t2 in ((w1, b1, dz, xs), (w2, b2, dys, act)):
            gw, gb = [], []
            for e in range(E):
                dw, db = _wgrad_ranged(ws[e], bs[e], g2, t2, seg, e, ctx.kern)
                gw.append(dw)
                gb.append(db)
            grads.append((gw, gb))
        (gw1, gb1), (gw2, gb2) = grads
        return (dx, dprob, None, None, None, *gw1, *gb1, *gw2, *gb2)


def _wgrad_ranged(weight, bias_p, g2, t2, seg, e, kern):
    """(dW, db) of expert e for autograd, each None when it went into the fp32 main_grad: queued as
    a ranged item (``DeferredWgrad``) or, on the twin without a main_grad, computed from the host
    copy of the segment (None for an expert without tokens)."""
    # not _wgrad_target: a ranged item only accumulates, so a lazily zeroed buffer is zeroed here
    mg = getattr(weight, "main_grad", None)
    bmg = getattr(bias_p, "main_grad", None)
    if mg is not None and bmg is not None and mg.dtype == torch.float32 and bmg.dtype == torch.float32:
        if DEFERRED_WGRAD.eligible(mg, g2, t2):
            DEFERRED_WGRAD.push(weight, mg, g2, t2, bias=bias_p, mrange=(seg, e))
            return None, None
        if kern:
            SF.wgrad_ranged(mg, g2, t2, seg, e, bmg)
        else:
            SF.wgrad_ranged_ref(mg, g2, t2, seg, e, bmg)
        _fire((weight, bias_p))
        return None, None
    if kern:
        raise RuntimeError("--moe-grouped-gemm: the experts' weights and biases need an fp32 main_grad")
    s, r = (int(v) for v in seg[e].tolist())
    if r == 0:
        return None, None
    return g2[s:s + r].t().matmul(t2[s:s + r]), g2[s:s + r].sum(0)


# Per-expert W^T for the grouped dgrads: one persistent [E, in, out] buffer per weight list with
# the pointer tables over it, both made once (the table's H2D copy would not be capturable, and a
# graph replay must find the W^T where the capture left them). The contents are re-transposed
# when the parameters changed: ``params_changed`` / ``drop_cached_weight_t`` advance the epoch.
_MOE_WT: dict = {}
_PARAMS_EPOCH = [0]


def moe_weight_t_tables(weights, biases):
    """([W_e^T], (table of the W_e^T, table of ``biases`` or None)) for ``gemm_tn_grouped``."""
    key = (tuple((w.data_ptr(), tuple(w.shape), w.dtype) for w in weights),
           tuple(b.data_ptr() for b in biases) if biases is not None else None)
    hit = _MOE_WT.get(id(weights[0]))
    if hit is None or hit["key"] != key:
        buf = weights[0].new_empty((len(weights), weights[0].shape[1], weights[0].shape[0]))
        wts = list(buf.unbind(0))
        hit = {"key": key, "wts": wts, "tabs": SF.moe_pointer_tables(wts, biases), "stamp": None}
        _MOE_WT[id(weights[0])] = hit
    stamp = (_PARAMS_EPOCH[0], tuple(w._version for w in weights))
    if hit["stamp"] != stamp:
        with torch.no_grad():
            for wt, w in zip(hit["wts"], weights):
                wt.copy_(w.detach().t())
        hit["stamp"] = stamp
    return hit["wts"], hit["tabs"]


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
    if not _NUM_CUS:
        _NUM_CUS.append(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)
    return (rows // 256) * (n // 256) >= _NUM_CUS[0]


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
    if not (_LM_HEAD_CE and tp > 1 and weight.shape[0] % 8 == 0 and weight.shape[0] <= 65536
            and weight.dtype == h.dtype):
        return False
    if h.is_cuda:
        return _ext.use_kernels(h) and h.dtype == torch.bfloat16
    return os.environ.get("SMDT_LM_HEAD_CE_CPU", "0") == "1"


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


def linear_with_grad_accumulation_and_async_allreduce(x, weight, bias, sequence_parallel=False,
                                                      async_grad_allreduce=False, add_bias=True, fp8=None,
                                                      bias_grad=True):
    if _DECODE["state"] is not None:    # generate(weight_format=...): unsharded, no gradients
        return _decode_route(_DECODE["state"], x, weight, bias, add_bias, fp8)
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
    if out is None and _RING_GEMM_TN and _CU_HELD and x.is_cuda:
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
    if _RING_GEMM_TN and _CU_HELD and a2.is_cuda and a2.is_contiguous() and d2.is_contiguous() \
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
    _CU_HELD.clear()
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
    """Identity whose backward sets ``DEFERRED_WGRAD.merge_repeats`` to ``on``. The sub-batch
    interleave wraps its output with on=True (the first node of the pass's backward) and its
    input with on=False (the last), so the merge of the two halves' pushes is scoped to that
    backward and every later pass flushes repeated pushes in order again."""

    @staticmethod
    def forward(ctx, x, on):
        ctx.on = bool(on)
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        DEFERRED_WGRAD.merge_repeats = ctx.on
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
    _CU_HELD.clear()


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
    DEFERRED_WGRAD.flush_opportunistic()


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


def _bias_grad(bias_p, g2):
    """Column sums of g2 into the bias' fp32 main_grad (returns None) or as a tensor."""
    if bias_p is None:
        return None
    tgt = SF.grad_accumulate_target(bias_p)
    if tgt is not None and g2.is_contiguous() and g2.shape[-1] % 8 == 0:
        _ext.ext().bias_grad(g2, tgt, True)
        bias_p._smdt_grad_ready(bias_p)
        return None
    return g2.sum(0)


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
