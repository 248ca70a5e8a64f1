"""Data parallelism: contiguous param + grad buffers, bucketed RCCL collectives overlapped with
backward, optional ZeRO-1/2 sharding of the reduction.

Replaces torch DDP's C++ Reducer, the SMDDP backend (P2), Megatron's "local" DDP
with a contiguous grad buffer (P3; one 63.65 MB all-reduce per iteration in the reference,
NB3:1847) and the reduction half of the distributed optimizer / ZeRO (P7, P8).

MI355X-first layout:
  * every trainable parameter lives in ONE flat model-dtype buffer and its gradient in ONE flat
    fp32 (or bf16) buffer with the same layout; ``param.data`` / ``param.main_grad`` are views;
  * the layout is split into *regions* by optimizer semantics — (weight-decay?, counts toward the
    grad norm on this rank?, sequence-parallel?) — so the fused Adam / L2-norm kernels run over a
    handful of contiguous ranges instead of hundreds of tensors;
  * each region is cut into *buckets* (reverse registration order ~ backward order); when the
    last gradient of a bucket lands, the bucket's all-reduce (or reduce-scatter for ZeRO) is
    launched asynchronously on RCCL while backward continues;
  * bucket sizes default to "auto" (comm/buckets.py): 8-32 MB chosen at start-up from a
    latency / bandwidth timing of the DP group's links, at least 4 buckets per rank, so the first
    reduce-scatter launches early in backward while each call still amortises its launch /
    protocol latency. Every bucket is padded to a multiple of dp * 64 elements so reduce-scatter
    shards stay 256-byte aligned.
"""
from __future__ import annotations

import contextlib
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch
import torch.distributed as dist
import torch.nn as nn

from ..comm import buckets as _buckets
from ..comm import health as _health
from ..comm import stats as _cs
from ..ops import _ext
from . import state as ps
from . import zero_init as _zi


@dataclass
class Bucket:
    index: int
    region: tuple
    start: int          # element offset in the flat buffers
    end: int            # (padded) end
    params: List[nn.Parameter] = field(default_factory=list)
    pending: dict = field(default_factory=dict)
    handle: object = None
    launched: bool = False
    ag_handle: object = None   # in-flight ZeRO param all-gather (overlap_param_gather)
    alone: bool = False        # holds only the pipeline-tied word embedding
    shard_off: int = 0         # offset of this rank's shard in the ZeRO-2/3 shard stores

    @property
    def numel(self):
        return self.end - self.start


def _region_key(p: nn.Parameter, st) -> tuple:
    wd = not (len(_zi.logical_shape(p)) < 2 or getattr(p, "no_weight_decay", False))
    tp_dup = (st.tp > 1 and not getattr(p, "tensor_model_parallel", False) and st.tp_rank != 0)
    pp_dup = getattr(p, "shared_embedding", False) and not st.is_first_stage(ignore_virtual=True)
    count = not (tp_dup or pp_dup)
    sp = bool(getattr(p, "sequence_parallel", False)) and st.tp > 1
    return (wd, count, sp)


class DistributedDataParallel(nn.Module):
    """Wraps a module; owns the flat param/grad buffers and the bucketed grad reduction.

    Usage per iteration::

        ddp.zero_grad_buffer()
        for micro in range(n):
            with ddp.no_sync() if micro < n - 1 else nullcontext():
                loss(ddp(...)).backward()
        ddp.finish_grad_sync()
    """

    def __init__(self, module: nn.Module, dp_group=None, grad_dtype=torch.float32, bucket_size="auto",
                 overlap_grad_reduce: bool = True, use_distributed_optimizer: bool = False,
                 average_in_collective: bool = True, torch_compat: bool = False,
                 overlap_param_gather: bool = False, zero_stage: int = 1, deterministic_reduce: bool = None):
        """``torch_compat=True`` gives drop-in ``torch.nn.parallel.DistributedDataParallel``
        semantics for scripts that drive a stock ``torch.optim`` optimizer: gradient sync is
        finalised automatically at the end of ``backward()`` (autograd-engine callback),
        reduced gradients are exposed as ``param.grad`` (views of the flat buffer) and the
        buffer is re-zeroed by the next forward."""
        super().__init__()
        self.module = module
        self.torch_compat = torch_compat
        self._needs_zero = False
        self._callback_queued = False
        st = ps.get_state()
        self.st = st
        # gradient reduction over dp x cp: context-parallel ranks hold the same parameters
        self.dp_group = dp_group if dp_group is not None else (st.dp_cp_group or st.dp_group)
        self.dp = dist.get_world_size(self.dp_group) if (dist.is_initialized() and self.dp_group is not None) else 1
        self.dp_rank = dist.get_rank(self.dp_group) if self.dp > 1 else 0
        self.overlap = overlap_grad_reduce
        self.zero = use_distributed_optimizer
        # ZeRO stage of the GRADIENTS: 1 keeps a full fp32 buffer on every rank (reduce-scatter
        # into it, the optimizer reads only its shard); >= 2 keeps only this rank's shard of
        # every bucket (``grad_store``, numel / dp) — a bucket's full fp32 buffer exists only
        # while its gradients are being accumulated and is dropped once its reduce-scatter
        # launched (DeepSpeed stage 2: reduced every micro-batch, accumulated into the shard).
        self.zero_stage = int(zero_stage) if use_distributed_optimizer else 0
        if self.zero_stage >= 2 and (torch_compat or ps.get_state().pp > 1):
            raise ValueError("ZeRO stage >= 2 gradient sharding needs the explicit-step API and pp == 1")
        self.grad_dtype = grad_dtype
        self.sync_enabled = True
        from ..comm import xgmi as _xgmi
        # "smddp" is RCCL underneath (comm/smddp.py): AVG reductions and the xGMI path apply to it
        rccl = self.dp > 1 and _xgmi.rccl_backend(self.dp_group)
        # (the loopback group of a single-GPU rank emulation averages like RCCL: comm/loopback.py)
        from ..comm import loopback as _loopback
        self.use_avg = average_in_collective and (rccl or (self.dp > 1 and _loopback.is_loopback(self.dp_group)))
        # Bucket all-reduces, ZeRO reduce-scatters and parameter all-gathers run on the xGMI IPC
        # kernel on its own stream (comm/xgmi.py) when SMDT_XGMI_ALLREDUCE=1 / the "smddp"
        # backend asks for it, or — by default — for each op a run-time timing on this node shows
        # faster than RCCL (SMDT_XGMI_ALLREDUCE=0: never); larger messages are chunked.
        self.xgmi = _xgmi.create_for_group(self.dp_group, auto=True) if rccl else None
        self.xgmi_in_graph = False     # see _xg: set by a caller that checks health between replays
        # Fixed-order combine (``deterministic_reduce`` / SMDT_DETERMINISTIC_REDUCE=1): every
        # gradient reduction all-gathers the ranks' buckets and sums them locally in rank order,
        # (g_0 + g_1) + g_2 + ..., then divides by dp — independent of the backend's ring / tree
        # association, so a run is bit-reproducible and a single-process reference that folds
        # the same micro-batch gradients in the same order matches it exactly. Costs dp x the
        # bucket bytes of an all-gather and runs synchronously: a debugging / testing mode.
        if deterministic_reduce is None:
            deterministic_reduce = os.environ.get("SMDT_DETERMINISTIC_REDUCE", "0") == "1"
        self.deterministic = bool(deterministic_reduce) and self.dp > 1
        if self.deterministic:
            self.xgmi = None
        self._syncs = 0

        params = [p for p in module.parameters() if p.requires_grad]
        total = sum(_zi.logical_numel(p) for p in {id(p): p for p in params}.values())
        # parameters built under parallel/zero_init.Init: only this rank's shard exists
        self._zero_init = any(_zi.is_partitioned(p) for p in params)
        if self._zero_init and self.zero_stage < 3:
            raise ValueError("parameters built under zero_init.Init need ZeRO stage 3")
        if bucket_size in (None, "auto", 0):
            # one bucket per region when nothing is reduced; else sized for this group's links
            # (comm/buckets.py: 8-32 MB from a start-up latency / bandwidth timing, >= 4 buckets)
            bucket_size = 40_000_000 if self.dp == 1 else _buckets.auto_bucket_elems(
                self.dp_group, total, torch.finfo(grad_dtype).bits // 8)
        self.bucket_size = int(bucket_size)
        seen = set()
        uniq = []
        for p in params:
            if id(p) not in seen:
                seen.add(id(p))
                uniq.append(p)
        params = uniq
        if not params:
            raise ValueError("DistributedDataParallel: module has no trainable parameters")
        dev = params[0].device
        pdtype = params[0].dtype
        for p in params:
            if p.dtype != pdtype:
                raise ValueError("all trainable parameters must share one dtype (cast the module first)")
        self.param_dtype = pdtype

        # ---- group into regions, reverse registration order inside a region
        regions: Dict[tuple, List[nn.Parameter]] = {}
        for p in reversed(params):
            regions.setdefault(_region_key(p, st), []).append(p)
        order = sorted(regions.keys(), key=lambda k: (not k[0], not k[1], k[2]))
        align = max(self.dp, 1) * 64
        self.buckets: List[Bucket] = []
        self.param_index: Dict[int, Tuple[int, int]] = {}
        self.param_bucket: Dict[int, Bucket] = {}
        off = 0
        for key in order:
            cur: Optional[Bucket] = None
            for p in regions[key]:
                n = _zi.logical_numel(p)
                # The pipeline-tied word embedding (first and last stage) sits alone in its bucket
                # so both stages shard it identically under ZeRO: the embedding-group gradient
                # all-reduce after the reduce-scatter then sums matching shards.
                alone = bool(getattr(p, "shared_embedding", False)) and st.pp > 1
                if cur is not None and cur.params and (alone or cur.alone):
                    cur.end = _round_up(off, align)
                    off = cur.end
                    cur = None
                if cur is None or (off - cur.start + n > bucket_size and cur.params):
                    if cur is not None:
                        cur.end = _round_up(off, align)
                        off = cur.end
                    cur = Bucket(len(self.buckets), key, off, off, alone=alone)
                    self.buckets.append(cur)
                self.param_index[id(p)] = (off, n)
                cur.params.append(p)
                self.param_bucket[id(p)] = cur
                off += _round_up(n, 16)  # every param view 16-element aligned (vector kernels need 16 B)
            if cur is not None:
                cur.end = _round_up(off, align)
                off = cur.end
        self.numel = off
        self.params = params
        # (zero-init: the partitioner assembles the shards; the full buffer never exists)
        self.param_data = torch.zeros(0 if self._zero_init else self.numel, dtype=pdtype, device=dev)
        self.shapes = {id(p): ((_zi.logical_shape(p), _contig_strides(_zi.logical_shape(p)))
                               if _zi.is_partitioned(p) else (tuple(p.shape), tuple(p.stride()))) for p in params}
        self.grad_store = None
        self.zero3 = None                                # ZeroParamPartitioner (parallel/zero3.py)
        self._staging: Dict[int, torch.Tensor] = {}    # bucket index -> full fp32 bucket (stage >= 2)
        self._rs_inflight: Dict[int, tuple] = {}       # bucket index -> (handle, tmp shard or None)
        # dp == 1 under stage >= 2: the "shard" is the whole bucket, so gradients accumulate
        # straight into ``grad_store`` (no per-micro-batch staging buffer, zero-fill or copy).
        self._direct = self.zero_stage >= 2 and self.dp == 1
        # Lazily zeroed staging buffers (stage >= 2 with dp > 1): a bucket's fp32 accumulation
        # buffer is allocated uninitialised and each parameter's slice is "fresh" until written —
        # the grouped wgrad launch STORES the first gradient of a fresh weight (no zero fill, no
        # read of zeros: LLaMA-7B SFT moves 27 GB less of each), any other writer zeroes the slice
        # on its first ``main_grad`` access, and slices nobody wrote are zeroed before the bucket's
        # reduce-scatter. SMDT_LAZY_GRAD_ZERO=0 allocates zeroed buffers.
        self._lazy_zero = (self.zero_stage >= 2 and not self._direct
                           and os.environ.get("SMDT_LAZY_GRAD_ZERO", "1") == "1")
        self._fresh: Dict[int, set] = {}               # bucket index -> ids of unwritten slices
        # ids whose slice a queued wgrad GEMM will STORE into (claimed, not yet issued): another
        # writer of such a slice (e.g. the tied embedding's lookup gradient next to the LM head's
        # wgrad) first flushes the queue, so the store lands before its accumulation
        self._claimed: set = set()
        self._gaps: Dict[int, list] = {}               # bucket index -> (lo, hi) padding ranges
        if self.zero_stage >= 2:
            off = 0
            for b in self.buckets:
                b.shard_off = off
                off += b.numel // self.dp
            self.grad_store = torch.zeros(off, dtype=grad_dtype, device=dev)
            self.grad_data = ShardedFlat(self, self.grad_store)
            self._store_fresh = set(range(len(self.buckets)))
        else:
            self.grad_data = torch.zeros(self.numel, dtype=grad_dtype, device=dev)
        with torch.no_grad():
            for p in params:
                o, n = self.param_index[id(p)]
                if not self._zero_init:
                    pv = _dense_view(self.param_data[o:o + n], p)
                    pv.copy_(p.data)
                    p.data = pv
                if self.zero_stage >= 2:
                    _make_lazy_grad_param(p, self)
                else:
                    p.main_grad = _dense_view(self.grad_data[o:o + n], p)
                p._smdt_grad_ready = self._on_grad_ready
        self._hooks = [p.register_post_accumulate_grad_hook(self._post_accumulate) for p in params]
        self.regions = self._region_ranges()
        # ZeRO param all-gather overlapped with the next forward (Megatron --overlap-param-gather):
        # the gathers are issued asynchronously bucket by bucket in forward order after the
        # optimizer step, and a forward pre-hook on each module waits only for the buckets that
        # hold its own parameters.
        self.overlap_param_gather = bool(overlap_param_gather and use_distributed_optimizer and self.dp > 1)
        self._pg_hooks = []
        if self.overlap_param_gather:
            for mod in module.modules():
                own = [p for p in mod._parameters.values() if p is not None and id(p) in self.param_bucket]
                if own:
                    bks = sorted({self.param_bucket[id(p)].index for p in own})
                    self._pg_hooks.append(mod.register_forward_pre_hook(self._make_gather_wait(bks)))
        # Optimizer step overlapped with the next forward (one DP rank, ZeRO optimizer, HIP): the
        # fused AdamW of each bucket runs on a side stream in FORWARD order and records an event;
        # a forward pre-hook on every transformer block (and on the root, for the embeddings /
        # head / final norm) makes the compute stream wait only for its own buckets. Each bucket's
        # gradients are re-zeroed on the side stream right after its update. Measured on LLaMA-7B
        # SFT: +0.9 % only (profiles/r3_optimizer_overlap/) — hipBLASLt's stream-K GEMMs hold every
        # CU, so the memory-bound update mostly finds free CUs between GEMMs, not under them. It
        # applies to one DP rank (single-GPU SFT); SMDT_OVERLAP_OPTIMIZER=0 keeps the step synchronous.
        self._opt_events: Dict[int, object] = {}
        self._async_zeroed = False
        self.overlap_optimizer = bool(use_distributed_optimizer and self.dp == 1 and dev.type == "cuda"
                                      and st.pp == 1 and not torch_compat
                                      and os.environ.get("SMDT_OVERLAP_OPTIMIZER", "1") == "1")
        self.opt_bucket_order = list(reversed(range(len(self.buckets))))
        if self.overlap_optimizer:
            self._install_update_waits(module)
        self._reset_pending()
        if self.dp > 1 and not self._zero_init:
            self.broadcast_params()

    # ---------------------------------------------------------------- layout helpers
    def _region_ranges(self):
        out = {}
        for b in self.buckets:
            s, e = out.get(b.region, (b.start, b.end))
            out[b.region] = (min(s, b.start), max(e, b.end))
        return out

    def shard_range(self, b: Bucket) -> Tuple[int, int]:
        """This DP rank's slice [s, e) of bucket ``b`` (ZeRO)."""
        sz = b.numel // self.dp
        s = b.start + self.dp_rank * sz
        return s, s + sz

    # ---------------------------------------------------------------- forward
    def forward(self, *args, **kwargs):
        if self.torch_compat and self._needs_zero and torch.is_grad_enabled():
            self.grad_data.zero_()
            self._needs_zero = False
        return self.module(*args, **kwargs)

    # ---------------------------------------------------------------- grad plumbing
    def _post_accumulate(self, p):
        if self.torch_compat and not self._callback_queued:
            self._callback_queued = True
            torch.autograd.Variable._execution_engine.queue_callback(self._auto_finalize)
        # The hook also fires when a backward returned None for the parameter, i.e. when a kernel
        # accumulated into main_grad itself (or queued that work: deferred wgrad) and reports
        # readiness through ``_smdt_grad_ready`` — counting that as ready would launch the
        # bucket's reduction before the gradient exists.
        if p.grad is None:
            return
        g = p.grad
        if g.data_ptr() != p.main_grad.data_ptr():
            if (g.is_cuda and g.dtype != p.main_grad.dtype and g.is_contiguous() and p.main_grad.is_contiguous()
                    and _ext.available()):
                # fused cast + accumulate (torch's mixed-dtype add is a slow generic path)
                _ext.ext().cast_(g, p.main_grad, True)
            else:
                p.main_grad.add_(g.view_as(p.main_grad))
        p.grad = None
        self._on_grad_ready(p)

    def _auto_finalize(self):
        self._callback_queued = False
        if self.sync_enabled:
            self.finish_grad_sync()
            for p in self.params:
                p.grad = p.main_grad
            self._needs_zero = True

    def _on_grad_ready(self, p):
        b = self.param_bucket.get(id(p))
        if b is not None and self.zero_stage >= 2:
            left = b.pending.get(id(p), 0) - 1
            if left > 0:
                b.pending[id(p)] = left
                return
            b.pending.pop(id(p), None)
            if self._direct and not b.pending:   # nothing to reduce: re-arm for the next micro-batch
                b.pending = {id(q): int(getattr(q, "_smdt_grad_contributions", 1)) for q in b.params}
            elif self.overlap and not b.pending and b.index in self._staging:
                self._launch(b)
            return
        if b is None or not self.sync_enabled:
            # Gradients of no_sync micro-batches are only accumulated: readiness is counted for
            # the synchronising pass alone (the counts are re-armed when sync is re-enabled).
            return
        # A parameter fed by several gradient paths (tied embedding: LM-head wgrad straight into
        # main_grad + the lookup's autograd accumulation) declares `_smdt_grad_contributions`;
        # it is ready only after the last one.
        left = b.pending.get(id(p), 0) - 1
        if left > 0:
            b.pending[id(p)] = left
            return
        b.pending.pop(id(p), None)
        if self.sync_enabled and self.overlap and not b.pending and not b.launched:
            self._launch(b)

    def _reset_pending(self):
        for b in self.buckets:
            b.pending = {id(p): int(getattr(p, "_smdt_grad_contributions", 1)) for p in b.params}
            b.launched = False
            b.handle = None

    def _launch(self, b: Bucket):
        b.launched = True
        if self.zero_stage >= 2:
            self._launch_sharded(b)
            return
        if self.dp == 1:
            return
        view = self.grad_data[b.start:b.end]
        nb = view.numel() * view.element_size()
        if self.deterministic:
            folded = self._fold(view)
            if self.zero:
                s, e = self.shard_range(b)
                self.grad_data[s:e].copy_(folded[s - b.start:e - b.start])
            else:
                view.copy_(folded)
            b.handle = None
            return
        if self.zero:
            s, e = self.shard_range(b)
            out = self.grad_data[s:e]
            h = self._xg().reduce_scatter_async(out, view, op="avg") if self._xg() is not None else None
            if h is not None:
                b.handle = h
                _cs.collective("reduce_scatter", self.dp_group, nb, transport="xgmi", events=h.timing())
                return
            if self.use_avg:
                b.handle = dist.reduce_scatter_tensor(out, view, op=dist.ReduceOp.AVG, group=self.dp_group,
                                                      async_op=True)
            else:
                view.div_(self.dp)
                b.handle = dist.reduce_scatter_tensor(out, view, group=self.dp_group, async_op=True)
            _cs.collective("reduce_scatter", self.dp_group, nb, work=b.handle)
        else:
            h = self._xg().all_reduce_async(view, op="avg") if self._xg() is not None else None
            if h is not None:
                b.handle = h
                _cs.collective("all_reduce", self.dp_group, nb, transport="xgmi", events=h.timing())
                return
            if self.use_avg:
                b.handle = dist.all_reduce(view, op=dist.ReduceOp.AVG, group=self.dp_group, async_op=True)
            else:
                view.div_(self.dp)
                b.handle = dist.all_reduce(view, group=self.dp_group, async_op=True)
            _cs.collective("all_reduce", self.dp_group, nb, work=b.handle)

    # ---------------------------------------------------------------- ZeRO-2 gradient shards
    def bucket_at(self, i: int) -> Bucket:
        """The bucket holding flat element ``i``."""
        import bisect
        if not hasattr(self, "_starts"):
            self._starts = [b.start for b in self.buckets]
        return self.buckets[bisect.bisect_right(self._starts, i) - 1]

    def _main_grad(self, p) -> torch.Tensor:
        """Stage >= 2: p's fp32 gradient view inside its bucket's accumulation buffer, allocated
        on first touch in a micro-batch (zeroed, or lazily: then a fresh slice is zeroed here)."""
        v = self._mg_raw(p)
        if self._lazy_zero:
            fr = self._fresh.get(self.param_bucket[id(p)].index)
            if fr is not None and id(p) in fr:
                fr.discard(id(p))
                v.zero_()
            elif id(p) in self._claimed:
                from .dense import flush_deferred_wgrad
                flush_deferred_wgrad()
                self._claimed.clear()          # everything queued has been issued
        return v

    def _mg_raw(self, p) -> torch.Tensor:
        """p's gradient view WITHOUT zeroing a fresh slice (the caller claims it: ``_mg_claim``)."""
        b = self.param_bucket[id(p)]
        if self._direct:
            o, n = self.param_index[id(p)]
            shape, stride = self.shapes[id(p)]
            flat = self.grad_store[b.shard_off + (o - b.start):b.shard_off + (o - b.start) + n]
            return flat.view(shape) if _is_dense(shape, stride) else flat.as_strided(shape, stride)
        buf = self._staging.get(b.index)
        if buf is None:
            buf = self._new_staging(b)
        o, n = self.param_index[id(p)]
        shape, stride = self.shapes[id(p)]
        flat = buf[o - b.start:o - b.start + n]
        return flat.view(shape) if _is_dense(shape, stride) else flat.as_strided(shape, stride)

    def _mg_claim(self, p) -> bool:
        """True if p's slice is still unwritten (the caller will STORE the whole gradient into
        it); the slice counts as written from now on."""
        if not self._lazy_zero:
            return False
        fr = self._fresh.get(self.param_bucket[id(p)].index)
        if fr is None or id(p) not in fr:
            return False
        fr.discard(id(p))
        self._claimed.add(id(p))
        return True

    def _new_staging(self, b: Bucket) -> torch.Tensor:
        dev = self.grad_store.device
        if not self._lazy_zero:
            buf = torch.zeros(b.numel, dtype=self.grad_dtype, device=dev)
        else:
            buf = torch.empty(b.numel, dtype=self.grad_dtype, device=dev)
            gaps = self._gaps.get(b.index)
            if gaps is None:
                spans = sorted((o - b.start, o - b.start + n) for o, n in (self.param_index[id(q)] for q in b.params))
                gaps, cur = [], 0
                for lo, hi in spans:
                    if lo > cur:
                        gaps.append((cur, lo))
                    cur = max(cur, hi)
                if cur < b.numel:
                    gaps.append((cur, b.numel))
                self._gaps[b.index] = gaps
            for lo, hi in gaps:            # alignment padding is reduce-scattered too: keep it 0
                buf[lo:hi].zero_()
            self._fresh[b.index] = {id(q) for q in b.params}
        self._staging[b.index] = buf
        return buf

    def _zero_unwritten(self, b: Bucket, buf: torch.Tensor):
        """Slices of bucket b nobody wrote this window (unused parameters) -> 0."""
        fr = self._fresh.pop(b.index, None)
        if not fr:
            return
        for q in b.params:
            if id(q) in fr:
                o, n = self.param_index[id(q)]
                buf[o - b.start:o - b.start + n].zero_()

    def _retire_rs(self, b: Bucket):
        """Wait for bucket b's previous reduce-scatter and fold its shard into ``grad_store``."""
        inflight = self._rs_inflight.pop(b.index, None)
        if inflight is None:
            return
        handle, tmp = inflight
        if handle is not None:
            handle.wait()
        if tmp is not None:
            sh = self.grad_store[b.shard_off:b.shard_off + b.numel // self.dp]
            sh.add_(tmp)

    def _launch_sharded(self, b: Bucket):
        """Reduce-scatter bucket b's accumulation buffer into this rank's shard, drop the buffer,
        and re-arm the bucket for the next micro-batch."""
        self._retire_rs(b)
        buf = self._staging.pop(b.index, None)
        b.pending = {id(q): int(getattr(q, "_smdt_grad_contributions", 1)) for q in b.params}
        b.launched = False
        if buf is None:
            self._fresh.pop(b.index, None)
            return
        if self._lazy_zero:
            self._zero_unwritten(b, buf)
        n = b.numel // self.dp
        sh = self.grad_store[b.shard_off:b.shard_off + n]
        fresh = b.index in self._store_fresh
        self._store_fresh.discard(b.index)
        out = sh if fresh else torch.empty_like(sh)
        h = self._xg().reduce_scatter_async(out, buf, op="avg") if (self._xg() is not None and self.dp > 1) else None
        nb = buf.numel() * buf.element_size()
        if self.deterministic:
            out.copy_(self._fold(buf)[self.dp_rank * n:(self.dp_rank + 1) * n])
            handle = None
        elif self.dp == 1:
            out.copy_(buf)
            handle = None
        elif h is not None:
            handle = h
            _cs.collective("reduce_scatter", self.dp_group, nb, transport="xgmi", events=h.timing())
        else:
            if self.use_avg:
                handle = dist.reduce_scatter_tensor(out, buf, op=dist.ReduceOp.AVG, group=self.dp_group,
                                                    async_op=True)
            else:
                buf.div_(self.dp)
                handle = dist.reduce_scatter_tensor(out, buf, group=self.dp_group, async_op=True)
            _cs.collective("reduce_scatter", self.dp_group, nb, work=handle)
        self._rs_inflight[b.index] = (handle, None if fresh else out)

    def _xg(self):
        """The xGMI engine for the next collective, or None. While a HIP graph is being captured:
        only with ``xgmi_in_graph`` — the engine's calls are replay-safe (per-block device call
        counters; `tests/test_xgmi.py::test_xgmi_engine_replays_from_a_hip_graph`), but its
        per-step health check (comm/health.py, launched in ``finish_grad_sync``) does not run inside
        a replay, so the replaying caller must run it between replays (``health_between_replays``,
        as bench.py's graph step does). Otherwise RCCL's collectives are captured instead."""
        if self.xgmi is None:
            return None
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing() and not self.xgmi_in_graph:
            return None
        return self.xgmi

    def health_between_replays(self) -> bool:
        """For a caller that replays a captured step with the xGMI engine in it: read the previous
        check, then launch this step's (eager, outside the graph). False once the engines fell back
        to RCCL (a peer timed out): the graph holds engine kernels and must not be replayed again."""
        mon = _health.monitor()
        mon.consume()
        if self.xgmi is not None and not self.xgmi.active:
            self.xgmi = None
            return False
        mon.launch()
        return True

    def _fold(self, x: torch.Tensor) -> torch.Tensor:
        """Fixed-order combine (``deterministic_reduce``): all-gather ``x`` from every rank of
        the DP group, sum the copies in rank order and divide by dp."""
        parts = x.new_empty((self.dp,) + tuple(x.shape))
        dist.all_gather_into_tensor(parts.view(-1), x.contiguous().view(-1), group=self.dp_group)
        _cs.collective("all_gather", self.dp_group, x.numel() * x.element_size())
        acc = parts[0].clone()
        for r in range(1, self.dp):
            acc.add_(parts[r])
        return acc.div_(self.dp)

    def bucket_shard_grad(self, b: Bucket) -> torch.Tensor:
        """This rank's reduced gradient shard of bucket b (any stage, after finish_grad_sync)."""
        s, e = self.shard_range(b)
        return self.grad_data[s:e]

    def set_sync_enabled(self, enabled: bool):
        """Gate bucket launches (gradient accumulation / pipeline schedules).

        Re-enabling sync first drains the deferred weight-gradient queue — GEMMs queued by the
        no_sync micro-batches must land, and report readiness, while counting is still off — and
        then re-arms every bucket's pending count, so the synchronising pass launches a bucket
        only after all of ITS gradients were accumulated."""
        enabled = bool(enabled)
        if enabled and not self.sync_enabled:
            from .dense import DEFERRED_WGRAD, flush_deferred_wgrad
            if not DEFERRED_WGRAD.hold:   # (a held accumulation window drains in its last pass)
                flush_deferred_wgrad()
            self._reset_pending()
        self.sync_enabled = enabled

    @contextlib.contextmanager
    def no_sync(self):
        prev = self.sync_enabled
        self.set_sync_enabled(False)
        try:
            yield
        finally:
            self.set_sync_enabled(prev)

    def start_grad_sync(self):
        from .dense import flush_deferred_wgrad
        flush_deferred_wgrad()          # queued weight-gradient GEMMs mark their params ready
        for b in self.buckets:
            if not b.launched:
                self._launch(b)

    def finish_grad_sync(self):
        """Launch what is left, wait for every bucket, then fix up sequence-parallel grads."""
        from .tensor_parallel import check_pending_adds
        check_pending_adds("finish_grad_sync")   # a deferred RS summand no consumer added
        self.wait_param_gather()  # params a forward never touched
        if self.zero_stage >= 2:
            from .dense import flush_deferred_wgrad
            flush_deferred_wgrad()
            for b in self.buckets:
                if b.index in self._staging:
                    self._launch_sharded(b)
            for b in self.buckets:
                self._retire_rs(b)
            self._check_xgmi()
            st = self.st
            if st.tp > 1 and st.tp_group is not None:
                for b in self.buckets:
                    if b.region[2]:
                        g = self.bucket_shard_grad(b)
                        with _cs.blocking("all_reduce", st.tp_group, g.numel() * g.element_size()):
                            dist.all_reduce(g, group=st.tp_group)
            self._reset_pending()
            if self.zero3 is not None:
                self.zero3.end_of_backward()
            return
        self.start_grad_sync()
        for b in self.buckets:
            if b.handle is not None:
                b.handle.wait()
        self._check_xgmi()
        st = self.st
        if st.tp > 1 and st.tp_group is not None:
            for key, (s, e) in self.regions.items():
                if key[2]:  # sequence-parallel params: sum partial grads over the TP group
                    with _cs.blocking("all_reduce", st.tp_group, (e - s) * self.grad_data.element_size()):
                        dist.all_reduce(self.grad_data[s:e], group=st.tp_group)
        self._reset_pending()

    def _check_xgmi(self):
        """Once per sync, the engines' sticky error words are agreed over the world without a host
        sync (comm/health.py): a peer that never arrived (its outputs were NaN-filled, so that step
        is skipped by found-inf) switches every xGMI engine off and the run continues on RCCL."""
        self._syncs += 1
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            return                       # (no engine runs inside a captured step: DDP._xg)
        _health.monitor().launch()

    def zero_grad_buffer(self):
        _health.monitor().consume()      # the previous step's engine-error flag (comm/health.py)
        if self.xgmi is not None and not self.xgmi.active:
            self.xgmi = None
        if self._async_zeroed:           # the overlapped optimizer re-zeroed every bucket
            self._async_zeroed = False
        elif self._direct:
            self.grad_store.zero_()
        elif self.zero_stage >= 2:
            for b in self.buckets:
                self._retire_rs(b)
            self._staging.clear()
            self._fresh.clear()
            self._claimed.clear()
            self._store_fresh = set(range(len(self.buckets)))   # the next reduce-scatter writes
        else:
            self.grad_data.zero_()
        for p in self.params:
            p.grad = None
        self._reset_pending()

    def grad_memory_numel(self) -> int:
        """Elements of persistent gradient storage on this rank (ZeRO-2: ~ numel / dp)."""
        return self.grad_store.numel() if self.grad_store is not None else self.grad_data.numel()

    @torch.no_grad()
    def broadcast_params(self):
        src = dist.get_global_rank(self.dp_group, 0) if self.dp > 1 else dist.get_rank()
        dist.broadcast(self.param_data, src=src, group=self.dp_group)

    @torch.no_grad()
    def all_gather_params(self):
        """ZeRO: after each rank updated its shard of ``param_data``, gather the full buffer.
        With ``overlap_param_gather`` the gathers are left in flight (forward order: the last
        bucket holds the first layers) and waited for by the forward pre-hooks."""
        if self.zero3 is not None:      # stage 3: only the persistent buckets stay gathered
            self.zero3.after_step()
            return
        if self.dp == 1:
            return
        self.wait_param_gather()
        for b in reversed(self.buckets):
            s, e = self.shard_range(b)
            full, mine = self.param_data[b.start:b.end], self.param_data[s:e]
            h = self._xg().all_gather_async(full, mine) if self._xg() is not None else None
            nb = full.numel() * full.element_size()
            if h is not None:
                b.ag_handle = h
                _cs.collective("all_gather", self.dp_group, nb, transport="xgmi", events=h.timing())
            else:
                b.ag_handle = dist.all_gather_into_tensor(full, mine, group=self.dp_group, async_op=True)
                _cs.collective("all_gather", self.dp_group, nb, work=b.ag_handle)
        if not self.overlap_param_gather:
            self.wait_param_gather()

    def wait_param_gather(self, indices=None):
        """Parameters of the given buckets (default: all) are final on the current stream: the
        overlapped ZeRO all-gather and / or the overlapped optimizer update have landed."""
        if self._opt_events:
            self.wait_param_update(indices)
        for b in (self.buckets if indices is None else (self.buckets[i] for i in indices)):
            h = getattr(b, "ag_handle", None)
            if h is not None:
                with _cs.waiting("dp"):
                    h.wait()
                b.ag_handle = None

    def wait_param_update(self, indices=None):
        cur = torch.cuda.current_stream(self.param_data.device) if self._opt_events else None
        for i in (list(self._opt_events) if indices is None else indices):
            ev = self._opt_events.pop(i, None)
            if ev is not None:
                cur.wait_event(ev)

    def _install_update_waits(self, module):
        """Forward pre-hooks for the overlapped optimizer (see __init__), and the bucket order
        the optimizer updates in: the root's own buckets first, then block by block."""
        blocks = [c for m in module.modules() if isinstance(m, nn.ModuleList) for c in m.children()]
        owned, order, groups = set(), [], []
        for blk in blocks:
            ids = {id(p) for p in blk.parameters() if id(p) in self.param_bucket}
            owned |= ids
            groups.append((blk, sorted({self.param_bucket[i].index for i in ids})))
        rest = {id(p) for p in module.parameters() if id(p) in self.param_bucket} - owned
        groups.insert(0, (module, sorted({self.param_bucket[i].index for i in rest})))
        for mod, bks in groups:
            for i in bks:
                if i not in order:
                    order.append(i)
            if bks:
                self._pg_hooks.append(mod.register_forward_pre_hook(self._make_update_wait(bks)))
        order += [i for i in range(len(self.buckets)) if i not in order]
        self.opt_bucket_order = order

    def _make_update_wait(self, indices):
        def hook(_mod, _inp):
            if self._opt_events:
                self.wait_param_update(indices)
        hook._smdt_internal = True
        return hook

    def _make_gather_wait(self, indices):
        def hook(_mod, _inp):
            self.wait_param_gather(indices)
        hook._smdt_gather_wait = True      # also run by modules used without forward() (Norm.fused)
        hook._smdt_internal = True         # reads no activation (tensor_parallel.foreign_hooks)
        return hook

    def state_dict(self, *args, **kwargs):
        self.wait_param_gather()
        if self.zero3 is not None:
            with self.zero3.gathered():
                return {k: v.detach().clone() for k, v in self.module.state_dict(*args, **kwargs).items()}
        return self.module.state_dict(*args, **kwargs)

    def gathered_params(self):
        """Context in which every parameter is materialised (a no-op below ZeRO-3)."""
        return self.zero3.gathered() if self.zero3 is not None else contextlib.nullcontext()

    def load_state_dict(self, sd, strict=True):
        return self.module.load_state_dict(sd, strict=strict)


def _dense_view(flat: torch.Tensor, p: torch.Tensor) -> torch.Tensor:
    """``flat`` (p.numel() elements) viewed with p's shape AND strides: a channels-last conv weight
    (dense but permuted strides) keeps its memory format inside the flat DDP buffers."""
    dense_permuted = ((p.dim() == 4 and p.is_contiguous(memory_format=torch.channels_last))
                      or (p.dim() == 5 and p.is_contiguous(memory_format=torch.channels_last_3d)))
    if p.is_contiguous() or not dense_permuted:
        return flat.view(p.shape)
    return flat.as_strided(p.shape, p.stride())


def _contig_strides(shape):
    st, acc = [], 1
    for d in reversed(shape):
        st.append(acc)
        acc *= d
    return tuple(reversed(st))


def _round_up(x, m):
    return ((x + m - 1) // m) * m


def _is_dense(shape, stride) -> bool:
    exp, st = 1, []
    for d in reversed(shape):
        st.append(exp)
        exp *= d
    return tuple(reversed(st)) == tuple(stride) or len(shape) == 0


class ShardedFlat:
    """Stand-in for a flat buffer of which this rank stores only its shard of every bucket
    (``store``, laid out bucket by bucket). Indexable by global ``[s:e]`` ranges that lie inside
    this rank's shard of one bucket — exactly the ranges the ZeRO optimizer touches — so the
    optimizer code is the same for every stage."""

    def __init__(self, ddp, store: torch.Tensor):
        self.ddp, self.store = ddp, store
        self.dtype, self.device = store.dtype, store.device
        self.is_cuda = store.is_cuda

    def __getitem__(self, sl):
        s, e = sl.start, sl.stop
        b = self.ddp.bucket_at(s)
        bs, be = self.ddp.shard_range(b)
        if not (bs <= s and e <= be):
            raise IndexError(f"[{s}:{e}] is outside this rank's shard [{bs}:{be}] of bucket {b.index}")
        o = b.shard_off + (s - bs)
        return self.store[o:o + (e - s)]

    def zero_(self):
        self.store.zero_()
        return self

    def numel(self):
        return self.store.numel()


class _LazyGradParameter(nn.Parameter):
    """A Parameter whose ``main_grad`` is resolved by its ZeRO-2 DDP on access (the fp32 bucket
    buffer it points into exists only while the bucket accumulates)."""

    @property
    def main_grad(self):
        return self._smdt_ddp._main_grad(self)

    def _smdt_mg_raw(self):
        return self._smdt_ddp._mg_raw(self)

    def _smdt_mg_claim(self):
        return self._smdt_ddp._mg_claim(self)

    @main_grad.setter
    def main_grad(self, v):
        raise AttributeError("main_grad of a ZeRO-2 parameter is owned by its DistributedDataParallel")


def _make_lazy_grad_param(p, ddp):
    p._smdt_ddp = ddp
    if type(p) is nn.Parameter:
        p.__class__ = _LazyGradParameter
