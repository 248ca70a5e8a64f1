"""Dense-linear base of ``parallel/``: what every linear shares, whatever its operand format or its
collectives.

Owns the CU-hold bookkeeping of in-flight exchanges, the weight-gradient accumulation into the fp32
``main_grad`` (the deferred, grouped wgrad queue ``DEFERRED_WGRAD`` and its immediate forms), the
dense GEMM routing (row split, gemm_tn, the cached W^T of the TN dgrad) and the invalidation of
cached weight forms (``params_changed`` / ``drop_cached_weight_t``; a feature module adds its own
cache with ``register_weight_cache``).

Bottom layer: no collectives, no ``torch.distributed``, no parallel state. The feature modules
(fp8_linear, decode_weights, moe_experts, lm_head) and tensor_parallel import it; it imports none
of them.
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from ..ops import _ext
from ..ops import functional as SF


def _nbytes(t):
    return t.numel() * t.element_size()


# CUs held by in-flight exchanges (id(work) -> workgroups): the relay engine's kernel (and its
# paced single-GPU stand-in) keeps 2 x world x sub workgroups resident for the whole transfer, one
# per CU (a GEMM workgroup fills a CU's register file, so neither can share a CU). A persistent
# GEMM launched beside it with one workgroup per CU (gemm_tn) would leave that many of its
# workgroups waiting for the transfer to end — or, launched first, keep the transfer from starting
# until the GEMM's tail: measured with the paced stand-in as ~every exchange fully exposed
# (profiles/r6_standin/). Chunk GEMMs issued while an exchange is in flight size their grid to
# the CUs left over (``gemm_tn_blocks``). SMDT_EXCHANGE_CU_RESERVE=0 turns this off. The exchanges
# themselves enter and leave the table (tensor_parallel ``_hold_cus`` / ``_wait_works``).
_CU_HELD = {}
_NUM_CUS = []


def gemm_tn_blocks() -> int:
    """max_blocks for a persistent gemm_tn launch now: 0 (every CU) unless exchanges in flight hold
    CUs, then the CUs they leave."""
    if not _CU_HELD:
        return 0
    if not _NUM_CUS:
        _NUM_CUS.append(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)
    # max, not sum: the exchanges in flight run one after another on their engine's stream
    return max(_NUM_CUS[0] - max(_CU_HELD.values()), _NUM_CUS[0] // 2)


# --------------------------------------------------------------------------------------------
# Fused fp32 wgrad accumulation (K7)


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


# What the exchange-wait fillers (tensor_parallel.fill_exchange_wait) need of the queue itself: the
# rate its items are priced at for the filler budget, and which GEMM issues a single filled item
_FILL_PFLOPS = 1.0
_FILL_IMPL = os.environ.get("SMDT_W_FILL_IMPL", "grouped")     # "grouped" (MFMA, split tail) / "blaslt"


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
# kernel of ours with nothing in between, that kernel makes the sums instead
# (tensor_parallel.bias_from_producer) and the linear queues its weight gradient without a bias:
# the wgrad's bias tiles are the slow tile of every round of 256 (profiles/bias_from_producer/).
_WGRAD_BIAS = os.environ.get("SMDT_WGRAD_BIAS", "1") == "1"


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


# --------------------------------------------------------------------------------------------
# Dense GEMM routing


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

# Every other cached form of a weight (a quantised copy, its transpose) lives in the feature module
# that makes it, which registers here how to drop all of it and how to drop one parameter's.
_WEIGHT_CACHES: list = []
# Counts the calls of ``params_changed`` / ``drop_cached_weight_t``. A cache that outlives those
# calls (the Switch experts' persistent W^T buffers, moe_experts) or whose entries must all go
# stale when any gathered weight is freed (mx_weight_q, decode_weight_q) keys on it.
WEIGHTS_EPOCH = [0]


def register_weight_cache(drop_all, drop_one):
    """Have ``params_changed()`` call ``drop_all()`` and ``drop_cached_weight_t(params)`` call
    ``drop_one(p)`` for each of its parameters (a feature module, once, at import)."""
    _WEIGHT_CACHES.append((drop_all, drop_one))


def params_changed():
    """Invalidate every cached W^T and FP8 q(W) (call before any out-of-autograd parameter write)."""
    _WT_CACHE.clear()
    WEIGHTS_EPOCH[0] += 1           # the Switch experts' W^T buffers (moe_weight_t_tables) refill
    for drop_all, _ in _WEIGHT_CACHES:
        drop_all()


def drop_cached_weight_t(params):
    """Forget the W^T of these parameters (ZeRO-3 frees a gathered bucket: its transposes must go
    with it, or the cache would end up holding a full bf16 copy of the model on every rank)."""
    WEIGHTS_EPOCH[0] += 1
    for p in params:
        _WT_CACHE.pop(id(p), None)
        for _, drop_one in _WEIGHT_CACHES:
            drop_one(p)      # q(W) and q(W)^T go with the gathered weight too


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
