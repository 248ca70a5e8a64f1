"""Weight formats for text generation: the ``decode_weights`` context, the cached MXFP8 / MXFP4
copies of the weights (``_DECODE_WQ``, registered with ``dense.register_weight_cache``) and the
route a linear takes inside the context (``_decode_route``).

Feature layer: built on ``dense``; tensor_parallel's dispatcher sends linears here and this module
does not import it.
"""
from __future__ import annotations

import weakref
from typing import Optional

import torch

from ..ops import functional as SF
from . import dense
from .dense import linear_rows

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
    key = (weight.data_ptr(), weight._version, tuple(weight.shape), weight.dtype, dense.WEIGHTS_EPOCH[0], fmt)
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


dense.register_weight_cache(_DECODE_WQ.clear, lambda p: _DECODE_WQ.pop(id(p), None))
