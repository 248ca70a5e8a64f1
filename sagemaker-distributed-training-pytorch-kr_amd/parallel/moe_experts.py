"""The grouped Switch experts at TP = 1 (--moe-grouped-gemm): ``GroupedSwitchExperts``, its ranged
weight gradients and the persistent per-expert W^T buffers (``_MOE_WT``), which refill when
``dense.WEIGHTS_EPOCH`` has advanced.

Feature layer: built on ``dense``; it does not import tensor_parallel.
"""
from __future__ import annotations

import torch

from ..ops import _ext
from ..ops import functional as SF
from . import dense
from .dense import _fire


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
        if dense.DEFERRED_WGRAD.eligible(mg, g2, t2):
            dense.DEFERRED_WGRAD.push(weight, mg, g2, t2, bias=bias_p, mrange=(seg, e))
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
    stamp = (dense.WEIGHTS_EPOCH[0], tuple(w._version for w in weights))
    if hit["stamp"] != stamp:
        with torch.no_grad():
            for wt, w in zip(hit["wts"], weights):
                wt.copy_(w.detach().t())
        hit["stamp"] = stamp
    return hit["wts"], hit["tabs"]
