"""Incremental decoding benchmark (not bench.py's flagship workload).

Kernel: time and effective K/V bandwidth of ``ops.functional.decode_attention`` (decode_attn.hip)
against ``torch.nn.functional.scaled_dot_product_attention`` on the same cache, with the K/V head
expansion SDPA needs under GQA, in the same process, alternating which runs first. Bytes are the
cache bytes the algorithm needs (2 * B * S * nkv * D * 2), computed here from the shape.

End to end: new tokens/s of ``generate`` on random-init built-in models, eager against
``use_graph=True`` (the prefill-only time, a 1-token call, is subtracted).

Linear (``--linear``): per decode-step GEMM shape of LLaMA-7B and OPT-125m and per M, the library
path (``F.linear``, what a decode step calls without ``weight_format``) against
``ops.functional.decode_linear`` (decode_linear.hip) in each weight format. Every timed call reads
another copy of the weight out of a ring larger than the chip's last-level cache, as a decode step
does (it streams every layer's weights once); bytes are the weight bytes of the format (elements
plus scale bytes), computed here from the shape.

``--e2e --weight-format F[,F...]`` adds ``generate(weight_format=F)`` beside the parent path (no
format), alternating, with ``use_graph=True``.

``--kv-format mxfp8`` (with ``--kernel``): ``decode_attention_mx`` (decode_attn_mx.hip) on an MXFP8
cache against ``decode_attention`` on the 16-bit cache of the same shape, same protocol; bytes are
2 * B * S * nkv * (D + D / 32). With ``--e2e``: ``generate(kv_cache_format=...)`` beside the 16-bit
cache on LLaMA-7B with a long prompt (``--kv-e2e B:S[,B:S...]``, default 8:3968,64:3968; Llama-2-7B geometry, 4096 positions).

    python benchmarks/bench_decode.py [--kernel] [--e2e] [--linear] [--weight-format native,mxfp8,mxfp4]
                                      [--kv-format mxfp8] [--kv-e2e 8:4096]
                                      [--only llama-7b:8:4096] [--out decode.jsonl] [--quick]

``--speculative``: the multi-token decode step and speculative ``generate`` (same protocol: device
events, alternating order, minimum of four): ``decode_attention_multi`` (decode_attn_multi.hip) at
T = 1, 2, 4, 8 against T calls of ``decode_attention`` and against SDPA with the tail mask;
``forward_extend(T)`` against ``forward_decode`` on LLaMA-7B at B 1 / 2 under each weight format; one
whole speculative round (OPT-125m-sized draft with the target's vocabulary, graph replay) against
the plain decode step, with the break-even number of accepted drafts per round that follows from the
two times; and a self-draft ``generate`` on OPT-125m for the accounting. Random-init pairs accept
almost nothing, so no tokens/s gain of a real pair is measured here.

One JSON line per measurement. Needs a GPU: there is no CPU fallback for a timing.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

HBM_PEAK = 8.0e12           # spec; ~6.3e12 is what a streaming copy reaches on the MI355X
GEOMETRIES = {"llama-7b": (32, 32, 128), "gqa-32-8": (32, 8, 128), "opt-125m": (12, 12, 64)}


def _time(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e-3 / reps


def bench_kernel(emit, quick=False, only=None):
    from smdt_amd.ops import functional as SF
    dev = torch.device("cuda", 0)
    for name, (nh, nkv, D) in GEOMETRIES.items():
        for B in (1, 8, 64):
            for S in (1024, 4096, 16384):
                if quick and (B, S) not in ((1, 1024), (8, 4096)):
                    continue
                if only and only != f"{name}:{B}:{S}":
                    continue
                q = torch.empty(B, nh, D, device=dev, dtype=torch.bfloat16).normal_()
                k = torch.empty(B, S, nkv, D, device=dev, dtype=torch.bfloat16).normal_()
                v = torch.empty(B, S, nkv, D, device=dev, dtype=torch.bfloat16).normal_()
                lens = torch.full((B,), S, dtype=torch.int32, device=dev)
                scale = 1.0 / math.sqrt(D)
                rep = nh // nkv

                def ours():
                    return SF.decode_attention(q, k, v, lens, scale)

                def sdpa():
                    kk, vv = k.transpose(1, 2), v.transpose(1, 2)              # [B, nkv, S, D] views
                    if rep > 1:                                                # the expansion SDPA needs
                        kk, vv = kk.repeat_interleave(rep, dim=1), vv.repeat_interleave(rep, dim=1)
                    return F.scaled_dot_product_attention(q.unsqueeze(2), kk, vv, scale=scale).squeeze(2)

                diff = (ours().float() - sdpa().float()).abs().max().item()
                nbytes = 2 * B * S * nkv * D * 2
                reps = max(5, min(200, int(0.1 / max(nbytes / 4e12, 2e-5))))
                for fn in (ours, sdpa):                                        # warm up both
                    _time(fn, 3)
                t = {"ours": [], "sdpa": []}
                for r in range(4):                                             # alternate the order
                    order = (("ours", ours), ("sdpa", sdpa)) if r % 2 == 0 else (("sdpa", sdpa), ("ours", ours))
                    for n, fn in order:
                        t[n].append(_time(fn, reps))
                to, ts = min(t["ours"]), min(t["sdpa"])
                emit({"bench": "decode_attention", "geometry": name, "nh": nh, "nkv": nkv, "D": D, "B": B, "S": S,
                      "kv_bytes": nbytes, "ours_us": to * 1e6, "sdpa_us": ts * 1e6, "sdpa_over_ours": ts / to,
                      "ours_GBps": nbytes / to / 1e9, "hbm_peak_frac": nbytes / to / HBM_PEAK,
                      "ours_runs_us": [x * 1e6 for x in t["ours"]], "sdpa_runs_us": [x * 1e6 for x in t["sdpa"]],
                      "max_abs_diff": diff, "reps": reps})
                del q, k, v
                torch.cuda.empty_cache()


def bench_kernel_kv(emit, fmt, quick=False, only=None):
    """``decode_attention_mx`` on an MXFP8 cache against ``decode_attention`` on the 16-bit cache."""
    from smdt_amd.ops import functional as SF
    assert fmt in SF.KV_CACHE_FORMATS, fmt
    dev = torch.device("cuda", 0)
    for name, (nh, nkv, D) in GEOMETRIES.items():
        for B in (1, 8, 64):
            for S in (1024, 4096, 16384):
                if quick and (B, S) not in ((1, 1024), (8, 4096)):
                    continue
                if only and only != f"{name}:{B}:{S}":
                    continue
                q = torch.empty(B, nh, D, device=dev, dtype=torch.bfloat16).normal_()
                k = torch.empty(B, S, nkv, D, device=dev, dtype=torch.bfloat16).normal_()
                v = torch.empty(B, S, nkv, D, device=dev, dtype=torch.bfloat16).normal_()
                kq = torch.empty(B, S, nkv, D, device=dev, dtype=torch.float8_e4m3fn)
                vq = torch.empty_like(kq)
                ks = torch.empty(B, S, nkv, D // 32, device=dev, dtype=torch.uint8)
                vs = torch.empty_like(ks)
                SF.kv_store_mx(k, v, kq, ks, vq, vs)
                lens = torch.full((B,), S, dtype=torch.int32, device=dev)
                scale = 1.0 / math.sqrt(D)

                def base():
                    return SF.decode_attention(q, k, v, lens, scale)

                def mx():
                    return SF.decode_attention_mx(q, kq, ks, vq, vs, lens, scale)

                diff = (mx().float() - base().float()).abs().max().item()
                b16, bmx = 2 * B * S * nkv * D * 2, 2 * B * S * nkv * (D + D // 32)
                reps = max(5, min(200, int(0.1 / max(b16 / 4e12, 2e-5))))
                for fn in (base, mx):
                    _time(fn, 3)
                t = {"bf16": [], fmt: []}
                for r in range(4):                                             # alternate the order
                    order = (("bf16", base), (fmt, mx)) if r % 2 == 0 else ((fmt, mx), ("bf16", base))
                    for n, fn in order:
                        t[n].append(_time(fn, reps))
                tb, tm = min(t["bf16"]), min(t[fmt])
                emit({"bench": "decode_attention_kv_format", "kv_format": fmt, "geometry": name, "nh": nh, "nkv": nkv,
                      "D": D, "B": B, "S": S, "kv_bytes_16bit": b16, "kv_bytes": bmx, "bf16_us": tb * 1e6,
                      "mx_us": tm * 1e6, "bf16_over_mx": tb / tm, "bf16_GBps": b16 / tb / 1e9, "mx_GBps": bmx / tm / 1e9,
                      "bf16_runs_us": [x * 1e6 for x in t["bf16"]], "mx_runs_us": [x * 1e6 for x in t[fmt]],
                      "max_abs_diff_vs_16bit_cache": diff, "reps": reps})
                del q, k, v, kq, ks, vq, vs
                torch.cuda.empty_cache()


def bench_e2e_kv(emit, fmt, cases, new=65):
    """``generate`` (graph replay) on LLaMA-7B with the 16-bit cache and with ``fmt``, alternating;
    the prefill-only time (a 1-token call) is subtracted. Reports the cache bytes allocated."""
    from smdt_amd.models.generation import KVCache
    from smdt_amd.models.hf import HFCausalLM
    dev = torch.device("cuda", 0)
    model = HFCausalLM.from_pretrained("meta-llama/Llama-2-7b-hf", params_dtype=torch.bfloat16, device=dev).eval()
    for B, S in cases:
        ids = torch.randint(3, 30000, (B, S), device=dev)
        arms = [None, fmt]
        caches = {f: KVCache(model.model.cfg, B, S + new, device=dev, format=f) for f in arms}
        nbytes = {f: sum(t.numel() * t.element_size() for t in c.k + c.v + getattr(c, "k_scale", []) +
                         getattr(c, "v_scale", [])) for f, c in caches.items()}

        def run(f, n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.generate(ids, max_new_tokens=n, eos_token_id=None, use_graph=True, cache=caches[f])
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        for f in arms:
            run(f, new)
        full = {f: [] for f in arms}
        pre = {f: [] for f in arms}
        for r in range(2):
            for f in (arms if r % 2 == 0 else arms[::-1]):
                full[f].append(run(f, new))
                pre[f].append(run(f, 1))
        base = None
        for f in arms:
            step = (min(full[f]) - min(pre[f])) / (new - 1)
            base = step if f is None else base
            emit({"bench": "generate_kv_cache_format", "model": "llama-2-7b", "B": B, "prompt": S, "new_tokens": new,
                  "kv_cache_format": f, "use_graph": True, "cache_bytes": nbytes[f], "ms_per_step": 1e3 * step,
                  "decode_tokens_per_s": B / step, "over_16bit": base / step, "calls_s": full[f],
                  "prefill_calls_s": pre[f]})
        del caches
        torch.cuda.empty_cache()


LINEAR_SHAPES = {      # (N, K) of the decode step's GEMMs
    "llama-7b": {"qkv": (12288, 4096), "proj": (4096, 4096), "fc1": (22016, 4096), "fc2": (4096, 11008),
                 "head": (32000, 4096)},
    "opt-125m": {"qkv": (2304, 768), "proj": (768, 768), "fc1": (3072, 768), "fc2": (768, 3072),
                 "head": (50272, 768)},
}
COPY_RATE = 6.3e12          # what a streaming copy reaches (the yardstick of the fractions below)
RING_BYTES = 768 << 20      # per format: beyond the 256 MB last-level cache several times over


def _weight_bytes(N, K, fmt):
    return N * K * 2 if fmt == "native" else N * K // (1 if fmt == "mxfp8" else 2) + N * K // 32


def bench_linear(emit, quick=False, only=None):
    from smdt_amd.ops import functional as SF
    dev = torch.device("cuda", 0)
    fmts = list(SF.DECODE_LINEAR_FORMATS)
    for model, shapes in LINEAR_SHAPES.items():
        for lname, (N, K) in shapes.items():
            if only and only != f"{model}:{lname}":
                continue
            if quick and lname not in ("proj", "fc2"):
                continue
            ncopy = max(2, min(256, RING_BYTES // (N * K * 2)))
            ws16 = [torch.empty(N, K, device=dev, dtype=torch.bfloat16).normal_(0, 0.02) for _ in range(ncopy)]
            q8, s8 = SF.decode_weight_quantize(ws16[0], "mxfp8")
            q4, s4 = SF.decode_weight_quantize(ws16[0], "mxfp4")
            ring = {"native": [(w, None) for w in ws16],
                    "mxfp8": [(q8.clone(), s8.clone()) for _ in range(max(2, min(256, RING_BYTES // (N * K))))],
                    "mxfp4": [(q4.clone(), s4.clone()) for _ in range(max(2, min(256, 2 * RING_BYTES // (N * K))))]}
            for M in (1, 2, 4, 8, 16):
                x = torch.empty(M, K, device=dev, dtype=torch.bfloat16).normal_()
                wsp = {f: (torch.empty(n, dtype=torch.float32, device=dev) if n else None)
                       for f in fmts for n in [SF.decode_linear_workspace_numel(M, N, K, f)]}
                pos = {"lib": 0, **{f: 0 for f in fmts}}

                def lib():
                    pos["lib"] = (pos["lib"] + 1) % len(ws16)
                    return F.linear(x, ws16[pos["lib"]])

                def ours(f):
                    def run():
                        pos[f] = (pos[f] + 1) % len(ring[f])
                        w, sc = ring[f][pos[f]]
                        return SF.decode_linear(x, w, sc, None, f, wsp[f])
                    return run
                fns = {"lib": lib, **{f: ours(f) for f in fmts}}
                ref = F.linear(x, ws16[0]).float()
                diff = {f: (SF.decode_linear(x, *ring[f][0], None, f, wsp[f]).float() - ref).abs().max().item()
                        for f in fmts}
                reps = max(20, min(400, int(0.05 / max(N * K * 2 / 2.5e12, 1e-5))))
                for fn in fns.values():
                    _time(fn, 5)
                t = {n: [] for n in fns}
                names = list(fns)
                for r in range(4):                                             # alternate the order
                    for n in (names if r % 2 == 0 else names[::-1]):
                        t[n].append(_time(fns[n], reps))
                best = {n: min(v) for n, v in t.items()}
                rec = {"bench": "decode_linear", "model": model, "linear": lname, "N": N, "K": K, "M": M,
                       "reps": reps, "ring_copies": {"native": len(ws16), "mxfp8": len(ring["mxfp8"]),
                                                     "mxfp4": len(ring["mxfp4"])},
                       "splits": {f: SF.decode_linear_plan(N, K, f)[0] for f in fmts},
                       "lib_us": best["lib"] * 1e6, "lib_GBps": _weight_bytes(N, K, "native") / best["lib"] / 1e9,
                       "max_abs_diff_vs_lib": diff, "runs_us": {n: [x_ * 1e6 for x_ in v] for n, v in t.items()}}
                for f in fmts:
                    b = _weight_bytes(N, K, f)
                    rec[f + "_us"] = best[f] * 1e6
                    rec[f + "_GBps"] = b / best[f] / 1e9
                    rec[f + "_copy_rate_frac"] = b / best[f] / COPY_RATE
                    rec["lib_over_" + f] = best["lib"] / best[f]
                emit(rec)
            del ws16, ring
            torch.cuda.empty_cache()


def bench_e2e_formats(emit, models, formats, quick=False):
    """``generate`` (graph replay) on the parent path and under each weight format, alternating."""
    from smdt_amd.models.hf import HFCausalLM
    dev = torch.device("cuda", 0)
    prompt, new = (32, 33) if quick else (128, 129)
    for name in models:
        model = HFCausalLM.from_pretrained(name, params_dtype=torch.bfloat16, device=dev).eval()
        for B in (1, 8):
            ids = torch.randint(3, 30000, (B, prompt), device=dev)

            def run(fmt, n):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                model.generate(ids, max_new_tokens=n, eos_token_id=None, use_graph=True, weight_format=fmt)
                torch.cuda.synchronize()
                return time.perf_counter() - t0
            arms = [None] + list(formats)
            for f in arms:
                run(f, new)                                 # warm up every shape, quantise once
            full = {f: [] for f in arms}
            pre = {f: [] for f in arms}
            for r in range(3):
                for f in (arms if r % 2 == 0 else arms[::-1]):
                    run(f, 1)                               # a weight keeps one copy: re-made here, untimed
                    full[f].append(run(f, new))
                    pre[f].append(run(f, 1))
            base = None
            for f in arms:
                tps = B * (new - 1) / (min(full[f]) - min(pre[f]))
                base = tps if f is None else base
                emit({"bench": "generate_weight_format", "model": name, "B": B, "prompt": prompt, "new_tokens": new,
                      "weight_format": f, "use_graph": True, "call_s": min(full[f]), "prefill_call_s": min(pre[f]),
                      "decode_tokens_per_s": tps, "ms_per_step": 1e3 * (min(full[f]) - min(pre[f])) / (new - 1),
                      "over_parent": tps / base, "calls_s": full[f]})
        del model
        torch.cuda.empty_cache()


def bench_e2e(emit, models, quick=False):
    from smdt_amd.models.hf import HFCausalLM
    dev = torch.device("cuda", 0)
    prompt, new = (32, 33) if quick else (128, 129)
    for name in models:
        model = HFCausalLM.from_pretrained(name, params_dtype=torch.bfloat16, device=dev).eval()
        for B in (1, 8):
            ids = torch.randint(3, 30000, (B, prompt), device=dev)
            res = {}
            for graph in (False, True):
                def run(n):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    model.generate(ids, max_new_tokens=n, eos_token_id=None, use_graph=graph)
                    torch.cuda.synchronize()
                    return time.perf_counter() - t0
                run(new)                                    # warm up every shape
                full = min(run(new) for _ in range(2))
                pre = min(run(1) for _ in range(2))
                res["graph" if graph else "eager"] = B * (new - 1) / (full - pre)
                emit({"bench": "generate", "model": name, "B": B, "prompt": prompt, "new_tokens": new,
                      "use_graph": graph, "call_s": full, "prefill_call_s": pre,
                      "decode_tokens_per_s": res["graph" if graph else "eager"]})
            emit({"bench": "generate_ratio", "model": name, "B": B, "graph_over_eager": res["graph"] / res["eager"]})
        del model
        torch.cuda.empty_cache()


def _alternate(arms, reps):
    """{name: min of four timings}, the arms alternating in order."""
    for fn in arms.values():
        _time(fn, 3)
    t = {n: [] for n in arms}
    names = list(arms)
    for r in range(4):
        for n in (names if r % 2 == 0 else names[::-1]):
            t[n].append(_time(arms[n], reps))
    return {n: min(v) for n, v in t.items()}


def bench_spec_kernel(emit, quick=False):
    from smdt_amd.ops import functional as SF
    dev = torch.device("cuda", 0)
    for name, (nh, nkv, D) in GEOMETRIES.items():
        for B, S in ((1, 4096), (8, 4096)) if not quick else ((1, 1024),):
            k = torch.empty(B, S, nkv, D, device=dev, dtype=torch.bfloat16).normal_()
            v = torch.empty(B, S, nkv, D, device=dev, dtype=torch.bfloat16).normal_()
            lens = torch.full((B,), S, dtype=torch.int32, device=dev)
            scale, rep = 1.0 / math.sqrt(D), nh // nkv
            for T in (1, 2, 4, 8):
                q = torch.empty(B, T, nh, D, device=dev, dtype=torch.bfloat16).normal_()
                qs = [q[:, t].contiguous() for t in range(T)]
                lt = [lens - (T - 1 - t) for t in range(T)]
                mask = torch.arange(S, device=dev)[None, :] <= (S - T + torch.arange(T, device=dev))[:, None]

                def multi():
                    return SF.decode_attention_multi(q, k, v, lens, scale)

                def calls():
                    return [SF.decode_attention(qs[t], k, v, lt[t], scale) for t in range(T)]

                def sdpa():
                    kk, vv = k.transpose(1, 2), v.transpose(1, 2)
                    if rep > 1:
                        kk, vv = kk.repeat_interleave(rep, dim=1), vv.repeat_interleave(rep, dim=1)
                    return F.scaled_dot_product_attention(q.transpose(1, 2), kk, vv, attn_mask=mask, scale=scale)

                diff = (multi().float() - sdpa().transpose(1, 2).float()).abs().max().item()
                nbytes = 2 * B * S * nkv * D * 2
                reps = max(5, min(200, int(0.1 / max(nbytes / 4e12, 2e-5))))
                t = _alternate({"multi": multi, "calls": calls, "sdpa": sdpa}, reps)
                emit({"bench": "decode_attention_multi", "geometry": name, "B": B, "S": S, "T": T, "kv_bytes": nbytes,
                      "multi_us": t["multi"] * 1e6, "t_calls_us": t["calls"] * 1e6, "sdpa_us": t["sdpa"] * 1e6,
                      "t_calls_over_multi": t["calls"] / t["multi"], "sdpa_over_multi": t["sdpa"] / t["multi"],
                      "multi_GBps": nbytes / t["multi"] / 1e9, "max_abs_diff_vs_sdpa": diff, "reps": reps})
            del k, v
            torch.cuda.empty_cache()


def bench_spec_model(emit, quick=False):
    """forward_extend(T) against forward_decode, and a whole round against the plain step."""
    from smdt_amd.models import generation as G
    from smdt_amd.models.hf import BUILTIN, HFCausalLM
    from smdt_amd.parallel import tensor_parallel as tp
    from smdt_amd.train.graphs import CapturedStep
    dev = torch.device("cuda", 0)
    tname = "facebook/opt-125m" if quick else "llama-7b"
    target = HFCausalLM.from_pretrained(tname, params_dtype=torch.bfloat16, device=dev).eval()
    model, S = target.model, 128
    with torch.no_grad():
        for B in (1, 2):
            ids = torch.randint(3, 30000, (B, S), device=dev)
            plen = torch.full((B,), S, dtype=torch.int64, device=dev)
            cache = G.KVCache(model.cfg, B, S + 16, torch.bfloat16, dev)
            model.forward_prefill(ids, plen, cache)
            for fmt in (None, "native", "mxfp8", "mxfp4"):
                state = G._decode_weights(model, fmt)
                arms = {}
                for T in (1, 2, 5, 8):
                    toks = torch.randint(3, 30000, (B, T), device=dev)

                    def ext(T=T, toks=toks):
                        cache.lens.fill_(S)
                        cache.advance(T)
                        return model.forward_extend(toks, cache)
                    arms[f"extend{T}"] = ext

                def dec(tok=torch.randint(3, 30000, (B,), device=dev)):
                    cache.lens.fill_(S)
                    cache.advance()
                    return model.forward_decode(tok, cache)
                arms["decode"] = dec
                with tp.decode_weights(state):
                    t = _alternate(arms, 10)
                emit({"bench": "forward_extend", "model": tname, "B": B, "S": S, "weight_format": fmt,
                      "decode_ms": t["decode"] * 1e3,
                      **{f"extend{T}_ms": t[f"extend{T}"] * 1e3 for T in (1, 2, 5, 8)},
                      **{f"extend{T}_over_decode": t[f"extend{T}"] / t["decode"] for T in (1, 2, 5, 8)}})
        # one whole round (graph replay) against the plain step (graph replay), B = 1, k = 4
        vocab = target.vocab_size
        draft = HFCausalLM(dict(BUILTIN["facebook/opt-125m"], vocab_size=vocab), params_dtype=torch.bfloat16,
                           device=dev).eval()
        for fmt in (None, "mxfp4"):
            state = G._decode_weights(model, fmt)
            ids = torch.randint(3, 30000, (1, S), device=dev)
            for k in (2, 4, 7):
                st = G.SpeculativeState(model, draft.model, ids, None, 1500, k, None, 0, None, state)
                rnd = CapturedStep(st.round, warmup=1)
                cache = G.KVCache(model.cfg, 1, S + 1500, torch.bfloat16, dev)
                model.forward_prefill(ids, torch.full((1,), S, dtype=torch.int64, device=dev), cache)
                cache.lens.fill_(S)

                def plain(tok):
                    cache.advance()
                    with tp.decode_weights(state):
                        return model.forward_decode(tok, cache)[:, :vocab].argmax(-1)
                stp = CapturedStep(plain, warmup=1)
                x = {"r": st.x0, "p": st.x0.clone()}

                def one_round():
                    x["r"] = rnd(x["r"])

                def one_step():
                    x["p"] = stp(x["p"])
                for _ in range(3):
                    one_round(), one_step()
                assert rnd.note == "captured" and stp.note == "captured", (rnd.note, stp.note)
                t = _alternate({"round": one_round, "step": one_step}, 10)
                emit({"bench": "speculative_round", "target": tname, "draft": "opt-125m-sized", "B": 1, "k": k,
                      "weight_format": fmt, "round_ms": t["round"] * 1e3, "plain_step_ms": t["step"] * 1e3,
                      "round_over_step": t["round"] / t["step"],
                      # a round emits accepted + 1 tokens: it pays once accepted + 1 > round / step
                      "break_even_accepted_per_round": t["round"] / t["step"] - 1.0})
                del st, rnd, stp, cache
                torch.cuda.empty_cache()
        del target, model, draft
        torch.cuda.empty_cache()
        # the accounting on a self-draft: every draft is accepted, k + 1 tokens per round
        m = HFCausalLM.from_pretrained("facebook/opt-125m", params_dtype=torch.bfloat16, device=dev).eval()
        ids = torch.randint(3, 30000, (1, S), device=dev)
        new = 33 if quick else 129

        def run(n, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = m.generate(ids, max_new_tokens=n, eos_token_id=None, use_graph=True, **kw)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out
        stats = {}
        spec = dict(draft_model=m, num_draft_tokens=4)
        run(new), run(new, **spec)
        tp_, op = min(run(new)[0] for _ in range(3)), run(new)[1]
        ts_, os_ = min(run(new, **spec)[0] for _ in range(3)), run(new, stats=stats, **spec)[1]
        emit({"bench": "generate_self_draft", "model": "facebook/opt-125m", "B": 1, "k": 4, "new_tokens": new,
              "plain_call_s": tp_, "speculative_call_s": ts_, "tokens_equal": bool(torch.equal(op, os_)), **stats,
              "acceptance": stats["accepted"] / max(stats["drafted"], 1)})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--linear", action="store_true", help="decode_linear against F.linear per shape and M")
    ap.add_argument("--speculative", action="store_true", help="the multi-token step and speculative generate")
    ap.add_argument("--weight-format", default=None,
                    help="with --e2e: comma-separated weight formats to run beside the parent path")
    ap.add_argument("--kv-format", default=None, help="with --kernel: decode_attention_mx against decode_attention; "
                    "with --e2e: generate(kv_cache_format=...) against the 16-bit cache on LLaMA-7B")
    ap.add_argument("--kv-e2e", default="8:3968,64:3968", help="B:S cases of --e2e --kv-format")
    ap.add_argument("--models", default="facebook/opt-125m,llama-7b")
    ap.add_argument("--quick", action="store_true", help="two small shapes only (a rehearsal)")
    ap.add_argument("--only", default=None, help="one kernel shape, geometry:B:S (e.g. for a profiler run); "
                    "with --linear, model:linear (llama-7b:fc2)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode.py measures on the GPU; none is visible")
    out = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    both = not (args.kernel or args.e2e or args.linear)
    with torch.no_grad():
        if args.speculative:
            if args.kernel or both:
                bench_spec_kernel(emit, args.quick)
            if args.e2e or both:
                bench_spec_model(emit, args.quick)
            return
        if args.kv_format:
            if args.kernel or both:
                bench_kernel_kv(emit, args.kv_format, args.quick, args.only)
            if args.e2e:
                bench_e2e_kv(emit, args.kv_format, [tuple(int(x) for x in c.split(":")) for c in args.kv_e2e.split(",")])
            return
        if args.kernel or both:
            bench_kernel(emit, args.quick, args.only)
        if args.linear:
            bench_linear(emit, args.quick, args.only)
        if args.e2e and args.weight_format:
            bench_e2e_formats(emit, [m for m in args.models.split(",") if m],
                              [f for f in args.weight_format.split(",") if f], args.quick)
        elif args.e2e or both:
            bench_e2e(emit, [m for m in args.models.split(",") if m], args.quick)


if __name__ == "__main__":
    main()
