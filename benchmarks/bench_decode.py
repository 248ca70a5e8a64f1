"""Incremental decoding benchmark (not bench.py's flagship workload).

Kernel: time and effective K/V bandwidth of ``ops.functional.decode_attention`` (decode_attn.hip)
against ``torch.nn.functional.scaled_dot_product_attention`` on the same cache, with the K/V head
expansion SDPA needs under GQA, in the same process, alternating which runs first. Bytes are the
cache bytes the algorithm needs (2 * B * S * nkv * D * 2), computed here from the shape.

End to end: new tokens/s of ``generate`` on random-init built-in models, eager against
``use_graph=True`` (the prefill-only time, a 1-token call, is subtracted).

    python benchmarks/bench_decode.py [--kernel] [--e2e] [--only llama-7b:8:4096] [--out decode.jsonl] [--quick]

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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--models", default="facebook/opt-125m,llama-7b")
    ap.add_argument("--quick", action="store_true", help="two small shapes only (a rehearsal)")
    ap.add_argument("--only", default=None, help="one kernel shape, geometry:B:S (e.g. for a profiler run)")
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

    both = not (args.kernel or args.e2e)
    with torch.no_grad():
        if args.kernel or both:
            bench_kernel(emit, args.quick, args.only)
        if args.e2e or both:
            bench_e2e(emit, [m for m in args.models.split(",") if m], args.quick)


if __name__ == "__main__":
    main()
