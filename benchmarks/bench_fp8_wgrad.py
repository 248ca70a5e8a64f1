"""FP8 weight-gradient GEMM (csrc/kernels/wgrad_fp8.hip, --fp8-wgrad) against the 16-bit grouped
wgrad of the same tree, on the GPT-2 345M layer shapes at M = 65,536 tokens (micro-batch 64 x 1024).

Each shape singly (one grouped launch of one problem) and the group the deferred queue issues
(``--layers`` layers of QKV / proj / fc1 / fc2 in one launch). The two sides alternate within a
round; every round is printed and the median reported, with the operand bytes per second each side
achieves (bytes = M (N + K) x element size, each operand counted once: re-reads by the tiles that
share a strip are not counted). One JSON line per case.

    python benchmarks/bench_fp8_wgrad.py [--rounds 5] [--iters 10] [--layers 5] [--m 65536]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from smdt_amd.ops import _ext  # noqa: E402

SHAPES = {"qkv": (3072, 1024), "proj": (1024, 1024), "fc1": (4096, 1024), "fc2": (1024, 4096)}


def timeit(fn, iters):
    fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3  # us


def problems(M, names, fmt):
    out = []
    for name in names:
        N, K = SHAPES[name]
        dy = torch.randn(M, N, device="cuda", dtype=torch.bfloat16)
        x = torch.randn(M, K, device="cuda", dtype=torch.bfloat16)
        out.append(dict(N=N, K=K, dy=dy, x=x, qdy=dy.to(fmt), qx=x.to(torch.float8_e4m3fn),
                        mg16=torch.zeros(N, K, device="cuda"), mg8=torch.zeros(N, K, device="cuda")))
    return out


def case(label, probs, M, rounds, iters):
    C = _ext.ext()
    one = torch.ones(1, device="cuda")
    n = len(probs)
    mg16, dys, xs = [p["mg16"] for p in probs], [p["dy"] for p in probs], [p["x"] for p in probs]
    mg8, qdys, qxs = [p["mg8"] for p in probs], [p["qdy"] for p in probs], [p["qx"] for p in probs]

    def bf16():
        assert C.wgrad_grouped(mg16, dys, xs)

    def fp8():
        assert C.wgrad_fp8_grouped(mg8, qdys, qxs, [one] * n, [one] * n)

    t16, t8 = [], []
    for _ in range(rounds):
        t16.append(timeit(bf16, iters))
        t8.append(timeit(fp8, iters))
    elems = sum(M * (p["N"] + p["K"]) for p in probs)
    flops = sum(2.0 * M * p["N"] * p["K"] for p in probs)
    m16, m8 = statistics.median(t16), statistics.median(t8)
    print(json.dumps({
        "case": label, "M": M, "problems": n,
        "bf16_us_rounds": [round(t, 1) for t in t16], "fp8_us_rounds": [round(t, 1) for t in t8],
        "bf16_us": round(m16, 1), "fp8_us": round(m8, 1), "fp8_over_bf16": round(m8 / m16, 3),
        "bf16_tflops": round(flops / m16 / 1e6, 1), "fp8_tflops": round(flops / m8 / 1e6, 1),
        "bf16_operand_TBps": round(2 * elems / m16 / 1e6, 3), "fp8_operand_TBps": round(elems / m8 / 1e6, 3),
    }), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--layers", type=int, default=5)
    ap.add_argument("--m", type=int, default=65536)
    ap.add_argument("--e4m3", action="store_true", help="E4M3 dY (--fp8-e4m3) instead of E5M2 (--fp8-hybrid)")
    a = ap.parse_args()
    fmt = torch.float8_e4m3fn if a.e4m3 else torch.float8_e5m2
    torch.manual_seed(0)
    for name in SHAPES:
        case(name, problems(a.m, [name], fmt), a.m, a.rounds, a.iters)
    if a.layers > 0:
        case(f"group_{a.layers}_layers", problems(a.m, list(SHAPES) * a.layers, fmt), a.m, a.rounds, a.iters)


if __name__ == "__main__":
    main()
