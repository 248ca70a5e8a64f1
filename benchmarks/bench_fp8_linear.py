"""FP8 linear against the 16-bit linear at the GPT-2 345M step shapes (65,536 tokens): forward +
dgrad per linear, the FP8 side INCLUDING the activation and gradient quantise passes
(fp8_quant.hip). The weight quantise (q(W) and q(W)^T in one pass) is amortised over an optimizer
step and reported separately. bf16 goes through ``linear_rows`` / ``dgrad`` with the cached W^T,
as the training step does, with the TunableOp table loaded as in bench.py.

The two sides alternate (bf16, fp8, bf16, fp8, ...) so clock and temperature drift hit both;
each round is the median of ``--iters`` timed calls and the JSON line per shape carries every
round, so the repeat spread is visible."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--fp8", choices=["hybrid", "e4m3"], default="hybrid")
    ap.add_argument("--no-tunable", action="store_true")
    a = ap.parse_args()
    table = os.path.join(ROOT, "profiles", "tunableop", "gfx950_gpt345m_results.csv")
    if not a.no_tunable and os.path.exists(table):
        import torch.cuda.tunable as tun
        tun.enable(True)
        tun.tuning_enable(False)
        tun.read_file(table)
    from smdt_amd.ops import functional as SF
    from smdt_amd.parallel import tensor_parallel as tp
    M, dt = a.m, torch.bfloat16
    gfmt = "e5m2" if a.fp8 == "hybrid" else "e4m3"
    tot = {"bf16": 0.0, "fp8": 0.0}
    for name, O, I in (("qkv", 3072, 1024), ("proj", 1024, 1024), ("fc1", 4096, 1024), ("fc2", 1024, 4096)):
        x = torch.randn(M, I, device="cuda", dtype=dt)
        dy = torch.randn(M, O, device="cuda", dtype=dt) * 1e-3
        w = torch.randn(O, I, device="cuda", dtype=dt) * 0.02
        wt = tp._dgrad_weight_t(w)
        # scales as delayed scaling would set them
        sc = torch.stack([448.0 / x.float().abs().max(), 448.0 / w.float().abs().max(),
                          SF.FP8_MAX[gfmt] / dy.float().abs().max()]).float()
        inv = sc.reciprocal()
        amax = torch.zeros(3, device="cuda")
        qw, qwt = SF.fp8_quantize(w, sc[1:2], amax[1:2], "e4m3", transpose=True)

        def bf16():
            tp.linear_rows(x, w)
            tp.dgrad(dy, w, wt)

        def fp8():
            qx = SF.fp8_quantize(x, sc[0:1], amax[0:1], "e4m3")
            SF.fp8_gemm(qx, qw, inv[0:1], inv[1:2], None, dt)
            qg = SF.fp8_quantize(dy, sc[2:3], amax[2:3], gfmt)
            SF.fp8_gemm(qg, qwt, inv[2:3], inv[1:2], None, dt)

        def fp8_gemms():
            SF.fp8_gemm(qx0, qw, inv[0:1], inv[1:2], None, dt)
            SF.fp8_gemm(qg0, qwt, inv[2:3], inv[1:2], None, dt)

        qx0 = SF.fp8_quantize(x, sc[0:1], amax[0:1], "e4m3")
        qg0 = SF.fp8_quantize(dy, sc[2:3], amax[2:3], gfmt)
        # sanity: the FP8 output is the 16-bit output up to quantisation error
        y16, y8 = tp.linear_rows(x, w).float(), SF.fp8_gemm(qx0, qw, inv[0:1], inv[1:2], None, dt).float()
        rel = ((y8 - y16).norm() / y16.norm()).item()
        rounds = {"bf16": [], "fp8": []}
        for _ in range(a.rounds):
            rounds["bf16"].append(median_ms(bf16, a.iters))
            rounds["fp8"].append(median_ms(fp8, a.iters))
        t_g = median_ms(fp8_gemms, a.iters)
        t_qx = median_ms(lambda: SF.fp8_quantize(x, sc[0:1], amax[0:1], "e4m3"), a.iters)
        t_qg = median_ms(lambda: SF.fp8_quantize(dy, sc[2:3], amax[2:3], gfmt), a.iters)
        t_qw = median_ms(lambda: SF.fp8_quantize(w, sc[1:2], amax[1:2], "e4m3", transpose=True), a.iters)
        t_tr = median_ms(lambda: tp._ext.ext().transpose2d(w), a.iters)
        med = {k: sorted(v)[len(v) // 2] for k, v in rounds.items()}
        for k in tot:
            tot[k] += med[k]
        print(json.dumps({
            "linear": name, "M": M, "out": O, "in": I, "fp8": a.fp8,
            "bf16_fwd_dgrad_ms": round(med["bf16"], 4), "fp8_fwd_dgrad_with_quant_ms": round(med["fp8"], 4),
            "speedup": round(med["bf16"] / med["fp8"], 3),
            "bf16_rounds_ms": [round(v, 4) for v in rounds["bf16"]],
            "fp8_rounds_ms": [round(v, 4) for v in rounds["fp8"]],
            "fp8_gemms_only_ms": round(t_g, 4), "quant_x_ms": round(t_qx, 4), "quant_dy_ms": round(t_qg, 4),
            "quant_x_GBps": round(x.numel() * 3 / t_qx / 1e6, 1), "quant_dy_GBps": round(dy.numel() * 3 / t_qg / 1e6, 1),
            "weight_quant_per_step_ms": round(t_qw, 4), "bf16_weight_transpose_per_step_ms": round(t_tr, 4),
            "fp8_vs_bf16_output_rel_err": round(rel, 5)}), flush=True)
        del x, dy, w, wt, qw, qwt, qx0, qg0, y16, y8
    print(json.dumps({"total_bf16_ms": round(tot["bf16"], 4), "total_fp8_ms": round(tot["fp8"], 4),
                      "speedup": round(tot["bf16"] / tot["fp8"], 3), "layers_per_step": 24}), flush=True)


if __name__ == "__main__":
    main()
