"""MXFP8 linear (--fp8-recipe mxfp8) against the delayed-scaling FP8 linear and the 16-bit linear
at the GPT-2 345M step shapes (65,536 tokens, h 1024): forward + dgrad per linear, both FP8 sides
INCLUDING their activation and gradient quantise passes (mx_quant.hip / fp8_quant.hip); the weight
quantise is amortised over an optimizer step and reported separately. Then the GEMMs alone:
``gemm_mx`` (gemm_mx.hip, the block-scaled MFMA), hipBLASLt's per-tensor FP8 GEMM and ``gemm_tn``.

The sides alternate (bf16, delayed, mxfp8, bf16, ...) so clock and temperature drift hit all of
them; each round is the median of ``--iters`` timed calls and the JSON line per shape carries every
round, so the repeat spread is visible."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchmarks.bench_fp8_linear import median_ms  # noqa: E402


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
    from smdt_amd.ops import _ext
    from smdt_amd.ops import functional as SF
    from smdt_amd.parallel import tensor_parallel as tp
    C = _ext.ext()
    M, dt = a.m, torch.bfloat16
    gfmt = "e5m2" if a.fp8 == "hybrid" else "e4m3"
    sides = ("bf16", "delayed", "mxfp8")
    tot = {k: 0.0 for k in sides}
    for name, O, I in (("qkv", 3072, 1024), ("proj", 1024, 1024), ("fc1", 4096, 1024), ("fc2", 1024, 4096)):
        x = torch.randn(M, I, device="cuda", dtype=dt)
        dy = torch.randn(M, O, device="cuda", dtype=dt) * 1e-3
        w = torch.randn(O, I, device="cuda", dtype=dt) * 0.02
        wt = tp._dgrad_weight_t(w)
        sc = torch.stack([448.0 / x.float().abs().max(), 448.0 / w.float().abs().max(),
                          SF.FP8_MAX[gfmt] / dy.float().abs().max()]).float()
        inv = sc.reciprocal()
        amax = torch.zeros(3, device="cuda")
        qw, qwt = SF.fp8_quantize(w, sc[1:2], amax[1:2], "e4m3", transpose=True)
        mw, msw, mwt, mswt = SF.mx_quantize_weight(w)

        def bf16():
            tp.linear_rows(x, w)
            tp.dgrad(dy, w, wt)

        def delayed():
            qx = SF.fp8_quantize(x, sc[0:1], amax[0:1], "e4m3")
            SF.fp8_gemm(qx, qw, inv[0:1], inv[1:2], None, dt)
            qg = SF.fp8_quantize(dy, sc[2:3], amax[2:3], gfmt)
            SF.fp8_gemm(qg, qwt, inv[2:3], inv[1:2], None, dt)

        def mxfp8():
            qx, sx = SF.mx_quantize(x, "e4m3")
            SF.gemm_mx(qx, sx, mw, msw, None, dt)
            qg, sg = SF.mx_quantize(dy, gfmt)
            SF.gemm_mx(qg, sg, mwt, mswt, None, dt)

        qx0 = SF.fp8_quantize(x, sc[0:1], amax[0:1], "e4m3")
        mx0, ms0 = SF.mx_quantize(x, "e4m3")
        y16 = tp.linear_rows(x, w).float()
        rel_mx = ((SF.gemm_mx(mx0, ms0, mw, msw, None, dt).float() - y16).norm() / y16.norm()).item()
        rel_pt = ((SF.fp8_gemm(qx0, qw, inv[0:1], inv[1:2], None, dt).float() - y16).norm() / y16.norm()).item()
        fns = {"bf16": bf16, "delayed": delayed, "mxfp8": mxfp8}
        rounds = {k: [] for k in sides}
        for _ in range(a.rounds):
            for k in sides:
                rounds[k].append(median_ms(fns[k], a.iters))
        med = {k: sorted(v)[len(v) // 2] for k, v in rounds.items()}
        for k in tot:
            tot[k] += med[k]
        # the forward GEMM alone, alternating as well
        gemms = {"gemm_mx": lambda: SF.gemm_mx(mx0, ms0, mw, msw, None, dt),
                 "blaslt_fp8": lambda: SF.fp8_gemm(qx0, qw, inv[0:1], inv[1:2], None, dt),
                 "gemm_tn": (lambda: C.gemm_tn(x, w)) if C.gemm_tn_shape_supported(M, O, I) else None}
        grounds = {k: [] for k, f in gemms.items() if f is not None}
        for _ in range(a.rounds):
            for k in grounds:
                grounds[k].append(median_ms(gemms[k], a.iters))
        gmed = {k: sorted(v)[len(v) // 2] for k, v in grounds.items()}
        t_qx = median_ms(lambda: SF.mx_quantize(x, "e4m3"), a.iters)
        t_qg = median_ms(lambda: SF.mx_quantize(dy, gfmt), a.iters)
        t_qw = median_ms(lambda: SF.mx_quantize_weight(w), a.iters)
        print(json.dumps({
            "linear": name, "M": M, "out": O, "in": I, "fp8": a.fp8,
            "fwd_dgrad_ms": {k: round(med[k], 4) for k in sides},
            "fwd_dgrad_rounds_ms": {k: [round(v, 4) for v in rounds[k]] for k in sides},
            "fwd_gemm_only_ms": {k: round(v, 4) for k, v in gmed.items()},
            "fwd_gemm_only_tflops": {k: round(2.0 * M * O * I / v / 1e9, 1) for k, v in gmed.items()},
            "fwd_gemm_only_rounds_ms": {k: [round(v, 4) for v in grounds[k]] for k in grounds},
            "mx_quant_x_ms": round(t_qx, 4), "mx_quant_dy_ms": round(t_qg, 4),
            "mx_quant_x_GBps": round(x.numel() * (3 + 1 / 32) / t_qx / 1e6, 1),
            "mx_weight_quant_per_step_ms": round(t_qw, 4),
            "output_rel_err_vs_bf16": {"mxfp8": round(rel_mx, 5), "delayed": round(rel_pt, 5)}}), flush=True)
        del x, dy, w, wt, qw, qwt, mw, mwt, qx0, mx0, y16
    print(json.dumps({"total_fwd_dgrad_ms": {k: round(v, 4) for k, v in tot.items()},
                      "mxfp8_vs_bf16": round(tot["bf16"] / tot["mxfp8"], 3),
                      "mxfp8_vs_delayed": round(tot["delayed"] / tot["mxfp8"], 3), "layers_per_step": 24}), flush=True)


if __name__ == "__main__":
    main()
