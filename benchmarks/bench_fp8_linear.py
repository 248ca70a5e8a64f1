"""FP8 linear against the 16-bit linear at the GPT-2 345M step shapes (65,536 tokens): forward +
dgrad per linear, the FP8 side INCLUDING the activation and gradient quantise passes
(fp8_quant.hip). The weight quantise (q(W) and q(W)^T in one pass) is amortised over an optimizer
step and reported separately. bf16 goes through ``linear_rows`` / ``dgrad`` with the cached W^T,
as the training step does, with the TunableOp table loaded as in bench.py.

The two sides alternate (bf16, fp8, bf16, fp8, ...) so clock and temperature drift hit both;
each round is the median of ``--iters`` timed calls and the JSON line per shape carries every
round, so the repeat spread is visible.

``--fused-quantize``: the same forward + dgrad of the four linears INCLUDING the kernel that produces
each input (LayerNorm -> QKV, bias-dropout-residual-LayerNorm -> fc1, bias-GeLU -> fc2; the
projection's input comes from attention and is quantised by the linear either way), with the
producer writing the E4M3 operand (--fp8-fused-quantize) against the producer followed by the
stand-alone quantise pass, in alternating rounds, with the 16-bit copy kept (16-bit wgrad) and
dropped (--fp8-wgrad). The producer kernels alone are timed as well."""
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


def fused_quantize_mode(a):
    from smdt_amd.ops import functional as SF
    M, dt, h = a.m, torch.bfloat16, 1024
    gfmt = "e5m2" if a.fp8 == "hybrid" else "e4m3"
    rnd = lambda *s, k=1.0: torch.randn(*s, device="cuda", dtype=dt) * k
    gamma, beta, hb, res = 1 + rnd(h, k=0.1), rnd(h, k=0.1), rnd(h, k=0.1), rnd(M, h)
    producers = {      # input width of the producer, fn(x, **fp8 keywords) -> y or (y, q)
        "qkv": (h, lambda x, **k: SF.layer_norm(x, gamma, beta, **k)),
        "proj": (h, None),
        "fc1": (h, lambda x, **k: SF.bias_dropout_add_norm(x, hb, res, gamma, beta, 0.1, True, **k)[0]),
        "fc2": (4 * h, lambda x, **k: SF.bias_gelu(x, b4, "tanh", **k)),
    }
    b4 = rnd(4 * h, k=0.1)
    tot = {}
    for name, O, I in (("qkv", 3072, 1024), ("proj", 1024, 1024), ("fc1", 4096, 1024), ("fc2", 1024, 4096)):
        width, prod = producers[name]
        xin, dy, w = rnd(M, width), rnd(M, O, k=1e-3), rnd(O, I, k=0.02)
        x0 = xin if prod is None else prod(xin)
        sc = torch.stack([448.0 / x0.float().abs().max(), 448.0 / w.float().abs().max(),
                          SF.FP8_MAX[gfmt] / dy.float().abs().max()]).float()
        inv, amax = sc.reciprocal(), torch.zeros(3, device="cuda")
        qw, qwt = SF.fp8_quantize(w, sc[1:2], amax[1:2], "e4m3", transpose=True)
        slot = (sc[0:1], amax[0:1])

        def gemms(qx):
            SF.fp8_gemm(qx, qw, inv[0:1], inv[1:2], None, dt)
            qg = SF.fp8_quantize(dy, sc[2:3], amax[2:3], gfmt)
            SF.fp8_gemm(qg, qwt, inv[2:3], inv[1:2], None, dt)

        def unfused():
            gemms(SF.fp8_quantize(xin if prod is None else prod(xin), sc[0:1], amax[0:1], "e4m3"))

        def fused(keep16):
            if prod is None:
                return unfused()
            gemms(prod(xin, fp8_out=slot, keep16=keep16)[1])

        forms = {"unfused": unfused, "fused_keep16": lambda: fused(True), "fused_q_only": lambda: fused(False)}
        rounds = {k: [] for k in forms}
        with torch.no_grad():
            for _ in range(a.rounds):
                for k, fn in forms.items():
                    rounds[k].append(median_ms(fn, a.iters))
            alone = {} if prod is None else {
                "producer_16bit_ms": median_ms(lambda: prod(xin), a.iters),
                "quant_x_ms": median_ms(lambda: SF.fp8_quantize(x0, sc[0:1], amax[0:1], "e4m3"), a.iters),
                "producer_keep16_ms": median_ms(lambda: prod(xin, fp8_out=slot, keep16=True), a.iters),
                "producer_q_only_ms": median_ms(lambda: prod(xin, fp8_out=slot, keep16=False), a.iters)}
        med = {k: sorted(v)[len(v) // 2] for k, v in rounds.items()}
        for k, v in med.items():
            tot[k] = tot.get(k, 0.0) + v
        print(json.dumps({"linear": name, "M": M, "out": O, "in": I, "fp8": a.fp8,
                          **{k + "_ms": round(v, 4) for k, v in med.items()},
                          **{k + "_rounds_ms": [round(t, 4) for t in v] for k, v in rounds.items()},
                          **{k: round(v, 4) for k, v in alone.items()}}), flush=True)
    print(json.dumps({"total_" + k + "_ms": round(v, 4) for k, v in tot.items()} | {"layers_per_step": 24}), flush=True)


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--fp8", choices=["hybrid", "e4m3"], default="hybrid")
    ap.add_argument("--no-tunable", action="store_true")
    ap.add_argument("--fused-quantize", action="store_true",
                    help="producers writing the E4M3 operand against producer + quantise pass")
    a = ap.parse_args()
    table = os.path.join(ROOT, "profiles", "tunableop", "gfx950_gpt345m_results.csv")
    if not a.no_tunable and os.path.exists(table):
        import torch.cuda.tunable as tun
        tun.enable(True)
        tun.tuning_enable(False)
        tun.read_file(table)
    if a.fused_quantize:
        return fused_quantize_mode(a)
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
