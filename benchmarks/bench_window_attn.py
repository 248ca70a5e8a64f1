"""Swin window-attention core, forward + backward: the fused kernels (csrc/kernels/window_attn.hip)
against the op chain of ``ShiftedWindowAttention.forward`` (roll, window partition, q scale, batched
QK^T, bias add, fp32 softmax, batched PV, reverse partition, roll back), both fed the qkv linear's
output on the padded grid. Shapes: swin_b's four stages at 128 x 128, 40 images per GPU (BASELINE
config 2): grids 35 / 21 / 14 / 7 after padding to the 7-token window, heads 4 / 8 / 16 / 32.

The sides alternate within a round; the figure is the median over the rounds of the mean time per
call. The chain here rolls and partitions 3 C channels where the module moves C before its qkv
linear, so its data movement is somewhat overstated; its GEMMs, bias add and softmax are the module's.

    python benchmarks/bench_window_attn.py [--rounds 5 --iters 20 --batch 40]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from smdt_amd.models.swin import ShiftedWindowAttention  # noqa: E402
from smdt_amd.ops import functional as SF  # noqa: E402

STAGES = [(35, 4), (21, 8), (14, 16), (7, 32)]   # (padded grid, heads)


def chain(qkv, bias, ws, shift, heads):
    B, ph, pw, C3 = qkv.shape
    C, N, nW = C3 // 3, ws * ws, (ph // ws) * (pw // ws)
    x = torch.roll(qkv, shifts=(-shift, -shift), dims=(1, 2)) if shift > 0 else qkv
    x = x.view(B, ph // ws, ws, pw // ws, ws, C3).permute(0, 1, 3, 2, 4, 5).reshape(B * nW, N, C3)
    q, k, v = x.view(B * nW, N, 3, heads, C // heads).permute(2, 0, 3, 1, 4).unbind(0)
    attn = (q * (C // heads) ** -0.5).matmul(k.transpose(-2, -1))
    attn = (attn.view(B, nW, heads, N, N) + bias.unsqueeze(0)).view_as(attn)
    attn = torch.softmax(attn.float(), dim=-1).to(q.dtype)
    x = attn.matmul(v).transpose(1, 2).reshape(B * nW, N, C)
    x = x.view(B, ph // ws, pw // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, ph, pw, C)
    return torch.roll(x, shifts=(shift, shift), dims=(1, 2)) if shift > 0 else x


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=40)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--iters", type=int, default=20)
    a = p.parse_args()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    ws = 7
    rows = []
    for grid, heads in STAGES:
        shift = 0 if grid <= ws else ws // 2
        C = 32 * heads
        mod = ShiftedWindowAttention(C, ws, shift, heads).to(dev)
        with torch.no_grad():
            mod.relative_position_bias_table.normal_(0, 0.5)
        table = mod.relative_position_bias_table
        qkv = torch.randn(a.batch, grid, grid, 3 * C, device=dev).bfloat16().requires_grad_()
        dout = torch.randn(a.batch, grid, grid, C, device=dev).bfloat16()

        def run_chain():
            bias = mod._bias(grid, grid, shift, dev, torch.bfloat16)
            chain(qkv, bias, ws, shift, heads).backward(dout)
            qkv.grad = table.grad = None

        def run_fused():
            SF.window_attention(qkv, table, ws, shift, heads).backward(dout)
            qkv.grad = table.grad = None

        for fn in (run_chain, run_fused):
            timed(fn, 3)
        t = {"chain": [], "fused": []}
        for _ in range(a.rounds):
            t["chain"].append(timed(run_chain, a.iters))
            t["fused"].append(timed(run_fused, a.iters))
        med = {k: statistics.median(v) for k, v in t.items()}
        rows.append({"grid": grid, "heads": heads, "shift": shift, "windows": a.batch * (grid // ws) ** 2,
                     "chain_ms": round(med["chain"], 4), "fused_ms": round(med["fused"], 4),
                     "chain_ms_min_max": [round(min(t["chain"]), 4), round(max(t["chain"]), 4)],
                     "fused_ms_min_max": [round(min(t["fused"]), 4), round(max(t["fused"]), 4)],
                     "speedup": round(med["chain"] / med["fused"], 2)})
        print(f"[bench_window_attn] grid {grid} heads {heads}: chain {med['chain']:.3f} ms, fused "
              f"{med['fused']:.3f} ms", file=sys.stderr, flush=True)
    print(json.dumps({"metric": "swin_b window attention core fwd+bwd, ms per call (eager launches)",
                      "batch": a.batch, "dtype": "bf16", "rounds": a.rounds, "iters": a.iters,
                      "device": torch.cuda.get_device_name(0), "stages": rows}), flush=True)


if __name__ == "__main__":
    main()
