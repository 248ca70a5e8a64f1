"""Fused BatchNorm + add + ReLU (csrc/kernels/batchnorm.hip) against the module chain
``nn.BatchNorm2d -> add -> relu`` at the ResNet-50 batch-64 / 224 px shapes: forward + backward,
bf16 channels_last, the two sides alternating round by round. Per shape: the plan, the median
microseconds of both sides, and the fused op's effective GB/s per pass (forward = statistics + apply
sweeps, backward = reduction + dx sweeps; bytes = what the sweeps read and write of activations).

    python benchmarks/bench_bn.py [--rounds 7] [--iters 20]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from smdt_amd.ops import functional as SF  # noqa: E402

# name, H = W, C, mode
SHAPES = [("stem.bn1", 112, 64, "relu"),
          ("layer1.bn1/2", 56, 64, "relu"), ("layer1.bn3", 56, 256, "residual_relu"), ("layer1.down", 56, 256, "plain"),
          ("layer2.bn1/2", 28, 128, "relu"), ("layer2.bn3", 28, 512, "residual_relu"), ("layer2.down", 28, 512, "plain"),
          ("layer3.bn1/2", 14, 256, "relu"), ("layer3.bn3", 14, 1024, "residual_relu"), ("layer3.down", 14, 1024, "plain"),
          ("layer4.bn1/2", 7, 512, "relu"), ("layer4.bn3", 7, 2048, "residual_relu"), ("layer4.down", 7, 2048, "plain")]


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--iters", type=int, default=20)
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    for name, hw, C, mode in SHAPES:
        has_res, relu = mode == "residual_relu", mode != "plain"
        mk = lambda: torch.randn(a.batch, hw, hw, C, device=dev).bfloat16().permute(0, 3, 1, 2)  # noqa: E731
        x, dy = mk().requires_grad_(), mk()
        res = mk().requires_grad_() if has_res else None
        bn = nn.BatchNorm2d(C).to(dev)
        leaves = [t for t in (x, res, bn.weight, bn.bias) if t is not None]

        def fused_fwd():
            return SF.batch_norm_act(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, True, 0.1, 1e-5,
                                     residual=res, relu=relu)

        def chain_fwd():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                y = bn(x)
                y = y + res if has_res else y
                return torch.relu(y) if relu else y

        def both(fwd):
            return lambda: torch.autograd.grad(fwd(), leaves, dy)

        sides = {"fused_fwd": fused_fwd, "fused": both(fused_fwd), "chain": both(chain_fwd)}
        for fn in sides.values():
            timed(fn, 5)
        t = {k: [] for k in sides}
        for _ in range(a.rounds):
            for k, fn in sides.items():
                t[k].append(timed(fn, a.iters))
        us = {k: statistics.median(v) for k, v in t.items()}
        M = a.batch * hw * hw
        act = 2 * M * C     # bytes of one activation
        fwd_bytes = act * (3 + has_res)                     # x twice, y, residual
        bwd_bytes = act * (2 * (2 + relu) + 1 + has_res)    # dy, x (, y) twice, dx, dres
        bwd_us = us["fused"] - us["fused_fwd"]
        print(json.dumps({"shape": name, "M": M, "C": C, "mode": mode, "plan": SF.bn_act_plan(M, C),
                          "fused_us": round(us["fused"], 1), "chain_us": round(us["chain"], 1),
                          "speedup": round(us["chain"] / us["fused"], 2),
                          "fused_fwd_us": round(us["fused_fwd"], 1), "fwd_GBps": round(fwd_bytes / us["fused_fwd"] / 1e3, 0),
                          "fused_bwd_us": round(bwd_us, 1), "bwd_GBps": round(bwd_bytes / bwd_us / 1e3, 0),
                          "spread_us": {k: [round(min(v), 1), round(max(v), 1)] for k, v in t.items()}}), flush=True)


if __name__ == "__main__":
    main()
