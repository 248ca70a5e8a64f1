"""One Switch MLP layer forward + backward with and without --moe-grouped-gemm.

h 1024, f 4096, T = 64 x 1024 tokens, E = 8, bf16. Both arms run in one process, alternating
(A B A B ...), each timed with device events over ``--iters`` calls after warm-up; one JSON line
per round and arm, and a summary line with the medians.

    python benchmarks/bench_moe.py [--rounds 5] [--iters 10] [--out bench_out/moe.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, default=1024)
    ap.add_argument("--ffn", type=int, default=4096)
    ap.add_argument("--seq", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--experts", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from smdt_amd.models.transformer import SwitchMLP, TransformerConfig
    from smdt_amd.parallel import state as ps
    from smdt_amd.parallel import tensor_parallel as tp
    ps.destroy_model_parallel()
    dev = "cuda"
    kw = dict(num_layers=2, hidden_size=a.hidden, ffn_hidden_size=a.ffn, num_attention_heads=a.hidden // 64,
              max_position_embeddings=a.seq, padded_vocab_size=1024, hidden_dropout=0.0, attention_dropout=0.0,
              seed=3, num_experts=a.experts, params_dtype=torch.bfloat16)
    arms = {"per_expert_loop": SwitchMLP(TransformerConfig(**kw), 1, device=dev)}
    arms["moe_grouped_gemm"] = SwitchMLP(TransformerConfig(**kw, moe_grouped_gemm=True), 1, device=dev)
    with torch.no_grad():
        arms["per_expert_loop"].router.mul_(20)
    arms["moe_grouped_gemm"].load_state_dict(arms["per_expert_loop"].state_dict())
    for m in arms.values():
        for p in m.parameters():
            p.main_grad = torch.zeros_like(p, dtype=torch.float32)
    x = torch.randn(a.seq, a.batch, a.hidden, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    x = x.to(torch.bfloat16).requires_grad_(True)
    dout = torch.randn_like(x)

    def call(m):
        x.grad = None
        m(x)[0].backward(dout)
        tp.flush_deferred_wgrad()

    def timed(m):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.iters):
            call(m)
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / a.iters

    for m in arms.values():
        for _ in range(3):
            call(m)
    torch.cuda.synchronize()
    out = open(a.out, "w") if a.out else None
    ms = {k: [] for k in arms}
    for r in range(a.rounds):
        for k, m in arms.items():
            t = timed(m)
            ms[k].append(t)
            line = json.dumps({"round": r, "arm": k, "ms_fwd_bwd": round(t, 4)})
            print(line, flush=True)
            if out:
                out.write(line + "\n")
    counts = arms["moe_grouped_gemm"].last_counts.tolist()
    line = json.dumps({"summary": {k: round(statistics.median(v), 4) for k, v in ms.items()},
                       "spread": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
                       "tokens_per_expert": counts, "hidden": a.hidden, "ffn": a.ffn,
                       "tokens": a.seq * a.batch, "experts": a.experts, "device": torch.cuda.get_device_name(0)})
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.close()


if __name__ == "__main__":
    main()
