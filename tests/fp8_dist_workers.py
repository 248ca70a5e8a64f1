"""Worker bodies for the multi-process (gloo, CPU) FP8 tests. Importable by spawned children."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def fp8_dp_worker(rank, world):
    """DP = world replicas of a tiny FP8 GPT, each on its own tokens, two optimizer steps.
    Returns the scale / history tables and the rank's own amax as it stood before each update."""
    from smdt_amd.comm import init_distributed
    from smdt_amd.models.gpt import GPTModel
    from smdt_amd.models.transformer import TransformerConfig
    from smdt_amd.optim.optimizer import MixedPrecisionAdam
    from smdt_amd.parallel import state as ps
    from smdt_amd.parallel.distributed import DistributedDataParallel
    init_distributed("gloo")
    ps.initialize_model_parallel(1, 1)
    cfg = TransformerConfig(num_layers=1, hidden_size=64, num_attention_heads=2, max_position_embeddings=32,
                            padded_vocab_size=128, hidden_dropout=0.0, attention_dropout=0.0, seed=7,
                            params_dtype=torch.bfloat16, fp8="hybrid", fp8_amax_history_len=2)
    m = GPTModel(cfg)
    ddp = DistributedDataParallel(m, grad_dtype=torch.float32)
    opt = MixedPrecisionAdam(ddp, lr=1e-3, weight_decay=0.0, clip_grad=1.0)
    st = m.decoder.fp8_state
    g = torch.Generator().manual_seed(100 + rank)              # different data on every rank
    own = []
    for _ in range(2):
        t = torch.randint(0, 120, (2, 33), generator=g)
        ddp.zero_grad_buffer()
        m(t[:, :-1], labels=t[:, 1:]).float().mean().backward()
        ddp.finish_grad_sync()
        own.append(st.amax.clone())
        opt.step()
    return {"scale": st.scale.clone(), "hist": st.amax_history.clone(), "own": torch.stack(own)}
