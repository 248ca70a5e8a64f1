"""--moe-grouped-gemm, CPU side: the torch twins of the device router, the grouped expert GEMM and
the ranged weight gradient (the padded layout and its tables against a brute-force construction),
the Switch layer with the flag against the per-expert loop in fp32, the flag's validation, and a
two-iteration pretrain_gpt.py run whose checkpoint reloads."""
import os
import subprocess
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["--num-layers", "2", "--hidden-size", "256", "--num-attention-heads", "4", "--seq-length", "32",
        "--max-position-embeddings", "32", "--micro-batch-size", "2"]
DEFAULTS = {"tokenizer_type": "GPT2BPETokenizer"}


def route_cases(T=512, E=4, seed=0):
    """name -> top-1 expert per token [T]: random; all to one expert; one expert with exactly 256
    tokens (no pad), with 257, with 1, with 0."""
    g = torch.Generator().manual_seed(seed)
    cases = {"random": torch.randint(0, E, (T,), generator=g), "all_to_one": torch.full((T,), 2)}
    for name, n in (("exactly_256", 256), ("one_with_257", 257), ("one_with_1", 1), ("one_with_0", 0)):
        e = torch.randint(1, E, (T,), generator=g)           # expert 0 gets exactly n tokens
        e[torch.randperm(T, generator=g)[:n]] = 0
        cases[name] = e
    return cases


def logits_for(experts, E=4, seed=1, dtype=torch.float32):
    """Logits whose arg-max is ``experts`` and whose top two differ by more than 1e-3 (here >= 1)."""
    g = torch.Generator().manual_seed(seed)
    lg = torch.rand(experts.numel(), E, generator=g)
    lg[torch.arange(experts.numel()), experts] += 2.0
    return lg.to(dtype)


def brute_force_tables(experts, E):
    """The layout from its definition, token by token."""
    T = experts.numel()
    R = (T // 256 + E) * 256
    counts = [int((experts == e).sum()) for e in range(E)]
    rows = [-(-c // 256) * 256 for c in counts]
    start = [sum(rows[:e]) for e in range(E)]
    row_of_token = [0] * T
    token_of_row = [-1] * R
    fill = list(start)
    for t in range(T):
        e = int(experts[t])
        row_of_token[t] = fill[e]
        token_of_row[fill[e]] = t
        fill[e] += 1
    tile_expert = [-1] * (R // 256)
    for e in range(E):
        for i in range(start[e] // 256, (start[e] + rows[e]) // 256):
            tile_expert[i] = e
    return dict(row_of_token=row_of_token, token_of_row=token_of_row, tile_expert=tile_expert,
                seg=[[start[e], rows[e]] for e in range(E)], counts=counts, R=R)


@pytest.mark.parametrize("case", ["random", "all_to_one", "exactly_256", "one_with_257", "one_with_1", "one_with_0"])
def test_routing_twin_matches_brute_force(case):
    from smdt_amd.ops import functional as SF
    E = 4
    experts = route_cases()[case]
    logits = logits_for(experts, E)
    top_p, top_e, row_of_token, token_of_row, tile_expert, seg, counts = SF.moe_route(logits)
    want = brute_force_tables(experts, E)
    assert SF.moe_rows(512, E) == want["R"] == 1536
    assert top_e.tolist() == experts.tolist()
    assert row_of_token.tolist() == want["row_of_token"]          # stable order inside a segment
    assert token_of_row.tolist() == want["token_of_row"]          # -1 on every pad row
    assert tile_expert.tolist() == want["tile_expert"]            # -1 on the unused tail tiles
    assert seg.tolist() == want["seg"] and counts.tolist() == want["counts"]
    assert int(seg[:, 1].sum()) <= want["R"] and all(r % 256 == 0 for r in seg[:, 1].tolist())
    assert token_of_row.dtype == torch.int64 and all(t.dtype == torch.int32 for t in (top_e, row_of_token, tile_expert,
                                                                                      seg, counts))
    torch.testing.assert_close(top_p, torch.softmax(logits, -1).max(-1).values, rtol=1e-6, atol=0)


def test_routing_twin_tie_goes_to_the_lowest_index():
    from smdt_amd.ops import functional as SF
    lg = torch.tensor([[0.5, 2.0, 2.0, 1.0], [3.0, 1.0, 3.0, 3.0]])
    assert SF.moe_route(lg)[1].tolist() == [1, 0]


def _switch_pair(seed=2, router_scale=50.0, h=32, f=64, E=4):
    from smdt_amd.models.transformer import SwitchMLP, TransformerConfig
    from smdt_amd.parallel import state as ps
    ps.destroy_model_parallel()
    base = dict(num_layers=2, hidden_size=h, ffn_hidden_size=f, num_attention_heads=2, max_position_embeddings=32,
                padded_vocab_size=64, params_dtype=torch.float32, hidden_dropout=0.0, attention_dropout=0.0,
                num_experts=E, seed=seed)
    ref = SwitchMLP(TransformerConfig(**base), 1)
    new = SwitchMLP(TransformerConfig(**base, moe_grouped_gemm=True), 1)
    with torch.no_grad():
        ref.router.mul_(router_scale)
    new.load_state_dict(ref.state_dict())
    return ref, new


@pytest.mark.parametrize("starve", [False, True])
def test_switch_layer_with_the_flag_equals_the_per_expert_loop_fp32(starve):
    """Output, input gradient, every expert's weight and bias gradient and the router gradient,
    both on the twins, at assert_close's fp32 defaults; an expert without tokens gets no gradient
    in both (``starve``: the router bias keeps every token away from expert 3)."""
    ref, new = _switch_pair()
    if starve:
        with torch.no_grad():
            for m in (ref, new):
                m.router_bias[3] = -1e4
    x = torch.randn(100, 3, 32, generator=torch.Generator().manual_seed(0))
    outs = []
    for m in (ref, new):
        xi = x.clone().requires_grad_(True)
        out, bias = m(xi)
        assert bias is None
        (out * torch.linspace(-1, 1, out.numel()).view_as(out)).sum().backward()
        outs.append((out.detach(), xi.grad))
    torch.testing.assert_close(outs[1][0], outs[0][0])
    torch.testing.assert_close(outs[1][1], outs[0][1])
    used = set(ref.route(x.reshape(-1, 32))[1].tolist())
    assert (3 not in used) if starve else (used == {0, 1, 2, 3})
    for (n, pr), pn in zip(ref.named_parameters(), new.parameters()):
        if pr.grad is None:
            assert pn.grad is None and "experts.3." in n, n
        else:
            torch.testing.assert_close(pn.grad, pr.grad, msg=lambda s, n=n: f"{n}: {s}")
    assert new.router.grad.abs().sum() > 0


def test_switch_layer_with_the_flag_accumulates_into_main_grad():
    """With fp32 main_grads the ranged twin accumulates there (and leaves an expert without tokens
    bit-unchanged) instead of handing gradients to autograd."""
    ref, new = _switch_pair()
    with torch.no_grad():
        for m in (ref, new):
            m.router_bias[3] = -1e4
    for p in new.parameters():
        p.main_grad = torch.full_like(p, 0.25)
    x = torch.randn(100, 3, 32, generator=torch.Generator().manual_seed(0))
    ref(x)[0].square().sum().backward()
    new(x)[0].square().sum().backward()
    from smdt_amd.parallel import tensor_parallel as tp
    tp.flush_deferred_wgrad()
    for (n, pr), pn in zip(ref.named_parameters(), new.parameters()):
        if "experts." not in n:
            continue
        assert pn.grad is None
        if "experts.3." in n:
            assert torch.equal(pn.main_grad, torch.full_like(pn, 0.25)), n
        else:
            torch.testing.assert_close(pn.main_grad - 0.25, pr.grad, rtol=1e-5, atol=1e-5, msg=lambda s, n=n: f"{n}: {s}")


def test_grouped_layer_raises_where_it_cannot_run():
    from smdt_amd.models.transformer import SwitchMLP, TransformerConfig
    from smdt_amd.parallel import state as ps
    ps.destroy_model_parallel()
    with pytest.raises(ValueError, match="num_experts"):
        TransformerConfig(moe_grouped_gemm=True)
    kw = dict(num_layers=1, hidden_size=32, num_attention_heads=2, max_position_embeddings=32, padded_vocab_size=64,
              params_dtype=torch.float32, num_experts=2, moe_grouped_gemm=True)
    x = torch.randn(4, 1, 32)
    with pytest.raises(RuntimeError, match="gelu"):
        SwitchMLP(TransformerConfig(**kw, activation="swiglu"), 1)(x)
    with pytest.raises(RuntimeError, match="biases"):
        SwitchMLP(TransformerConfig(**kw, add_bias_linear=False), 1)(x)


def _validate(extra, monkeypatch):
    from smdt_amd.train import arguments as A
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setenv("RANK", "0")
    return A.validate_args(A.parse_args(argv=BASE + extra), dict(DEFAULTS))


def test_validate_args_flag_and_rejections(monkeypatch):
    from smdt_amd.train import arguments as A
    from smdt_amd.train.checkpointing import CHECKPOINT_ARGS
    monkeypatch.delenv("SMDT_LAZY_GRAD_ZERO", raising=False)
    a = _validate(["--num-experts", "4", "--moe-grouped-gemm"], monkeypatch)
    a.padded_vocab_size = 64
    assert A.core_transformer_config_from_args(a).moe_grouped_gemm is True
    a = _validate(["--num-experts", "4"], monkeypatch)
    a.padded_vocab_size = 64
    assert A.core_transformer_config_from_args(a).moe_grouped_gemm is False     # opt-in
    assert "moe_grouped_gemm" in CHECKPOINT_ARGS
    ok = ["--num-experts", "4", "--moe-grouped-gemm"]
    with pytest.raises(ValueError, match="--num-experts"):
        _validate(["--moe-grouped-gemm"], monkeypatch)
    monkeypatch.setenv("WORLD_SIZE", "2")
    from smdt_amd.train import arguments as A2
    with pytest.raises(ValueError, match="tensor-model-parallel-size"):
        A2.validate_args(A2.parse_args(argv=BASE + ok + ["--tensor-model-parallel-size", "2"]), dict(DEFAULTS))
    for act in ("--swiglu", "--squared-relu", "--disable-bias-linear"):
        with pytest.raises(ValueError, match="GeLU"):
            _validate(ok + [act], monkeypatch)
    with pytest.raises(ValueError, match="multiples of 256"):
        _validate(ok + ["--hidden-size", "320"], monkeypatch)
    with pytest.raises(ValueError, match="multiples of 256"):
        _validate(ok + ["--ffn-hidden-size", "384"], monkeypatch)
    for fp8 in ("--fp8-hybrid", "--fp8-e4m3"):
        with pytest.raises(ValueError, match="fp8|num-experts"):
            _validate(ok + [fp8, "--bf16"], monkeypatch)
    monkeypatch.setenv("SMDT_LAZY_GRAD_ZERO", "1")
    with pytest.raises(ValueError, match="SMDT_LAZY_GRAD_ZERO"):
        _validate(ok, monkeypatch)


def test_deferred_queue_takes_ranged_items_and_fillers_pass_over_them():
    from smdt_amd.ops import functional as SF
    from smdt_amd.parallel.tensor_parallel import DeferredWgrad
    q = DeferredWgrad()
    q.allow_cpu = True
    experts = route_cases()["one_with_0"]
    route = SF.moe_route(logits_for(experts))
    seg, R = route[5], 1536
    g = torch.Generator().manual_seed(3)
    dy, x = torch.randn(R, 16, generator=g), torch.randn(R, 8, generator=g)
    mgs = [torch.full((16, 8), 0.5) for _ in range(4)]
    for e in range(4):
        q.push(None, mgs[e], dy, x, mrange=(seg, e))
    assert not q.fill_one() and q.fill_many(1e9) == 0 and len(q.items) == 4
    q.flush()
    for e, (s, r) in enumerate(seg.tolist()):
        want = 0.5 + (dy[s:s + r].t() @ x[s:s + r] if r else 0)
        torch.testing.assert_close(mgs[e], want * torch.ones(16, 8))
    assert torch.equal(mgs[0], torch.full((16, 8), 0.5))
    with pytest.raises(ValueError, match="ranged"):
        q.push(None, mgs[0], dy, x, mrange=(seg, 0), fresh=True)


@pytest.mark.slow
def test_pretrain_gpt_moe_grouped_gemm_trains_and_reloads(tmp_path):
    import re
    script = os.path.join(REPO, "recipes", "3_training_megatron-lm", "pretrain_gpt.py")
    ck = str(tmp_path / "ck")
    args = ["--num-layers", "2", "--hidden-size", "256", "--ffn-hidden-size", "256", "--num-attention-heads", "4",
            "--seq-length", "32", "--max-position-embeddings", "32", "--micro-batch-size", "2", "--global-batch-size",
            "2", "--lr", "0.001", "--lr-warmup-iters", "1", "--mock-data", "--log-interval", "1", "--eval-interval",
            "100", "--eval-iters", "1", "--vocab-size", "256", "--tokenizer-type", "NullTokenizer",
            "--num-experts", "4"]
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29547",
               CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    env.pop("SMDT_LAZY_GRAD_ZERO", None)
    r = subprocess.run([sys.executable, script] + args + ["--moe-grouped-gemm", "--train-iters", "2", "--save", ck,
                                                          "--save-interval", "2"],
                       env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    losses = [float(re.search(r"lm loss: (\S+)", ln).group(1)) for ln in r.stdout.splitlines()
              if "lm loss:" in ln and "iteration" in ln]
    assert len(losses) == 2 and all(torch.isfinite(torch.tensor(losses))), r.stdout[-2000:]
    saved = torch.load(os.path.join(ck, "iter_0000002", "mp_rank_00", "model_optim_rng.pt"), map_location="cpu",
                       weights_only=True)
    assert saved["args"]["moe_grouped_gemm"] is True
    # the flag comes back from the checkpoint with --use-checkpoint-args (it is not on this command line)
    r = subprocess.run([sys.executable, script] + args + ["--train-iters", "3", "--load", ck, "--use-checkpoint-args"],
                       env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "iteration        3/" in r.stdout or re.search(r"iteration\s+3/\s*3", r.stdout), r.stdout[-2000:]
