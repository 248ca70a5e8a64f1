"""FP8 linears with delayed scaling, CPU side: the flags and their validation, the scale-update
rule on hand-computed cases, a small GPT on the torch twins (recompute, micro-batches, a
hand-written quantise-dequantise composition) and the checkpoint round trip."""
import argparse
import warnings

import pytest
import torch

BASE = ["--num-layers", "2", "--hidden-size", "64", "--num-attention-heads", "4", "--seq-length", "32",
        "--max-position-embeddings", "32", "--micro-batch-size", "2"]
DEFAULTS = {"tokenizer_type": "GPT2BPETokenizer"}


def _validate(extra, monkeypatch, world=1):
    from smdt_amd.train import arguments as A
    monkeypatch.setenv("WORLD_SIZE", str(world))
    monkeypatch.setenv("RANK", "0")
    return A.validate_args(A.parse_args(argv=BASE + extra), dict(DEFAULTS))


def test_fp8_flags_take_effect(monkeypatch, capsys):
    from smdt_amd.train import arguments as A
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        a = _validate(["--fp8-hybrid", "--bf16", "--fp8-margin", "2", "--fp8-interval", "3",
                       "--fp8-amax-history-len", "4", "--fp8-amax-compute-algo", "max"], monkeypatch)
    assert not any("without effect" in str(x.message) for x in w)
    assert "weight gradients stay in bf16" in capsys.readouterr().out      # the one notice without --no-fp8-wgrad
    a.padded_vocab_size = 64
    cfg = A.core_transformer_config_from_args(a)
    assert cfg.fp8 == "hybrid" and cfg.fp8_margin == 2 and cfg.fp8_interval == 3
    assert cfg.fp8_amax_history_len == 4 and cfg.fp8_amax_compute_algo == "max"
    a = _validate(["--fp8-e4m3", "--fp16", "true", "--no-fp8-wgrad"], monkeypatch)
    assert "weight gradients" not in capsys.readouterr().out
    a.padded_vocab_size = 64
    assert A.core_transformer_config_from_args(a).fp8 == "e4m3"
    a = _validate(["--bf16"], monkeypatch)
    a.padded_vocab_size = 64
    assert A.core_transformer_config_from_args(a).fp8 is None
    # --transformer-impl still only warns
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        _validate(["--transformer-impl", "transformer_engine"], monkeypatch)
    assert any("--transformer-impl" in str(x.message) for x in w)


@pytest.mark.parametrize("extra,world,needle", [
    (["--fp8-hybrid"], 1, "--bf16 or --fp16"),
    (["--fp8-e4m3"], 1, "--bf16 or --fp16"),
    (["--fp8-hybrid", "--fp8-e4m3", "--bf16"], 1, "--fp8-e4m3 and --fp8-hybrid"),
    (["--fp8-hybrid", "--bf16", "--tensor-model-parallel-size", "2"], 2, "--tensor-model-parallel-size"),
    (["--fp8-e4m3", "--bf16", "--num-experts", "4"], 1, "--num-experts"),
    (["--fp8-hybrid", "--bf16", "--seq-length", "20"], 1, "--seq-length"),
    (["--fp8-e4m3", "--bf16", "--hidden-size", "72"], 1, "--hidden-size"),
])
def test_fp8_rejected_combinations(extra, world, needle, monkeypatch):
    with pytest.raises(ValueError) as e:
        _validate(extra, monkeypatch, world)
    assert needle in str(e.value) and "--fp8-" in str(e.value)


def test_fp8_config_rejects_tp_and_fp32():
    from smdt_amd.models.transformer import TransformerConfig
    with pytest.raises(ValueError):
        TransformerConfig(fp8="hybrid", params_dtype=torch.float32)
    with pytest.raises(ValueError):
        TransformerConfig(fp8="e5m2")
    with pytest.raises(ValueError):
        TransformerConfig(fp8="e4m3", num_experts=4)


def test_fp8_update_scales_hand_computed():
    from smdt_amd.ops import functional as SF
    fm = torch.tensor([448.0, 448.0, 57344.0])
    # history length 1, most_recent, margin 0: scale = fmt_max / amax
    s, h, a = torch.ones(3), torch.zeros(3, 1), torch.tensor([2.0, 7.0, 4.0])
    SF.fp8_update_scales(s, h, a, fm, 0, "most_recent")
    assert s.tolist() == [224.0, 64.0, 14336.0] and h[:, 0].tolist() == [2.0, 7.0, 4.0] and a.tolist() == [0, 0, 0]
    # amax 0 and inf (and NaN) keep the old scale
    a.copy_(torch.tensor([0.0, float("inf"), float("nan")]))
    SF.fp8_update_scales(s, h, a, fm, 0, "most_recent")
    assert s.tolist() == [224.0, 64.0, 14336.0]
    # history length 4, margin 2: most_recent follows the newest, max remembers the largest
    for algo, want in (("most_recent", [448 / 1 / 4, 448 / 8 / 4, 57344 / 2 / 4]),
                       ("max", [448 / 4 / 4, 448 / 8 / 4, 57344 / 16 / 4])):
        s, h, a = torch.ones(3), torch.zeros(3, 4), torch.zeros(3)
        for am in ([4.0, 1.0, 16.0], [2.0, 2.0, 4.0], [1.0, 8.0, 2.0]):
            a.copy_(torch.tensor(am))
            SF.fp8_update_scales(s, h, a, fm, 2, algo)
        assert s.tolist() == want, algo
        assert h.tolist() == [[1.0, 2.0, 4.0, 0.0], [8.0, 2.0, 1.0, 0.0], [2.0, 4.0, 16.0, 0.0]]
    # the max forgets a value once it rolls out of the history
    s, h, a = torch.ones(1), torch.zeros(1, 2), torch.zeros(1)
    for am, want in ((8.0, 56.0), (1.0, 56.0), (2.0, 224.0)):
        a.fill_(am)
        SF.fp8_update_scales(s, h, a, fm[:1], 0, "max")
        assert s.item() == want
    with pytest.raises(ValueError):
        SF.fp8_update_scales(s, h, a, fm[:1], 0, "mean")


def test_fp8_interval_updates_every_second_step():
    from smdt_amd.parallel import state as ps
    from smdt_amd.parallel import tensor_parallel as tp
    ps.destroy_model_parallel()
    st = tp.FP8State(1, "hybrid", interval=2)
    assert st.fmt_max.tolist() == [448.0, 448.0, 57344.0]
    st.amax.copy_(torch.tensor([2.0, 4.0, 8.0]))
    st.after_optimizer_step()
    assert st.scale.tolist() == [1.0, 1.0, 1.0] and st.amax.tolist() == [2.0, 4.0, 8.0]
    st.amax.copy_(torch.maximum(st.amax, torch.tensor([1.0, 8.0, 1.0])))      # the slot keeps merging
    st.after_optimizer_step()
    assert st.scale.tolist() == [224.0, 56.0, 7168.0] and st.amax.tolist() == [0.0, 0.0, 0.0]
    assert torch.equal(st.scale_inv, torch.tensor([224.0, 56.0, 7168.0]).reciprocal())


def test_fp8_tables_stay_fp32_when_the_model_is_cast():
    """training.py casts the built model with ``model.to(device, dtype=params_dtype)``: the scale /
    amax tables must stay fp32 with their exact values (the quantise kernel takes fp32 slots)."""
    from smdt_amd.parallel import state as ps
    from smdt_amd.parallel import tensor_parallel as tp
    ps.destroy_model_parallel()
    holder = torch.nn.Sequential(torch.nn.Linear(4, 4), tp.FP8State(2, "hybrid", history_len=2))
    st = holder[1]
    st.scale.fill_(37.123)                       # not a bf16 value
    want = st.scale.clone()
    for cast in (lambda m: m.to(dtype=torch.bfloat16), lambda m: m.half(), lambda m: m.to("cpu", torch.bfloat16)):
        holder = cast(holder)
        assert holder[0].weight.dtype in (torch.bfloat16, torch.float16)
        for n in ("scale", "amax_history", "amax", "fmt_max", "scale_inv"):
            assert getattr(st, n).dtype == torch.float32, n
        assert st.step_count.dtype == torch.int64 and torch.equal(st.scale, want)


def test_fp8_quantize_twin_semantics():
    from smdt_amd.ops import functional as SF
    x = torch.tensor([[0.0, 1.0625, 1.1875, 500.0, -500.0, 2.0 ** -10, float("inf"), 3.0] + [0.0] * 8]).bfloat16()
    amax = torch.zeros(1)
    q, qt = SF.fp8_quantize(x, torch.ones(1), amax, "e4m3", transpose=True)
    assert q.dtype == torch.float8_e4m3fn and qt.shape == (16, 1)
    assert q.float()[0, :8].tolist() == [0.0, 1.0, 1.25, 448.0, -448.0, 0.0, 448.0, 3.0]   # ties to even, saturation
    assert torch.isinf(amax).item()
    x[0, 6] = float("nan")
    amax.zero_()
    q = SF.fp8_quantize(x, torch.ones(1), amax, "e5m2")
    assert torch.isnan(q.float()[0, 6]) and torch.isnan(amax).item() and q.float()[0, 3].item() == 500.0 - 500.0 + 512.0
    with pytest.raises(ValueError):
        SF.fp8_quantize(torch.zeros(4, 24).bfloat16(), torch.ones(1), amax, "e4m3")
    with pytest.raises(ValueError):
        SF.fp8_quantize(torch.zeros(4, 32), torch.ones(1), amax, "e4m3")


def test_fp8_linear_gradients_against_independent_reference():
    """One FP8 linear on the twins, scales away from 1: y and dX equal a hand-written fp32 matmul
    of the dequantised operands up to the output rounding, and the weight gradient is the 16-bit
    one (dY^T x of the unquantised operands), not a product of FP8 values."""
    from smdt_amd.parallel import state as ps
    from smdt_amd.parallel import tensor_parallel as tp
    ps.destroy_model_parallel()
    g = torch.Generator().manual_seed(2)
    st = tp.FP8State(1, "hybrid")
    st.scale.copy_(torch.tensor([37.0, 1900.0, 410.0]))
    torch.reciprocal(st.scale, out=st.scale_inv)
    w = torch.nn.Parameter((0.05 * torch.randn(192, 64, generator=g)).bfloat16())
    w.main_grad = torch.zeros(192, 64)
    b = torch.nn.Parameter((0.1 * torch.randn(192, generator=g)).bfloat16())
    x = torch.randn(4, 16, 64, generator=g).bfloat16().requires_grad_()
    dy = (3 * torch.randn(4, 16, 192, generator=g)).bfloat16()
    y = tp.FP8Linear.apply(x, w, b, True, st, 0)
    y.backward(dy)
    tp.flush_deferred_wgrad()

    def dq(t, s, dt, mx):
        return (t.detach().float() * s).clamp(-mx, mx).to(dt).float() / s
    x2, dy2 = x.reshape(-1, 64), dy.reshape(-1, 192)
    wq = dq(w, 1900.0, torch.float8_e4m3fn, 448.0)
    y_ref = dq(x2, 37.0, torch.float8_e4m3fn, 448.0) @ wq.t() + b.detach().float()
    dx_ref = dq(dy2, 410.0, torch.float8_e5m2, 57344.0) @ wq
    for got, ref in ((y.detach().reshape(-1, 192), y_ref), (x.grad.reshape(-1, 64), dx_ref)):
        err = ((got.float() - ref).abs().amax(-1) / ref.abs().amax(-1)).max().item()
        assert err <= 2.0 ** -8, err                       # half a bf16 ulp of the row maximum
    # dX through q(W) instead of q(W)^T, or with the E4M3 gradient format, is far outside that
    assert (x.grad.float().reshape(-1, 64) - dx_ref).abs().max() < 0.05 * dx_ref.abs().max()
    dw_ref = dy2.float().t() @ x2.detach().float()
    # the CPU wgrad is a bf16 matmul added into fp32: one bf16 rounding (2^-8) of each entry
    torch.testing.assert_close(w.main_grad, dw_ref, atol=1e-2, rtol=2.0 ** -7)
    dw_fp8 = dq(dy2, 410.0, torch.float8_e5m2, 57344.0).t() @ dq(x2, 37.0, torch.float8_e4m3fn, 448.0)
    assert (dw_fp8 - dw_ref).abs().max() > 3 * (w.main_grad - dw_ref).abs().max()
    torch.testing.assert_close(b.grad.float(), dy2.float().sum(0), atol=1e-2, rtol=2.0 ** -7)
    assert torch.equal(st.amax, torch.stack([x2.detach().float().abs().max(), w.detach().float().abs().max(),
                                             dy2.float().abs().max()]))


# ---------------------------------------------------------------------------------- small GPT

KW = dict(num_layers=2, hidden_size=128, num_attention_heads=2, max_position_embeddings=32, padded_vocab_size=256,
          hidden_dropout=0.0, attention_dropout=0.0, seed=3, params_dtype=torch.bfloat16)


def _build(lr=1e-3, **kw):
    from smdt_amd.models.gpt import GPTModel
    from smdt_amd.models.transformer import TransformerConfig
    from smdt_amd.optim.optimizer import MixedPrecisionAdam
    from smdt_amd.parallel import state as ps
    from smdt_amd.parallel.distributed import DistributedDataParallel
    ps.destroy_model_parallel()
    model = GPTModel(TransformerConfig(**KW, **kw))
    ddp = DistributedDataParallel(model, grad_dtype=torch.float32)
    return model, ddp, MixedPrecisionAdam(ddp, lr=lr, weight_decay=0.0, clip_grad=1.0)


def _tokens(n=1, seed=4):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 250, (2, 33), generator=g) for _ in range(n)]


def _step(model, ddp, opt, batches):
    ddp.zero_grad_buffer()
    losses = []
    for t in batches:
        loss = model(t[:, :-1], labels=t[:, 1:]).float().mean()
        loss.backward()
        losses.append(loss.item())
    ddp.finish_grad_sync()
    grads = ddp.grad_data.clone()
    opt.step()
    return losses, grads


def test_fp8_gpt_loss_differs_and_recompute_is_bit_identical():
    toks = _tokens(3)
    plain = _build()
    fp8 = _build(fp8="hybrid")
    rec = _build(fp8="hybrid", recompute_granularity="full")
    assert [k for k in fp8[0].state_dict() if k not in plain[0].state_dict()] == [
        "decoder.fp8_state." + n for n in ("scale", "amax_history", "amax", "step_count")]
    for i, t in enumerate(toks):
        lp, _ = _step(*plain, [t])
        lf, gf = _step(*fp8, [t])
        lr_, gr = _step(*rec, [t])
        assert lf != lp, i                               # FP8 is really in the path
        assert abs(lf[0] - lp[0]) < 0.05 * abs(lp[0])    # and still the same model
        assert lf == lr_ and torch.equal(gf, gr), i      # recompute: same scales, idempotent amax
    sf, sr = fp8[0].decoder.fp8_state, rec[0].decoder.fp8_state
    for n in ("scale", "amax_history", "amax"):
        assert torch.equal(getattr(sf, n), getattr(sr, n))
    assert (sf.scale != 1).all() and sf.scale.numel() == 2 * 4 * 3


def test_fp8_micro_batches_share_scales():
    model, ddp, opt = _build(fp8="hybrid")
    st = model.decoder.fp8_state
    _step(model, ddp, opt, _tokens(1))                   # scales leave 1
    seen = []
    orig = st.slot

    def slot(t):
        seen.append((t, st.scale[t].item(), st._epoch))
        return orig(t)
    st.slot = slot
    before = st.scale.clone()
    ddp.zero_grad_buffer()
    amax = []
    for t in _tokens(2, seed=9):
        model(t[:, :-1], labels=t[:, 1:]).float().mean().backward()
        amax.append(st.amax.clone())
    assert torch.equal(st.scale, before) and len({e for _, _, e in seen}) == 1
    for t, s, _ in seen:
        assert s == before[t].item()
    assert (amax[1] >= amax[0]).all() and (amax[1] > amax[0]).any()      # the slots merge by max
    # the weights were quantised once for both micro-batches and the backward
    assert len(st._wq) == 8
    ddp.finish_grad_sync()
    opt.step()
    assert not torch.equal(st.scale, before) and len(st._wq) == 0


def test_fp8_gpt_equals_hand_written_quantise_dequantise_composition(monkeypatch):
    """With lr = 0 the first step only moves the scales. The second forward must equal, bit for
    bit, the 16-bit model whose four linears per layer are replaced by a hand-written
    quantise -> fp32 matmul -> dequantise with those scales."""
    from smdt_amd.parallel import tensor_parallel as tp
    toks = _tokens(2)
    model, ddp, opt = _build(lr=0.0, fp8="hybrid")
    _step(model, ddp, opt, toks[:1])
    scale = model.decoder.fp8_state.scale.clone()
    assert (scale != 1).all()
    with torch.no_grad():
        want = model(toks[1][:, :-1], labels=toks[1][:, 1:]).float()

    plain, _, _ = _build(bias_gelu_fusion=True)
    calls = []

    def q(t, s):                                          # E4M3 quantise, hand-written
        return (t.float() * s).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float()

    orig = tp.linear_with_grad_accumulation_and_async_allreduce

    def hand_linear(x, weight, bias, sequence_parallel=False, async_grad_allreduce=False, add_bias=True, fp8=None):
        i = len(calls)
        if i == 8:                                        # the LM head stays 16-bit
            return orig(x, weight, bias, sequence_parallel, async_grad_allreduce, add_bias)
        calls.append(tuple(weight.shape))
        sx, sw = scale[3 * i], scale[3 * i + 1]
        acc = q(x.reshape(-1, x.shape[-1]), sx) @ q(weight, sw).t() * ((1 / sx) * (1 / sw))
        if bias is not None and add_bias:
            acc = acc + bias.float()
        return acc.to(weight.dtype).view(tuple(x.shape[:-1]) + (weight.shape[0],))
    monkeypatch.setattr(tp, "linear_with_grad_accumulation_and_async_allreduce", hand_linear)
    with torch.no_grad():
        got = plain(toks[1][:, :-1], labels=toks[1][:, 1:]).float()
    assert calls == [(384, 128), (128, 128), (512, 128), (128, 512)] * 2
    assert torch.equal(got, want)


def test_fp8_data_parallel_ranks_share_scales():
    """Two DP ranks (gloo) on different tokens: the amax slots are max-reduced over the group before
    every update, so both ranks hold the same history and scales, and the history is the
    element-wise max of the two ranks' own amax, not either rank's alone."""
    from _dist import run_workers
    import fp8_dist_workers as W
    a, b = run_workers(W.fp8_dp_worker, 2)
    assert torch.equal(a["scale"].view(torch.int32), b["scale"].view(torch.int32))
    assert torch.equal(a["hist"], b["hist"]) and (a["scale"] != 1).all()
    assert not torch.equal(a["own"], b["own"])                      # the ranks really saw different data
    both = torch.maximum(a["own"], b["own"])                        # [step, T]; history column 0 is the newest
    assert torch.equal(a["hist"][:, 0], both[1]) and torch.equal(a["hist"][:, 1], both[0])
    act = torch.arange(a["scale"].numel()) % 3 != 1                 # x and dY slots; weights are replicas
    assert (a["own"][1][act] != both[1][act]).any() and (b["own"][1][act] != both[1][act]).any()


def test_fp8_checkpoint_round_trip(tmp_path, capsys):
    from smdt_amd.train import checkpointing as ck
    toks = _tokens(4)
    kw = dict(fp8="hybrid", fp8_amax_history_len=4, fp8_amax_compute_algo="max", fp8_interval=2, fp8_margin=1)
    a = _build(**kw)
    for t in toks[:3]:
        _step(*a, [t])
    args = argparse.Namespace(save=str(tmp_path), load=str(tmp_path))
    ck.save_checkpoint(3, a[1], a[2], None, args)
    b = _build(**kw)
    assert ck.load_checkpoint(b[1], b[2], None, args) == 3
    sa, sb = a[0].decoder.fp8_state, b[0].decoder.fp8_state
    for n in ("scale", "amax_history", "amax", "scale_inv"):
        assert torch.equal(getattr(sa, n).view(torch.int32), getattr(sb, n).view(torch.int32)), n
    assert sb._step == 3 and (sb.scale != 1).all() and (sb.amax != 0).all()     # step 3 sits between two updates
    la, ga = _step(*a, [toks[3]])
    lb, gb = _step(*b, [toks[3]])
    assert la == lb and torch.equal(ga, gb)
    assert torch.equal(sa.scale, sb.scale) and torch.equal(sa.amax_history, sb.amax_history)

    # a checkpoint without FP8 state loads into an FP8 model with scales 1 and a notice
    plain = _build()
    plain_keys = list(plain[0].state_dict())
    assert not any("fp8" in k for k in plain_keys)
    d2 = tmp_path / "plain"
    args2 = argparse.Namespace(save=str(d2), load=str(d2), no_save_optim=True, no_load_optim=True)
    ck.save_checkpoint(1, plain[1], plain[2], None, args2)
    capsys.readouterr()
    assert ck.load_checkpoint(b[1], b[2], None, args2) == 1
    assert "no scaling state" in capsys.readouterr().out
    assert (sb.scale == 1).all() and (sb.amax_history == 0).all() and sb._step == 0
    _step(*b, [toks[0]])                                  # and trains on
