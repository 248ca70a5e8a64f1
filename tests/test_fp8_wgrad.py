"""--fp8-wgrad, CPU side: the flag and its validation, the torch twin of the FP8 weight-gradient
GEMM against a hand-written float64 composition, one FP8 linear and a small GPT on the twins, and
FP8 items in the deferred wgrad queue."""
import math

import pytest
import torch

BASE = ["--num-layers", "2", "--hidden-size", "64", "--num-attention-heads", "4", "--seq-length", "32",
        "--max-position-embeddings", "32", "--micro-batch-size", "2"]
DEFAULTS = {"tokenizer_type": "GPT2BPETokenizer"}
FMT = {"e5m2": (torch.float8_e5m2, 57344.0), "e4m3": (torch.float8_e4m3fn, 448.0)}


def _validate(extra, monkeypatch):
    from smdt_amd.train import arguments as A
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setenv("RANK", "0")
    return A.validate_args(A.parse_args(argv=BASE + extra), dict(DEFAULTS))


def test_fp8_wgrad_flag(monkeypatch, capsys):
    from smdt_amd.models.transformer import TransformerConfig
    from smdt_amd.train import arguments as A
    a = _validate(["--fp8-hybrid", "--bf16", "--fp8-wgrad"], monkeypatch)
    assert "weight gradients stay" not in capsys.readouterr().out
    a.padded_vocab_size = 64
    cfg = A.core_transformer_config_from_args(a)
    assert cfg.fp8 == "hybrid" and cfg.fp8_wgrad is True
    a = _validate(["--fp8-hybrid", "--bf16"], monkeypatch)         # opt-in: off without the flag
    out = capsys.readouterr().out
    assert "weight gradients stay in bf16" in out and "--fp8-wgrad" in out
    a.padded_vocab_size = 64
    assert A.core_transformer_config_from_args(a).fp8_wgrad is False
    with pytest.raises(ValueError) as e:
        _validate(["--fp8-wgrad", "--bf16"], monkeypatch)
    assert "--fp8-hybrid" in str(e.value) and "--fp8-e4m3" in str(e.value)
    with pytest.raises(ValueError) as e:
        _validate(["--fp8-e4m3", "--bf16", "--fp8-wgrad", "--no-fp8-wgrad"], monkeypatch)
    assert "--fp8-wgrad" in str(e.value) and "--no-fp8-wgrad" in str(e.value)
    with pytest.raises(ValueError) as e:                           # 48 tokens: not the kernel's 64-row stage
        _validate(["--fp8-hybrid", "--bf16", "--fp8-wgrad", "--seq-length", "16", "--micro-batch-size", "3"],
                  monkeypatch)
    assert "multiple of 64" in str(e.value)
    with pytest.raises(ValueError):
        TransformerConfig(fp8_wgrad=True)


def _quant(t, scale, fmt):
    dt, mx = FMT[fmt]
    return (t.float() * scale).clamp(-mx, mx).to(dt)


@pytest.mark.parametrize("fmt", ["e5m2", "e4m3"])
@pytest.mark.parametrize("overwrite", [False, True])
def test_fp8_wgrad_twin_against_hand_written_composition(fmt, overwrite):
    from smdt_amd.ops import functional as SF
    g = torch.Generator().manual_seed(7)
    M, N, K = 96, 48, 80
    sdy, sx = 410.0, 37.0
    qdy = _quant(3 * torch.randn(M, N, generator=g), sdy, fmt)
    qx = _quant(torch.randn(M, K, generator=g), sx, "e4m3")
    inv_dy, inv_x = torch.tensor([1 / sdy]), torch.tensor([1 / sx])
    mg0 = torch.randn(N, K, generator=g)
    ref = (qdy.double() * inv_dy.double()).t() @ (qx.double() * inv_x.double())
    absref = (qdy.double().abs() * inv_dy.double()).t() @ (qx.double().abs() * inv_x.double())
    if not overwrite:
        ref = ref + mg0.double()
    mg = mg0.clone()
    out = SF.fp8_wgrad_ref(mg, qdy, qx, inv_dy, inv_x, overwrite)
    assert out is mg
    # fp32 operand rounding (2 x 2^-24) and an fp32 sum of M terms, on the sum of magnitudes
    bound = (M + 4) * 2.0 ** -24 * (absref + mg0.double().abs())
    assert ((mg.double() - ref).abs() <= bound).all()
    mg2 = mg0.clone()
    SF.fp8_wgrad(mg2, qdy, qx, inv_dy, inv_x, overwrite)           # CPU operands: the dispatcher runs the twin
    assert torch.equal(mg2, mg)


def test_fp8_linear_wgrad_is_the_product_of_the_quantised_operands():
    from smdt_amd.parallel import state as ps
    from smdt_amd.parallel import tensor_parallel as tp
    ps.destroy_model_parallel()
    g = torch.Generator().manual_seed(2)
    scales = [37.0, 1900.0, 410.0]

    def run(fp8_wgrad):
        st = tp.FP8State(1, "hybrid", fp8_wgrad=fp8_wgrad)
        st.scale.copy_(torch.tensor(scales))
        torch.reciprocal(st.scale, out=st.scale_inv)
        w = torch.nn.Parameter(w0.clone())
        w.main_grad = torch.zeros(192, 64)
        b = torch.nn.Parameter(b0.clone())
        x = x0.clone().requires_grad_()
        y = tp.FP8Linear.apply(x, w, b, True, st, 0)
        saved = y.grad_fn.saved_tensors[0]
        y.backward(dy)
        tp.flush_deferred_wgrad()
        return y.detach(), x.grad, w.main_grad, b.grad, saved, st

    w0 = (0.05 * torch.randn(192, 64, generator=g)).bfloat16()
    b0 = (0.1 * torch.randn(192, generator=g)).bfloat16()
    x0 = torch.randn(4, 16, 64, generator=g).bfloat16()
    dy = (3 * torch.randn(4, 16, 192, generator=g)).bfloat16()
    y1, dx1, dw1, db1, saved1, st1 = run(True)
    y0, dx0, dw0, db0, saved0, st0 = run(False)
    x2, dy2 = x0.reshape(-1, 64), dy.reshape(-1, 192)
    qx, qdy = _quant(x2, scales[0], "e4m3"), _quant(dy2, scales[2], "e5m2")
    # q(x) is what the forward keeps for the backward, not the 16-bit x
    assert saved1.dtype == torch.float8_e4m3fn and torch.equal(saved1.view(torch.uint8), qx.view(torch.uint8))
    assert saved0.dtype == torch.bfloat16
    dw_fp8 = (qdy.double() / scales[2]).t() @ (qx.double() / scales[0])
    dw_16 = dy2.double().t() @ x2.double()
    absprod = (qdy.double().abs() / scales[2]).t() @ (qx.double().abs() / scales[0])
    bound = (64 + 4) * 2.0 ** -24 * absprod
    assert ((dw1.double() - dw_fp8).abs() <= bound).all()
    # ... and the 16-bit product is far outside that tolerance for these inputs
    assert ((dw_16 - dw_fp8).abs() > 100 * bound).float().mean() > 0.9
    torch.testing.assert_close(db1.float(), dy2.float().sum(0), atol=1e-2, rtol=2.0 ** -7)
    assert torch.equal(db1, db0)                                   # the bias gradient: the 16-bit column sums
    assert torch.equal(y1, y0) and torch.equal(dx1, dx0)           # forward and dgrad are the same calls
    for n in ("amax", "scale"):
        assert torch.equal(getattr(st1, n), getattr(st0, n))


def test_fp8_linear_wgrad_without_main_grad_returns_the_product():
    from smdt_amd.parallel import state as ps
    from smdt_amd.parallel import tensor_parallel as tp
    ps.destroy_model_parallel()
    g = torch.Generator().manual_seed(3)
    st = tp.FP8State(1, "e4m3", fp8_wgrad=True)
    w = torch.nn.Parameter((0.05 * torch.randn(32, 16, generator=g)).bfloat16())
    x = torch.randn(16, 16, generator=g).bfloat16().requires_grad_()
    dy = torch.randn(16, 32, generator=g).bfloat16()
    tp.FP8Linear.apply(x, w, None, True, st, 0).backward(dy)
    ref = _quant(dy, 1.0, "e4m3").float().t() @ _quant(x.detach(), 1.0, "e4m3").float()
    assert w.grad.dtype == torch.bfloat16
    torch.testing.assert_close(w.grad.float(), ref, atol=0, rtol=2.0 ** -8)


@pytest.fixture
def queue():
    from smdt_amd.parallel import tensor_parallel as tp
    q = tp.DeferredWgrad()
    q.enabled, q.allow_cpu = True, True
    return q


def _fp8_item(g, M, N, K, fmt="e5m2"):
    qdy = _quant(torch.randn(M, N, generator=g), 8.0, fmt)
    qx = _quant(torch.randn(M, K, generator=g), 4.0, "e4m3")
    sc = (torch.tensor([1 / 8.0]), torch.tensor([1 / 4.0]))
    return qdy, qx, sc, (qdy.float() / 8.0).t() @ (qx.float() / 4.0)


def test_deferred_queue_mixes_16bit_and_fp8_items(queue):
    g = torch.Generator().manual_seed(5)
    ready = []
    w16, w8, w8b = (torch.nn.Parameter(torch.zeros(1)) for _ in range(3))
    for w in (w16, w8, w8b):
        w._smdt_grad_ready = ready.append
    mg16, mg8, mg8b = torch.ones(32, 48), torch.ones(32, 48), torch.full((16, 32), 2.0)
    dy16, x16 = torch.randn(64, 32, generator=g).bfloat16(), torch.randn(64, 48, generator=g).bfloat16()
    qdy, qx, sc, prod = _fp8_item(g, 64, 32, 48)
    qdy_b, qx_b, sc_b, prod_b = _fp8_item(g, 128, 16, 32, "e4m3")
    assert queue.eligible(mg8, qdy, qx) and queue.eligible(mg16, dy16, x16)
    assert not queue.eligible(mg8, qdy[:32], qx[:32])              # 32 rows: not the FP8 kernel's 64-row stage
    assert not queue.eligible(mg8, qdy, qx.view(torch.uint8).view(torch.float8_e5m2))   # x must be E4M3
    queue.push(w16, mg16, dy16, x16)
    queue.push(w8, mg8, qdy, qx, scales=sc)
    queue.push(w8b, mg8b, qdy_b, qx_b, scales=sc_b, fresh=True)    # an unwritten target: stored, not added
    assert not ready
    queue.flush()
    torch.testing.assert_close(mg16, 1 + (dy16.t() @ x16).float(), atol=1e-2, rtol=2.0 ** -7)
    torch.testing.assert_close(mg8, 1 + prod, atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(mg8b, prod_b, atol=1e-5, rtol=1e-5)
    assert ready == [w16, w8, w8b] and queue.stats["stores"] == 1 and not queue.items
    with pytest.raises(ValueError):
        queue.push(w8, mg8, qdy, qx)                               # FP8 bytes without their scales
    with pytest.raises(ValueError):
        queue.push(w16, mg16, dy16, x16, scales=sc)
    # the TP exchange fillers pass over FP8 items
    queue.push(w8, mg8, qdy, qx, scales=sc)
    assert queue.fill_one() is False and queue.fill_many(1e9) == 0 and len(queue.items) == 1
    queue.flush()


@pytest.mark.parametrize("concat", [True, False])
def test_deferred_queue_merges_fp8_segments(queue, concat):
    g = torch.Generator().manual_seed(6)
    w = torch.nn.Parameter(torch.zeros(1))
    mg = torch.zeros(32, 48)
    a = _fp8_item(g, 64, 32, 48)
    b = _fp8_item(g, 128, 32, 48)
    queue.concat_segments = concat
    queue.hold = True                       # an accumulation window: the second push merges
    queue.push(w, mg, a[0], a[1], scales=a[2])
    queue.hold = False
    queue.push(w, mg, b[0], b[1], scales=b[2])
    assert len(queue.items) == 1 and len(queue.items[0].segments) == 2
    queue.flush()
    assert queue.stats["max_segments"] == (1 if concat else 2)
    torch.testing.assert_close(mg, a[3] + b[3], atol=1e-5, rtol=1e-5)


def test_deferred_queue_refuses_a_modified_fp8_tensor(queue):
    g = torch.Generator().manual_seed(8)
    w = torch.nn.Parameter(torch.zeros(1))
    mg = torch.zeros(32, 48)
    qdy, qx, sc, _ = _fp8_item(g, 64, 32, 48)
    queue.push(w, mg, qdy, qx, scales=sc)
    qx.view(torch.uint8)[0, 0] = 1
    with pytest.raises(RuntimeError, match="modified in place"):
        queue.flush()


def test_small_gpt_trains_on_the_twins_with_fp8_wgrad():
    """Two optimizer steps of a 2-layer GPT (hidden 64) with fp8_wgrad on: finite losses, weight
    gradients that differ from the 16-bit-wgrad run, and after step 1 the same scale tables as that
    run (the forward, the dgrad and therefore every recorded amax are the same)."""
    from smdt_amd.models.gpt import GPTModel
    from smdt_amd.models.transformer import TransformerConfig
    from smdt_amd.optim.optimizer import MixedPrecisionAdam
    from smdt_amd.parallel import state as ps
    from smdt_amd.parallel.distributed import DistributedDataParallel
    kw = dict(num_layers=2, hidden_size=64, num_attention_heads=4, max_position_embeddings=32, padded_vocab_size=256,
              hidden_dropout=0.0, attention_dropout=0.0, seed=3, params_dtype=torch.bfloat16, fp8="hybrid")
    g = torch.Generator().manual_seed(4)
    toks = [torch.randint(0, 250, (2, 33), generator=g) for _ in range(2)]

    def run(fp8_wgrad):
        ps.destroy_model_parallel()
        model = GPTModel(TransformerConfig(**kw, fp8_wgrad=fp8_wgrad))
        assert model.decoder.fp8_state.fp8_wgrad is fp8_wgrad
        ddp = DistributedDataParallel(model, grad_dtype=torch.float32)
        opt = MixedPrecisionAdam(ddp, lr=1e-3, weight_decay=0.0, clip_grad=1.0)
        out = []
        for t in toks:
            ddp.zero_grad_buffer()
            loss = model(t[:, :-1], labels=t[:, 1:]).float().mean()
            loss.backward()
            ddp.finish_grad_sync()
            grads = ddp.grad_data.clone()
            opt.step()
            st = model.decoder.fp8_state
            out.append((loss.item(), grads, st.scale.clone(), st.amax_history.clone()))
        return out

    on, off = run(True), run(False)
    assert all(math.isfinite(o[0]) for o in on)
    assert on[0][0] == off[0][0]                                   # the first forward is the same
    assert not torch.equal(on[0][1], off[0][1])                    # the weight gradients are FP8 products
    assert torch.equal(on[0][2], off[0][2]) and torch.equal(on[0][3], off[0][3])
    assert (on[0][2] != 1).all()
