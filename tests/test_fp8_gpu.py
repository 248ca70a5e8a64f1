"""FP8 linears on the GPU: the quantise / scale-update kernels (csrc/kernels/fp8_quant.hip), the
per-tensor-scaled FP8 GEMM, the FP8 linear and a GPT step, each against the pure-torch twins in
``ops/functional.py`` (never against the kernel itself)."""
import pytest
import torch

from _numerics import assert_rows_close

pytestmark = pytest.mark.gpu

ULP = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _specials(fmt, scale, dtype):
    """Values whose product with ``scale`` is 0, exactly +-max, beyond +-max, FP8 subnormals and
    exact ties between two FP8 values (exact for the power-of-two scales; plain values otherwise)."""
    mx = 448.0 if fmt == "e4m3" else 57344.0
    sub = 2.0 ** -9 if fmt == "e4m3" else 2.0 ** -16          # smallest subnormal
    ties = [1.0625, 1.1875, -1.0625] if fmt == "e4m3" else [1.125, 1.375, -1.125]
    v = [0.0, mx, -mx, mx * 1.25, -mx * 1.25, sub, 3 * sub, -5 * sub, sub / 2, 1.5 * sub] + ties
    return (torch.tensor(v, dtype=torch.float32) / scale).to(dtype)


@pytest.mark.parametrize("shape", [(64, 64), (1, 16), (80, 144), (257, 1040)])
@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_fp8_quantize_matches_twin_bytewise(shape, fmt, dtype):
    from smdt_amd.ops import functional as SF
    g = torch.Generator().manual_seed(shape[0] * 7 + shape[1])
    for scale in (1.0, 0.37, 32.0):
        x = (torch.randn(shape, generator=g) * torch.exp(2.5 * torch.randn(shape, generator=g)) / scale).to(dtype)
        sp = _specials(fmt, scale, dtype)
        x.view(-1)[:sp.numel()] = sp
        x = x.cuda()
        st = torch.tensor([scale], device="cuda")
        for transpose in (False, True):
            amax = torch.zeros(1, device="cuda")
            amax_ref = torch.zeros(1, device="cuda")
            out = SF.fp8_quantize(x, st, amax, fmt, transpose=transpose)
            q_ref = SF.fp8_quantize_ref(x, st, amax_ref, fmt)
            q = out[0] if transpose else out
            assert q.dtype == SF.FP8_DTYPE[fmt] and q.shape == x.shape
            bad = (_bits(q) != _bits(q_ref)).sum().item()
            print(f"fp8_quantize {shape} {fmt} {dtype} scale {scale} T={transpose}: {bad} differing bytes")
            assert bad == 0, (shape, fmt, dtype, scale, bad)
            if transpose:
                assert out[1].shape == (shape[1], shape[0])
                assert torch.equal(_bits(out[1]), _bits(q).t())
            assert torch.equal(amax.view(torch.int32), amax_ref.view(torch.int32))
            assert torch.equal(amax.view(torch.int32), x.float().abs().max().reshape(1).view(torch.int32))
            # the merge is a max: quantising again (activation recompute) changes nothing
            SF.fp8_quantize(x, st, amax, fmt, transpose=transpose)
            assert torch.equal(amax.view(torch.int32), amax_ref.view(torch.int32))


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_fp8_quantize_nan_and_inf(fmt, dtype):
    """A NaN comes out as an FP8 NaN (the twin's byte), +-inf saturates, amax ends non-finite."""
    from smdt_amd.ops import functional as SF
    x = torch.randn(80, 144, generator=torch.Generator().manual_seed(5)).to(dtype)
    x[3, 17] = float("nan")
    x[70, 100] = float("inf")
    x[71, 101] = float("-inf")
    x = x.cuda()
    st = torch.tensor([0.37], device="cuda")
    amax = torch.zeros(1, device="cuda")
    q, qt = SF.fp8_quantize(x, st, amax, fmt, transpose=True)
    q_ref = SF.fp8_quantize_ref(x, st, torch.zeros(1, device="cuda"), fmt)
    assert torch.equal(_bits(q), _bits(q_ref))
    assert torch.equal(_bits(qt), _bits(q).t())
    assert torch.isnan(q[3, 17].float())
    mx = SF.FP8_MAX[fmt]
    assert q[70, 100].float().item() == mx and q[71, 101].float().item() == -mx
    assert not torch.isfinite(amax).item()
    # inf alone: amax is exactly inf
    x[3, 17] = 0
    amax.zero_()
    SF.fp8_quantize(x, st, amax, fmt)
    assert torch.isinf(amax).item()


def test_fp8_quantize_rejects_unsupported_shapes():
    from smdt_amd.ops import functional as SF
    st, am = torch.ones(1, device="cuda"), torch.zeros(1, device="cuda")
    with pytest.raises(ValueError):
        SF.fp8_quantize(torch.zeros(8, 24, device="cuda", dtype=torch.bfloat16), st, am, "e4m3")
    with pytest.raises(ValueError):
        SF.fp8_quantize(torch.zeros(8, 32, device="cuda"), st, am, "e4m3")
    with pytest.raises(RuntimeError):      # the binding itself refuses too
        from smdt_amd.ops import _ext
        _ext.ext().fp8_quantize(torch.zeros(8, 24, device="cuda", dtype=torch.bfloat16), st, am, 0, False)


@pytest.mark.parametrize("algo,H,margin", [("most_recent", 1, 0), ("max", 4, 2), ("most_recent", 4, 1)])
def test_fp8_update_scales_matches_twin_bitwise(algo, H, margin):
    from smdt_amd.ops import functional as SF
    T = 37
    g = torch.Generator().manual_seed(H + margin)
    fm = torch.full((T,), 448.0)
    fm[2::3] = 57344.0
    tabs = []
    for dev in ("cuda", "cpu"):
        tabs.append([torch.ones(T, device=dev), torch.zeros(T, H, device=dev), torch.zeros(T, device=dev), fm.to(dev)])
    for step in range(5):
        am = torch.exp(4 * torch.randn(T, generator=g))
        am[step] = 0.0
        am[step + 7] = float("inf")
        am[step + 14] = float("nan")
        am[20] = 1e-42                      # fmt_max / amax overflows: the scale is kept
        for tab in tabs:
            tab[2].copy_(am)
            SF.fp8_update_scales(tab[0], tab[1], tab[2], tab[3], margin, algo)
        (s, h, a, _), (sr, hr, ar, _) = tabs
        assert torch.equal(s.cpu().view(torch.int32), sr.view(torch.int32)), step
        assert torch.equal(torch.nan_to_num(h.cpu(), nan=-1.0), torch.nan_to_num(hr, nan=-1.0)), step
        assert torch.equal(a.cpu(), torch.zeros(T)) and torch.equal(ar, torch.zeros(T))
        assert torch.isfinite(s).all()


@pytest.mark.parametrize("mnk", [(128, 64, 64), (272, 192, 80)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("afmt", ["e4m3", "e5m2"])
def test_fp8_gemm_matches_fp32_matmul_of_dequantised_operands(mnk, dtype, afmt):
    from smdt_amd.ops import functional as SF
    M, N, K = mnk
    g = torch.Generator().manual_seed(M + K)
    sa, sb = torch.tensor([3.7], device="cuda"), torch.tensor([0.8], device="cuda")
    a = (torch.randn(M, K, generator=g).cuda() * sa).clamp(-400, 400).to(SF.FP8_DTYPE[afmt])
    b = (torch.randn(N, K, generator=g).cuda() * sb).to(torch.float8_e4m3fn)
    bias = torch.randn(N, generator=g).to(dtype).cuda()
    ia, ib = 1.0 / sa, 1.0 / sb
    for bi in (None, bias):
        out = SF.fp8_gemm(a, b, ia, ib, bi, dtype)
        ref = (a.float() * ia) @ (b.float() * ib).t()
        if bi is not None:
            ref = ref + bi.float()
        assert out.dtype == dtype and out.shape == (M, N)
        assert_rows_close(out, ref, ULP[dtype], f"fp8_gemm {mnk} {dtype} {afmt} bias={bi is not None}")
        # the twin itself sits inside the same bound
        assert_rows_close(SF.fp8_gemm_ref(a, b, ia, ib, bi, dtype), ref, ULP[dtype], "fp8_gemm_ref")


def _linear_pair(fmt, dtype, H=1, algo="most_recent", margin=0, bias=True, seed=0):
    """The same FP8 linear (64 -> 192) on the GPU (kernels) and on the CPU (the torch twin)."""
    from smdt_amd.parallel import tensor_parallel as tp
    g = torch.Generator().manual_seed(seed)
    w0 = (0.05 * torch.randn(192, 64, generator=g)).to(dtype)
    b0 = (0.1 * torch.randn(192, generator=g)).to(dtype)
    out = []
    for dev in ("cuda", "cpu"):
        st = tp.FP8State(1, fmt, margin=margin, history_len=H, algo=algo, device=dev)
        w = torch.nn.Parameter(w0.clone().to(dev))
        w.main_grad = torch.zeros(192, 64, dtype=torch.float32, device=dev)
        b = torch.nn.Parameter(b0.clone().to(dev)) if bias else None
        out.append((st, w, b))
    return out, g


def _linear_step(st, w, b, x, dy):
    from smdt_amd.parallel import tensor_parallel as tp
    x = x.detach().clone().to(w.device).requires_grad_()
    y = tp.FP8Linear.apply(x, w, b, True, st, 0)
    y.backward(dy.to(w.device))
    tp.flush_deferred_wgrad()
    return y.detach(), x.grad


def _dequantised(t, scale, fmt):
    """Hand-written quantise -> dequantise of ``t`` (fp32 result), independent of the library code."""
    mx = {"e4m3": 448.0, "e5m2": 57344.0}[fmt]
    dt = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}[fmt]
    return (t.float() * scale).clamp(-mx, mx).to(dt).float() / scale


@pytest.mark.parametrize("fmt", ["hybrid", "e4m3"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_fp8_linear_forward_backward_and_scale_state(fmt, dtype):
    """64 tokens x 64 -> 192, three steps with a scale update after each.

    * y and dX within one output ulp (of the row maximum) of the twin's, AND of an independent
      reference written here: the fp32 matmul of the dequantised operands, y = dq(x) dq(W)^T + b and
      dX = dq(dY) dq(W), with the scales read from the table before the step. A wrong inverse
      scale, weight slot, gradient format or q(W) in place of q(W)^T fails the second.
    * main_grad against fp32 dY^T x of the 16-bit operands, with O(1) dY so that entries are
      O(10-100): the criterion of ``test_wgrad_accumulates_into_fp32_main_grad`` and a row-relative
      1e-3. The products of 16-bit values are exact in fp32 and 64 of them are accumulated, so the
      kernel's error is below 64 * 2^-24 of the sum of magnitudes, orders under 1e-3; a wgrad fed
      the dequantised FP8 x or dY (2^-4 / 2^-3 per element) lands near 1e-2.
    * the scale / history tables bitwise equal to the twin's after every step."""
    (gpu, cpu), g = _linear_pair(fmt, dtype, H=4, algo="max", margin=1)
    gfmt = "e5m2" if fmt == "hybrid" else "e4m3"
    for step in range(3):
        x = (torch.randn(8, 8, 64, generator=g) * (1 + step)).to(dtype)
        dy = (torch.randn(8, 8, 192, generator=g) * (1 + 3 * step)).to(dtype)
        sx, sw, sg = gpu[0].scale.cpu().tolist()
        if step:
            assert sx != 1.0 and sw != 1.0 and sg != 1.0
        base = gpu[1].main_grad.clone()
        y, dx = _linear_step(*gpu, x, dy)
        yr, dxr = _linear_step(*cpu, x, dy)
        assert y.dtype == dtype and dx.dtype == dtype
        assert_rows_close(y, yr, ULP[dtype], f"y step {step}")
        assert_rows_close(dx, dxr, ULP[dtype], f"dX step {step}")
        # independent reference
        x2, dy2 = x.reshape(-1, 64), dy.reshape(-1, 192)
        wq = _dequantised(cpu[1].detach(), sw, "e4m3")
        y_ref = _dequantised(x2, sx, "e4m3") @ wq.t() + cpu[2].detach().float()
        dx_ref = _dequantised(dy2, sg, gfmt) @ wq
        assert_rows_close(y.reshape(-1, 192), y_ref, ULP[dtype], f"y vs dequantised matmul, step {step}")
        assert_rows_close(dx.reshape(-1, 64), dx_ref, ULP[dtype], f"dX vs dequantised matmul, step {step}")
        assert_rows_close(yr.reshape(-1, 192), y_ref, ULP[dtype], f"twin y, step {step}")
        assert_rows_close(dxr.reshape(-1, 64), dx_ref, ULP[dtype], f"twin dX, step {step}")
        dw_ref = dy2.float().t() @ x2.float()
        assert dw_ref.abs().mean() > 5.0
        torch.testing.assert_close(gpu[1].main_grad, base + dw_ref.cuda(), atol=0.25, rtol=1e-2)
        assert_rows_close(gpu[1].main_grad - base, dw_ref, 1e-3, f"main_grad step {step}")
        db_ref = dy2.float().sum(0)
        torch.testing.assert_close(gpu[2].grad.float().cpu(), db_ref, atol=1e-2, rtol=2.0 ** -7)
        gpu[2].grad = cpu[2].grad = None
        for st in (gpu[0], cpu[0]):
            st.after_optimizer_step()
        for name in ("scale", "amax_history", "amax", "scale_inv"):
            a, r = getattr(gpu[0], name).cpu(), getattr(cpu[0], name)
            assert torch.equal(a.view(torch.int32), r.view(torch.int32)), (name, step, a, r)
    assert not torch.equal(gpu[0].scale.cpu(), torch.ones(3))
    assert (gpu[0].amax_history[:, :3] != 0).all()      # three steps recorded


def test_fp8_linear_refuses_rows_not_multiple_of_16():
    (gpu, _), g = _linear_pair("hybrid", torch.bfloat16)
    x = torch.randn(9, 64, generator=g).bfloat16()
    with pytest.raises(ValueError, match="9 rows"):
        _linear_step(*gpu, x, torch.zeros(9, 192).bfloat16())


def test_fp8_linear_graph_capture_advances_its_own_scales():
    """forward + backward + fp8_update_scales of one linear captured in one graph; three replays
    with new inputs equal three eager steps (outputs and scale tables)."""
    from smdt_amd.parallel import tensor_parallel as tp
    dtype = torch.bfloat16
    g = torch.Generator().manual_seed(11)
    w = (0.05 * torch.randn(192, 64, generator=g)).to(dtype).cuda()
    xs = [(torch.randn(64, 64, generator=g) * (1 + i)).to(dtype).cuda() for i in range(3)]
    dys = [(1e-2 * torch.randn(64, 192, generator=g) * (1 + i)).to(dtype).cuda() for i in range(3)]

    def step(st, x, dy):
        x = x.detach().requires_grad_()
        y = tp.FP8Linear.apply(x, w, None, True, st, 0)
        (dx,) = torch.autograd.grad(y, x, dy)
        st._wq.clear()                       # the optimizer's params_changed()
        st.after_optimizer_step()
        return y.detach(), dx

    eager = tp.FP8State(1, "hybrid", history_len=2, algo="max", device="cuda")
    want = [step(eager, x, dy) for x, dy in zip(xs, dys)]
    want = [(y.clone(), dx.clone()) for y, dx in want]

    st = tp.FP8State(1, "hybrid", history_len=2, algo="max", device="cuda")
    sx, sdy = xs[0].clone(), dys[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(st, sx, sdy)                    # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.no_grad():
        st.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gy, gdx = step(st, sx, sdy)
    with torch.no_grad():
        st.reset()                           # the capture pass itself ran nothing
    for i in range(3):
        sx.copy_(xs[i])
        sdy.copy_(dys[i])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gy, want[i][0]), i
        assert torch.equal(gdx, want[i][1]), i
    for name in ("scale", "amax_history", "amax"):
        assert torch.equal(getattr(st, name), getattr(eager, name)), name
    assert not torch.equal(st.scale, torch.ones_like(st.scale))


def _gpt_losses(recompute, steps=3):
    from smdt_amd.models.gpt import GPTModel
    from smdt_amd.models.transformer import TransformerConfig
    from smdt_amd.optim.optimizer import MixedPrecisionAdam
    from smdt_amd.parallel import state as ps
    from smdt_amd.parallel.distributed import DistributedDataParallel
    ps.destroy_model_parallel()
    cfg = TransformerConfig(num_layers=2, hidden_size=128, num_attention_heads=2, max_position_embeddings=128,
                            padded_vocab_size=512, hidden_dropout=0.0, attention_dropout=0.0, seed=3,
                            params_dtype=torch.bfloat16, fp8="hybrid",
                            recompute_granularity="full" if recompute else None)
    model = GPTModel(cfg, device="cuda")
    ddp = DistributedDataParallel(model, grad_dtype=torch.float32)
    opt = MixedPrecisionAdam(ddp, lr=1e-3, weight_decay=0.01, clip_grad=1.0)
    toks = torch.randint(0, 500, (2, 129), generator=torch.Generator().manual_seed(4)).cuda()
    losses = []
    for _ in range(steps):
        ddp.zero_grad_buffer()
        loss = model(toks[:, :-1], labels=toks[:, 1:])
        loss.float().mean().backward()
        ddp.finish_grad_sync()
        opt.step()
        losses.append(loss.detach().float().cpu())
    return torch.stack(losses), model.decoder.fp8_state.scale.cpu().clone()


@pytest.mark.parametrize("recompute", [False, True])
def test_fp8_gpt_step_matches_twin_run(recompute, monkeypatch):
    """2 layers, h 128, 2 heads, seq 128, mbs 2, bf16 + hybrid FP8, three optimizer steps: the
    per-token losses of the kernel run against the same run on the torch twins
    (SMDT_DISABLE_KERNELS=1), with the loss tolerance of the gemm_tn GPT-step test."""
    import warnings
    got, scales = _gpt_losses(recompute)
    monkeypatch.setenv("SMDT_DISABLE_KERNELS", "1")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want, scales_ref = _gpt_losses(recompute)
    print(f"fp8 gpt step recompute={recompute}: max |loss diff| {(got - want).abs().max().item():.4g}, "
          f"mean loss {want.mean().item():.4f}")
    assert torch.isfinite(got).all()
    assert not torch.equal(scales, torch.ones_like(scales))
    torch.testing.assert_close(got, want, atol=0.1, rtol=1e-2)
