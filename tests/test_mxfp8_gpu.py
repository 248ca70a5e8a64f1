"""MXFP8 on the GPU (--fp8-recipe mxfp8): the block quantiser (csrc/kernels/mx_quant.hip), the
block-scaled GEMM on the scaled MFMA (csrc/kernels/gemm_mx.hip), ``tp.MXFP8Linear`` and a GPT step,
each against the pure-torch twins in ``ops/functional.py`` or references written here (never
against the kernel itself)."""
import pytest
import torch

from _numerics import assert_rows_close

pytestmark = pytest.mark.gpu

ULP = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _quant_input(shape, dtype, seed):
    """Log-normal magnitudes over many binades plus the special blocks of the CPU test: an all-zero
    block, a power-of-two amax, an element that scales into (464, 512), neighbours 2^20 apart,
    values at both ends of the dtype's range, fp16 subnormals, NaN and +-inf."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(shape, generator=g) * torch.exp(2.5 * torch.randn(shape, generator=g))).to(dtype)
    R, C = shape
    big, tiny = (3.0e38, 1.0e-40) if dtype == torch.bfloat16 else (60000.0, 3.0e-7)
    x[0, :16] = 0
    if R >= 32 and C >= 32:
        x[:32, :32] = 0                                   # zero blocks in both directions
        x[1, 0], x[2, 1] = 4.0, 1.75                      # power-of-two amax
        x[3, :32] = 0.25
        x[3, 5] = 1.9375                                  # e = -8 (E4M3): 1.9375 * 256 = 496, in (464, 512)
        x[4, 3], x[5, 3] = 2.0 ** 10, 2.0 ** -10          # neighbours 2^20 apart (rows and blocks)
        x[6, 0], x[6, 31] = big, -big
        x[7, :32] = 0
        x[7, 2], x[7, 9] = tiny, -tiny / 2
        x[8, 4], x[9, 4], x[10, 4] = float("nan"), float("inf"), float("-inf")
        x[11, :32] = float("inf")                          # no finite value in a row block
    return x.cuda()


@pytest.mark.parametrize("shape", [(1, 32), (64, 128), (80, 160), (257, 1056)])
@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_mx_quantize_rows_match_twin_bytewise(shape, fmt, dtype):
    from smdt_amd.ops import functional as SF
    x = _quant_input(shape, dtype, shape[0] + shape[1])
    q, s = SF.mx_quantize(x, fmt)
    qr, sr = SF.mx_quantize_ref(x, fmt)
    assert q.dtype == SF.FP8_DTYPE[fmt] and q.shape == x.shape and s.dtype == torch.uint8
    assert s.shape == (shape[0], shape[1] // 32)
    bad_q, bad_s = (_bits(q) != _bits(qr)).sum().item(), (s != sr).sum().item()
    print(f"mx_quantize rows {shape} {fmt} {dtype}: {bad_q} differing bytes, {bad_s} differing scales")
    assert bad_q == 0 and bad_s == 0
    assert (s != 255).all()


@pytest.mark.parametrize("shape", [(32, 16), (96, 144), (1056, 272)])
@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_mx_quantize_columns_match_twin_bytewise(shape, fmt, dtype):
    from smdt_amd.ops import functional as SF
    x = _quant_input(shape, dtype, shape[0] * 3 + shape[1])
    qt, st = SF.mx_quantize(x, fmt, columnwise=True)
    qr, sr = SF.mx_quantize_ref(x, fmt, columnwise=True)
    assert qt.shape == (shape[1], shape[0]) and st.shape == (shape[1], shape[0] // 32)
    bad_q, bad_s = (_bits(qt) != _bits(qr)).sum().item(), (st != sr).sum().item()
    print(f"mx_quantize columns {shape} {fmt} {dtype}: {bad_q} differing bytes, {bad_s} differing scales")
    assert bad_q == 0 and bad_s == 0
    assert (st != 255).all()


@pytest.mark.parametrize("shape", [(32, 32), (96, 160), (1056, 288)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_mx_quantize_weight_equals_the_two_calls(shape, dtype):
    from smdt_amd.ops import functional as SF
    w = _quant_input(shape, dtype, 17)
    q, s, qt, st = SF.mx_quantize_weight(w)
    q1, s1 = SF.mx_quantize(w, "e4m3")
    q2, s2 = SF.mx_quantize(w, "e4m3", columnwise=True)
    assert torch.equal(_bits(q), _bits(q1)) and torch.equal(s, s1)
    assert torch.equal(_bits(qt), _bits(q2)) and torch.equal(st, s2)
    qr, sr, qtr, str_ = SF.mx_quantize_weight_ref(w)
    assert torch.equal(_bits(q), _bits(qr)) and torch.equal(s, sr)
    assert torch.equal(_bits(qt), _bits(qtr)) and torch.equal(st, str_)


def test_mx_quantize_rejects_unsupported_shapes():
    from smdt_amd.ops import functional as SF
    from smdt_amd.ops import _ext
    with pytest.raises(ValueError, match=r"\(8, 48\)"):
        SF.mx_quantize(torch.zeros(8, 48, device="cuda", dtype=torch.bfloat16), "e4m3")
    with pytest.raises(ValueError, match=r"\(48, 32\)"):
        SF.mx_quantize(torch.zeros(48, 32, device="cuda", dtype=torch.bfloat16), "e4m3", columnwise=True)
    with pytest.raises(ValueError):
        SF.mx_quantize(torch.zeros(8, 32, device="cuda"), "e4m3")
    with pytest.raises(RuntimeError):      # the binding itself refuses too
        _ext.ext().mx_quantize(torch.zeros(8, 48, device="cuda", dtype=torch.bfloat16), 0, True, False)


_EXACT_VALUES = [0.0, 0.5, -0.5, 1.0, -1.0, 1.5, -1.5, 2.0, -2.0, 3.0, -3.0]


def _exact_operands(M, N, K, afmt, seed):
    """Operand bytes drawn independently for A and B from a few small values, scale bytes drawn
    independently per row and per block from 125..129: every product (at most 9 * 2^4 in quarter
    units of 2^-4) and every partial sum over K <= 512 is exact in fp32."""
    from smdt_amd.ops import functional as SF
    g = torch.Generator().manual_seed(seed)
    vals = torch.tensor(_EXACT_VALUES)
    a = vals[torch.randint(0, len(vals), (M, K), generator=g)].to(SF.FP8_DTYPE[afmt]).cuda()
    b = vals[torch.randint(0, len(vals), (N, K), generator=g)].to(torch.float8_e4m3fn).cuda()
    sa = torch.randint(125, 130, (M, K // 32), generator=g).to(torch.uint8).cuda()
    sb = torch.randint(125, 130, (N, K // 32), generator=g).to(torch.uint8).cuda()
    return a, sa, b, sb


@pytest.mark.parametrize("mnk", [(128, 128, 128), (128, 128, 384), (256, 384, 256), (384, 128, 512)])
@pytest.mark.parametrize("afmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_gemm_mx_exact_data_is_bitwise(mnk, afmt, dtype):
    """Lane maps, scale association and the tile walk: with independent (asymmetric) operand and
    scale bytes a swapped row / column, a scale read from the wrong row or block, a wrong k order
    across blocks or a tile written to the wrong place all change the exact result. The reference
    is the fp32 matmul of the dequantised operands; its sums are exact whatever their order."""
    from smdt_amd.ops import functional as SF
    M, N, K = mnk
    a, sa, b, sb = _exact_operands(M, N, K, afmt, M + 2 * N + 3 * K)
    ref32 = SF.mx_dequantize(a, sa).double() @ SF.mx_dequantize(b, sb).double().t()
    assert ref32.abs().max() < 2 ** 24 and torch.equal(ref32, ref32.float().double())
    out = SF.gemm_mx(a, sa, b, sb, None, dtype)
    ref = SF.gemm_mx_ref(a, sa, b, sb, None, dtype)
    assert out.dtype == dtype and out.shape == (M, N)
    assert torch.equal(ref, ref32.to(dtype))
    bad = (out != ref).sum().item()
    print(f"gemm_mx exact {mnk} {afmt} {dtype}: {bad} of {M * N} differ")
    assert bad == 0


def test_gemm_mx_single_workgroup_walks_every_tile():
    from smdt_amd.ops import functional as SF
    M, N, K = 384, 256, 256
    a, sa, b, sb = _exact_operands(M, N, K, "e5m2", 5)
    bias = torch.arange(N, dtype=torch.float32).sub(N / 2).to(torch.bfloat16).cuda()
    ref = SF.gemm_mx_ref(a, sa, b, sb, bias, torch.bfloat16)
    for cap in (1, 3):
        out = SF.gemm_mx(a, sa, b, sb, bias, torch.bfloat16, max_blocks=cap)
        assert torch.equal(out, ref), cap


@pytest.mark.parametrize("mnk", [(128, 256, 128), (256, 128, 640)])
@pytest.mark.parametrize("afmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_gemm_mx_random_data(mnk, afmt, dtype):
    from smdt_amd.ops import functional as SF
    M, N, K = mnk
    g = torch.Generator().manual_seed(M + K)
    x = (torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-6, 7, (M, 1), generator=g).float())).to(dtype).cuda()
    w = (torch.randn(N, K, generator=g) * torch.exp2(torch.randint(-4, 3, (N, 1), generator=g).float())).to(dtype).cuda()
    a, sa = SF.mx_quantize(x, afmt)
    b, sb = SF.mx_quantize(w, "e4m3")
    bias = torch.randn(N, generator=g).to(dtype).cuda()
    for bi in (None, bias):
        ref = SF.mx_dequantize(a, sa) @ SF.mx_dequantize(b, sb).t()
        if bi is not None:
            ref = ref + bi.float()
        out = SF.gemm_mx(a, sa, b, sb, bi, dtype)
        assert_rows_close(out, ref, ULP[dtype], f"gemm_mx {mnk} {afmt} {dtype} bias={bi is not None}")
        assert_rows_close(SF.gemm_mx_ref(a, sa, b, sb, bi, dtype), ref, ULP[dtype], "gemm_mx_ref")


def test_gemm_mx_refusals_name_the_shape():
    from smdt_amd.ops import functional as SF
    from smdt_amd.ops import _ext

    def ops(M, N, K):
        z = lambda r, c, dt: torch.zeros(r, c, device="cuda").to(dt)
        return (z(M, K, torch.float8_e4m3fn), torch.full((M, K // 32), 127, dtype=torch.uint8, device="cuda"),
                z(N, K, torch.float8_e4m3fn), torch.full((N, K // 32), 127, dtype=torch.uint8, device="cuda"))

    assert SF.gemm_mx_supported(128, 256, 384) and not SF.gemm_mx_supported(120, 128, 128)
    assert _ext.ext().gemm_mx_supported(128, 256, 384) and not _ext.ext().gemm_mx_supported(128, 128, 96)
    with pytest.raises(ValueError, match="120 x 128 x 128"):
        SF.gemm_mx(*ops(120, 128, 128))
    with pytest.raises(ValueError, match="128 x 128 x 96"):
        SF.gemm_mx(*ops(128, 128, 96))
    a, sa, b, sb = ops(128, 128, 256)
    with pytest.raises(ValueError, match="128 x 128 x 128.*contiguous"):
        SF.gemm_mx(a[:, :128], sa[:, :4], b[:, :128], sb[:, :4])
    with pytest.raises(RuntimeError, match="120 x 128 x 128"):      # the binding itself refuses too
        _ext.ext().gemm_mx(*ops(120, 128, 128))
    with pytest.raises(RuntimeError, match="128 x 128 x 128"):
        _ext.ext().gemm_mx(a[:, :128], sa[:, :4].contiguous(), b[:, :128].contiguous(), sb[:, :4].contiguous())


def _indep_dq(t, fmt):
    """Quantise -> dequantise of t [M, K] (blocks along K), written here: frexp / ldexp in float64."""
    fmax, emax = {"e4m3": (448.0, 8), "e5m2": (57344.0, 15)}[fmt]
    dt = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}[fmt]
    M, K = t.shape
    b = t.double().cpu().reshape(M, K // 32, 32)
    a = b.abs().amax(-1)
    _, ex = torch.frexp(a)
    e = torch.where(a == 0, torch.zeros_like(ex), (ex - 1 - emax).clamp(-127, 127))
    unit = torch.ldexp(torch.ones_like(a), e).unsqueeze(-1)
    return ((b / unit).clamp(-fmax, fmax).float().to(dt).double() * unit).reshape(M, K)


def _mx_pair(dtype, seed=0):
    """The same linear (128 -> 384) on the GPU (kernels) and on the CPU (the torch twins)."""
    g = torch.Generator().manual_seed(seed)
    w0 = (0.05 * torch.randn(384, 128, generator=g) * torch.exp2(torch.randint(-3, 4, (384, 1), generator=g).float())).to(dtype)
    b0 = (0.1 * torch.randn(384, generator=g)).to(dtype)
    out = []
    for dev in ("cuda", "cpu"):
        w = torch.nn.Parameter(w0.clone().to(dev))
        w.main_grad = torch.zeros(384, 128, dtype=torch.float32, device=dev)
        out.append((w, torch.nn.Parameter(b0.clone().to(dev))))
    return out, w0, b0, g


def _mx_step(w, b, x, dy, gfmt):
    from smdt_amd.parallel import tensor_parallel as tp
    x = x.detach().clone().to(w.device).requires_grad_()
    y = tp.MXFP8Linear.apply(x, w, b, True, gfmt)
    y.backward(dy.to(w.device))
    tp.flush_deferred_wgrad()
    tp.params_changed()
    return y.detach(), x.grad


@pytest.mark.parametrize("fmt", ["hybrid", "e4m3"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_mxfp8_linear_forward_backward(fmt, dtype):
    """128 tokens x 128 -> 384, two steps: y and dX within one output ulp (of the row maximum) of
    the CPU twin run AND of the independent dequantised matmul written here; main_grad and the bias
    gradient under the criteria of tests/test_fp8_gpu.py."""
    gfmt = "e5m2" if fmt == "hybrid" else "e4m3"
    (gpu, cpu), w0, b0, g = _mx_pair(dtype)
    for step in range(2):
        x = (torch.randn(4, 32, 128, generator=g) * (1 + step)).to(dtype)
        dy = (torch.randn(4, 32, 384, generator=g) * (1 + 3 * step)).to(dtype)
        base = gpu[0].main_grad.clone()
        y, dx = _mx_step(*gpu, x, dy, gfmt)
        yr, dxr = _mx_step(*cpu, x, dy, gfmt)
        assert y.dtype == dtype and dx.dtype == dtype
        assert_rows_close(y, yr, ULP[dtype], f"y step {step}")
        assert_rows_close(dx, dxr, ULP[dtype], f"dX step {step}")
        x2, dy2 = x.reshape(-1, 128), dy.reshape(-1, 384)
        y_ref = (_indep_dq(x2, "e4m3") @ _indep_dq(w0, "e4m3").t() + b0.double()).float()
        dx_ref = (_indep_dq(dy2, gfmt) @ _indep_dq(w0.t().contiguous(), "e4m3").t()).float()
        assert_rows_close(y.reshape(-1, 384), y_ref, ULP[dtype], f"y vs dequantised matmul, step {step}")
        assert_rows_close(dx.reshape(-1, 128), dx_ref, ULP[dtype], f"dX vs dequantised matmul, step {step}")
        assert_rows_close(yr.reshape(-1, 384), y_ref, ULP[dtype], f"twin y, step {step}")
        assert_rows_close(dxr.reshape(-1, 128), dx_ref, ULP[dtype], f"twin dX, step {step}")
        dw_ref = dy2.float().t() @ x2.float()
        assert dw_ref.abs().mean() > 5.0
        torch.testing.assert_close(gpu[0].main_grad, base + dw_ref.cuda(), atol=0.25, rtol=1e-2)
        assert_rows_close(gpu[0].main_grad - base, dw_ref, 1e-3, f"main_grad step {step}")
        db = gpu[1].grad if gpu[1].grad is not None else gpu[1].main_grad
        torch.testing.assert_close(db.float().cpu(), dy2.float().sum(0), atol=1e-2, rtol=2.0 ** -7)
        gpu[1].grad = cpu[1].grad = None


def test_mxfp8_linear_refuses_rows_not_multiple_of_128():
    (gpu, _), _, _, g = _mx_pair(torch.bfloat16)
    with pytest.raises(ValueError, match="120 rows"):
        _mx_step(*gpu, torch.randn(120, 128, generator=g).bfloat16(), torch.zeros(120, 384).bfloat16(), "e5m2")


def test_mxfp8_linear_graph_capture_equals_eager():
    """forward + backward of one linear captured in one graph (nothing reads the host, no state to
    advance); three replays on changing inputs are bitwise equal to eager."""
    from smdt_amd.parallel import tensor_parallel as tp
    dtype = torch.bfloat16
    g = torch.Generator().manual_seed(11)
    w = (0.05 * torch.randn(384, 128, generator=g)).to(dtype).cuda()
    xs = [(torch.randn(128, 128, generator=g) * 4.0 ** i).to(dtype).cuda() for i in range(3)]
    dys = [(1e-2 * torch.randn(128, 384, generator=g) * 8.0 ** i).to(dtype).cuda() for i in range(3)]

    def step(x, dy):
        x = x.detach().requires_grad_()
        y = tp.MXFP8Linear.apply(x, w, None, True, "e5m2")
        (dx,) = torch.autograd.grad(y, x, dy)
        tp.params_changed()                  # the optimizer's: q(W) is made again inside the step
        return y.detach(), dx

    want = [tuple(t.clone() for t in step(x, dy)) for x, dy in zip(xs, dys)]
    sx, sdy = xs[0].clone(), dys[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(sx, sdy)                        # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gy, gdx = step(sx, sdy)
    for i in range(3):
        sx.copy_(xs[i])
        sdy.copy_(dys[i])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gy, want[i][0]), i
        assert torch.equal(gdx, want[i][1]), i


def _gpt_losses(recompute, steps=3):
    from smdt_amd.models.gpt import GPTModel
    from smdt_amd.models.transformer import TransformerConfig
    from smdt_amd.optim.optimizer import MixedPrecisionAdam
    from smdt_amd.parallel import state as ps
    from smdt_amd.parallel import tensor_parallel as tp
    from smdt_amd.parallel.distributed import DistributedDataParallel
    ps.destroy_model_parallel()
    cfg = TransformerConfig(num_layers=2, hidden_size=128, num_attention_heads=2, max_position_embeddings=128,
                            padded_vocab_size=512, hidden_dropout=0.0, attention_dropout=0.0, seed=3,
                            params_dtype=torch.bfloat16, fp8="hybrid", fp8_recipe="mxfp8",
                            recompute_granularity="full" if recompute else None)
    model = GPTModel(cfg, device="cuda")
    assert not any(isinstance(m, tp.FP8State) for m in model.modules())
    assert not any("fp8" in k for k in model.state_dict())
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
    return torch.stack(losses)


@pytest.mark.parametrize("recompute", [False, True])
def test_mxfp8_gpt_step_matches_twin_run(recompute, monkeypatch):
    """2 layers, h 128, 2 heads, seq 128, mbs 2, bf16 + hybrid + mxfp8, three optimizer steps: the
    per-token losses of the kernel run against the same run on the torch twins
    (SMDT_DISABLE_KERNELS=1), as ``test_fp8_gpt_step_matches_twin_run`` compares its own."""
    import warnings
    got = _gpt_losses(recompute)
    monkeypatch.setenv("SMDT_DISABLE_KERNELS", "1")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = _gpt_losses(recompute)
    print(f"mxfp8 gpt step recompute={recompute}: max |loss diff| {(got - want).abs().max().item():.4g}, "
          f"mean loss {want.mean().item():.4f}")
    assert torch.isfinite(got).all()
    torch.testing.assert_close(got, want, atol=0.1, rtol=1e-2)
