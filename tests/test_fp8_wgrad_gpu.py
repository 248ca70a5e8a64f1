"""--fp8-wgrad on the GPU: the FP8 weight-gradient kernel (csrc/kernels/wgrad_fp8.hip) against its
torch twin, bit for bit on exactly representable inputs and under the fp32 summation bound on
random ones; the binding's refusals; FP8Linear, graph capture and a small GPT step with it on."""
import warnings

import pytest
import torch

from _numerics import wgrad_exact_case, wgrad_exact_twin

pytestmark = pytest.mark.gpu

S = 64                                   # the kernel's stage: rows of m per LDS stage
FMT = {"e5m2": torch.float8_e5m2, "e4m3": torch.float8_e4m3fn}


def _ext():
    from smdt_amd.ops import _ext
    return _ext.ext()


def _exact_case(g, M, N, K, fmt):
    """Operands from {0, +-0.5, +-1, +-2} (exact in E5M2 and E4M3), a target of small integers."""
    return wgrad_exact_case(g, M, N, K, FMT[fmt], FMT["e4m3"])[:3]


def _twin(mg, a, b, inv_dy, inv_x, overwrite):
    """The twin on the CPU (SF.fp8_wgrad_ref), checked against float64: see wgrad_exact_twin."""
    return wgrad_exact_twin(mg, a, b, overwrite, inv_dy, inv_x)


INV_DY, INV_X = 0.5, 4.0

# (M, N, K): one stage / fewer stages than ring buffers / the ring wraps / partial tiles in n and k
# (clamped loads, skipped stores) / two tiles share the B strip / 32 stages, where the tail tiles
# of a launch are cut along m and added with atomics (4 tiles: 4 pieces each on the whole chip,
# 2 pieces each with cus = 8)
SHAPES = [(S, 256, 256), (3 * S, 256, 256), (5 * S, 256, 256), (2 * S, 272, 80), (4 * S, 512, 256),
          (32 * S, 512, 512)]


@pytest.fixture(scope="module")
def exact_cases():
    g = torch.Generator().manual_seed(21)
    inv = (torch.tensor([INV_DY]), torch.tensor([INV_X]))
    out = {}
    for fmt in FMT:
        for shape in SHAPES:
            a, b, mg = _exact_case(g, *shape, fmt)
            out[fmt, shape] = (a, b, mg, {ow: _twin(mg, a, b, *inv, ow) for ow in (False, True)})
    return out


@pytest.mark.parametrize("cus", [0, 8])
@pytest.mark.parametrize("overwrite", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("fmt", ["e5m2", "e4m3"])
def test_fp8_wgrad_kernel_equals_twin_bit_for_bit(exact_cases, fmt, shape, overwrite, cus):
    a, b, mg, want = exact_cases[fmt, shape]
    inv_dy, inv_x = torch.tensor([INV_DY]).cuda(), torch.tensor([INV_X]).cuda()
    got = mg.clone().cuda()
    assert _ext().wgrad_fp8_grouped([got], [a.cuda()], [b.cuda()], [inv_dy], [inv_x], [overwrite], cus)
    torch.cuda.synchronize()
    diff = (got.cpu() != want[overwrite])
    assert not diff.any(), (f"{int(diff.sum())} of {diff.numel()} elements differ; rows "
                            f"{diff.any(1).nonzero().flatten()[:8].tolist()}, cols {diff.any(0).nonzero().flatten()[:8].tolist()}")


@pytest.mark.parametrize("group,cus", [
    ([(S, 256, 256), (2 * S, 272, 80), (3 * S, 512, 256)], 0),     # whole tiles, three shapes
    ([(S, 256, 256), (2 * S, 272, 80), (3 * S, 512, 256)], 8),
    ([(32 * S, 256, 256), (S, 272, 80)], 0),       # a split tail with a shorter problem in it (empty pieces)
])
@pytest.mark.parametrize("fmt", ["e5m2", "e4m3"])
def test_fp8_wgrad_grouped_launch_equals_twin_bit_for_bit(fmt, group, cus):
    g = torch.Generator().manual_seed(22)
    inv = (torch.tensor([INV_DY]), torch.tensor([INV_X]))
    cases = [_exact_case(g, *shape, fmt) for shape in group]
    ows = [i % 2 == 1 for i in range(len(group))]
    want = [_twin(mg, a, b, *inv, ow) for (a, b, mg), ow in zip(cases, ows)]
    got = [mg.clone().cuda() for _, _, mg in cases]
    n = len(group)
    assert _ext().wgrad_fp8_grouped(got, [c[0].cuda() for c in cases], [c[1].cuda() for c in cases],
                                    [inv[0].cuda()] * n, [inv[1].cuda()] * n, ows, cus)
    torch.cuda.synchronize()
    for i in range(n):
        assert torch.equal(got[i].cpu(), want[i]), (i, group[i])


def _bound(a, b, inv_dy, inv_x, M):
    """The standard fp32 summation bound: 2 (M + 2) 2^-24 (|A|^T |B|) inv_dy inv_x, per element."""
    return 2 * (M + 2) * 2.0 ** -24 * (a.double().abs().t() @ b.double().abs()) * inv_dy * inv_x


@pytest.mark.parametrize("fmt", ["e5m2", "e4m3"])
def test_fp8_wgrad_kernel_random_data_within_the_fp32_summation_bound(fmt):
    from smdt_amd.ops import functional as SF
    M, N, K = 4 * S, 272, 336
    g = torch.Generator().manual_seed(23)
    sdy, sx = 410.0, 37.0
    mx = 57344.0 if fmt == "e5m2" else 448.0
    a = (3 * torch.randn(M, N, generator=g) * sdy).clamp(-mx, mx).to(FMT[fmt])
    b = (torch.randn(M, K, generator=g) * sx).clamp(-448, 448).to(FMT["e4m3"])
    inv_dy, inv_x = torch.tensor([1 / sdy]), torch.tensor([1 / sx])
    R = (a.double().t() @ b.double()) * inv_dy.double() * inv_x.double()
    bound = _bound(a, b, inv_dy.double(), inv_x.double(), M)
    got = torch.zeros(N, K, device="cuda")
    SF.fp8_wgrad(got, a.cuda(), b.cuda(), inv_dy.cuda(), inv_x.cuda())
    err = (got.cpu().double() - R).abs()
    print(f"fp8 wgrad {fmt}: max err / bound {(err / bound).max().item():.3g}, max |R| {R.abs().max().item():.3g}")
    assert (err <= bound).all()
    assert R.abs().mean() > 100 * bound.mean()             # the bound is tight against the values


def test_fp8_wgrad_binding_refuses_what_the_kernel_cannot_take():
    from smdt_amd.ops import functional as SF
    C = _ext()
    dev = "cuda"
    mg = torch.zeros(256, 256, device=dev)
    a = torch.zeros(128, 256, device=dev).to(torch.float8_e5m2)
    b = torch.zeros(128, 256, device=dev).to(torch.float8_e4m3fn)
    one = torch.ones(1, device=dev)

    def call(mgs, dys, xs, inv=None):
        n = len(mgs)
        return C.wgrad_fp8_grouped(mgs, dys, xs, inv or [one] * n, [one] * n, [False] * n)

    before = mg.clone()
    assert not call([mg], [a], [b.view(torch.uint8).view(torch.float8_e5m2)])          # x must be E4M3
    assert not call([mg], [a.view(torch.uint8).view(torch.int8)], [b])                 # dy must be FP8
    assert not call([mg], [torch.zeros(128, 256, device=dev).bfloat16()], [b])
    assert not call([mg], [a.t().contiguous().t()], [b])                                # non-contiguous dy
    assert not call([mg], [a], [torch.zeros(256, 128, device=dev).to(torch.float8_e4m3fn).t()])
    assert not call([mg], [a[:96]], [b[:96]])                                           # M not a multiple of 64
    assert not call([mg], [a[:, :72].contiguous()], [b])                                # N not a multiple of 16
    assert not call([mg.half()], [a], [b])                                              # fp32 targets only
    assert not call([mg[:128]], [a], [b])                                               # target size
    assert not call([mg, mg], [a, a], [b, b])                                           # overlapping targets
    assert not call([mg, torch.zeros_like(mg)], [a, a.view(torch.uint8).view(torch.float8_e4m3fn)], [b, b])
    with pytest.raises(RuntimeError):
        call([mg], [a], [b], inv=[torch.ones(1)])                                       # a factor on the host
    with pytest.raises(RuntimeError, match="multiple of 64"):
        SF.fp8_wgrad(mg, a[:96], b[:96], one, one)
    torch.cuda.synchronize()
    assert torch.equal(mg, before)
    assert C.wgrad_fp8_supported(64, 16, 16) and not C.wgrad_fp8_supported(32, 256, 256)
    assert SF.fp8_wgrad_supported(64, 16, 16) and not SF.fp8_wgrad_supported(32, 256, 256)


def _linear(fmt, dtype, dev, fp8_wgrad, w0, b0):
    from smdt_amd.parallel import tensor_parallel as tp
    st = tp.FP8State(1, fmt, margin=1, history_len=2, algo="max", device=dev, fp8_wgrad=fp8_wgrad)
    w = torch.nn.Parameter(w0.clone().to(dev))
    w.main_grad = torch.zeros(w0.shape, dtype=torch.float32, device=dev)
    return st, w, torch.nn.Parameter(b0.clone().to(dev))


def _linear_step(st, w, b, x, dy):
    from smdt_amd.parallel import tensor_parallel as tp
    x = x.detach().clone().to(w.device).requires_grad_()
    y = tp.FP8Linear.apply(x, w, b, True, st, 0)
    y.backward(dy.to(w.device))
    tp.flush_deferred_wgrad()
    return y.detach(), x.grad


@pytest.mark.parametrize("fmt", ["hybrid", "e4m3"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_fp8_linear_with_fp8_wgrad(fmt, dtype):
    """128 tokens, 64 -> 80, two steps with a scale update between them. main_grad against the
    float64 product of the dequantised bytes under the fp32 summation bound; y, dX and the amax /
    scale state bit-identical to the run with fp8_wgrad off (the forward and dgrad are the same
    calls); the bias gradient the 16-bit column sums."""
    g = torch.Generator().manual_seed(31)
    w0 = (0.05 * torch.randn(80, 64, generator=g)).to(dtype)
    b0 = (0.1 * torch.randn(80, generator=g)).to(dtype)
    on, off = _linear(fmt, dtype, "cuda", True, w0, b0), _linear(fmt, dtype, "cuda", False, w0, b0)
    gdt = FMT["e5m2" if fmt == "hybrid" else "e4m3"]
    gmx = 57344.0 if fmt == "hybrid" else 448.0
    for step in range(2):
        x = (torch.randn(2, 64, 64, generator=g) * (1 + step)).to(dtype)
        dy = (torch.randn(2, 64, 80, generator=g) * (1 + 3 * step)).to(dtype)
        sx, _, sg = on[0].scale.cpu().double().tolist()
        ix, _, ig = on[0].scale_inv.cpu().double().tolist()
        on[1].main_grad.zero_()
        off[1].main_grad.zero_()
        y1, dx1 = _linear_step(*on, x, dy)
        y0, dx0 = _linear_step(*off, x, dy)
        assert torch.equal(y1, y0) and torch.equal(dx1, dx0), step
        qx = (x.reshape(-1, 64).float() * float(sx)).clamp(-448, 448).to(FMT["e4m3"])
        qdy = (dy.reshape(-1, 80).float() * float(sg)).clamp(-gmx, gmx).to(gdt)
        R = (qdy.double().t() @ qx.double()) * ig * ix
        bound = _bound(qdy, qx, ig, ix, 128)
        err = (on[1].main_grad.cpu().double() - R).abs()
        print(f"fp8 linear {fmt} {dtype} step {step}: max err / bound {(err / bound).max().item():.3g}")
        assert (err <= bound).all(), step
        assert not torch.equal(on[1].main_grad, off[1].main_grad)
        torch.testing.assert_close(on[2].grad.float().cpu(), dy.reshape(-1, 80).float().sum(0), atol=1e-2 * (1 + 3 * step),
                                   rtol=2.0 ** -7)
        assert torch.equal(on[2].grad, off[2].grad)
        on[2].grad = off[2].grad = None
        for st in (on[0], off[0]):
            st.after_optimizer_step()
        for name in ("scale", "amax_history", "amax", "scale_inv"):
            assert torch.equal(getattr(on[0], name), getattr(off[0], name)), (name, step)
    assert not torch.equal(on[0].scale.cpu(), torch.ones(3))


def test_fp8_linear_fp8_wgrad_graph_capture():
    """forward + backward (weight gradient into main_grad through the deferred queue) + scale update
    of one linear with fp8_wgrad captured in one graph; three replays with new inputs equal three
    eager steps bit for bit: outputs, main_grad and scale tables. 128 tokens are two stages, so no
    tile of the launch is split and nothing is added with atomics: bit-identity is well defined."""
    from smdt_amd.parallel import tensor_parallel as tp
    dtype = torch.bfloat16
    g = torch.Generator().manual_seed(11)
    w = torch.nn.Parameter((0.05 * torch.randn(80, 64, generator=g)).to(dtype).cuda())
    xs = [(torch.randn(128, 64, generator=g) * (1 + i)).to(dtype).cuda() for i in range(3)]
    dys = [(1e-2 * torch.randn(128, 80, generator=g) * (1 + i)).to(dtype).cuda() for i in range(3)]

    def step(st, x, dy):
        x = x.detach().requires_grad_()
        y = tp.FP8Linear.apply(x, w, None, True, st, 0)
        (dx,) = torch.autograd.grad(y, x, dy)
        tp.flush_deferred_wgrad()
        st._wq.clear()                       # the optimizer's params_changed()
        st.after_optimizer_step()
        return y.detach(), dx

    def fresh():
        return tp.FP8State(1, "hybrid", history_len=2, algo="max", device="cuda", fp8_wgrad=True)

    w.main_grad = torch.zeros(80, 64, device="cuda")
    eager = fresh()
    want = []
    for x, dy in zip(xs, dys):
        y, dx = step(eager, x, dy)
        want.append((y.clone(), dx.clone(), w.main_grad.clone()))
    assert want[0][2].abs().max() > 0

    st = fresh()
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
        w.main_grad.zero_()
    for i in range(3):
        sx.copy_(xs[i])
        sdy.copy_(dys[i])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gy, want[i][0]), i
        assert torch.equal(gdx, want[i][1]), i
        assert torch.equal(w.main_grad, want[i][2]), i
    for name in ("scale", "amax_history", "amax"):
        assert torch.equal(getattr(st, name), getattr(eager, name)), name
    assert not torch.equal(st.scale, torch.ones_like(st.scale))


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
                            params_dtype=torch.bfloat16, fp8="hybrid", fp8_wgrad=True,
                            recompute_granularity="full" if recompute else None)
    model = GPTModel(cfg, device="cuda")
    ddp = DistributedDataParallel(model, grad_dtype=torch.float32)
    opt = MixedPrecisionAdam(ddp, lr=1e-3, weight_decay=0.01, clip_grad=1.0)
    toks = torch.randint(0, 500, (2, 129), generator=torch.Generator().manual_seed(4)).cuda()
    losses = []
    items0 = tp.DEFERRED_WGRAD.stats["items"]
    for _ in range(steps):
        ddp.zero_grad_buffer()
        loss = model(toks[:, :-1], labels=toks[:, 1:])
        loss.float().mean().backward()
        ddp.finish_grad_sync()
        opt.step()
        losses.append(loss.detach().float().cpu())
    return torch.stack(losses), model.decoder.fp8_state.scale.cpu().clone(), tp.DEFERRED_WGRAD.stats["items"] - items0


@pytest.mark.parametrize("recompute", [False, True])
def test_fp8_wgrad_gpt_step_matches_twin_run(recompute, monkeypatch):
    """The shape of test_fp8_gpt_step_matches_twin_run (2 layers, h 128, 2 heads, seq 128, mbs 2,
    bf16 + hybrid FP8, three optimizer steps) with fp8_wgrad on: the per-token losses of the kernel
    run against the same run on the torch twins (SMDT_DISABLE_KERNELS=1), with that test's
    tolerance."""
    got, scales, queued = _gpt_losses(recompute)
    if not recompute:       # the eight FP8 linears went through the deferred queue; under recompute autograd
        assert queued >= 3 * 8      # hands FP8Linear a detached weight (no main_grad): the product is returned
    monkeypatch.setenv("SMDT_DISABLE_KERNELS", "1")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want, scales_ref, _ = _gpt_losses(recompute)
    print(f"fp8 wgrad gpt step recompute={recompute}: max |loss diff| {(got - want).abs().max().item():.4g}, "
          f"mean loss {want.mean().item():.4f}")
    assert torch.isfinite(got).all()
    assert not torch.equal(scales, torch.ones_like(scales))
    torch.testing.assert_close(got, want, atol=0.1, rtol=1e-2)
