"""--moe-grouped-gemm on the GPU: the device router against its twin, the grouped GEMM and the
ranged weight gradient bit-exact against the existing single-expert entry points, the Switch
layer against the per-expert loop and an fp32 twin run, and a captured GPT step."""
import functools

import pytest
import torch

from smdt_amd.ops import _ext
from smdt_amd.ops import functional as SF
from test_moe_grouped import logits_for, route_cases

pytestmark = pytest.mark.gpu
DEV = "cuda"
CASES = ["random", "all_to_one", "exactly_256", "one_with_257", "one_with_1", "one_with_0"]
NAMES = ("top_p", "expert_of_token", "row_of_token", "token_of_row", "tile_expert", "seg", "counts")
T, E, H, F = 512, 4, 256, 512
R = 1536


@functools.lru_cache(maxsize=None)
def _route(case):
    """(logits on the device, the twin's tables from the same logits on the CPU); never modified."""
    lg = logits_for(route_cases(T, E)[case], E)
    return lg.to(DEV), SF.moe_route(lg)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", CASES)
def test_moe_route_tables_equal_the_twin(case, dtype):
    lg, want = _route(case)
    lg = lg.to(dtype)
    want = SF.moe_route(lg.cpu()) if dtype != torch.float32 else want
    got = SF.moe_route(lg)
    for n, g, w in zip(NAMES[1:], got[1:], want[1:]):
        assert g.dtype == w.dtype and torch.equal(g.cpu(), w), n
    # (E + a few) x 2^-24 for E <= 64
    torch.testing.assert_close(got[0].cpu(), torch.softmax(lg.float().cpu(), -1).max(-1).values, rtol=1e-5, atol=0)


def test_moe_route_writes_every_word():
    """Two calls into buffers pre-filled with 0x7f bytes give the twin's tables both times."""
    C = _ext.ext()
    lg, want = _route("one_with_1")
    i32 = dict(dtype=torch.int32, device=DEV)
    for _ in range(2):
        bufs = [torch.empty(T, dtype=torch.float32, device=DEV), torch.empty(T, **i32), torch.empty(T, **i32),
                torch.empty(R, dtype=torch.int64, device=DEV), torch.empty(R // 256, **i32), torch.empty(E, 2, **i32),
                torch.empty(E, **i32)]
        for b in bufs:
            b.view(torch.uint8).fill_(0x7F)
        C.moe_route_into(lg, *bufs)
        for n, g, w in zip(NAMES[1:], bufs[1:], want[1:]):
            assert torch.equal(g.cpu(), w), n
        torch.testing.assert_close(bufs[0].cpu(), want[0], rtol=1e-5, atol=0)


@functools.lru_cache(maxsize=None)
def _gemm_inputs(dtype):
    g = torch.Generator(device=DEV).manual_seed(5)
    a = torch.randn(R, H, device=DEV, dtype=dtype, generator=g)
    ws = [torch.randn(F, H, device=DEV, dtype=dtype, generator=g) * 0.05 for _ in range(E)]
    bs = [torch.randn(F, device=DEV, dtype=dtype, generator=g) for _ in range(E)]
    aux = torch.randn(R, F, device=DEV, dtype=dtype, generator=g) * 2
    return a, ws, bs, aux


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("epi", [0, 1, 2, 3])
def test_grouped_gemm_tiles_bit_equal_gemm_tn(epi, dtype):
    """Every used 256-row tile equals gemm_tn on those rows with that expert's weight and bias: a
    tile's K order does not depend on where the tile lies. The second output too, and the column
    sums of the SUMS form."""
    C = _ext.ext()
    a, ws, bs, aux = _gemm_inputs(dtype)
    te = _route("random")[1][4]
    assert sorted(set(te.tolist())) == [-1, 0, 1, 2, 3]
    ted = te.to(DEV)
    outs = SF.gemm_tn_grouped(a, ws, ted, epi, bs if epi else None, aux if epi == 3 else None)
    part = SF.gemm_tn_grouped(a, ws, ted, 3, bs, aux, sums=True) if epi == 3 else None
    for i, e in enumerate(te.tolist()):
        if e < 0:
            continue
        r = slice(256 * i, 256 * i + 256)
        ref = C.gemm_tn(a[r], ws[e], epi, bs[e] if epi else None, None, None, 0, 0, aux[r].contiguous() if epi == 3 else None)
        assert len(ref) == len(outs)
        for o, w in zip(outs, ref):
            assert torch.equal(o[r], w), (i, e)
        if part is not None:
            db = torch.zeros(F, device=DEV)
            dz = C.gemm_tn_dgelu_dbias(a[r], ws[e], bs[e], aux[r].contiguous(), db, False)
            assert torch.equal(part[0][r], dz) and torch.equal(part[1][2 * i] + part[1][2 * i + 1], db), (i, e)


@pytest.mark.parametrize("case", ["random", "one_with_0"])
@pytest.mark.parametrize("mode", ["plain", "bias", "overwrite"])
def test_ranged_wgrad_bit_equal_single_expert_wgrad(mode, case):
    """Each expert's main_grad (accumulated into a non-zero buffer) equals wgrad_mfma(max_splits=1)
    on its segment slice; an expert with no rows leaves it bit-unchanged (zeros with overwrite);
    the bias tiles' column sums are within fp32 summation error of the segment's column sums."""
    C = _ext.ext()
    seg = _route(case)[1][5]
    segd = seg.to(DEV)
    g = torch.Generator(device=DEV).manual_seed(9)
    dy = torch.randn(R, F, device=DEV, dtype=torch.bfloat16, generator=g)
    x = torch.randn(R, H, device=DEV, dtype=torch.bfloat16, generator=g)
    mg0 = torch.randn(F, H, device=DEV, generator=g)
    mgs = [mg0.clone() for _ in range(E)]
    bgs = [torch.ones(F, device=DEV) for _ in range(E)]
    none = torch.empty(0, device=DEV)
    assert C.wgrad_grouped(mgs, [dy] * E, [x] * E, bgs if mode == "bias" else [none] * E, [mode == "overwrite"] * E, 0,
                           [segd] * E, list(range(E)))
    for e, (s, r) in enumerate(seg.tolist()):
        ref = torch.zeros_like(mg0) if mode == "overwrite" else mg0.clone()
        if r:
            assert C.wgrad_mfma(ref, dy[s:s + r], x[s:s + r], 1)
        assert torch.equal(mgs[e], ref), (e, s, r)
        if mode == "bias":
            want = dy[s:s + r].double().sum(0)
            err = (bgs[e].double() - 1.0 - want).abs()
            assert bool((err <= (r + 2) * 2.0 ** -24 * (dy[s:s + r].double().abs().sum(0) + 1.0)).all()), e
    if case == "one_with_0":
        assert seg[0].tolist() == [0, 0]


def _layers(dtype=torch.bfloat16):
    from smdt_amd.models.transformer import SwitchMLP, TransformerConfig
    from smdt_amd.parallel import state as ps
    ps.destroy_model_parallel()
    kw = dict(num_layers=2, hidden_size=H, ffn_hidden_size=F, num_attention_heads=4, max_position_embeddings=256,
              padded_vocab_size=1024, hidden_dropout=0.0, attention_dropout=0.0, seed=3, num_experts=E)
    old = SwitchMLP(TransformerConfig(**kw, params_dtype=dtype), 1, device=DEV)
    with torch.no_grad():
        old.router.mul_(20)
    new = SwitchMLP(TransformerConfig(**kw, params_dtype=dtype, moe_grouped_gemm=True), 1, device=DEV)
    new.load_state_dict(old.state_dict())
    twin = SwitchMLP(TransformerConfig(**kw, params_dtype=torch.float32, moe_grouped_gemm=True), 1)
    twin.load_state_dict({k: v.float().cpu() for k, v in old.state_dict().items()})
    for p in new.parameters():
        p.main_grad = torch.zeros_like(p, dtype=torch.float32)
    x = torch.randn(128, 4, H, device=DEV, generator=torch.Generator(device=DEV).manual_seed(0)).to(dtype)
    return old, new, twin, x


def test_switch_layer_grouped_matches_existing_path_and_fp32_twin(monkeypatch):
    """(The fp32 twin takes the discrete routing decision from the device run: its own fp32 logits
    can put a token whose top two bf16 logits nearly tie on the other expert, which would compare
    two different functions. Everything else in the twin is fp32.)"""
    from smdt_amd.parallel import tensor_parallel as tp
    old, new, twin, x = _layers()
    with torch.no_grad():
        want = old(x)[0]
    assert len(set(old.route(x.reshape(-1, H))[1].tolist())) == E
    xn = x.clone().requires_grad_(True)
    routes, real = [], SF.moe_route
    monkeypatch.setattr(SF, "moe_route", lambda lg: routes.append(real(lg)) or routes[-1])
    out = new(xn)[0]
    monkeypatch.setattr(SF, "moe_route", lambda lg: tuple(t.cpu() for t in routes[0]))
    # the existing layer test's own tolerance (test_switch_mlp_on_kernels_matches_per_expert_composition)
    torch.testing.assert_close(out.float(), want.float(), atol=2e-2, rtol=2e-2)
    # random loss weights: with a ramp over the tokens every column of a bias gradient is the same
    # signed sum over an expert's tokens, which cancels (expert 3: 4.3e-2 of a near-zero norm from
    # the bf16 rounding of dOut alone) and measures the conditioning of the sum, not the kernels
    wgt = torch.randn(out.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    (out.float() * wgt).sum().backward()
    tp.flush_deferred_wgrad()
    xt = x.float().cpu().requires_grad_(True)
    (twin(xt)[0] * wgt.cpu()).sum().backward()
    assert new.last_counts.tolist() == twin.last_counts.tolist() and min(new.last_counts.tolist()) > 0
    # 3e-2 relative norm error per tensor: tests/test_gemm_tn_epilogue_gpu.py:175 (the bound
    # test_gpt_step_matches_fp32_reference allows each parameter)
    pairs = [("input", xn.grad.float().cpu(), xt.grad)]
    for (n, pn), pt in zip(new.named_parameters(), twin.parameters()):
        got = pn.main_grad.cpu() if "experts." in n else pn.grad.float().cpu()
        pairs.append((n, got, pt.grad))
    for n, got, ref in pairs:
        err = ((got - ref).norm() / ref.norm().clamp_min(1e-12)).item()
        print(f"{n}: grouped vs fp32 twin {err:.3e}")
        assert err < 3e-2, (n, err)


def test_switch_layer_grouped_runs_without_a_host_sync():
    from smdt_amd.parallel import tensor_parallel as tp
    _, new, _, x = _layers()
    for i in range(2):        # the first call builds the pointer tables
        if i == 1:
            torch.cuda.set_sync_debug_mode("error")
        try:
            xn = x.clone().requires_grad_(True)
            new(xn)[0].float().sum().backward()
            tp.flush_deferred_wgrad()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.isfinite(xn.grad.float()).all()


def _gpt_run(graph):
    from smdt_amd.models.gpt import GPTModel
    from smdt_amd.models.transformer import TransformerConfig
    from smdt_amd.optim.optimizer import MixedPrecisionAdam
    from smdt_amd.parallel import state as ps
    from smdt_amd.parallel.distributed import DistributedDataParallel as DDP
    from smdt_amd.train.graphs import CapturedStep
    ps.destroy_model_parallel()
    cfg = TransformerConfig(num_layers=2, hidden_size=H, num_attention_heads=4, padded_vocab_size=1024,
                            max_position_embeddings=256, hidden_dropout=0.0, attention_dropout=0.0,
                            params_dtype=torch.bfloat16, seed=5, num_experts=E, moe_grouped_gemm=True)
    model = GPTModel(cfg, device=DEV)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("mlp.router"):
                p.mul_(20)
    ddp = DDP(model, grad_dtype=torch.float32)
    opt = MixedPrecisionAdam(ddp, lr=1e-3, weight_decay=0.01, clip_grad=1.0, capturable=True)
    g = torch.Generator(device=DEV).manual_seed(11)
    toks = [torch.randint(0, 1000, (2, 257), device=DEV, generator=g) for _ in range(3)]
    mlps = [m for m in model.modules() if type(m).__name__ == "SwitchMLP"]

    def step(t):
        ddp.zero_grad_buffer()
        loss = model(t[:, :-1], labels=t[:, 1:]).float().mean()
        loss.backward()
        ddp.finish_grad_sync()
        opt.step()
        return loss.detach()

    run = CapturedStep(step, warmup=1, enabled=graph)
    losses, grads, counts = [], [], []
    for t in toks:
        losses.append(float(run(t)))
        grads.append(ddp.grad_data[::997].clone().cpu())
        counts.append([m.last_counts.tolist() for m in mlps])
    torch.cuda.synchronize()
    ps.destroy_model_parallel()
    return losses, grads, counts, run.note


def test_captured_moe_gpt_step_equals_eager():
    """A 2-layer GPT with 4 experts and the flag under CapturedStep (one eager warm-up step, then the
    capture replayed on two different batches) against the same steps run eagerly: the routing
    differs between the replays, and losses and a sample of main_grad agree to the summation-order
    criterion of test_captured_emulated_dp8_step_equals_eager."""
    le, ge, ce, _ = _gpt_run(False)
    lg, gg, cg, note = _gpt_run(True)
    assert note == "captured", note
    assert cg == ce and cg[1] != cg[2] and all(sum(c) == 512 for c in cg[1])
    for a, b in zip(le, lg):
        assert abs(a - b) <= 1e-5 * max(1.0, abs(a)), (le, lg)
    for a, b in zip(ge, gg):
        torch.testing.assert_close(b, a, rtol=1e-5, atol=1e-6)
