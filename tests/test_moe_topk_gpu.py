"""--moe-router-topk on the GPU: route tables against the twin, the combine kernels against float64,
the grouped top-2 layer against the fp32 torch path, a captured GPT step, a run without host syncs."""
import functools

import pytest
import torch

from smdt_amd.ops import _ext
from smdt_amd.ops import functional as SF

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def profile_logits(profile, T, E, k):
    g = torch.Generator().manual_seed(T * 64 + E)
    if profile == "ties":                    # a grid of three values, exact in bf16
        return torch.randint(0, 3, (T, E), generator=g).float() * 0.5
    lg = torch.randn(T, E, generator=g)
    if profile == "same_k":                  # every token on experts 1 .. k (0 .. k - 1 when k = E)
        lg[:, (k < E):(k < E) + k] += 20.0
    if profile == "empty":                   # nobody picks the last expert (where k < E)
        lg[:, -1] = -10.0
    return lg


@pytest.mark.parametrize("profile", ["random", "same_k", "empty", "ties"])
@pytest.mark.parametrize("T,E,k", [(T, E, k) for T in (1, 255, 256, 257, 700) for E in (2, 8, 64) for k in (2, 4)
                                   if k <= E])
def test_topk_route_tables_equal_the_twin(T, E, k, profile):
    """Every table bit-equal to the twin's on the same device logits (so the same exp), bf16 and fp32."""
    for dtype in (torch.bfloat16, torch.float32):
        lg = profile_logits(profile, T, E, k).to(DEV, dtype)
        got, want = SF.moe_route(lg, topk=k), SF.moe_route_ref(lg, topk=k)
        assert len(got) == len(want) == 8
        for i, (a, b) in enumerate(zip(got, want)):         # top_p, experts, rows, tokens, tiles, seg, counts, p_of_row
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (i, dtype)


def test_topk_route_writes_every_word_and_top1_is_unchanged():
    """Two calls into buffers pre-filled with 0x7f bytes give moe_route's tables. topk = 1 is the top-1
    entry point as before: integer tables equal to moe_route_ref's, top_p to test_moe_grouped_gpu.py's
    tolerance for that pair (the twin's softmax sums in another order: it was never bitwise equal)."""
    lg = profile_logits("random", 700, 8, 2).to(DEV, torch.bfloat16)
    want = SF.moe_route(lg, topk=2)
    for _ in range(2):
        bufs = [torch.empty_like(t) for t in want]
        for b in bufs:
            b.view(torch.uint8).fill_(0x7F)
        _ext.ext().moe_route_topk_into(lg, 2, *bufs)
        assert all(torch.equal(a, b) for a, b in zip(bufs, want))
    one, ref = SF.moe_route(lg), SF.moe_route_ref(lg)
    assert len(one) == 7 and all(torch.equal(a, b) for a, b in zip(one, SF.moe_route(lg, topk=1)))
    assert all(a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(one[1:], ref[1:]))
    torch.testing.assert_close(one[0], ref[0], rtol=1e-5, atol=0)


@functools.lru_cache(maxsize=None)
def _combine_case(h, T, k, dtype):
    """(route of T tokens over 8 experts, y [R, h], dout [T, h]) on the device; never modified.
    Magnitudes of 0.5 and more with one random sign per column: the k terms of a combine share a
    sign and a gate weight is at least ~1e-3, so every 16-bit result lies in fp16's normal range
    (above 2^-14), where rounding is relative and the bounds apply (a subnormal result rounds with
    up to 2^-25 absolute error whatever the kernel does). gate_grad's dot products still cancel."""
    g = torch.Generator(device=DEV).manual_seed(h + T + k)
    route = SF.moe_route(torch.randn(T, 8, device=DEV, generator=g), topk=k)

    def draw(n):
        sign = torch.randint(0, 2, (1, h), device=DEV, generator=g) * 2.0 - 1.0
        return ((torch.randn(n, h, device=DEV, generator=g).abs() + 0.5) * sign).to(dtype)
    return route, draw(route[3].numel()), draw(T)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("k", [2, 8])
@pytest.mark.parametrize("T", [1, 257])
@pytest.mark.parametrize("h", [8, 264, 1024])
def test_combine_kernels_against_float64(h, T, k, dtype):
    """Each kernel twice (bitwise equal) and against float64 from the same 16-bit inputs: moe_combine
    (gate and unit weights) |err| <= eps |ref| + k 2^-22 sum_j |w_j y_j| (fp32 sum of k terms, one
    rounding); moe_scatter_scaled |err| <= eps |ref|, pad rows exactly zero; moe_gate_grad |err| <=
    h 2^-24 sum_i |dout_i y_i| (exact products, fp32 sum of h terms)."""
    route, y, dout = _combine_case(h, T, k, dtype)
    top_p, row, tok, p_row = route[0], route[2], route[3], route[7]
    rows = y.double()[row.long()]                                    # [T, k, h]
    for w in (top_p, None):
        terms = rows * (w.double().unsqueeze(-1) if w is not None else 1.0)
        got = SF.moe_combine(y, row, w)
        assert got.dtype == dtype and torch.equal(got, SF.moe_combine(y, row, w))
        bound = EPS[dtype] * terms.sum(1).abs() + k * 2.0 ** -22 * terms.abs().sum(1)
        assert bool(((got.double() - terms.sum(1)).abs() <= bound).all()), w is None
    ref = dout.double()[tok.clamp_min(0)] * p_row.double().unsqueeze(-1) * (tok >= 0).unsqueeze(-1)
    got = SF.moe_scatter_scaled(dout, tok, p_row)
    assert got.dtype == dtype and torch.equal(got, SF.moe_scatter_scaled(dout, tok, p_row))
    assert int((tok < 0).sum()) > 0 and bool((got[tok < 0] == 0).all())
    assert bool(((got.double() - ref).abs() <= EPS[dtype] * ref.abs()).all())
    terms = rows * dout.double().unsqueeze(1)
    got = SF.moe_gate_grad(dout, y, row)
    assert got.dtype == torch.float32 and got.shape == (T, k) and torch.equal(got, SF.moe_gate_grad(dout, y, row))
    assert bool(((got.double() - terms.sum(-1)).abs() <= h * 2.0 ** -24 * terms.abs().sum(-1)).all())


H, FFN, E, SEQ, B = 256, 512, 4, 100, 3          # T = 300 tokens


def _layer(k, dtype, grouped, device=None):
    from smdt_amd.models.transformer import SwitchMLP, TransformerConfig
    from smdt_amd.parallel import state as ps
    ps.destroy_model_parallel()
    return SwitchMLP(TransformerConfig(num_layers=2, hidden_size=H, ffn_hidden_size=FFN, num_attention_heads=4,
                                       max_position_embeddings=256, padded_vocab_size=1024, hidden_dropout=0.0,
                                       attention_dropout=0.0, seed=3, num_experts=E, moe_router_topk=k,
                                       params_dtype=dtype, moe_grouped_gemm=grouped), 1, device=device)


def _layer_errors(k, monkeypatch):
    """name -> relative norm error of the grouped bf16 top-k layer against fp32 on the CPU: k = 1 the
    grouped twin (the parent's comparison), k >= 2 the non-grouped torch path. The fp32 run takes the
    expert choice from the device run, so both compute the same function (as test_moe_grouped_gpu.py)."""
    from smdt_amd.parallel import tensor_parallel as tp
    new = _layer(k, torch.bfloat16, True, DEV)
    with torch.no_grad():
        new.router.mul_(20)
    twin = _layer(k, torch.float32, k == 1)
    twin.load_state_dict({n: v.float().cpu() for n, v in new.state_dict().items()})
    for p in new.parameters():
        p.main_grad = torch.zeros_like(p, dtype=torch.float32)
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randn(SEQ, B, H, device=DEV, generator=g).to(torch.bfloat16)
    wgt = torch.randn(SEQ, B, H, device=DEV, generator=g)
    routes, real = [], SF.moe_route
    monkeypatch.setattr(SF, "moe_route", lambda lg, **kk: routes.append(real(lg, **kk)) or routes[-1])
    xn = x.clone().requires_grad_(True)
    out = new(xn)[0]
    (out.float() * wgt).sum().backward()
    tp.flush_deferred_wgrad()
    assert int(new.last_counts.sum()) == SEQ * B * k and int(new.last_counts.min()) > 0
    if k == 1:
        monkeypatch.setattr(SF, "moe_route", lambda lg: tuple(t.cpu() for t in routes[0]))
    else:
        top_e = routes[0][1].long().cpu()
        twin.route = lambda flat: (torch.softmax((flat @ twin.router.t() + twin.router_bias).gather(1, top_e), -1),
                                   top_e)
    xt = x.float().cpu().requires_grad_(True)
    ref = twin(xt)[0]
    (ref * wgt.cpu()).sum().backward()
    monkeypatch.setattr(SF, "moe_route", real)
    pairs = [("output", out.detach().float().cpu(), ref.detach()), ("input", xn.grad.float().cpu(), xt.grad)]
    for (n, pn), pt in zip(new.named_parameters(), twin.parameters()):
        pairs.append((n, pn.main_grad.cpu() if "experts." in n else pn.grad.float().cpu(), pt.grad))
    return {n: ((a - b).norm() / b.norm().clamp_min(1e-12)).item() for n, a, b in pairs}


def test_grouped_top2_layer_matches_the_fp32_torch_path(monkeypatch):
    """Output, dx, the router's gradient and every expert's main_grad: at most twice the error the
    k = 1 grouped layer has against its own fp32 twin at these shapes (k = 2 sums two such
    outputs). Measured on MI355X: profiles/moe_topk/README.md."""
    e1, e2 = _layer_errors(1, monkeypatch), _layer_errors(2, monkeypatch)
    print("\n".join(f"{n}: k = 1 {e1[n]:.3e}   k = 2 {e2[n]:.3e}" for n in e1))
    assert all(e2[n] <= 2 * e1[n] for n in e1), (e1, e2)


def test_grouped_top2_layer_runs_without_a_host_sync():
    from smdt_amd.parallel import tensor_parallel as tp
    new = _layer(2, torch.bfloat16, True, DEV)
    for p in new.parameters():
        p.main_grad = torch.zeros_like(p, dtype=torch.float32)
    x = torch.randn(SEQ, B, H, device=DEV).to(torch.bfloat16)
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
    assert torch.isfinite(xn.grad.float()).all() and torch.isfinite(new.router.grad.float()).all()


def test_captured_top2_gpt_step_equals_eager(monkeypatch):
    """test_captured_moe_gpt_step_equals_eager's run (a 2-layer GPT, 4 experts, one eager warm-up
    step, then two replays, against eager steps) with top-2 routing in its config; same criterion."""
    from smdt_amd.models import transformer
    from test_moe_grouped_gpu import _gpt_run
    monkeypatch.setattr(transformer, "TransformerConfig",
                        functools.partial(transformer.TransformerConfig, moe_router_topk=2))
    le, ge, ce, _ = _gpt_run(False)
    lg, gg, cg, note = _gpt_run(True)
    assert note == "captured", note
    assert cg == ce and cg[1] != cg[2] and all(sum(c) == 1024 for c in cg[1])
    for a, b in zip(le, lg):
        assert abs(a - b) <= 1e-5 * max(1.0, abs(a)), (le, lg)
    for a, b in zip(ge, gg):
        torch.testing.assert_close(b, a, rtol=1e-5, atol=1e-6)
