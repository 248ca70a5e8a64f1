"""The GeLU epilogues of the hand-written TN GEMM (csrc/kernels/gemm_tn.hip: EPI_BIAS_GELU in the
fc1 forward, EPI_DGELU in the fc2 dgrad) with the sigmoid-form GeLU / GeLU' on packed fp32
(csrc/kernels/activations.h), at the smallest shapes on which each path of the kernel can go
wrong:

    256 x 256 x 128, every CU    one tile, 2 K-stages of 64: only the peeled stage pair runs
    512 x 512 x 256, 1 block     four tiles on one persistent workgroup: every tile boundary
    768 x 512 x 384, 3 blocks    six tiles on three workgroups, an odd number of stage pairs

in bf16 and fp16, with the criteria of test_gemm_tn_gpu.py: against the fp32 reference and against
the unfused twin (bias_act_fwd / bias_act_bwd, which share activations.h). The tails check that
the sigmoid form saturates without inf * 0: pre + bias at +-8 and exactly 0 (and at +-30, where
2^t overflows to inf)."""
import functools

import pytest
import torch

from smdt_amd.ops import _ext

pytestmark = pytest.mark.gpu
DEV = "cuda"

CASES = [(256, 256, 128, 0), (512, 512, 256, 1), (768, 512, 384, 3)]
DTYPES = [torch.bfloat16, torch.float16]
TAILS = (8.0, -8.0, 0.0, 30.0, -30.0)   # pre + bias of row 0, columns 0..4, in the tail calls


def _rel(got, ref):
    return ((got.float() - ref).abs().max() / ref.abs().max().clamp_min(1e-6)).item()


def _gelu(z):
    return torch.nn.functional.gelu(z, approximate="tanh")


def _gelu_grad(z):
    z = z.detach().clone().requires_grad_()
    _gelu(z).backward(torch.ones_like(z))
    return z.grad


@functools.lru_cache(maxsize=None)
def _inputs(M, N, K, dtype):
    """Operands and the fp32 product, made once per (shape, dtype) and never modified."""
    g = torch.Generator(device=DEV).manual_seed(M + 3 * N + 7 * K)
    a = torch.randn(M, K, device=DEV, dtype=dtype, generator=g)
    b = torch.randn(N, K, device=DEV, dtype=dtype, generator=g) * 0.05
    bias = torch.randn(N, device=DEV, dtype=dtype, generator=g)
    pre = torch.randn(M, N, device=DEV, dtype=dtype, generator=g) * 2
    prod = a.float() @ b.float().t()
    return a, b, bias, pre, prod


@pytest.mark.parametrize("M,N,K,blocks", CASES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_bias_gelu_epilogue(M, N, K, blocks, dtype):
    C = _ext.ext()
    a, b, bias, _, prod = _inputs(M, N, K, dtype)
    pre, act = C.gemm_tn(a, b, 2, bias, None, None, blocks)
    assert torch.isfinite(pre).all() and torch.isfinite(act).all()
    assert _rel(pre, prod) < 1e-2
    ref_act = _gelu(prod + bias.float())
    scale = ref_act.abs().max().item()
    e_ref = (act.float() - ref_act).abs().max().item()
    unf = C.bias_act_fwd(pre, bias, 0)
    e_unf = (act.float() - unf.float()).abs().max().item()
    print(f"bias_gelu {M}x{N}x{K} {dtype}: vs fp32 {e_ref / scale:.3e}, vs unfused {e_unf / scale:.3e} (of max |ref|)")
    assert e_ref < 3e-2 * scale
    assert e_unf <= 1e-2 * scale


@pytest.mark.parametrize("M,N,K,blocks", CASES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gelu_backward_epilogue(M, N, K, blocks, dtype):
    C = _ext.ext()
    a, b, bias, pre, prod = _inputs(M, N, K, dtype)
    got = C.gemm_tn(a, b, 3, bias, None, None, blocks, 0, pre)[0]
    assert torch.isfinite(got).all()
    ref = prod * _gelu_grad(pre.float() + bias.float())
    e_ref = _rel(got, ref)
    unf = C.bias_act_bwd(prod.to(dtype), pre, bias, 0, False, None)[0]
    e_unf = (got.float() - unf.float()).abs().max().item() / ref.abs().max().item()
    print(f"dgelu {M}x{N}x{K} {dtype}: vs fp32 {e_ref:.3e}, vs unfused {e_unf:.3e} (of max |ref|)")
    assert e_ref < 2e-2
    assert e_unf <= 1e-2


@pytest.mark.parametrize("dtype", DTYPES)
def test_epilogue_tails_saturate(dtype):
    """pre + bias at +-8, 0 and +-30 in row 0 (a zero row of a, so the product there is exactly 0
    and the forward's pre + bias is the bias; the backward is given pre = 0 there and, so that its
    product is not 0, the original a): gelu -> z, -0, 0, z, -0 and gelu' -> 1, 0, 0.5, 1, 0, all
    finite. The error allowed is the rounding of the 16-bit output (2^-8 relative, bf16) plus
    1e-6 for the values that are 0 up to the tanh form's own ~1e-7."""
    C = _ext.ext()
    M, N, K, blocks = CASES[1]
    a, b, bias, pre, prod = _inputs(M, N, K, dtype)
    nt = len(TAILS)
    tails = torch.tensor(TAILS, device=DEV)
    bias_t = bias.clone()
    bias_t[:nt] = tails.to(dtype)
    a0 = a.clone()
    a0[0] = 0
    pre_o, act = C.gemm_tn(a0, b, 2, bias_t, None, None, blocks)
    assert torch.isfinite(pre_o).all() and torch.isfinite(act).all()
    assert pre_o[0].abs().max().item() == 0
    want = _gelu(tails)
    err = (act[0, :nt].float() - want).abs()
    assert (err <= 2.0 ** -8 * want.abs() + 1e-6).all(), (act[0, :nt], want)
    unf = C.bias_act_fwd(pre_o, bias_t, 0)
    assert torch.isfinite(unf).all()
    assert (act.float() - unf.float()).abs().max().item() <= 1e-2 * _gelu(prod + bias_t.float()).abs().max().item()

    pre_t = pre.clone()
    pre_t[0, :nt] = 0
    dz = C.gemm_tn(a, b, 3, bias_t, None, None, blocks, 0, pre_t)[0]
    assert torch.isfinite(dz).all()
    want = prod[0, :nt] * _gelu_grad(tails)
    err = (dz[0, :nt].float() - want).abs()
    # the product is rounded to 16 bits before the derivative multiplies it, then the result is
    assert (err <= 2 * 2.0 ** -8 * want.abs() + 1e-6).all(), (dz[0, :nt], want)
    unf = C.bias_act_bwd(prod.to(dtype), pre_t, bias_t, 0, False, None)[0]
    assert torch.isfinite(unf).all()
    ref = prod * _gelu_grad(pre_t.float() + bias_t.float())
    assert (dz.float() - unf.float()).abs().max().item() <= 1e-2 * ref.abs().max().item()


def _gpt_fc1_grads(fused, monkeypatch):
    from smdt_amd.models.gpt import GPTModel
    from smdt_amd.models.transformer import TransformerConfig
    from smdt_amd.parallel import state as ps
    from smdt_amd.parallel import tensor_parallel as tp
    from smdt_amd.parallel.distributed import DistributedDataParallel
    monkeypatch.setattr(tp, "_FUSED_BIAS_GELU", fused)
    monkeypatch.setattr(tp, "_fills_chip", lambda rows, n: True)   # test shapes: a few tiles only
    calls = {"n": 0}
    orig = tp.FusedGeLUMLP.forward

    def counted(ctx, *args):
        calls["n"] += 1
        return orig(ctx, *args)
    monkeypatch.setattr(tp.FusedGeLUMLP, "forward", staticmethod(counted))
    ps.destroy_model_parallel()
    cfg = TransformerConfig(num_layers=2, hidden_size=256, num_attention_heads=4, max_position_embeddings=128,
                            padded_vocab_size=1024, hidden_dropout=0.0, attention_dropout=0.0, seed=5,
                            params_dtype=torch.bfloat16)
    model = GPTModel(cfg, device="cuda")
    ddp = DistributedDataParallel(model)
    g = torch.Generator().manual_seed(6)
    toks = torch.randint(0, 1000, (2, 129), generator=g).cuda()
    ddp.zero_grad_buffer()
    loss = model(toks[:, :-1], labels=toks[:, 1:]).float().mean()
    loss.backward()
    ddp.finish_grad_sync()
    torch.cuda.synchronize()
    grads = {n: p.main_grad.float().clone() for n, p in model.named_parameters() if ".fc1." in n}
    return loss.item(), grads, calls["n"]


def test_gpt_fused_mlp_fc1_grads_match_unfused(monkeypatch):
    """A 2-layer GPT (h 256, 4 heads, 128 x 2 tokens) forward + backward through FusedGeLUMLP
    against the same model with the fused path off (the library GEMMs and the bias_act passes):
    fc1's weight and bias gradients, to the 3e-2 relative norm error that
    test_gpt_step_matches_fp32_reference allows each parameter."""
    lf, gf, nf = _gpt_fc1_grads(True, monkeypatch)
    lu, gu, nu = _gpt_fc1_grads(False, monkeypatch)
    assert nf == 2 and nu == 0
    assert sorted(gf) == sorted(gu) and len(gf) == 4   # weight + bias of both layers
    assert abs(lf - lu) <= 1e-2 * abs(lu) + 3e-2
    for n in gf:
        assert torch.isfinite(gf[n]).all()
        err = ((gf[n] - gu[n]).norm() / gu[n].norm().clamp_min(1e-12)).item()
        print(f"{n}: fused vs unfused {err:.3e}")
        assert err < 3e-2, (n, err)
