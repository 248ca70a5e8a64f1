"""--fp8-recipe mxfp8, CPU side: the torch twin of the block quantiser against a per-block Python
loop, the GEMM twin against a float64 loop, ``tp.MXFP8Linear`` against an independent reference,
the point of the recipe (rows of very different magnitude) against the per-tensor twin, the flag's
validation, and a two-iteration pretrain_gpt.py run whose checkpoint reloads."""
import math
import os
import subprocess
import sys

import pytest
import torch

from _numerics import assert_rows_close

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["--num-layers", "2", "--hidden-size", "128", "--num-attention-heads", "2", "--seq-length", "64",
        "--max-position-embeddings", "64", "--micro-batch-size", "2"]
DEFAULTS = {"tokenizer_type": "GPT2BPETokenizer"}
ULP = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}
FMAX = {"e4m3": 448.0, "e5m2": 57344.0}
EMAX = {"e4m3": 8, "e5m2": 15}
FDT = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _loop_quantize(x, fmt):
    """The definition, block by block in Python: (q bytes [M, K], s [M, K / 32])."""
    M, K = x.shape
    q = torch.empty(M, K, dtype=torch.uint8)
    s = torch.empty(M, K // 32, dtype=torch.uint8)
    for m in range(M):
        for kb in range(K // 32):
            blk = x[m, 32 * kb:32 * kb + 32].float()
            fin = [abs(v) for v in blk.tolist() if math.isfinite(v)]
            a = max(fin) if fin else 0.0
            e = 0 if a == 0 else min(max(math.floor(math.log2(a)) - EMAX[fmt], -127), 127)
            s[m, kb] = e + 127
            scaled = (blk.double() * 2.0 ** -e).clamp(-FMAX[fmt], FMAX[fmt])     # exact in float64; clamp keeps NaN
            q[m, 32 * kb:32 * kb + 32] = _bits(scaled.float().to(FDT[fmt]))
    return q, s


def _special_input(dtype):
    """[12, 96]: one block per case (see the names), the rest log-normal."""
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(12, 96, generator=g) * torch.exp(2.0 * torch.randn(12, 96, generator=g))).to(dtype)
    x[0, :32] = 0                                                   # an all-zero block
    x[1, :32] = torch.linspace(-1, 1, 32).to(dtype); x[1, 7] = 4.0  # amax an exact power of two
    x[2, :32] = 0.25; x[2, 5] = 1.9375                              # scales into (464, 512): saturates to 448 (E4M3)
    x[3, :32] = 2.0 ** 10 * torch.linspace(0.5, 1, 32)              # neighbouring blocks 2^20 apart
    x[3, 32:64] = 2.0 ** -10 * torch.linspace(0.5, 1, 32)
    if dtype == torch.bfloat16:
        x[4, :32] = 0; x[4, 3] = 1e-40; x[4, 4] = -3e-39            # bf16 subnormals: e clamps at -127
        x[4, 32:64] = 2.0 ** -120 * torch.linspace(0.5, 1, 32)      # e = -127 - ... just above the clamp
        x[5, :32] = 3.0e38 * torch.linspace(-1, 1, 32)              # the largest exponents
    else:
        x[4, :32] = 0; x[4, 3] = 6e-8; x[4, 4] = -3e-7; x[4, 9] = 5e-6   # fp16 subnormals
        x[5, :32] = 60000.0 * torch.linspace(-1, 1, 32)
    x[6, 4], x[6, 40], x[6, 70] = float("nan"), float("inf"), float("-inf")
    x[7, :32] = float("inf"); x[7, 32:64] = float("nan")            # blocks without a finite value
    return x


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_mx_quantize_twin_matches_block_loop(fmt, dtype):
    from smdt_amd.ops import functional as SF
    x = _special_input(dtype)
    q, s = SF.mx_quantize(x, fmt)                     # CPU tensors take the twin
    ql, sl = _loop_quantize(x, fmt)
    assert q.dtype == FDT[fmt] and s.dtype == torch.uint8 and s.shape == (12, 3)
    assert torch.equal(s, sl), (s, sl)
    assert torch.equal(_bits(q), ql)
    assert (s != 255).all()
    # the named cases
    assert s[0, 0] == 127 and (q[0, :32].float() == 0).all()
    assert s[1, 0] == 127 + 2 - EMAX[fmt]
    if fmt == "e4m3":
        assert s[2, 0] == 127 - 8 and q[2, 5].float() == 448.0 and q[2, 0].float() == 64.0
    assert int(s[3, 0]) - int(s[3, 1]) == 20
    if dtype == torch.bfloat16:
        assert s[4, 0] == 0                           # e = -127, the lower clamp
        assert s[5, 0] == 127 + 127 - EMAX[fmt]       # floor(log2 3e38) = 127: the clamp at +127 is never binding
    assert torch.isnan(q[6, 4].float()) and q[6, 40].float() == FMAX[fmt] and q[6, 70].float() == -FMAX[fmt]
    assert s[7, 0] == 127 and s[7, 1] == 127 and (q[7, :32].float() == FMAX[fmt]).all()
    # column form: the quantisation of the transpose, not the transposed bytes
    xc = _special_input(dtype)[:, :64].t().contiguous().repeat(1, 4)[:, :16].contiguous()      # [64, 16]
    qt, st = SF.mx_quantize(xc, fmt, columnwise=True)
    ql, sl = _loop_quantize(xc.t().contiguous(), fmt)
    assert qt.shape == (16, 64) and st.shape == (16, 2)
    assert torch.equal(st, sl) and torch.equal(_bits(qt), ql)
    w = _special_input(dtype)[:, :64].repeat(3, 1)[:32].contiguous()                           # [32, 64]
    both = SF.mx_quantize_weight(w, fmt)
    rows, cols = SF.mx_quantize(w, fmt), SF.mx_quantize(w, fmt, columnwise=True)
    for got, want in zip(both, rows + cols):
        assert torch.equal(_bits(got), _bits(want))
    assert not torch.equal(_bits(both[2]), _bits(both[0]).t())
    with pytest.raises(ValueError, match=r"\(12, 48\)"):
        SF.mx_quantize(x[:, :48], fmt)
    with pytest.raises(ValueError, match=r"\(12, 96\)"):
        SF.mx_quantize(x, fmt, columnwise=True)


def test_mx_dequantize_and_gemm_ref_against_float64_loop():
    from smdt_amd.ops import functional as SF
    g = torch.Generator().manual_seed(2)
    M, N, K = 128, 128, 128
    a, sa = SF.mx_quantize((torch.randn(M, K, generator=g) * 30).bfloat16(), "e5m2")
    b, sb = SF.mx_quantize((torch.randn(N, K, generator=g) * 0.02).bfloat16(), "e4m3")
    bias = torch.randn(N, generator=g).bfloat16()
    out = SF.gemm_mx(a, sa, b, sb, bias, torch.bfloat16)
    assert torch.equal(out, SF.gemm_mx_ref(a, sa, b, sb, bias, torch.bfloat16))
    af, bf = a.float().double(), b.float().double()
    for m, n in [(0, 0), (5, 17), (127, 3), (64, 127)]:
        acc = 0.0
        for k in range(K):
            acc += (af[m, k].item() * 2.0 ** (int(sa[m, k // 32]) - 127)) * (bf[n, k].item() * 2.0 ** (int(sb[n, k // 32]) - 127))
        want = acc + bias[n].float().item()
        assert abs(out[m, n].float().item() - want) <= 2.0 ** -8 * abs(want) + 1e-6, (m, n)
    dq = SF.mx_dequantize(a, sa)
    assert dq.dtype == torch.float32 and dq[3, 40].item() == af[3, 40].item() * 2.0 ** (int(sa[3, 1]) - 127)
    with pytest.raises(ValueError, match="120 x 128 x 128"):
        SF.gemm_mx(a[:120], sa[:120], b, sb)
    with pytest.raises(ValueError, match="128 x 128 x 96"):
        SF.gemm_mx(a[:, :96].contiguous(), sa[:, :3].contiguous(), b[:, :96].contiguous(), sb[:, :3].contiguous())
    assert SF.gemm_mx_supported(256, 128, 384) and not SF.gemm_mx_supported(128, 64, 128)


def _indep_dq(t, fmt):
    """Quantise -> dequantise of t [M, K] (blocks along K) written independently of the library:
    frexp for floor(log2), ldexp for the scale, float64 throughout. Finite inputs."""
    M, K = t.shape
    b = t.double().reshape(M, K // 32, 32)
    a = b.abs().amax(-1)
    _, ex = torch.frexp(a)                                   # a = m 2^ex, m in [0.5, 1)
    e = (ex - 1 - EMAX[fmt]).clamp(-127, 127)
    e = torch.where(a == 0, torch.zeros_like(e), e)
    unit = torch.ldexp(torch.ones_like(a), e).unsqueeze(-1)
    q = (b / unit).clamp(-FMAX[fmt], FMAX[fmt]).float().to(FDT[fmt]).double()
    return (q * unit).reshape(M, K)


def _mx_linear(dev, dtype, w0, b0):
    w = torch.nn.Parameter(w0.clone().to(dev))
    w.main_grad = torch.zeros(w0.shape, dtype=torch.float32, device=dev)
    b = torch.nn.Parameter(b0.clone().to(dev)) if b0 is not None else None
    return w, b


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
def test_mxfp8_linear_against_independent_reference(fmt, dtype):
    """128 tokens x 128 -> 384. y and dX within one output ulp (of the row maximum, the criterion
    of tests/test_fp8_gpu.py) of y = dq_row(x) dq_row(W)^T + b and dX = dq_row(dY) dq_col(W)^T with
    the quantise-dequantise written here: a wrong gradient format, the row form of W in the dgrad
    or transposed row-form bytes fail it. main_grad against fp32 dY^T x of the 16-bit operands under
    that file's main_grad criterion (see the note at the assertion for bf16 on the CPU): a wgrad fed
    dequantised operands lands near 1e-2."""
    from smdt_amd.parallel import tensor_parallel as tp
    gfmt = "e5m2" if fmt == "hybrid" else "e4m3"
    assert tp.MXFP8Recipe(fmt).grad_fmt == gfmt
    g = torch.Generator().manual_seed(3)
    w0 = (0.05 * torch.randn(384, 128, generator=g) * torch.exp2(torch.randint(-3, 4, (384, 1), generator=g).float())).to(dtype)
    b0 = (0.1 * torch.randn(384, generator=g)).to(dtype)
    w, b = _mx_linear("cpu", dtype, w0, b0)
    for step in range(2):
        x = (torch.randn(4, 32, 128, generator=g) * (1 + step)).to(dtype)
        dy = (torch.randn(4, 32, 384, generator=g) * (1 + 3 * step)).to(dtype)
        base = w.main_grad.clone()
        y, dx = _mx_step(w, b, x, dy, gfmt)
        assert y.dtype == dtype and dx.dtype == dtype and y.shape == (4, 32, 384) and dx.shape == x.shape
        x2, dy2 = x.reshape(-1, 128), dy.reshape(-1, 384)
        y_ref = _indep_dq(x2, "e4m3") @ _indep_dq(w0, "e4m3").t() + b0.double()
        dx_ref = _indep_dq(dy2, gfmt) @ _indep_dq(w0.t().contiguous(), "e4m3").t()
        assert_rows_close(y.reshape(-1, 384), y_ref.float(), ULP[dtype], f"y step {step}")
        assert_rows_close(dx.reshape(-1, 128), dx_ref.float(), ULP[dtype], f"dX step {step}")
        dw_ref = dy2.float().t() @ x2.float()
        assert dw_ref.abs().mean() > 5.0
        torch.testing.assert_close(w.main_grad, base + dw_ref, atol=0.25, rtol=1e-2)
        # that file's row-relative 1e-3 is for the fp32-accumulating kernel (tests/test_mxfp8_gpu.py
        # asserts it for both dtypes). The CPU weight gradient is a 16-bit matmul added into fp32,
        # one rounding of each entry (tests/test_fp8.py): 2^-11 in fp16, inside 1e-3, and 2^-8 of
        # the row maximum in bf16, which is what is asserted there.
        assert_rows_close(w.main_grad - base, dw_ref, 1e-3 if dtype == torch.float16 else 2.0 ** -8,
                          f"main_grad step {step}")
        torch.testing.assert_close(b.grad.float(), dy2.float().sum(0), atol=1e-2 * (1 + 3 * step), rtol=2.0 ** -7)
        b.grad = None
    with pytest.raises(ValueError, match="120 rows"):
        _mx_step(w, b, torch.zeros(120, 128, dtype=dtype), torch.zeros(120, 384, dtype=dtype), gfmt)


def test_mx_weight_forms_are_cached_per_optimizer_step():
    from smdt_amd.parallel import fp8_linear
    from smdt_amd.parallel import tensor_parallel as tp
    w = torch.nn.Parameter(torch.randn(128, 128).bfloat16())
    a = tp.mx_weight_q(w)
    assert tp.mx_weight_q(w)[0] is a[0]                # one quantise per step
    tp.params_changed()
    b = tp.mx_weight_q(w)
    assert b[0] is not a[0] and torch.equal(_bits(b[0]), _bits(a[0]))
    with torch.no_grad():
        w.mul_(2)                                      # an in-autograd write bumps the version
    assert tp.mx_weight_q(w)[0] is not b[0]
    tp.drop_cached_weight_t([w])
    assert id(w) not in fp8_linear._MX_WQ


def _no_saturation(t):
    """Pull mantissas above 1.75 down to 1.75: no element then scales into the band (448, 512) that
    E4M3's floor-scale saturates, whatever block it ends up leading."""
    m, ex = torch.frexp(t.float())
    return torch.ldexp(m.clamp(-0.875, 0.875), ex)


def test_block_scaling_holds_rows_of_any_magnitude_where_one_scale_per_tensor_does_not():
    """The point of the recipe. x [128, 128] has rows alternating in magnitude between 2^12 and
    2^-12; y = x W^T through ``MXFP8Linear`` (bf16) against the float64 product of the 16-bit
    operands.

    Bound, per output y[m, n]. An E4M3 element of a block with scale unit u = 2^e is stored as
    v / u rounded to 3 mantissa bits: a normal (|v| / u >= 2^-6) is off by at most half an ulp,
    2^-4 |v|; a subnormal by at most half the subnormal spacing, 2^-10 u. The block's leading
    element scales into [256, 512); the inputs keep mantissas <= 1.75, so it stays <= 448 and
    nothing saturates. So |dq(v) - v| <= d(v) = max(2^-4 |v|, 2^-10 u), with u = 2^(floor(log2
    amax_block) - 8) computed here from the data. For the product,
        |sum_k dq(x_k) dq(w_k) - sum_k x_k w_k| <= sum_k d(x_k) |w_k| + |x_k| d(w_k) + d(x_k) d(w_k),
    plus the bf16 output's half ulp 2^-9 |y| and 2^-20 sum_k |x_k w_k| for the fp32 accumulation
    of 128 terms (128 * 2^-24 = 2^-17 of the partial sums' magnitude, rounded up generously).
    Every row of the MX result is inside it. The per-tensor twin (``fp8_quantize_ref`` at the
    tensor's own amax, scale = 448 / amax) flushes the small rows, 2^-24 of the tensor's amax and
    so below half the smallest E4M3 subnormal 2^-10 of 448, to zero: its error there is the whole
    of y, which breaks the bound on every small row."""
    from smdt_amd.ops import functional as SF
    from smdt_amd.parallel import tensor_parallel as tp
    g = torch.Generator().manual_seed(7)
    rows = torch.where(torch.arange(128) % 2 == 0, 2.0 ** 12, 2.0 ** -12).unsqueeze(1)
    x = _no_saturation(torch.randn(128, 128, generator=g) * rows).bfloat16()
    w0 = _no_saturation(0.05 * torch.randn(256, 128, generator=g)).bfloat16()
    small = torch.arange(128) % 2 == 1

    def d(t):
        b = t.double().reshape(t.shape[0], -1, 32)
        _, ex = torch.frexp(b.abs().amax(-1))
        unit = torch.ldexp(torch.ones(ex.shape, dtype=torch.float64), ex - 1 - 8).unsqueeze(-1)
        return torch.maximum(2.0 ** -4 * b.abs(), 2.0 ** -10 * unit).reshape(t.shape)

    xd, wd = x.double(), w0.double()
    y_true = xd @ wd.t()
    mag = xd.abs() @ wd.abs().t()
    bound = d(x) @ wd.abs().t() + xd.abs() @ d(w0).t() + d(x) @ d(w0).t() + 2.0 ** -9 * y_true.abs() + 2.0 ** -20 * mag
    w, _ = _mx_linear("cpu", torch.bfloat16, w0, None)
    y = tp.MXFP8Linear.apply(x, w, None, True, "e5m2").double()
    tp.params_changed()
    excess = ((y - y_true).abs() / bound)
    print(f"mxfp8: max error / bound {excess.max().item():.3f} (small rows {excess[small].max().item():.3f})")
    assert (excess <= 1.0).all()
    # one scale per tensor at the tensors' own amax
    one = torch.ones(1)
    sx, sw = 448.0 / x.float().abs().max(), 448.0 / w0.float().abs().max()
    qx = SF.fp8_quantize_ref(x, sx * one, torch.zeros(1), "e4m3")
    qw = SF.fp8_quantize_ref(w0, sw * one, torch.zeros(1), "e4m3")
    y_pt = SF.fp8_gemm_ref(qx, qw, 1.0 / sx, 1.0 / sw, None, torch.bfloat16).double()
    excess_pt = (y_pt - y_true).abs() / bound
    print(f"per-tensor: max error / bound on the large rows {excess_pt[~small].max().item():.3f}, "
          f"on the small rows {excess_pt[small].amax(-1).min().item():.3f} .. {excess_pt[small].max().item():.3f}")
    assert (excess_pt[~small] <= 1.0).all()                  # the large rows are fine either way
    assert (qx[small].float() == 0).all()
    assert (excess_pt[small].amax(-1) > 1.0).all()           # every small row breaks the bound


def _validate(extra, monkeypatch, world=1):
    from smdt_amd.train import arguments as A
    monkeypatch.setenv("WORLD_SIZE", str(world))
    monkeypatch.setenv("RANK", "0")
    return A.validate_args(A.parse_args(argv=BASE + extra), dict(DEFAULTS))


def test_fp8_recipe_flag_takes_effect(monkeypatch):
    from smdt_amd.train import arguments as A
    from smdt_amd.models.transformer import TransformerConfig
    a = _validate(["--fp8-hybrid", "--bf16", "--fp8-recipe", "mxfp8"], monkeypatch)
    a.padded_vocab_size = 256
    cfg = A.core_transformer_config_from_args(a)
    assert cfg.fp8 == "hybrid" and cfg.fp8_recipe == "mxfp8"
    a = _validate(["--fp8-hybrid", "--bf16"], monkeypatch)
    a.padded_vocab_size = 256
    assert A.core_transformer_config_from_args(a).fp8_recipe == "delayed"       # opt-in
    assert TransformerConfig().fp8_recipe == "delayed"
    with pytest.raises(ValueError, match="fp8_recipe"):
        TransformerConfig(fp8_recipe="mxfp8")
    with pytest.raises(ValueError, match="fp8_recipe"):
        TransformerConfig(fp8_recipe="block", fp8="hybrid", params_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="fp8_wgrad"):
        TransformerConfig(fp8_recipe="mxfp8", fp8="hybrid", fp8_wgrad=True, params_dtype=torch.bfloat16)


MX = ["--fp8-hybrid", "--bf16", "--fp8-recipe", "mxfp8"]


@pytest.mark.parametrize("extra,world,needle", [
    (["--bf16", "--fp8-recipe", "mxfp8"], 1, "--fp8-hybrid"),
    (MX + ["--tensor-model-parallel-size", "2"], 2, "--tensor-model-parallel-size"),
    (MX + ["--num-experts", "4"], 1, "--num-experts"),
    (MX + ["--fp8-wgrad"], 1, "--fp8-wgrad"),
    (MX + ["--fp8-margin", "1"], 1, "--fp8-margin"),
    (MX + ["--fp8-interval", "2"], 1, "--fp8-interval"),
    (MX + ["--fp8-amax-history-len", "4"], 1, "--fp8-amax-history-len"),
    (MX + ["--fp8-amax-compute-algo", "max"], 1, "--fp8-amax-compute-algo"),
    (MX + ["--seq-length", "32"], 1, "tokens per micro-batch"),
    (MX + ["--hidden-size", "192", "--num-attention-heads", "2", "--kv-channels", "64"], 1, "--hidden-size"),
    (MX + ["--ffn-hidden-size", "448"], 1, "--ffn-hidden-size"),
    (MX + ["--kv-channels", "32"], 1, "--num-attention-heads x --kv-channels"),
    (MX + ["--hidden-size", "256", "--num-attention-heads", "4", "--group-query-attention", "--num-query-groups", "1"],
     1, "--num-query-groups x --kv-channels"),
])
def test_fp8_recipe_rejected_combinations(extra, world, needle, monkeypatch):
    with pytest.raises(ValueError) as e:
        _validate(extra, monkeypatch, world)
    assert needle in str(e.value) and "--fp8-recipe mxfp8" in str(e.value), str(e.value)


def _tiny_gpt(recipe):
    from smdt_amd.models.gpt import GPTModel
    from smdt_amd.models.transformer import TransformerConfig
    from smdt_amd.parallel import state as ps
    ps.destroy_model_parallel()
    cfg = TransformerConfig(num_layers=1, hidden_size=128, num_attention_heads=2, max_position_embeddings=64,
                            padded_vocab_size=128, hidden_dropout=0.0, attention_dropout=0.0, seed=3,
                            params_dtype=torch.bfloat16, fp8="hybrid", fp8_recipe=recipe)
    return GPTModel(cfg, device="cpu")


def test_mxfp8_model_has_no_fp8_state_and_loads_a_delayed_checkpoint(capsys):
    from smdt_amd.parallel import tensor_parallel as tp
    delayed, mx = _tiny_gpt("delayed"), _tiny_gpt("mxfp8")
    sd = delayed.state_dict()
    assert any("fp8_state" in k for k in sd)
    assert not any("fp8" in k for k in mx.state_dict())
    assert not any(isinstance(m, tp.FP8State) for m in mx.modules())
    assert len(list(mx.buffers())) == len(list(_tiny_gpt("delayed").buffers())) - 6     # the table's six buffers
    for lin in (mx.decoder.layers[0].attention.qkv, mx.decoder.layers[0].mlp.fc2):
        assert isinstance(lin._fp8[0], tp.MXFP8Recipe) and lin._fp8[0].grad_fmt == "e5m2"
    capsys.readouterr()
    mx.load_state_dict(sd)                              # strict: the table is dropped, with one notice
    out = capsys.readouterr().out
    assert out.count("--fp8-recipe mxfp8 keeps no scaling state") == 1
    delayed.load_state_dict(mx.state_dict())            # the other direction starts from scales 1
    assert "holds no scaling state" in capsys.readouterr().out
    toks = torch.randint(0, 100, (2, 65), generator=torch.Generator().manual_seed(4))
    loss = mx(toks[:, :-1], labels=toks[:, 1:]).float().mean()
    loss.backward()
    tp.flush_deferred_wgrad()
    tp.params_changed()
    assert torch.isfinite(loss) and loss.item() != delayed(toks[:, :-1], labels=toks[:, 1:]).float().mean().item()


@pytest.mark.slow
def test_pretrain_gpt_mxfp8_trains_and_reloads(tmp_path):
    import re
    script = os.path.join(REPO, "recipes", "3_training_megatron-lm", "pretrain_gpt.py")
    ck = str(tmp_path / "ck")
    args = BASE + ["--global-batch-size", "2", "--lr", "0.001", "--lr-warmup-iters", "1", "--mock-data",
                   "--log-interval", "1", "--eval-interval", "100", "--eval-iters", "1", "--vocab-size", "256",
                   "--tokenizer-type", "NullTokenizer"] + MX
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29549",
               CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, script] + args + ["--train-iters", "2", "--save", ck, "--save-interval", "2"],
                       env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    losses = [float(re.search(r"lm loss: (\S+)", ln).group(1)) for ln in r.stdout.splitlines()
              if "lm loss:" in ln and "iteration" in ln]
    assert len(losses) == 2 and all(torch.isfinite(torch.tensor(losses))), r.stdout[-2000:]
    saved = torch.load(os.path.join(ck, "iter_0000002", "mp_rank_00", "model_optim_rng.pt"), map_location="cpu",
                       weights_only=True)
    assert saved["args"]["fp8_recipe"] == "mxfp8"
    assert not any("fp8" in k for k in saved["model"])
    r = subprocess.run([sys.executable, script] + args + ["--train-iters", "3", "--load", ck],
                       env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "iteration        3/" in r.stdout or re.search(r"iteration\s+3/\s*3", r.stdout), r.stdout[-2000:]
