"""--fp8-fused-quantize on the GPU: the FP8-output forms of layernorm.hip and bias_act.hip against the
chain of kernels they replace (16-bit producer, then ``fp8_quantize``), bit for bit, at one row width
per (G, C) geometry class of the norm (the table of tests/test_norm_softmax_gpu.py, plus 768) and at
the activation kernel's column-block and row-batch tails; a float64 bound; the saturation, NaN and
amax edges; ``FP8Linear`` with a handed-over operand; and a 2-layer GPT step with the flag on
against the same step with it off."""
import pytest
import torch
import torch.nn.functional as F

from smdt_amd.ops import functional as SF

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, HF = torch.bfloat16, torch.float16
NORMS = ["layer_norm", "rms_norm", "layer_norm_1p", "bda_norm_p0", "bda_norm_p0.1"]
ACTS = ["gelu_tanh", "gelu_erf", "swiglu"]
# width -> row counts. Past one grid pass: the norm forward loops past 2048 blocks of 256 / G rows,
# the activation kernel past 65535 slices of 4 rows (6 rows: one batch of 4 and a tail of 2).
SHAPES = {"norm": {512: (1, 17), 520: (1, 17), 768: (1, 17, 8195), 1536: (1, 17), 2048: (1, 17, 8195), 2056: (1, 17),
                   5120: (1, 17, 2051), 12288: (1, 17), 16384: (1, 17, 2051)},
          "act": {16: (1, 6, 17, 262145), 1040: (1, 6, 17), 2048: (1, 6, 17), 4112: (1, 6, 17)}}


def _producer(name, rows, width, T, seed=0, nan=False):
    """fn(**fp8 keywords) -> (y or (y, q), s or None) on fixed inputs, and fn64(s) -> float64 reference."""
    g = torch.Generator(device=DEV).manual_seed(1000 + seed)
    rnd = lambda *s, k=1.0: (k * torch.randn(*s, device=DEV, generator=g)).to(T)
    x = rnd(rows, 2 * width if name == "swiglu" else width)
    if nan:
        x[3, 5] = float("nan")
    # layer_norm_1p: what Norm.fused hands the kernel, 1 + a zero-centred weight
    gamma = rnd(width, k=0.2) + 1 if name == "layer_norm_1p" else rnd(width, k=0.5) + 1.5
    res, beta, bias = rnd(rows, width), rnd(width, k=0.2), rnd(width, k=0.2)
    d = lambda t: t.double()
    if name == "swiglu":
        return (lambda **k: (SF.swiglu(x, **k), None)), lambda s: F.silu(d(x)[:, :width]) * d(x)[:, width:]
    if name in ACTS:
        approx = "tanh" if name == "gelu_tanh" else "none"
        return (lambda **k: (SF.bias_gelu(x, bias, approx, **k), None)), lambda s: F.gelu(d(x) + d(bias), approximate=approx)
    ln64 = lambda s: F.layer_norm(d(s), (width,), d(gamma), d(beta), 1e-5)
    if name.startswith("bda"):      # the reference normalises the residual stream s as the kernel rounded it
        p = float(name.split("_p")[1])
        return (lambda **k: SF.bias_dropout_add_norm(x, bias, res, gamma, beta, p, True, rng=SF.PhiloxState(7), **k)), ln64
    if name == "rms_norm":
        return (lambda **k: (SF.rms_norm(x, gamma, 1e-5, **k), None)), \
            lambda s: d(x) * torch.rsqrt(d(x).pow(2).mean(-1, keepdim=True) + 1e-5) * d(gamma)
    return (lambda **k: (SF.layer_norm(x, gamma, beta, **k), None)), lambda s: ln64(x)


def _same_as_chain(fn, keep16, scale=37.0, amax0=0.0):
    """Asserts q, amax, s and (kept) y16 of the fused producer equal the chain of existing kernels;
    returns (y of the chain, q, amax)."""
    sc = torch.tensor([scale], device=DEV)
    a_ref, a = (torch.tensor([amax0], device=DEV) for _ in range(2))
    (y_ref, s_ref), ((y, q), s) = fn(), fn(fp8_out=(sc, a), keep16=keep16)
    # the existing quantise kernel takes multiples of 16 columns; the rule is elementwise
    y2 = y_ref.reshape(-1, 8).repeat(1, 2) if y_ref.shape[-1] % 16 else y_ref
    q_ref = SF.fp8_quantize(y2, sc, a_ref, "e4m3")[:, :y_ref.numel() // y2.shape[0]].reshape(y_ref.shape)
    assert q.dtype == torch.float8_e4m3fn and torch.equal(q.view(torch.uint8), q_ref.view(torch.uint8))
    assert torch.equal(a.view(torch.int32), a_ref.view(torch.int32))
    assert s_ref is None or torch.equal(s, s_ref)
    if keep16:
        assert torch.equal(y.view(torch.int16), y_ref.view(torch.int16))
    else:                           # no 16-bit output was written: y only carries the gradient
        assert y.shape == y_ref.shape and y.dtype == y_ref.dtype and y.untyped_storage().nbytes() == 2
    return y_ref, q, a


@pytest.mark.parametrize("keep16", [True, False], ids=["keep16", "q_only"])
@pytest.mark.parametrize("T", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", NORMS + ACTS)
def test_fp8_out_equals_the_two_kernel_chain(name, T, keep16):
    for width, row_counts in SHAPES["act" if name in ACTS else "norm"].items():
        for rows in row_counts:
            _, _, a = _same_as_chain(_producer(name, rows, width, T)[0], keep16)
            assert a.item() > 0


@pytest.mark.parametrize("T", [BF, HF], ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", NORMS + ACTS)
def test_dequantised_output_against_float64(name, T):
    """|q / scale - ref| <= |ref| (r16 + 2^-4) + 2^-10 / scale: one rounding to the 16-bit dtype
    (r16 = 2^-9 bf16, 2^-11 fp16), the E4M3 half-ulp of a normal (2^-4 relative) and of a subnormal
    (2^-10 absolute, before unscaling). The scale puts the largest |ref| at half of 448."""
    fn, fn64 = _producer(name, 17, 1040 if name in ACTS else 768, T, seed=1)
    ref = fn64(fn()[1])
    scale = 224.0 / ref.abs().max().item()
    (_, q), _ = fn(fp8_out=(torch.tensor([scale], device=DEV), torch.zeros(1, device=DEV)), keep16=False)
    err = (q.double() / scale - ref).abs()
    bound = ref.abs() * ((2.0 ** -9 if T == BF else 2.0 ** -11) + 2.0 ** -4) + 2.0 ** -10 / scale
    print(f"{name} {T}: worst err / bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("keep16", [True, False], ids=["keep16", "q_only"])
@pytest.mark.parametrize("name", ["layer_norm", "gelu_tanh"])
def test_saturation_nan_and_amax_edges(name, keep16):
    rows, width = 17, 1040 if name in ACTS else 768
    fn = _producer(name, rows, width, BF, seed=2)[0]
    top = fn()[0].float().abs().max().item()
    # a scale that saturates part of every row: clamped to +-448, as the chain clamps
    _, q, _ = _same_as_chain(fn, keep16, 4 * 448.0 / top)
    assert q.float().abs().max().item() == 448.0 and 0 < (q.float().abs() == 448.0).float().mean().item() < 0.5
    # an amax above the tensor's stays, one below becomes exactly the tensor's
    for amax0, want in ((2 * top, 2 * top), (0.5 * top, top)):
        assert _same_as_chain(fn, keep16, amax0=amax0)[2].item() == torch.tensor(want).float().item()
    # a NaN input stays a NaN byte (a whole row behind a norm), the 16-bit NaN is the chain's, amax is NaN
    y, q, a = _same_as_chain(_producer(name, rows, width, BF, seed=2, nan=True)[0], keep16)
    assert torch.equal(q.float().isnan(), y.isnan()) and q.float().isnan()[3, 5] and not q.float().isnan()[4].any()
    assert a.isnan().all()


@pytest.mark.parametrize("fp8_wgrad", [False, True], ids=["wgrad16", "wgrad8"])
def test_fp8_linear_takes_a_handed_over_operand(fp8_wgrad):
    from smdt_amd.parallel import state as ps
    from smdt_amd.parallel import tensor_parallel as tp
    ps.destroy_model_parallel()
    g = torch.Generator(device=DEV).manual_seed(3)
    rnd = lambda *s, k=1.0: (k * torch.randn(*s, device=DEV, generator=g)).bfloat16()
    w0, b0, x0, dy = rnd(192, 128, k=0.05), rnd(192, k=0.1), rnd(4, 32, 128), rnd(4, 32, 192, k=3.0)

    def run(handed):
        st = tp.FP8State(1, "hybrid", device=DEV, fp8_wgrad=fp8_wgrad)
        st.scale.copy_(torch.tensor([37.0, 1900.0, 410.0]))
        torch.reciprocal(st.scale, out=st.scale_inv)
        w, b = torch.nn.Parameter(w0.clone()), torch.nn.Parameter(b0.clone())
        w.main_grad = torch.zeros(192, 128, device=DEV)
        x = x0.clone().requires_grad_()
        qx = SF.fp8_quantize(x0.reshape(-1, 128), *st.slot(0)[:2], "e4m3").view(x0.shape) if handed else None
        y = tp.FP8Linear.apply(x, w, b, True, st, 0, qx)
        y.backward(dy)
        tp.flush_deferred_wgrad()
        return y.detach(), x.grad, w.main_grad, b.grad, st.amax.clone()

    for a, b in zip(run(True), run(False)):
        assert torch.equal(a, b)


def _gpt_step(fused, fp8_wgrad, graph, dropout):
    from smdt_amd.models.gpt import GPTModel
    from smdt_amd.models.transformer import TransformerConfig
    from smdt_amd.optim.optimizer import MixedPrecisionAdam
    from smdt_amd.parallel import state as ps
    from smdt_amd.parallel.distributed import DistributedDataParallel as DDP
    from smdt_amd.parallel.random import get_rng
    from smdt_amd.train.graphs import CapturedStep
    ps.destroy_model_parallel()
    for kind in ("default", "tp"):          # both runs of a pair draw the same dropout offsets
        get_rng(kind).load_state_dict({"seed": 1234, "offset": 0})
    cfg = TransformerConfig(num_layers=2, hidden_size=256, num_attention_heads=4, padded_vocab_size=1024,
                            max_position_embeddings=128, hidden_dropout=dropout, attention_dropout=dropout,
                            params_dtype=torch.bfloat16, seed=5, fp8="hybrid", fp8_wgrad=fp8_wgrad,
                            fp8_fused_quantize=fused)
    with torch.random.fork_rng(devices=[0]):     # later test files draw from the global generators
        torch.manual_seed(1234)
        model = GPTModel(cfg, device=DEV)
        ddp = DDP(model, grad_dtype=torch.float32)
        opt = MixedPrecisionAdam(ddp, lr=1e-3, weight_decay=0.01, clip_grad=1.0, capturable=True)
        g = torch.Generator(device=DEV).manual_seed(11)
        toks = [torch.randint(0, 1000, (2, 129), device=DEV, generator=g) for _ in range(3)]

        def step(t):
            ddp.zero_grad_buffer()
            loss = model(t[:, :-1], labels=t[:, 1:]).float().mean()
            loss.backward()
            ddp.finish_grad_sync()
            opt.step()
            return loss.detach()

        run = CapturedStep(step, warmup=1, enabled=graph)
        st = model.decoder.fp8_state
        out = []
        for t in toks:
            out += [run(t).clone(), ddp.grad_data.clone(), st.scale.clone(), st.amax_history.clone()]
        torch.cuda.synchronize()
    assert run.note == ("captured" if graph else "eager"), run.note
    ps.destroy_model_parallel()
    return out


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "captured"])
@pytest.mark.parametrize("fp8_wgrad", [False, True], ids=["wgrad16", "wgrad8"])
def test_gpt_step_equals_the_unfused_fp8_step(fp8_wgrad, graph):
    """Three steps with dropout 0.1 (eager, and one eager step then a capture replayed twice): loss,
    all of main_grad and the FP8 table after each scale update, flag on against flag off."""
    on, off = _gpt_step(True, fp8_wgrad, graph, 0.1), _gpt_step(False, fp8_wgrad, graph, 0.1)
    assert (off[2] != 1).any() and not torch.equal(off[1], off[5])
    for a, b in zip(on, off):
        assert torch.equal(a, b)


def test_captured_fused_step_equals_eager():
    """With the flag on, the replayed capture against the same steps run eagerly, bitwise. Without
    dropout: a capture freezes the dropout offsets of the step it recorded, flag or no flag."""
    for a, b in zip(_gpt_step(True, True, False, 0.0), _gpt_step(True, True, True, 0.0)):
        assert torch.equal(a, b)
