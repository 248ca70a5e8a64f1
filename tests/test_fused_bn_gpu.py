"""Fused BatchNorm + add + ReLU kernels (csrc/kernels/batchnorm.hip) on the GPU.

Everything is judged against the float64 twin on the same 16-bit inputs; the backward reference is
given the kernel's own ``y`` for the ReLU mask (the contract: the mask is the sign of the stored
output). With u = 2^-24 and r = one ulp of the activation type, reductions may err by
64 u sum|summand| and elementwise outputs by r |ref| plus 64 u times the magnitudes of their terms.
``invstd`` and the running statistics carry the reductions' bound through their formulas. Each test
prints its largest error / bound ratio (profiles/fused_bn/README.md). Row counts come from
``bn_act_plan``: the smallest at which the kernels can go wrong.

The two rows of the M = 2 cases are drawn at least 2 apart in every channel. Two random values that
nearly coincide make a channel with |mean| invstd in the hundreds, where the rounding of a mean
stored in fp32 alone can move dx by more than the bound, whatever computes it: that is the condition
of the problem, not a property of the kernel. With rows that far apart dx is eps / var times a
difference and lands among fp16's subnormals, so r |ref| is taken as what it stands for, one ulp of
the output type at ref: never below the type's smallest subnormal (2^-24 for fp16)."""
import pytest
import torch
import torch.nn.functional as F

from smdt_amd.models.resnet import resnet
from smdt_amd.ops import functional as SF

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DTYPES = {"bf16": (torch.bfloat16, 2.0 ** -8), "fp16": (torch.float16, 2.0 ** -11)}
TINY = {2.0 ** -8: 2.0 ** -133, 2.0 ** -11: 2.0 ** -24}     # smallest subnormal of the type with ulp r
MODES = {"plain": (False, False), "relu": (False, True), "residual_relu": (True, True)}
CHANNELS = [8, 24, 64, 520]     # one group; 3 groups; one full tile; two tiles of 33 + 32 groups
ROWS = ["two", "slab-1", "slab", "slab+1", "many_slabs"]
EPS, MOM = 1e-5, 0.1


def _rows(kind, C):
    slab = SF.bn_act_plan(2, C)["slab_rows"]
    lanes = SF.bn_act_constants()["finalize_lanes"]
    M = {"two": 2, "slab-1": slab - 1, "slab": slab, "slab+1": slab + 1, "many_slabs": slab * (lanes + 1) + 3}[kind]
    assert SF.bn_act_plan(M, C)["slabs"] == {"two": 1, "slab-1": 1, "slab": 1, "slab+1": 2, "many_slabs": lanes + 2}[kind]
    return M


def _nhwc(M, C, dtype, gen, scale=2.0, shift=0.5):
    """A channels_last [N, C, H, W] tensor with N H W = M and H W odd."""
    h, w = next(hw for hw in ((13, 13), (7, 9), (5, 3), (11, 1), (1, 5), (3, 1), (1, 1)) if M % (hw[0] * hw[1]) == 0)
    t = torch.randn(M // (h * w), h, w, C, device="cuda", generator=gen) * scale + shift
    return t.to(dtype).permute(0, 3, 1, 2)


def _inputs(M, C, dtype, has_res, seed=0):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = _nhwc(M, C, dtype, gen)
    if M == 2:
        centre, spread = x[:1].float(), x[1:].float().abs() / 2 + 1
        x = torch.cat([centre + spread, centre - spread]).to(dtype).contiguous(memory_format=torch.channels_last)
    x.requires_grad_()
    res = _nhwc(M, C, dtype, gen, 1.0, 0.0).requires_grad_() if has_res else None
    dy = _nhwc(M, C, dtype, gen, 1.0, 0.0)
    gamma = (torch.rand(C, device="cuda", generator=gen) + 0.5).requires_grad_()
    beta = (torch.rand(C, device="cuda", generator=gen) - 0.5).requires_grad_()
    return x, res, dy, gamma, beta


def _run(x, res, dy, gamma, beta, rm, rv, training, relu):
    assert SF.batch_norm_act_supported(x, gamma, beta, rm, rv, res, relu)
    y = SF.batch_norm_act(x, gamma, beta, rm, rv, training, MOM, EPS, residual=res, relu=relu)
    assert y.shape == x.shape and y.dtype == x.dtype and y.permute(0, 2, 3, 1).is_contiguous()
    grads = torch.autograd.grad(y, [t for t in (x, res, gamma, beta) if t is not None], dy)
    return (y.detach(),) + grads


def _ratio(name, got, ref, bound, out):
    out[name] = ((got.double() - ref).abs() / bound.clamp_min(1e-300)).max().item()


def _check(ratios, label):
    print(f"\n[fused_bn] {label}: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios


def _sum(t):
    return t.sum((0, 2, 3))


def _ulp(ref, r):
    return (r * ref.abs()).clamp_min(TINY[r])


def _y_bound(x, res, gamma, beta, mean, invstd, ref, r):
    sh = (1, -1, 1, 1)
    a = gamma.double() * invstd
    b = beta.double() - mean * a
    terms = (a.view(sh) * x.double()).abs() + b.abs().view(sh) + (0 if res is None else res.double().abs())
    return _ulp(ref, r) + 64 * U * terms


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("C", CHANNELS)
def test_training_forward_backward(C, rows, dt, mode):
    (dtype, r), (has_res, relu) = DTYPES[dt], MODES[mode]
    M = _rows(rows, C)
    x, res, dy, gamma, beta = _inputs(M, C, dtype, has_res)
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    y, dx, *rest = _run(x, res, dy, gamma, beta, rm, rv, True, relu)
    dres = rest.pop(0) if has_res else None
    dgamma, dbeta = rest
    with torch.no_grad():
        sh = (1, -1, 1, 1)
        xd, dyd, gd = x.double(), dy.double(), gamma.double()
        rm64, rv64 = torch.zeros_like(rm, dtype=torch.float64), torch.ones_like(rv, dtype=torch.float64)
        yref = SF.batch_norm_act_ref(xd, gd, beta.double(), rm64, rv64, True, MOM, EPS,
                                     residual=None if res is None else res.double(), relu=relu)
        mean = xd.mean((0, 2, 3))
        var = (xd - mean.view(sh)).square().mean((0, 2, 3))
        invstd = (var + EPS).rsqrt()
        mean_b = 64 * U * _sum(xd.abs()) / M
        var_b = 64 * U * var
        out = {}
        _ratio("running_mean", rm, rm64, MOM * mean_b, out)
        _ratio("running_var", rv, rv64, MOM * var_b * (M / (M - 1)), out)
        _ratio("y", y, yref, _y_bound(x, res, gamma, beta, mean, invstd, yref, r), out)
        dxr, g, dgr, dbr = SF.batch_norm_act_backward_ref(dyd, xd, y if relu else None, gd, mean, invstd, True)
        xhat = (xd - mean.view(sh)) * invstd.view(sh)
        sg, sgx = _sum(g.abs()), _sum((g * xhat).abs())
        _ratio("dbeta", dbeta, dbr, 64 * U * sg, out)
        _ratio("dgamma", dgamma, dgr, 64 * U * sgx, out)
        a = (gd * invstd).abs().view(sh)
        _ratio("dx", dx, dxr, _ulp(dxr, r) + 64 * U * a * (g.abs() + (sg / M).view(sh) + xhat.abs() * (sgx / M).view(sh)),
               out)
        if has_res:
            assert torch.equal(dres, g.to(dtype))
    _check(out, f"C {C} M {M} {dt} {mode}")


@pytest.mark.parametrize("dt", DTYPES)
def test_statistics_and_cancellation(dt):
    """mean and invstd themselves: running statistics started at (0, 0) and moved with momentum 1
    are the batch mean and the unbiased batch variance. Channel 5 holds only 64 and 64.5: variance
    0.0625 under mean^2 = 4096, where E[x^2] - mean^2 in fp32 has no correct digit."""
    dtype, _ = DTYPES[dt]
    C = 24
    M = _rows("many_slabs", C)
    x, _, _, gamma, beta = _inputs(M, C, dtype, False, seed=1)
    with torch.no_grad():
        pick = torch.rand(x[:, 5].shape, device="cuda") < 0.5
        x[:, 5] = torch.where(pick, 64.0, 64.5).to(dtype)
        rm, rv = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
        SF.batch_norm_act(x, gamma, beta, rm, rv, True, 1.0, EPS, relu=False)
        xd = x.double()
        mean = xd.mean((0, 2, 3))
        var = (xd - mean.view(1, -1, 1, 1)).square().mean((0, 2, 3))
        assert abs(var[5].item() - 0.0625) < 1e-3
        out = {}
        _ratio("mean", rm, mean, 64 * U * _sum(xd.abs()) / M, out)
        got = (rv.double() * ((M - 1) / M) + EPS).rsqrt()       # invstd from the stored unbiased variance
        ref = (var + EPS).rsqrt()
        _ratio("invstd", got, ref, 0.5 * ref ** 3 * 64 * U * var, out)
    _check(out, f"cancellation {dt}")


@pytest.mark.parametrize("dt", DTYPES)
def test_bitwise_repeatable(dt):
    C = 520
    x, res, dy, gamma, beta = _inputs(_rows("many_slabs", C), C, DTYPES[dt][0], True)
    runs = [_run(x, res, dy, gamma, beta, torch.zeros(C, device="cuda"), torch.ones(C, device="cuda"), True, True)
            for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(*runs))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dt", DTYPES)
def test_eval_mode(dt, mode):
    (dtype, r), (has_res, relu) = DTYPES[dt], MODES[mode]
    C = 520
    x, res, dy, gamma, beta = _inputs(_rows("slab+1", C), C, dtype, has_res)
    rm = torch.randn(C, device="cuda") * 0.5 + 0.5
    rv = torch.rand(C, device="cuda") * 4 + 1
    rm0, rv0 = rm.clone(), rv.clone()
    y, dx, *_ = _run(x, res, dy, gamma, beta, rm, rv, False, relu)
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0)
    with torch.no_grad():
        mean, invstd = rm.double(), (rv.double() + EPS).rsqrt()
        yref = SF.batch_norm_act_ref(x.double(), gamma.double(), beta.double(), mean, rv.double(), False, MOM, EPS,
                                     residual=None if res is None else res.double(), relu=relu)
        out = {}
        _ratio("y", y, yref, _y_bound(x, res, gamma, beta, mean, invstd, yref, r), out)
        dxr, g, _, _ = SF.batch_norm_act_backward_ref(dy.double(), x.double(), y if relu else None, gamma.double(),
                                                      mean, invstd, False)
        _ratio("dx", dx, dxr, _ulp(dxr, r) + 64 * U * dxr.abs(), out)
    _check(out, f"eval {dt} {mode}")


def test_graph_capture_replays_eager():
    C, dtype = 64, torch.bfloat16
    x, res, dy, gamma, beta = _inputs(_rows("many_slabs", C), C, dtype, True)
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _run(x, res, dy, gamma, beta, rm, rv, True, True)
    torch.cuda.current_stream().wait_stream(side)
    rm.zero_(), rv.fill_(1.0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = _run(x, res, dy, gamma, beta, rm, rv, True, True)
    erm, erv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    for _ in range(3):
        graph.replay()
        eager = _run(x, res, dy, gamma, beta, erm, erv, True, True)
        assert all(torch.equal(a, b) for a, b in zip(outs, eager))
        assert torch.equal(rm, erm) and torch.equal(rv, erv)
    assert not torch.equal(rm, torch.zeros_like(rm))


def test_resnet18_fused_against_unfused():
    """One bf16-autocast training step, channels_last: the fused model may differ from the unfused
    one by at most twice what the unfused one differs from its own fp32 run (relative Frobenius
    distance of the logits, and of all parameter gradients together)."""
    torch.manual_seed(0)
    plain = resnet("resnet18", 10).cuda().to(memory_format=torch.channels_last)
    fused = resnet("resnet18", 10, fused_bn=True).cuda().to(memory_format=torch.channels_last)
    fused.load_state_dict(plain.state_dict())
    x = torch.randn(8, 3, 64, 64, device="cuda").contiguous(memory_format=torch.channels_last)
    labels = torch.arange(8, device="cuda") % 10

    def step(model, autocast):
        model.zero_grad(set_to_none=True)
        state = {k: v.clone() for k, v in model.state_dict().items()}
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            logits = model(x)
        F.cross_entropy(logits.float(), labels).backward()
        model.load_state_dict(state)    # every run starts from the same running statistics
        return logits.detach().double(), torch.cat([p.grad.double().flatten() for p in model.parameters()])

    dist = lambda a, b: ((a - b).norm() / b.norm()).item()  # noqa: E731
    exact, lowp, ours = step(plain, False), step(plain, True), step(fused, True)
    for name, e, l, o in zip(("logits", "gradients"), exact, lowp, ours):
        yard, d = dist(l, e), dist(o, l)
        print(f"\n[fused_bn] resnet18 {name}: unfused bf16 vs fp32 {yard:.3e}, fused vs unfused {d:.3e}")
        assert d <= 2 * yard, (name, d, yard)
