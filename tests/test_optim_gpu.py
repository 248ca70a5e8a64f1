"""optim.hip at every grid and tail geometry, dtype and mode, against the float64 references of
tests/_numerics.py.

The fused Adam / AdamW kernel gives each thread one 4-element vector (256 per block, no
grid-stride loop) and leaves n % 4 elements to a scalar tail in block 0; a buffer below 4 elements
is launched as one block that runs only the tail. The sizes below are a tail alone, no tail, one
vector plus tail, one full block, a second block with a single live lane, and several blocks plus
tail. ``sumsq``, ``scale_`` and ``cast_`` are grid-stride loops over 16-byte vectors (32 bytes for
``cast_``) capped at 2048 blocks, with a scalar tail in block 0: their sizes put elements in the
tail, in the last full vector and in a last, partial trip of the loop past the cap.

Every buffer a kernel writes sits between guard elements that must come back bit-unchanged. Adam's
m', v' and p' are judged by ``adam_excess`` at ADAM_TOL (4x the error of the fp32 emulation of the
kernel, measured on the CPU by tests/test_numerics_sensitivity.py, which also shows that the
criterion rejects a step with one term wrong); the 16-bit model copy, the skipped step, the
capturable form, ``cast_`` and fp32 ``scale_`` are judged bit for bit.
"""
import math

import pytest
import torch
import torch.nn as nn

from smdt_amd.ops import _ext

import _numerics as N

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
PAD = 16                    # guard elements on each side: the middle slice stays 32 / 64-byte aligned
SENTINEL = -77.0            # exact in fp32, bf16 and fp16
E32 = torch.finfo(F32).eps


def _C():
    return _ext.ext()


def _guarded(t):
    """A device buffer [sentinel x PAD | t | sentinel x PAD] and the view of its middle."""
    n = t.numel()
    buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=t.dtype, device=DEV)
    buf[PAD:PAD + n] = t.to(DEV)
    return buf, buf[PAD:PAD + n]


def _guards_intact(buf):
    g = torch.full((PAD,), SENTINEL, dtype=buf.dtype, device=buf.device)
    return torch.equal(buf[:PAD], g) and torch.equal(buf[-PAD:], g)


def _bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


def _vec(dtype):
    return 16 // torch.empty((), dtype=dtype).element_size()


# ------------------------------------------------------------------------------------- Adam

class _AdamState:
    """p, g, m, v (and the model copy) of one ``adam_case`` on the device, each between guards."""

    def __init__(self, case, model_dtype):
        self.bufs, self.model_dtype = {}, model_dtype
        for k in ("p", "g", "m", "v"):
            self.bufs[k], view = _guarded(case[k])
            setattr(self, k, view)
        self.model = None
        if model_dtype is not None:     # starts as a copy of nothing the kernel writes: all ones
            self.bufs["model"], self.model = _guarded(torch.ones(case["p"].numel(), dtype=model_dtype))

    def snapshot(self):
        return {k: getattr(self, k).clone() for k in ("p", "g", "m", "v")} | (
            {} if self.model is None else {"model": self.model.clone()})

    def assert_guards(self, what):
        for k, b in self.bufs.items():
            assert _guards_intact(b), f"{what}: the kernel wrote outside '{k}'"


def _mul(mode):
    return None if mode["grad_mul"] is None else torch.tensor([mode["grad_mul"]], dtype=F32, device=DEV)


def _adam(st, mode, found=None, step=None):
    _C().adam(st.p, st.g, st.m, st.v, st.model, N.ADAM_LR, mode["betas"][0], mode["betas"][1], N.ADAM_EPS,
              mode["wd"], mode["step"] if step is None else step, mode["adamw"], _mul(mode), found)


def _judge_step(st, before, mode, what, step=None):
    """One kernel step from ``before`` (the state it started from) against ``adam_ref`` of the same
    state; prints every figure first."""
    hy = N.adam_hyper(mode)
    if step is not None:
        hy["step"] = step
    cpu = {k: before[k].cpu() for k in ("p", "g", "m", "v")}
    ref = N.adam_ref(cpu["p"], cpu["g"], cpu["m"], cpu["v"], **hy)
    ex = N.adam_excess((st.p, st.m, st.v), ref, cpu["p"])
    print(f"adam {what}: error / bound " + " ".join(f"{k}={x:.3f}" for k, x in ex.items()))
    st.assert_guards(what)
    assert torch.equal(st.g, before["g"]), f"{what}: the gradient was written"
    dead = (before["p"] == 0) & (before["g"] == 0)
    assert bool((st.p[dead] == 0).all()), f"{what}: an element with p = g = 0 moved"
    assert max(ex.values()) <= 1.0, (what, ex)
    if st.model is not None:
        assert torch.equal(_bits(st.model), _bits(st.p.to(st.model_dtype))), f"{what}: model copy != p' cast once"


@pytest.mark.parametrize("n", N.ADAM_SIZES)
def test_adam_geometry(n):
    """Every grid / tail shape of the launcher (see the header), AdamW with weight decay, grad_mul
    and a bf16 model copy; guards around all five buffers."""
    mode = N.ADAM_GEOMETRY_MODE
    st = _AdamState(N.adam_case(n, N.adam_kind(mode["adamw"])), mode["model"])
    before = st.snapshot()
    _adam(st, mode)
    _judge_step(st, before, mode, f"n={n}")


_MODE_PARAMS = [(i, n) for i, md in enumerate(N.ADAM_MODES) for n in md["sizes"]]


@pytest.mark.parametrize("i,n", _MODE_PARAMS)
def test_adam_modes(i, n):
    """AdamW / L2 with and without weight decay, grad_mul None / 0.37, steps 1 / 2 / 1000 / 100000,
    betas (0.9, 0.95) / (0.9, 0.999), model copy bf16 / fp16 / none (the tail with a null model_out
    included: n = 3, 5, 1027, 3074)."""
    mode = N.ADAM_MODES[i]
    st = _AdamState(N.adam_case(n, N.adam_kind(mode["adamw"])), mode["model"])
    before = st.snapshot()
    _adam(st, mode)
    _judge_step(st, before, mode, f"mode {i} n={n}")


@pytest.mark.parametrize("dtype", [BF, HF])
def test_adam_model_copy_follows_every_step(dtype):
    """Four consecutive AdamW steps at lr = 1e-2 on the same gradients: p crosses 16-bit rounding
    boundaries on most elements, every step is judged from the state the kernel itself left, the
    model copy equals p' cast once after EVERY step and differs from the previous step's copy on
    more than a tenth of the elements (a copy written before the update, written once, or
    truncated cannot pass; tests/test_numerics_sensitivity.py counts the elements on the CPU)."""
    mode = dict(N.ADAM_MODES[0], model=dtype)
    n = 3074
    st = _AdamState(N.adam_case(n, "mixed"), dtype)
    for step in (1, 2, 3, 4):
        before = st.snapshot()
        _adam(st, mode, step=step)
        _judge_step(st, before, mode, f"{dtype} step {step}", step=step)
        changed = (_bits(st.model) != _bits(before["model"])).float().mean().item()
        stale = (_bits(st.model) != _bits(before["p"].to(dtype))).float().mean().item()
        print(f"adam model copy {dtype} step {step}: changed on {changed:.2f}, differs from cast(p before) on {stale:.2f}")
        assert changed > 0.1 and stale > 0.1, (step, changed, stale)


@pytest.mark.parametrize("n", [3, 1027])
def test_adam_found_inf_skips_everything(n):
    """Flag set and inf / nan in the gradient (vector part and tail): p, m, v and the model copy
    are bit-unchanged and finite. Flag present but 0: bit-equal to the step without a flag."""
    mode = N.ADAM_GEOMETRY_MODE
    case = N.adam_case(n, "mixed")
    bad = {k: t.clone() for k, t in case.items()}
    bad["g"][0] = float("inf")
    bad["g"][n - 1] = float("nan")
    bad["g"][n // 2] = float("-inf")
    good = _AdamState(case, BF)
    _adam(good, mode)                                # a clean step first: the model copy holds real values
    good.g.copy_(bad["g"].to(DEV))
    before = good.snapshot()
    _adam(good, mode, found=torch.ones(1, dtype=torch.int32, device=DEV))
    good.assert_guards("skip with inf / nan")
    for k in ("p", "m", "v", "model"):
        assert torch.equal(_bits(getattr(good, k)), _bits(before[k])), f"found_inf = 1 changed '{k}'"
        assert bool(torch.isfinite(getattr(good, k).float()).all()), k
    a, b = _AdamState(case, BF), _AdamState(case, BF)
    _adam(a, mode, found=None)
    _adam(b, mode, found=torch.zeros(1, dtype=torch.int32, device=DEV))
    for k in ("p", "m", "v", "model"):
        assert torch.equal(_bits(getattr(a, k)), _bits(getattr(b, k))), f"found_inf = 0 changed '{k}'"


@pytest.mark.parametrize("adamw", [True, False])
def test_adam_capturable_equals_adam(adamw):
    """``adam_capturable`` reads hyper = [lr, bc1, bc2] (float64, cast to fp32) from the device:
    all four outputs are bit-equal to ``adam`` at steps 1, 2 and 1000 with betas (0.9, 0.999),
    where swapped corrections differ by orders of magnitude. ONE hyper tensor is rewritten in
    place between the calls and each call follows it: the replay property of a captured step."""
    n, b1, b2, wd = 1027, 0.9, 0.999, 0.1
    case = N.adam_case(n, N.adam_kind(adamw))
    a, b = _AdamState(case, BF), _AdamState(case, BF)
    mul = torch.tensor([0.37], dtype=F32, device=DEV)
    hyper = torch.zeros(3, dtype=F32, device=DEV)
    prev = None
    for step, lr in ((1, 1e-2), (2, 1e-2), (1000, 3e-3)):
        hyper.copy_(torch.tensor([lr, 1.0 - b1 ** step, 1.0 - b2 ** step], dtype=torch.float64).float())
        _C().adam(a.p, a.g, a.m, a.v, a.model, lr, b1, b2, N.ADAM_EPS, wd, step, adamw, mul, None)
        _C().adam_capturable(b.p, b.g, b.m, b.v, b.model, hyper, b1, b2, N.ADAM_EPS, wd, adamw, mul, None)
        for k in ("p", "m", "v", "model"):
            assert torch.equal(_bits(getattr(a, k)), _bits(getattr(b, k))), f"step {step}: '{k}' differs"
        b.assert_guards(f"capturable step {step}")
        assert prev is None or not torch.equal(prev, b.p)
        prev = b.p.clone()


def test_optimizer_bindings_refuse_misaligned_buffers():
    """Host-side only: a view one element into a buffer is refused by name before any launch."""
    def views(dtype):
        buf = torch.zeros(64, dtype=dtype, device=DEV)
        return buf[PAD:PAD + 32], buf[1:33]

    ok, off = views(F32)
    ok16, off16 = views(BF)
    hyper = torch.ones(3, dtype=F32, device=DEV)
    names = ("adam master", "adam grad", "adam exp_avg", "adam exp_avg_sq", "adam model_out")
    for i, name in enumerate(names):
        args = [off if j == i else ok for j in range(4)] + [off16 if i == 4 else ok16]
        with pytest.raises(RuntimeError, match=f"'{name}' must be 16-byte aligned"):
            _C().adam(*args, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, True, None, None)
        with pytest.raises(RuntimeError, match=f"'{name}' must be 16-byte aligned"):
            _C().adam_capturable(*args, hyper, 0.9, 0.999, 1e-8, 0.0, True, None, None)
    for o in (off, off16):
        with pytest.raises(RuntimeError, match="'sumsq x' must be 16-byte aligned"):
            _C().sumsq(o, None)
        with pytest.raises(RuntimeError, match="'scale_ x' must be 16-byte aligned"):
            _C().scale_(o, None, 0.5)
    with pytest.raises(RuntimeError, match="'cast_ x' must be 16-byte aligned"):
        _C().cast_(off16, ok, False)
    with pytest.raises(RuntimeError, match="'cast_ y' must be 16-byte aligned"):
        _C().cast_(ok, off16, False)
    assert bool((ok == 0).all()) and bool((ok16 == 0).all())


# ------------------------------------------------------------------------------------ sumsq

SUMSQ_CAP = 2048 * 1024 * 4          # elements at which smdt_sumsq_nblocks reaches its 2048-block cap
SUMSQ_BIG = SUMSQ_CAP + 4099         # past it: every thread loops, the last trip is partial; tail 3


def _sumsq_geometry(n, dtype):
    """(vector width, full vectors, threads of the grid, trips of the grid-stride loop)."""
    V = _vec(dtype)
    nb = min(2048, max(1, (n // 4 + 1 + 1023) // 1024))
    nvec, threads = n // V, nb * 256
    return V, nvec, threads, (nvec + threads - 1) // threads, nb


def _sumsq_input(n, dtype):
    g = torch.Generator(device=DEV).manual_seed(1234 + n % 97)
    return (torch.randn(n, device=DEV, generator=g) * 3.0).to(dtype)


@pytest.mark.parametrize("dtype", [F32, BF, HF])
@pytest.mark.parametrize("which", ["1", "3", "7", "8", "9", "1024V+5", "big"])
def test_sumsq_sum(dtype, which):
    """The sum against float64, twice (bit-equal: fixed reduction order). Bound: the terms are
    non-negative, so the relative error of the fp32 sum is at most (number of roundings on the
    longest path) x eps32 / 2; the path is one square and one add per element a thread visits
    (trips x V, plus one tail element), 12 shuffle stages of the block sum, then in the finalize
    kernel ceil(blocks / 256) adds and 12 more stages. The bound below uses eps32 per rounding,
    twice the worst case."""
    V = _vec(dtype)
    n = SUMSQ_BIG if which == "big" else 1024 * V + 5 if which == "1024V+5" else int(which)
    _, _, _, trips, nb = _sumsq_geometry(n, dtype)
    x = _sumsq_input(n, dtype)
    found = torch.zeros(1, dtype=torch.int32, device=DEV)
    s1 = _C().sumsq(x, found)
    s2 = _C().sumsq(x, found)
    ref = x.double().square().sum().item()
    depth = 2 * (trips * V + 1) + 12 + (nb + 255) // 256 + 12
    rel = abs(s1.double().item() - ref) / ref
    print(f"sumsq {dtype} n={n} trips={trips} blocks={nb}: rel error {rel:.3g}, bound {depth * E32:.3g}")
    assert torch.equal(_bits(s1), _bits(s2)), "sumsq is not deterministic"
    assert rel <= depth * E32, (rel, depth * E32)
    assert found.item() == 0


@pytest.mark.parametrize("dtype", [F32, BF, HF])
@pytest.mark.parametrize("which", ["1", "7", "1024V+5", "big"])
def test_sumsq_flags_bad_values_anywhere(dtype, which):
    """+inf, -inf and nan at element 0, in the last full vector, in the scalar tail and in a vector
    a thread reaches only on its last trip of the loop: each sets the flag; the flag stays set
    after a following clean call and stays 0 on clean input; without a flag the call just returns."""
    V = _vec(dtype)
    n = SUMSQ_BIG if which == "big" else 1024 * V + 5 if which == "1024V+5" else int(which)
    V, nvec, threads, trips, _ = _sumsq_geometry(n, dtype)
    x = _sumsq_input(n, dtype)
    places = {"first": 0}
    if nvec:
        places["last vector"] = nvec * V - 1
    if n % V:
        places["tail"] = n - 1
    if trips > 1:
        places["last trip"] = ((trips - 1) * threads + min(3, nvec - (trips - 1) * threads - 1)) * V + 1
        assert (trips - 1) * threads * V <= places["last trip"] < nvec * V
    if which in ("1024V+5", "big"):
        assert len(places) == 4
    found = torch.zeros(1, dtype=torch.int32, device=DEV)
    _C().sumsq(x, found)
    assert found.item() == 0, "flag set on clean input"
    for where, idx in places.items():
        for bad in (float("inf"), float("-inf"), float("nan")):
            keep = x[idx].clone()
            x[idx] = bad
            found.zero_()
            _C().sumsq(x, found)
            assert found.item() == 1, f"{bad} at {where} (element {idx} of {n}) not flagged"
            out = _C().sumsq(x, None)                       # no flag: just returns the (non-finite) sum
            assert not math.isfinite(out.item())
            x[idx] = keep
            _C().sumsq(x, found)
            assert found.item() == 1, "a clean call cleared the flag"
    found.zero_()
    assert math.isfinite(_C().sumsq(x, found).item()) and found.item() == 0


# -------------------------------------------------------------------------------- clip_coef

@pytest.mark.parametrize("inv_scale", [1.0, 1.0 / 1024])
@pytest.mark.parametrize("max_norm", [1.0, 0.0])
def test_clip_coef(max_norm, inv_scale):
    """norm = sqrt(sumsq) * inv_scale and mul = min(1, max_norm / (norm + 1e-6)) * inv_scale
    (max_norm = 0: no clipping, mul = inv_scale) against float64, for sumsq = 0 and norms below,
    above and equal to max_norm. Relative 1e-6: five fp32 roundings of 6e-8 each."""
    for norm in (0.0, 0.5, 3.0, 1.0):
        ss = (norm / inv_scale) ** 2
        ss32 = torch.tensor([ss], dtype=F32, device=DEV)
        mul, out = _C().clip_coef(ss32, max_norm, inv_scale)
        nref = math.sqrt(ss32.double().item()) * inv_scale
        cref = min(1.0, max_norm / (nref + 1e-6)) if max_norm > 0 else 1.0
        mref = cref * inv_scale
        print(f"clip_coef max_norm={max_norm} inv_scale={inv_scale} norm={norm}: mul {mul.item():.9g} (ref {mref:.9g}) "
              f"norm {out.item():.9g} (ref {nref:.9g})")
        assert abs(out.double().item() - nref) <= 1e-6 * nref
        assert abs(mul.double().item() - mref) <= 1e-6 * mref
        if max_norm == 0:
            assert mul.item() == N.f32_value(inv_scale)
        if norm == 3.0 and max_norm > 0:
            assert mul.item() < 0.34 * inv_scale


# ---------------------------------------------------------------------------- scale_ / cast_

STREAM_BIG = 2048 * 256 * 8 + 2053     # past the 2048-block cap of scale_ / cast_ for every dtype; odd


@pytest.mark.parametrize("dtype", [F32, BF, HF])
@pytest.mark.parametrize("with_mul", [True, False])
def test_scale(dtype, with_mul):
    """x *= mul * cmul (mul a device scalar or absent, cmul = 0.37) at n = 1, V - 1, V, V + 1 and a
    size whose last trip of the grid-stride loop is partial, against x (float64) times the fp32
    factor, rounded to the dtype: exact for fp32 (the fp32 product is that rounding), at most one
    representable value off for the 16-bit types (they round the fp32 product a second time)."""
    V = _vec(dtype)
    cmul = 0.37
    mul = torch.tensor([1.7], dtype=F32, device=DEV) if with_mul else None
    f = torch.tensor(cmul, dtype=F32, device=DEV)
    if with_mul:
        f = mul[0] * f
    for n in (1, V - 1, V, V + 1, STREAM_BIG):
        g = torch.Generator(device=DEV).manual_seed(77 + n % 89)
        buf, x = _guarded((torch.randn(n, device=DEV, generator=g) * 5.0).to(dtype))
        ref = (x.double() * f.double()).to(dtype)
        _C().scale_(x, mul, cmul)
        d = N.ulp_distance(x, ref)
        print(f"scale_ {dtype} mul={with_mul} n={n}: ulp distance {d}")
        assert _guards_intact(buf), f"scale_ wrote outside x at n={n}"
        assert d <= (0 if dtype == F32 else 1), (n, d)
        if dtype == F32:
            assert torch.equal(_bits(x), _bits(ref))


_CAST_PAIRS = [(F32, BF), (F32, HF), (BF, F32), (HF, F32), (F32, F32)]


@pytest.mark.parametrize("ti,to", _CAST_PAIRS)
@pytest.mark.parametrize("accumulate", [False, True])
def test_cast(ti, to, accumulate):
    """y = x (cast once) or y += x (fp32 sum, cast once), bit for bit, for the five supported type
    pairs at n = 1, 7, 8, 9, 4101 and a size past the block cap; guards around y, x unchanged."""
    for n in (1, 7, 8, 9, 4101, STREAM_BIG):
        g = torch.Generator(device=DEV).manual_seed(5 + n % 83)
        x = (torch.randn(n, device=DEV, generator=g) * 4.0).to(ti)
        y0 = (torch.randn(n, device=DEV, generator=g) * 4.0).to(to)
        keep = x.clone()
        buf, y = _guarded(y0)
        _C().cast_(x, y, accumulate)
        ref = (x.float() + y0.float()).to(to) if accumulate else x.to(to)
        assert _guards_intact(buf), f"cast_ wrote outside y at n={n}"
        assert torch.equal(_bits(x), _bits(keep))
        assert torch.equal(_bits(y), _bits(ref)), f"cast_ {ti}->{to} accumulate={accumulate} n={n}"


def test_cast_refuses_bf16_to_fp16():
    x = torch.ones(64, dtype=BF, device=DEV)
    y = torch.zeros(64, dtype=HF, device=DEV)
    with pytest.raises(RuntimeError):
        _C().cast_(x, y, False)
    assert bool((y == 0).all())


# ------------------------------------------------------------------------ MixedPrecisionAdam

def test_mixed_precision_adam_step():
    """Two clipped AdamW steps of ``MixedPrecisionAdam`` over the flat buffers of a bf16 model whose
    parameter sizes (888, 37, 185, 5) are no multiples of 16, so the buffers hold alignment padding:
    the masters and moments follow ``adam_ref`` driven by the float64 clip coefficient (each step from
    the state the optimizer held, ADAM_TOL), ``param_data`` is the masters cast once, ``grad_norm`` is the
    float64 norm, every padding element stays exactly 0, and a third step with one inf gradient
    changes nothing."""
    from smdt_amd.optim.optimizer import MixedPrecisionAdam
    from smdt_amd.parallel import state as ps
    from smdt_amd.parallel.distributed import DistributedDataParallel as DDP
    ps.destroy_model_parallel()
    ps.initialize_emulated_tensor_parallel(1, 8)
    try:
        torch.manual_seed(11)
        model = nn.Sequential(nn.Linear(24, 37), nn.Linear(37, 5)).cuda().bfloat16()
        ddp = DDP(model, torch_compat=True, bucket_size=4096)
        lr, b1, b2, eps, wd, clip = 1e-2, 0.9, 0.999, 1e-8, 0.1, 1.0
        opt = MixedPrecisionAdam(ddp, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, clip_grad=clip)
        assert not opt.zero and ddp.param_data.dtype == BF and ddp.grad_data.dtype == F32
        live = torch.zeros(ddp.numel, dtype=torch.bool, device=DEV)
        for p in ddp.params:
            o, n = ddp.param_index[id(p)]
            live[o:o + n] = True
        assert int(live.sum()) == 888 + 37 + 185 + 5 and bool((~live).any())
        gen = torch.Generator().manual_seed(19)
        mag = torch.pow(10.0, -9.0 + 10.0 * torch.rand(ddp.numel, generator=gen, dtype=torch.float64))
        grads = ((torch.randint(0, 2, (ddp.numel,), generator=gen) * 2.0 - 1.0) * mag).float().to(DEV)
        grads[~live] = 0.0
        ddp.grad_data.copy_(grads)
        pieces = [(s, e, key, mo) for (s, e, key), mo in zip(opt.pieces, opt.master_off) if e > s]
        assert all(key[1] for _, _, key, _ in pieces) and {key[0] for _, _, key, _ in pieces} == {True, False}
        norm = math.sqrt(grads.double().square().sum().item())
        coef = min(1.0, clip / (norm + 1e-6))
        assert coef < 0.5                                     # the clip is active
        for step in (1, 2):
            before = [(opt.master[mo:mo + e - s].cpu(), opt.exp_avg[mo:mo + e - s].cpu(),
                       opt.exp_avg_sq[mo:mo + e - s].cpu()) for s, e, _, mo in pieces]
            opt.step()
            assert abs(opt.grad_norm.double().item() - norm) <= 1e-6 * norm, (opt.grad_norm.item(), norm)
            for (s, e, key, mo), (P, M, V) in zip(pieces, before):
                n = e - s
                ref = N.adam_ref(P, grads[s:e].cpu(), M, V, lr=lr, b1=b1, b2=b2, eps=eps, wd=wd if key[0] else 0.0,
                                 step=step, adamw=True, grad_mul=coef)
                got = (opt.master[mo:mo + n], opt.exp_avg[mo:mo + n], opt.exp_avg_sq[mo:mo + n])
                ex = N.adam_excess(got, ref, P)
                print(f"MixedPrecisionAdam step {step} piece [{s}:{e}] wd={key[0]}: error / bound "
                      + " ".join(f"{k}={x:.3f}" for k, x in ex.items()))
                assert max(ex.values()) <= 1.0, (step, s, e, ex)
                assert torch.equal(_bits(ddp.param_data[s:e]), _bits(opt.master[mo:mo + n].to(BF)))
                pad = ~live[s:e]
                for t in (opt.master[mo:mo + n], opt.exp_avg[mo:mo + n], opt.exp_avg_sq[mo:mo + n], ddp.param_data[s:e]):
                    assert bool((t[pad] == 0).all()), "alignment padding moved"
            assert opt.found_inf.item() == 0
        idx = int(live.nonzero()[100])
        ddp.grad_data[idx] = float("inf")
        keep = [t.clone() for t in (opt.master, opt.exp_avg, opt.exp_avg_sq, ddp.param_data)]
        opt.step()
        assert opt.found_inf.item() == 1
        for a, b in zip(keep, (opt.master, opt.exp_avg, opt.exp_avg_sq, ddp.param_data)):
            assert torch.equal(_bits(a), _bits(b)), "an overflow step changed the optimizer state"
    finally:
        ps.destroy_model_parallel()
