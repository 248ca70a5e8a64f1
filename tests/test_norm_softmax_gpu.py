"""layernorm.hip and softmax.hip at every row geometry they dispatch to, against the float64
references of tests/_numerics.py.

The norm picks G in {64, 256} threads per row and C in 1..8 register chunks per thread; its
backward is a software-pipelined grid-stride loop (512 blocks at most) whose dgamma / dbeta / dbias
partials live in registers across the rows of a group, and its forward loops past 2048 blocks. The
row counts below make a group own 2-3 rows with an uneven tail, so the prefetch of the next row,
the cross-row accumulation and the tail are all run. The softmax picks C in {1, 2, 4, 8} chunks
per lane and three mask modes. Every tolerance comes from the CPU emulations in
tests/test_numerics_sensitivity.py (4x the emulation's error), which also shows that each
criterion rejects a kernel with one term wrong.
"""
import math

import pytest
import torch

from smdt_amd.ops import _ext
from smdt_amd.ops import functional as SF

import _numerics as N

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 1e-5
BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32


def _C():
    return _ext.ext()


# ------------------------------------------------------------------------------------- norm

def _norm_fwd(c, rms, p=0.0, seed=0, offset=0):
    return _C().layernorm_fwd(c["x"], c.get("res"), c.get("bias"), c["gamma"], None if rms else c["beta"], EPS,
                              p, seed, offset, rms, True, None, c.get("x2"))


def _norm_bwd(c, s, mean, rstd, rms, p=0.0, seed=0, offset=0, acc=(None, None, None)):
    return _C().layernorm_bwd(c["dy"], c.get("ds_in"), s, c["gamma"], mean, rstd, p, seed, offset, rms, True,
                              "bias" in c, acc[0], acc[1], acc[2], None, c.get("dy2"))


def _check_norm(c, rms, what):
    """Forward and backward (p = 0) of one case against ``ln_ref``; prints every figure first."""
    T = c["x"].dtype
    rows, H = c["x"].shape
    y, s, mean, rstd = _norm_fwd(c, rms)
    # s is the fp32 sum in the kernel's order rounded once to T: equal, or one representable value
    # off where the compiler contracted a multiply-add
    s_ulp = N.ulp_distance(s, N.ln_s_emulation(c["x"], c.get("x2"), c.get("bias"), c.get("res")))
    ref = N.ln_ref(s, c["gamma"], c["beta"], c["dy"], EPS, rms, ds_in=c.get("ds_in"), dy2=c.get("dy2"))
    ds, dx, dg, db, dbi = _norm_bwd(c, s, mean, rstd, rms)
    assert dx.data_ptr() == ds.data_ptr()                       # without dropout dx IS ds
    e = {"y": N.row_rel_err(y, ref["y"]), "ds": N.row_rel_err(ds, ref["ds"]),
         "rstd": ((rstd.double() - ref["rstd"]).abs() / ref["rstd"]).max().item(),
         "dgamma": N.col_rel_err(dg, ref["dgamma"], ref["sg"])}
    if not rms:
        e["mean"] = ((mean.double() - ref["mean"]).abs() / s.double().abs().mean(-1)).max().item()
        e["dbeta"] = N.col_rel_err(db, ref["dbeta"], ref["sb"])
    else:
        assert db.numel() == 0
    if "bias" in c:
        e["dbias"] = N.col_rel_err(dbi, ref["dbias"], ref["sbi"])
    else:
        assert dbi.numel() == 0
    geo = N.ln_geometry(H, rows)
    print(f"norm {what} G={geo['G']} C={geo['C']} rows/group fwd {rows / geo['fwd_rstep']:.2f} bwd "
          f"{rows / geo['bwd_rstep']:.2f}: s_ulp={s_ulp} " + " ".join(f"{k}={v:.3g}" for k, v in e.items()))
    assert s_ulp <= 1, s_ulp
    for k, v in e.items():
        tol = N.LN_ELEM_TOL[T] if k in ("y", "ds") else (N.LN_STAT_TOL if k in ("mean", "rstd") else N.LN_COL_TOL)
        assert v <= tol, f"{what}: {k} error {v:.4g} > {tol:.4g}"


# (H, rows): one point per kernel shape, not the cross product
_SWEEP = [
    (8, 3),         # G 64, C 1, one lane live; fewer rows than groups in a block
    (512, 4101),    # G 64, C 1 full; backward: 2-3 rows per group, uneven tail
    (520, 1),       # G 64, C 2 with one chunk in the second pass; a single row
    (1536, 4101),   # G 64, C 3
    (2048, 8195),   # G 64, C 4 full (last H of the wave-per-row kernel); forward loop too
    (2056, 1029),   # G 256, C 2 (first H of the block-per-row kernel); backward: 2-3 rows per block
    (5120, 1029),   # G 256, C 3
    (12288, 1029),  # G 256, C 6
    (16384, 2051),  # G 256, C 8 full; forward loop at G 256
]
_TYPED = [(1536, 4101), (5120, 1029)]
_NORM_CASES = ([(H, r, BF, BF, "plain") for H, r in _SWEEP]
               + [(H, r, T, W, "plain") for H, r in _TYPED for T, W in ((BF, F32), (HF, HF), (HF, F32), (F32, F32))]
               + [(H, r, BF, BF, form) for H, r in _TYPED for form in ("fused", "summands")])


def _dt(t):
    return str(t).replace("torch.", "").replace("bfloat16", "bf16").replace("float16", "fp16").replace("float32", "fp32")


@pytest.mark.parametrize("rms", [False, True], ids=["layernorm", "rmsnorm"])
@pytest.mark.parametrize("H,rows,T,W,form", _NORM_CASES,
                         ids=[f"H{H}-r{r}-{_dt(T)}-w{_dt(W)}-{form}" for H, r, T, W, form in _NORM_CASES])
def test_norm_geometry(H, rows, T, W, form, rms):
    """plain: y = norm(x). fused: bias + residual in the forward, ds_in in the backward (p = 0).
    summands: the fused form plus the second summands x2 / dy2 a deferred reduce-scatter leaves."""
    c = N.ln_case(rows, H, T, W, fused=form != "plain", summands=form == "summands", device=DEV)
    _check_norm(c, rms, f"H={H} rows={rows} {_dt(T)}/{_dt(W)} {form} {'rms' if rms else 'ln'}")


def test_norm_pending_summand_through_autograd():
    """The forward summand through ``bias_dropout_add_norm`` (x._smdt_add, left by a deferred
    reduce-scatter) with 2-3 rows per group: it reaches the kernel, x's gradient is that of
    x + x2, and the parameter gradients come back in the parameters' dtype."""
    H, rows = 1536, 4101
    c = N.ln_case(rows, H, BF, BF, fused=True, summands=True, device=DEV)
    x, res = c["x"].clone().requires_grad_(), c["res"].clone().requires_grad_()
    g, be, bi = (c[k].clone().requires_grad_() for k in ("gamma", "beta", "bias"))
    x._smdt_add = c["x2"]
    y, s = SF.bias_dropout_add_norm(x, bi, res, g, be, 0.0, True, EPS, False)
    assert not hasattr(x, "_smdt_add")
    assert N.ulp_distance(s.detach(), N.ln_s_emulation(c["x"], c["x2"], c["bias"], c["res"])) <= 1
    ref = N.ln_ref(s.detach(), c["gamma"], c["beta"], c["dy"], EPS, False, ds_in=c["ds_in"])
    torch.autograd.backward([y, s], [c["dy"], c["ds_in"]])
    assert N.row_rel_err(y, ref["y"]) <= N.LN_ELEM_TOL[BF]
    assert N.row_rel_err(x.grad, ref["dx"]) <= N.LN_ELEM_TOL[BF]
    assert torch.equal(res.grad, x.grad)
    # the parameter gradients are the fp32 sums rounded once to bf16: 2^-8 of the value on top
    for p_, k, sc in ((g, "dgamma", "sg"), (be, "dbeta", "sb"), (bi, "dbias", "sbi")):
        assert p_.grad.dtype == BF
        err = (p_.grad.double() - ref[k]).abs()
        assert (err <= N.LN_COL_TOL * ref[sc] + 2.0 ** -8 * ref[k].abs()).all(), k


@pytest.mark.parametrize("H", [16392, 12])
def test_norm_rejects_unsupported_width(H):
    """H > 16384 or H % 8 != 0 has no kernel: the GPU path raises, it does not return a tensor."""
    x = torch.randn(4, H, device=DEV, dtype=BF)
    g, b = torch.ones(H, device=DEV, dtype=BF), torch.zeros(H, device=DEV, dtype=BF)
    with pytest.raises(RuntimeError, match="layernorm_fwd"):
        SF.bias_dropout_add_norm(x, None, None, g, b, 0.0, False, EPS, False)
    with pytest.raises(RuntimeError, match="layernorm_fwd"):
        _C().layernorm_fwd(x, None, None, g, None, EPS, 0.0, 0, 0, True, True, None, None)
    st = torch.ones(4, device=DEV)
    with pytest.raises(RuntimeError, match="layernorm_bwd"):
        _C().layernorm_bwd(x, None, x, g, st, st, 0.0, 0, 0, False, True, False, None, None, None, None, None)
    torch.cuda.synchronize()


@pytest.mark.parametrize("H,rows", _TYPED)
def test_norm_accumulate_into_main_grad(H, rows):
    """``dgamma_acc`` / ``dbeta_acc`` / ``dbias_acc`` prefilled with O(10) values: the result is
    prefill + reference under the column criterion (an overwrite is ~1e-2 away, see the sensitivity
    test); with only ``dgamma_acc`` given, dbeta and dbias are plain sums (the acc_mask bits)."""
    c = N.ln_case(rows, H, BF, BF, fused=True, device=DEV)
    y, s, mean, rstd = _norm_fwd(c, False)
    ref = N.ln_ref(s, c["gamma"], c["beta"], c["dy"], EPS, False, ds_in=c["ds_in"])
    gen = torch.Generator().manual_seed(4)
    pre = [(10 * torch.randn(H, generator=gen)).to(DEV) for _ in range(4)]
    acc = [p_.clone() for p_ in pre[:3]]
    _, _, dg, db, dbi = _norm_bwd(c, s, mean, rstd, False, acc=tuple(acc))
    assert dg.data_ptr() == acc[0].data_ptr() and db.data_ptr() == acc[1].data_ptr() and dbi.data_ptr() == acc[2].data_ptr()
    e = [N.col_rel_err(a, p_.double() + ref[k], ref[sc])
         for a, p_, (k, sc) in zip(acc, pre, (("dgamma", "sg"), ("dbeta", "sb"), ("dbias", "sbi")))]
    only = pre[3].clone()
    _, _, dg2, db2, dbi2 = _norm_bwd(c, s, mean, rstd, False, acc=(only, None, None))
    e += [N.col_rel_err(only, pre[3].double() + ref["dgamma"], ref["sg"]),
          N.col_rel_err(db2, ref["dbeta"], ref["sb"]), N.col_rel_err(dbi2, ref["dbias"], ref["sbi"])]
    print(f"norm accumulate H={H} rows={rows}: " + " ".join(f"{v:.3g}" for v in e))
    assert max(e) <= N.LN_COL_TOL, e


@pytest.mark.parametrize("H,rows", [(1024, 4101), (4096, 1029)])
def test_norm_dropout_across_the_loop(H, rows):
    """p = 0.1, residual 0, gamma 1, with 2-3 rows per group in the backward loop (G 64 and G 256).
    The keep mask is read off the forward's s; every bound is binomial (6 sigma) or one rounding."""
    p, seed, offset = 0.1, 1234, 7
    rate = math.floor(p * 65536 + 0.5) / 65536           # the realised drop rate: a 16-bit threshold
    ks = 1.0 / (1.0 - rate)
    c = N.ln_case(rows, H, BF, BF, device=DEV)
    c["gamma"] = torch.ones_like(c["gamma"])
    c["bias"] = torch.zeros_like(c["gamma"])
    c["res"] = torch.zeros_like(c["x"])
    y, s, mean, rstd = _norm_fwd(c, False, p, seed, offset)
    keep = s != 0
    n = keep.numel()
    frac = keep.float().mean().item()
    sig = math.sqrt(rate * (1 - rate) / n)
    print(f"dropout H={H} rows={rows}: keep fraction {frac:.6f} vs {1 - rate:.6f} (6 sigma = {6 * sig:.2g})")
    assert abs(frac - (1 - rate)) <= 6 * sig
    want_s = N.ln_s_emulation(c["x"], None, None, None, keep, 65536.0 / (65536.0 - rate * 65536))
    assert N.ulp_distance(s, want_s) <= 1                        # kept: x / (1 - rate) rounded once
    ref = N.ln_ref(s, c["gamma"], c["beta"], c["dy"], EPS, False, keep=keep, keep_scale=ks)
    ds, dx, dg, db, dbi = _norm_bwd(c, s, mean, rstd, False, p, seed, offset)
    assert dx.data_ptr() != ds.data_ptr()
    assert (dx[~keep] == 0).all()                                # exactly zero where s was dropped
    e = {"y": N.row_rel_err(y, ref["y"]), "ds": N.row_rel_err(ds, ref["ds"]), "dx": N.row_rel_err(dx, ref["dx"]),
         "dgamma": N.col_rel_err(dg, ref["dgamma"], ref["sg"]), "dbeta": N.col_rel_err(db, ref["dbeta"], ref["sb"]),
         "dbias": N.col_rel_err(dbi, ref["dbias"], ref["sbi"])}
    # dbias against the float64 column sum of the kernel's own (bf16-rounded) dx: each term carries
    # an independent rounding error, uniform within half a bf16 ulp (<= 2^-9 |dx|, std <= 2^-9 |dx| /
    # sqrt 3), so the sum of n of them stays within 6 sigma = 6 * 2^-9 / sqrt 3 * sqrt(sum dx^2)
    own = dx.double()
    allow = N.LN_COL_TOL * own.abs().sum(0) + 6 * 2.0 ** -9 / math.sqrt(3) * own.pow(2).sum(0).sqrt()
    own_err = ((dbi.double() - own.sum(0)).abs() / allow).max().item()
    # the masks of row r and of row r + rstep (same group, next loop iteration) are independent:
    # they agree on p^2 + (1 - p)^2 of the elements, nowhere near all of them
    rstep = N.ln_geometry(H, rows)["bwd_rstep"]
    assert 0 < rstep < rows
    kb = dx != 0
    q = rate * rate + (1 - rate) * (1 - rate)
    sig2 = math.sqrt(q * (1 - q) / ((rows - rstep) * H))
    agree_f = (keep[:-rstep] == keep[rstep:]).float().mean().item()
    agree_b = (kb[:-rstep] == kb[rstep:]).float().mean().item()
    print(f"  " + " ".join(f"{k}={v:.3g}" for k, v in e.items()) + f" own-dx dbias {own_err:.3g} of its bound; "
          f"rows r / r+{rstep} agree fwd {agree_f:.5f} bwd {agree_b:.5f} vs {q:.5f} (6 sigma = {6 * sig2:.2g})")
    for k, v in e.items():
        tol = N.LN_ELEM_TOL[BF] if k in ("y", "ds", "dx") else N.LN_COL_TOL
        assert v <= tol, f"{k} error {v:.4g} > {tol:.4g}"
    assert own_err <= 1
    assert (kb == keep).float().mean().item() >= 1 - 1e-6       # dx != 0 exactly where kept (ds == 0 aside)
    assert abs(agree_f - q) <= 6 * sig2 and abs(agree_b - q) <= 6 * sig2


# ---------------------------------------------------------------------------------- softmax

# (sk, sq): C = 1 with 1 lane live, C = 1 with 17 lanes, C = 2 with one lane in the second pass,
# C = 8 full, 1 * 3 * 7 = 21 rows (no multiple of a block's 4), C = 4 with its 4th pass idle. b = 1, np = 3: the
# inputs are exactly those the CPU emulation is run on (test_softmax_dtype_tolerances), because the
# criterion's floor is statistical for bf16: a causal row with two live keys can sit at a few
# per cent of its floor from the rounding of the stored y alone, whatever the kernel does.
_SM = [(8, 8), (136, 40), (520, 64), (4096, 64), (136, 7), (1536, 8)]
_SM_CASES = [(sk, sq, BF) for sk, sq in _SM] + [(sk, 64, T) for sk in (520, 4096) for T in (HF, F32)]


def _check_softmax(x, dy, causal, mask, what):
    T = x.dtype
    ty, tdx = N.SOFTMAX_TOLS[T]
    xg = x.clone().requires_grad_()
    y = SF.scaled_masked_softmax(xg, mask, 0.125, causal)
    yr, dxr = N.softmax_ref(x, dy, 0.125, causal, mask, dtype=torch.float64)
    y.backward(dy)
    ey = N.row_rel_err(y, yr)
    edx = N.row_rel_err(xg.grad, dxr, row_floor=N.softmax_grad_floor(yr, dy, 0.125, T))
    print(f"softmax {what}: y={ey:.3g} (tol {ty:.3g}) dx={edx:.3g} (tol {tdx:.3g})")
    assert y.dtype == T and torch.isfinite(y).all() and torch.isfinite(xg.grad).all()
    assert ey <= ty, f"{what}: y row-relative error {ey:.4g} > {ty:.4g}"
    assert edx <= tdx, f"{what}: dx row-relative error {edx:.4g} > {tdx:.4g}"
    if causal:
        i, j = torch.arange(x.shape[-2], device=DEV)[:, None], torch.arange(x.shape[-1], device=DEV)[None, :]
        assert (y[..., j > i] == 0).all() and (xg.grad[..., j > i] == 0).all()
    if mask is not None:
        assert (y[mask.expand_as(y)] == 0).all() and (xg.grad[mask.expand_as(y)] == 0).all()
    return y, xg.grad


# causal at C = 4 is test_kernels_gpu.test_scaled_masked_softmax's square sk = 2048 case: a causal
# [8, 1536] input has at most 8 live keys per row and says nothing about the later chunks
_SM_PARAMS = [(sk, sq, T, mode) for sk, sq, T in _SM_CASES for mode in (0, 1, 2) if not (sk == 1536 and mode == 1)]


@pytest.mark.parametrize("sk,sq,T,mode", _SM_PARAMS,
                         ids=[f"sk{sk}-sq{sq}-{_dt(T)}-{('nomask', 'causal', 'mask')[m]}" for sk, sq, T, m in _SM_PARAMS])
def test_softmax_geometry(sk, sq, T, mode):
    x, dy = N.softmax_case(sk, mode == 1, b=1, np_=3, sq=sq, dtype=T, device=DEV)
    mask = None
    if mode == 2:
        mask = (torch.rand(1, 1, sq, sk, generator=torch.Generator().manual_seed(1)) < 0.3).to(DEV)
    _check_softmax(x, dy, mode == 1, mask, f"sk={sk} sq={sq} {_dt(T)} mode={mode}")


def test_softmax_fully_masked_row():
    """One query row of batch 0 has every key masked: exact zeros and no NaN forward, exact zeros
    in dx, for every head; the other rows are unaffected."""
    sk, sq = 136, 40
    x, dy = N.softmax_case(sk, False, b=2, np_=3, sq=sq, device=DEV)
    mask = torch.rand(2, 1, sq, sk, generator=torch.Generator().manual_seed(2)) < 0.3
    mask[0, 0, 5] = True
    y, dx = _check_softmax(x, dy, False, mask.to(DEV), "fully masked row")
    assert (y[0, :, 5] == 0).all() and (dx[0, :, 5] == 0).all()
    assert (y[1, :, 5].float().sum(-1) - 1).abs().max() < 0.02


def test_softmax_mask_broadcast_over_batch():
    """A [1, 1, sq, sk] mask serves both batch entries."""
    sk, sq = 520, 64
    x, dy = N.softmax_case(sk, False, b=2, np_=3, sq=sq, device=DEV)
    mask = (torch.rand(1, 1, sq, sk, generator=torch.Generator().manual_seed(3)) < 0.3).to(DEV)
    _check_softmax(x, dy, False, mask, "broadcast mask")


@pytest.mark.parametrize("sk", [4104, 12])
def test_softmax_widths_without_a_kernel(sk):
    """sk > 4096 or sk % 8 != 0: ``scaled_masked_softmax`` takes its PyTorch path and still matches
    the reference in all three modes; the binding itself raises."""
    sq = 16
    for mode in (0, 1, 2):
        x, dy = N.softmax_case(sk, mode == 1, b=2, np_=2, sq=sq, device=DEV)
        mask = (torch.rand(2, 1, sq, sk, generator=torch.Generator().manual_seed(1)) < 0.3).to(DEV) if mode == 2 else None
        _check_softmax(x, dy, mode == 1, mask, f"sk={sk} torch path mode={mode}")
    with pytest.raises(RuntimeError, match="softmax_fwd"):
        _C().softmax_fwd(x, None, 0, 0.125)
    with pytest.raises(RuntimeError, match="softmax_bwd"):
        _C().softmax_bwd(dy, dy, 0, 0.125)
    torch.cuda.synchronize()


def test_causal_softmax_rectangular_kernel_equals_torch_path(monkeypatch):
    """causal with sq = 40 != sk = 136: the kernel and the PyTorch branch (the opt-out
    SMDT_DISABLE_KERNELS=1 takes it on the same tensors) mask the same elements, key j > query i,
    and give the same probabilities and gradients."""
    x, dy = N.softmax_case(136, True, b=1, np_=3, sq=40, device=DEV)
    yk, dxk = _check_softmax(x, dy, True, None, "causal 40x136 kernel")
    monkeypatch.setenv("SMDT_DISABLE_KERNELS", "1")
    with pytest.warns(UserWarning, match="SMDT_DISABLE_KERNELS"):
        yt, dxt = _check_softmax(x, dy, True, None, "causal 40x136 torch")
    monkeypatch.delenv("SMDT_DISABLE_KERNELS")
    assert torch.equal(yk == 0, yt == 0)
    assert N.row_rel_err(yk, yt.double()) <= N.SOFTMAX_TOL
    assert N.row_rel_err(dxk, dxt.double(), row_floor=N.softmax_grad_floor(yt, dy, 0.125)) <= N.SOFTMAX_TOL
