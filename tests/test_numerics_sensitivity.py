"""The kernel tests' criteria can fail (CPU twin of every mutation check).

For each numerics case used by ``test_kernels_gpu.py`` (cross entropy, padded-vocab CE, LM head +
CE, scaled / causal / masked softmax): an emulation of the kernel's rounding points passes the
row-relative criterion at the tolerance the GPU test uses, while a wrong implementation fails it:
softmax term dropped, softmax term x1.1, all-zero output, all-zero gradient, or a gradient that
is zero beyond row 64.
"""
import pytest
import torch

import _numerics as N
from _numerics import (CE_TOL, SOFTMAX_TOL, ce_case, ce_kernel_emulation, ce_ref, lmce_case,
                       lmce_kernel_emulation, lmce_ref, row_rel_err, softmax_case, softmax_grad_floor,
                       softmax_ref)


@pytest.mark.parametrize("V,vocab", [(50304, 0), (1000, 0), (1024, 1017)])
def test_ce_criterion_rejects_mutations(V, vocab):
    logits, tgt, dl = ce_case(300 if V > 2000 else 200, V, vocab)
    _, good = ce_ref(logits, tgt, dl, vocab)
    _, emu = ce_kernel_emulation(logits, tgt, dl, vocab)
    assert row_rel_err(emu, good) <= CE_TOL / 3
    for soft in (0.0, 1.1, 0.9):
        _, bad = ce_ref(logits, tgt, dl, vocab, soft=soft)
        assert row_rel_err(bad, good) > 2 * CE_TOL, soft


@pytest.mark.parametrize("V,vocab", [(50304, 50257), (1000, 0)])
def test_lm_head_ce_criterion_rejects_mutations(V, vocab):
    h, w, tgt, dl = lmce_case(s=48, b=3, V=V, vocab=vocab)
    lg = (h.float().reshape(-1, h.shape[-1]) @ w.float().t()).bfloat16()
    loss, dh, dw = lmce_ref(h, w, lg, tgt, dl, vocab)
    eloss, edh, edw = lmce_kernel_emulation(h, w, lg, tgt, dl, vocab)
    assert (eloss - loss).abs().max().item() < 1e-3
    assert row_rel_err(edh, dh) <= CE_TOL / 3, row_rel_err(edh, dh)
    assert row_rel_err(edw, dw) <= CE_TOL / 3, row_rel_err(edw, dw)
    for soft in (0.0, 1.1):
        _, bdh, bdw = lmce_ref(h, w, lg, tgt, dl, vocab, soft=soft)
        assert row_rel_err(bdh, dh) > 2 * CE_TOL, (soft, row_rel_err(bdh, dh))
        assert row_rel_err(bdw, dw) > 2 * CE_TOL, (soft, row_rel_err(bdw, dw))


@pytest.mark.parametrize("sk", [128, 1024])
@pytest.mark.parametrize("causal", [True, False])
def test_softmax_criterion_rejects_mutations(sk, causal):
    x, dy = softmax_case(sk, causal, b=1, np_=2)
    y, dx = softmax_ref(x, dy, 0.125, causal)
    # kernel emulation: y stored 16-bit, dx = scale * y (dy - sum(dy y)) from the 16-bit y, stored 16-bit
    yb = y.bfloat16().float()
    dxe = (0.125 * yb * (dy.float() - (dy.float() * yb).sum(-1, keepdim=True))).bfloat16()
    assert row_rel_err(yb, y) <= SOFTMAX_TOL / 3
    fl = softmax_grad_floor(y, dy, 0.125)
    assert row_rel_err(dxe, dx, row_floor=fl) <= SOFTMAX_TOL / 3, row_rel_err(dxe, dx, row_floor=fl)
    assert row_rel_err(torch.zeros_like(y), y) > 2 * SOFTMAX_TOL
    assert row_rel_err(torch.zeros_like(dx), dx, row_floor=fl) > 2 * SOFTMAX_TOL
    assert row_rel_err(1.1 * dx, dx, row_floor=fl) > 2 * SOFTMAX_TOL
    cut = dx.clone()
    cut[..., 64:, :] = 0
    assert row_rel_err(cut, dx, row_floor=fl) > 2 * SOFTMAX_TOL


def test_masked_softmax_criterion_rejects_mutations():
    g = torch.Generator().manual_seed(6)
    x = (8 * torch.randn(2, 3, 64, 256, generator=g)).bfloat16()
    mask = torch.rand(2, 1, 64, 256, generator=g) < 0.3
    dy = torch.randn(2, 3, 64, 256, generator=g).bfloat16()
    y, dx = softmax_ref(x, dy, 0.125, False, mask)
    assert row_rel_err(y.bfloat16(), y) <= SOFTMAX_TOL / 3
    unmasked = torch.softmax(x.float() * 0.125, -1)
    assert row_rel_err(unmasked, y) > 2 * SOFTMAX_TOL
    assert row_rel_err(1.1 * dx, dx, row_floor=softmax_grad_floor(y, dy, 0.125)) > 2 * SOFTMAX_TOL


@pytest.mark.parametrize("V,vocab", [(50304, 50257), (1024, 0)])
def test_vocab_parallel_lm_head_ce_math_cpu(V, vocab):
    """CPU twin of test_kernels_gpu.test_vocab_parallel_lm_head_ce_two_shards: the two-shard math
    (local pass, combined statistics, one-hot at one element, hidden-side scale) equals the fp32
    reference on the same 16-bit logits within the criterion, and the same math with the
    softmax term mutated would not."""
    h, w, tgt, dl = lmce_case(s=32, b=3, V=V, vocab=vocab)
    from _numerics import vp_lmce_two_shards
    loss, dh, dw, lg = vp_lmce_two_shards(h, w, tgt, dl, vocab)
    rl, rdh, rdw = lmce_ref(h, w, lg, tgt, dl, vocab)
    assert (loss - rl).abs().max().item() < 1e-3
    assert row_rel_err(dh, rdh) <= CE_TOL / 3, row_rel_err(dh, rdh)
    assert row_rel_err(dw, rdw) <= CE_TOL / 3, row_rel_err(dw, rdw)
    _, bdh, bdw = lmce_ref(h, w, lg, tgt, dl, vocab, soft=1.1)
    assert row_rel_err(bdh, rdh) > 2 * CE_TOL and row_rel_err(bdw, rdw) > 2 * CE_TOL


# ------------------------------------------------------------------ fused norm (layernorm.hip)

def _ln_inputs(rows, H, dtype, rms, form, seed=21):
    """The case, the 16-bit s the kernel would store, and the keyword arguments shared by
    ``ln_ref`` and ``ln_kernel_emulation``. form: plain | fused (bias, residual, ds_in, x2, dy2) |
    drop (bias, residual, ds_in and a p = 0.1 keep mask)."""
    c = N.ln_case(rows, H, dtype, torch.float32 if dtype == torch.float16 else None,
                  fused=form != "plain", summands=form == "fused", seed=seed)
    keep, ks = None, 1.0
    if form == "drop":
        keep = torch.rand(rows, H, generator=torch.Generator().manual_seed(3)) >= 0.1
        ks = 1 / 0.9
    s = N.ln_s_emulation(c["x"], c.get("x2"), c.get("bias"), c.get("res"), keep, ks)
    return c, s, dict(keep=keep, keep_scale=ks, ds_in=c.get("ds_in"), dy2=c.get("dy2"))


def _ln_errors(out, ref):
    e = {k: N.row_rel_err(out[k], ref[k]) for k in ("y", "ds", "dx") if k in out}
    e.update({k: N.col_rel_err(out[k], ref[k], ref[sc])
              for k, sc in (("dgamma", "sg"), ("dbeta", "sb"), ("dbias", "sbi")) if k in out})
    return e


@pytest.mark.parametrize("rows,H", [(4101, 512), (4101, 1536), (1029, 5120), (2300, 64), (3, 8)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_ln_emulation_within_a_quarter_of_the_tolerances(rows, H, dtype):
    """The measurement the LN_* tolerances are sized from (4x the largest value seen here, see the
    comment beside them in _numerics.py): the kernel's rounding points against the float64
    reference, under every criterion the GPU tests use."""
    for rms in (False, True):
        for form in ("plain", "fused", "drop"):
            c, s, kw = _ln_inputs(rows, H, dtype, rms, form)
            ref = N.ln_ref(s, c["gamma"], c["beta"], c["dy"], 1e-5, rms, **kw)
            emu = N.ln_kernel_emulation(s, c["gamma"], c["beta"], c["dy"], 1e-5, rms, **kw)
            e = _ln_errors(emu, ref)
            e["mean"] = ((emu["mean"].double() - ref["mean"]).abs() / s.double().abs().mean(-1)).max().item()
            e["rstd"] = ((emu["rstd"].double() - ref["rstd"]).abs() / ref["rstd"]).max().item()
            print(f"ln emulation {dtype} {rows}x{H} rms={rms} {form}: " + " ".join(f"{k}={v:.3g}" for k, v in e.items()))
            for k in ("y", "ds", "dx"):
                assert e[k] <= N.LN_ELEM_TOL[dtype] / 4 * 1.01, (rms, form, k, e[k])
            for k in ("dgamma", "dbeta", "dbias"):
                assert e[k] <= N.LN_COL_TOL / 4 * 1.01, (rms, form, k, e[k])
            assert e["mean"] <= N.LN_STAT_TOL / 4 * 1.01 and e["rstd"] <= N.LN_STAT_TOL / 4 * 1.01, (rms, form, e)


# mutation -> (rows, H, the outputs whose criterion must reject it). m2 / (H + 8) differs from
# m2 / H by 8 / (H + 8): at H = 512 that is 1.5 % of one term of ds, below ten bf16 tolerances by
# arithmetic, so it is shown at H = 8 (the sweep's smallest row), where the term is halved.
_LN_MUT = {"no_m1": (4101, 512, ("ds", "dx")), "m2_h_plus_8": (2300, 8, ("ds", "dx")),
           "dgamma_first_pass": (4101, 512, ("dgamma",)), "dbeta_no_last_row": (4101, 512, ("dbeta",)),
           "stale_rstd": (4101, 512, ("ds", "dx")), "dx_unmasked": (4101, 512, ("dx", "dbias"))}


@pytest.mark.parametrize("mutation", N.LN_MUTATIONS)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_ln_criteria_reject_mutations(mutation, dtype):
    """Each mutation of ``ln_ref`` (one term of the backward wrong) is at least 10 tolerances away
    from the true reference under the criterion of every output it touches, while the emulation of
    the kernel passes the same criterion on the same inputs."""
    rows, H, outs = _LN_MUT[mutation]
    rstep = N.ln_geometry(H, rows)["bwd_rstep"]
    for rms in (False, True):
        if rms and mutation == "no_m1":
            continue                        # RMSNorm has no m1 term
        c, s, kw = _ln_inputs(rows, H, dtype, rms, "drop")
        ref = N.ln_ref(s, c["gamma"], c["beta"], c["dy"], 1e-5, rms, **kw)
        emu = _ln_errors(N.ln_kernel_emulation(s, c["gamma"], c["beta"], c["dy"], 1e-5, rms, **kw), ref)
        bad = _ln_errors(N.ln_ref(s, c["gamma"], c["beta"], c["dy"], 1e-5, rms, mutate=mutation, rstep=rstep, **kw), ref)
        print(f"ln mutation {mutation} {dtype} rms={rms}: " + " ".join(f"{k}={bad[k]:.3g}" for k in outs))
        for k in outs:
            tol = N.LN_ELEM_TOL[dtype] if k in ("y", "ds", "dx") else N.LN_COL_TOL
            assert emu[k] <= tol, (k, emu[k])
            assert bad[k] >= 10 * tol, (rms, k, bad[k], tol)


def test_ln_accumulate_criterion_rejects_overwrite():
    """The accumulate form (``dgamma_acc`` = an fp32 main_grad with O(10) content): prefill + the
    emulation's sum passes the column criterion against prefill + reference; a kernel that
    overwrote the buffer is >= 10 tolerances away."""
    c, s, kw = _ln_inputs(4101, 512, torch.bfloat16, False, "fused")
    ref = N.ln_ref(s, c["gamma"], c["beta"], c["dy"], 1e-5, False, **kw)
    emu = N.ln_kernel_emulation(s, c["gamma"], c["beta"], c["dy"], 1e-5, False, **kw)
    pre = 10 * torch.randn(512, generator=torch.Generator().manual_seed(4))
    for k, sc in (("dgamma", "sg"), ("dbeta", "sb"), ("dbias", "sbi")):
        want = pre.double() + ref[k]
        assert N.col_rel_err(pre + emu[k], want, ref[sc]) <= N.LN_COL_TOL
        e = N.col_rel_err(emu[k], want, ref[sc])
        print(f"ln accumulate overwritten {k}: {e:.3g}")
        assert e >= 10 * N.LN_COL_TOL


def test_ln_s_check_is_one_rounding():
    """``ulp_distance``: equal tensors 0, neighbours 1, across zero 2 (+-tiny), and a s rounded
    twice (fp32 -> fp16-precision -> bf16) or scaled by 1 + 2^-6 is farther than the 1 ulp the GPU
    test allows."""
    a = torch.tensor([1.0, -1.0, 3.0], dtype=torch.bfloat16)
    assert N.ulp_distance(a, a.clone()) == 0
    assert N.ulp_distance(a, torch.tensor([1.0078125, -1.0, 3.0], dtype=torch.bfloat16)) == 1
    c = N.ln_case(64, 512, fused=True)
    s = N.ln_s_emulation(c["x"], None, c["bias"], c["res"])
    assert N.ulp_distance(s, (s.float() * (1 + 2.0 ** -6)).bfloat16()) > 1
    assert N.ulp_distance(s, N.ln_s_emulation(c["x"], None, None, c["res"])) > 1     # bias forgotten


# ---------------------------------------------------------- softmax in fp16 / fp32 and the edges

_SM_CASES = [(8, 8), (136, 40), (520, 64), (4096, 64), (136, 7), (1536, 8)]


@pytest.mark.parametrize("sk,sq", _SM_CASES)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_softmax_dtype_tolerances(sk, sq, dtype):
    """The measurement SOFTMAX_TOLS is sized from, on the very inputs test_norm_softmax_gpu.py
    gives the kernel (b = 1, np = 3): the emulation of softmax.hip's rounding points in each dtype
    against the float64 reference stays within a quarter of the fp16 / fp32 tolerances in all three
    mask modes, and within 0.6 of bf16's SOFTMAX_TOL (fixed at 0.03 earlier; the bf16 emulation
    reaches 0.016 on a causal row with few live keys, where the row is judged against its floor);
    an all-zero output, dx x 1.1 and an unmasked forward are rejected."""
    ty, tdx = N.SOFTMAX_TOLS[dtype]
    for mode in (0, 1, 2):
        if sk == 1536 and mode == 1:
            continue            # not a GPU case: causal C = 4 is the square sk = 2048 test
        x, dy = N.softmax_case(sk, mode == 1, b=1, np_=3, sq=sq, dtype=dtype)
        mask = None
        if mode == 2:
            mask = torch.rand(1, 1, sq, sk, generator=torch.Generator().manual_seed(1)) < 0.3
        y, dx = N.softmax_ref(x, dy, 0.125, mode == 1, mask, dtype=torch.float64)
        ye, dxe = N.softmax_kernel_emulation(x, dy, 0.125, mode == 1, mask)
        fl = N.softmax_grad_floor(y, dy, 0.125, dtype)
        ey, edx = N.row_rel_err(ye, y), N.row_rel_err(dxe, dx, row_floor=fl)
        print(f"softmax emulation {dtype} sk={sk} sq={sq} mode={mode}: y={ey:.3g} dx={edx:.3g}")
        frac = 0.6 if dtype == torch.bfloat16 else 0.2525
        assert ey <= ty * frac and edx <= tdx * frac, (mode, ey, edx)
        assert N.row_rel_err(torch.zeros_like(y), y) > 2 * ty
        assert N.row_rel_err(torch.zeros_like(dx), dx, row_floor=fl) > 2 * tdx
        assert N.row_rel_err(1.1 * dx, dx, row_floor=fl) > 2 * tdx
        if mode:
            assert N.row_rel_err(torch.softmax(x.double() * 0.125, -1), y) > 2 * ty


def test_softmax_ref_fully_masked_row_is_zero():
    x, dy = N.softmax_case(136, False, b=1, np_=2, sq=5)
    mask = torch.zeros(1, 1, 5, 136, dtype=torch.bool)
    mask[0, 0, 3] = True
    y, dx = N.softmax_ref(x, dy, 0.125, False, mask, dtype=torch.float64)
    assert torch.isfinite(y).all() and torch.isfinite(dx).all()
    assert (y[:, :, 3] == 0).all() and (dx[:, :, 3] == 0).all() and (y[:, :, 2].sum(-1) - 1).abs().max() < 1e-12
    ye, dxe = N.softmax_kernel_emulation(x, dy, 0.125, False, mask)
    assert (ye[:, :, 3] == 0).all() and (dxe[:, :, 3] == 0).all()


def test_causal_softmax_rectangular_is_top_left_aligned():
    """``scaled_masked_softmax(causal=True)`` with sq != sk masks key j > query i (what the kernel
    and the docstring say), not j > i + sk - sq: the PyTorch path at sq = 40, sk = 136 equals the
    reference's ``triu(1)`` mask and differs from the bottom-right form by a whole probability."""
    from smdt_amd.ops import functional as SF
    x, dy = N.softmax_case(136, True, b=1, np_=3, sq=40)
    y = SF.scaled_masked_softmax(x, None, 0.125, causal=True)
    yr, _ = N.softmax_ref(x, dy, 0.125, True, dtype=torch.float64)
    assert N.row_rel_err(y, yr) <= N.SOFTMAX_TOL
    assert (y[..., 0, 0] == 1).all() and (y[..., 0, 1:] == 0).all()          # query 0 sees key 0 only
    i, j = torch.arange(40)[:, None], torch.arange(136)[None, :]
    assert (y[..., j > i] == 0).all() and (y[..., 39, :40] > 0).any()
    br = torch.softmax((x.double() * 0.125).masked_fill(j > i + 96, float("-inf")), -1)
    assert N.row_rel_err(br, yr) > 0.5


# ------------------------------------------------------------------------------------------
# Flash attention forward: the lazy reference max and its rescue (CPU twin of fwd_kernel).

def _flash_twin_excess(profile, dtype, window, causal, **kw):
    """max over (o, lse) of twin error / bound (``N.flash_excess``: 2 x the emulation's error + one
    ulp at the row max) on one profile; B 1, S 256 (4 key tiles, 2 query blocks), GQA 2 : 1, D 64."""
    doc = kw.pop("doc_start", None)
    q, k, v, do = N.flash_score_case(profile, B=1, S=256, H=2, Hkv=1, D=64, dtype=dtype)
    ref = N.flash_ref(q, k, v, do, N.FLASH_SCALE, causal, doc_start=doc)
    emu = N.flash_kernel_emulation(q, k, v, do, N.FLASH_SCALE, causal, doc_start=doc)
    o, lse = N.flash_lazy_max_twin(q, k, v, N.FLASH_SCALE, causal, dtype, window, doc_start=doc, **kw)
    return max(N.flash_excess(o, emu["o"], ref["o"], dtype)[0], N.flash_excess(lse, emu["lse"], ref["lse"], dtype)[0]), o


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("profile", sorted(N.FLASH_PROFILES))
def test_flash_twin_matches_float64(profile, causal):
    """fwd_kernel's tile-by-tile algorithm (bf16, window [2^-64, 2^64], the guarded alpha) is within
    the GPU tests' bound of float64 attention on every score profile (measured: 0.56 - 0.60 of the
    bound for o, 0.04 - 0.32 for lse)."""
    e, _ = _flash_twin_excess(profile, torch.bfloat16, N.FLASH_WINDOWS[torch.bfloat16], causal)
    assert e <= 1.0, e


# mutation -> (profile, causal) that must reject it; measured twin error / bound in the comment
_FLASH_CATCH = {
    "no_o_rescale": ("up_late", False),            # o 2585x
    "no_l_rescale": ("up_late", False),            # o 117x, lse 4.3x
    "lse_without_m": ("low_start", False),         # lse 252x
    "rescue_ignores_mask": ("low_start", True),    # o 176x, lse 898x (causal only: the mask is the diagonal's)
    "select_all_lanes": ("opposed", False),        # NaN: the falling lanes' l * exp2(+144) overflows
}


@pytest.mark.parametrize("mutate", N.FLASH_MUTATIONS)
def test_flash_criterion_rejects_rescue_mutations(mutate):
    """Every step of the rescue is visible to the criterion: the twin with one step broken exceeds
    the bound on the profile named in ``_FLASH_CATCH`` (factors there), and stays inside it on
    ``plain``, which never rescues — randn-like scores cannot see any of these."""
    prof, causal = _FLASH_CATCH[mutate]
    e, _ = _flash_twin_excess(prof, torch.bfloat16, (-64, 64), causal, mutate=mutate)
    assert not e <= 4.0, (mutate, e)
    e, _ = _flash_twin_excess("plain", torch.bfloat16, (-64, 64), causal, mutate=mutate)
    assert e <= 1.0, (mutate, e)


def test_flash_select_all_lanes_breaks_dead_doc_rows():
    """DOC: a wave whose rows 0..15 ask for a downward rescue on a tile where rows 16..31 (a later
    document) are dead: d = tmax = -inf for the dead lanes is NaN, d = bad ? tmax : 0 is not."""
    ds = torch.zeros(1, 256, dtype=torch.int32)
    ds[:, 80:] = 80
    e, _ = _flash_twin_excess("low_start", torch.bfloat16, (-64, 64), True, doc_start=ds)
    assert e <= 1.0, e
    e, _ = _flash_twin_excess("low_start", torch.bfloat16, (-64, 64), True, doc_start=ds, mutate="select_all_lanes")
    assert not e <= 4.0, e


@pytest.mark.parametrize("causal", [True, False])
def test_flash_fp16_needs_its_own_window(causal):
    """Why fwd_kernel's window depends on the type. With the window bf16 uses, [2^-64, 2^64], the
    fp16 twin overflows p to inf on ``fp16_high`` (natural score 20 -> p = 2^29 > 65504) and on
    ``low_start`` (after the move to -60 the -30 tiles give 2^43), and flushes every p to zero on
    ``fp16_low`` (p = 2^-36: O = 0 while l counts them). A lower bound of 2^-14 that only keeps p
    non-zero leaves ``fp16_subnormal`` ~16x over the bound (2^-24: ~44x). With [2^0, 2^15] every
    profile passes."""
    old = N.FLASH_WINDOW_PARENT
    e, o = _flash_twin_excess("fp16_high", torch.float16, old, causal)
    assert not torch.isfinite(o.float()).all() and not e <= 1.0
    e, o = _flash_twin_excess("low_start", torch.float16, old, causal)
    assert not torch.isfinite(o.float()).all()
    e, o = _flash_twin_excess("fp16_low", torch.float16, old, causal)
    assert (o[:, 1::2].float() == 0).all() and e > 100, e       # the rows with qa = 16: all zero
    for lo in (-24, -14):
        e, _ = _flash_twin_excess("fp16_subnormal", torch.float16, (lo, 15), causal)
        assert e > 4.0, (lo, e)
    assert N.FLASH_WINDOWS[torch.float16] == (0, 15)
    for prof in N.FLASH_PROFILES:
        e, _ = _flash_twin_excess(prof, torch.float16, N.FLASH_WINDOWS[torch.float16], causal)
        assert e <= 1.0, (prof, e)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("profile", ["very_low", "very_low_first"])
def test_flash_downward_rescue_needs_alpha_guard(profile, dtype):
    """A first tile whose row max is below 2^-128 (natural score -100): alpha = exp2(-tmax) = inf,
    and l = 0 * inf = NaN with the unguarded rescale; alpha = 1 where l == 0 gives the reference."""
    w = N.FLASH_WINDOWS[dtype]
    e, o = _flash_twin_excess(profile, dtype, w, False, alpha_guard=False)
    assert torch.isnan(o[:, 1::2].float()).all() and not e <= 1.0
    e, o = _flash_twin_excess(profile, dtype, w, False)
    assert e <= 1.0, e


@pytest.mark.parametrize("profile,dtype,causal", [("plain", torch.bfloat16, True), ("up_late", torch.bfloat16, True),
                                                  ("very_low", torch.bfloat16, False), ("very_low", torch.bfloat16, True),
                                                  ("very_low", torch.float16, False)])
def test_flash_criterion_rejects_wrong_gradient_rows(profile, dtype, causal):
    """The gradients' criterion (per-row emulation error, one ulp, ``flash_grad_floors``) can fail,
    row by row. The emulation at the kernel's reference max stands in for the kernel (0.33 - 0.5 of
    the bound against itself); all-zero, x2, x1.25 and ONE zeroed row (37 or 200) of dq, dk and dv
    are rejected. Measured worst error / bound, bf16: ``plain`` causal zero 79 - 101, x1.25 33 -
    48, one row 21 - 54; ``up_late`` causal zero 83 - 93, one row 22 - 54; ``very_low`` dq zero
    2.9 - 7.7, one row 1.7 - 2.9. bf16 dk / dv on ``very_low`` are the weak spot: the dK / dV kernel
    prescales K where the forward prescales Q, at |score| ~ 100 its P is off by up to 2^0.5, the
    emulation's own row error is 0.3 - 0.5, and the factor 2 leaves zero 2.4 - 4.8, one row 1.08 -
    1.5 (fp16: zero 22 - 127, one row 21 - 60); x1.25 is not asked there (0.7 - 1.0 of the bound: on
    the reserved channel, |k| = 50, the rounding floor of the cancelling dS sum is that large).
    The emulation with a true row max (no lazy-max rounding of P) misses the bound on causal dq of
    ``plain`` and ``up_late`` (1.4 - 2x): that rounding point is part of the kernel."""
    q, k, v, do = N.flash_score_case(profile, B=1, S=256, H=2, Hkv=1, D=64, dtype=dtype)
    ref = N.flash_ref(q, k, v, do, N.FLASH_SCALE, causal)
    emu = N.flash_emulation_at_kernel_max(q, k, v, do, N.FLASH_SCALE, causal)
    fl = N.flash_grad_floors(q, k, v, do, N.FLASH_SCALE, causal)
    for n in ("dq", "dk", "dv"):
        g = emu[n]
        ex = lambda t: N.flash_excess(t, emu[n], ref[n], dtype, fl[n])[0]
        assert ex(g) <= 0.5 + 1e-9, (n, ex(g))
        muts = [("zero", torch.zeros_like(g)), ("x2", 2 * g)]
        if profile != "very_low":
            muts.append(("x1.25", 1.25 * g.float()))
        for what, bad in muts:
            assert ex(bad) > 1.0, (n, what, ex(bad))
        for r in (37, 200):
            z = g.clone()
            z[0, r, 0] = 0
            assert ex(z) > 1.0, (n, r, ex(z))
    if profile != "very_low":
        true_max = N.flash_kernel_emulation(q, k, v, do, N.FLASH_SCALE, causal)
        assert N.flash_excess(true_max["dq"], emu["dq"], ref["dq"], dtype, fl["dq"])[0] > 1.0
