"""Shared numerics for the kernel tests: inputs that make every term of a gradient visible, a
row-relative error criterion, and fp32 references with a knob that mutates the softmax term.

The GPU tests (``test_kernels_gpu.py``) judge the HIP kernels against these references; the CPU
test ``test_numerics_sensitivity.py`` proves each criterion can fail: an emulation of the kernel's
16-bit rounding points passes it, while the same reference with the softmax term dropped
(``soft=0``) or scaled by 1.1 (``soft=1.1``), an all-zero output, or a gradient zeroed past row 64
is rejected. A check that a wrong kernel can pass is no check.
"""
import torch

# Row-relative tolerances used by the GPU tests (sized from the CPU sensitivity test: the bf16
# emulations land at <= 0.8 % of the row max, every mutation at >= 6 %).
CE_TOL = 0.03
SOFTMAX_TOL = 0.03

# Row-relative tolerances (y, dx) of the softmax kernels per dtype. bf16 keeps SOFTMAX_TOL; fp16 and
# fp32 are 4x the largest error of ``softmax_kernel_emulation`` against the float64 reference over
# sk 8 / 136 / 520 / 4096 and the three mask modes (test_numerics_sensitivity.py measures them:
# fp16 y 4.8e-4, dx 8.4e-3 (a causal row judged against its floor); fp32 y 2.2e-7, dx 7.7e-6).
SOFTMAX_TOLS = {torch.bfloat16: (SOFTMAX_TOL, SOFTMAX_TOL), torch.float16: (1.9e-3, 3.4e-2),
                torch.float32: (8.8e-7, 3.1e-5)}

# Fused norm. Each tolerance is 4x the largest error of ``ln_kernel_emulation`` against ``ln_ref``
# measured by test_numerics_sensitivity.py over rows x H = 4101 x 512, 4101 x 1536, 1029 x 5120,
# 2300 x 64 and 3 x 8, LayerNorm and RMSNorm, plain / fused / dropout forms:
#   y, ds, dx (row-relative): bf16 3.9e-3 (one rounding, 2^-8 of a row max just above a power of
#     two), fp16 4.9e-4 (2^-11), fp32 8.6e-7 (fp32 arithmetic on rows with |mean| >> std);
#   dgamma, dbeta, dbias (per column, relative to the sum over rows of |term|): 3.1e-7 (3 rows),
#     <= 5e-8 at >= 1000 rows;
#   mean (relative to the row's mean |s|) 1.8e-7, rstd (relative) 1.9e-7.
LN_ELEM_TOL = {torch.bfloat16: 2.0 ** -6, torch.float16: 2.0 ** -9, torch.float32: 3.5e-6}
LN_COL_TOL = 1.25e-6
LN_STAT_TOL = 7.5e-7


def row_rel_err(out, ref, floor_frac: float = 1e-4, row_floor=None) -> float:
    """max over rows of max|out - ref| / max|ref| (rows = every index but the last). Rows whose
    reference is ~0 are judged against ``floor_frac`` of the global max instead; ``row_floor``
    (one value per row) raises a row's denominator to the error its 16-bit inputs alone imply.
    A float64 reference is compared in float64 (fp32 kernels are judged at fp32 accuracy)."""
    wd = torch.float64 if ref.dtype == torch.float64 else torch.float32
    o = out.detach().to(wd).reshape(-1, out.shape[-1])
    r = ref.detach().to(wd).reshape(-1, ref.shape[-1]).to(o.device)
    den = r.abs().amax(-1).clamp_min(floor_frac * r.abs().max().clamp_min(1e-30))
    if row_floor is not None:
        den = torch.maximum(den, row_floor.detach().to(wd).reshape(-1).to(o.device))
    return ((o - r).abs().amax(-1) / den).max().item()


def softmax_grad_floor(y, dy, scale, dtype=torch.bfloat16):
    """Per-row magnitude of the error a y stored in ``dtype`` alone puts into
    scale * y (dy - sum(dy y)): a few roundings (2 eps: 2^-6 for bf16, 2^-9 for fp16, 2^-22 for
    fp32) * scale * max|dy| * max y (y_i + y_j != 1 after rounding). Rows of a peaked softmax
    cancel down to that level."""
    return 2.0 * torch.finfo(dtype).eps * scale * dy.float().abs().amax(-1) * y.float().amax(-1)


def assert_rows_close(out, ref, tol, what="", row_floor=None):
    e = row_rel_err(out, ref, row_floor=row_floor)
    assert e <= tol, f"{what}: row-relative error {e:.4g} > {tol}"


# ------------------------------------------------------------------------------ cross entropy

def ce_case(N, V, vocab=0, device="cpu", seed=9, scale=8.0):
    """Peaked bf16 logits (std ``scale``) so softmax mass sits on a few columns; half the targets
    are the row's argmax, half are random columns (the softmax term then dominates), one row is
    ignored (-100). O(1) signed per-row dloss."""
    g = torch.Generator().manual_seed(seed)
    nv = vocab or V
    logits = (scale * torch.randn(N, V, generator=g)).bfloat16()
    tgt = torch.randint(0, nv, (N,), generator=g)
    am = logits[:, :nv].float().argmax(-1)
    tgt[::2] = am[::2]
    tgt[5] = -100
    dl = torch.randn(N, generator=g)
    return logits.to(device), tgt.to(device), dl.to(device)


def ce_ref(logits, tgt, dl, vocab=0, soft=1.0):
    """fp32 per-token CE loss and d(sum dl * loss)/dlogits with the softmax term scaled by
    ``soft`` (1 = correct). Columns >= vocab (if > 0) are padding: no mass, zero gradient."""
    z = logits.float()
    V = z.shape[-1]
    nv = vocab or V
    zz = z[:, :nv]
    lse = torch.logsumexp(zz, -1)
    valid = tgt >= 0
    t = tgt.clamp_min(0)
    loss = torch.where(valid, lse - zz.gather(1, t[:, None])[:, 0], torch.zeros_like(lse))
    p = torch.softmax(zz, -1)
    grad = torch.zeros_like(z)
    grad[:, :nv] = soft * p
    grad[torch.arange(z.shape[0], device=z.device), t] -= 1.0
    grad = grad * (dl * valid)[:, None]
    return loss, grad


def ce_kernel_emulation(logits, tgt, dl, vocab=0):
    """The CE kernels' rounding: fp32 math, dlogits stored in the logits' 16-bit type."""
    loss, grad = ce_ref(logits, tgt, dl, vocab)
    return loss, grad.to(logits.dtype)


# ---------------------------------------------------------------------- LM head + CE (TP = 1)

def lmce_case(s=96, b=3, H=256, V=50304, vocab=0, device="cpu", seed=12):
    """h ~ N(0, 1), W ~ N(0, 0.25^2): logits with std ~4 (peaked); targets half argmax, half
    random, one ignored; O(1) signed dloss."""
    g = torch.Generator().manual_seed(seed)
    nv = vocab or V
    h = torch.randn(s, b, H, generator=g).bfloat16()
    w = (0.25 * torch.randn(V, H, generator=g)).bfloat16()
    lg = (h.float().reshape(-1, H) @ w.float().t())[:, :nv]
    tgt = torch.randint(0, nv, (s * b,), generator=g)
    tgt[::2] = lg.argmax(-1)[::2]
    tgt[3 * b + 1] = -100
    dl = torch.randn(s, b, generator=g)
    return h.to(device), w.to(device), tgt.view(s, b).to(device), dl.to(device)


def lmce_ref(h, w, logits16, tgt, dl, vocab=0, soft=1.0):
    """fp32 loss / dh / dW of sum(dl * CE(h W^T)) given the 16-bit logits the kernel's GEMM made
    (so the check isolates the CE + backward GEMMs from the forward GEMM's output rounding)."""
    H = h.shape[-1]
    loss, G = ce_ref(logits16.reshape(-1, logits16.shape[-1]), tgt.reshape(-1), dl.reshape(-1).float(), vocab, soft)
    dh = (G @ w.float()).view(h.shape)
    dw = G.t() @ h.float().reshape(-1, H)
    return loss.view(tgt.shape), dh, dw


def lmce_kernel_emulation(h, w, logits16, tgt, dl, vocab=0):
    """LMHeadCrossEntropy's rounding points: D = softmax - onehot stored 16-bit in place; dX = D W
    in 16-bit then scaled by dl in 16-bit; dW = D^T (h * dl rounded to 16-bit), fp32 accumulate."""
    H = h.shape[-1]
    loss, D = ce_ref(logits16.reshape(-1, logits16.shape[-1]), tgt.reshape(-1),
                     torch.ones(tgt.numel(), device=h.device), vocab)
    D = D.to(h.dtype).float()
    d = dl.reshape(-1, 1).float()
    dh = ((D @ w.float()).to(h.dtype).float() * d).to(h.dtype).view(h.shape)
    hs = (h.float().reshape(-1, H) * d).to(h.dtype).float()
    dw = D.t() @ hs
    return loss.view(tgt.shape), dh, dw


# ----------------------------------------------------------------------------------- softmax

def softmax_case(sk, causal, b=2, np_=4, device="cpu", seed=5, std=8.0, sq=None, dtype=torch.bfloat16):
    """Sharp scores: x ~ N(0, std^2) with scale 0.125 -> scaled std 1 (not near-uniform rows).
    ``sq`` (default sk: square) and ``dtype`` (default bf16) select the other kernel instances."""
    g = torch.Generator().manual_seed(seed)
    sq = sk if sq is None else sq
    x = (std * torch.randn(b, np_, sq, sk, generator=g)).to(dtype)
    dy = torch.randn(b, np_, sq, sk, generator=g).to(dtype)
    return x.to(device), dy.to(device)


def softmax_ref(x, dy, scale, causal, mask=None, dtype=torch.float32):
    """softmax(scale x) and its gradient in ``dtype`` (float64 to judge the fp16 / fp32 kernels).
    ``causal`` masks key j > query i for any [sq, sk] (top-left aligned, the kernel's and
    ``scaled_masked_softmax``'s semantic); a fully masked row is all zeros with a zero gradient."""
    xr = x.detach().to(dtype).requires_grad_()
    s = xr * scale
    sk = x.shape[-1]
    if causal:
        s = s.masked_fill(torch.ones(x.shape[-2], sk, device=x.device, dtype=torch.bool).triu(1), float("-inf"))
    elif mask is not None:
        s = s.masked_fill(mask, float("-inf"))
    dead = torch.isinf(s).all(-1, keepdim=True)
    y = torch.softmax(s.masked_fill(dead, 0.0), -1).masked_fill(dead, 0.0)
    y.backward(dy.to(dtype))
    return y.detach(), xr.grad


def softmax_kernel_emulation(x, dy, scale, causal=False, mask=None):
    """softmax.hip's rounding points in x's dtype T: fp32 math with the fast exponential
    (exp2 of the fp32 product (v - max) * log2 e), y rounded once to T, and
    dx = scale * y (dy - sum(dy y)) from the stored y, rounded once to T."""
    T = x.dtype
    v = x.float() * torch.tensor(scale, dtype=torch.float32)
    if causal:
        v = v.masked_fill(torch.ones(x.shape[-2], x.shape[-1], dtype=torch.bool, device=x.device).triu(1),
                          float("-inf"))
    elif mask is not None:
        v = v.masked_fill(mask, float("-inf"))
    mx = v.amax(-1, keepdim=True)
    dead = torch.isinf(mx)
    e = torch.exp2((v - mx.masked_fill(dead, 0.0)) * 1.4426950408889634)
    e = e.masked_fill(dead, 0.0)
    sm = e.sum(-1, keepdim=True)
    y = (e * torch.where(sm > 0, 1.0 / sm, torch.zeros_like(sm))).to(T)
    yf, g = y.float(), dy.float()
    dx = (torch.tensor(scale, dtype=torch.float32) * yf * (g - (yf * g).sum(-1, keepdim=True))).to(T)
    return y, dx


# ------------------------------------------------- fused (bias + dropout + residual) -> norm

def ln_geometry(H, rows):
    """layernorm.hip's dispatch for a [rows, H] input: G threads per row, C 8-element register
    chunks per thread, and the row strides of the forward / backward grid-stride loops (the group
    that owns row r also owns r + stride, ...)."""
    G = 64 if H <= 2048 else 256
    C = (H // 8 + G - 1) // G
    gpb = 256 // G
    blocks = max(1, (rows + gpb - 1) // gpb)
    return {"G": G, "C": C, "gpb": gpb, "fwd_rstep": min(blocks, 2048) * gpb, "bwd_nblocks": min(blocks, 512),
            "bwd_rstep": min(blocks, 512) * gpb}


def ln_case(rows, H, dtype=torch.bfloat16, wdtype=None, fused=False, summands=False, device="cpu", seed=21):
    """Inputs that make every term of the norm's gradient visible. x has a per-row offset
    ~ N(0, 2^2) and a per-row std in [0.5, 4] (so mean and rstd differ from row to row and a row
    normalised with another row's statistics is wrong); gamma = 1 + 0.5 N(0, 1); dy = N(0, 1) + a_r
    + b_r xhat with a_r, b_r ~ N(0, 1) per row: O(1) and signed, with a row mean (the m1 term) and a
    correlation with xhat (the m2 term) of O(1) in every row. ``fused`` adds bias, residual and
    ds_in; ``summands`` adds x2 and dy2. Seeded CPU generator; composed on ``device``."""
    g = torch.Generator().manual_seed(seed)
    wdtype = wdtype or dtype

    def rn(*shape):
        return torch.randn(*shape, generator=g).to(device)

    z = rn(rows, H)
    off, sd = 2.0 * rn(rows, 1), 0.5 + 3.5 * torch.rand(rows, 1, generator=g).to(device)
    zc = z - z.mean(-1, keepdim=True)
    xh = zc * torch.rsqrt(zc.pow(2).mean(-1, keepdim=True) + 1e-12)
    c = {"x": (off + sd * z).to(dtype), "gamma": (1 + 0.5 * rn(H)).to(wdtype), "beta": (0.5 * rn(H)).to(wdtype),
         "dy": (rn(rows, H) + rn(rows, 1) + rn(rows, 1) * xh).to(dtype)}
    del z, zc, xh
    if fused:
        c["bias"] = (0.5 * rn(H)).to(wdtype)
        c["res"] = rn(rows, H).to(dtype)
        c["ds_in"] = rn(rows, H).to(dtype)
    if summands:
        c["x2"] = rn(rows, H).to(dtype)
        c["dy2"] = (0.5 * rn(rows, H)).to(dtype)
    return c


def ln_s_emulation(x, x2=None, bias=None, res=None, keep=None, keep_scale=1.0):
    """The forward kernel's s = res + keep * scale * (x + x2 + bias): fp32 sums in the kernel's
    order, rounded once to x's dtype."""
    v = x.float()
    if x2 is not None:
        v = v + x2.float()
    if bias is not None:
        v = v + bias.float()
    if keep is not None:
        v = v * (keep.float() * torch.tensor(keep_scale, dtype=torch.float32))
    if res is not None:
        v = v + res.float()
    return v.to(x.dtype)


def ulp_distance(a, b):
    """max over elements of the number of representable values of the (common) dtype between a
    and b (0: bitwise equal up to the sign of zero)."""
    assert a.dtype == b.dtype
    it = torch.int32 if a.dtype == torch.float32 else torch.int16
    top = 0x7FFFFFFF if a.dtype == torch.float32 else 0x7FFF

    def key(t):
        i = t.contiguous().view(it).long()
        return torch.where(i < 0, -(i & top), i)

    return (key(a) - key(b)).abs().max().item()


LN_MUTATIONS = ("no_m1", "m2_h_plus_8", "dgamma_first_pass", "dbeta_no_last_row", "stale_rstd", "dx_unmasked")


def ln_ref(s, gamma, beta, dy, eps, rms, keep=None, keep_scale=1.0, ds_in=None, dy2=None, mutate=None,
           rstep=None):
    """float64 reference of the fused norm, forward and backward, from the stored LayerNorm input
    ``s`` (the kernel's own 16-bit s, so the rounding of s is judged apart) and the dropout keep
    mask. Returns y, mean, rstd, ds (gradient to s, plus ``ds_in``), dx = keep * keep_scale * ds,
    dgamma / dbeta / dbias and, per column, the sums over rows of |term| the three are judged
    against (``sg``, ``sb``, ``sbi``). ``mutate`` (one of LN_MUTATIONS) breaks one term; the
    sensitivity test shows that every criterion rejects it. ``rstep`` is the backward loop's row
    stride (``ln_geometry``), used by the stale-statistics mutation."""
    assert mutate is None or mutate in LN_MUTATIONS, mutate
    S, g = s.double(), gamma.double()
    H = S.shape[-1]
    mu = torch.zeros_like(S[:, :1]) if rms else S.mean(-1, keepdim=True)
    rs = torch.rsqrt((S - mu).pow(2).mean(-1, keepdim=True) + eps)
    xh = (S - mu) * rs
    y = xh * g
    if not rms and beta is not None:
        y = y + beta.double()
    d = dy.double() if dy2 is None else dy.double() + dy2.double()
    dyg = d * g
    m1 = torch.zeros_like(mu) if (rms or mutate == "no_m1") else dyg.mean(-1, keepdim=True)
    m2 = (dyg * xh).sum(-1, keepdim=True) / (H + 8 if mutate == "m2_h_plus_8" else H)
    rs_b = rs
    if mutate == "stale_rstd":     # row r computed with row r + rstep's rstd (the next loop iteration's)
        rs_b = rs.clone()
        rs_b[:-rstep] = rs[rstep:]
    ds = rs_b * (dyg - m1 - xh * m2)
    if ds_in is not None:
        ds = ds + ds_in.double()
    dx = ds
    if keep is not None and mutate != "dx_unmasked":
        dx = ds * keep.double() * keep_scale
    tg = d * xh
    out = {"y": y, "mean": mu[:, 0], "rstd": rs[:, 0], "ds": ds, "dx": dx,
           "dgamma": (tg[:2048] if mutate == "dgamma_first_pass" else tg).sum(0),
           "dbeta": (d[:-1] if mutate == "dbeta_no_last_row" else d).sum(0), "dbias": dx.sum(0),
           "sg": tg.abs().sum(0), "sb": d.abs().sum(0), "sbi": dx.abs().sum(0)}
    return out


def ln_kernel_emulation(s, gamma, beta, dy, eps, rms, keep=None, keep_scale=1.0, ds_in=None, dy2=None):
    """layernorm.hip's rounding points: fp32 arithmetic throughout (two-pass mean / variance);
    y, ds and dx each rounded once to s's dtype (dx from the unrounded ds); the column sums
    accumulated in fp32 in the backward's slab order: one register partial per (block, group)
    over rows r, r + rstep, ..., then the block's groups, then the blocks."""
    T = s.dtype
    rows, H = s.shape
    geo = ln_geometry(H, rows)
    S, g = s.float(), gamma.float()
    mu = torch.zeros_like(S[:, :1]) if rms else S.sum(-1, keepdim=True) / H
    rs = torch.rsqrt((S - mu).pow(2).sum(-1, keepdim=True) / H + torch.tensor(eps, dtype=torch.float32))
    xh = (S - mu) * rs
    y = xh * g
    if not rms and beta is not None:
        y = y + beta.float()
    d = dy.float() if dy2 is None else dy.float() + dy2.float()
    dyg = d * g
    m1 = torch.zeros_like(mu) if rms else dyg.sum(-1, keepdim=True) / H
    m2 = (dyg * xh).sum(-1, keepdim=True) / H
    ds = rs * (dyg - m1 - xh * m2)
    if ds_in is not None:
        ds = ds + ds_in.float()
    dx = ds if keep is None else ds * keep.float() * torch.tensor(keep_scale, dtype=torch.float32)

    def colsum(term):
        rstep, gpb = geo["bwd_rstep"], geo["gpb"]
        acc = torch.zeros(rstep, H, dtype=torch.float32, device=term.device)
        for r0 in range(0, rows, rstep):
            n = min(rstep, rows - r0)
            acc[:n] += term[r0:r0 + n]
        acc = acc.view(-1, gpb, H)
        blk = acc[:, 0].clone()
        for q in range(1, gpb):
            blk += acc[:, q]
        return blk.sum(0)

    return {"y": y.to(T), "mean": mu[:, 0], "rstd": rs[:, 0], "ds": ds.to(T), "dx": dx.to(T),
            "dgamma": colsum(d * xh), "dbeta": colsum(d), "dbias": colsum(dx)}


def col_rel_err(out, ref, scale) -> float:
    """max over columns of |out - ref| / scale, with ``scale`` the float64 sum over rows of |term|:
    a parameter gradient is judged against what fp32 accumulation of its terms can deliver, not
    against a sum that may cancel to ~0."""
    o = out.detach().double().reshape(-1)
    r = ref.detach().double().reshape(-1).to(o.device)
    return ((o - r).abs() / scale.detach().double().reshape(-1).to(o.device).clamp_min(1e-300)).max().item()


def vp_lmce_two_shards(h, w, tgt, dl, vocab=0, ranks=2, local_pass=None):
    """The vocab-parallel LM-head CE math of ``VocabParallelLMHeadCE`` run for ``ranks`` vocab
    shards in one process: per shard the logits GEMM and ``local_pass`` (the HIP kernel or its CPU
    reference), the statistics combined, the one-hot subtracted at one element per row, and the
    backward products with the per-row scale c dl on the hidden side. Returns (loss, dh, dW,
    16-bit logits of all shards) for comparison with ``lmce_ref`` on the same logits."""
    from smdt_amd.parallel import tensor_parallel as tp
    local_pass = local_pass or tp.ce_local_pass
    H = h.shape[-1]
    V = w.shape[0]
    vl = V // ranks
    x = h.reshape(-1, H)
    t = tgt.reshape(-1)
    shards, stats, lgs = [], [], []
    for r in range(ranks):
        ws_ = w[r * vl:(r + 1) * vl]
        lg = x @ ws_.t() if not x.is_cuda else tp.linear_rows(x, ws_)
        lg = lg.to(h.dtype)
        lgs.append(lg.clone())
        vv = min(max(vocab - r * vl, 0), vl) if vocab else 0
        vv = 0 if vv == vl else vv
        st = local_pass(lg, t, r * vl, vv)
        shards.append((lg, vv))
        stats.append(st)
    allst = torch.stack(stats)
    d = dl.reshape(-1).float()
    dh = torch.zeros(x.shape, dtype=torch.float32, device=x.device)
    dws = []
    for r, (e, vv) in enumerate(shards):
        loss, c = tp.combine_ce_stats(allst, stats[r], t, -100)
        tp.subtract_onehot_(e, t, c, r * vl, vv, -100)
        rr = (d * c)[:, None]
        dh += (e.float() @ w[r * vl:(r + 1) * vl].float()) * rr
        dws.append(e.float().t() @ (x.float() * rr).to(h.dtype).float())
    return loss.view(tgt.shape), dh.view(h.shape), torch.cat(dws), torch.cat(lgs, -1)
