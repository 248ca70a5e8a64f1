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


# --------------------------------------------------------------------------- flash attention
#
# Scores that move the forward kernel's lazy reference max. flash_attn.hip's forward takes
# p = exp2(S - m) with m = 0 and moves m (the "rescue") only when a row's 64-key tile sum leaves a
# window; randn inputs (scores ~ N(0, 1)) never get there. ``flash_score_case`` puts a chosen level
# on every (query, key tile) through one reserved channel of the head dim, ``flash_lazy_max_twin``
# follows the forward tile by tile in torch (fp32, the kernel's rounding points and move rule, with
# mutations), and ``flash_kernel_emulation`` is float64 attention with only the three kernels'
# 16-bit rounding points: the yardstick the GPU tests judge the kernels against.

FLASH_SCALE = 0.125          # passed explicitly for D = 64 and D = 128: the offsets stay exact
FLASH_TILE = 64              # kTile: keys per tile of the forward sweep
_LOG2E_F32 = 1.4426950408889634
# Move-rule windows (log2 of the tile sum) of fwd_kernel per type; FLASH_WINDOW_PARENT is the one
# every type shared before the fp16 fix (kept for the CPU record of the defect).
FLASH_WINDOW_PARENT = (-64, 64)
FLASH_WINDOWS = {torch.bfloat16: (-64, 64), torch.float16: (0, 15)}

# name -> (natural-log level per key tile for a query with qa = 16 (cycled past 4 tiles), qa values
# of even / odd queries). A query with qa = 0 sees plain scores, so the lanes of a wave disagree.
FLASH_PROFILES = {
    "plain": ((0, 0, 0, 0), (0, 16)),                  # control
    "up_late": ((0, 50, 100, 50), (0, 16)),            # upward rescue after l > 0, twice; causal diagonal too
    "low_start": ((-60, -60, -30, -30), (0, 16)),      # downward rescue with l == 0
    "very_low": ((-100, -100, -100, -100), (0, 16)),   # tmax < -128 (log2): alpha = exp2(-tmax) = inf
    "very_low_first": ((-100, 0, 0, 0), (0, 16)),      # ... and real mass afterwards
    "fp16_high": ((20, 20, 20, 20), (0, 16)),          # inside the bf16 window, above fp16's maximum
    "fp16_low": ((-25, -25, -25, -25), (0, 16)),       # inside the bf16 window, below fp16's minimum
    # p = exp2(S) ~ 2^-20 is finite and non-zero in fp16 but a subnormal with 4 bits: a lower window
    # bound that only keeps p away from zero is not enough (this profile sets fp16's lower bound)
    "fp16_subnormal": ((-14, -14, -14, -14), (0, 16)),
    # odd queries rise as in up_late while even queries fall: at the tile where the odd lanes ask
    # for the rescue the even lanes hold l > 0 and tmax < -128 (moving them would overflow l)
    "opposed": ((0, 50, 100, 50), (-16, 16)),
}


def flash_score_case(profile, B=2, S=256, H=2, Hkv=2, D=64, dtype=torch.bfloat16, device="cpu", seed=31):
    """q, k, v, do ([B, S, heads, D], ``dtype``) whose scores (with scale FLASH_SCALE) carry the
    profile's level per 64-key tile: channel 0 holds qa[q] (a power of two, or 0) in q and
    kb[k] = level / (FLASH_SCALE * 16) (a multiple of 1/2) in k, both exact in bf16 and fp16, so the
    added score FLASH_SCALE * qa * kb is exact; the other channels are randn scaled to an O(1)
    score contribution, so the keys of a plateau differ and no row is degenerate."""
    levels, qa_vals = FLASH_PROFILES[profile]
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, S, H, D, generator=g) * (8.0 / D ** 0.5)
    k = torch.randn(B, S, Hkv, D, generator=g)
    v = torch.randn(B, S, Hkv, D, generator=g)
    do = torch.randn(B, S, H, D, generator=g)
    ar = torch.arange(S)
    qa = torch.where(ar % 2 == 1, float(qa_vals[1]), float(qa_vals[0]))
    lv = torch.tensor([levels[(t // FLASH_TILE) % len(levels)] for t in range(S)], dtype=torch.float32)
    kb = lv / (FLASH_SCALE * 16.0)
    q[..., 0] = qa[None, :, None]
    k[..., 0] = kb[None, :, None]
    out = tuple(t.to(dtype).to(device) for t in (q, k, v, do))
    assert torch.equal(out[1][..., 0].float().cpu(), kb[None, :, None].expand(B, S, Hkv)), "kb not exact"
    return out


def _bhsd(t, H, wd):
    """[B, S, heads, D] -> [B, H, S, D] in ``wd`` (kv heads repeated for GQA)."""
    t = t.detach().to(wd).transpose(1, 2)
    return t if t.shape[1] == H else t.repeat_interleave(H // t.shape[1], dim=1)


def _flash_masked(B, S, causal, doc_start, device):
    """bool [B, 1, S, S], True = masked (key after the query / before the query's document)."""
    ar = torch.arange(S, device=device)
    m = torch.zeros(B, 1, S, S, dtype=torch.bool, device=device)
    if causal:
        m = m | (ar[None, :] > ar[:, None])
    if doc_start is not None:
        m = m | (ar[None, None, :] < doc_start.to(device)[:, :, None].long()).unsqueeze(1)
    return m


def flash_ref(q, k, v, do, scale, causal, dropout_p=0.0, keep=None, doc_start=None):
    """float64 attention on the given 16-bit inputs: o and the three gradients from
    ``attention_ref`` on ``.double()`` copies, lse = logsumexp of the masked scores. [B, S, heads, D];
    lse [B, H, S]."""
    from smdt_amd.ops import functional as SF
    qd, kd, vd = (t.detach().double().requires_grad_() for t in (q, k, v))
    o = SF.attention_ref(qd, kd, vd, scale, causal, dropout_p, keep, doc_start)
    assert o.dtype == torch.float64
    o.backward(do.detach().double())
    B, S, H, _ = q.shape
    s = torch.matmul(_bhsd(q, H, torch.float64), _bhsd(k, H, torch.float64).transpose(-1, -2)) * scale
    s = s.masked_fill(_flash_masked(B, S, causal, doc_start, q.device), float("-inf"))
    return {"o": o.detach(), "lse": torch.logsumexp(s, -1), "dq": qd.grad, "dk": kd.grad, "dv": vd.grad}


def _drop_consts(dropout_p):
    """(1 / (1 - p_realised), 1 - p_realised, fp32 log2 of the first) as the launcher makes them."""
    if not dropout_p:
        return 1.0, 1.0, 0.0
    from smdt_amd.ops import functional as SF
    thr, inv = SF.flash_dropout_thr(dropout_p)
    import math
    return float(torch.tensor(inv, dtype=torch.float32)), float(torch.tensor((128.0 - thr) / 128.0, dtype=torch.float32)), \
        float(torch.tensor(math.log2(inv), dtype=torch.float32))


def flash_kernel_emulation(q, k, v, do, scale, causal, dropout_p=0.0, keep=None, doc_start=None, m_ref=None):
    """float64 attention, forward and backward, with only the rounding points of flash_attn.hip in
    the inputs' 16-bit type T (a true row max, no window; ``m_ref``, [B, H, S] in the log2 domain,
    replaces the row max as the point P is rounded at, see ``flash_emulation_at_kernel_max``):
      * forward and dQ kernel: Q' = T(q * scale * log2 e) (fp32 product), scores Q' K^T in the log2
        domain; the dK / dV kernel prescales K instead: scores Q K'^T with K' = T(k * scale * log2 e);
      * forward: P = exp2(S - max) rounded to T before P V (l sums the unrounded, undropped p),
        O = T(P V / l / (1 - p)), lse = fp32 (max + log2 l) ln 2;
      * backward: P' = exp2(S - lse log2 e + log2 inv) from the forward's lse (fp32 row constant),
        delta' = keep * sum(dO O) from the stored 16-bit O; P' (dV) and dS = P' (dP - delta') (dQ,
        dK) rounded to T; dQ = T(scale dS K), dK = T(scale dS^T Q), dV = T(P'^T dO), the kv heads'
        groups summed before the rounding.
    Returns o, lse, dq, dk, dv like ``flash_ref``."""
    T, f64 = q.dtype, torch.float64
    B, S, H, D = q.shape
    Hkv = k.shape[2]
    c2 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(_LOG2E_F32, dtype=torch.float32)
    inv, keepf, log2inv = _drop_consts(dropout_p)
    Q, K, V, DO = (_bhsd(t, H, f64) for t in (q, k, v, do))
    Qp = _bhsd((q.float() * c2).to(T), H, f64)
    Kp = _bhsd((k.float() * c2).to(T), H, f64)
    masked = _flash_masked(B, S, causal, doc_start, q.device)
    kp = torch.ones((), dtype=f64, device=q.device) if keep is None else keep.to(f64)
    sq = torch.matmul(Qp, K.transpose(-1, -2)).masked_fill(masked, float("-inf"))
    sk = torch.matmul(Q, Kp.transpose(-1, -2)).masked_fill(masked, float("-inf"))
    m = sq.amax(-1, keepdim=True) if m_ref is None else m_ref.to(f64)[..., None]
    p = torch.exp2(sq - m)
    l = p.sum(-1, keepdim=True)
    O = (torch.matmul(p.to(T).to(f64) * kp, V) * (inv / l)).to(T)
    lse = ((m + torch.log2(l)) * 0.6931471805599453).float()[..., 0]
    nlse2 = (log2inv - lse * torch.tensor(_LOG2E_F32, dtype=torch.float32)).to(f64)[..., None]
    delta = keepf * (O.to(f64) * DO).sum(-1, keepdim=True)
    dP = torch.matmul(DO, V.transpose(-1, -2)) * (kp if keep is not None else 1.0)
    Pq, Pk = torch.exp2(sq + nlse2), torch.exp2(sk + nlse2)
    dSq = (Pq * (dP - delta)).to(T).to(f64)
    dSk = (Pk * (dP - delta)).to(T).to(f64)
    dq = (torch.matmul(dSq, K) * scale).to(T)
    dk = torch.matmul(dSk.transpose(-1, -2), Q).view(B, Hkv, H // Hkv, S, D).sum(2)
    dv = torch.matmul((Pk.to(T).to(f64) * kp).transpose(-1, -2), DO).view(B, Hkv, H // Hkv, S, D).sum(2)
    return {"o": O.transpose(1, 2), "lse": lse, "dq": dq.transpose(1, 2), "dk": (dk * scale).to(T).transpose(1, 2),
            "dv": dv.to(T).transpose(1, 2)}


def flash_emulation_at_kernel_max(q, k, v, do, scale, causal, dropout_p=0.0, keep=None, doc_start=None):
    """``flash_kernel_emulation`` with P rounded where the kernel rounds it: at the lazy reference
    max the forward ends with (``flash_lazy_max_twin``'s m, 0 for a row that never asked for the
    rescue), not at the row max. With a true max the row's largest p is exactly 1 and survives the
    rounding to T; at the lazy m it is some 2^x that rounds by up to half an ulp while l sums the
    unrounded p, so O of a row with one dominant key is off by that half ulp, and delta = sum(dO O)
    no longer cancels dP in dS = P (dP - delta): a causal row 0 (one key, exact dq = 0) gets a dq of
    ~2^-9 |dO . v| |k| in bf16. That is rounding of the design, not a defect; the GPU tests measure
    the kernels against this emulation."""
    T, S = q.dtype, q.shape[1]
    qp, kp, vp, dsp = q, k, v, doc_start
    if S % 128:       # the launcher pads a causal sequence at its end (pad rows: a document of their own)
        assert causal and keep is None
        pad = lambda t: torch.nn.functional.pad(t, (0, 0, 0, 0, 0, -S % 128))
        qp, kp, vp = pad(q), pad(k), pad(v)
        if doc_start is not None:
            dsp = torch.cat([doc_start, doc_start.new_full((doc_start.shape[0], -S % 128), S)], 1)
    m = flash_lazy_max_twin(qp, kp, vp, scale, causal, T, FLASH_WINDOWS[T], dsp, keep, None, dropout_p,
                            return_m=True)[2][..., :S]
    return flash_kernel_emulation(q, k, v, do, scale, causal, dropout_p, keep, doc_start, m_ref=m)


FLASH_MUTATIONS = ("no_o_rescale", "no_l_rescale", "lse_without_m", "rescue_ignores_mask", "select_all_lanes")


def flash_lazy_max_twin(q, k, v, scale, causal, dtype, window, doc_start=None, keep=None, mutate=None,
                        dropout_p=0.0, alpha_guard=True, return_m=False):
    """fwd_kernel of flash_attn.hip in torch, tile by tile, in fp32: 64-key tiles, Q prescaled by
    scale * log2 e and rounded to ``dtype``, m = 0 at the start and p = exp2(S - m) taken at once;
    a row is "bad" when its tile sum is above 2^window[1] (or not finite) or, with l == 0, below
    2^window[0]; a 32-row wave with a bad row recomputes the tile, and d = bad ? tile max : 0 moves
    m and rescales l and o by alpha = exp2(-d). p is rounded to ``dtype`` (and dropped with ``keep``)
    before P V; l sums the unrounded, undropped p. ``alpha_guard`` False is the rule before the fix
    (alpha is applied even where nothing was accumulated: 0 * inf). The causal / DOC tile skips and
    masks are the kernel's (wave- and block-uniform). ``mutate`` (FLASH_MUTATIONS) breaks one step
    of the rescue. Returns o ([B, S, H, D], ``dtype``) and lse (fp32 [B, H, S]); ``return_m`` adds the
    final reference max m (log2 domain, [B, H, S])."""
    assert mutate is None or mutate in FLASH_MUTATIONS, mutate
    f32, T = torch.float32, dtype
    B, S, H, D = q.shape
    dev = q.device
    lo, hi = (torch.tensor(2.0 ** w, dtype=f32) for w in window)
    c2 = torch.tensor(scale, dtype=f32) * torch.tensor(_LOG2E_F32, dtype=f32)
    Qp = _bhsd((q.float() * c2).to(T), H, torch.float64)
    K, V = _bhsd(k.to(T), H, torch.float64), _bhsd(v.to(T), H, torch.float64)
    s2 = torch.matmul(Qp, K.transpose(-1, -2)).to(f32)          # fp32 accumulators of the score MFMAs
    inv = _drop_consts(dropout_p)[0]
    ar = torch.arange(S, device=dev)
    qw, q0 = ar // 32 * 32, ar // 128 * 128
    m = torch.zeros(B, H, S, dtype=f32, device=dev)
    l = torch.zeros_like(m)
    o = torch.zeros(B, H, S, D, dtype=f32, device=dev)
    doc = doc_start is not None
    if doc:
        ds = doc_start.to(dev).long()
        ds_q, ds_lo = ds[:, None, :], ds[:, qw][:, None, :]
        tfirst = (torch.minimum(ds[:, q0].clamp_min(0), q0[None]) // FLASH_TILE)[:, None, :]
    for t in range(S // FLASH_TILE):
        kb = t * FLASH_TILE
        keys = kb + torch.arange(FLASH_TILE, device=dev)
        visit = torch.ones(B, 1, S, dtype=torch.bool, device=dev)
        masked = torch.zeros(B, 1, S, FLASH_TILE, dtype=torch.bool, device=dev)
        if causal:
            visit = visit & (kb <= qw + 31)[None, None, :]
            masked = masked | (keys[None, :] > ar[:, None])
        dead = torch.zeros(B, 1, S, dtype=torch.bool, device=dev)
        if doc:
            visit = visit & (t >= tfirst) & (kb + FLASH_TILE > ds_lo)
            masked = masked | (keys[None, None, None, :] < ds_q[..., None])
            dead = kb + FLASH_TILE <= ds_q
        raw = s2[..., kb:kb + FLASH_TILE]

        def scores(mask=True):
            st = raw - m[..., None]
            return st.masked_fill(masked, float("-inf")) if mask else st

        p = torch.exp2(scores())
        rsum = p.sum(-1)
        bad = visit & ~dead & (~(rsum <= hi) | ((l == 0) & (rsum < lo)))
        ballot = bad.view(B, H, S // 32, 32).any(-1, keepdim=True).expand(B, H, S // 32, 32).reshape(B, H, S)
        if bool(ballot.any()):
            st = scores(mask=mutate != "rescue_ignores_mask")
            tmax = st.amax(-1)
            sel = ballot if mutate == "select_all_lanes" else bad
            d = torch.where(sel, tmax, torch.zeros_like(tmax))
            alpha = torch.exp2(-d)
            if alpha_guard:
                alpha = torch.where(l > 0, alpha, torch.ones_like(alpha))
            if mutate != "no_l_rescale":
                l = torch.where(ballot, l * alpha, l)
            if mutate != "no_o_rescale":
                o = torch.where(ballot[..., None], o * alpha[..., None], o)
            p2 = torch.exp2(st - d[..., None])
            m = torch.where(ballot, m + d, m)
            p = torch.where(ballot[..., None], p2, p)
            rsum = p.sum(-1)
        pb = p.to(T)
        if keep is not None:
            pb = pb * keep[..., kb:kb + FLASH_TILE].to(T)
        # fp32 accumulation of P V; 0 * inf and inf - inf come out as in the MFMA (NaN)
        pv = torch.matmul(pb.double(), V[:, :, kb:kb + FLASH_TILE]).to(f32)
        l = torch.where(visit.expand_as(l), l + rsum, l)
        o = torch.where(visit[..., None].expand_as(o), o + pv, o)
    rinv = torch.where(l > 0, inv / l, torch.zeros_like(l))
    lse = (torch.log2(l) if mutate == "lse_without_m" else m + torch.log2(l)) * 0.6931471805599453
    out = (o * rinv[..., None]).to(T).transpose(1, 2)
    return (out, lse, m) if return_m else (out, lse)


def row_rel_errs(out, ref, floor_frac: float = 1e-4):
    """The per-row terms of ``row_rel_err`` (same floor) and the rows' max|ref|, float64."""
    o = out.detach().double().reshape(-1, out.shape[-1])
    r = ref.detach().double().reshape(-1, ref.shape[-1]).to(o.device)
    rmax = r.abs().amax(-1)
    den = rmax.clamp_min(floor_frac * r.abs().max().clamp_min(1e-30))
    return (o - r).abs().amax(-1) / den, rmax, den


def ulp_at(x, dtype):
    """One unit in the last place of ``dtype`` at magnitude x (float64 tensor; the spacing of the
    smallest normal below it)."""
    fi = torch.finfo(dtype)
    return torch.exp2(torch.floor(torch.log2(x.clamp_min(fi.tiny)))) * fi.eps


def flash_grad_floors(q, k, v, do, scale, causal, dropout_p=0.0, keep=None, doc_start=None):
    """Per row of dq / dk / dv ([B, S, heads]), the absolute error that the rounding of the 16-bit
    MFMA operands alone can put into the row (as ``softmax_grad_floor`` does for the softmax): two
    implementations with the same rounding points still differ in which way single values round,
    and a row that sums many of them (exactly cancelling ones included) sees the sum. From float64
    attention on the same inputs, worst case (all errors aligned), u = half an ulp of the type:
      dS = P (dP - delta) as a 16-bit operand: |err| <= u |dS| + D 2^-24 P (sum_d |O dO| + sum_d |dO V|)
        (its rounding, and the fp32 sums of D terms behind delta and dP, which cancel in dP - delta);
      dq = scale dS K -> scale sum_k err |K|;  dk = scale dS^T Q -> scale sum_q err |Q|;
      dv = P^T dO with P a 16-bit operand -> sum_q u P |dO|;  each the max over the row's columns."""
    f64 = torch.float64
    B, S, H, D = q.shape
    Hkv = k.shape[2]
    u, g32 = torch.finfo(q.dtype).eps / 2, D * 2.0 ** -24
    inv = _drop_consts(dropout_p)[0]
    Q, K, V, DO = (_bhsd(t, H, f64) for t in (q, k, v, do))
    s = (torch.matmul(Q, K.transpose(-1, -2)) * scale).masked_fill(_flash_masked(B, S, causal, doc_start, q.device),
                                                                    float("-inf"))
    P = torch.softmax(s, -1)
    Pd = P * inv if keep is None else P * keep.to(f64) * inv
    O = torch.matmul(Pd, V)
    dP = torch.matmul(DO, V.transpose(-1, -2))
    dS = Pd * dP - P * (O * DO).sum(-1, keepdim=True)
    err = u * dS.abs() + g32 * P * inv * ((O.abs() * DO.abs()).sum(-1, keepdim=True)
                                         + torch.matmul(DO.abs(), V.abs().transpose(-1, -2)))
    grp = lambda t: t.view(B, Hkv, H // Hkv, S, D).sum(2)
    return {"dq": (scale * torch.matmul(err, K.abs())).amax(-1).transpose(1, 2),
            "dk": grp(scale * torch.matmul(err.transpose(-1, -2), Q.abs())).amax(-1).transpose(1, 2),
            "dv": grp(torch.matmul((u * Pd).transpose(-1, -2), DO.abs())).amax(-1).transpose(1, 2)}


def flash_excess(out, emu, ref, dtype, floor=None):
    """The flash criterion. Row by row (rows and denominators as in ``row_rel_err``, with its floor):
    the kernel's error <= 2 x the error of the emulation IN THE SAME ROW against the same float64
    reference + one ulp of the 16-bit type at the row's denominator + ``floor`` (per row, absolute:
    ``flash_grad_floors`` for the gradients). A bound taken from the emulation's worst row would let
    that one row (a causal row 0 with exact dq = 0, judged against the floor) excuse every other
    row. The criterion as the issue words it, error <= 2 x ``row_rel_err`` of the emulation + one ulp
    at the row's max, is kept beside it; the result is the larger of the two excesses. Returns
    (worst kernel error / bound over the rows, largest kernel error, largest emulation error); lse
    ([B, H, S]) is judged one value per row. Not finite anywhere -> inf."""
    if out.dim() == 3:
        out, emu, ref = out[..., None], emu[..., None], ref[..., None]
    ee = row_rel_errs(emu, ref)[0]
    if not bool(torch.isfinite(out.detach().double()).all()):
        return float("inf"), float("inf"), ee.max().item()
    ek, rmax, den = row_rel_errs(out, ref)
    fl = 0.0 if floor is None else floor.detach().double().reshape(-1).to(den.device)
    own = ek / (2.0 * ee + (ulp_at(den, dtype) + fl) / den)
    worst = ek / (2.0 * ee.max() + ulp_at(rmax, dtype) / den)
    return max(own.max().item(), worst.max().item()), ek.max().item(), ee.max().item()


def assert_flash_close(got, emu, ref, dtype, names=("o", "lse", "dq", "dk", "dv"), what="", floors=None):
    """``flash_excess`` <= 1 for every named output (``floors``: ``flash_grad_floors``); prints each
    figure before it asserts."""
    fails = []
    for n in names:
        ratio, ek, ee = flash_excess(got[n], emu[n], ref[n], dtype, (floors or {}).get(n))
        print(f"flash {what} {n}: kernel {ek:.3e} emulation {ee:.3e} kernel/bound {ratio:.3f}")
        if not ratio <= 1.0:
            fails.append(f"{n}: error {ek:.4g} vs emulation {ee:.4g}, {ratio:.3g}x the bound")
    assert not fails, f"{what}: " + "; ".join(fails)


# ---------------------------------------------------------------------- weight gradient, exact data
#
# Operands on which every sum of the weight-gradient kernels is exact, so a kernel is compared bit
# for bit whatever its summation order (split-K and tail pieces add with atomics).

def wgrad_exact_case(g, M, N, K, dy_dtype, x_dtype=None):
    """dY [M, N] and x [M, K] from {0, +-0.5, +-1, +-2} (exact in bf16, fp16, E5M2 and E4M3), a
    target [N, K] and a bias target [N] of small integers."""
    vals = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0])
    a = vals[torch.randint(0, 7, (M, N), generator=g)].to(dy_dtype)
    b = vals[torch.randint(0, 7, (M, K), generator=g)].to(x_dtype or dy_dtype)
    mg = torch.randint(-8, 9, (N, K), generator=g).float()
    bg = torch.randint(-8, 9, (N,), generator=g).float()
    return a, b, mg, bg


def wgrad_exact_twin(mg, a, b, overwrite, inv_dy=None, inv_x=None):
    """The twin on the CPU, with the check that makes it an exact reference: its fp32 result equals
    the float64 one, so no sum of these inputs rounds (every product is a multiple of 1/4 no larger
    than 4, every partial sum a multiple of 1/4 below 2^22 for M <= 2^18, the two dequantisation
    factors of the FP8 form are powers of two and the target holds small integers: any order,
    atomics included, is exact). ``inv_dy`` / ``inv_x`` (one-element tensors) select the FP8 twin."""
    assert a.shape[0] <= 2 ** 18
    if inv_dy is None:
        prod = a.float().t().matmul(b.float())
        out = prod if overwrite else mg + prod
        r64 = a.double().t() @ b.double()
    else:
        from smdt_amd.ops import functional as SF
        out = SF.fp8_wgrad_ref(mg.clone(), a, b, inv_dy, inv_x, overwrite)
        r64 = (a.double() * inv_dy.double()).t() @ (b.double() * inv_x.double())
    if not overwrite:
        r64 = r64 + mg.double()
    assert torch.equal(out.double(), r64)
    return out


def wgrad_exact_bias_twin(bg, a):
    """start + column sums of dY, exact for the same reason."""
    out = bg + a.float().sum(0)
    assert torch.equal(out.double(), bg.double() + a.double().sum(0))
    return out
