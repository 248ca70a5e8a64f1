"""cross_entropy.hip, rope.hip, bias_act.hip and the row gather of transpose.hip at every tail,
dtype and mode they dispatch to, against the float64 references of tests/_numerics.py.

Every shape is the smallest at which the named code path still runs: the two-kernel CE sweeps 2048
columns per trip (V = 8 leaves 255 threads with m = -inf, 2056 gives thread 0 a second vector), the
fused CE keeps 4 / 7 / 8 vectors per thread, RoPE picks a token-per-block kernel at
nh * rot / 16 >= 64, the partial-free bias-activation launches give a thread 4 rows and the d(bias)
launches about 1024 blocks. Every tolerance comes from the CPU emulations in
tests/test_numerics_sensitivity.py (4x the emulation's error), which also shows that each criterion
rejects a twin with one thing wrong. Each case prints its figures before it asserts.
"""
import pytest
import torch

from smdt_amd.ops import _ext
from smdt_amd.ops import functional as SF

import _numerics as N

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, HF, F32 = N.PL_DTYPES
_NAME = {BF: "bf16", HF: "fp16", F32: "fp32"}
ALL = pytest.mark.parametrize("dtype", N.PL_DTYPES, ids=[_NAME[t] for t in N.PL_DTYPES])
HALF = pytest.mark.parametrize("dtype", (BF, HF), ids=["bf16", "fp16"])


def _C():
    return _ext.ext()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _report(fails, ok, line):
    print(line)
    if not ok:
        fails.append(line)


# ------------------------------------------------------------ cross entropy, two kernels

def _ce_run(lg, tgt, dl, vv, ignore_index=-100, inplace=False):
    """``cross_entropy`` forward + backward on the GPU; returns loss, the gradient tensor the
    backward handed to autograd, and the logits tensor it ran on."""
    x = lg.to(DEV).clone().requires_grad_()
    got = []
    x.register_hook(got.append)
    loss = SF.cross_entropy(x, tgt.to(DEV), ignore_index=ignore_index, inplace_grad=inplace, vocab_size=vv)
    loss.backward(dl.to(DEV))
    return loss.detach(), got[0], x


def _ce_judge(fails, what, dtype, loss, grad, lg, tgt, dl, vv, ignored=5):
    tol = N.PL_CE_TOL[dtype]
    rl, rg, rmax, fl = N.pl_ce_ref(lg, tgt, dl, vv)
    el, eg = N.ce_loss_err(loss, rl, rmax), N.row_rel_err(grad, rg, row_floor=fl)
    exact = bool((grad[:, vv or lg.shape[1]:] == 0).all() and (grad[ignored] == 0).all() and loss[ignored] == 0)
    ok = el <= tol["loss"] and eg <= tol["grad"] and exact and bool(torch.isfinite(grad).all())
    _report(fails, ok, f"CE {what} {_NAME[dtype]}: loss {el:.3g} (tol {tol['loss']:.3g}) grad {eg:.3g} "
                       f"(tol {tol['grad']:.3g}) padding / ignored row exactly zero: {exact}")


@ALL
def test_ce_two_kernel_tails_padding_and_profiles(dtype):
    """ce_stats_kernel / ce_bwd_kernel through ``cross_entropy``: V on both sides of the 2048-column
    sweep, padding inside the last vector / dropping a vector / down to one column, and the logit
    profiles (ascending: every online update rescales; offset; scattered -inf; columns 8..15 all
    -inf, thread 1's first vector). Padding columns and the ignored row are exactly zero."""
    fails = []
    for V, vv, prof in N.PL_CE_CASES:
        lg, tgt, dl = N.pl_ce_case(V, dtype, prof, vv)
        loss, grad, _ = _ce_run(lg, tgt, dl, vv)
        _ce_judge(fails, f"V={V} vvalid={vv} {prof}", dtype, loss, grad, lg, tgt, dl, vv)
    assert not fails, "\n".join(fails)


@ALL
@pytest.mark.parametrize("V,vv,shards", N.PL_CE_SHARD_CASES, ids=[f"V{V}-vv{vv}-x{s}" for V, vv, s in N.PL_CE_SHARD_CASES])
def test_ce_vocab_shards_without_a_process_group(V, vv, shards, dtype):
    """ce_stats per vocab slice with vstart = r V / R (targets fall below, inside and above each
    slice), the statistics combined on the host by ``_FusedCE.forward``'s formula, ce_bwd per slice
    with the global statistics: loss and the concatenated gradient equal the full-row reference."""
    C = _C()
    lg, tgt, dl = N.pl_ce_case(V, dtype, "peaked", vv)
    vl = V // shards
    t, d = tgt.to(DEV), dl.to(DEV)
    parts = [(lg[:, r * vl:(r + 1) * vl].contiguous().to(DEV), r * vl, N.ce_shard_vvalid(vv or V, r, vl))
             for r in range(shards)]
    gmax, se, tg = N.ce_combine_stats([C.ce_stats(x, t, vs, v) for x, vs, v in parts])
    loss = N.ce_loss_from_stats(gmax, se, tg, t)
    outs = []
    for x, vs, v in parts:
        out = torch.empty_like(x)
        C.ce_bwd(x, t, gmax, se, d, out, vs, -100, v)
        outs.append(out)
    fails = []
    _ce_judge(fails, f"V={V} vvalid={vv} in {shards} slices", dtype, loss, torch.cat(outs, -1), lg, tgt, dl, vv)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("ignore_index", [-100, -1])
def test_ce_ignore_index(ignore_index):
    fails = []
    for dtype in N.PL_DTYPES:
        lg, tgt, dl = N.pl_ce_case(520, dtype, ignore_index=ignore_index)
        assert tgt[5] == ignore_index
        loss, grad, _ = _ce_run(lg, tgt, dl, 0, ignore_index)
        rl, rg, rmax, fl = N.pl_ce_ref(lg, tgt, dl, 0, ignore_index)
        el, eg = N.ce_loss_err(loss, rl, rmax), N.row_rel_err(grad, rg, row_floor=fl)
        exact = bool(loss[5] == 0 and (grad[5] == 0).all())
        _report(fails, exact and el <= N.PL_CE_TOL[dtype]["loss"] and eg <= N.PL_CE_TOL[dtype]["grad"],
                f"CE ignore_index={ignore_index} {_NAME[dtype]}: loss {el:.3g} grad {eg:.3g} ignored row zero: {exact}")
    assert not fails, "\n".join(fails)


@ALL
def test_ce_inplace_grad_shares_storage_and_equals_out_of_place(dtype):
    lg, tgt, dl = N.pl_ce_case(2056, dtype, "peaked", 2049)
    l0, g0, x0 = _ce_run(lg, tgt, dl, 2049)
    l1, g1, x1 = _ce_run(lg, tgt, dl, 2049, inplace=True)
    assert g0.data_ptr() != x0.data_ptr() and torch.equal(x0.detach().cpu(), lg)
    assert g1.data_ptr() == x1.data_ptr()
    assert torch.equal(l0, l1) and torch.equal(g0.view(torch.int32 if dtype == F32 else torch.int16),
                                               g1.view(torch.int32 if dtype == F32 else torch.int16))


# ------------------------------------------------------------------ cross entropy, fused

@HALF
def test_ce_fused_register_counts_and_padding(dtype):
    """ce_fused_kernel<T, NV = 4 | 7 | 8>: V at the edge of thread 1023's first vector (8184 | 8192 |
    8200) and on both sides of each NV boundary; loss and the in-place softmax - onehot against
    float64, padding and the ignored row exactly zero, two runs bitwise equal."""
    C, tol, fails = _C(), N.PL_CEF_TOL[dtype], []
    for V in N.PL_CEF_V:
        for vv in (0, V - 1, V - 8, 1):
            if not 0 <= vv < V:
                continue
            lg, tgt, _ = N.pl_ce_case(V, dtype, "peaked", vv, rows=5)
            tgt[2] = -100
            rl, rd, rmax, fl = N.pl_ce_ref(lg, tgt, None, vv)
            x, x2, t = lg.to(DEV).clone(), lg.to(DEV).clone(), tgt.to(DEV)
            loss, loss2 = C.ce_fused(x, t, -100, vv), C.ce_fused(x2, t, -100, vv)
            el, ed = N.ce_loss_err(loss, rl, rmax), N.row_rel_err(x, rd, row_floor=fl)
            exact = bool((x[:, vv or V:] == 0).all() and (x[2] == 0).all() and loss[2] == 0)
            same = torch.equal(x.view(torch.int16), x2.view(torch.int16)) and torch.equal(loss, loss2)
            _report(fails, el <= tol["loss"] and ed <= tol["d"] and exact and same,
                    f"ce_fused {_NAME[dtype]} V={V} vvalid={vv} NV={4 if V <= 32768 else 7 if V <= 57344 else 8}: loss {el:.3g} "
                    f"(tol {tol['loss']:.3g}) d {ed:.3g} (tol {tol['d']:.3g}) zeros exact: {exact} runs equal: {same}")
    assert not fails, "\n".join(fails)


def test_ce_fused_rejects_what_it_has_no_kernel_for():
    C = _C()
    t = torch.zeros(2, dtype=torch.long, device=DEV)
    with pytest.raises(RuntimeError, match="ce_fused"):
        C.ce_fused(torch.zeros(2, 65544, device=DEV, dtype=BF), t, -100, 0)
    with pytest.raises(RuntimeError, match="ce_fused"):
        C.ce_fused(torch.zeros(2, 1024, device=DEV, dtype=F32), t, -100, 0)
    with pytest.raises(RuntimeError, match="ce_fused_local"):
        C.ce_fused_local(torch.zeros(2, 1024, device=DEV, dtype=F32), t, 0, 0)
    torch.cuda.synchronize()


@HALF
@pytest.mark.parametrize("V,vv", [(8200, 0), (8200, 8193), (32776, 32769)])
def test_ce_fused_local_statistics(V, vv, dtype):
    """The vocab-parallel form: targets below, inside, above the slice and in its padding.
    stats[0] is the row max of the valid columns exactly, stats[2] the target logit exactly (or 0),
    stats[1] and e = exp(x - m) within tolerance, e exactly 0 on padding."""
    tol = N.PL_CEF_TOL[dtype]
    lg, _, _ = N.pl_ce_case(V, dtype, "peaked", vv, rows=5)
    nv, vstart = vv or V, 3 * V
    tgt = torch.tensor([vstart - 3, vstart + 5, vstart + V + 2, vstart + nv - 1, vstart + min(nv + 1, V - 1)])
    x = lg.to(DEV).clone()
    st = _C().ce_fused_local(x, tgt.to(DEV), vstart, vv).cpu()
    re_, rs = N.ce_local_ref(lg, vv)
    want_t = torch.tensor([0.0, lg[1, 5].item(), 0.0, lg[3, nv - 1].item(), 0.0 if vv else lg[4, V - 1].item()])
    ee = N.row_rel_err(x, re_)
    es = ((st[1].double() - rs).abs() / rs).max().item()
    print(f"ce_fused_local {_NAME[dtype]} V={V} vvalid={vv}: e {ee:.3g} (tol {tol['d']:.3g}) sum {es:.3g} (tol {tol['sum']:.3g})")
    assert torch.equal(st[0], lg[:, :nv].float().amax(-1))
    assert torch.equal(st[2], want_t)
    assert (x[:, nv:] == 0).all()
    assert ee <= tol["d"] and es <= tol["sum"]


# ----------------------------------------------------------------------------------- RoPE

# name, pos_div, pos_mod = s, table rows (exactly s: the last row is read; or more). b = 3, s = 5.
_LAYOUTS = (("sb", 3, 5, 5), ("bs", 1, 5, 9))
_B, _S = 3, 5


def _tables(rows, rot):
    return SF.rope_tables(rows, rot, base=N.PL_ROPE_BASE, device=DEV)


@ALL
@pytest.mark.parametrize("nh,d,rot", N.PL_ROPE_SHAPES, ids=[f"nh{a}-d{b}-rot{c}" for a, b, c in N.PL_ROPE_SHAPES])
def test_rope_forward_backward_roundtrip(nh, d, rot, dtype):
    """``rope_`` and ``apply_rope`` with its autograd backward, in the [s, b] (pos_div = b) and
    [b, s] (pos_div = 1) layouts, on both kernels and with partial rotary: forward against the
    float64 rotation, backward against its inverse applied to dy, forward then inverse back to x;
    elements [rot, d) bitwise unchanged."""
    C, tol, fails = _C(), N.PL_ROPE_TOL[dtype], []
    g = _gen(23 + nh + rot)
    for name, pdiv, s, trows in _LAYOUTS:
        cos, sin = _tables(trows, rot)
        x = torch.randn(_B * _S, nh, d, generator=g).to(dtype).to(DEV)
        dy = torch.randn(_B * _S, nh, d, generator=g).to(dtype).to(DEV)
        y = x.clone()
        C.rope_(y, cos, sin, rot, pdiv, s, False)
        xg = x.clone().requires_grad_()
        ya = SF.apply_rope(xg, cos, sin, pdiv, s, rot)
        ya.backward(dy)
        back = y.clone()
        C.rope_(back, cos, sin, rot, pdiv, s, True)
        ef = N.row_rel_err(y, N.rope_ref(x, cos, sin, rot, pdiv, s))
        eb = N.row_rel_err(xg.grad, N.rope_ref(dy, cos, sin, rot, pdiv, s, inverse=True))
        er = N.row_rel_err(back, x.double())
        tails = (torch.equal(y[..., rot:], x[..., rot:]) and torch.equal(xg.grad[..., rot:], dy[..., rot:])
                 and torch.equal(back[..., rot:], x[..., rot:]) and torch.equal(ya.detach(), y))
        _report(fails, ef <= tol["rot"] and eb <= tol["rot"] and er <= tol["roundtrip"] and tails,
                f"rope {N.rope_kernel_for(nh, rot)} {_NAME[dtype]} nh={nh} d={d} rot={rot} [{name}]: fwd {ef:.3g} bwd {eb:.3g} "
                f"(tol {tol['rot']:.3g}) roundtrip {er:.3g} (tol {tol['roundtrip']:.3g}) tails / apply_rope bitwise: {tails}")
    assert not fails, "\n".join(fails)


@ALL
def test_rope_grid_stride_second_trip(dtype):
    """nh = 1, rot = d = 16, 524,293 tokens: 5 work items past the 2048 blocks x 256 threads of the
    grid-stride kernel, so its loop makes a second trip."""
    ntok, pdiv, s = 524293, 3, 1031
    cos, sin = _tables(s, 16)
    x = torch.randn(ntok, 1, 16, generator=_gen(3)).to(dtype).to(DEV)
    y = x.clone()
    _C().rope_(y, cos, sin, 16, pdiv, s, False)
    ref = N.rope_ref(x, cos, sin, 16, pdiv, s)
    e, e_tail = N.row_rel_err(y, ref), N.row_rel_err(y[-8:], ref[-8:])
    print(f"rope grid second trip {_NAME[dtype]}: {e:.3g}, last 8 tokens {e_tail:.3g} (tol {N.PL_ROPE_TOL[dtype]['rot']:.3g})")
    assert e <= N.PL_ROPE_TOL[dtype]["rot"] and e_tail <= N.PL_ROPE_TOL[dtype]["rot"]


@pytest.mark.parametrize("nh", [2, 4], ids=["grid", "tok"])
def test_rope_inside_a_fused_qkv_row(nh):
    """The strided q + k view inside a wider [tokens, 3 nh d] row, whole and as a row-offset slice
    (the length-grouped SFT path): the heads are rotated, the rest of the buffer is bitwise unchanged."""
    d, ntok, tol = 128, _B * _S, N.PL_ROPE_TOL[BF]["rot"]
    cos, sin = _tables(_S, d)
    buf0 = torch.randn(ntok, 3 * nh * d, generator=_gen(8)).bfloat16().to(DEV)
    for o, n in ((0, ntok), (4, 9)):
        buf = buf0.clone()
        view = buf[o:o + n, :2 * nh * d].view(n, 2 * nh, d)
        assert not view.is_contiguous()
        _C().rope_(view, cos, sin, d, _B, _S, False)
        ref = N.rope_ref(buf0[o:o + n, :2 * nh * d].reshape(n, 2 * nh, d), cos, sin, d, _B, _S)
        e = N.row_rel_err(view, ref)
        print(f"rope qkv view nh={nh} rows {o}..{o + n}: {e:.3g} (tol {tol:.3g})")
        assert e <= tol
        assert torch.equal(buf[:, 2 * nh * d:], buf0[:, 2 * nh * d:])
        assert torch.equal(buf[:o], buf0[:o]) and torch.equal(buf[o + n:], buf0[o + n:])


def test_apply_rope_fallbacks_equal_the_reference():
    """rot % 16 != 0 has no kernel (PyTorch path); a non-unit last stride is made contiguous first."""
    g = _gen(9)
    cos, sin = _tables(_S, 24)
    x = torch.randn(_B * _S, 4, 32, generator=g).bfloat16().to(DEV)
    e1 = N.row_rel_err(SF.apply_rope(x, cos, sin, _B, _S, 24), N.rope_ref(x, cos, sin, 24, _B, _S))
    cos, sin = _tables(_S, 32)
    xs = torch.randn(_B * _S, 4, 64, generator=g).bfloat16().to(DEV)[..., ::2]
    assert xs.stride(-1) == 2
    e2 = N.row_rel_err(SF.apply_rope(xs, cos, sin, _B, _S, 32), N.rope_ref(xs, cos, sin, 32, _B, _S))
    print(f"apply_rope fallbacks: rot 24 {e1:.3g}, strided {e2:.3g} (tol {N.PL_ROPE_TOL[BF]['rot']:.3g})")
    assert e1 <= N.PL_ROPE_TOL[BF]["rot"] and e2 <= N.PL_ROPE_TOL[BF]["rot"]
    with pytest.raises(RuntimeError, match="rope"):
        _C().rope_(x, cos[:, :12].contiguous(), sin[:, :12].contiguous(), 24, _B, _S, False)


# ---------------------------------------------------------------- bias + GeLU, d(bias)

def _act_check(fails, what, dtype, key, x, b, dy, act, want_db=False):
    tol = N.PL_ACT_TOL[dtype][key]
    xd, bd, dyd = x.to(DEV), None if b is None else b.to(DEV), dy.to(DEV)
    y = _C().bias_act_fwd(xd, bd, act)
    dx, db = _C().bias_act_bwd(dyd, xd, bd, act, want_db, None)
    ry, rdx = N.bias_act_ref(x, b, dy, act)
    ey, edx = N.row_rel_err(y, ry), N.row_rel_err(dx, rdx)
    fin = bool(torch.isfinite(y).all() and torch.isfinite(dx).all())
    _report(fails, ey <= tol and edx <= tol and fin and (want_db or db.numel() == 0),
            f"bias_act {what} {_NAME[dtype]} act={act}: y {ey:.3g} dx {edx:.3g} (tol {tol:.3g}) finite: {fin}")
    return dx, db


@ALL
@pytest.mark.parametrize("act", [0, 1], ids=["tanh", "erf"])
def test_bias_gelu_forward_and_dx_row_tails(act, dtype):
    """bias_act_fwd_kernel / bias_act_bwd_kernel without d(bias) (4 rows per thread): every row tail,
    N on both sides of a 2048-column block, bias given and None; 262,141 rows make a 5-row slice
    (one batch of 4 plus a tail of 1) past grid.y's 65535 slices."""
    fails = []
    for rows in N.PL_ACT_ROWS:
        for n in N.PL_ACT_N:
            for bias in (True, False):
                x, b, dy = N.act_case(rows, n, dtype, bias=bias)
                _act_check(fails, f"rows={rows} N={n} bias={bias}", dtype, "gelu", x, b, dy, act)
    x, b, dy = N.act_case(262141, 8, dtype)
    _act_check(fails, "rows=262141 N=8", dtype, "gelu", x, b, dy, act)
    assert not fails, "\n".join(fails)


@ALL
@pytest.mark.parametrize("act", [0, 1], ids=["tanh", "erf"])
def test_bias_gelu_saturation(act, dtype):
    """z in +-6, +-12, +-40, +-1e4 (+-65504 for fp16): no NaN, values and derivatives at the float64 limits."""
    fails = []
    x, dy = N.gelu_saturation_case(dtype)
    _act_check(fails, "saturated z", dtype, "saturation", x, None, dy, act)
    assert not fails, "\n".join(fails)


@ALL
@pytest.mark.parametrize("rows,n", N.PL_DBIAS_SHAPES, ids=[f"{r}x{n}" for r, n in N.PL_DBIAS_SHAPES])
def test_bias_gelu_dbias_fresh_and_accumulated(rows, n, dtype):
    """d(bias) against the float64 column sum of the kernel's own rounded dx (isolates the two-phase
    reduce), fresh and accumulated into a pre-filled fp32 buffer (old + sum); dx against the
    reference; ``want_dbias=False`` returns the empty tensor."""
    fails = []
    x, b, dy = N.act_case(rows, n, dtype)
    dx, db = _act_check(fails, f"d(bias) rows={rows} N={n}", dtype, "gelu", x, b, dy, 0, want_db=True)
    ref, sc = N.col_sum_ref(dx)
    pre = 10.0 * torch.randn(n, generator=_gen(rows))
    acc = pre.to(DEV)
    dx2, db2 = _C().bias_act_bwd(dy.to(DEV), x.to(DEV), b.to(DEV), 0, True, acc)
    refp, scp = N.col_sum_ref(dx, pre)
    e1, e2 = N.col_rel_err(db, ref, sc), N.col_rel_err(acc, refp, scp)
    _report(fails, e1 <= N.PL_COL_TOL and e2 <= N.PL_COL_TOL and db.dtype == F32,
            f"d(bias) {_NAME[dtype]} rows={rows} N={n} slices={N.bias_act_slices(rows, n)}: fresh {e1:.3g} accumulated {e2:.3g} "
            f"(tol {N.PL_COL_TOL:.3g})")
    assert db2.data_ptr() == acc.data_ptr() and torch.equal(dx2, dx)
    assert _C().bias_act_bwd(dy.to(DEV), x.to(DEV), b.to(DEV), 0, False, None)[1].numel() == 0
    assert not fails, "\n".join(fails)


def test_bias_gelu_autograd_accumulates_into_main_grad():
    """``SF.bias_gelu`` with a bias that owns an fp32 ``main_grad``: the backward adds d(bias) to it,
    reports the parameter ready and returns no bias gradient."""
    x, b, dy = N.act_case(1025, 8, BF)
    pre = 10.0 * torch.randn(8, generator=_gen(1))
    bias = torch.nn.Parameter(b.to(DEV))
    bias.main_grad = pre.to(DEV)
    ready = []
    bias._smdt_grad_ready = ready.append
    xg = x.to(DEV).requires_grad_()
    y = SF.bias_gelu(xg, bias, "tanh")
    y.backward(dy.to(DEV))
    ry, rdx = N.bias_act_ref(x, b, dy, 0)
    refp, scp = N.col_sum_ref(xg.grad, pre)
    e = N.col_rel_err(bias.main_grad, refp, scp)
    print(f"bias_gelu autograd main_grad: {e:.3g} (tol {N.PL_COL_TOL:.3g})")
    assert bias.grad is None and len(ready) == 1 and ready[0] is bias and e <= N.PL_COL_TOL
    assert N.row_rel_err(y, ry) <= N.PL_ACT_TOL[BF]["gelu"] and N.row_rel_err(xg.grad, rdx) <= N.PL_ACT_TOL[BF]["gelu"]
    # a plain tensor bias: d(bias) comes back in the bias' dtype
    b2 = b.to(DEV).requires_grad_()
    SF.bias_gelu(x.to(DEV), b2, "none").backward(dy.to(DEV))
    assert b2.grad.dtype == BF and b2.grad.shape == b.shape


# --------------------------------------------------------------------------------- SwiGLU

@ALL
def test_swiglu_forward_and_both_gradient_halves(dtype):
    """swiglu_fwd_kernel / swiglu_bwd_kernel: F on both sides of a column block, 65,537 rows for the
    row loop past grid.y, gates of +-100 (saturation, no NaN); y, d gate and d up against float64."""
    tol, fails = N.PL_ACT_TOL[dtype]["swiglu"], []
    for rows, F in [(r, f) for r in (1, 3) for f in N.PL_ACT_N] + [(65537, 8)]:
        x, dy = N.swiglu_case(rows, F, dtype)
        x[0, :8], x[-1, :8] = 100.0, -100.0
        xg = x.to(DEV).requires_grad_()
        y = SF.swiglu(xg)
        y.backward(dy.to(DEV))
        ry, rdx = N.swiglu_ref(x, dy)
        dx = xg.grad
        e = (N.row_rel_err(y, ry), N.row_rel_err(dx[:, :F], rdx[:, :F]), N.row_rel_err(dx[:, F:], rdx[:, F:]))
        fin = bool(torch.isfinite(y).all() and torch.isfinite(dx).all())
        _report(fails, max(e) <= tol and fin and y.shape == (rows, F),
                f"swiglu {_NAME[dtype]} rows={rows} F={F}: y {e[0]:.3g} dgate {e[1]:.3g} dup {e[2]:.3g} (tol {tol:.3g}) finite: {fin}")
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------- bias_grad on its own

@ALL
def test_bias_grad_overwrite_and_accumulate(dtype):
    """col_sum_rows_kernel + the slab reduce (``parallel/dense.py`` calls it on the training path):
    per column against float64, overwriting and accumulating."""
    fails = []
    for rows in (1, 7, 1025):
        for n in (8, 2056):
            dy = N.act_case(rows, n, dtype)[2]
            pre = 10.0 * torch.randn(n, generator=_gen(rows + n))
            out, acc = pre.to(DEV), pre.to(DEV)
            _C().bias_grad(dy.to(DEV), out, False)
            _C().bias_grad(dy.to(DEV), acc, True)
            (ref, sc), (refp, scp) = N.col_sum_ref(dy), N.col_sum_ref(dy, pre)
            e1, e2 = N.col_rel_err(out, ref, sc), N.col_rel_err(acc, refp, scp)
            _report(fails, e1 <= N.PL_COL_TOL and e2 <= N.PL_COL_TOL,
                    f"bias_grad {_NAME[dtype]} rows={rows} N={n}: overwrite {e1:.3g} accumulate {e2:.3g} (tol {N.PL_COL_TOL:.3g})")
    assert not fails, "\n".join(fails)


# ----------------------------------------------------------------------------- row gather

@pytest.mark.parametrize("cols", [8, 512, 520], ids=["16B", "1024B", "1040B"])
def test_gather_rows_bitwise(cols):
    """Row bytes 16 / 1024 / 1040 (a second chunk with one lane); 1, 8 and 9 destination rows (9 is
    past one block's 8 waves); -1, an index >= nsrc and duplicates in the map. Bitwise (integer
    view, NaN patterns included) against index_select with zero rows."""
    nsrc = 5
    bits = torch.randint(-32768, 32768, (nsrc, cols), generator=_gen(cols), dtype=torch.int32).to(torch.int16)
    bits[0, 0], bits[1, 1] = 0x7FC1, -1                   # NaN patterns
    src = bits.view(torch.bfloat16).to(DEV)
    for m in ([3], [-1], [nsrc], [3, -1, 3, 7, 0, 4, 4, -5], [3, -1, 3, 7, 0, 4, 4, -5, 1]):
        mp = torch.tensor(m)
        live = (mp >= 0) & (mp < nsrc)
        want = bits.index_select(0, mp.clamp(0, nsrc - 1)) * live[:, None].to(torch.int16)
        out = _C().gather_rows(src, mp.to(DEV))
        assert out.shape == (len(m), cols) and out.dtype == torch.bfloat16
        assert torch.equal(out.view(torch.int16).cpu(), want), m


# --------------------------------------------------------------------------- empty inputs

def test_empty_input_gives_empty_output():
    """rows == 0: every launcher of this group returns success and launches nothing."""
    C = _C()
    e = lambda *s, dt=BF: torch.empty(*s, device=DEV, dtype=dt)
    t0 = torch.empty(0, dtype=torch.long, device=DEV)
    lg = e(0, 16).requires_grad_()
    loss = SF.cross_entropy(lg, t0)
    loss.sum().backward()
    assert loss.shape == (0,) and loss.dtype == F32 and lg.grad.shape == (0, 16)
    assert C.ce_fused(e(0, 16), t0, -100, 0).shape == (0,)
    assert C.ce_fused_local(e(0, 16), t0, 0, 0).shape == (3, 0)
    b = torch.ones(16, device=DEV, dtype=BF, requires_grad=True)
    xg = e(0, 16).requires_grad_()
    y = SF.bias_gelu(xg, b)
    y.sum().backward()
    assert y.shape == (0, 16) and xg.grad.shape == (0, 16) and (b.grad == 0).all()
    xs = e(0, 32).requires_grad_()
    ys = SF.swiglu(xs)
    ys.sum().backward()
    assert ys.shape == (0, 16) and xs.grad.shape == (0, 32)
    cos, sin = _tables(4, 32)
    xr = e(0, 4, 32).requires_grad_()
    yr = SF.apply_rope(xr, cos, sin, 1, 4)
    yr.sum().backward()
    assert yr.shape == (0, 4, 32) and xr.grad.shape == (0, 4, 32)
    out = torch.full((16,), 3.0, device=DEV)
    C.bias_grad(e(0, 16), out, True)
    assert (out == 3).all()
    C.bias_grad(e(0, 16), out, False)
    assert (out == 0).all()
    assert C.gather_rows(torch.ones(5, 8, device=DEV, dtype=BF), t0).shape == (0, 8)
    torch.cuda.synchronize()
