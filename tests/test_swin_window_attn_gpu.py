"""Fused shifted-window attention kernels (csrc/kernels/window_attn.hip) on the GPU.

Numerics are judged against the float64 twin on the same, already rounded inputs, with the module's
existing arithmetic (16-bit bmm, bias add, fp32 softmax, 16-bit bmm) as the yardstick: the kernel's
maximum and Frobenius-relative errors may not exceed twice the yardstick's own. The shapes are the
smallest at which the kernel can go wrong, not the workload's."""
import functools

import pytest
import torch

from smdt_amd.models import zoo
from smdt_amd.models.swin import ShiftedWindowAttention
from smdt_amd.ops import _ext
from smdt_amd.ops import functional as SF

pytestmark = pytest.mark.gpu

# (window, shift, ph, pw, B, heads)
CASES = {
    "ws7_14x14_shift3": (7, 3, 14, 14, 2, 2),      # four windows, wrap in both axes, all nine regions
    "ws7_14x21_shift3": (7, 3, 14, 21, 2, 2),      # nW = 6, ph != pw
    "ws7_7x7_single": (7, 0, 7, 7, 2, 2),          # one window, rows and columns 49..63 padded
    "ws7_b3_h4": (7, 3, 14, 14, 3, 4),             # batch and head strides
    "ws4_8x8_shift2": (4, 2, 8, 8, 2, 2),          # N = 16, 48 padded columns
    "ws8_16x16_shift4": (8, 4, 16, 16, 2, 2),      # N = 64, no padded rows
}
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _yardstick(qkv, table, ws, shift, heads):
    """ShiftedWindowAttention.forward's arithmetic between the qkv and proj linears, on the grid."""
    B, ph, pw, C3 = qkv.shape
    N, C, d = ws * ws, C3 // 3, C3 // 3 // heads
    src, region = SF.window_attention_map(ph, pw, ws, shift, qkv.device)
    nW = src.shape[0]
    x = qkv.reshape(B, ph * pw, 3, heads, d)[:, src.flatten()].view(B, nW, N, 3, heads, d)
    q, k, v = (t.permute(0, 1, 3, 2, 4) for t in x.unbind(3))
    q = q * d ** -0.5
    attn = q.matmul(k.transpose(-2, -1))
    t = torch.arange(N, device=qkv.device)
    c = (t // ws) * (2 * ws - 1) + t % ws
    bias = table[c[:, None] - c[None, :] + 2 * ws * (ws - 1)].permute(2, 0, 1)[None]
    if shift > 0:
        bias = bias + (region[:, :, None] != region[:, None, :]).float().mul(-100.0)[:, None]
    attn = attn + bias.to(attn.dtype)[None]
    attn = torch.softmax(attn.float(), dim=-1).to(q.dtype)
    o = attn.matmul(v).permute(0, 1, 3, 2, 4).reshape(B, nW * N, C)
    return o[:, torch.argsort(src.flatten())].view(B, ph, pw, C)


def _run(fn, qkv, table, dout, *args):
    qkv = qkv.detach().clone().requires_grad_()
    table = table.detach().clone().requires_grad_()
    out = fn(qkv, table, *args)
    out.backward(dout.to(out.dtype))
    return out.detach(), qkv.grad, table.grad


@functools.lru_cache(maxsize=None)
def _case(name, dt):
    ws, shift, ph, pw, B, heads = CASES[name]
    g = torch.Generator(device="cuda").manual_seed(sum(map(ord, name + dt)))
    qkv = torch.randn(B, ph, pw, 96 * heads, device="cuda", generator=g).to(DTYPES[dt])
    table = torch.randn((2 * ws - 1) ** 2, heads, device="cuda", generator=g) * 0.5
    dout = torch.randn(B, ph, pw, 32 * heads, device="cuda", generator=g).to(DTYPES[dt])
    ref = _run(SF.window_attention_ref, qkv.double(), table.double(), dout.double(), ws, shift, heads)
    return qkv, table, dout, ref


def _errs(x, ref):
    e = (x.double() - ref).abs()
    return e.max().item(), (e.norm() / ref.norm()).item()


def _check(tag, got, yard, ref):
    bad = []
    for what, a, b, r in zip(("out", "dqkv", "dtable"), got, yard, ref):
        (amax, afro), (bmax, bfro) = _errs(a, r), _errs(b, r)
        print(f"{tag} {what}: kernel max {amax:.3e} fro {afro:.3e} | yardstick max {bmax:.3e} fro {bfro:.3e}")
        if not (amax <= 2 * bmax and afro <= 2 * bfro):
            bad.append(what)
    assert not bad, f"{tag}: kernel error above 2x the op chain's for {bad}"


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", list(CASES))
def test_numerics_against_float64_twin(name, dt):
    ws, shift, _, _, _, heads = CASES[name]
    qkv, table, dout, ref = _case(name, dt)
    got = _run(SF._WindowAttn.apply, qkv, table, dout, ws, shift, heads)
    yard = _run(_yardstick, qkv, table, dout, ws, shift, heads)
    assert got[0].dtype == qkv.dtype and got[1].dtype == qkv.dtype and got[2].dtype == torch.float32
    _check(f"[{name} {dt}]", got, yard, ref)


def test_shift_mask_isolates_regions():
    ws, shift, ph, pw, B, heads = CASES["ws7_14x14_shift3"]
    qkv, table, _, _ = _case("ws7_14x14_shift3", "bf16")
    src, region = SF.window_attention_map(ph, pw, ws, shift, "cuda")
    win = src.shape[0] - 1                                   # bottom-right window: four regions
    assert region[win].unique().numel() == 4
    key = 0
    poked = qkv.clone().view(B, ph * pw, 3, heads, 32)
    poked[:, src[win, key], 2] = 1e4                         # this key's v, every head
    tf = table.float()
    C = _ext.ext()
    base = C.window_attn_fwd(qkv, tf, ws, shift, heads)[0].view(B, ph * pw, -1)
    out = C.window_attn_fwd(poked.view_as(qkv), tf, ws, shift, heads)[0].view(B, ph * pw, -1)
    other = src[win][region[win] != region[win, key]]
    same = src[win][region[win] == region[win, key]]
    # a masked pair's probability is below exp(-100) times the row's largest: nothing reaches the row
    assert torch.equal(out[:, other], base[:, other])
    assert (out[:, same] - base[:, same]).abs().max() > 1.0
    rest = torch.ones(ph * pw, dtype=torch.bool, device="cuda")
    rest[src[win]] = False
    assert torch.equal(out[:, rest], base[:, rest])


@pytest.mark.parametrize("name", ["ws7_14x21_shift3", "ws8_16x16_shift4"])
def test_backward_is_deterministic(name):
    ws, shift, _, _, _, heads = CASES[name]
    qkv, table, dout, _ = _case(name, "bf16")
    C = _ext.ext()
    tf = table.float()
    _, lse = C.window_attn_fwd(qkv, tf, ws, shift, heads)
    a = C.window_attn_bwd(qkv, tf, lse, dout, ws, shift, heads)
    b = C.window_attn_bwd(qkv, tf, lse, dout, ws, shift, heads)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("why,shape,ws,shift,heads,dtype", [
    ("d16", (2, 14, 14, 96), 7, 3, 2, torch.bfloat16),
    ("ws9", (2, 9, 9, 192), 9, 0, 2, torch.bfloat16),
    ("fp32", (2, 14, 14, 192), 7, 3, 2, torch.float32),
])
def test_refusals(why, shape, ws, shift, heads, dtype, monkeypatch):
    torch.manual_seed(0)
    qkv = torch.randn(*shape, device="cuda").to(dtype)
    table = torch.randn((2 * ws - 1) ** 2, heads, device="cuda")
    with pytest.raises(RuntimeError, match="window_attn"):
        _ext.ext().window_attn_fwd(qkv, table, ws, shift, heads)
    with pytest.raises(RuntimeError, match="window_attn"):
        _ext.ext().window_attn_bwd(qkv, table, torch.zeros(1, device="cuda"), qkv, ws, shift, heads)

    def no_kernel(*a):
        raise AssertionError("the kernel path was taken")
    monkeypatch.setattr(SF._WindowAttn, "apply", no_kernel)
    assert torch.equal(SF.window_attention(qkv, table, ws, shift, heads),
                       SF.window_attention_ref(qkv, table, ws, shift, heads))


def _module_run(m, x, dy, autocast):
    m.zero_grad(set_to_none=True)
    x = x.detach().clone().requires_grad_()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        y = m(x)
    y.backward(dy.to(y.dtype))
    return [y.detach(), x.grad] + [p.grad.clone() for p in m.parameters()]


def test_module_under_autocast():
    torch.manual_seed(3)
    a = ShiftedWindowAttention(128, 7, 3, 4).cuda()
    with torch.no_grad():
        a.relative_position_bias_table.normal_(0, 0.5)
    b = ShiftedWindowAttention(128, 7, 3, 4, fused=True).cuda()
    b.load_state_dict(a.state_dict())
    x = torch.randn(2, 9, 15, 128, device="cuda")
    dy = torch.randn(2, 9, 15, 128, device="cuda")
    ref = [t.double() for t in _module_run(a, x, dy, False)]
    yard = _module_run(a, x, dy, True)
    got = _module_run(b, x, dy, True)
    names = ["out", "dx"] + [n for n, _ in a.named_parameters()]
    bad = []
    for n, g, y, r in zip(names, got, yard, ref):
        (gm, gf), (ym, yf) = _errs(g, r), _errs(y, r)
        print(f"[module bf16 autocast] {n}: fused max {gm:.3e} fro {gf:.3e} | unfused max {ym:.3e} fro {yf:.3e}")
        if not (gm <= 2 * ym and gf <= 2 * yf):
            bad.append(n)
    assert not bad, bad


def test_graph_capture_matches_eager():
    """Forward + backward of the fused swin_t block stack (every stage, patch merging, norm, head) on
    the patch embedding of a [2, 3, 64, 64] batch: two replays with new inputs equal eager bit for bit."""
    torch.manual_seed(4)
    m = zoo.create("swin_t", 10, fused_window_attention=True, stochastic_depth_prob=0.0).cuda()
    embed, stack = m.features[0], m.features[1:]
    params = [p for mod in (stack, m.norm, m.head) for p in mod.parameters()]
    names = [n for n, _ in m.named_parameters() if not n.startswith("features.0.")]

    def tokens(seed):
        x = torch.randn(2, 3, 64, 64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))
        with torch.no_grad():
            return embed(x)

    def step(t):
        with torch.autocast("cuda", dtype=torch.bfloat16, cache_enabled=False):
            y = m.head(m.flatten(m.avgpool(m.permute(m.norm(stack(t))))))
        y.float().square().mean().backward()
        return y

    static_t = tokens(4)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            m.zero_grad(set_to_none=True)
            step(static_t)
    torch.cuda.current_stream().wait_stream(side)
    m.zero_grad(set_to_none=True)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static_y = step(static_t)
    static_grads = [p.grad for p in params]
    assert all(s is not None for s in static_grads)
    for seed in (5, 6):
        t = tokens(seed)
        static_t.copy_(t)
        g.replay()
        gy, gg = static_y.clone(), [s.clone() for s in static_grads]
        for p in params:
            p.grad = None
        ey = step(t)
        assert torch.equal(gy, ey)
        differ = [n for n, p, a in zip(names, params, gg) if not torch.equal(a, p.grad)]
        assert not differ, differ
        for p, s in zip(params, static_grads):
            p.grad = s
