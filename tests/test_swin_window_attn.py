"""Fused shifted-window attention, CPU side: the torch twin ``window_attention_ref`` states the
kernel's index mapping (gather by source coordinate, region id from the rolled coordinate) and must
reproduce the module's pad / roll / partition op chain; the ``fused`` switch changes no parameter,
buffer or state-dict key anywhere it is threaded through."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from smdt_amd.models import zoo
from smdt_amd.models.swin import ShiftedWindowAttention
from smdt_amd.ops import functional as SF


class _Tap(nn.Module):
    """Stands in for the qkv linear and keeps its output (window-partitioned order) and that
    output's gradient."""

    def __init__(self, weight):
        super().__init__()
        self.weight = weight

    def forward(self, x):
        self.out = F.linear(x, self.weight)
        self.out.retain_grad()
        return self.out


def _to_grid(t, B, ph, pw, ws, shift):
    """[B nW, N, X] in the module's rolled, window-partitioned order -> [B, ph, pw, X] unrolled."""
    t = t.view(B, ph // ws, pw // ws, ws, ws, -1).permute(0, 1, 3, 2, 4, 5).reshape(B, ph, pw, -1)
    return torch.roll(t, shifts=(shift, shift), dims=(1, 2)) if shift > 0 else t


# (window, module shift, ph, pw)
MAPPING_CASES = [(7, 3, 14, 14), (7, 3, 14, 21), (7, 3, 7, 7), (4, 2, 8, 8), (8, 4, 16, 16)]


@pytest.mark.parametrize("ws,shift,ph,pw", MAPPING_CASES)
def test_twin_matches_module_op_chain(ws, shift, ph, pw):
    torch.manual_seed(ws * 100 + ph + pw)
    B, heads, C = 2, 2, 64
    m = ShiftedWindowAttention(C, ws, shift, heads)
    with torch.no_grad():
        m.relative_position_bias_table.normal_(0, 0.5)
    m.qkv = _Tap(torch.randn(3 * C, C) * C ** -0.5)
    m.proj = nn.Identity()
    x = torch.randn(B, ph, pw, C, requires_grad=True)
    dout = torch.randn(B, ph, pw, C)
    out_m = m(x)
    out_m.backward(dout)
    eff = 0 if (ws >= ph and ws >= pw) else shift
    qkv = _to_grid(m.qkv.out.detach(), B, ph, pw, ws, eff).requires_grad_()
    dqkv_m = _to_grid(m.qkv.out.grad, B, ph, pw, ws, eff)
    table = m.relative_position_bias_table.detach().clone().requires_grad_()
    out_t = SF.window_attention_ref(qkv, table, ws, eff, heads)
    out_t.backward(dout)
    torch.testing.assert_close(out_t, out_m, rtol=0, atol=1e-5)
    torch.testing.assert_close(qkv.grad, dqkv_m, rtol=0, atol=1e-5)
    torch.testing.assert_close(table.grad, m.relative_position_bias_table.grad, rtol=0, atol=1e-5)


def test_cpu_op_is_the_twin():
    torch.manual_seed(0)
    qkv, table = torch.randn(1, 8, 8, 192), torch.randn(49, 2)
    torch.testing.assert_close(SF.window_attention(qkv, table, 4, 2, 2),
                               SF.window_attention_ref(qkv, table, 4, 2, 2), rtol=0, atol=0)


@pytest.mark.parametrize("shape", [(2, 8, 8, 64), (2, 9, 15, 64)])
def test_fused_module_equals_unfused(shape):
    torch.manual_seed(1)
    a = ShiftedWindowAttention(64, 7, 3, 2, fused=False)
    with torch.no_grad():
        a.relative_position_bias_table.normal_(0, 0.5)
    b = ShiftedWindowAttention(64, 7, 3, 2, fused=True)
    b.load_state_dict(a.state_dict())
    assert list(a.state_dict()) == list(b.state_dict())
    x = torch.randn(*shape)
    dy = torch.randn(*shape)
    ya, yb = a(x), b(x)
    ya.backward(dy)
    yb.backward(dy)
    torch.testing.assert_close(yb, ya, rtol=1e-5, atol=1e-5)
    for (n, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        torch.testing.assert_close(pb.grad, pa.grad, rtol=1e-4, atol=1e-5, msg=lambda s, n=n: f"{n}: {s}")


def test_zoo_switch_keeps_parameters_and_logits():
    torch.manual_seed(2)
    base = zoo.create("swin_t", 10).eval()
    fused = zoo.create("swin_t", 10, fused_window_attention=True).eval()
    assert all(blk.attn.fused for stage in (fused.features[i] for i in (1, 3, 5, 7)) for blk in stage)
    assert not any(blk.attn.fused for stage in (base.features[i] for i in (1, 3, 5, 7)) for blk in stage)
    assert list(base.state_dict()) == list(fused.state_dict())
    assert sum(p.numel() for p in base.parameters()) == sum(p.numel() for p in fused.parameters())
    fused.load_state_dict(base.state_dict())
    base.load_state_dict(fused.state_dict())
    x = torch.randn(2, 3, 64, 64)
    with torch.no_grad():
        torch.testing.assert_close(fused(x), base(x), rtol=1e-4, atol=1e-5)
    with pytest.raises(TypeError):
        zoo.create("resnet18", 10, fused_window_attention=True)


def test_fused_refuses_attention_dropout():
    with pytest.raises(ValueError):
        ShiftedWindowAttention(64, 7, 3, 2, attention_dropout=0.1, fused=True)
    ShiftedWindowAttention(64, 7, 3, 2, attention_dropout=0.1, fused=False)


@pytest.mark.parametrize("ph,pw,shift", [(14, 14, 3), (14, 21, 3)])
def test_region_ids_reproduce_the_shift_mask(ph, pw, shift):
    m = ShiftedWindowAttention(32, 7, shift, 2)
    with torch.no_grad():
        m.relative_position_bias_table.zero_()
    masked = m._bias(ph, pw, shift, torch.device("cpu"), torch.float32)[:, 0] < -50        # [nW, N, N]
    _, region = SF.window_attention_map(ph, pw, 7, shift)
    assert torch.equal(region[:, :, None] != region[:, None, :], masked)
    assert masked.any() and not masked.all()
