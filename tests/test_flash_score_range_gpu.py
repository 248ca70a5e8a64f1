"""Flash attention at scores that move the forward's lazy reference max (flash_attn.hip).

``N.flash_score_case`` puts a chosen natural-log level on every (query, 64-key tile): far above and
below the window inside which ``fwd_kernel`` leaves its reference max alone, above fp16's maximum
and below its minimum while inside bf16's window, with only every other lane of a wave affected.
Forward ``o`` and ``lse`` and ``dq`` / ``dk`` / ``dv`` are judged against float64 attention on the
same 16-bit inputs: everything finite, and row by row the error within 2 x the error that
``N.flash_emulation_at_kernel_max`` (float64 attention with only the kernels' rounding points, P
rounded at the forward's lazy reference max) has in the same row + one ulp of the 16-bit type + for
the gradients the rounding floor of the row (``N.flash_grad_floors``); the issue's wording (2 x the
emulation's worst row + one ulp) is checked beside it (``N.flash_excess``). The CPU twins of the forward and
the proof that this criterion rejects a broken rescue and wrong gradient rows are in tests/test_numerics_sensitivity.py;
measured kernel / emulation ratios in profiles/flash_score_range/README.md.
"""
import pytest
import torch

import _numerics as N

pytestmark = pytest.mark.gpu

DEV = "cuda"
SCALE = N.FLASH_SCALE
PROFILES = sorted(N.FLASH_PROFILES)


def _kernels(q, k, v, do, causal, p=0.0, seed=0, off=0, doc_start=None):
    """o, lse, dq, dk, dv of the HIP kernels ([B, S, heads, D]; lse fp32 [B, H, S])."""
    from smdt_amd.ops import _ext
    from smdt_amd.ops import functional as SF
    ds, de = SF._doc_args(doc_start, q.shape[1], q.shape[1])
    qg, kg, vg = (t.detach().clone().requires_grad_() for t in (q, k, v))
    o = SF._FlashAttn.apply(qg, kg, vg, SCALE, causal, p, seed, off, ds, de)
    o.backward(do)
    o2, lse = _ext.ext().flash_fwd(q, k, v, SCALE, causal, None, p, seed, off, ds)
    assert torch.equal(o2.view(torch.int16), o.detach().view(torch.int16))   # same bits (NaN included)
    return {"o": o.detach(), "lse": lse, "dq": qg.grad, "dk": kg.grad, "dv": vg.grad}


def _check(profile, dt, causal, heads=(2, 2), D=64, S=256, p=0.0, doc_start=None, what=""):
    from smdt_amd.ops import functional as SF
    H, Hkv = heads
    q, k, v, do = N.flash_score_case(profile, B=2, S=S, H=H, Hkv=Hkv, D=D, dtype=dt, device=DEV)
    seed, off = 4321, 9
    keep = SF.flash_dropout_keep_mask(2, H, S, p, seed, off, DEV) if p > 0 else None
    got = _kernels(q, k, v, do, causal, p, seed, off, doc_start)
    ref = N.flash_ref(q, k, v, do, SCALE, causal, p, keep, doc_start)
    emu = N.flash_emulation_at_kernel_max(q, k, v, do, SCALE, causal, p, keep, doc_start)
    fl = N.flash_grad_floors(q, k, v, do, SCALE, causal, p, keep, doc_start)
    N.assert_flash_close(got, emu, ref, dt, what=f"{what or profile} {dt} D{D} H{H}/{Hkv} causal={causal}", floors=fl)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("heads", [(2, 2), (4, 1)])
@pytest.mark.parametrize("profile", PROFILES)
def test_flash_score_profiles(profile, heads, D, causal, dt):
    """B 2, S 256 (4 key tiles, 2 query blocks), MHA and GQA 4 : 1, both head dims and types."""
    _check(profile, dt, causal, heads, D)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_flash_rescue_across_the_ring_wrap(dt):
    """S 384, D 64: six key tiles through the three-buffer ring, the second upward rescue (tile 2,
    the ring's last slot) and the levels of tiles 3 .. 5 arrive while the ring wraps."""
    _check("up_late", dt, True, (2, 2), 64, S=384)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("profile", ["up_late", "low_start"])
def test_flash_dropout_through_a_rescue(profile, D, dt):
    """Dropout 0.1 with the bit-exact keep mask: l must sum the undropped p through a rescue."""
    _check(profile, dt, True, (4, 1), D, p=0.1, what=profile + " dropout")


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("bounds", [(80, 200), (64, 192)], ids=["in_wave", "tile_edge"])
@pytest.mark.parametrize("profile", ["up_late", "low_start"])
def test_flash_doc_through_a_rescue(profile, bounds, D, dt):
    """Per-document attention: boundaries inside a wave (rows 80, 200: the dead rows of a tile
    share the ballot with rows that ask for the rescue) and on tile edges (64, 192)."""
    ds = torch.zeros(2, 256, dtype=torch.int32, device=DEV)
    for b in bounds:
        ds[:, b:] = b
    ds[1, bounds[1]:] = bounds[0]           # the second sample has one boundary only
    _check(profile, dt, True, (2, 2), D, doc_start=ds, what=f"{profile} doc {bounds}")


def test_flash_qkv_entry_on_up_late():
    """The fused-QKV strided entry (flash_attention_qkv, seq-first) on ``up_late``."""
    from smdt_amd.ops import functional as SF
    dt, H, D, S, B = torch.bfloat16, 4, 64, 256, 2
    q, k, v, do = N.flash_score_case("up_late", B=B, S=S, H=H, Hkv=H, D=D, dtype=dt, device=DEV)
    qkv = torch.cat([t.flatten(-2) for t in (q, k, v)], -1).transpose(0, 1).contiguous().requires_grad_()
    o = SF.flash_attention_qkv(qkv, H, H, D, seq_first=True, causal=True, scale=SCALE)
    o.backward(do.flatten(-2).transpose(0, 1).contiguous())
    dq, dk, dv = SF._qkv_views(qkv.grad, H, H, D, True)
    got = {"o": o.detach().unflatten(-1, (H, D)).transpose(0, 1), "dq": dq, "dk": dk, "dv": dv}
    ref = N.flash_ref(q, k, v, do, SCALE, True)
    emu = N.flash_emulation_at_kernel_max(q, k, v, do, SCALE, True)
    N.assert_flash_close(got, emu, ref, dt, names=("o", "dq", "dk", "dv"), what="up_late qkv",
                         floors=N.flash_grad_floors(q, k, v, do, SCALE, True))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_flash_plain_case_is_a_no_op(dt):
    """The case builder itself changes nothing: on ``plain`` (kb = 0 everywhere) the outputs are
    bitwise those of the same tensors with the reserved channel cleared."""
    from smdt_amd.ops import functional as SF
    q, k, v, do = N.flash_score_case("plain", B=2, S=256, H=4, Hkv=1, D=64, dtype=dt, device=DEV)
    assert (k[..., 0] == 0).all() and (q[:, 1::2, :, 0] == 16).all()
    q0 = q.clone()
    q0[..., 0] = 0
    for causal in (True, False):
        assert torch.equal(SF.flash_attention(q, k, v, SCALE, causal), SF.flash_attention(q0, k, v, SCALE, causal))
