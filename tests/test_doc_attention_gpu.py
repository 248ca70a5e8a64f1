"""Per-document flash attention (the DOC variants of flash_attn.hip) on the GPU: forward and
dq / dk / dv against the fp32 ``attention_ref`` with the same ``doc_start``, the fused-QKV and padded
entry points, a GPT step against the CPU reference path, and HIP-graph capture. Tolerances are
those of ``test_flash_attention`` in tests/test_kernels_gpu.py."""
import functools
import math

import pytest
import torch

import _numerics as N
from smdt_amd.ops import functional as SF
from smdt_amd.train.utils import document_ends, document_starts

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, S = 2, 512

# doc_start change points of batch row 0 (row 1 has no boundary: per-batch indexing)
BOUNDARIES = {
    "70": [70],            # inside a 32-row wave, off any tile edge: rows with a fully masked first tile
    "192": [192],          # on a 64-key tile edge
    "256": [256],          # on a 128-row block edge: whole tiles skipped, nothing to mask
    "300_301": [300, 301], # a one-token document
    "511": [511],          # the last token alone
}


def _doc_start(points, b=B, s=S, device=DEV):
    ds = torch.zeros(b, s, dtype=torch.int32, device=device)
    for p in points:
        ds[0, p:] = p
    return ds


@functools.lru_cache(maxsize=None)
def _inputs(heads, D, dt):
    """q, k, v and dO of one shape: made once, shared by every boundary / dropout case, never
    written to (each test works on detached views that require grad)."""
    H, Hkv = heads
    g = torch.Generator(device=DEV).manual_seed(10 + D + H)
    mk = lambda h: torch.randn(B, S, h, D, device=DEV, dtype=dt, generator=g)
    return mk(H), mk(Hkv), mk(Hkv), mk(H)


def _rows_check(got, q, k, v, do, scale, p=0.0, keep=None, ds=None):
    """The row-relative criterion of tests/test_flash_score_range_gpu.py beside the global one: per
    row within 2 x the error of the kernels' rounding points against float64 attention + one ulp
    at the row's max, so a single wrong row cannot hide under 0.05 * max|ref|. ``got``: o, dq, dk,
    dv as [B, S, heads, D]."""
    ref = N.flash_ref(q, k, v, do, scale, True, p, keep, ds)
    emu = N.flash_emulation_at_kernel_max(q, k, v, do, scale, True, p, keep, ds)
    N.assert_flash_close(dict(zip(("o", "dq", "dk", "dv"), got)), emu, ref, q.dtype, names=("o", "dq", "dk", "dv"),
                         what="doc", floors=N.flash_grad_floors(q, k, v, do, scale, True, p, keep, ds))


def _check(o, orf, pairs, rows=None):
    """``rows`` = (q, k, v, do, scale, p, keep, doc_start) adds ``_rows_check`` on o and the pairs'
    gradients (dq, dk, dv)."""
    assert torch.isfinite(o.float()).all()
    torch.testing.assert_close(o.float(), orf, atol=2e-2, rtol=2e-2)
    for a, r in pairs:
        assert torch.isfinite(a.float()).all()
        err = (a.float() - r).abs().max().item()
        assert err < 0.05 * max(1.0, r.abs().max().item()), err
    if rows is not None:
        _rows_check([o.detach()] + [a for a, _ in pairs], *rows)


def _kernel_vs_ref(points, heads, D, dt, p):
    q0, k0, v0, do = _inputs(heads, D, dt)
    q, k, v = (t.detach().clone().requires_grad_() for t in (q0, k0, v0))
    ds = _doc_start(points)
    scale = 1 / math.sqrt(D)
    seed, off = 4321, 9
    o = SF._FlashAttn.apply(q, k, v, scale, True, p, seed, off, ds, document_ends(ds))
    keep = SF.flash_dropout_keep_mask(B, heads[0], S, p, seed, off, DEV) if p > 0 else None
    qr, kr, vr = (t.detach().float().requires_grad_() for t in (q, k, v))
    orf = SF.attention_ref(qr, kr, vr, scale, True, p, keep, doc_start=ds)
    o.backward(do)
    orf.backward(do.float())
    _check(o, orf, [(a.grad, r.grad) for a, r in ((q, qr), (k, kr), (v, vr))],
           rows=(q0, k0, v0, do, scale, p, keep, ds))


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("heads", [(4, 4), (8, 2)])
@pytest.mark.parametrize("bound", list(BOUNDARIES))
def test_doc_flash_attention_bf16(bound, heads, D, p):
    _kernel_vs_ref(BOUNDARIES[bound], heads, D, torch.bfloat16, p)


@pytest.mark.parametrize("bound", list(BOUNDARIES))
def test_doc_flash_attention_fp16(bound):
    _kernel_vs_ref(BOUNDARIES[bound], (8, 2), 64, torch.float16, 0.1)


def test_doc_flash_attention_all_boundaries_at_once():
    """Every change point of the table in one row: consecutive straddling tiles, a document that
    starts and ends inside one wave, and blocks whose sweep starts mid-sequence."""
    pts = sorted(p for v in BOUNDARIES.values() for p in v)
    _kernel_vs_ref(pts, (8, 2), 64, torch.bfloat16, 0.1)
    _kernel_vs_ref(pts, (4, 4), 128, torch.bfloat16, 0.0)


@pytest.mark.parametrize("D", [64, 128])
def test_single_document_is_bit_identical_to_the_causal_kernel(D):
    """``doc_start == 0`` everywhere: same tiles, same order, no mask taken — output and lse equal
    the plain causal kernel's bit for bit."""
    from smdt_amd.ops import _ext
    C = _ext.ext()
    q, k, v, _ = _inputs((8, 2), D, torch.bfloat16)
    scale = 1 / math.sqrt(D)
    ds = torch.zeros(B, S, dtype=torch.int32, device=DEV)
    for p in (0.0, 0.1):
        o0, l0 = C.flash_fwd(q, k, v, scale, True, None, p, 5, 6)
        o1, l1 = C.flash_fwd(q, k, v, scale, True, None, p, 5, 6, ds)
        assert torch.equal(o0, o1) and torch.equal(l0, l1)


def test_binding_checks_the_descriptor():
    from smdt_amd.ops import _ext
    C = _ext.ext()
    q, k, v, _ = _inputs((4, 4), 64, torch.bfloat16)
    ds = torch.zeros(B, S, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="int32"):
        C.flash_fwd(q, k, v, 0.125, True, None, 0.0, 0, 0, ds.long())
    with pytest.raises(RuntimeError, match=r"\[B, S\]"):
        C.flash_fwd(q, k, v, 0.125, True, None, 0.0, 0, 0, ds[:, :256].contiguous())
    with pytest.raises(RuntimeError, match=r"\[B, S\]"):
        C.flash_fwd(q, k, v, 0.125, True, None, 0.0, 0, 0, ds.t().contiguous().t())
    with pytest.raises(RuntimeError, match="causal"):
        C.flash_fwd(q, k, v, 0.125, False, None, 0.0, 0, 0, ds)
    with pytest.raises(RuntimeError):
        C.flash_fwd(q, k, v, 0.125, True, None, 0.0, 0, 0, ds.cpu())


@pytest.mark.parametrize("seq_first", [True, False])
def test_doc_flash_attention_qkv_fused_strides(seq_first, monkeypatch):
    monkeypatch.setenv("SMDT_ASSERT_FLASH", "1")
    torch.manual_seed(11)
    s, b, nh, nkv, hd = 256, 2, 4, 2, 64
    W = (nh + 2 * nkv) * hd
    shape = (s, b, W) if seq_first else (b, s, W)
    qkv = torch.randn(*shape, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    ds = torch.zeros(b, s, dtype=torch.int32, device=DEV)
    ds[0, 70:] = 70
    ds[1, 129:] = 129
    ds[1, 200:] = 200
    o = SF.flash_attention_qkv(qkv, nh, nkv, hd, seq_first=seq_first, causal=True, doc_start=ds)
    do = torch.randn_like(o)
    o.backward(do)
    monkeypatch.delenv("SMDT_ASSERT_FLASH")
    qr = qkv.detach().float().requires_grad_()
    qv, kv, vv = SF._qkv_views(qr, nh, nkv, hd, seq_first)
    orf = SF.attention_ref(qv, kv, vv, 1 / math.sqrt(hd), True, doc_start=ds)          # [b, s, nh, hd]
    orf = (orf.transpose(0, 1) if seq_first else orf).flatten(-2)
    orf.backward(do.float())
    _check(o, orf, [(qkv.grad, qr.grad)])
    unf = lambda t: (t.transpose(0, 1) if seq_first else t).unflatten(-1, (nh, hd))
    _rows_check([unf(o.detach())] + list(SF._qkv_views(qkv.grad, nh, nkv, hd, seq_first)),
                *(t.detach() for t in SF._qkv_views(qkv, nh, nkv, hd, seq_first)), unf(do), 1 / math.sqrt(hd), ds=ds)


def test_doc_flash_attention_padded_length(monkeypatch):
    """S = 200: padded to 256 with the pad rows as a document of their own."""
    monkeypatch.setenv("SMDT_ASSERT_FLASH", "1")
    torch.manual_seed(13)
    b, s, H, Hkv, D = 2, 200, 4, 2, 64
    q = torch.randn(b, s, H, D, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    k = torch.randn(b, s, Hkv, D, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    v = torch.randn(b, s, Hkv, D, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    ds = torch.zeros(b, s, dtype=torch.int32, device=DEV)
    ds[0, 70:] = 70
    ds[0, 199:] = 199
    ds[1, 128:] = 128
    scale = 1 / math.sqrt(D)
    o = SF.flash_attention(q, k, v, scale, True, doc_start=ds)
    do = torch.randn_like(o)
    o.backward(do)
    monkeypatch.delenv("SMDT_ASSERT_FLASH")
    qr, kr, vr = (t.detach().float().requires_grad_() for t in (q, k, v))
    orf = SF.attention_ref(qr, kr, vr, scale, True, doc_start=ds)
    orf.backward(do.float())
    _check(o, orf, [(a.grad, r.grad) for a, r in ((q, qr), (k, kr), (v, vr))],
           rows=(q.detach(), k.detach(), v.detach(), do, scale, 0.0, None, ds))


EOD = 5


@functools.lru_cache(maxsize=None)
def _gpt_reference():
    """The CPU fp32 reference run of the model test (weights, tokens, losses, grads), made once."""
    from smdt_amd.models.gpt import GPTModel
    from smdt_amd.models.transformer import TransformerConfig
    from smdt_amd.parallel import state as ps
    ps.destroy_model_parallel()
    kw = dict(num_layers=2, hidden_size=256, num_attention_heads=4, max_position_embeddings=256,
              padded_vocab_size=1024, hidden_dropout=0.0, attention_dropout=0.0, seed=3)
    ref = GPTModel(TransformerConfig(**kw, params_dtype=torch.float32))
    with torch.no_grad():
        for pr in ref.parameters():
            pr.copy_(pr.to(torch.bfloat16).float())            # what the bf16 model can hold
    g = torch.Generator().manual_seed(4)
    toks = torch.randint(6, 1000, (4, 257), generator=g)
    for i, pos in enumerate((100, 127, 77, 200)):              # one mid-sequence EOD per sample
        toks[i, pos] = EOD
    ds = document_starts(toks[:, :-1], EOD)
    loss = ref(toks[:, :-1], labels=toks[:, 1:], doc_start=ds)
    loss.mean().backward()
    plain = ref(toks[:, :-1], labels=toks[:, 1:]).detach()
    return kw, ref, toks, ds, loss.detach(), plain


@pytest.mark.parametrize("recompute", [False, True])
def test_gpt_step_with_doc_start_matches_cpu_reference(recompute, monkeypatch):
    from smdt_amd.models.gpt import GPTModel
    from smdt_amd.models.transformer import TransformerConfig
    from smdt_amd.parallel import state as ps
    from smdt_amd.parallel.distributed import DistributedDataParallel
    kw, ref, toks, ds, loss_ref, loss_plain = _gpt_reference()
    assert (loss_ref - loss_plain).abs().max() > 0.05          # the boundary matters in this sample
    monkeypatch.setenv("SMDT_ASSERT_FLASH", "1")
    ps.destroy_model_parallel()
    rk = dict(recompute_granularity="full", recompute_method="uniform", recompute_num_layers=1) if recompute else {}
    gpu = GPTModel(TransformerConfig(**kw, **rk, params_dtype=torch.bfloat16), device="cuda")
    with torch.no_grad():
        for pr, pg in zip(ref.parameters(), gpu.parameters()):
            pg.copy_(pr.to(torch.bfloat16))
    ddp = DistributedDataParallel(gpu)
    ddp.zero_grad_buffer()
    loss = gpu(toks[:, :-1].cuda(), labels=toks[:, 1:].cuda(), doc_start=ds.cuda())
    loss.float().mean().backward()
    ddp.finish_grad_sync()
    assert torch.isfinite(loss.float()).all()
    torch.testing.assert_close(loss.float().cpu(), loss_ref, atol=3e-2, rtol=1e-2)
    for (n, pr), pg in zip(ref.named_parameters(), gpu.parameters()):
        err = (pg.main_grad.float().cpu() - pr.grad).norm() / pr.grad.norm().clamp_min(1e-12)
        assert err < 3e-2, (n, err.item())


def test_doc_attention_captured_in_a_graph_matches_eager():
    """Descriptor (from a token tensor, on the device) + forward + backward captured once; two
    replays on different tokens equal the eager runs: nothing in the path syncs with the host, and
    the kernels read the descriptor at run time."""
    torch.manual_seed(17)
    s, b, nh, hd = 256, 2, 4, 64
    qkv = torch.randn(s, b, 3 * nh * hd, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    do = torch.randn(s, b, nh * hd, device=DEV, dtype=torch.bfloat16)
    tok_a = torch.full((b, s), 9, device=DEV)
    tok_b = tok_a.clone()
    tok_a[0, 69] = tok_a[1, 127] = EOD
    tok_b[0, 191] = tok_b[0, 192] = EOD
    static_tok = tok_a.clone()

    def step(tok):
        qkv.grad = None
        ds = document_starts(tok, EOD)
        o = SF.flash_attention_qkv(qkv, nh, nh, hd, seq_first=True, causal=True, doc_start=ds)
        o.backward(do)
        return o.detach(), qkv.grad

    eager = [tuple(t.clone() for t in step(tok)) for tok in (tok_a, tok_b)]
    assert not torch.equal(eager[0][0], eager[1][0])
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        so, sg = step(static_tok)
    for tok, (eo, eg) in zip((tok_a, tok_b), eager):
        static_tok.copy_(tok)
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(so, eo) and torch.equal(sg, eg)
