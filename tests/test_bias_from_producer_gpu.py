"""Bias gradients from the kernels that produce a linear's dY (SMDT_BIAS_FROM_PRODUCER): the flash
attention backward emits the token sums of dQ | dK | dV (the QKV bias gradient) and the fc2 dgrad's
GeLU-backward epilogue the column sums of d(pre) (the fc1 bias gradient), both summed in fp32
BEFORE the 16-bit rounding of dY and reduced in a fixed order.

The bound every sum is held to, per column j, against the kernel's own rounded output x (M rows):

    |db[j] - sum_m x[m, j]| <= (eps + M 2^-24) sum_m |x[m, j]|      (sum_m x in fp64)

eps = 2^-9 for bf16, 2^-11 for fp16: the sums differ from the column sums of x only by x's own
rounding (the eps term) and by the fp32 summation (M 2^-24, worst case). Shapes are the smallest
that cross every reduction: two 128-token blocks per sequence (the cross-workgroup reduce), D = 64
and 128, and for the GEMM 2 x 2 tiles with the smallest even stage count — on every CU and on ONE
persistent workgroup (four tiles in a row: the running sums restart per tile)."""
import functools
import math

import pytest
import torch

from smdt_amd.ops import _ext

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -11}


def check_bound(db, x, dtype, what):
    """db fp32 [N] against the rounded 16-bit x [M, N]; prints the observed ratio to the bound."""
    M = x.shape[0]
    xd = x.double()
    err = (db.double() - xd.sum(0)).abs()
    bound = (EPS[dtype] + M * 2.0 ** -24) * xd.abs().sum(0)
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: max |db - sum x| / bound = {ratio:.4f} (M = {M})")
    assert torch.isfinite(db).all(), what
    assert bool((err <= bound).all()), (what, ratio)


# --------------------------------------------------------------------------------------------
# flash attention backward

B, S, H = 2, 256, 4
# (name, Hkv, causal, dropout, doc)
FLASH_CASES = [("causal", 4, True, 0.0, False), ("causal_drop", 4, True, 0.1, False),
               ("full_drop", 4, False, 0.1, False), ("gqa", 2, True, 0.0, False), ("doc", 4, True, 0.1, True)]


@functools.lru_cache(maxsize=None)
def _flash_inputs(D, Hkv, dtype):
    g = torch.Generator(device=DEV).manual_seed(17 * D + Hkv)
    qkv = torch.randn(B, S, (H + 2 * Hkv) * D, device=DEV, dtype=dtype, generator=g)
    dout = torch.randn(B, S, H, D, device=DEV, dtype=dtype, generator=g)
    # documents end inside a 128-block (at 40 and 200) in batch 0, one document in batch 1
    ar = torch.arange(S, dtype=torch.int32, device=DEV)
    ds0 = torch.where(ar < 40, 0, torch.where(ar < 200, 40, 200)).to(torch.int32)
    doc_start = torch.stack([ds0, torch.zeros_like(ds0)]).contiguous()
    return qkv, dout, doc_start


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name,Hkv,causal,p,doc", FLASH_CASES)
def test_flash_bwd_token_sums(name, Hkv, causal, p, doc, dtype, D):
    from smdt_amd.ops import functional as SF
    C = _ext.ext()
    qkv, dout, doc_start = _flash_inputs(D, Hkv, dtype)
    q, k, v = SF._qkv_views(qkv, H, Hkv, D, False)
    scale = 1.0 / math.sqrt(D)
    ds = doc_start if doc else None
    de = SF.document_ends(doc_start) if doc else None
    o, lse = C.flash_fwd(q, k, v, scale, causal, None, p, 5, 11, ds)
    dq0, dk0, dv0 = C.flash_bwd(q, k, v, o, dout, lse, scale, causal, None, None, None, p, 5, 11, ds, de)
    N = (H + 2 * Hkv) * D
    db = torch.full((N,), float("nan"), device=DEV)
    dq, dk, dv = C.flash_bwd_dbias(q, k, v, o, dout, lse, scale, causal, db, False, None, None, None, p, 5, 11,
                                   ds, de)
    # the outputs do not change with the sums
    assert torch.equal(dq, dq0) and torch.equal(dk, dk0) and torch.equal(dv, dv0)
    x = torch.cat([dq.flatten(-2), dk.flatten(-2), dv.flatten(-2)], dim=-1).reshape(B * S, N)
    check_bound(db, x, dtype, f"flash {name} D{D} {dtype}")
    # bitwise reproducible, and accumulate adds into the target
    db2 = torch.ones(N, device=DEV)
    C.flash_bwd_dbias(q, k, v, o, dout, lse, scale, causal, db2, True, None, None, None, p, 5, 11, ds, de)
    assert torch.equal(db2, 1.0 + db)
    db3 = torch.empty(N, device=DEV)
    C.flash_bwd_dbias(q, k, v, o, dout, lse, scale, causal, db3, False, None, None, None, p, 5, 11, ds, de)
    assert torch.equal(db3, db)


def test_flash_bwd_token_sums_into_fused_buffer():
    """The training layout: dq / dk / dv are views of one fused [B, S, 3h] d(qkv) buffer, and the
    sums are the column sums of that buffer."""
    from smdt_amd.ops import functional as SF
    C = _ext.ext()
    D, dtype = 64, torch.bfloat16
    qkv, dout, _ = _flash_inputs(D, H, dtype)
    q, k, v = SF._qkv_views(qkv, H, H, D, False)
    o, lse = C.flash_fwd(q, k, v, 0.125, True, None, 0.1, 3, 4, None)
    dqkv = torch.empty_like(qkv)
    dq, dk, dv = SF._qkv_views(dqkv, H, H, D, False)
    db = torch.empty(3 * H * D, device=DEV)
    C.flash_bwd_dbias(q, k, v, o, dout, lse, 0.125, True, db, False, dq, dk, dv, 0.1, 3, 4, None, None)
    check_bound(db, dqkv.reshape(B * S, -1), dtype, "flash fused d(qkv)")


# --------------------------------------------------------------------------------------------
# gemm_tn EPI_DGELU


@functools.lru_cache(maxsize=None)
def _gemm_inputs(dtype):
    M, N, K = 512, 512, 128
    g = torch.Generator(device=DEV).manual_seed(23)
    a = torch.randn(M, K, device=DEV, dtype=dtype, generator=g)
    b = torch.randn(N, K, device=DEV, dtype=dtype, generator=g) * 0.05
    bias = torch.randn(N, device=DEV, dtype=dtype, generator=g)
    pre = torch.randn(M, N, device=DEV, dtype=dtype, generator=g) * 2
    return a, b, bias, pre


@pytest.mark.parametrize("blocks", [0, 1])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_dgelu_epilogue_column_sums(dtype, blocks):
    C = _ext.ext()
    a, b, bias, pre = _gemm_inputs(dtype)
    N = b.shape[0]
    ref = C.gemm_tn(a, b, 3, bias, None, None, blocks, 0, pre)[0]
    db = torch.full((N,), float("nan"), device=DEV)
    out = C.gemm_tn_dgelu_dbias(a, b, bias, pre, db, False, None, blocks)
    assert torch.equal(out, ref)                      # the output does not change with the sums
    check_bound(db, out, dtype, f"dgelu {dtype} blocks {blocks}")
    db2 = torch.ones(N, device=DEV)
    out2 = C.gemm_tn_dgelu_dbias(a, b, bias, pre, db2, True, None, blocks)
    assert torch.equal(out2, ref) and torch.equal(db2, 1.0 + db)
    db3 = torch.empty(N, device=DEV)
    C.gemm_tn_dgelu_dbias(a, b, bias, pre, db3, False, None, blocks)
    assert torch.equal(db3, db)                       # bitwise reproducible


# --------------------------------------------------------------------------------------------
# module level: one transformer layer, h = 256, 4 heads, S = 256, B = 2, TP = 1


def _model(use_flash=True):
    from smdt_amd.models.gpt import GPTModel
    from smdt_amd.models.transformer import TransformerConfig
    from smdt_amd.parallel import state as ps
    from smdt_amd.parallel.distributed import DistributedDataParallel
    ps.destroy_model_parallel()
    cfg = TransformerConfig(num_layers=1, hidden_size=256, num_attention_heads=4, max_position_embeddings=256,
                            padded_vocab_size=2048, hidden_dropout=0.0, attention_dropout=0.0, seed=3,
                            params_dtype=torch.bfloat16, use_flash_attn=use_flash)
    model = GPTModel(cfg, device=DEV)
    with torch.no_grad():       # biases start at zero: make them part of the function
        for n, p in model.named_parameters():
            if n.endswith("bias"):
                p.normal_(0, 0.02, generator=torch.Generator(device=DEV).manual_seed(len(n)))
    return model, DistributedDataParallel(model)


def _biases(model):
    named = dict(model.named_parameters())
    qkv = next(p for n, p in named.items() if n.endswith("qkv.bias"))
    fc1 = next(p for n, p in named.items() if n.endswith("fc1.bias"))
    return qkv, fc1


def _step(model, ddp, toks, monkeypatch, producer, zero=True):
    """One forward + backward; returns (qkv db, fc1 db, {bias numel: dY}, {bias numel: bias pushed
    with the wgrad}) with dY the 16-bit output gradients the wgrad queue received."""
    from smdt_amd.parallel import dense
    from smdt_amd.parallel import tensor_parallel as tp
    monkeypatch.setattr(tp, "_BIAS_FROM_PRODUCER", producer)
    # FusedGeLUMLP is taken only where its GEMMs have a tile per CU; let this 8-tile layer take it
    monkeypatch.setattr(dense, "_NUM_CUS", [1])
    dys, with_bias = {}, {}
    push = tp.DEFERRED_WGRAD.push

    def spy(weight, mg, g2, t2, bias=None, fresh=False):
        dys[g2.shape[1]] = g2
        with_bias[g2.shape[1]] = bias is not None
        return push(weight, mg, g2, t2, bias=bias, fresh=fresh)

    monkeypatch.setattr(tp.DEFERRED_WGRAD, "push", spy)
    if zero:
        ddp.zero_grad_buffer()
    loss = model(toks[:, :-1], labels=toks[:, 1:])
    loss.float().mean().backward()
    ddp.finish_grad_sync()
    monkeypatch.setattr(tp.DEFERRED_WGRAD, "push", push)
    qb, fb = _biases(model)
    return qb.main_grad.clone(), fb.main_grad.clone(), dys, with_bias


def _tokens(seed):
    return torch.randint(0, 1000, (2, 257), generator=torch.Generator().manual_seed(seed)).to(DEV)


def test_layer_bias_grads_match_wgrad_routing(monkeypatch):
    model, ddp = _model()
    qb, fb = _biases(model)
    toks = _tokens(4)
    q_new, f_new, dys, wb = _step(model, ddp, toks, monkeypatch, True)
    assert wb[qb.numel()] is False and wb[fb.numel()] is False       # the wgrad ran without bias tiles
    q_old, f_old, dys_old, wb_old = _step(model, ddp, toks, monkeypatch, False)
    assert wb_old[qb.numel()] is True and wb_old[fb.numel()] is True
    for n in (qb.numel(), fb.numel()):                                 # same dY on both routings
        assert torch.equal(dys[n], dys_old[n])
    check_bound(q_new, dys[qb.numel()], torch.bfloat16, "layer qkv bias, producer")
    check_bound(q_old, dys[qb.numel()], torch.bfloat16, "layer qkv bias, wgrad tiles")
    check_bound(f_new, dys[fb.numel()], torch.bfloat16, "layer fc1 bias, producer")
    check_bound(f_old, dys[fb.numel()], torch.bfloat16, "layer fc1 bias, wgrad tiles")


def test_layer_bias_grads_accumulate_over_micro_batches(monkeypatch):
    model, ddp = _model()
    t1, t2 = _tokens(5), _tokens(6)
    q1, f1, _, _ = _step(model, ddp, t1, monkeypatch, True)
    q2, f2, _, _ = _step(model, ddp, t2, monkeypatch, True)
    _step(model, ddp, t1, monkeypatch, True)
    q12, f12, _, _ = _step(model, ddp, t2, monkeypatch, True, zero=False)
    assert torch.equal(q12, q1 + q2) and torch.equal(f12, f1 + f2)


def test_gated_out_configuration_keeps_the_wgrad_bias(monkeypatch):
    """Without flash attention d(qkv) is not a kernel of ours' output: the QKV bias gradient stays
    with the wgrad launch (fc1 still comes from the epilogue)."""
    model, ddp = _model(use_flash=False)
    qb, fb = _biases(model)
    q, f, dys, wb = _step(model, ddp, _tokens(7), monkeypatch, True)
    assert wb[qb.numel()] is True and wb[fb.numel()] is False
    assert q.abs().max() > 0
    check_bound(q, dys[qb.numel()], torch.bfloat16, "no-flash qkv bias, wgrad tiles")
    check_bound(f, dys[fb.numel()], torch.bfloat16, "no-flash fc1 bias, producer")
