"""The 16-bit weight-gradient kernel (csrc/kernels/wgrad_gemm.hip over wgrad_core.h) bit for bit
against its torch twin on exactly representable data, bf16 and fp16: the grouped launch (one stage,
fewer stages than ring buffers, the ring wrap, partial tiles, a shared B strip, the split tail and
its empty pieces, `overwrite`, `cus`), the bias column sums of the same launch, and the single
launch with and without split-K. The shapes are those of tests/test_fp8_wgrad_gpu.py at this
kernel's stage of 32 rows; on these operands no sum rounds, so atomics are exact in any order."""
import pytest
import torch

from _numerics import wgrad_exact_bias_twin, wgrad_exact_case, wgrad_exact_twin

pytestmark = pytest.mark.gpu

S = 32                                   # the kernel's stage: rows of m per LDS stage
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}

# (M, N, K): one stage / fewer stages than ring buffers / the ring wraps / partial tiles in n and k
# (clamped loads, skipped stores) / two tiles share the B strip / 32 stages, where the tail tiles
# of a launch are cut along m and added with atomics (4 tiles: 4 pieces each on the whole chip,
# 2 pieces each with cus = 8)
SHAPES = [(S, 256, 256), (3 * S, 256, 256), (5 * S, 256, 256), (2 * S, 272, 80), (4 * S, 512, 256),
          (32 * S, 512, 512)]
BIAS_SHAPES = [(2 * S, 272, 80), (32 * S, 512, 512)]   # the n < N guard / atomic bias adds


def _ext():
    from smdt_amd.ops import _ext
    return _ext.ext()


@pytest.fixture(scope="module")
def exact_cases():
    g = torch.Generator().manual_seed(41)
    out = {}
    for dt in DT:
        for shape in SHAPES:
            a, b, mg, bg = wgrad_exact_case(g, *shape, DT[dt])
            out[dt, shape] = (a, b, mg, bg, {ow: wgrad_exact_twin(mg, a, b, ow) for ow in (False, True)},
                              wgrad_exact_bias_twin(bg, a))
    return out


def _assert_same(got, want, what=""):
    diff = got.cpu() != want
    assert not diff.any(), (f"{what}: {int(diff.sum())} of {diff.numel()} elements differ; rows "
                            f"{diff.reshape(diff.shape[0], -1).any(1).nonzero().flatten()[:8].tolist()}")


@pytest.mark.parametrize("cus", [0, 8])
@pytest.mark.parametrize("overwrite", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_wgrad_grouped_one_problem_equals_twin_bit_for_bit(exact_cases, dt, shape, overwrite, cus):
    a, b, mg, _, want, _ = exact_cases[dt, shape]
    got = mg.clone().cuda()
    assert _ext().wgrad_grouped([got], [a.cuda()], [b.cuda()], [], [overwrite], cus)
    torch.cuda.synchronize()
    _assert_same(got, want[overwrite], "main_grad")


@pytest.mark.parametrize("cus", [0, 8])
@pytest.mark.parametrize("overwrite", [False, True])
@pytest.mark.parametrize("shape", BIAS_SHAPES)
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_wgrad_grouped_bias_equals_column_sums_bit_for_bit(exact_cases, dt, shape, overwrite, cus):
    a, b, mg, bg, want, want_bias = exact_cases[dt, shape]
    got, gb = mg.clone().cuda(), bg.clone().cuda()
    assert _ext().wgrad_grouped([got], [a.cuda()], [b.cuda()], [gb], [overwrite], cus)
    torch.cuda.synchronize()
    _assert_same(got, want[overwrite], "main_grad")
    _assert_same(gb, want_bias, "bias")


GROUPS = [
    ([(S, 256, 256), (2 * S, 272, 80), (3 * S, 512, 256)], 0),     # whole tiles, three shapes
    ([(S, 256, 256), (2 * S, 272, 80), (3 * S, 512, 256)], 8),
    ([(32 * S, 256, 256), (S, 272, 80)], 0),       # a split tail with a shorter problem in it (empty pieces)
]


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("group,cus", GROUPS)
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_wgrad_grouped_launch_equals_twin_bit_for_bit(dt, group, cus, with_bias):
    """Alternating `overwrite`; with_bias: every problem but the second has a bias target."""
    g = torch.Generator().manual_seed(42)
    cases = [wgrad_exact_case(g, *shape, DT[dt]) for shape in group]
    ows = [i % 2 == 1 for i in range(len(group))]
    want = [wgrad_exact_twin(mg, a, b, ow) for (a, b, mg, _), ow in zip(cases, ows)]
    got = [c[2].clone().cuda() for c in cases]
    gbs = [c[3].clone().cuda() if i != 1 else torch.empty(0, device="cuda") for i, c in enumerate(cases)]
    assert _ext().wgrad_grouped(got, [c[0].cuda() for c in cases], [c[1].cuda() for c in cases],
                                gbs if with_bias else [], ows, cus)
    torch.cuda.synchronize()
    for i, c in enumerate(cases):
        _assert_same(got[i], want[i], f"main_grad {i} {group[i]}")
        if with_bias and i != 1:
            _assert_same(gbs[i], wgrad_exact_bias_twin(c[3], c[0]), f"bias {i} {group[i]}")


@pytest.mark.parametrize("shape,max_splits", [
    ((32 * S, 256, 256), 0),    # one tile of 32 stages: the host's split model picks four splits (atomic epilogue)
    ((5 * S, 272, 80), 1),      # plain read-modify-write on partial tiles
])
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_wgrad_mfma_single_launch_equals_twin_bit_for_bit(dt, shape, max_splits):
    g = torch.Generator().manual_seed(43)
    a, b, mg, _ = wgrad_exact_case(g, *shape, DT[dt])
    want = wgrad_exact_twin(mg, a, b, False)
    got = mg.clone().cuda()
    assert _ext().wgrad_mfma(got, a.cuda(), b.cuda(), max_splits)
    torch.cuda.synchronize()
    _assert_same(got, want, "main_grad")
