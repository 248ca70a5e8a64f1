"""Fused BatchNorm + add + ReLU, CPU side: the torch twin ``batch_norm_act_ref`` must reproduce the
module chain ``nn.BatchNorm2d -> add -> relu`` (outputs, the four gradients, running statistics),
and ``fused_bn`` changes no parameter, buffer, state-dict key or result of a ResNet."""
import pytest
import torch
import torch.nn as nn

from smdt_amd.models import zoo
from smdt_amd.models.resnet import resnet
from smdt_amd.ops import functional as SF

MODES = {"plain": (False, False), "relu": (False, True), "residual_relu": (True, True)}


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("mode", MODES)
def test_twin_matches_module_chain(mode, training):
    has_res, relu = MODES[mode]
    torch.manual_seed(0)
    C = 6
    bn = nn.BatchNorm2d(C, momentum=0.3).double().train(training)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
        bn.running_mean.uniform_(-0.3, 0.3)
        bn.running_var.uniform_(0.5, 2.0)
    gamma, beta = (p.detach().clone().requires_grad_() for p in (bn.weight, bn.bias))
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    for step in range(2):   # two steps: the running statistics compound
        x = torch.randn(3, C, 5, 7, dtype=torch.float64).mul(2).add(0.5)
        res = torch.randn_like(x) if has_res else None
        dy = torch.randn_like(x)
        leaves = [[t.clone().requires_grad_() for t in (x, res) if t is not None] for _ in range(2)]
        want = bn(leaves[0][0])
        want = want + leaves[0][1] if has_res else want
        want = want.relu() if relu else want
        got = SF.batch_norm_act(leaves[1][0], gamma, beta, rm, rv, training, 0.3, bn.eps,
                                residual=leaves[1][1] if has_res else None, relu=relu)
        torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
        gw = torch.autograd.grad(want, leaves[0] + [bn.weight, bn.bias], dy)
        gg = torch.autograd.grad(got, leaves[1] + [gamma, beta], dy)
        for a, b in zip(gg, gw):
            torch.testing.assert_close(a, b, rtol=1e-11, atol=1e-11)
        torch.testing.assert_close(rm, bn.running_mean, rtol=1e-13, atol=1e-13)
        torch.testing.assert_close(rv, bn.running_var, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_resnet18_fused_bn_is_the_same_model(training):
    torch.manual_seed(0)
    plain = resnet("resnet18", 10)
    fused = resnet("resnet18", 10, fused_bn=True)
    assert list(fused.state_dict()) == list(plain.state_dict())
    fused.load_state_dict(plain.state_dict())
    plain.train(training), fused.train(training)
    x = torch.randn(4, 3, 64, 64)
    torch.testing.assert_close(fused(x), plain(x), rtol=1e-4, atol=1e-4)
    for (k, a), b in zip(fused.state_dict().items(), plain.state_dict().values()):
        if k.endswith("num_batches_tracked"):
            assert a.item() == b.item() == int(training), k
        else:
            torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5, msg=k)


def test_zoo_threads_fused_bn():
    assert zoo.create("resnet18", 10, fused_bn=True).layer1[0].fused_bn
    assert not zoo.create("resnet50", 10).layer4[2].fused_bn
    with pytest.raises(TypeError):
        zoo.create("resnet18", 10, fused_btachnorm=True)
    with pytest.raises(TypeError):
        zoo.create("mnist_cnn", 10, fused_bn=True)


def test_refusals():
    C = 8
    g, b, rm, rv = torch.ones(C), torch.zeros(C), torch.zeros(C), torch.ones(C)
    x = torch.randn(2, C, 3, 3)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        SF.batch_norm_act(torch.randn(1, C, 1, 1), g, b, rm, rv, True, 0.1, 1e-5)
    SF.batch_norm_act(torch.randn(1, C, 1, 1), g, b, rm, rv, False, 0.1, 1e-5)     # eval takes it
    with pytest.raises(ValueError, match="momentum=None"):
        SF.batch_norm_act(x, g, b, rm, rv, True, None, 1e-5)
    for bad in (torch.randn(2, C, 3, 1), x.double(), x.contiguous(memory_format=torch.channels_last)):
        with pytest.raises(ValueError, match="residual must have x's shape, dtype and memory format"):
            SF.batch_norm_act(x, g, b, rm, rv, True, 0.1, 1e-5, residual=bad)
    assert not SF.batch_norm_act_supported(x, g, b, rm, rv)
