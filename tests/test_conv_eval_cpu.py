# -*- coding: utf-8 -*-
"""ops.conv3x3.conv_bn_act and the models that call it, off the GPU: the
helper is exactly the two module calls it stands for, and the ResNet
forwards are bit for bit the composition they were before the helper, in
train and eval, with the eval flag on or off."""
import copy
import os
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

from fedtorch_amd.ops import conv3x3 as c3
from fedtorch_amd.ops.batchnorm import (
    BNAddReLU, BNReLU, convert_to_fused_bn)
from fedtorch_amd.components.models.resnet import (
    BasicBlock, Bottleneck, resnet)


@pytest.fixture(params=(False, True), ids=('flag_off', 'flag_on'))
def flag(request, monkeypatch):
    monkeypatch.setattr(c3, '_EVAL_ENABLED', request.param)
    return request.param


def _randomize_bn(model, seed):
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, nn.BatchNorm2d):
            C = m.num_features
            m.running_mean.copy_(torch.randn(C, generator=g) * 0.2)
            m.running_var.copy_(torch.rand(C, generator=g) + 0.5)
            m.weight.data.copy_(torch.rand(C, generator=g) + 0.5)
            m.bias.data.copy_(torch.randn(C, generator=g) * 0.2)


def _same_state(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


@pytest.mark.parametrize('train', (True, False), ids=('train', 'eval'))
@pytest.mark.parametrize('fused', (False, True), ids=('stock_bn', 'fused_bn'))
@pytest.mark.parametrize('kind', ('bnrelu', 'bnaddrelu'))
def test_conv_bn_act_is_the_two_module_calls(kind, fused, train, flag):
    torch.manual_seed(3)
    C, N, W = 16, 2, 32
    conv = c3.NhwcConv3x3(C, C, 3, stride=1, padding=1, bias=False)
    holder = nn.Sequential(BNReLU(C) if kind == 'bnrelu' else BNAddReLU(C))
    if fused:
        convert_to_fused_bn(holder)
    _randomize_bn(holder, 5)
    bn_mod = holder[0]
    x = torch.randn(N, C, W, W).to(memory_format=torch.channels_last)
    res = torch.randn(N, C, W, W) if kind == 'bnaddrelu' else None
    conv.train(train), bn_mod.train(train)
    conv2, bn_mod2 = copy.deepcopy(conv), copy.deepcopy(bn_mod)
    for no_grad in (False, True):
        with torch.set_grad_enabled(not no_grad):
            got = c3.conv_bn_act(conv, bn_mod, x, res)
            want = bn_mod2(conv2(x)) if res is None \
                else bn_mod2(conv2(x), res)
        assert torch.equal(got, want)
        _same_state(bn_mod, bn_mod2)


def _parent_block(b, x):
    """BasicBlock.forward / Bottleneck.forward before conv_bn_act"""
    identity = x if b.downsample is None else b.downsample(x)
    out = b.bn1(b.conv1(x))
    if isinstance(b, Bottleneck):
        out = b.bn2(b.conv2(out))
        return b.bn3(b.conv3(out), identity)
    return b.bn2(b.conv2(out), identity)


def _parent_forward(m, x):
    x = m.bn1(m.conv1(x))
    for layer in (m.layer1, m.layer2, m.layer3):
        for b in layer:
            assert isinstance(b, (BasicBlock, Bottleneck))
            x = _parent_block(b, x)
    return m.fc(m.avgpool(x).flatten(1))


@pytest.mark.parametrize('train', (True, False), ids=('train', 'eval'))
@pytest.mark.parametrize('fused', (False, True), ids=('stock_bn', 'fused_bn'))
def test_resnet20_cpu_forward_unchanged(fused, train, flag):
    torch.manual_seed(41)
    m = resnet(SimpleNamespace(arch='resnet20', data='cifar10'))
    if fused:
        convert_to_fused_bn(m)
    _randomize_bn(m, 9)
    m.train(train)
    m2 = copy.deepcopy(m)
    torch.manual_seed(42)
    x = torch.randn(4, 3, 32, 32)
    with torch.set_grad_enabled(train):
        got, want = m(x), _parent_forward(m2, x)
    assert torch.equal(got, want)
    _same_state(m, m2)


@pytest.mark.parametrize('train', (True, False), ids=('train', 'eval'))
def test_bottleneck_cpu_forward_unchanged(train, flag):
    torch.manual_seed(43)
    down = nn.Sequential(nn.Conv2d(16, 64, 1, bias=False),
                         nn.BatchNorm2d(64))
    b = convert_to_fused_bn(Bottleneck(16, 16, 1, down))
    _randomize_bn(b, 10)
    b.train(train)
    b2 = copy.deepcopy(b)
    x = torch.randn(3, 16, 8, 8)
    with torch.set_grad_enabled(train):
        assert torch.equal(b(x), _parent_block(b2, x))
    _same_state(b, b2)


def test_eval_flag_parses():
    assert c3._EVAL_DEFAULT in ('0', '1')
    assert c3._EVAL_ENABLED is (
        os.environ.get('FEDTORCH_MFMA_EVAL', c3._EVAL_DEFAULT) == '1')
    # off the GPU the path never applies, whatever the flag says
    x = torch.zeros(1, 16, 8, 32)
    with torch.no_grad():
        old = c3._EVAL_ENABLED
        c3._EVAL_ENABLED = True
        try:
            assert not c3.eval_active(x)
        finally:
            c3._EVAL_ENABLED = old
