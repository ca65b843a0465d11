# -*- coding: utf-8 -*-
"""The fork path of ops/batchnorm.py (`grad_fork`, `_GradFork`, `fork_ok`)
where no GPU is needed: it must leave the CPU path alone, pass a lone
gradient through, add two, and be taken under exactly one combination of its
conditions."""
import copy
import itertools

import torch
import torch.nn as nn

from fedtorch_amd.components.models.resnet import BasicBlock
from fedtorch_amd.ops import batchnorm as bnm


def _block_step(block, x0):
    block = copy.deepcopy(block).train()
    x = x0.clone().requires_grad_(True)
    # the block input is a BN output in the network: give it a grad_fn
    out = block(x * 1.0)
    out.square().sum().backward()
    return [out.detach(), x.grad] + [p.grad for p in block.parameters()]


def test_basic_block_cpu_same_with_flag_on_and_off(monkeypatch):
    torch.manual_seed(3)
    down = nn.Sequential(nn.Conv2d(8, 16, 1, stride=2, bias=False),
                         nn.BatchNorm2d(16))
    for block, fused in ((BasicBlock(8, 8), False),
                         (BasicBlock(8, 16, 2, down), True)):
        if fused:
            bnm.convert_to_fused_bn(block)
        x = torch.randn(2, 8, 8, 8).to(memory_format=torch.channels_last)
        res = {}
        for flag in (True, False):
            monkeypatch.setattr(bnm, '_FORK_ENABLED', flag)
            res[flag] = _block_step(block, x)
        assert len(res[True]) == len(res[False])
        for u, v in zip(res[True], res[False]):
            assert torch.equal(u, v)
    assert not bnm._FORK_TAGS


def test_grad_fork_is_identity_off_the_kernel_path(monkeypatch):
    monkeypatch.setattr(bnm, '_FORK_ENABLED', True)
    x = (torch.randn(2, 8, 4, 4).to(memory_format=torch.channels_last)
         .requires_grad_(True) * 1.0)
    for training in (True, False):
        a, b = bnm.grad_fork(x, training)
        assert a is x and b is x
    with torch.no_grad():
        a, b = bnm.grad_fork(x, True)
    assert a is x and b is x


def test_grad_fork_function_gradients():
    x = torch.randn(2, 4, 3, 3, requires_grad=True)
    w1, w2 = torch.randn_like(x), torch.randn_like(x)
    for use1, use2 in ((True, False), (False, True), (True, True)):
        x.grad = None
        t1, t2 = bnm._GradFork.apply(x, None)
        assert torch.equal(t1, x) and torch.equal(t2, x)
        loss = 0
        want = torch.zeros_like(x)
        if use1:
            loss = loss + (t1 * w1).sum()
            want = want + w1
        if use2:
            loss = loss + (t2 * w2).sum()
            want = want + w2
        loss.backward()
        assert torch.equal(x.grad, want)
    # neither output used: no gradient at all
    x.grad = None
    t1, t2 = bnm._GradFork.apply(x, None)
    (x * 2).sum().backward()
    assert torch.equal(x.grad, torch.full_like(x, 2))
    assert not bnm._FORK_TAGS


def test_fork_ok_truth_table():
    names = ('enabled', 'training', 'grad_on', 'kernels', 'cl', 'nhwc',
             'defer', 'from_bn')
    taken = [v for v in itertools.product((False, True), repeat=len(names))
             if bnm.fork_ok(*v)]
    assert taken == [(True, True, True, True, True, True, False, True)]
    assert bnm.fork_ok(**dict(zip(names, taken[0]))) is True


def test_fork_keeps_deepcopy_and_state(monkeypatch):
    """no new module state: the state_dict and a deepcopy are what they
    were"""
    monkeypatch.setattr(bnm, '_FORK_ENABLED', True)
    b = bnm.convert_to_fused_bn(BasicBlock(8, 8))
    keys = set(b.state_dict())
    _block_step(b, torch.randn(2, 8, 4, 4))
    assert set(copy.deepcopy(b).state_dict()) == keys
    assert set(vars(b)) == set(vars(BasicBlock(8, 8)))
