# -*- coding: utf-8 -*-
"""Eval-mode ResNet forward on the kernel pack (FEDTORCH_MFMA_EVAL): module
routing of ops.conv3x3.conv_bn_act / FusedBatchNorm2d in eval, the launch
counts of a full converted ResNet-20, its accuracy against an fp32 reference
next to the library path's, and a do_validate-style pass with a partial last
batch that leaves the training path intact."""
import contextlib
import copy
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

import fedtorch_amd.ops as ops
from fedtorch_amd.ops import conv3x3 as c3
from fedtorch_amd.ops.batchnorm import (
    BNAddReLU, FusedBatchNorm2d, convert_to_fused_bn)

pytestmark = pytest.mark.gpu

CL = torch.channels_last
OPS = ('conv3x3_bn_act_fwd', 'bn_fwd_eval', 'stem_conv_fwd',
       'bn_fwd_train_part', 'conv3x3_bn_fwd', 'conv3x3s2_bn_fwd')


@contextlib.contextmanager
def _eval_flag(flag):
    old = c3._EVAL_ENABLED
    c3._EVAL_ENABLED = flag
    try:
        yield
    finally:
        c3._EVAL_ENABLED = old


@pytest.fixture
def calls(monkeypatch):
    """list of the names of the recorded ops._C / F.batch_norm calls, with
    the strides of the conv3x3_bn_act_fwd calls kept aside"""
    rec = []
    for name in OPS:
        fn = getattr(ops._C, name)
        monkeypatch.setattr(
            ops._C, name,
            lambda *a, _fn=fn, _n=name: (rec.append(
                (_n, a[-1]) if _n == 'conv3x3_bn_act_fwd' else _n),
                _fn(*a))[1])
    stock = torch.nn.functional.batch_norm
    monkeypatch.setattr(
        torch.nn.functional, 'batch_norm',
        lambda *a, **k: (rec.append('F.batch_norm'), stock(*a, **k))[1])
    return rec


def _count(rec, name):
    return sum(1 for r in rec if r == name or
               (isinstance(r, tuple) and r[0] == name))


def _set_bn_state(model, seed):
    """seeded non-trivial buffers and affine parameters: fresh 0/1 buffers
    would hide a wrong fold"""
    g = torch.Generator().manual_seed(seed)
    n = 0
    for m in model.modules():
        if isinstance(m, nn.BatchNorm2d):
            C = m.num_features
            dev = m.weight.device
            m.running_mean.copy_((torch.randn(C, generator=g) * 0.2).to(dev))
            m.running_var.copy_((torch.rand(C, generator=g) + 0.5).to(dev))
            m.weight.data.copy_((torch.rand(C, generator=g) + 0.5).to(dev))
            m.bias.data.copy_((torch.randn(C, generator=g) * 0.2).to(dev))
            n += 1
    return n


# --------------------------------------------------------------------------
# module routing
# --------------------------------------------------------------------------
def _pair(C, stride=1):
    torch.manual_seed(7)
    conv = c3.NhwcConv3x3(C, C * stride, 3, stride=stride, padding=1,
                          bias=False).cuda().to(memory_format=CL)
    conv.weight.data = conv.weight.data.bfloat16()
    holder = convert_to_fused_bn(nn.Sequential(BNAddReLU(C * stride))).cuda()
    _set_bn_state(holder, 3)
    assert isinstance(holder[0].bn, FusedBatchNorm2d)
    return conv, holder[0]


def test_conv_bn_act_routing(calls):
    C, W, N = 16, 32, 3
    conv, bn_mod = _pair(C)
    x = torch.randn(N, C, W, W, device='cuda').to(memory_format=CL).bfloat16()
    res = torch.randn(N, C, W, W, device='cuda').to(
        memory_format=CL).bfloat16()
    with _eval_flag(True):
        conv.eval(), bn_mod.eval()
        with torch.no_grad():
            y = c3.conv_bn_act(conv, bn_mod, x, res)
        assert calls == [('conv3x3_bn_act_fwd', 1)]
        # same result as the two modules through the library
        with _eval_flag(False), torch.no_grad():
            ref = bn_mod(conv(x), res)
        assert _count(calls, 'F.batch_norm') == 1
        rel = (y.float() - ref.float()).abs().max().item() / \
            ref.float().abs().max().item()
        print('conv_bn_act vs library rel %.5f' % rel)
        assert rel < 0.02
        # eval with grad enabled: none
        del calls[:]
        with torch.enable_grad():
            c3.conv_bn_act(conv, bn_mod, x, res)
        assert _count(calls, 'conv3x3_bn_act_fwd') == 0
        assert _count(calls, 'bn_fwd_eval') == 0
        # train mode: none, and the training kernels with the handoff run
        del calls[:]
        conv.train(), bn_mod.train()
        with torch.no_grad():
            c3.conv_bn_act(conv, bn_mod, x, res)
        assert calls == ['conv3x3_bn_fwd', 'bn_fwd_train_part']


def test_fused_bn_eval_routing(calls):
    C, W, N = 32, 16, 3
    _conv, bn_mod = _pair(C)
    bn = bn_mod.bn.eval()
    x = torch.randn(N, C, W, W, device='cuda').to(memory_format=CL).bfloat16()
    res = torch.randn_like(x)
    with _eval_flag(True), torch.no_grad():
        y = bn(x, res=res)
        assert calls == ['bn_fwd_eval']
        nbt = int(bn.num_batches_tracked) + bn._nbt_pending
        with _eval_flag(False):
            ref = bn(x, res=res)
        assert calls == ['bn_fwd_eval', 'F.batch_norm']
        assert int(bn.num_batches_tracked) + bn._nbt_pending == nbt
    assert (y.float() - ref.float()).abs().max().item() <= \
        0.02 * ref.float().abs().max().item()
    with _eval_flag(True):                   # grad enabled: stock path
        bn(x, res=res)
    assert calls[-1] == 'F.batch_norm'


# --------------------------------------------------------------------------
# full model
# --------------------------------------------------------------------------
@pytest.fixture(scope='module')
def resnet20():
    """seeded converted channels_last ResNet-20 as the training loop holds
    it (4-D weights in bf16; the stem's stay fp32, which is what the stem
    kernel reads), in eval mode, plus its input"""
    from fedtorch_amd.components.models.resnet import resnet
    from fedtorch_amd.ops.stemconv import NhwcStemConv, convert_stem
    torch.manual_seed(41)
    m = resnet(SimpleNamespace(arch='resnet20', data='cifar10')).cuda().to(
        memory_format=CL)
    convert_to_fused_bn(m)
    convert_stem(m)
    assert isinstance(m.conv1, NhwcStemConv)
    assert _set_bn_state(m, 5) == 21
    for p_ in m.parameters():
        if p_.dim() == 4 and p_ is not m.conv1.weight:
            p_.data = p_.data.bfloat16()
    ref = copy.deepcopy(m).float()           # same weight values, in fp32
    m.eval(), ref.eval()
    torch.manual_seed(42)
    x = torch.randn(5, 3, 32, 32, device='cuda').to(memory_format=CL)
    return m, ref, x


def _forward(m, x):
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
        return m(x).float()


def test_full_model_launch_counts(resnet20, calls):
    m, _ref, x = resnet20
    with _eval_flag(True):
        out = _forward(m, x)
    assert out.shape == (5, 10) and torch.isfinite(out).all().item()
    strides = [r[1] for r in calls if isinstance(r, tuple)]
    assert len(strides) == 18 and strides.count(1) == 16 \
        and strides.count(2) == 2, strides
    assert _count(calls, 'bn_fwd_eval') == 3
    assert _count(calls, 'stem_conv_fwd') == 1
    assert _count(calls, 'F.batch_norm') == 0
    for name in ('bn_fwd_train_part', 'conv3x3_bn_fwd', 'conv3x3s2_bn_fwd'):
        assert _count(calls, name) == 0
    # flag off: today's path, all 21 BNs on the stock kernel
    del calls[:]
    with _eval_flag(False):
        _forward(m, x)
    assert _count(calls, 'F.batch_norm') == 21
    assert _count(calls, 'conv3x3_bn_act_fwd') == 0
    assert _count(calls, 'bn_fwd_eval') == 0


def test_full_model_accuracy(resnet20, monkeypatch):
    """e_new <= 2 * e_lib: max-abs logit errors of the kernel path and of the
    library path against the fp32 stock-module reference.  The kernel path
    rounds to bf16 once per conv+BN+add+ReLU where the library path rounds
    three to four times; the factor 2 covers summation-order differences."""
    m, ref, x = resnet20
    with _eval_flag(True):
        new = _forward(m, x)
    with _eval_flag(False):
        lib = _forward(m, x)
    monkeypatch.setattr(ops, 'FORCE_EAGER', True)
    with torch.no_grad():
        want = ref(x)
    assert want.dtype == torch.float32
    e_new = (new - want).abs().max().item()
    e_lib = (lib - want).abs().max().item()
    print('eval logits max-abs err vs fp32: new %.5f library %.5f '
          '(max |logit| %.3f)' % (e_new, e_lib, want.abs().max().item()))
    assert e_new <= 2 * e_lib, (e_new, e_lib)


def test_validate_style_pass_then_train(resnet20, calls):
    """a do_validate-style loop (eval -> no_grad + autocast inference ->
    train) over two batches, the last one partial, then one training
    forward: the conv epilogue still hands its partials to the BN."""
    from fedtorch_amd.trainings.eval import inference
    m = copy.deepcopy(resnet20[0])
    g = torch.Generator().manual_seed(11)
    loader = [(torch.randn(n, 3, 32, 32, generator=g),
               torch.randint(0, 10, (n,), generator=g)) for n in (8, 3)]
    criterion = nn.CrossEntropyLoss()
    m.train()
    with _eval_flag(True):
        m.eval()
        seen = []
        for _input, _target in loader:
            _input = _input.cuda().to(memory_format=CL)
            _target = _target.cuda()
            with torch.no_grad(), \
                    torch.autocast('cuda', dtype=torch.bfloat16):
                loss, perf = inference(m, criterion, (1, 5), _input, _target)
            seen.append((float(loss), perf))
        m.train()
        assert _count(calls, 'conv3x3_bn_act_fwd') == 36
        assert _count(calls, 'F.batch_norm') == 0
        for loss, perf in seen:
            assert loss == loss and abs(loss) != float('inf')
            assert all(0.0 <= p <= 100.0 for p in perf)
        assert m.training and all(mod.training for mod in m.modules())
        del calls[:]
        x = loader[0][0].cuda().to(memory_format=CL)
        with torch.autocast('cuda', dtype=torch.bfloat16):
            out = m(x)
        assert torch.isfinite(out.float()).all().item()
    assert _count(calls, 'bn_fwd_train_part') == 18
    assert _count(calls, 'conv3x3_bn_act_fwd') == 0
    assert _count(calls, 'bn_fwd_eval') == 0
