# -*- coding: utf-8 -*-
"""The routing of fedtorch_amd.ops.conv3x3 as truth tables, on the CPU: the
shape predicate `_mfma_stride`, the backward plan `_bwd_plan`, and
NhwcConv3x3.forward staying exactly F.conv2d off the GPU whatever the flags
say."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from fedtorch_amd.ops import conv3x3 as c3

CL = torch.channels_last
BF16 = torch.bfloat16


def _conv(Ci, Co, stride, padding=1, bias=False):
    return c3.NhwcConv3x3(Ci, Co, 3, stride=stride, padding=padding,
                          bias=bias)


def _x(C, H, W, dtype=BF16, fmt=CL):
    return torch.zeros(1, C, H, W, dtype=dtype).contiguous(memory_format=fmt)


# (Ci, Co, W_in, stride) at the smallest valid H -> the stride returned
SUPPORTED = [
    (16, 16, 32, 1, 8),
    (32, 32, 16, 1, 8),
    (64, 64, 8, 1, 8),
    (16, 32, 32, 2, 16),
    (32, 64, 16, 2, 16),
]


@pytest.mark.parametrize('Ci,Co,W,stride,H', SUPPORTED)
def test_mfma_stride_supported(Ci, Co, W, stride, H):
    assert c3._mfma_stride(_conv(Ci, Co, stride), _x(Ci, H, W)) == stride


# one near miss per condition of the predicate, each off a supported case
NEAR_MISSES = {
    'H=4': (_conv(64, 64, 1), _x(64, 4, 8)),
    'H=8 at stride 2': (_conv(16, 32, 2), _x(16, 8, 32)),
    'fp32 x': (_conv(16, 16, 1), _x(16, 8, 32, dtype=torch.float32)),
    'NCHW x': (_conv(16, 16, 1), _x(16, 8, 32, fmt=torch.contiguous_format)),
    'bias': (_conv(16, 16, 1, bias=True), _x(16, 8, 32)),
    'padding 0': (_conv(16, 16, 1, padding=0), _x(16, 8, 32)),
    'Ci != Co at stride 1': (_conv(16, 32, 1), _x(16, 8, 32)),
    'Co != 2 Ci at stride 2': (_conv(16, 16, 2), _x(16, 16, 32)),
    '(16, W=16)': (_conv(16, 16, 1), _x(16, 8, 16)),
    '(64, W=16)': (_conv(64, 64, 1), _x(64, 8, 16)),
    '3D input': (_conv(16, 16, 1), _x(16, 8, 32)[0]),
}


@pytest.mark.parametrize('name', sorted(NEAR_MISSES))
def test_mfma_stride_near_miss(name):
    conv, x = NEAR_MISSES[name]
    assert c3._mfma_stride(conv, x) == 0


def test_mfma_stride_v1_rows():
    """wrw v1 tiles H by its 32-position K-tile, not by 8 rows: H = 4 at
    W = 8 is its shape and not the fused forward's"""
    conv, x = _conv(64, 64, 1), _x(64, 4, 8)
    assert c3._mfma_stride(conv, x) == 0
    assert c3._mfma_stride(conv, x, v1_rows=True) == 1
    assert c3._mfma_stride(conv, _x(64, 3, 8), v1_rows=True) == 0


# (_DGRAD_ENABLED, _ENABLED, _WRW2_ENABLED, C in _WRW2_SHAPES) ->
#   (dx path, dw path, combined) without a tag, then with one
T, F_ = True, False
PLAN = {
    (F_, F_, F_, F_): (('lib', 'lib', T), ('dgrad_bn', 'lib', F_)),
    (F_, F_, F_, T): (('lib', 'wrw2', F_), ('dgrad_bn', 'wrw2', F_)),
    (F_, F_, T, F_): (('lib', 'wrw2', F_), ('dgrad_bn', 'wrw2', F_)),
    (F_, F_, T, T): (('lib', 'wrw2', F_), ('dgrad_bn', 'wrw2', F_)),
    (F_, T, F_, F_): (('lib', 'wrw', F_), ('dgrad_bn', 'lib', F_)),
    (F_, T, F_, T): (('lib', 'wrw2', F_), ('dgrad_bn', 'wrw2', F_)),
    (F_, T, T, F_): (('lib', 'wrw2', F_), ('dgrad_bn', 'wrw2', F_)),
    (F_, T, T, T): (('lib', 'wrw2', F_), ('dgrad_bn', 'wrw2', F_)),
    (T, F_, F_, F_): (('dgrad', 'lib', F_), ('dgrad_bn', 'lib', F_)),
    (T, F_, F_, T): (('dgrad', 'wrw2', F_), ('dgrad_bn', 'wrw2', F_)),
    (T, F_, T, F_): (('dgrad', 'wrw2', F_), ('dgrad_bn', 'wrw2', F_)),
    (T, F_, T, T): (('dgrad', 'wrw2', F_), ('dgrad_bn', 'wrw2', F_)),
    (T, T, F_, F_): (('dgrad', 'wrw', F_), ('dgrad_bn', 'lib', F_)),
    (T, T, F_, T): (('dgrad', 'wrw2', F_), ('dgrad_bn', 'wrw2', F_)),
    (T, T, T, F_): (('dgrad', 'wrw2', F_), ('dgrad_bn', 'wrw2', F_)),
    (T, T, T, T): (('dgrad', 'wrw2', F_), ('dgrad_bn', 'wrw2', F_)),
}


def test_plan_table_is_complete():
    assert sorted(PLAN) == sorted(itertools.product((F_, T), repeat=4))


@pytest.mark.parametrize('flags', sorted(PLAN))
def test_bwd_plan(flags, monkeypatch):
    dgrad, v1, wrw2, in_shapes = flags
    C = 32
    monkeypatch.setattr(c3, '_DGRAD_ENABLED', dgrad)
    monkeypatch.setattr(c3, '_ENABLED', v1)
    monkeypatch.setattr(c3, '_WRW2_ENABLED', wrw2)
    monkeypatch.setattr(c3, '_WRW2_SHAPES', {16, C} if in_shapes else {16})
    plain, tagged = PLAN[flags]
    assert c3._bwd_plan(C, False) == plain
    assert c3._bwd_plan(C, True) == tagged


FLAGS = ('_ENABLED', '_FWD_ENABLED', '_WRW2_ENABLED', '_DGRAD_ENABLED',
         '_BNDEFER_ENABLED', '_S2BWD_ENABLED', '_EVAL_ENABLED')


@pytest.mark.parametrize('Ci,Co,W,stride,H', SUPPORTED[::2])
def test_forward_on_cpu_is_conv2d(Ci, Co, W, stride, H, monkeypatch):
    """every flag setting, training and eval: a CPU input of a supported
    shape, bf16 channels_last weight included, takes F.conv2d bit for bit"""
    torch.manual_seed(3)
    m = _conv(Ci, Co, stride).to(BF16).to(memory_format=CL)
    x = torch.randn(1, Ci, H, W).to(BF16).contiguous(memory_format=CL)
    assert c3._mfma_stride(m, x) == stride
    want = F.conv2d(x, m.weight, None, stride, 1)
    for values in itertools.product((False, True), repeat=len(FLAGS)):
        for name, v in zip(FLAGS, values):
            monkeypatch.setattr(c3, name, v)
        for train in (True, False):
            m.train(train)
            assert torch.equal(m(x), want), (values, train)
