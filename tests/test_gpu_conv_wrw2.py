# -*- coding: utf-8 -*-
"""MFMA weight gradient of the 3x3/stride-1 body convs (hip/convwrw2.h):
conv3x3_wrw2 (main kernel + one final reduce/cast/scatter kernel) vs the
fp32 aten reference at batch sizes around the launcher's stream cap, exact
one-hot tap checks, determinism, and the autograd routing behind
FEDTORCH_WRW2_C (plain and deferred-BN backward)."""
import contextlib
import functools

import pytest
import torch

import fedtorch_amd.ops as ops

pytestmark = pytest.mark.gpu

CL = torch.channels_last
SHAPES = ((16, 32), (32, 16), (64, 8))     # (C, W); Co = Ci = C, H = W
SPOS = {16: 128, 32: 128, 64: 64}          # positions per supertile


def _ref_wrw(dy, x):
    C = x.shape[1]
    w = torch.zeros(C, C, 3, 3, device=x.device).to(memory_format=CL)
    return torch.ops.aten.convolution_backward(
        dy.float(), x.float(), w, None, [1, 1], [1, 1], [1, 1], False,
        [0, 0], 1, [False, True, False])[1]


@functools.lru_cache(maxsize=None)
def _case(C, W, N):
    """random (dy, x) and the fp32 reference dw, computed once per shape and
    shared (read-only) by the tests."""
    g = torch.Generator(device='cuda').manual_seed(1000 * C + N)
    x = torch.randn(N, C, W, W, device='cuda', generator=g).to(
        memory_format=CL).bfloat16()
    dy = torch.randn(N, C, W, W, device='cuda', generator=g).to(
        memory_format=CL).bfloat16()
    return dy, x, _ref_wrw(dy, x)


def _rel(out, ref):
    return (out.float() - ref).abs().max().item() / ref.abs().max().item()


def _remainder_batch(C, W):
    """smallest-ish N whose supertile count exceeds the launcher's stream cap
    and is not a multiple of it (a supertile is SPOS positions of one image,
    so no supertile spans two images and any N is allowed)."""
    cap = ops._C.conv3x3_wrw2_grid_cap(C)
    per_img = W * W // SPOS[C]
    n = cap // per_img + 3
    assert n * per_img > cap and (n * per_img) % cap != 0
    return n


@pytest.mark.parametrize('N', (1, 3, 'remainder'))
@pytest.mark.parametrize('C,W', SHAPES)
def test_wrw2_numerics(C, W, N):
    if N == 'remainder':
        N = _remainder_batch(C, W)
    dy, x, ref = _case(C, W, N)
    dw = ops._C.conv3x3_wrw2(dy, x)
    assert dw.shape == ref.shape == (C, C, 3, 3)
    assert dw.dtype == torch.bfloat16
    assert dw.is_contiguous(memory_format=CL)
    rel = _rel(dw, ref)
    print('wrw2 C%d N%d rel %.5f' % (C, N, rel))
    assert rel < 0.01, 'C%d N%d rel %.5f' % (C, N, rel)


def _positions(H, W):
    return ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1),
            (H // 2, W // 2 - 1))


@pytest.mark.parametrize('C,W', SHAPES)
def test_wrw2_one_hot_exact(C, W):
    """one-hot dy x one-hot x, every tap: exactly one dw element is set;
    a tap that lands in the padding finds nothing (x is then set where a
    wrapped index would look) and dw is all zero."""
    N, n = 3, 2
    for i, (ho, wo) in enumerate(_positions(W, W)):
        dy = torch.zeros(N, C, W, W, device='cuda').to(
            memory_format=CL).bfloat16()
        for tap in range(9):
            dh, dw_ = tap // 3, tap % 3
            co = (7 * tap + 13 * i + 5) % C
            ci = (5 * tap + 3 * i + 1) % C
            hi, wi = ho + dh - 1, wo + dw_ - 1
            inside = 0 <= hi < W and 0 <= wi < W
            x = torch.zeros(N, C, W, W, device='cuda').to(
                memory_format=CL).bfloat16()
            x[n, ci, hi % W, wi % W] = 1.0
            dy.zero_()
            dy[n, co, ho, wo] = 1.0
            dw = ops._C.conv3x3_wrw2(dy, x).float()
            ref = _ref_wrw(dy, x)
            where = 'pos (%d,%d) tap %d' % (ho, wo, tap)
            assert torch.equal(dw, ref), where
            if inside:
                assert dw[co, ci, dh, dw_].item() == 1.0, where
                assert int((dw != 0).sum().item()) == 1, where
            else:
                assert int((dw != 0).sum().item()) == 0, where


@pytest.mark.parametrize('C,W', SHAPES)
def test_wrw2_deterministic(C, W):
    dy, x, _ = _case(C, W, _remainder_batch(C, W))
    a = ops._C.conv3x3_wrw2(dy, x)
    b = ops._C.conv3x3_wrw2(dy, x)
    assert torch.equal(a, b)


@contextlib.contextmanager
def _flags(wrw2_c, defer):
    """set conv3x3._WRW2_SHAPES from a FEDTORCH_WRW2_C-style string and
    conv3x3._BNDEFER_ENABLED, as the module does at import; the two
    all-shapes wrw switches are held at their defaults (off)"""
    from fedtorch_amd.ops import conv3x3 as c3
    old = (c3._WRW2_SHAPES, c3._BNDEFER_ENABLED, c3._WRW2_ENABLED,
           c3._ENABLED)
    c3._WRW2_SHAPES = set(int(c) for c in wrw2_c.split(',') if c.strip())
    c3._BNDEFER_ENABLED = defer
    c3._WRW2_ENABLED = c3._ENABLED = False
    try:
        yield
    finally:
        (c3._WRW2_SHAPES, c3._BNDEFER_ENABLED, c3._WRW2_ENABLED,
         c3._ENABLED) = old


def _stack_grads(C, W, wrw2_c, defer, calls):
    """conv -> BN+ReLU -> conv at N = 4; the first conv's backward takes the
    deferred-BN branch when defer is on.  Returns the two weight grads."""
    import torch.nn as nn
    from fedtorch_amd.ops import batchnorm as bnm
    from fedtorch_amd.ops import conv3x3 as c3
    with _flags(wrw2_c, defer):
        torch.manual_seed(21)
        m = nn.Sequential(
            c3.NhwcConv3x3(C, C, 3, padding=1, bias=False),
            bnm.BNReLU(C),
            c3.NhwcConv3x3(C, C, 3, padding=1, bias=False),
        ).cuda().to(memory_format=CL)
        bnm.convert_to_fused_bn(m)
        for p_ in m.parameters():
            if p_.dim() == 4:
                p_.data = p_.data.bfloat16()
        m.train()
        torch.manual_seed(33)
        x = torch.randn(4, C, W, W, device='cuda').to(
            memory_format=CL).bfloat16().requires_grad_(True)
        del calls[:]
        m(x).float().square().mean().backward()
        assert not c3._BNBWD_TAGS, 'side table must drain'
        return [p_.grad.float().clone() for p_ in m.parameters()
                if p_.dim() == 4]


@pytest.mark.parametrize('defer', (False, True))
@pytest.mark.parametrize('C,W', SHAPES)
def test_wrw2_module_routing(C, W, defer, monkeypatch):
    """NhwcConv3x3 backward with the default FEDTORCH_WRW2_C against the
    same stack with it empty (library wrw): a channel count in the default
    goes through conv3x3_wrw2 in the plain AND the deferred-BN branch, any
    other stays on the library, and the weight gradients agree."""
    from fedtorch_amd.ops import conv3x3 as c3
    calls = []
    fn = ops._C.conv3x3_wrw2
    monkeypatch.setattr(
        ops._C, 'conv3x3_wrw2',
        lambda *a: (calls.append('wrw2'), fn(*a))[1])
    default = c3._WRW2_DEFAULT_C
    got = _stack_grads(C, W, default, defer, calls)
    in_default = C in set(int(c) for c in default.split(',') if c.strip())
    assert len(calls) == (2 if in_default else 0)
    want = _stack_grads(C, W, '', defer, calls)
    assert len(calls) == 0
    for i, (a, b) in enumerate(zip(got, want)):
        rel = _rel(a, b)
        print('module C%d defer %d conv %d rel %.5f' % (C, defer, i, rel))
        assert rel < 0.01, 'conv %d dw rel %.5f' % (i, rel)
