# -*- coding: utf-8 -*-
"""MFMA backward of the 3x3/stride-2 transition convs (hip/convs2bwd.h):
conv3x3s2_dgrad / conv3x3s2_wrw vs the fp32 aten reference, exact one-hot
tap checks, the autograd wiring behind FEDTORCH_MFMA_S2_BWD and the
launchers' argument checks."""
import functools

import pytest
import torch

import fedtorch_amd.ops as ops

pytestmark = pytest.mark.gpu

CL = torch.channels_last
SHAPES = ((16, 32), (32, 16))          # (Ci, Wi); Co = 2*Ci, Hi = Wi


def _ref_bwd(dy, x, w, mask):
    return torch.ops.aten.convolution_backward(
        dy.float(), x.float(), w.float(), None, [2, 2], [1, 1], [1, 1],
        False, [0, 0], 1, mask)


@functools.lru_cache(maxsize=None)
def _case(Ci, Wi, N):
    """random (dy, x, w) and the fp32 reference (dx, dw), computed once per
    shape and shared (read-only) by the dgrad and wrw tests."""
    Co, Wo = 2 * Ci, Wi // 2
    g = torch.Generator(device='cuda').manual_seed(1000 * Ci + N)
    x = torch.randn(N, Ci, Wi, Wi, device='cuda', generator=g).to(
        memory_format=CL).bfloat16()
    dy = torch.randn(N, Co, Wo, Wo, device='cuda', generator=g).to(
        memory_format=CL).bfloat16()
    w = (torch.randn(Co, Ci, 3, 3, device='cuda', generator=g)
         / (9 * Ci) ** .5).to(memory_format=CL).bfloat16()
    dx, dw, _ = _ref_bwd(dy, x, w, [True, True, False])
    return dy, x, w, dx, dw


def _rel(out, ref):
    return (out.float() - ref).abs().max().item() / ref.abs().max().item()


def _remainder_batch(Ci, Wi):
    """smallest-ish N whose supertile count exceeds the launcher's grid cap
    and is not a multiple of it (supertile = 8 output rows of one image)."""
    cap = ops._C.conv3x3s2_wrw_grid_cap(Ci)
    per_img = (Wi // 2) // 8
    n = cap // per_img + 3
    assert n * per_img > cap and (n * per_img) % cap != 0
    return n


@pytest.mark.parametrize('N', (1, 3, 64))
@pytest.mark.parametrize('Ci,Wi', SHAPES)
def test_s2_dgrad_numerics(Ci, Wi, N):
    dy, _x, w, ref, _ = _case(Ci, Wi, N)
    dx = ops._C.conv3x3s2_dgrad(dy, w)
    assert dx.shape == ref.shape and dx.is_contiguous(memory_format=CL)
    rel = _rel(dx, ref)
    print('dgrad Ci%d N%d rel %.5f' % (Ci, N, rel))
    assert rel < 0.01, 'Ci%d N%d rel %.5f' % (Ci, N, rel)


@pytest.mark.parametrize('N', (1, 3, 64, 'remainder'))
@pytest.mark.parametrize('Ci,Wi', SHAPES)
def test_s2_wrw_numerics(Ci, Wi, N):
    if N == 'remainder':
        N = _remainder_batch(Ci, Wi)
    dy, x, _w, _, ref = _case(Ci, Wi, N)
    dw = ops._C.conv3x3s2_wrw(dy, x)
    assert dw.shape == ref.shape and dw.is_contiguous(memory_format=CL)
    rel = _rel(dw, ref)
    print('wrw Ci%d N%d rel %.5f' % (Ci, N, rel))
    assert rel < 0.01, 'Ci%d N%d rel %.5f' % (Ci, N, rel)


def _positions(Ho, Wo):
    return ((0, 0), (0, Wo - 1), (Ho - 1, 0), (Ho - 1, Wo - 1),
            (Ho // 2, Wo // 2 - 1))


@pytest.mark.parametrize('Ci,Wi', SHAPES)
def test_s2_dgrad_one_hot_exact(Ci, Wi):
    """a single 1.0 in dy: every dx element has at most one contribution,
    so dx is bit-exact and zero outside the 3x3 footprint."""
    Co, Ho = 2 * Ci, Wi // 2
    N, n = 3, 2
    _dy, _x, w, _, _ = _case(Ci, Wi, 3)
    x = torch.zeros(N, Ci, Wi, Wi, device='cuda').to(
        memory_format=CL).bfloat16()
    for i, (ho, wo) in enumerate(_positions(Ho, Ho)):
        co = (11 * i + 5) % Co
        dy = torch.zeros(N, Co, Ho, Ho, device='cuda').to(
            memory_format=CL).bfloat16()
        dy[n, co, ho, wo] = 1.0
        dx = ops._C.conv3x3s2_dgrad(dy, w)
        ref = _ref_bwd(dy, x, w, [True, False, False])[0].bfloat16()
        assert torch.equal(dx, ref), 'pos (%d,%d)' % (ho, wo)
        foot = torch.zeros(N, 1, Wi, Wi, dtype=torch.bool, device='cuda')
        foot[n, :, max(2 * ho - 1, 0):2 * ho + 2,
             max(2 * wo - 1, 0):2 * wo + 2] = True
        assert (dx.float() * (~foot)).abs().max().item() == 0.0
        assert dx.float().abs().max().item() > 0.0


@pytest.mark.parametrize('Ci,Wi', SHAPES)
def test_s2_wrw_one_hot_exact(Ci, Wi):
    """one-hot dy x one-hot x, every tap: exactly one dw element is set;
    a tap that lands in the padding finds nothing (x is then set where a
    wrapped index would look) and dw is all zero."""
    Co, Ho, Hi = 2 * Ci, Wi // 2, Wi
    N, n = 3, 2
    w = torch.zeros(Co, Ci, 3, 3, device='cuda').to(
        memory_format=CL).bfloat16()
    for i, (ho, wo) in enumerate(_positions(Ho, Ho)):
        dy = torch.zeros(N, Co, Ho, Ho, device='cuda').to(
            memory_format=CL).bfloat16()
        for tap in range(9):
            dh, dw_ = tap // 3, tap % 3
            co = (7 * tap + 13 * i + 5) % Co
            ci = (5 * tap + 3 * i + 1) % Ci
            hi, wi = 2 * ho + dh - 1, 2 * wo + dw_ - 1
            inside = 0 <= hi < Hi and 0 <= wi < Hi
            x = torch.zeros(N, Ci, Hi, Hi, device='cuda').to(
                memory_format=CL).bfloat16()
            x[n, ci, hi % Hi, wi % Hi] = 1.0
            dy.zero_()
            dy[n, co, ho, wo] = 1.0
            dw = ops._C.conv3x3s2_wrw(dy, x).float()
            ref = _ref_bwd(dy, x, w, [False, True, False])[1]
            where = 'pos (%d,%d) tap %d' % (ho, wo, tap)
            assert torch.equal(dw, ref), where
            if inside:
                assert dw[co, ci, dh, dw_].item() == 1.0, where
                assert int((dw != 0).sum().item()) == 1, where
            else:
                assert int((dw != 0).sum().item()) == 0, where


def _s2bwd(flag):
    """context manager toggling conv3x3._S2BWD_ENABLED"""
    import contextlib
    from fedtorch_amd.ops import conv3x3 as c3

    @contextlib.contextmanager
    def cm():
        old = c3._S2BWD_ENABLED
        c3._S2BWD_ENABLED = flag
        try:
            yield
        finally:
            c3._S2BWD_ENABLED = old
    return cm()


@pytest.mark.parametrize('Ci,Wi', SHAPES)
def test_s2_bwd_module(Ci, Wi, monkeypatch):
    """NhwcConv3x3 stride 2 with the flag on: both grads come from the new
    kernels and match the fp32 F.conv2d autograd reference."""
    import torch.nn.functional as F
    from fedtorch_amd.ops.conv3x3 import NhwcConv3x3
    calls = []
    for name in ('conv3x3s2_dgrad', 'conv3x3s2_wrw'):
        fn = getattr(ops._C, name)
        monkeypatch.setattr(
            ops._C, name,
            lambda *a, _fn=fn, _n=name: (calls.append(_n), _fn(*a))[1])
    torch.manual_seed(19)
    m = NhwcConv3x3(Ci, 2 * Ci, 3, stride=2, padding=1,
                    bias=False).cuda().to(memory_format=CL)
    m.weight.data = m.weight.data.bfloat16()
    m.train()
    x = torch.randn(8, Ci, Wi, Wi, device='cuda').to(
        memory_format=CL).bfloat16().requires_grad_(True)
    with _s2bwd(True):
        y = m(x)
        y.float().square().mean().backward()
    assert sorted(calls) == ['conv3x3s2_dgrad', 'conv3x3s2_wrw']
    xr = x.detach().float().requires_grad_(True)
    wr = m.weight.detach().float().requires_grad_(True)
    F.conv2d(xr, wr, None, 2, 1).square().mean().backward()
    rel_x, rel_w = _rel(x.grad, xr.grad), _rel(m.weight.grad, wr.grad)
    print('module Ci%d rel dx %.5f dw %.5f' % (Ci, rel_x, rel_w))
    assert rel_x < 0.01, 'dx rel %.5f' % rel_x
    assert rel_w < 0.01, 'dw rel %.5f' % rel_w


def _resnet_step(s2bwd, defer=False):
    from types import SimpleNamespace
    from fedtorch_amd.ops import conv3x3 as c3
    from fedtorch_amd.components.models.resnet import resnet
    from fedtorch_amd.ops.batchnorm import convert_to_fused_bn
    old = c3._BNDEFER_ENABLED
    c3._BNDEFER_ENABLED = defer
    try:
        with _s2bwd(s2bwd):
            torch.manual_seed(41)
            args = SimpleNamespace(arch='resnet20', data='cifar10')
            m = resnet(args).cuda().to(memory_format=CL)
            convert_to_fused_bn(m)
            for p_ in m.parameters():
                if p_.dim() == 4:
                    p_.data = p_.data.bfloat16()
            m.train()
            torch.manual_seed(42)
            x = torch.randn(32, 3, 32, 32, device='cuda').to(
                memory_format=CL)
            with torch.autocast('cuda', dtype=torch.bfloat16):
                out = m(x)
                loss = out.float().square().mean()
            loss.backward()
            gs = [p_.grad.float().clone() for p_ in m.parameters()
                  if p_.grad is not None]
    finally:
        c3._BNDEFER_ENABLED = old
    return gs


def _assert_params_close(got, want):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        scale = b.abs().max().item() + 1e-5
        rel = (a - b).abs().max().item() / scale
        assert rel < 0.05, 'param %d rel %.4f' % (i, rel)


@pytest.fixture(scope='module')
def resnet_grads_off():
    return _resnet_step(False)


def test_s2_bwd_full_resnet_matches_library(resnet_grads_off):
    """a full ResNet-20 step with the stride-2 backward on the new kernels
    vs the same step with it on the library."""
    _assert_params_close(_resnet_step(True), resnet_grads_off)


def test_s2_bwd_full_resnet_with_bn_defer(resnet_grads_off):
    """both opt-ins together: the deferred-BN tag landing on a stride-2
    conv feeds the materialized dy_conv to the new kernels and the side
    table drains."""
    from fedtorch_amd.ops import conv3x3 as c3
    gs = _resnet_step(True, defer=True)
    assert not c3._BNBWD_TAGS, 'side table must drain'
    _assert_params_close(gs, resnet_grads_off)


def test_s2_bwd_launchers_reject_bad_arguments():
    Ci, Wi = 16, 32
    dy, x, w, _, _ = _case(Ci, Wi, 3)
    # wrong shape: a body (stride-1) conv's tensors, and a mismatched dy
    dy_s1 = torch.zeros(3, 16, 32, 32, device='cuda').to(
        memory_format=CL).bfloat16()
    w_s1 = torch.zeros(16, 16, 3, 3, device='cuda').to(
        memory_format=CL).bfloat16()
    with pytest.raises(RuntimeError):
        ops._C.conv3x3s2_dgrad(dy_s1, w_s1)
    with pytest.raises(RuntimeError):
        ops._C.conv3x3s2_wrw(dy_s1, x)
    with pytest.raises(RuntimeError):
        ops._C.conv3x3s2_wrw(dy[:2].contiguous(memory_format=CL), x)
    # wrong dtype
    with pytest.raises(RuntimeError):
        ops._C.conv3x3s2_dgrad(dy.float(), w.float())
    with pytest.raises(RuntimeError):
        ops._C.conv3x3s2_wrw(dy.float(), x.float())
    # not channels_last
    with pytest.raises(RuntimeError):
        ops._C.conv3x3s2_dgrad(dy.contiguous(), w)
    with pytest.raises(RuntimeError):
        ops._C.conv3x3s2_dgrad(dy, w.contiguous())
    with pytest.raises(RuntimeError):
        ops._C.conv3x3s2_wrw(dy.contiguous(), x)
    with pytest.raises(RuntimeError):
        ops._C.conv3x3s2_wrw(dy, x.contiguous())
