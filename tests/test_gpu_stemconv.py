# -*- coding: utf-8 -*-
"""NHWC stem convolution (hip/stemconv.h): stem_conv_fwd / stem_conv_wrw
bit-exact against a float64 reference on integer-valued inputs, for both
compiled Co, every input / output dtype, a 1x1 image (every tap but the
centre is padding), an odd non-square image and the native 32x32, plus the
weight-gradient launcher's argument checks.

x and dy hold integers in [-2, 2] and the fp32 weights integers in
{-1, 0, 1}, so every product and partial sum is an integer far below 2^24:
the fp32 accumulators, the in-LDS float atomics of the weight gradient and
its partial rows are exact in any order, and the comparisons are
torch.equal."""
import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

import fedtorch_amd.ops as ops

pytestmark = pytest.mark.gpu

DEV = 'cuda'
CL = torch.channels_last
F64 = torch.float64
EXACT = float(2 ** 24)
NHW = ((1, 1, 1), (3, 5, 7), (2, 32, 32))
DTYPES = ('float32', 'bfloat16')


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


def _dev(t, dtype='float32'):
    return t.float().to(DEV).to(memory_format=CL).to(getattr(torch, dtype))


def _first_diff(got, want):
    got, want = got.cpu(), want.cpu()
    bad = ((got != want) | (got != got)).nonzero()
    if bad.numel() == 0:
        return 'no mismatch'
    i = tuple(bad[0].tolist())
    return 'first mismatch at %s: got %s want %s (%d differ)' % (
        i, got[i].item(), want[i].item(), bad.shape[0])


@functools.lru_cache(maxsize=None)
def _case(Co, N, H, W):
    """integer (x, w, dy) in float64 and the float64 references (y, dw),
    computed once per shape and shared read-only"""
    g = _gen('stem', Co, N, H, W)
    x = _ints(g, -2, 2, N, 3, H, W)
    w = _ints(g, -1, 1, Co, 3, 3, 3)
    dy = _ints(g, -2, 2, N, Co, H, W)
    assert not torch.equal(w, w.flip(2, 3))
    assert not torch.equal(w, w.transpose(2, 3))
    # bounds on every partial sum: 27 products per output, N*H*W per dw
    assert 27 * x.abs().max().item() * w.abs().max().item() <= 256
    assert N * H * W * x.abs().max().item() * dy.abs().max().item() < EXACT
    y = F.conv2d(x, w, None, 1, 1)
    dw = torch.ops.aten.convolution_backward(
        dy, x, w, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1,
        [False, True, False])[1]
    return x, w, dy, y, dw


@pytest.mark.parametrize('out_bf16', (False, True), ids=('f32out', 'bf16out'))
@pytest.mark.parametrize('xdtype', DTYPES)
@pytest.mark.parametrize('N,H,W', NHW)
@pytest.mark.parametrize('Co', (16, 32))
def test_stem_fwd_exact(Co, N, H, W, xdtype, out_bf16):
    x, w, _dy, y64, _dw = _case(Co, N, H, W)
    y = ops._C.stem_conv_fwd(_dev(x, xdtype), _dev(w), out_bf16)
    want = y64.float().bfloat16() if out_bf16 else y64.float()
    assert y.dtype == want.dtype and y.shape == want.shape
    assert y.is_contiguous(memory_format=CL)
    assert torch.equal(y.cpu(), want), 'stem fwd Co%d N%d %dx%d x %s: %s' % (
        Co, N, H, W, xdtype, _first_diff(y, want))
    if (H, W) == (1, 1):
        # only the centre tap sees the image
        centre = torch.einsum('oc,nc->no', w[:, :, 1, 1], x[:, :, 0, 0])
        assert torch.equal(y.double().cpu().view(N, Co), centre)


@pytest.mark.parametrize('dydtype', DTYPES)
@pytest.mark.parametrize('xdtype', DTYPES)
@pytest.mark.parametrize('N,H,W', NHW)
@pytest.mark.parametrize('Co', (16, 32))
def test_stem_wrw_exact(Co, N, H, W, xdtype, dydtype):
    x, _w, dy, _y, dw64 = _case(Co, N, H, W)
    dw = ops._C.stem_conv_wrw(_dev(dy, dydtype), _dev(x, xdtype))
    assert dw.dtype == torch.float32 and dw.shape == (Co, 3, 3, 3)
    assert dw.is_contiguous(memory_format=CL)
    assert torch.equal(dw.cpu(), dw64.float()), \
        'stem wrw Co%d N%d %dx%d x %s dy %s (co, ci, kh, kw): %s' % (
            Co, N, H, W, xdtype, dydtype, _first_diff(dw, dw64.float()))
    if (H, W) == (1, 1):
        off_centre = dw.cpu().clone()
        off_centre[:, :, 1, 1] = 0
        assert (off_centre == 0).all().item()


def test_stem_conv_wrw_reject_bad_arguments():
    """every malformed tensor is at least as large in bytes as the
    well-formed one it replaces and lives on the GPU: a lost check could not
    turn into an out-of-bounds access here"""
    Co, N, H, W = 16, 3, 5, 7
    x64, _w, dy64, _y, _dw = _case(Co, N, H, W)
    x, dy = _dev(x64), _dev(dy64)
    f = ops._C.stem_conv_wrw
    f(dy, x)                                             # well-formed

    def zeros(*shape, dtype=torch.float32):
        return torch.zeros(shape, dtype=dtype, device=DEV).to(
            memory_format=CL)

    def rejects(*args):
        with pytest.raises(RuntimeError):
            f(*args)

    # dy does not match x in N, H, W
    rejects(zeros(N + 1, Co, H, W), x)
    rejects(zeros(N, Co, H + 1, W), x)
    rejects(zeros(N, Co, H, W + 1), x)
    rejects(zeros(N, Co, W, H + 2), x)                   # transposed, larger
    rejects(dy, zeros(N + 1, 3, H, W))
    # unsupported channel counts
    rejects(zeros(N, 24, H, W), x)
    rejects(dy, zeros(N, 4, H, W))
    # not floating point
    rejects(zeros(N, Co, H, W, dtype=torch.int32), x)
    rejects(dy, zeros(N, 3, H, W, dtype=torch.int32))
    # not channels_last
    rejects(torch.zeros(N, Co, H, W, device=DEV), x)
    rejects(dy, torch.zeros(N, 3, H, W, device=DEV))
