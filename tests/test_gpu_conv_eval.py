# -*- coding: utf-8 -*-
"""Inference kernels: conv3x3_bn_act_fwd (hip/convfwd.h
conv3x3_bn_act_fwd_k: 3x3 conv, stride 1 or 2, with the eval-mode
BN [+ residual] [+ ReLU] applied to the accumulators) and bn_fwd_eval
(hip/batchnorm.h bnh_eval_k), bit-exact against a float64 reference.

Exactness: x, w, res, gamma, beta and running_mean are small integers,
running_var is one of {0.25, 1, 4} and eps = 0, so 1/sqrt(var) is 2, 1 or
0.5 (IEEE sqrt and divide are exact there), the scale a = gamma/sqrt(var) is
one of 0, +-0.5 .. +-6 and the shift b = beta - mean*a a multiple of 0.5.
Every accumulator is an integer, every a*acc + b (+ res) a multiple of 0.5,
all far below 2^24: exact in fp32 in any order, with or without fma
contraction, and the kernel's store is RNE-to-bf16 of an exact fp32.  The
comparisons are torch.equal; each exact test asserts the < 2^24
precondition on its reference first.  Random-valued companions cover
inexact coefficients (rel < 0.01 of the reference max, the sibling files'
criterion).  Malformed arguments are never smaller than the well-formed
ones they replace."""
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
EXACT = float(2 ** 24)                  # integers below this are exact in fp32
SHAPES = ((16, 32), (32, 16), (64, 8))  # stride 1: (C, W); Co = Ci = C
S2_SHAPES = ((16, 32), (32, 16))        # stride 2: (Ci, Wi); Co = 2*Ci
S2_NH = ((1, 16), (3, 32))              # (N, H_in)
VARIANTS = ('relu', 'norelu', 'res_relu')
VARS = (0.25, 1.0, 4.0)


def _nh(W):
    """(N, H): one row block with both halo rows zero in the same workgroup;
    two row blocks (halo from the neighbour) with odd N; the native square"""
    return tuple(dict.fromkeys(((1, 8), (3, 16), (3, W))))


# (Ci, Wi, N, H_in, stride)
CASES = [(C, W, N, H, 1) for C, W in SHAPES for N, H in _nh(W)] + \
        [(Ci, Wi, N, HI, 2) for Ci, Wi in S2_SHAPES for N, HI in S2_NH]
NATIVE = [(C, W, 1) for C, W in SHAPES] + [(C, W, 2) for C, W in S2_SHAPES]


def _gen(*key):
    """CPU generator seeded by the case's name (stable across runs)"""
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _ints(g, lo, hi, *shape):
    """float64 tensor of uniform integers in [lo, hi]"""
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


def _cl(t, dtype=torch.bfloat16):
    return t.float().to(DEV).to(memory_format=CL).to(dtype)


def _f32(t):
    return t.float().to(DEV)


def _empty():
    return torch.empty(0, device=DEV)


def _first_diff(got, want):
    """index and values of the first mismatch ((n, c, h, w) for an
    activation), NaN included"""
    got, want = got.cpu(), want.cpu()
    bad = ((got != want) | (got != got)).nonzero()
    if bad.numel() == 0:
        return 'no mismatch'
    i = tuple(bad[0].tolist())
    return 'first mismatch at %s: got %s want %s (%d differ)' % (
        i, got[i].item(), want[i].item(), bad.shape[0])


def _assert_exact(got, want64, where):
    """got (bf16/fp32 from the kernel) must equal RNE(want64) bit for bit"""
    assert torch.isfinite(got.float()).all().item(), where + ': non-finite'
    want = want64.float().to(got.dtype)
    assert got.shape == want.shape, '%s shape %s' % (where, tuple(got.shape))
    assert torch.equal(got.cpu(), want), '%s %s' % (
        where, _first_diff(got, want))


def _exact_coefs(g, C):
    """(gamma, beta, mean, var) float64 [C] and the folded (a, b): gamma has
    a 0, a negative and a positive entry, var takes all three values"""
    gamma = _ints(g, -3, 3, C)
    gamma[:3] = torch.tensor([0., -3., 2.], dtype=F64)
    beta = _ints(g, -4, 4, C)
    mean = _ints(g, -4, 4, C)
    var = torch.tensor(VARS, dtype=F64)[
        torch.randint(0, 3, (C,), generator=g)]
    var[:3] = torch.tensor(VARS, dtype=F64)
    a = gamma / var.sqrt()
    b = beta - mean * a
    for t in (a, b):                         # multiples of 0.5
        assert (t * 2 == (t * 2).round()).all().item()
    assert a.abs().max().item() <= 6 and (mean * a != 0).any().item()
    return (gamma, beta, mean, var), a, b


def _v(t):
    return t.view(1, -1, 1, 1)


def _apply(y64, a, b, res, relu):
    out = _v(a) * y64 + _v(b)
    if res is not None:
        out = out + res
    return out.clamp_min(0) if relu else out


# --------------------------------------------------------------------------
# conv3x3_bn_act_fwd, exact
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _conv_inputs(Ci, Wi, N, HI, stride):
    """device tensors + the float64 conv output and folded coefficients,
    computed once per case and shared read-only"""
    Co = Ci * stride
    g = _gen('eval', Ci, Wi, N, HI, stride)
    x = _ints(g, -2, 2, N, Ci, HI, Wi)
    w = _ints(g, -1, 1, Co, Ci, 3, 3)
    res = _ints(g, -3, 3, N, Co, HI // stride, Wi // stride)
    coefs, a, b = _exact_coefs(g, Co)
    assert not torch.equal(w, w.flip(2, 3))
    assert 9 * Ci * x.abs().max().item() * w.abs().max().item() < EXACT
    conv64 = F.conv2d(x, w, None, stride, 1)
    # multiples of 0.5: twice the largest intermediate must stay exact
    bound = _v(a.abs()) * conv64.abs() + _v(b.abs()) + res.abs()
    assert 2 * bound.max().item() < EXACT
    dev = (_cl(x), _cl(w)) + tuple(_f32(t) for t in coefs) + (_cl(res),)
    return dev, conv64, a, b, res


def _run_conv(dev, variant, eps=0.0):
    x, w, gamma, beta, mean, var, res = dev
    return ops._C.conv3x3_bn_act_fwd(
        x, w, gamma, beta, mean, var, eps, variant != 'norelu',
        res if variant == 'res_relu' else _empty(), _dev_stride(dev))


def _dev_stride(dev):
    return dev[1].shape[0] // dev[1].shape[1]


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('Ci,Wi,N,HI,stride', CASES)
def test_conv_bn_act_exact(Ci, Wi, N, HI, stride, variant):
    dev, conv64, a, b, res = _conv_inputs(Ci, Wi, N, HI, stride)
    where = 'conv_bn_act %s Ci%d Wi%d N%d H%d s%d' % (
        variant, Ci, Wi, N, HI, stride)
    ref = _apply(conv64, a, b, res if variant == 'res_relu' else None,
                 variant != 'norelu')
    # each part of the epilogue must be visible in the reference
    assert not torch.equal(ref, conv64)
    if variant != 'norelu':
        assert (_apply(conv64, a, b, res if variant == 'res_relu' else None,
                       False) < 0).any().item()
    if variant == 'res_relu':
        assert not torch.equal(ref, _apply(conv64, a, b, None, True))
    y = _run_conv(dev, variant)
    assert y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=CL)
    _assert_exact(y, ref, where)


# --------------------------------------------------------------------------
# conv3x3_bn_act_fwd, random values + determinism
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rand_case(Ci, Wi, stride):
    N, Co, Wo = 3, Ci * stride, Wi // stride
    g = _gen('evalrand', Ci, Wi, stride)
    dev = (
        _cl(torch.randn(N, Ci, Wi, Wi, generator=g)),
        _cl(torch.randn(Co, Ci, 3, 3, generator=g) / (9 * Ci) ** .5),
        _f32(torch.randn(Co, generator=g)),                 # gamma
        _f32(torch.randn(Co, generator=g)),                 # beta
        _f32(torch.randn(Co, generator=g)),                 # running_mean
        _f32(torch.rand(Co, generator=g) * 1.5 + 0.5),      # running_var
        _cl(torch.randn(N, Co, Wo, Wo, generator=g)),       # res
    )
    return dev, tuple(t.cpu().contiguous().double() for t in dev)


@pytest.mark.parametrize('Ci,Wi,stride', NATIVE)
def test_conv_bn_act_random(Ci, Wi, stride):
    eps = 1e-5
    dev, (x, w, gamma, beta, mean, var, res) = _rand_case(Ci, Wi, stride)
    a = gamma / (var + eps).sqrt()
    b = beta - mean * a
    ref = _apply(F.conv2d(x, w, None, stride, 1), a, b, res, True)
    y = _run_conv(dev, 'res_relu', eps)
    err = (y.double().cpu() - ref).abs().max().item()
    rel = err / ref.abs().max().item()
    print('conv_bn_act random Ci%d s%d rel %.5f' % (Ci, stride, rel))
    assert torch.isfinite(y.float()).all().item()
    assert rel < 0.01, 'Ci%d s%d rel %.5f' % (Ci, stride, rel)


@pytest.mark.parametrize('Ci,Wi,stride', NATIVE)
def test_conv_bn_act_deterministic(Ci, Wi, stride):
    dev, _ = _rand_case(Ci, Wi, stride)
    for variant in ('res_relu', 'norelu'):
        p, q = _run_conv(dev, variant, 1e-5), _run_conv(dev, variant, 1e-5)
        assert torch.isfinite(p.float()).all().item()
        assert torch.equal(p, q), 'Ci%d s%d %s' % (Ci, stride, variant)


# --------------------------------------------------------------------------
# conv3x3_bn_act_fwd argument checks.  Every malformed tensor is at least as
# large in bytes as the well-formed one it replaces, so a lost check could
# not turn into an out-of-bounds access here.
# --------------------------------------------------------------------------
def _nchw(t):
    """same sizes and dtype, NCHW-contiguous"""
    out = torch.zeros(t.shape, dtype=t.dtype, device=t.device)
    assert out.is_contiguous() and not out.is_contiguous(memory_format=CL)
    return out


def _zeros_cl(*shape, dtype=torch.bfloat16):
    return torch.zeros(shape, dtype=dtype, device=DEV).to(memory_format=CL)


def _rejects(fn, *args):
    with pytest.raises(RuntimeError, match=fn.__name__):
        fn(*args)


def test_conv_bn_act_reject_bad_arguments():
    f = ops._C.conv3x3_bn_act_fwd
    # stride 1
    C, W, N, H = 16, 32, 3, 16
    (x, w, ga, be, mu, va, res), *_ = _conv_inputs(C, W, N, H, 1)
    f(x, w, ga, be, mu, va, 0.0, True, res, 1)           # well-formed
    vecs = (ga, be, mu, va)
    _rejects(f, x.float(), w, *vecs, 0.0, True, res, 1)  # wrong dtype
    _rejects(f, x, w.float(), *vecs, 0.0, True, res, 1)
    _rejects(f, x, w, *vecs, 0.0, True, res.float(), 1)
    _rejects(f, _nchw(x), w, *vecs, 0.0, True, res, 1)   # NCHW layout
    _rejects(f, x, _nchw(w), *vecs, 0.0, True, res, 1)
    _rejects(f, x, w, *vecs, 0.0, True, _nchw(res), 1)
    _rejects(f, _zeros_cl(N, C, H + 4, W), w, *vecs, 0.0, True, _empty(),
             1)                                          # H % 8
    _rejects(f, x, w, *vecs, 0.0, True, res, 3)          # stride
    _rejects(f, x, w, *vecs, 0.0, True, res, 2)          # s2 needs Co = 2*Ci
    for i in range(4):
        for bad in (torch.zeros(C + 1, device=DEV),      # [Co+1]
                    torch.zeros(C),                      # on the CPU
                    torch.zeros(C, device=DEV, dtype=F64),
                    torch.zeros(2 * C, device=DEV)[::2]):    # strided
            v = list(vecs)
            v[i] = bad
            _rejects(f, x, w, *v, 0.0, True, res, 1)
    # stride 2: res is checked against the OUTPUT shape
    Ci, Wi, HI = 16, 32, 32
    (x2, w2, ga2, be2, mu2, va2, res2), *_ = _conv_inputs(Ci, Wi, N, HI, 2)
    vecs2 = (ga2, be2, mu2, va2)
    f(x2, w2, *vecs2, 0.0, True, res2, 2)                # well-formed
    _rejects(f, x2, w2, *vecs2, 0.0, True, torch.zeros_like(x2), 2)
    _rejects(f, x2, w2, *vecs2, 0.0, True,
             _zeros_cl(N, 2 * Ci, HI, Wi), 2)            # input H, W
    _rejects(f, _zeros_cl(N, Ci, HI + 8, Wi), w2, *vecs2, 0.0, True,
             _empty(), 2)                                # H_in % 16
    _rejects(f, x2, w2, *vecs2, 0.0, True, res2, 1)      # s1 needs Co = Ci


# --------------------------------------------------------------------------
# bn_fwd_eval, exact
# --------------------------------------------------------------------------
BN_NHW = ((3, 7, 9),     # vector count no multiple of the block
          (1, 1, 1),
          (2, 8, 32))    # more than one block


@functools.lru_cache(maxsize=None)
def _bn_inputs(C, N, H, W):
    g = _gen('bneval', C, N, H, W)
    x = _ints(g, -8, 8, N, C, H, W)
    res = _ints(g, -3, 3, N, C, H, W)
    coefs, a, b = _exact_coefs(g, C)
    assert 2 * (_v(a.abs()) * x.abs() + _v(b.abs()) + res.abs()
                ).max().item() < EXACT
    return x, res, tuple(_f32(t) for t in coefs), a, b


@pytest.mark.parametrize('relu', (False, True), ids=('norelu', 'relu'))
@pytest.mark.parametrize('has_res', (False, True), ids=('nores', 'res'))
@pytest.mark.parametrize('N,H,W', BN_NHW)
@pytest.mark.parametrize('C', (16, 32, 64))
@pytest.mark.parametrize('dtype', (torch.bfloat16, torch.float32),
                         ids=('bf16', 'fp32'))
def test_bn_fwd_eval_exact(dtype, C, N, H, W, has_res, relu):
    x, res, vecs, a, b = _bn_inputs(C, N, H, W)
    where = 'bn_fwd_eval %s C%d %s res%d relu%d' % (
        dtype, C, (N, H, W), has_res, relu)
    ref = _apply(x, a, b, res if has_res else None, relu)
    assert not torch.equal(ref, x)
    y = ops._C.bn_fwd_eval(_cl(x, dtype), *vecs, 0.0, relu,
                           _cl(res, dtype) if has_res else _empty())
    assert y.dtype == dtype and y.is_contiguous(memory_format=CL)
    _assert_exact(y, ref, where)


def test_bn_fwd_eval_random_and_rejects():
    f = ops._C.bn_fwd_eval
    C, N, H, W = 32, 3, 7, 9
    g = _gen('bnrand')
    x = _cl(torch.randn(N, C, H, W, generator=g))
    res = _cl(torch.randn(N, C, H, W, generator=g))
    vecs = (_f32(torch.randn(C, generator=g)),
            _f32(torch.randn(C, generator=g)),
            _f32(torch.randn(C, generator=g)),
            _f32(torch.rand(C, generator=g) * 1.5 + 0.5))
    ga, be, mu, va = (t.double().cpu() for t in vecs)
    a = ga / (va + 1e-5).sqrt()
    ref = _apply(x.double().cpu(), a, be - mu * a, res.double().cpu(), True)
    y = f(x, *vecs, 1e-5, True, res)
    rel = (y.double().cpu() - ref).abs().max().item() / ref.abs().max().item()
    print('bn_fwd_eval random rel %.5f' % rel)
    assert rel < 0.01
    assert torch.equal(y, f(x, *vecs, 1e-5, True, res))
    _rejects(f, _nchw(x), *vecs, 1e-5, True, res)
    _rejects(f, x, *vecs, 1e-5, True, res.float())
    _rejects(f, x, *vecs, 1e-5, True, _zeros_cl(N + 1, C, H, W))
    _rejects(f, x, torch.zeros(C + 1, device=DEV), *vecs[1:], 1e-5, True, res)
    _rejects(f, x, *vecs[:3], torch.zeros(C), 1e-5, True, res)
    _rejects(f, x.double(), *vecs, 1e-5, True, _empty())
    _rejects(f, _zeros_cl(N, 24, H, W), *(torch.zeros(24, device=DEV),) * 4,
             1e-5, True, _empty())                       # 3 channel groups
