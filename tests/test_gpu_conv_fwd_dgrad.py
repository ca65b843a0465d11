# -*- coding: utf-8 -*-
"""MFMA conv forward (stride 1 and 2, with the FUSE_IN / HAS_RES / relu_in
staging variants), backward-data and the deferred-BN TRF dgrad
(hip/convfwd.h), plus the BN finalize that consumes the forward's stats
partials: bit-exact against a float64 reference on integer-valued inputs.

Small-integer bf16 inputs make every product and every partial sum an
integer far below 2^24, so the fp32 MFMA accumulators, the fused-input
values, the TRF values and the per-workgroup (sum, sumsq) partials are exact
in ANY summation order and the kernel's bf16 store is RNE of an exact fp32:
the comparisons are torch.equal, one missing / duplicated / misplaced term
fails.  Every exact test asserts that < 2^24 precondition on the reference
before it looks at the kernel output.  Random-valued companions cover the
inexact bf16 conversions of the staging path (rel < 0.01 of the reference
max, the sibling files' criterion), and the launchers' argument checks are
exercised with malformed tensors that are never smaller than the
well-formed ones they replace."""
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
SHAPES = ((16, 32), (32, 16), (64, 8))  # (C, W); Co = Ci = C
CO_TILE = {16: 16, 32: 32, 64: 32}      # channels per workgroup
S2_SHAPES = ((16, 32), (32, 16))        # (Ci, Wi); Co = 2*Ci, CO_TILE = 32
S2_NH = ((1, 16), (3, 32))              # (N, H_in)
VARIANTS = ('plain', 'fuse_relu', 'fuse_norelu', 'fuse_res_relu')


def _nh(W):
    """(N, H): one row block with both halo rows zero in the same workgroup;
    two row blocks (halo from the neighbour) with odd N; the native square"""
    return tuple(dict.fromkeys(((1, 8), (3, 16), (3, W))))


S1_CASES = [(C, W, N, H) for C, W in SHAPES for N, H in _nh(W)]
S2_CASES = [(Ci, Wi, N, HI) for Ci, Wi in S2_SHAPES for N, HI in S2_NH]
TRF_CASES = [(C, W, 3, 16) for C, W in SHAPES] + [(16, 32, 1, 8)]


def _gen(*key):
    """CPU generator seeded by the case's name (stable across runs)"""
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _ints(g, lo, hi, *shape):
    """float64 tensor of uniform integers in [lo, hi]"""
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


def _bf16_cl(t):
    return t.float().to(DEV).to(memory_format=CL).bfloat16()


def _f32(t):
    return t.float().to(DEV)


def _empty():
    return torch.empty(0, device=DEV)


def _nan_part(grid, Co):
    return torch.full((grid, Co, 2), float('nan'), device=DEV)


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
    want = want64.float().to(got.dtype)
    assert got.shape == want.shape, '%s shape %s' % (where, tuple(got.shape))
    assert torch.equal(got.cpu(), want), '%s %s' % (
        where, _first_diff(got, want))


def _expected_part(y64, tile):
    """[grid, C, 2] float64 partial rows of the stats epilogue: row
    (n*(H/8) + rb)*(C/tile) + cob holds (sum y, sum y^2) of image n's 8
    rows for channels [cob*tile, (cob+1)*tile) and 0 elsewhere.  Also
    asserts the exactness precondition of the partials."""
    N, C, H, W = y64.shape
    T = C // tile
    blk = y64.reshape(N, C, H // 8, 8 * W)
    assert blk.abs().sum(-1).max().item() < EXACT
    assert blk.square().sum(-1).max().item() < EXACT
    sq = torch.stack((blk.sum(-1), blk.square().sum(-1)), -1)  # [N,C,H/8,2]
    sq = sq.permute(0, 2, 1, 3)                                # [N,H/8,C,2]
    out = torch.zeros(N, H // 8, T, C, 2, dtype=F64)
    own = torch.zeros(N, H // 8, T, C, dtype=torch.bool)
    for t in range(T):
        ch = slice(t * tile, (t + 1) * tile)
        out[:, :, t, ch] = sq[:, :, ch]
        own[:, :, t, ch] = True
    return out.reshape(-1, C, 2), own.reshape(-1, C)


def _assert_part(part, want64, own, where):
    p = part.cpu()
    assert p.shape == want64.shape, '%s part shape' % where
    assert torch.isfinite(p).all().item(), \
        '%s part has unwritten/non-finite entries: %s' % (
            where, _first_diff(p, want64.float()))
    want = want64.float()
    assert torch.equal(p[own], want[own]), \
        '%s owned (row, channel, sum|sumsq): %s' % (
            where, _first_diff(p * own[..., None], want))
    assert (p[~own] == 0).all().item(), \
        '%s rows must hold 0.0 for channels of another workgroup: %s' % (
            where, _first_diff(p * ~own[..., None], want * 0))


# --------------------------------------------------------------------------
# forward, stride 1
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _s1_inputs(C, W, N, H):
    g = _gen('s1', C, W, N, H)
    x = _ints(g, -2, 2, N, C, H, W)
    w = _ints(g, -1, 1, C, C, 3, 3)
    a = _ints(g, -2, 2, C)
    b = _ints(g, -3, 3, C)
    res = _ints(g, -2, 2, N, C, H, W)
    assert not torch.equal(w, w.flip(2, 3)) and b.abs().max().item() > 0
    return x, w, a, b, res


@functools.lru_cache(maxsize=None)
def _s1_case(C, W, N, H, variant):
    """device inputs + the float64 reference (y, partial rows), computed
    once per case and shared read-only.  The transform applies to the image
    only: conv2d pads the TRANSFORMED input with zeros, so with b != 0 a
    kernel that transforms its halo gets a non-zero border."""
    x, w, a, b, res = _s1_inputs(C, W, N, H)
    xt = x
    if variant != 'plain':
        xt = a.view(1, C, 1, 1) * x + b.view(1, C, 1, 1)
        if variant == 'fuse_res_relu':
            xt = xt + res
        if variant != 'fuse_norelu':
            xt = xt.clamp_min(0)
        assert (xt != x).any().item()
    # every partial sum of the accumulators is bounded by this
    assert 9 * C * xt.abs().max().item() * w.abs().max().item() < EXACT
    y64 = F.conv2d(xt, w, None, 1, 1)
    part64, own = _expected_part(y64, CO_TILE[C])
    e = _empty()
    fuse = variant != 'plain'
    args = (_bf16_cl(x), _bf16_cl(w),
            _f32(a) if fuse else e, _f32(b) if fuse else e,
            _bf16_cl(res) if variant == 'fuse_res_relu' else e,
            variant in ('fuse_relu', 'fuse_res_relu'))
    return args, y64, part64, own


def _run_s1(args, part):
    x, w, a, b, res, relu_in = args
    return ops._C.conv3x3_bn_fwd(x, w, part, a, b, res, relu_in)


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('C,W,N,H', S1_CASES)
def test_fwd_s1_exact(C, W, N, H, variant):
    args, y64, part64, own = _s1_case(C, W, N, H, variant)
    where = 'fwd %s C%d W%d N%d H%d' % (variant, C, W, N, H)
    if variant != 'plain':
        # the variant must be visible in the result
        assert not torch.equal(y64, _s1_case(C, W, N, H, 'plain')[1])
    grid = N * (H // 8) * (C // CO_TILE[C])
    part = _nan_part(grid, C)
    y = _run_s1(args, part)
    assert y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=CL)
    _assert_exact(y, y64, where)
    _assert_part(part, part64, own, where)
    y2 = _run_s1(args, _empty())
    assert torch.equal(y2, y), '%s: y differs without ysum' % where


# --------------------------------------------------------------------------
# forward, stride 2
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _s2_case(Ci, Wi, N, HI):
    Co = 2 * Ci
    g = _gen('s2', Ci, Wi, N, HI)
    x = _ints(g, -2, 2, N, Ci, HI, Wi)
    w = _ints(g, -1, 1, Co, Ci, 3, 3)
    assert 9 * Ci * x.abs().max().item() * w.abs().max().item() < EXACT
    y64 = F.conv2d(x, w, None, 2, 1)
    part64, own = _expected_part(y64, 32)
    return (_bf16_cl(x), _bf16_cl(w)), y64, part64, own


@pytest.mark.parametrize('Ci,Wi,N,HI', S2_CASES)
def test_fwd_s2_exact(Ci, Wi, N, HI):
    (x, w), y64, part64, own = _s2_case(Ci, Wi, N, HI)
    Co = 2 * Ci
    where = 'fwd s2 Ci%d Wi%d N%d HI%d' % (Ci, Wi, N, HI)
    grid = N * (HI // 2 // 8) * (Co // 32)
    part = _nan_part(grid, Co)
    y = ops._C.conv3x3s2_bn_fwd(x, w, part)
    assert y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=CL)
    _assert_exact(y, y64, where)
    _assert_part(part, part64, own, where)
    y2 = ops._C.conv3x3s2_bn_fwd(x, w, _empty())
    assert torch.equal(y2, y), '%s: y differs without ysum' % where


# --------------------------------------------------------------------------
# backward-data, plain and TRF (deferred BN backward)
# --------------------------------------------------------------------------
def _ref_dgrad(dy64, w64):
    x = torch.zeros(dy64.shape[0], w64.shape[1], *dy64.shape[2:], dtype=F64)
    return torch.ops.aten.convolution_backward(
        dy64, x, w64, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1,
        [True, False, False])[0]


@functools.lru_cache(maxsize=None)
def _dgrad_case(C, W, N, H):
    g = _gen('dgrad', C, W, N, H)
    dy = _ints(g, -2, 2, N, C, H, W)
    w = _ints(g, -1, 1, C, C, 3, 3)
    # asymmetric in every sense a tap flip or a transpose could hide in
    assert not torch.equal(w, w.flip(2, 3))
    assert not torch.equal(w, w.flip(2)) and not torch.equal(w, w.flip(3))
    assert not torch.equal(w, w.transpose(2, 3))
    assert not torch.equal(w, w.transpose(0, 1))
    assert 9 * C * dy.abs().max().item() * w.abs().max().item() < EXACT
    return (_bf16_cl(dy), _bf16_cl(w)), _ref_dgrad(dy, w)


@pytest.mark.parametrize('C,W,N,H', S1_CASES)
def test_dgrad_exact(C, W, N, H):
    (dy, w), dx64 = _dgrad_case(C, W, N, H)
    dx = ops._C.conv3x3_dgrad(dy, w)
    assert dx.dtype == torch.bfloat16 and dx.is_contiguous(memory_format=CL)
    _assert_exact(dx, dx64, 'dgrad C%d W%d N%d H%d' % (C, W, N, H))


@functools.lru_cache(maxsize=None)
def _trf_case(C, W, N, H, relu):
    g = _gen('trf', C, W, N, H)
    dz = _ints(g, -2, 2, N, C, H, W)
    xbn = _ints(g, -2, 2, N, C, H, W)
    z = _ints(g, -1, 2, N, C, H, W)
    w = _ints(g, -1, 1, C, C, 3, 3)
    A = _ints(g, -2, 2, C)
    B = _ints(g, -3, 3, C)
    D = _ints(g, -2, 2, C)
    neg0 = (z == 0) & (torch.rand(z.shape, generator=g) < 0.5)
    z = torch.where(neg0, torch.full_like(z, -0.0), z)
    zero = z == 0
    assert (zero & torch.signbit(z)).any().item()       # -0.0 present
    assert (zero & ~torch.signbit(z)).any().item()      # +0.0 present
    assert not torch.equal(w, w.flip(2, 3))
    gm = dz * (z > 0) if relu else dz                   # +-0.0 are masked
    v = lambda t: t.view(1, C, 1, 1)
    dyc = v(A) * gm + v(B) + v(D) * xbn
    assert dyc.abs().max().item() <= 256                # exact in bf16
    assert 9 * C * dyc.abs().max().item() * w.abs().max().item() < EXACT
    dx = _ref_dgrad(dyc, w)
    zd = _bf16_cl(z)
    assert torch.equal(torch.signbit(zd.float().cpu()), torch.signbit(z))
    args = (_bf16_cl(dz), _bf16_cl(w), _bf16_cl(xbn), zd,
            _f32(torch.stack((A, B, D))).contiguous())
    return args, dx, dyc, gm


@pytest.mark.parametrize('want_dres', (False, True), ids=('nodres', 'dres'))
@pytest.mark.parametrize('relu', (False, True), ids=('norelu', 'relu'))
@pytest.mark.parametrize('C,W,N,H', TRF_CASES)
def test_dgrad_bn_exact(C, W, N, H, relu, want_dres):
    (dz, w, xbn, z, coefs), dx64, dyc64, g64 = _trf_case(C, W, N, H, relu)
    where = 'dgrad_bn C%d W%d N%d H%d relu%d dres%d' % (
        C, W, N, H, relu, want_dres)
    if relu:
        assert not torch.equal(g64, _trf_case(C, W, N, H, False)[3])
    # sentinel 7.0 is no value g can take; the buffer is either handed to
    # the kernel (dres) or only stands by as a decoy
    buf = torch.full_like(dz, 7.0)
    dres = buf if want_dres else torch.empty(0, device=DEV,
                                             dtype=torch.bfloat16)
    dx, dyc = ops._C.conv3x3_dgrad_bn(dz, w, xbn, z, coefs, relu, dres)
    for t in (dx, dyc):
        assert t.dtype == torch.bfloat16
        assert t.is_contiguous(memory_format=CL)
    _assert_exact(dyc, dyc64, where + ' dyc')
    _assert_exact(dx, dx64, where + ' dx')
    if want_dres:
        _assert_exact(buf, g64, where + ' dres')
    else:
        assert (buf == 7.0).all().item(), where + ': decoy buffer written'


# --------------------------------------------------------------------------
# random-valued companions: the inexact bf16 conversions of the staging
# --------------------------------------------------------------------------
def _rel(out, ref):
    return (out.double().cpu() - ref).abs().max().item() / \
        ref.abs().max().item()


@functools.lru_cache(maxsize=None)
def _rand_case(C, W, N):
    """random-normal (x, w, a, b, res, dy) on the device and their float64
    copies of the same bf16 / fp32 values"""
    g = _gen('rand', C, W, N)
    dev = {
        'x': _bf16_cl(torch.randn(N, C, W, W, generator=g)),
        'dy': _bf16_cl(torch.randn(N, C, W, W, generator=g)),
        'res': _bf16_cl(torch.randn(N, C, W, W, generator=g)),
        'w': _bf16_cl(torch.randn(C, C, 3, 3, generator=g) / (9 * C) ** .5),
        'a': _f32(torch.rand(C, generator=g) + 0.5),
        'b': _f32(torch.randn(C, generator=g) * 0.1),
    }
    return dev, {k: v.cpu().contiguous().double() for k, v in dev.items()}


@pytest.mark.parametrize('N', (1, 3))
@pytest.mark.parametrize('C,W', SHAPES)
def test_fwd_s1_random(C, W, N):
    d, r = _rand_case(C, W, N)
    e = _empty()
    y = ops._C.conv3x3_bn_fwd(d['x'], d['w'], e, e, e, e, False)
    rel = _rel(y, F.conv2d(r['x'], r['w'], None, 1, 1))
    print('fwd plain C%d N%d rel %.5f' % (C, N, rel))
    assert rel < 0.01, 'fwd plain C%d N%d rel %.5f' % (C, N, rel)
    # fused: the reference rounds x~ to bf16 before the conv, as the kernel
    xt = (r['a'].view(1, C, 1, 1) * r['x'] + r['b'].view(1, C, 1, 1)
          + r['res']).clamp_min(0).float().bfloat16().double()
    y = ops._C.conv3x3_bn_fwd(d['x'], d['w'], e, d['a'], d['b'], d['res'],
                              True)
    rel = _rel(y, F.conv2d(xt, r['w'], None, 1, 1))
    print('fwd fuse+res C%d N%d rel %.5f' % (C, N, rel))
    assert rel < 0.01, 'fwd fuse+res C%d N%d rel %.5f' % (C, N, rel)


@pytest.mark.parametrize('N', (1, 3))
@pytest.mark.parametrize('C,W', SHAPES)
def test_dgrad_random(C, W, N):
    d, r = _rand_case(C, W, N)
    dx = ops._C.conv3x3_dgrad(d['dy'], d['w'])
    rel = _rel(dx, _ref_dgrad(r['dy'], r['w']))
    print('dgrad C%d N%d rel %.5f' % (C, N, rel))
    assert rel < 0.01, 'dgrad C%d N%d rel %.5f' % (C, N, rel)


# --------------------------------------------------------------------------
# BN finalize from the forward's partial rows, both sides of the > 64 switch
# --------------------------------------------------------------------------
def _bf16_ulp(v64):
    """ulp of the bf16 binade that holds |v| (0 for v == 0)"""
    _m, e = torch.frexp(v64.abs())          # |v| = m * 2^e, m in [0.5, 1)
    return torch.where(v64 == 0, torch.zeros_like(v64),
                       torch.ldexp(torch.ones_like(v64), e - 8))


@pytest.mark.parametrize('C,W,H,N', [
    (16, 32, 32, 16), (16, 32, 32, 17),     # B = 64 | 68
    (32, 16, 16, 32), (32, 16, 16, 33),     # B = 64 | 66
    (64, 8, 8, 32), (64, 8, 8, 33),         # B = 64 | 66
])
def test_bn_finalize_from_partials(C, W, H, N):
    """save_mean / save_ivar / running stats at rtol 5e-6: the sums are exact
    (asserted), what remains is a handful of fp32 roundings in mean,
    q*inv_n - mean^2 and rsqrtf, each <= 2^-24 relative to E[y^2]; with
    E[y^2]/var <= 2 (asserted) that is < 1e-6 relative on ivar, 5e-6 leaves
    about 5x.  z within one bf16 ulp of |z|: beta puts every channel's zero
    crossing half way between two integers, so no integer y lands closer
    than 2^-9 to it (asserted) and the fp32 evaluation error (~1e-5
    absolute) stays below half a bf16 ulp of every non-zero z."""
    args, y64, _p, _o = _s1_case(C, W, N, H, 'plain')
    where = 'bn finalize C%d N%d H%d' % (C, N, H)
    grid = N * (H // 8) * (C // CO_TILE[C])
    assert (grid > 64) == (N % 2 == 1)
    assert grid <= 64 or grid % 32 != 0     # rows collapse into 32 unevenly
    NI = N * H * W
    s64, q64 = y64.sum((0, 2, 3)), y64.square().sum((0, 2, 3))
    assert y64.abs().sum((0, 2, 3)).max().item() < EXACT
    assert q64.max().item() < EXACT
    assert y64.abs().max().item() <= 256    # y itself is exact in bf16
    mean = s64 / NI
    var = q64 / NI - mean * mean
    assert ((q64 / NI) / var).max().item() <= 2.0
    eps, mom = 1e-5, 0.1
    ivar = (var + eps).rsqrt()
    g = _gen('bn', C, N)
    gamma = (torch.rand(C, generator=g) + 0.5).double()
    beta = (gamma * ivar * (mean - (mean.floor() + 0.5))).float().double()
    v = lambda t: t.view(1, C, 1, 1)
    f64 = (y64 - v(mean)) * v(ivar * gamma) + v(beta)
    assert f64.abs().min().item() >= 2.0 ** -9
    assert (f64 < 0).any().item() and (f64 > 0).any().item()
    z64 = f64.clamp_min(0)
    rm0 = mean.sign() * 0.25
    rv0 = torch.full((C,), 1.5, dtype=F64)
    rm, rv = _f32(rm0), _f32(rv0)

    part = _nan_part(grid, C)
    y = _run_s1(args, part)
    _assert_exact(y, y64, where + ' y')
    z, sm, siv, _ = ops._C.bn_fwd_train_part(
        y, part, _f32(gamma), _f32(beta), rm, rv, eps, mom, True, _empty())
    assert z.dtype == torch.bfloat16 and z.is_contiguous(memory_format=CL)

    def close(got, want, name):
        got = got.double().cpu()
        err = ((got - want).abs() / want.abs().clamp_min(1e-300)).max()
        print('%s %s max rel err %.3g' % (where, name, err.item()))
        assert torch.allclose(got, want, rtol=5e-6, atol=0), \
            '%s %s rel err %.3g' % (where, name, err.item())

    close(sm, mean, 'save_mean')
    close(siv, ivar, 'save_ivar')
    close(rm, (1 - mom) * rm0 + mom * mean, 'running_mean')
    close(rv, (1 - mom) * rv0 + mom * var * NI / (NI - 1), 'running_var')
    dz = (z.double().cpu() - z64).abs()
    ulps = torch.where(z64 == 0, dz, dz / _bf16_ulp(z64).clamp_min(1e-300))
    print('%s z max err %.3f bf16 ulp' % (where, ulps.max().item()))
    assert (dz <= _bf16_ulp(z64)).all().item(), \
        '%s z off by %.3f ulp' % (where, ulps.max().item())


# --------------------------------------------------------------------------
# determinism (no atomics anywhere in convfwd.h)
# --------------------------------------------------------------------------
@pytest.mark.parametrize('C,W', SHAPES)
def test_fwd_dgrad_deterministic(C, W):
    N = 3
    d, _r = _rand_case(C, W, N)
    grid = N * (W // 8) * (C // CO_TILE[C])

    def fwd():
        part = _nan_part(grid, C)
        y = ops._C.conv3x3_bn_fwd(d['x'], d['w'], part, d['a'], d['b'],
                                  d['res'], True)
        return y, part

    def dgrad_bn():
        coefs = torch.stack((d['a'], d['b'], d['a'] - 1.0)).contiguous()
        dres = torch.full_like(d['dy'], 7.0)
        dx, dyc = ops._C.conv3x3_dgrad_bn(d['dy'], d['w'], d['x'], d['res'],
                                          coefs, True, dres)
        return dx, dyc, dres

    for name, fn in (('fwd', fwd), ('dgrad_bn', dgrad_bn),
                     ('dgrad', lambda: (ops._C.conv3x3_dgrad(d['dy'],
                                                             d['w']),))):
        for i, (p, q) in enumerate(zip(fn(), fn())):
            assert torch.isfinite(p.float()).all().item(), (name, i)
            assert torch.equal(p, q), '%s C%d output %d' % (name, C, i)


@pytest.mark.parametrize('Ci,Wi', S2_SHAPES)
def test_fwd_s2_deterministic(Ci, Wi):
    N, Co = 3, 2 * Ci
    g = _gen('s2rand', Ci)
    x = _bf16_cl(torch.randn(N, Ci, Wi, Wi, generator=g))
    w = _bf16_cl(torch.randn(Co, Ci, 3, 3, generator=g) / (9 * Ci) ** .5)
    grid = N * (Wi // 2 // 8) * (Co // 32)
    outs = []
    for _ in range(2):
        part = _nan_part(grid, Co)
        outs.append((ops._C.conv3x3s2_bn_fwd(x, w, part), part))
    for i, (p, q) in enumerate(zip(*outs)):
        assert torch.isfinite(p.float()).all().item(), i
        assert torch.equal(p, q), 's2 fwd Ci%d output %d' % (Ci, i)


# --------------------------------------------------------------------------
# launcher argument checks.  Every malformed tensor is at least as large in
# bytes as the well-formed one it replaces and lives on the GPU, so a lost
# check could not turn into an out-of-bounds access here.
# --------------------------------------------------------------------------
def _nchw(t):
    """same sizes and dtype, NCHW-contiguous"""
    out = torch.zeros(t.shape, dtype=t.dtype, device=t.device)
    assert out.is_contiguous() and not out.is_contiguous(memory_format=CL)
    return out


def _zeros_cl(*shape, dtype=torch.bfloat16):
    return torch.zeros(shape, dtype=dtype, device=DEV).to(memory_format=CL)


def _rejects(fn, *args):
    with pytest.raises(RuntimeError):
        fn(*args)


def test_conv3x3_bn_fwd_reject_bad_arguments():
    C, W, N, H = 16, 32, 3, 16
    (x, w, a, b, res, _), _y, _p, _o = _s1_case(C, W, N, H, 'fuse_res_relu')
    f = ops._C.conv3x3_bn_fwd
    e = _empty()
    part = _nan_part(N * (H // 8), C)
    f(x, w, part, a, b, res, True)                       # well-formed
    # x
    _rejects(f, x.float(), w, part, a, b, res, True)
    _rejects(f, _nchw(x), w, part, a, b, res, True)
    _rejects(f, _zeros_cl(N, C, H + 4, W), w, e, a, b, e, True)  # H % 8
    # w: shape, dtype, layout
    _rejects(f, x, _zeros_cl(2 * C, C, 3, 3), part, a, b, res, True)
    _rejects(f, x, _zeros_cl(C, 2 * C, 3, 3), part, a, b, res, True)
    _rejects(f, x, _zeros_cl(C, C, 3, 5), part, a, b, res, True)
    _rejects(f, x, torch.zeros(C, C, 9, dtype=torch.bfloat16, device=DEV),
             part, a, b, res, True)                      # not 4-D
    _rejects(f, x, w.float(), part, a, b, res, True)
    _rejects(f, x, _nchw(w), part, a, b, res, True)
    # ysum: shape, dtype, layout
    _rejects(f, x, w, _nan_part(2 * N * (H // 8), C), a, b, res, True)
    _rejects(f, x, w, part.double(), a, b, res, True)
    _rejects(f, x, w, torch.zeros(N * (H // 8), C, 4, device=DEV)[..., ::2],
             a, b, res, True)
    # in_a / in_b: size, dtype, pairing
    a2, b2 = torch.cat((a, a)), torch.cat((b, b))
    _rejects(f, x, w, part, a2, b, res, True)
    _rejects(f, x, w, part, a, b2, res, True)
    _rejects(f, x, w, part, a2, b2, res, True)
    _rejects(f, x, w, part, a.double(), b, res, True)
    _rejects(f, x, w, part, a, b.double(), res, True)
    _rejects(f, x, w, part, a, e, res, True)
    _rejects(f, x, w, part, a2[::2], b, res, True)       # strided
    # res: shape, dtype, layout, and no residual without in_a / in_b
    _rejects(f, x, w, part, a, b, _zeros_cl(N + 1, C, H, W), True)
    _rejects(f, x, w, part, a, b, _zeros_cl(N, C, H + 8, W), True)
    _rejects(f, x, w, part, a, b, res.float(), True)
    _rejects(f, x, w, part, a, b, _nchw(res), True)
    _rejects(f, x, w, part, e, e, res, True)


def test_conv3x3s2_bn_fwd_reject_bad_arguments():
    Ci, Wi, N, HI = 16, 32, 3, 32
    Co = 2 * Ci
    (x, w), _y, _p, _o = _s2_case(Ci, Wi, N, HI)
    f = ops._C.conv3x3s2_bn_fwd
    grid = N * (HI // 16) * (Co // 32)
    part = _nan_part(grid, Co)
    f(x, w, part)                                        # well-formed
    _rejects(f, x.float(), w, part)
    _rejects(f, _nchw(x), w, part)
    _rejects(f, _zeros_cl(N, Ci, HI + 8, Wi), w, _empty())   # H_in % 16
    _rejects(f, x, _zeros_cl(2 * Co, Ci, 3, 3), part)
    _rejects(f, x, _zeros_cl(Co, 2 * Ci, 3, 3), part)
    _rejects(f, x, _zeros_cl(Co, Ci, 3, 5), part)
    _rejects(f, x, w.float(), part)
    _rejects(f, x, _nchw(w), part)
    _rejects(f, x, w, _nan_part(2 * grid, Co))
    _rejects(f, x, w, part.double())
    _rejects(f, x, w, torch.zeros(grid, Co, 4, device=DEV)[..., ::2])


def test_conv3x3_dgrad_reject_bad_arguments():
    C, W, N, H = 16, 32, 3, 16
    (dy, w), _dx = _dgrad_case(C, W, N, H)
    f = ops._C.conv3x3_dgrad
    f(dy, w)                                             # well-formed
    _rejects(f, dy.float(), w)
    _rejects(f, _nchw(dy), w)
    _rejects(f, _zeros_cl(N, C, H + 4, W), w)            # H % 8
    _rejects(f, dy, _zeros_cl(2 * C, C, 3, 3))
    _rejects(f, dy, _zeros_cl(C, 2 * C, 3, 3))
    _rejects(f, dy, _zeros_cl(C, C, 3, 5))
    _rejects(f, dy, w.float())
    _rejects(f, dy, _nchw(w))


def test_conv3x3_dgrad_bn_reject_bad_arguments():
    C, W, N, H = 16, 32, 3, 16
    (dz, w, xbn, z, coefs), _dx, _dyc, _g = _trf_case(C, W, N, H, True)
    f = ops._C.conv3x3_dgrad_bn
    dres = torch.full_like(dz, 7.0)
    f(dz, w, xbn, z, coefs, True, dres)                  # well-formed
    big = _zeros_cl(N + 1, C, H, W)
    tall = _zeros_cl(N, C, H + 8, W)
    _rejects(f, dz.float(), w, xbn, z, coefs, True, dres)
    _rejects(f, _nchw(dz), w, xbn, z, coefs, True, dres)
    # w: shape, dtype, layout
    _rejects(f, dz, _zeros_cl(2 * C, C, 3, 3), xbn, z, coefs, True, dres)
    _rejects(f, dz, _zeros_cl(C, 2 * C, 3, 3), xbn, z, coefs, True, dres)
    _rejects(f, dz, w.float(), xbn, z, coefs, True, dres)
    _rejects(f, dz, _nchw(w), xbn, z, coefs, True, dres)
    # xbn, z, dres: shape, dtype, layout
    for i in (2, 3, 6):
        for bad in (big, tall, dz.float(), _nchw(dz)):
            args = [dz, w, xbn, z, coefs, True, dres]
            args[i] = bad
            _rejects(f, *args)
    # coefs: dtype, size
    _rejects(f, dz, w, xbn, z, coefs.double(), True, dres)
    _rejects(f, dz, w, xbn, z, torch.cat((coefs, coefs), 1), True, dres)
    assert (dres.float() != 7.0).any().item()            # only the good call
