# -*- coding: utf-8 -*-
"""Case generators and the float64 reference for the BatchNorm training
kernels (hip/batchnorm.h), shared by tests/test_gpu_batchnorm.py (GPU) and
tests/test_bn_reference_cpu.py (no GPU).  Imports torch only.

The reference is BatchNorm written out from its formulas in float64:

  forward   mean = sum(x)/n, var = sum(x^2)/n - mean^2 (biased),
            ivar = 1/sqrt(var + eps), f = (x - mean)*ivar*gamma + beta + res,
            y = relu(f); running_mean += mom*(mean - running_mean),
            running_var likewise with the UNBIASED variance var*n/(n-1)
  backward  g = dy where y > 0 else 0 (relu) -- also the residual's gradient,
            xhat = (x - mean)*ivar, dbeta = sum(g), dgamma = sum(g*xhat),
            dx = gamma*ivar*(g - dbeta/n - xhat*dgamma/n)

with n = N*H*W per channel.  The backward takes mean/ivar from the caller
(the kernels read them from save_mean/save_ivar), so a test may pass
integers and powers of two and get an exactly representable result.

Every case builder asserts the preconditions its comparison rests on (sums
exact in fp32 in any order, representable intermediates, both signs present,
zero crossings away from every input) before it returns, so building all
cases on a machine without a GPU proves the reference alone meets them."""
import functools
import zlib

import torch

F64 = torch.float64
EXACT = float(2 ** 24)      # integers below this are exact in fp32
U = 2.0 ** -24              # fp32 unit roundoff
EPS = 1e-5
DTYPES = {'bf16': torch.bfloat16, 'fp32': torch.float32}
VN = {'bf16': 8, 'fp32': 4}  # elements per 16-byte vector
BLOCK = 256                 # threads per workgroup (FT_BLOCK)


def gen(*key):
    """CPU generator seeded by the case's name (stable across runs)"""
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def ints(g, lo, hi, *shape):
    """float64 tensor of uniform integers in [lo, hi]"""
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


def pick(g, values, n):
    v = torch.tensor(values, dtype=F64)
    return v[torch.randint(0, len(values), (n,), generator=g)]


def is_pow2(n):
    return n >= 1 and (n & (n - 1)) == 0


def fp32_exact(t):
    """every entry of the float64 tensor is an fp32 number"""
    return torch.equal(t.float().double(), t)


def bf16_ulp(v64):
    """ulp of the bf16 binade that holds |v| (0 for v == 0)"""
    _m, e = torch.frexp(v64.abs())          # |v| = m * 2^e, m in [0.5, 1)
    return torch.where(v64 == 0, torch.zeros_like(v64),
                       torch.ldexp(torch.ones_like(v64), e - 8))


def per_channel(t):
    """[N, C, H, W] -> [C, N*H*W] (a copy)"""
    return t.permute(1, 0, 2, 3).reshape(t.shape[1], -1)


def from_per_channel(m, shape):
    N, C, H, W = shape
    return m.reshape(C, N, H, W).permute(1, 0, 2, 3).contiguous()


def vc(t):
    return t.view(1, -1, 1, 1)


def pack_mask(y):
    """the ReLU bitmask of the NHWC bf16 kernels: bit (e & 7) of byte
    (e >> 3) is y > 0, e the flat NHWC element index"""
    bits = (y.permute(0, 2, 3, 1).reshape(-1, 8) > 0).to(torch.int64)
    weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128])
    return (bits * weights).sum(1).to(torch.uint8)


# --------------------------------------------------------------------------
# shapes
# --------------------------------------------------------------------------
def rows_per_pass(C, dt):
    """rows one 256-thread pass of the NHWC kernels covers: a thread owns one
    16-byte channel group of one row"""
    return BLOCK // (C // VN[dt])


def _nhw(rows):
    if rows == 1:
        return (1, 1, 1)
    if rows == 1024:
        return (4, 16, 16)
    if rows % 3 == 0 and rows > 3:
        return (3, 1, rows // 3)
    return (1, 1, rows)


def _cl_shapes():
    out = []
    for dt in ('bf16', 'fp32'):
        for C in (VN[dt], 16, 32, 64, 256):
            rp = rows_per_pass(C, dt)
            # 1 row (a 1x1 map is also NCHW-contiguous: the launcher routes
            # it to the NCHW kernels), 3, one below / above a single pass,
            # a power of two
            for rows in sorted({1, 3, rp - 1, rp + 1, 1024}):
                out.append(('cl', dt, C) + _nhw(rows))
    return out


# 66560 rows x 8 groups: 260 reduce iterations of work for a 256-block cap,
# 2080 blocks of elementwise work for a 1024-block cap -- both caps bind,
# every thread loops, the last pass is ragged
CL_LARGE = ('cl', 'bf16', 64, 65, 32, 32)
CL_SHAPES = _cl_shapes()

# (layout, dtype, C, N, H, W); HW = 64 is the vector path for both types,
# HW = 49 the scalar path for both, HW = 4 vector for fp32 / scalar for bf16
NCHW_SHAPES = [('nchw', dt, C, N, H, W) for dt in ('bf16', 'fp32')
               for C, N, H, W in (
                   (3, 2, 8, 8),        # vector, 1 block per channel
                   (2, 31, 8, 8),       # one below a full 256-thread pass
                   (2, 33, 8, 8),       # one above (bf16) / two passes
                   (3, 16, 8, 8),       # 1024 rows, power of two
                   (5, 3, 7, 7),        # scalar
                   (3, 5, 2, 2),        # HW = 4
                   (3, 64, 2, 2),       # HW = 4, power-of-two rows
                   (8, 1, 1, 1),        # 1 row
               )]
# 65 x 1024 rows at C = 32: 33 blocks of work per channel against caps of
# 512/C = 16 reduce and 1024/C = 32 elementwise blocks -- ragged last pass
NCHW_LARGE = ('nchw', 'bf16', 32, 65, 32, 32)

SHAPES = CL_SHAPES + NCHW_SHAPES
LARGE = [CL_LARGE, NCHW_LARGE]
BWD_FLAGS = [(False, False), (False, True), (True, False), (True, True)]
# (relu, has_res, affine, track)
FWD_FLAGS = [(False, False, False, False), (True, False, False, True),
             (True, False, True, True), (True, True, True, True),
             (False, True, True, False)]
FWD_SHAPES = [s for s in SHAPES if s[3] * s[4] * s[5] > 1]


def case_id(c):
    return '%s-%s-C%d-%dx%dx%d' % c


def rows_of(case):
    return case[3] * case[4] * case[5]


def mask_ok(case):
    """the bitmask exists for bf16 channels_last only (and a 1x1 map is not
    channels_last for the launcher)"""
    _l, dt, C, N, H, W = case
    return case[0] == 'cl' and dt == 'bf16' and H * W > 1


# --------------------------------------------------------------------------
# backward
# --------------------------------------------------------------------------
def ref_bwd(x, dy, y, mean, ivar, w, relu):
    """float64 BatchNorm backward from the formulas; w None = no affine"""
    NI = x.shape[0] * x.shape[2] * x.shape[3]
    C = x.shape[1]
    g = torch.where(y <= 0, torch.zeros_like(dy), dy) if relu else dy
    xhat = (x - vc(mean)) * vc(ivar)
    s1 = g.sum((0, 2, 3))
    s2 = (g * xhat).sum((0, 2, 3))
    mdy, mdyxh = s1 / NI, s2 / NI
    k1 = (w if w is not None else torch.ones(C, dtype=F64)) * ivar
    t1 = g - vc(mdy)
    prod = xhat * vc(mdyxh)
    br = t1 - prod
    return {'g': g, 'xhat': xhat, 'dbias': s1, 'dweight': s2, 'mdy': mdy,
            'mdyxh': mdyxh, 'k1': k1, 't1': t1, 'prod': prod, 'br': br,
            'dx': vc(k1) * br, 'dres': g,
            # the magnitude the fp32 roundings of dx are relative to
            'scale': vc(k1).abs() * (g.abs() + vc(mdy).abs() + prod.abs())}


@functools.lru_cache(maxsize=None)
def bwd_inputs(case):
    """integer x / dy / y / save_mean, power-of-two save_ivar and weight;
    the same tensors for every flag combination of a case"""
    _l, dt, C, N, H, W = case
    NI = N * H * W
    g = gen('bwd', case)
    R = 2 if NI > 4096 else 4            # keeps the big sums exact
    shape = (N, C, H, W)
    x = ints(g, -R, R, *shape)
    dy = per_channel(ints(g, -R, R, *shape))
    y = per_channel(ints(g, -2, 2, *shape))
    if NI >= 3:
        # zero, negative and positive y in every channel, and a non-zero dy
        # on the zero so that masking y < 0 instead of y <= 0 changes sums
        y[:, 0], y[:, 1], y[:, 2] = 0, -1, 2
        dy[:, 0], dy[:, 2] = 3, -3
    else:
        for r in range(NI):
            y[:, r] = (torch.arange(C) + r) % 3 - 1
        dy[dy == 0] = 1
    y, dy = from_per_channel(y, shape), from_per_channel(dy, shape)
    mean = ints(g, -1, 1, C)
    ivar = pick(g, (0.5, 1.0, 2.0), C)
    w = pick(g, (-1.0, 0.5, 1.0, 2.0), C)
    if C >= 4:
        assert len(set((w * ivar).tolist())) > 1      # varies per channel
    return {'x': x, 'dy': dy, 'y': y, 'mean': mean, 'ivar': ivar, 'w': w}


@functools.lru_cache(maxsize=None)
def bwd_case(case, relu, affine=True):
    """(inputs, reference, exact): preconditions asserted.  exact says dx
    (and the deferred coefficients) are exactly representable, i.e. the rows
    are a power of two and every intermediate of the kernel's expression is
    an fp32 number, so contraction to FMA cannot change the result."""
    i = bwd_inputs(case)
    NI = rows_of(case)
    r = ref_bwd(i['x'], i['dy'], i['y'], i['mean'], i['ivar'],
                i['w'] if affine else None, relu)
    # g*xhat are multiples of 1/2: below 2^23 every partial sum, in any
    # order, is an fp32 number
    assert r['g'].abs().sum((0, 2, 3)).max().item() < EXACT / 2
    assert (r['g'] * r['xhat']).abs().sum((0, 2, 3)).max().item() < EXACT / 2
    assert i['x'].abs().max().item() <= 256 and \
        i['dy'].abs().max().item() <= 256        # exact in bf16
    if relu and NI >= 3:
        yc = per_channel(i['y'])
        assert ((yc == 0).any(1) & (yc < 0).any(1) & (yc > 0).any(1)).all()
        assert ((yc == 0) & (per_channel(i['dy']) != 0)).any(1).all()
    exact = is_pow2(NI)
    if exact:
        for k in ('mdy', 'mdyxh', 'xhat', 'prod', 't1', 'br', 'dx'):
            assert fp32_exact(r[k]), '%s %s not representable' % (case, k)
    return i, r, exact


def dx_bound(r, dt):
    """|dx - dx64| allowed when 1/n is inexact.  With u = 2^-24:
    inv_n = fl(1/n) is within 3u (division need not be correctly rounded on
    the device), mdy = fl(s1*inv_n) and mdyxh likewise within 4u (the sums
    are exact); t1 = fl(g - mdy) errs by u|t1| + 4u|mdy|; the bracket
    fl(t1 - xhat*mdyxh), fused or not, adds u|br| + 5u|xhat*mdyxh|; xhat and
    the product with the power-of-two k1 are exact.  With |t1| <= |g| + |mdy|
    and |br| <= |g| + |mdy| + |xhat*mdyxh| that is at most
    6u * |k1| * (|g| + |mdy| + |xhat*mdyxh|); the bound is 8u of it (1.33x
    slack).  A bf16 store adds half a bf16 ulp of the stored value."""
    b = 8 * U * r['scale']
    if dt == 'bf16':
        b = b + 0.5 * bf16_ulp(r['dx'].abs() + b)
    return b


# --------------------------------------------------------------------------
# deferred backward: dx = A*g + Bc + D*x
# --------------------------------------------------------------------------
DEFER_CASES = [
    ('cl', 'bf16', 16, 4, 16, 16),      # 1 block of partials
    ('cl', 'bf16', 64, 3, 5, 7),        # odd rows
    ('cl', 'fp32', 64, 4, 16, 16),
    ('cl', 'bf16', 64, 17, 32, 32),     # 68 blocks > 64: partials collapse
    ('cl', 'bf16', 256, 8, 32, 32),     # C = 256, 128 blocks: wide collapse
]
DEFER_FLAGS = [(False, False), (True, False), (True, True)]  # relu, has_res


def defer_blocks(case):
    """reduce blocks bn_bwd_defer launches (256 threads x 8 iterations each,
    at most 256)"""
    _l, dt, C, N, H, W = case
    tasks = N * H * W * (C // VN[dt])
    return max(1, min(256, -(-tasks // (BLOCK * 8))))


@functools.lru_cache(maxsize=None)
def defer_case(case, relu):
    i, r, exact = bwd_case(case, relu)
    A = r['k1']
    mi = i['mean'] * i['ivar']
    p = mi * r['mdyxh']
    inner = p - r['mdy']
    coefs = torch.stack((A, A * inner, -A * i['ivar'] * r['mdyxh']))
    if exact:
        assert fp32_exact(p) and fp32_exact(inner) and fp32_exact(coefs)
    # mdy, mdyxh within 4u (see dx_bound); fl(fma(mean*ivar, mdyxh, -mdy))
    # adds u|inner|: 5u(|mean*ivar*mdyxh| + |mdy|) on row 1, 4u on row 2,
    # row 0 exact.  8u of those magnitudes (<= 2x slack).
    bound = 8 * U * torch.stack((
        torch.zeros_like(A), A.abs() * (p.abs() + r['mdy'].abs()),
        (A * i['ivar'] * r['mdyxh']).abs()))
    return i, r, coefs, bound, exact


# --------------------------------------------------------------------------
# forward
# --------------------------------------------------------------------------
def ref_fwd(x, w, b, res, relu, eps, mom, rm0, rv0):
    """float64 BatchNorm forward from the formulas.  w/b/res/rm0 may be
    None."""
    NI = x.shape[0] * x.shape[2] * x.shape[3]
    s, q = x.sum((0, 2, 3)), x.square().sum((0, 2, 3))
    mean = s / NI
    var = q / NI - mean * mean
    ivar = (var + eps).rsqrt()
    scale = ivar * w if w is not None else ivar
    f = (x - vc(mean)) * vc(scale)
    if b is not None:
        f = f + vc(b)
    if res is not None:
        f = f + res
    out = {'s': s, 'q': q, 'mean': mean, 'var': var, 'ivar': ivar,
           'scale': scale, 'f': f, 'y': f.clamp_min(0) if relu else f}
    if rm0 is not None:
        unbiased = var * NI / max(NI - 1, 1)
        out['rm'] = (1 - mom) * rm0 + mom * mean
        out['rv'] = (1 - mom) * rv0 + mom * unbiased
    return out


def _centered_x(g, shape, R):
    """integers with, per channel, a spread of at least 2R and a mean whose
    distance to the nearest integer is >= 1/4 and whose magnitude is
    <= 1/2 + 1/n: E[x^2]/var stays small and no integer sits on the zero
    crossing of (x - mean)"""
    N, C, H, W = shape
    NI = N * H * W
    assert NI >= 2
    xv = per_channel(ints(g, -R, R, *shape))
    xv[:, 0], xv[:, 1] = R, -R
    s = xv.sum(1)
    xv -= (s / NI).round().view(C, 1)
    s = xv.sum(1)
    m = torch.where(s.abs() * 4 < NI, -(-NI // 4) - s, torch.zeros_like(s))
    xv += (torch.arange(NI).view(1, NI) < m.view(C, 1)).to(F64)
    return from_per_channel(xv, shape)


def z_err_bound(x, r, b, res):
    """absolute fp32 evaluation error allowed on f = fma(x, scale, shift)
    [+ res].  With the sums exact: mean is within 4u (see dx_bound), ivar
    within 1e-6 relative (the 5e-6 statistics bound's derivation: 13u*E[x^2]
    + u*var on var, E[x^2]/var <= 2, halved by the square root, plus rsqrtf),
    scale = fl(w*ivar) within 1e-6 + u, shift = fl(b - fl(mean*scale)) errs by
    |mean*scale|(1e-6 + 6u) + u|shift|, the fma by |x*scale|(1e-6 + u) + u|f|,
    the residual add by u|f|.  Every term is below (1e-6 + 9u) = 1.54e-6
    times M = (|x| + |mean|)|scale| + |b| + |res|; the bound is 4e-6*M
    (2.6x slack)."""
    M = (x.abs() + vc(r['mean']).abs()) * vc(r['scale']).abs()
    if b is not None:
        M = M + vc(b).abs()
    if res is not None:
        M = M + res.abs()
    return 4e-6 * M


def _fwd_finish(case, x, flags, g, mom):
    """parameters, residual, reference and preconditions for integer x"""
    relu, has_res, affine, track = flags
    _l, dt, C, N, H, W = case
    NI = N * H * W
    pre = ref_fwd(x, None, None, None, False, EPS, mom, None, None)
    assert x.abs().sum((0, 2, 3)).max().item() < EXACT
    assert pre['q'].max().item() < EXACT
    assert x.abs().max().item() <= 256                  # exact in bf16
    assert ((pre['q'] / NI) / pre['var']).max().item() <= 2.0
    w = b = res = rm0 = rv0 = None
    if affine:
        # the zero crossing of every channel lies half way between two
        # integers (shifted by -1, 0 or 1 per channel)
        w = (torch.rand(C, generator=g) + 0.5).double()
        j = ints(g, -1, 1, C)
        b = (w * pre['ivar'] * (pre['mean'] - (pre['mean'].floor() + 0.5)
                                + j)).float().double()
    f0 = ref_fwd(x, w, b, None, False, EPS, mom, None, None)['f']
    if has_res:
        # half the residuals push f away from zero, half cancel it down to
        # its fraction plus a non-zero integer: the ReLU decision flips
        # against f's sign there, never within 1/2 of zero
        away = f0.sign() * ints(g, 0, 3, N, C, H, W)
        d = pick(g, (-2.0, -1.0, 1.0, 2.0), x.numel()).view(x.shape)
        coin = torch.rand(x.shape, generator=g) < 0.5
        res = torch.where(coin, away, d - f0.round())
        assert res.abs().max().item() <= 256
    if track:
        rm0 = torch.where(pre['mean'] < 0, -0.25, 0.25).to(F64)
        rv0 = torch.full((C,), 1.5, dtype=F64)
    r = ref_fwd(x, w, b, res, relu, EPS, mom, rm0, rv0)
    f = r['f']
    E = z_err_bound(x, r, b, res)
    assert f.abs().min().item() >= 2.0 ** -9
    assert (E < f.abs()).all().item()           # the sign cannot flip
    assert (f < 0).any().item() and (f > 0).any().item()
    if dt == 'bf16':
        # RNE of a value within E <= ulp/2 of f lands within one ulp of f
        assert (E <= 0.5 * bf16_ulp(f)).all().item()
    if has_res and relu:
        assert ((f0 > 0) & (f < 0)).any().item()
        assert ((f0 < 0) & (f > 0)).any().item()
    if is_pow2(NI):
        assert fp32_exact(r['mean'])
        if track:
            assert fp32_exact(r['rm']) and fp32_exact(mom * r['mean'])
    return {'x': x, 'w': w, 'b': b, 'res': res, 'rm0': rm0, 'rv0': rv0,
            'mom': mom, 'eps': EPS, 'relu': relu}, r, E


def momentum_for(NI):
    """a power of two when the rows are, so running_mean is exact"""
    return 0.25 if is_pow2(NI) else 0.1


@functools.lru_cache(maxsize=None)
def fwd_case(case, flags):
    _l, dt, C, N, H, W = case
    NI = N * H * W
    g = gen('fwd', case, flags)
    x = _centered_x(g, (N, C, H, W), 2 if NI > 4096 else 4)
    return _fwd_finish(case, x, flags, g, momentum_for(NI))


@functools.lru_cache(maxsize=None)
def fwd_one_row_case(dt):
    """N*H*W = 1: the variance is 0, the unbiased divisor n - 1 is guarded,
    x - mean is exactly 0 and f = beta + res.  x in {-1, 0, 1} and
    |beta| in [2, 3] keep the rounding of mean*scale (scale ~ 316*gamma)
    below half a bf16 ulp of f."""
    C = 16
    g = gen('fwd1', dt)
    x = ints(g, -1, 1, 1, C, 1, 1)
    w = (torch.rand(C, generator=g) * 0.5 + 0.5).double()
    b = (pick(g, (-1.0, 1.0), C) * (2 + torch.rand(C, generator=g))
         ).float().double()
    res = vc(b.sign() * ints(g, 0, 3, C)).clone()
    rm0 = pick(g, (-0.25, 0.25), C)
    rv0 = torch.full((C,), 1.5, dtype=F64)
    r = ref_fwd(x, w, b, res, True, EPS, 0.25, rm0, rv0)
    assert (r['var'] == 0).all().item() and torch.equal(r['mean'],
                                                        x.view(C))
    assert torch.equal(r['rv'], 0.75 * rv0)
    E = z_err_bound(x, r, b, res)
    assert (E < r['f'].abs()).all().item()
    assert (r['f'] < 0).any().item() and (r['f'] > 0).any().item()
    assert (E <= 0.5 * bf16_ulp(r['f'])).all().item()
    return {'x': x, 'w': w, 'b': b, 'res': res, 'rm0': rm0, 'rv0': rv0,
            'mom': 0.25, 'eps': EPS, 'relu': True}, r, E


# --------------------------------------------------------------------------
# forward from hand-made partial rows
# --------------------------------------------------------------------------
PART_B = (1, 2, 63, 64, 65, 100, 1000)
PART_C = (16, 64, 128, 256)
PART_CASES = [(dt, C, B) for dt in ('bf16', 'fp32') for C in PART_C
              for B in PART_B]


def part_shape(dt, C, B):
    """1024 rows (exact mean) for even B, 105 for odd"""
    return ('cl', dt, C) + ((4, 16, 16) if B % 2 == 0 else (3, 5, 7))


def part_flags(dt, C, B):
    """rotate the flag combinations over the grid; the collapse cases
    (B > 64) of every C see at least one with and one without statistics"""
    k = PART_B.index(B) + PART_C.index(C) + (dt == 'fp32')
    return FWD_FLAGS[k % len(FWD_FLAGS)]


@functools.lru_cache(maxsize=None)
def part_case(dt, C, B):
    """(inputs, reference, E, part [B, C, 2]): the rows of x are dealt
    unevenly to the live partial rows; about half the partial rows (for
    B > 2) stay all zero"""
    case = part_shape(dt, C, B)
    _l, _d, _C, N, H, W = case
    NI = N * H * W
    g = gen('part', dt, C, B)
    x = _centered_x(g, (N, C, H, W), 4)
    i, r, E = _fwd_finish(case, x, part_flags(dt, C, B), g,
                          momentum_for(NI))
    live = torch.arange(B)
    if B > 2:
        live = torch.randperm(B, generator=g)[:(B + 1) // 2]
    # uneven deal: square a uniform variate so low slots get more rows
    slot = (torch.rand(NI, generator=g) ** 2 * len(live)).long()
    owner = live[slot.clamp_max(len(live) - 1)]
    rows = x.permute(0, 2, 3, 1).reshape(NI, C)
    part = torch.zeros(B, C, 2, dtype=F64)
    part[:, :, 0].index_add_(0, owner, rows)
    part[:, :, 1].index_add_(0, owner, rows.square())
    assert torch.equal(part[:, :, 0].sum(0), r['s'])
    assert torch.equal(part[:, :, 1].sum(0), r['q'])
    if B > 2:
        assert (part.abs().sum((1, 2)) == 0).any().item()
    if B > 1 and NI >= 2 * B:
        cnt = torch.bincount(owner, minlength=B)
        assert cnt.max().item() > 2 * cnt[cnt > 0].min().item()
    return i, r, E, part
