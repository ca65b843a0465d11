# -*- coding: utf-8 -*-
"""Case generators and the step-loop reference for the GRU sequence kernels
(hip/gru.h), shared by tests/test_gpu_gru.py (GPU) and tests/test_gru_cpu.py
(no GPU).  Imports torch only.

Reference (PyTorch gate order r, z, n; w_hh [3H, H]; gx = x W_ih^T + b_ih):

  forward, per step   gh = h W_hh^T + b_hh
                      r = sigmoid(gx_r + gh_r)     z = sigmoid(gx_z + gh_z)
                      q = gh_n                     n = tanh(gx_n + r q)
                      h' = (1 - z) n + z h
                      out[:, t] = h',  gates[:, t] = (r, z, n, q)
  backward, t = T-1 .. 0
                      dh   = dout[:, t] + dh_next
                      da_n = dh (1 - z) (1 - n^2)
                      da_z = dh (h_prev - n) z (1 - z)
                      da_r = da_n q r (1 - r)
                      dgx[:, t] = (da_r, da_z, da_n)
                      dgh[:, t] = (da_r, da_z, da_n r)
                      dh_next = dh z + dgh[:, t] W_hh
                      dw_hh = sum_t dgh[:, t]^T h_prev,  db_hh = sum dgh

``ref_fwd`` / ``ref_bwd`` run it in the dtype they are given: float64 is THE
reference, float32 (torch on the CPU) gives ``e32``, the error of the same
loop in the kernels' own precision.

Tolerance of the random cases, per tensor:

    |kernel - ref64| <= 4 e32 + 16 ulp32(max |ref64|),  e32 = max |ref32 - ref64|

The factor covers a different summation order and the device's exp / tanh
against libm; the ulp floor covers tensors where e32 is a single rounding.

Exact cases use small integers and dyadic fractions such that every sum the
kernels can form, in ANY order, is an fp32 number: ``order_free_exact`` checks
sum |terms| / unit < 2^24 with unit the common power-of-two granule of the
terms.  tests/test_gru_cpu.py proves these preconditions without a GPU."""
import math
import zlib

import torch

F64 = torch.float64
F32 = torch.float32
DTYPES = {'bf16': torch.bfloat16, 'fp32': torch.float32}

# exact forward (operand maps): T = 1
MAP_H = [1, 4, 16, 17, 50, 64]
MAP_B = [1, 3, 16, 17, 33]
# exact time indexing: (B, H) and T
TIME_BH = [(17, 50), (1, 1), (3, 17)]
TIME_T = [1, 2, 7]
# exact backward: (B, H) and T
BWD_BH = [(3, 17), (17, 50), (33, 64), (1, 1), (16, 16)]
BWD_T = [1, 2]
# padding: (B, T, H)
PAD_SHAPES = [(3, 2, 50), (17, 3, 17)]
# random companions: (B, T, H)
RANDOM = [(10, 50, 50), (33, 7, 64), (1, 1, 1), (17, 2, 17)]


def gen(*key):
    """CPU generator seeded by the case's name (stable across runs)"""
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def ints(g, lo, hi, *shape):
    """float64 tensor of uniform integers in [lo, hi]"""
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


# --------------------------------------------------------------------------
# reference
# --------------------------------------------------------------------------
def ref_fwd(gx, w_hh, b_hh, h0, dtype=F64):
    """-> out [B, T, H], gates [B, T, 4, H] = (r, z, n, q), in ``dtype``"""
    gx, w, b, h = (t.to(dtype) for t in (gx, w_hh, b_hh, h0))
    H = h.size(1)
    outs, gates = [], []
    for t in range(gx.size(1)):
        gh = h @ w.t() + b
        r = torch.sigmoid(gx[:, t, :H] + gh[:, :H])
        z = torch.sigmoid(gx[:, t, H:2 * H] + gh[:, H:2 * H])
        q = gh[:, 2 * H:]
        n = torch.tanh(gx[:, t, 2 * H:] + r * q)
        h = (1 - z) * n + z * h
        outs.append(h)
        gates.append(torch.stack((r, z, n, q), dim=1))
    return torch.stack(outs, dim=1), torch.stack(gates, dim=1)


def ref_bwd(dout, out, gates, w_hh, h0, dtype=F64, trace=None):
    """-> dict(dgx, dgh, dh0, dw, db) in ``dtype``.  ``trace``, a list,
    receives (name, terms, result) of every sum of more than two terms and
    (name, None, value) of every other intermediate."""
    dout, out, gates, w, h0 = (t.to(dtype)
                               for t in (dout, out, gates, w_hh, h0))
    B, T, H = out.shape
    dhn = torch.zeros(B, H, dtype=dtype)
    dgx, dgh = [None] * T, [None] * T

    def note(name, value, terms=None):
        if trace is not None:
            trace.append((name, terms, value))
        return value

    for t in range(T - 1, -1, -1):
        r, z, n, q = gates[:, t].unbind(1)
        hp = out[:, t - 1] if t > 0 else h0
        dh = note('dh', dout[:, t] + dhn)
        dn = note('dn', dh * (1 - z))
        dz = note('dz', dh * (hp - n))
        dan = note('da_n', dn * note('1-n^2', 1 - n * n))
        daz = note('da_z', dz * note('z(1-z)', z * (1 - z)))
        dar = note('da_r', note('da_n q', dan * q) *
                   note('r(1-r)', r * (1 - r)))
        dhr = note('da_n r', dan * r)
        dhz = note('dh z', dh * z)
        dgx[t] = torch.cat((dar, daz, dan), dim=1)
        dgh[t] = torch.cat((dar, daz, dhr), dim=1)
        # [B, 3H, H] products, then the sum over 3H plus dh z
        terms = torch.cat((dgh[t].unsqueeze(2) * w.unsqueeze(0),
                           dhz.unsqueeze(1)), dim=1)
        dhn = note('dh_next', dhz + dgh[t] @ w, terms)
    dgx, dgh = torch.stack(dgx, dim=1), torch.stack(dgh, dim=1)
    h_prev = torch.cat((h0.unsqueeze(1), out[:, :-1]), dim=1)
    return dict(dgx=dgx, dgh=dgh, dh0=dhn,
                dw=dgh.reshape(-1, 3 * H).t() @ h_prev.reshape(-1, H),
                db=dgh.sum((0, 1)))


# --------------------------------------------------------------------------
# exactness helpers
# --------------------------------------------------------------------------
def fp32_exact(t):
    """every element of the float64 tensor is an fp32 number"""
    return bool(torch.equal(t.to(F32).to(F64), t))


def dyadic_unit(t):
    """largest 2^-k (k in 0..60) of which every element is a multiple"""
    for k in range(61):
        s = t * 2.0 ** k
        if bool(torch.equal(s, s.round())):
            return 2.0 ** -k
    raise AssertionError('not dyadic')


def order_free_exact(terms, dim):
    """the sum of ``terms`` over ``dim`` is exact in fp32 in any order (and
    with or without fma): all partial sums are multiples of the terms' unit
    and bounded by sum |terms| < 2^24 units"""
    unit = dyadic_unit(terms)
    return bool((terms.abs().sum(dim) / unit < 2.0 ** 24).all())


def ulp32(x):
    """fp32 unit in the last place at magnitude x (a float)"""
    if x == 0.0:
        return 0.0
    return 2.0 ** (max(math.floor(math.log2(x)), -126) - 23)


def tolerance(ref64, ref32):
    """(tol, e32) of one tensor: tol = 4 e32 + 16 ulp32(max |ref64|)"""
    e32 = (ref32.to(F64) - ref64).abs().max().item()
    return 4.0 * e32 + 16.0 * ulp32(ref64.abs().max().item()), e32


# --------------------------------------------------------------------------
# exact cases
# --------------------------------------------------------------------------
def map_case(B, H):
    """T = 1, integer h0 in [-4, 4], asymmetric integer w_hh in [-3, 3],
    integer b_hh in [-4, 4]; gx ~ N(0, 1).  q = h0 W_hn^T + b_hn is an
    integer below 2^10.  -> gx, w, b, h0, out, gates (float64)"""
    g = gen('map', B, H)
    w = ints(g, -3, 3, 3 * H, H)
    if H > 1:
        # every gate block differs from its transpose
        for k in range(3):
            blk = w[k * H:(k + 1) * H]
            if bool(torch.equal(blk, blk.t())):
                blk[0, 1] = blk[1, 0] + 1 if blk[1, 0] < 3 else 2
    b = ints(g, -4, 4, 3 * H)
    h0 = ints(g, -4, 4, B, H)
    gx = torch.randn(B, 1, 3 * H, generator=g).to(F32).to(F64)
    out, gates = ref_fwd(gx, w, b, h0)
    return gx, w, b, h0, out, gates


def time_case(B, T, H):
    """w_hh = b_hh = gx = 0 and integer h0 in [-8, 8]: r = z = 1/2, n = 0,
    so out[:, t] = h0 2^-(t+1) exactly.  -> gx, w, b, h0, out (float64)"""
    g = gen('time', B, T, H)
    h0 = ints(g, -8, 8, B, H)
    out = torch.stack([h0 * 2.0 ** -(t + 1) for t in range(T)], dim=1)
    return (torch.zeros(B, T, 3 * H, dtype=F64),
            torch.zeros(3 * H, H, dtype=F64), torch.zeros(3 * H, dtype=F64),
            h0, out)


def bwd_case(B, T, H, trace=None):
    """hand-made gates r = z = n = 1/2, integer q in [-1, 1], integer h0 and
    out in [-2, 2], dout = k/8 with |k| <= 4, integer w_hh in [-1, 1].
    -> dout, out, gates, w, h0, dict(dgx, dgh, dh0, dw, db) (float64)"""
    g = gen('bwd', B, T, H)
    gates = torch.full((B, T, 4, H), 0.5, dtype=F64)
    gates[:, :, 3] = ints(g, -1, 1, B, T, H)
    h0 = ints(g, -2, 2, B, H)
    out = ints(g, -2, 2, B, T, H)
    dout = ints(g, -4, 4, B, T, H) / 8.0
    w = ints(g, -1, 1, 3 * H, H)
    if H > 1 and bool(torch.equal(w[:H], w[:H].t())):
        w[0, 1] = -w[1, 0] if w[1, 0] != 0 else 1.0
    return dout, out, gates, w, h0, ref_bwd(dout, out, gates, w, h0,
                                            trace=trace)


def nan_framed(t, dtype=None):
    """a contiguous copy of ``t`` cut out of the middle of a larger
    NaN-filled buffer (one extra slice on each side of dim 0)"""
    t = t if dtype is None else t.to(dtype)
    big = torch.full((t.size(0) + 2,) + tuple(t.shape[1:]), float('nan'),
                     dtype=t.dtype, device=t.device)
    big[1:-1] = t
    view = big[1:-1]
    assert view.is_contiguous()
    return view


# --------------------------------------------------------------------------
# random cases
# --------------------------------------------------------------------------
_RANDOM_CACHE = {}


def random_case(B, T, H):
    """weights U(+-1/sqrt(H)), gx ~ N(0, 1), h0 U(+-1), dout ~ N(0, 1), all
    fp32 values.  -> dict with the inputs (float64 copies of fp32 numbers),
    ``ref`` (float64 results) and ``tol`` / ``e32`` per tensor name.  Built
    once per shape; callers must not modify it."""
    key = (B, T, H)
    if key in _RANDOM_CACHE:
        return _RANDOM_CACHE[key]
    g = gen('random', B, T, H)
    k = 1.0 / math.sqrt(H)

    def uni(*shape):
        return ((torch.rand(*shape, generator=g) * 2 - 1) * k).to(F32)

    w, b = uni(3 * H, H).to(F64), uni(3 * H).to(F64)
    gx = torch.randn(B, T, 3 * H, generator=g).to(F32).to(F64)
    h0 = (torch.rand(B, H, generator=g) * 2 - 1).to(F32).to(F64)
    dout = torch.randn(B, T, H, generator=g).to(F32).to(F64)
    res = {}
    for dt in (F64, F32):
        out, gates = ref_fwd(gx, w, b, h0, dt)
        r = ref_bwd(dout, out, gates, w, h0, dt)
        r.update(out=out, gates=gates)
        res[dt] = r
    tol, e32 = {}, {}
    for name, ref64 in res[F64].items():
        tol[name], e32[name] = tolerance(ref64, res[F32][name])
    case = dict(gx=gx, w=w, b=b, h0=h0, dout=dout, ref=res[F64], tol=tol,
                e32=e32)
    _RANDOM_CACHE[key] = case
    return case
