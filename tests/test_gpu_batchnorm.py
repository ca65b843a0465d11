# -*- coding: utf-8 -*-
"""BatchNorm training kernels (hip/batchnorm.h) on their `ops._C` entry
points -- bn_bwd, bn_fwd_train, bn_fwd_train_part, bn_bwd_defer -- against
the float64 reference of tests/bn_cases.py (plain BatchNorm from its
formulas, checked against torch autograd in tests/test_bn_reference_cpu.py).

Backward: the caller supplies save_mean / save_ivar, so with integer x, dy,
y and save_mean and power-of-two save_ivar and weight every sum is exact in
fp32 in any order: dbias, dweight and dres are torch.equal at every shape,
dx too when the rows are a power of two (each intermediate asserted to be an
fp32 number), within a derived bound otherwise (bn_cases.dx_bound).  The
ReLU mask is taken from the saved output and, for bf16 channels_last, from a
bitmask the test packs itself, with identical results.

Forward: integer x keeps the sums exact; what remains is a handful of fp32
roundings -- statistics at rtol 5e-6, the output within one bf16 ulp (bf16)
or bn_cases.z_err_bound (fp32), zero crossings kept away from every input.

Outputs are allocated by the launchers, so instead of a NaN prefill every
output is checked for isfinite and compared in full."""
import os
import subprocess
import sys

import pytest
import torch

import fedtorch_amd.ops as ops

import bn_cases as bc

pytestmark = pytest.mark.gpu

DEV = 'cuda'
CL = torch.channels_last
F64 = torch.float64


def _act(t, case):
    """activation-shaped float64 -> the case's dtype and layout on the GPU"""
    if t is None:
        return _empty()
    t = t.to(bc.DTYPES[case[1]]).to(DEV)
    return t.contiguous(memory_format=CL) if case[0] == 'cl' else t


def _f32(t):
    return _empty() if t is None else t.float().to(DEV)


def _empty(dtype=torch.float32):
    return torch.empty(0, device=DEV, dtype=dtype)


def _first_diff(got, want):
    bad = ((got != want) | (got != got)).nonzero()
    if bad.numel() == 0:
        return 'no mismatch'
    i = tuple(bad[0].tolist())
    return 'first mismatch at %s: got %s want %s (%d differ)' % (
        i, got[i].item(), want[i].item(), bad.shape[0])


def _assert_exact(got, want64, where):
    """got must be finite and equal RNE(want64) bit for bit"""
    got = got.cpu()
    want = want64.float().to(got.dtype)
    assert got.shape == want.shape, '%s shape %s' % (where, tuple(got.shape))
    assert torch.isfinite(got).all().item(), '%s not finite' % where
    assert torch.equal(got, want), '%s %s' % (where, _first_diff(got, want))


def _assert_within(got, want64, bound, where):
    """|got - want64| <= bound elementwise; prints the largest error as a
    fraction of its bound"""
    got = got.double().cpu()
    assert got.shape == want64.shape, '%s shape' % where
    assert torch.isfinite(got).all().item(), '%s not finite' % where
    err = (got - want64).abs()
    frac = torch.where(err == 0, torch.zeros_like(err),
                       err / bound.clamp_min(1e-300)).max().item()
    print('%s max err %.3g = %.3f of its bound' % (
        where, err.max().item(), frac))
    assert (err <= bound).all().item(), \
        '%s off by %.3g x bound' % (where, frac)


def _assert_rel(got, want64, where, rtol=5e-6):
    got = got.double().cpu()
    assert got.shape == want64.shape, '%s shape' % where
    assert torch.isfinite(got).all().item(), '%s not finite' % where
    err = ((got - want64).abs() / want64.abs().clamp_min(1e-300))
    err = torch.where(got == want64, torch.zeros_like(err), err).max()
    print('%s max rel err %.3g (bound %.1g)' % (where, err.item(), rtol))
    assert torch.allclose(got, want64, rtol=rtol, atol=0), \
        '%s rel err %.3g' % (where, err.item())


def _same(a, b, where):
    for k, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u.cpu(), v.cpu()), '%s output %d: %s' % (
            where, k, _first_diff(u.cpu(), v.cpu()))


# --------------------------------------------------------------------------
# backward
# --------------------------------------------------------------------------
def _run_bwd(case, i, relu, has_res, affine=True, mask=None):
    y = _act(i['y'], case) if relu and mask is None else _empty()
    return ops._C.bn_bwd(
        _act(i['dy'], case), _act(i['x'], case), y,
        mask if mask is not None else _empty(torch.uint8),
        _f32(i['mean']), _f32(i['ivar']), _f32(i['w'] if affine else None),
        relu, has_res)


def _check_bwd(out, case, r, exact, has_res, where):
    dx, dweight, dbias, dres = out
    _assert_exact(dbias, r['dbias'], where + ' dbias')
    _assert_exact(dweight, r['dweight'], where + ' dweight')
    if has_res:
        _assert_exact(dres, r['dres'], where + ' dres')
        assert dres.dtype == dx.dtype and dres.stride() == dx.stride()
    else:
        assert dres.numel() == 0
    assert dx.dtype == bc.DTYPES[case[1]]
    if exact:
        _assert_exact(dx, r['dx'], where + ' dx')
    else:
        _assert_within(dx, r['dx'], bc.dx_bound(r, case[1]), where + ' dx')


BWD_PARAMS = [(c, f) for c in bc.SHAPES for f in bc.BWD_FLAGS] + \
    [(c, (True, True)) for c in bc.LARGE]


@pytest.mark.parametrize(
    'case,flags', BWD_PARAMS,
    ids=['%s-relu%d-res%d' % (bc.case_id(c), f[0], f[1])
         for c, f in BWD_PARAMS])
def test_bn_bwd(case, flags):
    """dbias / dweight / dres exact everywhere, dx exact for power-of-two
    rows and within bn_cases.dx_bound (6u derived, 8u asserted, plus half a
    bf16 ulp) otherwise; the mask path must reproduce the y path bit for
    bit with an empty y."""
    relu, has_res = flags
    i, r, exact = bc.bwd_case(case, relu, True)
    where = 'bn_bwd %s relu%d res%d' % (bc.case_id(case), relu, has_res)
    out = _run_bwd(case, i, relu, has_res)
    _check_bwd(out, case, r, exact, has_res, where)
    if relu and bc.mask_ok(case):
        mask = bc.pack_mask(i['y']).to(DEV)
        assert mask.numel() * 8 == i['y'].numel()
        out_m = _run_bwd(case, i, relu, has_res, mask=mask)
        _check_bwd(out_m, case, r, exact, has_res, where + ' (mask)')
        _same(out, out_m, where + ' y vs mask')


@pytest.mark.parametrize('case', [
    ('cl', 'bf16', 32, 3, 5, 7), ('cl', 'fp32', 16, 4, 16, 16),
    ('nchw', 'bf16', 3, 2, 8, 8), ('nchw', 'fp32', 5, 3, 7, 7)],
    ids=bc.case_id)
def test_bn_bwd_no_weight(case):
    """an empty weight means gamma = 1"""
    i, r, exact = bc.bwd_case(case, True, False)
    where = 'bn_bwd no-weight %s' % bc.case_id(case)
    _check_bwd(_run_bwd(case, i, True, True, affine=False), case, r, exact,
               True, where)


# --------------------------------------------------------------------------
# forward
# --------------------------------------------------------------------------
def _fwd_args(case, i):
    rm, rv = _f32(i['rm0']), _f32(i['rv0'])
    return (_f32(i['w']), _f32(i['b']), rm, rv, i['eps'], i['mom'],
            i['relu'], _act(i['res'], case)), rm, rv


def _check_fwd(out, rm, rv, case, i, r, E, where):
    """y, save_mean, save_ivar, running stats against the reference"""
    y, sm, siv, mask = out
    NI = bc.rows_of(case)
    assert mask.numel() == 0, '%s: the mask is opt-in' % where
    assert y.dtype == bc.DTYPES[case[1]] and y.shape == i['x'].shape
    if case[0] == 'cl':
        assert y.is_contiguous(memory_format=CL)
    else:
        assert y.is_contiguous()
    if bc.is_pow2(NI):
        _assert_exact(sm, r['mean'], where + ' save_mean')
    else:
        _assert_rel(sm, r['mean'], where + ' save_mean')
    _assert_rel(siv, r['ivar'], where + ' save_ivar')
    if i['rm0'] is not None:
        if bc.is_pow2(NI) and bc.is_pow2(round(1 / i['mom'])):
            _assert_exact(rm, r['rm'], where + ' running_mean')
        else:
            _assert_rel(rm, r['rm'], where + ' running_mean')
        _assert_rel(rv, r['rv'], where + ' running_var')
    y64 = r['y']
    if case[1] == 'bf16':
        bound = bc.bf16_ulp(y64)            # 0 where the ReLU output is 0
    else:
        bound = torch.where(y64 == 0, torch.zeros_like(E), E)
    _assert_within(y, y64, bound, where + ' y')


FWD_PARAMS = [(c, f) for c in bc.FWD_SHAPES for f in bc.FWD_FLAGS] + \
    [(c, (True, True, True, True)) for c in bc.LARGE]


@pytest.mark.parametrize(
    'case,flags', FWD_PARAMS,
    ids=['%s-relu%d-res%d-aff%d-trk%d' % ((bc.case_id(c),) + f)
         for c, f in FWD_PARAMS])
def test_bn_fwd_train(case, flags):
    """statistics at rtol 5e-6 (sums exact, E[x^2]/var <= 2 asserted; the
    derivation is test_bn_finalize_from_partials's), save_mean and
    running_mean torch.equal for power-of-two rows and momentum; y within
    one bf16 ulp (bf16: the fp32 error bound bn_cases.z_err_bound is
    asserted to stay below half an ulp of every output) or within that bound
    itself (fp32); outputs the ReLU clamps are exactly 0."""
    i, r, E = bc.fwd_case(case, flags)
    where = 'bn_fwd_train %s %s' % (bc.case_id(case), flags)
    args, rm, rv = _fwd_args(case, i)
    out = ops._C.bn_fwd_train(_act(i['x'], case), *args)
    _check_fwd(out, rm, rv, case, i, r, E, where)


@pytest.mark.parametrize('dt', ('bf16', 'fp32'))
def test_bn_fwd_train_one_row(dt):
    """N*H*W = 1: variance 0, ivar = 1/sqrt(eps), the unbiased divisor is
    guarded (running_var only decays), y = relu(beta + res)"""
    case = ('cl', dt, 16, 1, 1, 1)
    i, r, E = bc.fwd_one_row_case(dt)
    args, rm, rv = _fwd_args(case, i)
    out = ops._C.bn_fwd_train(_act(i['x'], case), *args)
    _check_fwd(out, rm, rv, case, i, r, E, 'bn_fwd_train one row ' + dt)
    _assert_exact(rv, r['rv'], 'one row running_var')


@pytest.mark.parametrize('dt,C,B', bc.PART_CASES,
                         ids=['%s-C%d-B%d' % p for p in bc.PART_CASES])
def test_bn_fwd_train_part(dt, C, B):
    """statistics finalized from hand-made integer partial rows (uneven, some
    all zero), on both sides of the 64-row switch to part_reduce_k and for
    C up to 256 (2*C = 512 columns > 256 threads).  Same bounds as
    test_bn_fwd_train."""
    i, r, E, part = bc.part_case(dt, C, B)
    case = bc.part_shape(dt, C, B)
    where = 'bn_fwd_train_part %s C%d B%d %s' % (dt, C, B,
                                                  bc.part_flags(dt, C, B))
    args, rm, rv = _fwd_args(case, i)
    pd = part.float().to(DEV)
    keep = pd.clone()
    out = ops._C.bn_fwd_train_part(_act(i['x'], case), pd, *args)
    _check_fwd(out, rm, rv, case, i, r, E, where)
    assert torch.equal(pd, keep), '%s: the partials were modified' % where


# --------------------------------------------------------------------------
# deferred backward
# --------------------------------------------------------------------------
def _run_defer(case, i, relu, has_res):
    return ops._C.bn_bwd_defer(
        _act(i['dy'], case), _act(i['x'], case),
        _act(i['y'], case) if relu else _empty(),
        _f32(i['mean']), _f32(i['ivar']), _f32(i['w']), relu, has_res)


DEFER_PARAMS = [(c, f) for c in bc.DEFER_CASES for f in bc.DEFER_FLAGS]


@pytest.mark.parametrize(
    'case,flags', DEFER_PARAMS,
    ids=['%s-relu%d-res%d' % (bc.case_id(c), f[0], f[1])
         for c, f in DEFER_PARAMS])
def test_bn_bwd_defer(case, flags):
    """coefs [3, C] = (A, A*(mean*ivar*mdyxh - mdy), -A*ivar*mdyxh) with
    A = gamma*ivar: exact for power-of-two rows, within
    bn_cases.defer_case's bound (5u derived, 8u asserted) otherwise;
    dweight, dbias and dres exact.  Covers <= 64 and > 64 reduce blocks."""
    relu, has_res = flags
    i, r, coefs64, bound, exact = bc.defer_case(case, relu)
    where = 'bn_bwd_defer %s relu%d res%d' % (bc.case_id(case), relu,
                                              has_res)
    coefs, dweight, dbias, dres = _run_defer(case, i, relu, has_res)
    _assert_exact(dbias, r['dbias'], where + ' dbias')
    _assert_exact(dweight, r['dweight'], where + ' dweight')
    if has_res:
        _assert_exact(dres, r['dres'], where + ' dres')
    else:
        assert dres.numel() == 0
    assert coefs.shape == (3, case[2]) and coefs.dtype == torch.float32
    if exact:
        _assert_exact(coefs, coefs64, where + ' coefs')
    else:
        _assert_within(coefs, coefs64, bound, where + ' coefs')


def test_bn_bwd_defer_block_counts():
    """the cases sit on both sides of the 64-block collapse"""
    blocks = [bc.defer_blocks(c) for c in bc.DEFER_CASES]
    assert min(blocks) == 1 and sorted(blocks)[-2:] == [68, 128], blocks
    assert any(c[2] == 256 and b > 64
               for c, b in zip(bc.DEFER_CASES, blocks))


# --------------------------------------------------------------------------
# mask produced by the forward (FT_BNH_MASK=1 is read once per process)
# --------------------------------------------------------------------------
def test_bn_fwd_mask_child_process():
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                         'bn_mask_child.py')
    env = dict(os.environ)
    env['FT_BNH_MASK'] = '1'
    p = subprocess.run([sys.executable, child], env=env, timeout=300,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    print(p.stdout.decode(errors='replace'))
    assert p.returncode == 0, 'mask child exit status %d' % p.returncode


# --------------------------------------------------------------------------
# determinism (no atomics anywhere in batchnorm.h)
# --------------------------------------------------------------------------
@pytest.mark.parametrize('case', [
    ('cl', 'bf16', 64, 4, 16, 16), ('cl', 'fp32', 256, 1, 1, 5),
    ('nchw', 'bf16', 2, 33, 8, 8), ('nchw', 'fp32', 5, 3, 7, 7)],
    ids=bc.case_id)
def test_bn_deterministic(case):
    i, _r, _e = bc.bwd_case(case, True, True)
    where = 'deterministic %s' % bc.case_id(case)
    _same(_run_bwd(case, i, True, True), _run_bwd(case, i, True, True),
          where + ' bn_bwd')
    if bc.mask_ok(case):
        mask = bc.pack_mask(i['y']).to(DEV)
        _same(_run_bwd(case, i, True, True, mask=mask),
              _run_bwd(case, i, True, True, mask=mask),
              where + ' bn_bwd mask')
    fi, _fr, _fe = bc.fwd_case(case, (True, True, True, True))

    def fwd():
        args, rm, rv = _fwd_args(case, fi)
        return tuple(ops._C.bn_fwd_train(_act(fi['x'], case), *args)) + (
            rm, rv)

    _same(fwd(), fwd(), where + ' bn_fwd_train')


@pytest.mark.parametrize('dt,C,B', [('bf16', 64, 64), ('bf16', 256, 1000),
                                    ('fp32', 128, 65)])
def test_bn_fwd_train_part_deterministic(dt, C, B):
    i, _r, _e, part = bc.part_case(dt, C, B)
    case = bc.part_shape(dt, C, B)
    pd = part.float().to(DEV)

    def fwd():
        args, rm, rv = _fwd_args(case, i)
        return tuple(ops._C.bn_fwd_train_part(_act(i['x'], case), pd,
                                              *args)) + (rm, rv)

    _same(fwd(), fwd(), 'deterministic part %s C%d B%d' % (dt, C, B))


@pytest.mark.parametrize('case', [bc.DEFER_CASES[1], bc.DEFER_CASES[3]],
                         ids=bc.case_id)
def test_bn_bwd_defer_deterministic(case):
    i, _r, _c, _b, _e = bc.defer_case(case, True)
    _same(_run_defer(case, i, True, True), _run_defer(case, i, True, True),
          'deterministic defer %s' % bc.case_id(case))


# --------------------------------------------------------------------------
# argument checks: every call below is rejected before anything is launched,
# and no malformed tensor is smaller than the well-formed one it replaces
# --------------------------------------------------------------------------
def _rejects(who, fn, *args):
    with pytest.raises(RuntimeError, match=who):
        fn(*args)


def _nchw_like(t):
    out = torch.zeros(t.shape, dtype=t.dtype, device=t.device)
    assert out.is_contiguous() and not out.is_contiguous(memory_format=CL)
    return out


def _bigger(t):
    """one more image, same dtype and layout"""
    s = (t.shape[0] + 1,) + tuple(t.shape[1:])
    out = torch.zeros(s, dtype=t.dtype, device=t.device)
    return out.contiguous(memory_format=CL) \
        if t.is_contiguous(memory_format=CL) else out


REJ_CASE = ('cl', 'bf16', 16, 2, 4, 4)


def _rej_vectors(C):
    one = torch.ones(C, device=DEV)
    return one, one.double(), torch.ones(2 * C, device=DEV)


def test_bn_bwd_reject_bad_arguments():
    case = REJ_CASE
    C = case[2]
    i = bc.bwd_inputs(case)
    f = ops._C.bn_bwd
    who = 'bn_bwd'
    dy, x, y = _act(i['dy'], case), _act(i['x'], case), _act(i['y'], case)
    m, iv, w = _f32(i['mean']), _f32(i['ivar']), _f32(i['w'])
    _one, dbl, long_ = _rej_vectors(C)
    nomask = _empty(torch.uint8)
    mask = bc.pack_mask(i['y']).to(DEV)
    f(dy, x, y, nomask, m, iv, w, True, True)            # well-formed
    f(dy, x, _empty(), mask, m, iv, w, True, True)
    # dy: dtype, layout, shape
    _rejects(who, f, dy.float(), x, y, nomask, m, iv, w, True, True)
    _rejects(who, f, _nchw_like(dy), x, y, nomask, m, iv, w, True, True)
    _rejects(who, f, _bigger(dy), x, y, nomask, m, iv, w, True, True)
    # y: dtype, layout, shape, missing
    _rejects(who, f, dy, x, y.float(), nomask, m, iv, w, True, True)
    _rejects(who, f, dy, x, _nchw_like(y), nomask, m, iv, w, True, True)
    _rejects(who, f, dy, x, _bigger(y), nomask, m, iv, w, True, True)
    _rejects(who, f, dy, x, _empty(), nomask, m, iv, w, True, True)
    # save_mean / save_ivar / weight: dtype, length, missing statistics
    _rejects(who, f, dy, x, y, nomask, dbl, iv, w, True, True)
    _rejects(who, f, dy, x, y, nomask, long_, iv, w, True, True)
    _rejects(who, f, dy, x, y, nomask, _empty(), iv, w, True, True)
    _rejects(who, f, dy, x, y, nomask, m, dbl, w, True, True)
    _rejects(who, f, dy, x, y, nomask, m, long_, w, True, True)
    _rejects(who, f, dy, x, y, nomask, m, _empty(), w, True, True)
    _rejects(who, f, dy, x, y, nomask, m, iv, dbl, True, True)
    _rejects(who, f, dy, x, y, nomask, m, iv, long_, True, True)
    # mask: length, dtype, fp32 x (VN = 4), NCHW x
    _rejects(who, f, dy, x, _empty(), torch.cat((mask, mask)), m, iv, w,
             True, True)
    _rejects(who, f, dy, x, _empty(), mask.to(torch.int8), m, iv, w, True,
             True)
    _rejects(who, f, dy.float(), x.float(), _empty(), mask, m, iv, w, True,
             True)
    xn, dyn = _nchw_like(x), _nchw_like(dy)
    _rejects(who, f, dyn, xn, _empty(), mask, m, iv, w, True, True)
    # NCHW: relu without y used to reach the device with a null pointer
    f(dyn, xn, _nchw_like(y), nomask, m, iv, w, True, True)  # well-formed
    _rejects(who, f, dyn, xn, _empty(), nomask, m, iv, w, True, True)
    _rejects(who, f, dyn, xn, y, nomask, m, iv, w, True, True)   # y layout
    _rejects(who, f, dy, xn, _nchw_like(y), nomask, m, iv, w, True, True)
    # x: not 4-D, unsupported channel count for channels_last
    _rejects(who, f, dy, x.reshape(2, 16, 16), y, nomask, m, iv, w, True,
             True)
    x12 = torch.zeros(2, 12, 4, 4, dtype=torch.bfloat16,
                      device=DEV).contiguous(memory_format=CL)
    v12 = torch.ones(12, device=DEV)
    _rejects(who, f, x12, x12, x12, nomask, v12, v12, v12, True, True)
    torch.cuda.synchronize()


def _fwd_reject_common(who, call, case, i):
    """res / weight / bias / running statistics checks shared by the two
    forward launchers; call(x, w, b, rm, rv, res) runs the launcher"""
    C = case[2]
    x, res = _act(i['x'], case), _act(i['res'], case)
    one, dbl, long_ = _rej_vectors(C)
    e = _empty()
    call(x, one, one, one.clone(), one.clone(), res)     # well-formed
    call(x, e, e, e, e, e)
    # res: dtype, layout, shape
    _rejects(who, call, x, one, one, e, e, res.float())
    _rejects(who, call, x, one, one, e, e, _nchw_like(res))
    _rejects(who, call, x, one, one, e, e, _bigger(res))
    # parameter vectors: dtype, length
    for bad in (dbl, long_):
        _rejects(who, call, x, bad, one, e, e, e)
        _rejects(who, call, x, one, bad, e, e, e)
        _rejects(who, call, x, one, one, bad, one.clone(), e)
        _rejects(who, call, x, one, one, one.clone(), bad, e)
    # running statistics go together
    _rejects(who, call, x, one, one, one.clone(), e, e)
    _rejects(who, call, x, one, one, e, one.clone(), e)
    return x, one, e


def test_bn_fwd_train_reject_bad_arguments():
    case = REJ_CASE
    i, _r, _e = bc.fwd_case(case, (True, True, True, True))
    f = ops._C.bn_fwd_train
    who = 'bn_fwd_train'

    def call(x, w, b, rm, rv, res):
        return f(x, w, b, rm, rv, 1e-5, 0.1, True, res)

    x, one, e = _fwd_reject_common(who, call, case, i)
    # NCHW x wants an NCHW res
    xn = _nchw_like(x)
    call(xn, one, one, e, e, _nchw_like(x))              # well-formed
    _rejects(who, call, xn, one, one, e, e, x)
    _rejects(who, call, x.reshape(2, 16, 16), one, one, e, e, e)
    torch.cuda.synchronize()


def test_bn_fwd_train_part_reject_bad_arguments():
    case = REJ_CASE
    C = case[2]
    i, _r, _e = bc.fwd_case(case, (True, True, True, True))
    f = ops._C.bn_fwd_train_part
    who = 'bn_fwd_train_part'
    part = torch.zeros(3, C, 2, device=DEV)
    part[0, :, 0] = 1.0
    part[0, :, 1] = 64.0

    def call(x, w, b, rm, rv, res, part=part):
        return f(x, part, w, b, rm, rv, 1e-5, 0.1, True, res)

    x, one, e = _fwd_reject_common(who, call, case, i)
    # part: no rows, not contiguous, dtype, channel count, rank
    for bad in (torch.zeros(0, C, 2, device=DEV),
                torch.zeros(3, C, 4, device=DEV)[..., ::2],
                part.double(),
                torch.zeros(3, 2 * C, 2, device=DEV),
                torch.zeros(3, C * 2, device=DEV),
                torch.zeros(70, 2 * C, 2, device=DEV)):
        _rejects(who, call, x, one, one, e, e, e, bad)
    # (the N*HW < 2^31 check needs a >= 32 GiB activation: not exercised)
    # channels_last only; unsupported C is refused before part_reduce_k runs
    _rejects(who, call, _nchw_like(x), one, one, e, e, e)
    x12 = torch.zeros(2, 12, 4, 4, dtype=torch.bfloat16,
                      device=DEV).contiguous(memory_format=CL)
    v12 = torch.ones(12, device=DEV)
    _rejects(who, call, x12, v12, v12, e, e, e,
             torch.zeros(70, 12, 2, device=DEV))
    torch.cuda.synchronize()


def test_bn_bwd_defer_reject_bad_arguments():
    case = REJ_CASE
    C = case[2]
    i = bc.bwd_inputs(case)
    f = ops._C.bn_bwd_defer
    who = 'bn_bwd_defer'
    dz, x, z = _act(i['dy'], case), _act(i['x'], case), _act(i['y'], case)
    m, iv, w = _f32(i['mean']), _f32(i['ivar']), _f32(i['w'])
    _one, dbl, long_ = _rej_vectors(C)
    f(dz, x, z, m, iv, w, True, True)                    # well-formed
    f(dz, x, _empty(), m, iv, _empty(), False, False)
    # dz / z: dtype, layout, shape, missing
    _rejects(who, f, dz.float(), x, z, m, iv, w, True, True)
    _rejects(who, f, _nchw_like(dz), x, z, m, iv, w, True, True)
    _rejects(who, f, _bigger(dz), x, z, m, iv, w, True, True)
    _rejects(who, f, dz, x, z.float(), m, iv, w, True, True)
    _rejects(who, f, dz, x, _nchw_like(z), m, iv, w, True, True)
    _rejects(who, f, dz, x, _bigger(z), m, iv, w, True, True)
    _rejects(who, f, dz, x, _empty(), m, iv, w, True, False)
    # dres is the ReLU-masked dz: the mask needs z
    _rejects(who, f, dz, x, _empty(), m, iv, w, False, True)
    # x layout
    _rejects(who, f, _nchw_like(dz), _nchw_like(x), _nchw_like(z), m, iv, w,
             True, True)
    # vectors
    for bad in (dbl, long_):
        _rejects(who, f, dz, x, z, bad, iv, w, True, True)
        _rejects(who, f, dz, x, z, m, bad, w, True, True)
        _rejects(who, f, dz, x, z, m, iv, bad, True, True)
    _rejects(who, f, dz, x, z, _empty(), iv, w, True, True)
    _rejects(who, f, dz, x, z, m, _empty(), w, True, True)
    torch.cuda.synchronize()
