# -*- coding: utf-8 -*-
"""cnn_local_rounds (hip/cnnround.h) on the GPU against the float64 step loop
of tests/cnnround_cases.py: the three geometries with operands cut out of
NaN-filled buffers, bounded by the fp32 CPU loop's own error; both orders of
the conv weights, determinism, launcher argument checks and graph capture.

The packed round through ClientPack on the GPU is in
test_gpu_packed_cnnround.py (it builds an on-GPU Client, which changes
process-wide state; no test here does).

Measured on an MI355X: see profiles/packed_cnn_notes.md."""
import math

import pytest
import torch

import linround_cases as lc
import cnnround_cases as cc
import fedtorch_amd.ops as ops

pytestmark = pytest.mark.gpu

NAN = float('nan')
PAD = 96
KEYS = ('X', 'Y', 'idx', 'steps', 'lr', 'server', 'replicas', 'in_mom',
        'mom_init', 'snap')


def _cut(t, fill):
    """a contiguous GPU copy of t in the middle of a buffer filled with
    `fill`; returns (view, buffer)"""
    buf = torch.full((t.numel() + 2 * PAD,), fill, dtype=t.dtype,
                     device='cuda')
    buf[PAD:PAD + t.numel()] = t.reshape(-1).cuda()
    return buf[PAD:PAD + t.numel()].view(t.shape), buf


def _guards_intact(buf, fill):
    g = torch.cat([buf[:PAD], buf[-PAD:]]).cpu()
    if isinstance(fill, float) and math.isnan(fill):
        return bool(torch.isnan(g).all())
    return bool((g == fill).all())


def _kw(case, hp, wd_numel):
    return dict(layout=case['layout'], wd_numel=wd_numel,
                weight_decay=hp['wd'], momentum=hp['m'],
                dampening=hp['damp'], nesterov=hp['nesterov'])


def run_cut(case, lr, k_cut, hp, snap, wd_numel):
    """the HIP path with every operand cut out of a NaN-filled (float) or
    plausible-but-wrong (int) buffer, NaN in the rows of the offline client;
    asserts the guard zones afterwards"""
    M = case['X'].shape[0]
    fills = dict(X=NAN, Y=case['layout']['fc2'][2] - 1, idx=M - 1, steps=0,
                 lr=NAN, server=NAN, replicas=NAN, in_mom=NAN, mom_init=7,
                 snap=NAN)
    src = dict(case, lr=lr.clone(), snap=snap)
    off = [c for c, ns in enumerate(case['steps'].tolist()) if ns == 0]
    src['lr'][off] = NAN
    if src['in_mom'] is not None:
        src['in_mom'] = src['in_mom'].clone()
        src['in_mom'][off] = NAN
    v, bufs = {}, {}
    for k in KEYS:
        if src[k] is None:
            v[k] = None
        else:
            v[k], bufs[k] = _cut(src[k], fills[k])
    loss = ops.cnn_local_rounds(
        v['X'], v['Y'], v['idx'], v['steps'], v['lr'], v['server'],
        v['replicas'], v['in_mom'], v['mom_init'], v['snap'], k_cut,
        **_kw(case, hp, wd_numel))
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert _guards_intact(b, fills[k]), 'guard zone of %s written' % k
    for k in ('X', 'Y', 'idx', 'steps', 'lr', 'server'):   # inputs unchanged
        assert torch.equal(v[k].cpu().view(torch.int32),
                           src[k].view(torch.int32)), k
    assert loss.dtype == torch.float32 and loss.is_contiguous()
    assert loss.shape == case['idx'].shape[:2]
    return dict(replicas=v['replicas'], in_mom=v['in_mom'],
                mom_init=v['mom_init'], snap=v['snap'], loss=loss), off


def test_limits_match_the_extension():
    lim = ops.cnn_round_limits()
    assert list(ops._C.cnn_round_limits()) == [
        lim['B'], lim['K'], lim['Cin'], lim['S'], lim['C1'], lim['C2'],
        lim['H']]
    assert lim['B'] == ops.CNNROUND_MAXB == ops.MLPROUND_MAXB
    assert lim['K'] == ops.CNNROUND_MAXK == ops.MLPROUND_MAXK


# --------------------------------------------------------------------------
# numerics and guards
# --------------------------------------------------------------------------
def _assert_bounded(got, ref, e32, label, index=None, off=()):
    """`off`: the offline clients, whose in_mom rows run_cut filled with
    NaN"""
    pick = (lambda t: t) if index is None else (lambda t: t[:, index])
    if ref['in_mom'] is not None:
        ref = dict(ref, in_mom=ref['in_mom'].clone())
        ref['in_mom'][list(off)] = NAN
    for k in cc.OUTPUTS:
        if ref[k] is None:
            assert got[k] is None
            continue
        want = ref[k] if k == 'loss' else pick(ref[k])
        assert lc.same_nan_pattern(got[k], want), k
        e, tol = lc.err(got[k], want), lc.bound(e32[k], cc.scale_of(ref[k]))
        print('%s %s: err %.3e  e32 %.3e  err/e32 %.2f  err/tol %.3f'
              % (label, k, e, e32[k], e / e32[k] if e32[k] else 0.0, e / tol))
        assert e <= tol, (k, e, tol)


@pytest.mark.parametrize('geo', cc.SHAPES)
def test_against_float64_replay(geo):
    """bound: 8x the fp32 CPU replay's own error plus 16 fp32 ulps of the
    output's scale (lc.bound)"""
    case, lr, k_cut, hp, snap, wd_numel, ref, e32 = cc.case(geo)
    got, off = run_cut(case, lr, k_cut, hp, snap, wd_numel)
    assert torch.equal(got['mom_init'].cpu(), ref['mom_init'])
    _assert_bounded(got, ref, e32, str(geo), off=off)
    on = [c for c in range(len(case['steps'])) if c not in off]
    for c in off:                          # offline: nothing written
        assert torch.isnan(got['replicas'][c]).all()
        assert torch.isnan(got['snap'][c]).all()
        assert not got['loss'][c].any()
        if got['in_mom'] is not None:
            assert torch.isnan(got['in_mom'][c]).all()
    gap = cc.gap_mask(case['layout'], case['N'])
    for c in on:
        if got['in_mom'] is not None:      # pad gaps of in_mom stay
            assert torch.equal(got['in_mom'][c].cpu()[gap],
                               case['in_mom'][c][gap])
        assert torch.equal(got['replicas'][c].cpu()[gap],   # the server's
                           case['server'][gap])


def test_weight_orders_agree_with_each_others_reference():
    """the mid case (both conv weights nhwc) re-packed in [co][ci][kh][kw]
    order: each run within the bound of the other order's reference,
    element for element"""
    case, lr, k_cut, hp, snap, wd_numel, ref, e32 = cc.case(cc.MID)
    layout, index = cc.reorder_index(case['layout'], (0, 0))
    plain = dict(case, layout=layout, server=case['server'][index],
                 in_mom=case['in_mom'][:, index])
    got_p, off = run_cut(plain, lr, k_cut, hp, snap, wd_numel)
    _assert_bounded(got_p, ref, e32, 'plain vs nhwc reference', index, off)
    ref_p = cc.run_ref(plain, lr, k_cut, hp, snap, wd_numel)
    back = torch.empty_like(index)
    back[index] = torch.arange(len(index))
    got_n, off = run_cut(case, lr, k_cut, hp, snap, wd_numel)
    _assert_bounded(got_n, ref_p, e32, 'nhwc vs plain reference', back, off)


def test_empty_step_stays_finite_and_in_bounds():
    """no valid row in an executed step (the twin refuses it; the launcher
    cannot see a device idx during capture): everything finite, guards
    intact"""
    case, lr, k_cut, hp, snap, wd_numel, _ref, _e = cc.case(cc.MID)
    case = dict(case, idx=case['idx'].clone())
    case['idx'][0, 1, :] = -1
    got, _off = run_cut(case, lr, k_cut, hp, snap, wd_numel)
    for c in (0, 2):
        assert torch.isfinite(got['replicas'][c]).all()
        assert torch.isfinite(got['in_mom'][c]).all()
    assert torch.isfinite(got['loss']).all() and got['loss'][0, 1] == 0


# --------------------------------------------------------------------------
# behaviour
# --------------------------------------------------------------------------
def _same(a, b):
    for k in ('replicas', 'in_mom', 'snap', 'loss', 'mom_init'):
        x, y = a[k].cpu(), b[k].cpu()
        assert torch.equal(torch.isnan(x), torch.isnan(y)), k
        assert torch.equal(x[~torch.isnan(x)], y[~torch.isnan(y)]), k


def test_two_runs_bit_identical():
    case, lr, k_cut, hp, snap, wd_numel, _ref, _e = cc.case(cc.STOCK)
    a = cc.call_op(ops, case, lr, k_cut, hp, snap, wd_numel, device='cuda')
    b = cc.call_op(ops, case, lr, k_cut, hp, snap, wd_numel, device='cuda')
    _same(a, b)


def _args(case, lr, k_cut, hp, snap, wd_numel):
    d = lambda t: t.clone().cuda()  # noqa: E731
    pos = [d(case['X']), d(case['Y']), d(case['idx']), d(case['steps']),
           d(lr), d(case['server']), d(case['replicas']), d(case['in_mom']),
           d(case['mom_init']), d(snap), k_cut]
    kw = _kw(case, hp, wd_numel)
    kw['layout'] = dict(kw['layout'])
    return pos, kw


def test_argument_checks_raise_before_launch():
    case, lr, k_cut, hp, snap, wd_numel, _r, _e = cc.case(cc.MID)
    X, Y, IDX, STEPS, LR, SRV, REP, MOM, MI, SNAP, KCUT = range(11)

    def bad(mutate, match):
        pos, kw = _args(case, lr, k_cut, hp, snap, wd_numel)
        mutate(pos, kw)
        before = [None if t is None or not torch.is_tensor(t) else t.clone()
                  for t in pos]
        with pytest.raises((RuntimeError, ValueError), match=match):
            ops.cnn_local_rounds(*pos, **kw)
        torch.cuda.synchronize()
        for t, b in zip(pos, before):      # nothing was written
            if b is not None:
                assert torch.equal(torch.isnan(t), torch.isnan(b))
                assert torch.equal(t[~torch.isnan(t)], b[~torch.isnan(b)])

    def setp(i, fn):
        return lambda pos, kw: pos.__setitem__(i, fn(pos[i]))

    bad(setp(X, lambda t: t.double()), 'X must be fp32')
    bad(setp(Y, lambda t: t.long()), 'Y must be')
    bad(setp(IDX, lambda t: t.long()), 'idx must be')
    bad(setp(LR, lambda t: t.half()), 'lr must be')
    bad(setp(REP, lambda t: t.double()), 'replicas must be')
    bad(setp(MI, lambda t: t.bool()), 'mom_init must be')
    bad(setp(X, lambda t: t.t().contiguous().t()), 'contiguous')
    bad(setp(REP, lambda t: t[:, :-1]), 'replicas must be contiguous')
    bad(setp(SRV, lambda t: t.cpu()), 'GPU')
    bad(setp(MOM, lambda t: t[:-1].contiguous()), 'in_mom must be')
    bad(setp(SNAP, lambda t: t[:, :-64].contiguous()), 'snap must be')
    bad(setp(STEPS, lambda t: t + 9), 'steps holds')
    bad(setp(KCUT, lambda k: -1), 'k_cut')
    bad(setp(IDX, lambda t: t[:, :, :0].contiguous()), 'unsupported B=0')
    bad(setp(IDX, lambda t: torch.cat([t] * 16, 2).contiguous()),
        'unsupported B=80')

    def oob(pos, kw):
        pos[IDX][0, 0, 0] = case['X'].shape[0]
    bad(oob, 'idx holds row')

    def lay(key, i, v):
        def mutate(pos, kw):
            t = list(kw['layout'][key])
            t[i] = v
            kw['layout'][key] = tuple(t)
        return mutate
    bad(lay('conv1', 1, 64), 'overlap')
    bad(lay('fc2', 0, 10 ** 6), 'does not fit')
    bad(lay('conv2', 0, -1), 'does not fit')
    bad(lay('image', 0, 2), 'X has 1200 features')
    bad(lay('image', 1, 18), 'does not pool evenly')
    bad(lay('image', 1, 12), 'does not pool evenly')
    bad(lay('image', 1, 36), 'unsupported image')
    bad(lay('image', 0, 5), 'unsupported image')
    bad(lay('conv1', 2, 25), 'unsupported C1=25')
    bad(lay('conv2', 2, 65), 'C2=65')
    bad(lay('fc1', 2, 4097), 'H=4097')
    bad(lay('fc2', 2, 129), 'unsupported K=129')
    bad(lay('conv2', 3, 2), 'nhwc flag')
    bad(lambda pos, kw: kw['layout'].__setitem__(
        'fc1', kw['layout']['fc1'][:2]), 'a layout is')
    bad(lambda pos, kw: kw.__setitem__('wd_numel', case['N'] + 1), 'wd_numel')
    bad(lambda pos, kw: kw.__setitem__('dampening', 0.5), 'nesterov')


def test_graph_capture_replays():
    case, lr, k_cut, hp, snap, wd_numel, _r, _e = cc.case(cc.MID)
    want = cc.call_op(ops, case, lr, k_cut, hp, snap, wd_numel,
                      device='cuda')
    pos, kw = _args(case, lr, k_cut, hp, snap, wd_numel)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss = ops.cnn_local_rounds(*pos, **kw)
    # put the in/out operands back and replay
    pos[6].copy_(case['replicas'])
    pos[7].copy_(case['in_mom'])
    pos[8].copy_(case['mom_init'])
    pos[9].copy_(snap)
    g.replay()
    torch.cuda.synchronize()
    _same(dict(replicas=pos[6], in_mom=pos[7], mom_init=pos[8], snap=pos[9],
               loss=loss), want)
