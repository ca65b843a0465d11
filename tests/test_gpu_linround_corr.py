# -*- coding: utf-8 -*-
"""The gradient-correction term of linear_local_rounds (hip/linearround.h) and
the two batched row kernels on the GPU: exact cases bit-equal to float64 with
every operand cut out of a NaN-filled buffer, random-valued companions
bounded by the fp32 CPU loop's own error, NaN in everything the kernel must
not read, determinism, launcher rejections, graph capture, and packed
SCAFFOLD / FedGATE federations through ClientPack with both flags on against
the slot loop.

Measured on an MI355X: see profiles/packed_linear_notes.md."""
import math
import os

import numpy as np
import pytest
import torch

import linround_cases as lc
import linround_corr_cases as cc
import fedtorch_amd.ops as ops
from fedtorch_amd.parallel import multiclient

pytestmark = pytest.mark.gpu

NAN = float('nan')
PAD = 96
KEYS = ('X', 'Y', 'idx', 'steps', 'lr', 'server', 'replicas', 'in_mom',
        'mom_init', 'snap', 'delta', 'ctrl_server', 'ctrl_client')
INPUTS = ('X', 'Y', 'idx', 'steps', 'lr', 'server', 'delta', 'ctrl_server',
          'ctrl_client')


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


def run_cut(case, lr, k_cut, hp, snap, corr):
    """the HIP path with every operand, the correction's included, cut out
    of a NaN-filled (float) or plausible-but-wrong (int) buffer; asserts the
    guard zones and that the inputs are unchanged"""
    M = case['X'].shape[0]
    fills = dict(X=NAN, Y=NAN if case['loss_kind'] else case['K'] - 1,
                 idx=M - 1, steps=0, lr=NAN, server=NAN, replicas=NAN,
                 in_mom=NAN, mom_init=7, snap=NAN, delta=NAN,
                 ctrl_server=NAN, ctrl_client=NAN)
    src = dict(case, lr=lr, snap=snap, delta=corr['delta'],
               ctrl_server=corr['ctrl_server'],
               ctrl_client=corr['ctrl_client'])
    v, bufs = {}, {}
    for k in KEYS:
        if src[k] is None:
            v[k] = None
        else:
            v[k], bufs[k] = _cut(src[k], fills[k])
    loss = ops.linear_local_rounds(
        v['X'], v['Y'], v['idx'], v['steps'], v['lr'], v['server'],
        v['replicas'], v['in_mom'], v['mom_init'], v['snap'], k_cut,
        w_off=case['w_off'], b_off=case['b_off'], K=case['K'],
        loss_kind=case['loss_kind'], weight_decay=hp['wd'],
        momentum=hp['m'], dampening=hp['damp'], nesterov=hp['nesterov'],
        delta=v['delta'], ctrl_server=v['ctrl_server'],
        ctrl_client=v['ctrl_client'], prox_mu=corr['prox_mu'])
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert _guards_intact(b, fills[k]), 'guard zone of %s written' % k
    for k in INPUTS:
        if src[k] is not None:
            assert torch.equal(v[k].cpu().view(torch.int32),
                               src[k].view(torch.int32)), k
    assert loss.dtype == torch.float32 and loss.is_contiguous()
    assert loss.shape == case['idx'].shape[:2]
    return dict(replicas=v['replicas'], in_mom=v['in_mom'],
                mom_init=v['mom_init'], snap=v['snap'], loss=loss)


def _assert_exact(got, ref, case):
    for k in ('replicas', 'in_mom', 'snap'):
        if ref[k] is None:
            continue
        # the NaN prefill survives in the rows of the offline client and in
        # snap rows that were not due, and nowhere else: the NaN of the
        # correction's pad gaps and offline rows was never read
        assert lc.same_nan_pattern(got[k], ref[k]), k
        assert lc.err(got[k], ref[k]) == 0.0, k
    assert torch.equal(got['mom_init'].cpu(), ref['mom_init'])
    for c, s in enumerate(case['steps'].tolist()):
        if s == 0:
            assert torch.isnan(got['replicas'][c]).all()
            assert not got['loss'][c].any()
            if got['in_mom'] is not None:
                assert torch.equal(got['in_mom'][c].cpu(), case['in_mom'][c])
        else:
            assert torch.isfinite(got['replicas'][c]).all()


# --------------------------------------------------------------------------
# exact cases
# --------------------------------------------------------------------------
@pytest.mark.parametrize('kind', cc.KINDS)
@pytest.mark.parametrize('F,B,tau,lr_exp,wd,m,mu', cc.EXACT_LS)
def test_exact_least_squares(kind, F, B, tau, lr_exp, wd, m, mu):
    case, lr, k_cut, hp, snap, corr, ref = cc.exact_case(
        kind, F, B, tau, lr_exp, wd, m, mu)
    assert case['steps'].tolist()[1] == 0
    if m:
        assert case['mom_init'].tolist() == [0, 1, 0]
    got = run_cut(case, lr, k_cut, hp, snap, corr)
    _assert_exact(got, ref, case)
    assert torch.equal(got['loss'].double().cpu(), ref['loss'])


@pytest.mark.parametrize('kind', cc.KINDS)
@pytest.mark.parametrize('F,B,lr_exp,m,mu', cc.EXACT_CE)
def test_exact_softmax_ce_from_zero(kind, F, B, lr_exp, m, mu):
    """zero weights: p = 1/2 exactly, so W, b and momentum are exact (the
    loss is checked by test_gpu_linround.py; the correction does not enter
    it in a single step)."""
    case, lr, k_cut, hp, snap, corr, ref = cc.exact_case(
        kind, F, B, 1, lr_exp, 0.0, m, mu, loss_kind=0)
    got = run_cut(case, lr, k_cut, hp, snap, corr)
    _assert_exact(got, ref, case)


# --------------------------------------------------------------------------
# random-valued companions
# --------------------------------------------------------------------------
@pytest.mark.parametrize('kind', cc.KINDS)
@pytest.mark.parametrize('loss_kind,K,F,B,C,tau', cc.RANDOM)
def test_random_against_float64(kind, loss_kind, K, F, B, C, tau):
    case, lr, k_cut, hp, snap, corr, ref, e32 = cc.random_case(
        kind, loss_kind, K, F, B, C, tau)
    got = run_cut(case, lr, k_cut, hp, snap, corr)
    assert torch.equal(got['mom_init'].cpu(), ref['mom_init'])
    for k in cc.OUTPUTS:
        assert lc.same_nan_pattern(got[k], ref[k]), k
        scale = ref[k][~torch.isnan(ref[k])].abs().max().item()
        e, tol = lc.err(got[k], ref[k]), lc.bound(e32[k], scale)
        print('%s %s K=%d F=%d: err %.3e  e32 %.3e  err/e32 %.2f  '
              'err/tol %.3f' % (kind, k, K, F, e, e32[k],
                                e / e32[k] if e32[k] else 0.0, e / tol))
        assert e <= tol, (k, e, tol)
    # the correction took part
    plain = lc.call_op(ops, case, lr, k_cut, hp, snap, device='cuda')
    assert (plain['replicas'][0] - got['replicas'][0]).abs().max() > 1e-4


# --------------------------------------------------------------------------
# behaviour
# --------------------------------------------------------------------------
def _same(x, y):
    x, y = x.cpu(), y.cpu()
    return torch.equal(torch.isnan(x), torch.isnan(y)) \
        and torch.equal(x[~torch.isnan(x)], y[~torch.isnan(y)])


@pytest.mark.parametrize('kind', cc.KINDS)
def test_two_runs_bit_identical(kind):
    case, lr, k_cut, hp, snap, corr, _r, _e = cc.random_case(kind,
                                                             *cc.RANDOM[1])
    a = cc.call_op(ops, case, lr, k_cut, hp, snap, corr, device='cuda')
    b = cc.call_op(ops, case, lr, k_cut, hp, snap, corr, device='cuda')
    for k in ('replicas', 'in_mom', 'snap', 'loss', 'mom_init'):
        assert _same(a[k], b[k]), k


def _args(case, lr, k_cut, hp, snap, corr):
    d = lambda t: t.clone().cuda()  # noqa: E731
    pos = [d(case['X']), d(case['Y']), d(case['idx']), d(case['steps']),
           d(lr), d(case['server']), d(case['replicas']), d(case['in_mom']),
           d(case['mom_init']), d(snap), k_cut]
    kw = dict(w_off=case['w_off'], b_off=case['b_off'], K=case['K'],
              loss_kind=case['loss_kind'], weight_decay=hp['wd'],
              momentum=hp['m'], dampening=hp['damp'],
              nesterov=hp['nesterov'], **cc.corr_kwargs(corr, 'cuda'))
    return pos, kw


def test_correction_checks_raise_before_launch():
    case, lr, k_cut, hp, snap, corr, _r, _e = cc.random_case('ctrl',
                                                             *cc.RANDOM[0])
    dl = cc.make_corr(lc.gen('rej'), case, 'delta', False, 0.0)['delta']

    def bad(mutate, match):
        pos, kw = _args(case, lr, k_cut, hp, snap, corr)
        mutate(kw)
        before = [t.clone() for t in pos if torch.is_tensor(t)]
        with pytest.raises(RuntimeError, match=match):
            ops.linear_local_rounds(*pos, **kw)
        torch.cuda.synchronize()
        for t, b in zip([t for t in pos if torch.is_tensor(t)], before):
            assert _same(t, b)                 # nothing was written

    def setk(name, fn):
        return lambda kw: kw.__setitem__(name, fn(kw[name]))

    bad(setk('ctrl_client', lambda t: None), 'pair')
    bad(setk('ctrl_server', lambda t: None), 'pair')
    bad(setk('delta', lambda t: dl.cuda()), 'together')
    bad(setk('ctrl_client', lambda t: t.double()), 'ctrl_client must be')
    bad(setk('ctrl_client', lambda t: t[:-1].contiguous()),
        'ctrl_client must be contiguous')
    bad(setk('ctrl_client', lambda t: t[:, :-1]), 'ctrl_client must be')
    bad(setk('ctrl_server', lambda t: t[:-4].contiguous()),
        'ctrl_server must be contiguous')
    bad(setk('ctrl_server', lambda t: t.cpu()), 'GPU')
    bad(setk('ctrl_server', lambda t: t.half()), 'ctrl_server must be')

    def only_delta(fn):
        def mutate(kw):
            kw.update(ctrl_server=None, ctrl_client=None, delta=fn(dl.cuda()))
        return mutate
    bad(only_delta(lambda t: t.double()), 'delta must be')
    bad(only_delta(lambda t: t[:, :-1]), 'delta must be contiguous')
    bad(only_delta(lambda t: t[0]), 'delta must be contiguous')
    bad(only_delta(lambda t: t.cpu()), 'GPU')
    bad(setk('prox_mu', lambda v: NAN), 'prox_mu')


@pytest.mark.parametrize('kind', cc.KINDS)
def test_graph_capture_replays(kind):
    case, lr, k_cut, hp, snap, corr, _r, _e = cc.random_case(kind,
                                                             *cc.RANDOM[1])
    want = cc.call_op(ops, case, lr, k_cut, hp, snap, corr, device='cuda')
    pos, kw = _args(case, lr, k_cut, hp, snap, corr)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss = ops.linear_local_rounds(*pos, **kw)
    # put the in/out operands back and replay
    pos[6].copy_(case['replicas'])
    pos[7].copy_(case['in_mom'])
    pos[8].copy_(case['mom_init'])
    pos[9].copy_(snap)
    g.replay()
    torch.cuda.synchronize()
    got = dict(replicas=pos[6], in_mom=pos[7], mom_init=pos[8], snap=pos[9],
               loss=loss)
    for k in got:
        assert _same(got[k], want[k]), k


# --------------------------------------------------------------------------
# the two row kernels
# --------------------------------------------------------------------------
def _dev(t):
    return {k: v.cuda() for k, v in t.items()}


# N = 4 * 256 * 3 + 4: more than one block, a ragged last one
@pytest.mark.parametrize('C,N', [(1, 64), (3, 192), (5, 3076)])
def test_row_kernels_against_float64(C, N):
    t = cc.row_case(C, N)
    d = _dev(t)
    want, w32 = cc.ref_delta_rows(t), cc.ref_delta_rows(t, torch.float32)
    delta, buf = _cut(t['state'], NAN)
    ops.multi_delta_update(delta, d['server'], d['agg'], d['replicas'],
                           d['inv'])
    torch.cuda.synchronize()
    assert _guards_intact(buf, NAN)
    assert lc.same_nan_pattern(delta, want)        # offline rows untouched
    scale = want[~torch.isnan(want)].abs().max().item()
    e, tol = lc.err(delta, want), lc.bound(lc.err(w32, want), scale)
    print('delta rows C=%d N=%d: err %.3e tol %.3e' % (C, N, e, tol))
    assert e <= tol
    (wc, wo), (c32, o32) = cc.ref_ctrl_rows(t), cc.ref_ctrl_rows(
        t, torch.float32)
    ctrl, cbuf = _cut(t['state'], NAN)
    out, obuf = _cut(torch.full((N,), NAN), NAN)
    ops.multi_scaffold_control_update(ctrl, d['ctrl_server'], d['server'],
                                      d['replicas'], d['inv'], d['weights'],
                                      out)
    torch.cuda.synchronize()
    assert _guards_intact(cbuf, NAN) and _guards_intact(obuf, NAN)
    assert lc.same_nan_pattern(ctrl, wc) and not torch.isnan(out).any()
    scale = wc[~torch.isnan(wc)].abs().max().item()
    e, tol = lc.err(ctrl, wc), lc.bound(lc.err(c32, wc), scale)
    eo, tolo = lc.err(out, wo), lc.bound(lc.err(o32, wo),
                                         wo.abs().max().item())
    print('ctrl rows C=%d N=%d: err %.3e tol %.3e  out err %.3e tol %.3e'
          % (C, N, e, tol, eo, tolo))
    assert e <= tol and eo <= tolo
    for k in ('server', 'agg', 'replicas', 'inv', 'weights', 'ctrl_server'):
        assert _same(d[k], t[k]), k                # inputs unchanged


def test_row_kernels_one_row_equal_the_single_row_kernels():
    t = cc.row_case(1, 3076, offline=())
    d = _dev(t)
    coef = float(t['inv'][0])
    a = d['state'].clone()
    ops.multi_delta_update(a, d['server'], d['agg'], d['replicas'], d['inv'])
    b = d['state'][0].clone()
    ops.delta_update(b, d['server'], d['agg'], d['replicas'][0].contiguous(),
                     coef)
    assert torch.equal(a[0], b)
    ctrl, out = d['state'].clone(), torch.empty(3076, device='cuda')
    ops.multi_scaffold_control_update(ctrl, d['ctrl_server'], d['server'],
                                      d['replicas'], d['inv'], d['weights'],
                                      out)
    new, diff = torch.empty_like(out), torch.empty_like(out)
    ops.scaffold_control_update(new, d['state'][0].contiguous(),
                                d['ctrl_server'], d['server'],
                                d['replicas'][0].contiguous(), coef)
    ops.scaled_diff(new, d['state'][0].contiguous(), diff,
                    float(t['weights'][0]))
    assert torch.equal(ctrl[0], new) and torch.equal(out, diff)


def test_row_kernels_reject_bad_operands():
    d = _dev(cc.row_case(3, 192))
    before = d['state'].clone()
    for kw, match in ((dict(server=d['server'][:-4].contiguous()), 'server'),
                      (dict(inv=d['inv'].double()), 'inv'),
                      (dict(replicas=d['replicas'][:2].contiguous()),
                       'replicas'),
                      (dict(agg=d['agg'].cpu()), 'agg')):
        a = dict(d, **kw)
        with pytest.raises(RuntimeError, match=match):
            ops.multi_delta_update(a['state'], a['server'], a['agg'],
                                   a['replicas'], a['inv'])
    out = torch.empty(192, device='cuda')
    for kw, match in ((dict(weights=d['weights'][:2].contiguous()),
                       'weights'),
                      (dict(ctrl_server=d['ctrl_server'].half()),
                       'ctrl_server')):
        a = dict(d, **kw)
        with pytest.raises(RuntimeError, match=match):
            ops.multi_scaffold_control_update(
                a['state'], a['ctrl_server'], a['server'], a['replicas'],
                a['inv'], a['weights'], out)
    with pytest.raises(RuntimeError, match='out'):
        ops.multi_scaffold_control_update(
            d['state'], d['ctrl_server'], d['server'], d['replicas'],
            d['inv'], d['weights'], out[:-4])
    torch.cuda.synchronize()
    assert _same(d['state'], before)


# --------------------------------------------------------------------------
# packed federations through ClientPack: both flags on against the slot loop
# --------------------------------------------------------------------------
def _federation(ftype, batched, monkeypatch, record):
    from fedtorch_amd.parameters import get_args
    from fedtorch_amd.nodes import Client
    monkeypatch.setattr(multiclient, '_BATCHED_ENABLED', batched)
    monkeypatch.setattr(multiclient, '_BATCHED_CORR_ENABLED', batched)
    os.environ['FEDTORCH_SYNTH_SIZE'] = '200'
    torch.manual_seed(5)
    np.random.seed(5)
    args = get_args([
        '-d', 'synthetic', '-a', 'logistic_regression', '-f', 'true',
        '--iid_data', 'false',
        '--federated_type', ftype, '--num_comms', '3',
        '--clients_per_rank', '4', '-b', '10', '--lr', '0.1',
        '--federated_sync_type', 'local_step', '--local_step', '3',
        '--online_client_rate', '1.0', '--in_momentum', 'true',
        '--in_momentum_factor', '0.9', '--weight_decay', '1e-3',
        '--stop_criteria', 'epoch', '--num_epochs', '8',
        '--on_cuda', 'true', '-j', '0', '--manual_seed', '7',
        '--checkpoint', '/tmp/ft_linround_corr_gpu', '--debug', 'false'])
    client = Client(args, 0)
    client.initialize()
    client.initialize_dataset()
    client.load_local_dataset()
    client.gen_aux_models()
    pack = multiclient.ClientPack(client, 4)
    pack.build_loaders()
    assert pack.batched_eligible() == batched, pack.batched_blockers()
    assert pack.linear_layout()[2:] == (10, 60)
    out = cc.run_federation(client, pack, monkeypatch, record=record,
                            record_calls=batched)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('ftype', ['scaffold', 'fedgate'])
def test_packed_federation_kernel_against_slot_loop(ftype, monkeypatch):
    """C = 4, tau = 3, F = 60, K = 10, 3 rounds through real
    DeviceCachedLoaders: both flags on (one launch and one row-kernel launch
    per round) against flags off (the slot loop).  Every recorded kernel
    call is bounded against the float64 loop over its own operands; the
    final distance between the two trajectories stays within the bound of
    the fp32-vs-float64 replay of the whole trajectory."""
    with monkeypatch.context() as m:
        off, meta, rec = _federation(ftype, False, m, True)
    with monkeypatch.context() as m:
        on, _meta, brec = _federation(ftype, True, m, False)
    assert not rec['calls'] and len(brec['calls']) == 3
    key = 'delta' if ftype == 'fedgate' else 'ctrl_client'
    for r, call in enumerate(brec['calls']):
        pos, kw = call['pos'], call['kw']
        assert pos[2].shape == (4, 3, 10) and pos[3].tolist() == [3] * 4
        assert kw[key] is not None and kw.get('prox_mu', 0.0) == 0.0
        # from round 2 on the correction is live
        assert bool(kw[key].any()) == (r > 0), r
        case = dict(X=pos[0], Y=pos[1], idx=pos[2], steps=pos[3],
                    server=pos[5], replicas=pos[6], in_mom=pos[7],
                    mom_init=pos[8], w_off=kw['w_off'], b_off=kw['b_off'],
                    K=kw['K'], loss_kind=kw['loss_kind'])
        hp = dict(wd=kw['weight_decay'], m=kw['momentum'],
                  damp=kw['dampening'], nesterov=kw['nesterov'])
        corr = dict(delta=kw.get('delta'), ctrl_server=kw.get('ctrl_server'),
                    ctrl_client=kw.get('ctrl_client'), prox_mu=0.0)
        r64 = cc.ref_rounds_corr(case, pos[4], 0, hp, corr)
        r32 = cc.ref_rounds_corr(case, pos[4], 0, hp, corr,
                                 dtype=torch.float32)
        for k in ('replicas', 'in_mom'):
            e32 = lc.err(r32[k], r64[k])
            tol = lc.bound(e32, r64[k].abs().max().item())
            e = lc.err(call[k], r64[k])
            print('%s round %d %s: kernel err %.3e  e32 %.3e  tol %.3e'
                  % (ftype, r + 1, k, e, e32, tol))
            assert e <= tol, (r, k, e, tol)
    t64, entering = cc.replay_federation(rec, meta, torch.float64)
    t32, _e = cc.replay_federation(rec, meta, torch.float32)
    assert entering[0] == 0.0 and entering[1] > 1e-3 and entering[2] > 1e-3
    assert sorted(on) == sorted(off) == sorted(t64)
    for k in sorted(t64):
        e32 = lc.err(t32[k], t64[k])
        tol = lc.bound(e32, t64[k].abs().max().item())
        d = (on[k] - off[k]).abs().max().item()
        print('%s %s: on-off %.3e  on err %.3e  off err %.3e  e32 %.3e  '
              'tol %.3e' % (ftype, k, d, lc.err(on[k], t64[k]),
                            lc.err(off[k], t64[k]), e32, tol))
        assert d <= tol, (k, d, tol)
