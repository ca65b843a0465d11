# -*- coding: utf-8 -*-
"""linear_local_rounds (hip/linearround.h) on the GPU against the float64
step loop of tests/linround_cases.py: exact least-squares and softmax-CE
cases with operands cut out of NaN-filled buffers, random-valued companions
bounded by the fp32 CPU loop's own error, determinism, launcher argument
checks, graph capture, and a packed round through ClientPack with the flag on
against the slot loop.

Measured on an MI355X: see profiles/packed_linear_notes.md."""
import math
import os

import numpy as np
import pytest
import torch

import linround_cases as lc
import fedtorch_amd.ops as ops
from fedtorch_amd.parallel import multiclient

pytestmark = pytest.mark.gpu

NAN = float('nan')
PAD = 96
_REAL_OP = ops.linear_local_rounds
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


def run_cut(case, lr, k_cut, hp, snap):
    """the HIP path with every operand cut out of a NaN-filled (float) or
    plausible-but-wrong (int) buffer; asserts the guard zones afterwards"""
    M = case['X'].shape[0]
    fills = dict(X=NAN, Y=NAN if case['loss_kind'] else case['K'] - 1,
                 idx=M - 1, steps=0, lr=NAN, server=NAN, replicas=NAN,
                 in_mom=NAN, mom_init=7, snap=NAN)
    src = dict(case, lr=lr, snap=snap)
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
        momentum=hp['m'], dampening=hp['damp'], nesterov=hp['nesterov'])
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert _guards_intact(b, fills[k]), 'guard zone of %s written' % k
    for k in ('X', 'Y', 'idx', 'steps', 'lr', 'server'):   # inputs unchanged
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
        # the NaN prefill survives in the rows of offline clients and in
        # snap rows that were not due
        assert lc.same_nan_pattern(got[k], ref[k]), k
        assert lc.err(got[k], ref[k]) == 0.0, k
    assert torch.equal(got['mom_init'].cpu(), ref['mom_init'])
    off = [c for c, s in enumerate(case['steps'].tolist()) if s == 0]
    for c in off:
        assert torch.isnan(got['replicas'][c]).all()
        assert not got['loss'][c].any()
        if got['in_mom'] is not None:
            assert torch.equal(got['in_mom'][c].cpu(), case['in_mom'][c])


def test_limits_match_the_extension():
    assert ops._C.linear_round_max_floats(False) == \
        ops.linear_round_max_floats(False) == ops.LINROUND_LDS_FLOATS
    assert ops._C.linear_round_max_floats(True) == \
        ops.linear_round_max_floats(True)
    for F, K, B, m in ((784, 10, 50, True), (60, 10, 50, False),
                       (1, 1, 2, True), (3072, 16, 64, False)):
        assert ops._C.linear_round_lds_floats(F, K, B, m) == \
            ops.linear_round_lds_floats(F, K, B, m)


# --------------------------------------------------------------------------
# exact cases
# --------------------------------------------------------------------------
@pytest.mark.parametrize('F,B,C,tau,lr_exp,wd,m', lc.EXACT_LS)
def test_exact_least_squares(F, B, C, tau, lr_exp, wd, m):
    case, lr, k_cut, hp, snap, ref = lc.exact_case(F, B, C, tau, lr_exp, wd,
                                                   m)
    got = run_cut(case, lr, k_cut, hp, snap)
    _assert_exact(got, ref, case)
    assert torch.equal(got['loss'].double().cpu(), ref['loss'])


@pytest.mark.parametrize('F,B,C,lr_exp,m', lc.EXACT_CE)
def test_exact_softmax_ce_from_zero(F, B, C, lr_exp, m):
    """zero weights: p = 1/2 exactly, so W, b and momentum are exact.  The
    loss is log 2: logf is good to 2 ulps, the B - 1 additions of the row
    losses round once each (<= 2^-24 relative), the division by B is exact
    (B a power of two; a short batch adds one more rounding)."""
    case, lr, k_cut, hp, snap, ref = lc.exact_case(F, B, C, 1, lr_exp, 0.0,
                                                   m, loss_kind=0)
    got = run_cut(case, lr, k_cut, hp, snap)
    _assert_exact(got, ref, case)
    e = (got['loss'].double().cpu() - ref['loss']).abs().max().item()
    tol = math.log(2) * (B + 4) * 2.0 ** -24
    print('CE loss err %.3e tol %.3e' % (e, tol))
    assert e <= tol


# --------------------------------------------------------------------------
# random-valued companions
# --------------------------------------------------------------------------
@pytest.mark.parametrize('loss_kind,K,F,B,C,tau', lc.RANDOM)
def test_random_against_float64(loss_kind, K, F, B, C, tau):
    case, lr, k_cut, hp, snap, ref, e32 = lc.random_case(loss_kind, K, F, B,
                                                         C, tau)
    got = run_cut(case, lr, k_cut, hp, snap)
    assert torch.equal(got['mom_init'].cpu(), ref['mom_init'])
    for k in ('replicas', 'in_mom', 'snap', 'loss'):
        assert lc.same_nan_pattern(got[k], ref[k]), k
        scale = ref[k][~torch.isnan(ref[k])].abs().max().item()
        e, tol = lc.err(got[k], ref[k]), lc.bound(e32[k], scale)
        print('%s K=%d F=%d: err %.3e  e32 %.3e  err/e32 %.2f  err/tol %.3f'
              % (k, K, F, e, e32[k], e / e32[k] if e32[k] else 0.0, e / tol))
        assert e <= tol, (k, e, tol)


# --------------------------------------------------------------------------
# behaviour
# --------------------------------------------------------------------------
def test_two_runs_bit_identical():
    case, lr, k_cut, hp, snap, _ref, _e = lc.random_case(*lc.RANDOM[1])
    a = lc.call_op(ops, case, lr, k_cut, hp, snap, device='cuda')
    b = lc.call_op(ops, case, lr, k_cut, hp, snap, device='cuda')
    for k in ('replicas', 'in_mom', 'snap', 'loss', 'mom_init'):
        x, y = a[k].cpu(), b[k].cpu()
        assert torch.equal(torch.isnan(x), torch.isnan(y))
        assert torch.equal(x[~torch.isnan(x)], y[~torch.isnan(y)]), k


def _args(case, lr, k_cut, hp, snap):
    d = lambda t: t.clone().cuda()  # noqa: E731
    pos = [d(case['X']), d(case['Y']), d(case['idx']), d(case['steps']),
           d(lr), d(case['server']), d(case['replicas']), d(case['in_mom']),
           d(case['mom_init']), d(snap), k_cut]
    kw = dict(w_off=case['w_off'], b_off=case['b_off'], K=case['K'],
              loss_kind=case['loss_kind'], weight_decay=hp['wd'],
              momentum=hp['m'], dampening=hp['damp'],
              nesterov=hp['nesterov'])
    return pos, kw


def test_argument_checks_raise_before_launch():
    case, lr, k_cut, hp, snap, _r, _e = lc.random_case(*lc.RANDOM[0])
    X, Y, IDX, STEPS, LR, SRV, REP, MOM, MI, SNAP = range(10)

    def bad(mutate, match):
        pos, kw = _args(case, lr, k_cut, hp, snap)
        mutate(pos, kw)
        before = [None if t is None or not torch.is_tensor(t) else t.clone()
                  for t in pos]
        with pytest.raises(RuntimeError, match=match):
            ops.linear_local_rounds(*pos, **kw)
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
    bad(setp(IDX, lambda t: t.transpose(1, 2).contiguous().transpose(1, 2)),
        'contiguous')
    bad(setp(REP, lambda t: t[:, :-1]), 'replicas must be contiguous')
    bad(setp(SRV, lambda t: t.cpu()), 'GPU')
    bad(setp(MOM, lambda t: t[:-1].contiguous()), 'in_mom must be')
    bad(setp(STEPS, lambda t: t + 9), 'steps holds')

    def oob(pos, kw):
        pos[IDX][0, 0, 0] = case['X'].shape[0]
    bad(oob, 'idx holds row')
    bad(lambda pos, kw: kw.__setitem__('K', 17), 'unsupported K=17')
    bad(lambda pos, kw: kw.__setitem__('loss_kind', 1), 'MSE needs K == 1')
    bad(lambda pos, kw: kw.__setitem__('b_off', kw['w_off'] + 1),
        'do not fit')

    # over the LDS limit: F * (K | 1) floats alone exceed it with momentum
    F, K = 2048, 10
    g = lc.gen('big')
    big = lc.make_case(g, F, K, 4, 1, 1, 8, 0, [1], integer=False, m=0.9)
    assert ops.linear_round_lds_floats(F, K, 4, True) \
        > ops.LINROUND_LDS_FLOATS
    pos, kw = _args(big, torch.full((1, 1), .1), 0, hp,
                    torch.full((1, big['N']), NAN))
    with pytest.raises(RuntimeError, match='floats of LDS'):
        ops.linear_local_rounds(*pos, **kw)
    kw.update(momentum=0.0, nesterov=False)        # fits without momentum
    assert ops.linear_round_lds_floats(F, K, 4, False) \
        <= ops.LINROUND_LDS_FLOATS
    ops.linear_local_rounds(*pos, **kw)
    torch.cuda.synchronize()
    assert not torch.isnan(pos[REP]).any()


def test_graph_capture_replays():
    case, lr, k_cut, hp, snap, _r, _e = lc.random_case(*lc.RANDOM[1])
    want = lc.call_op(ops, case, lr, k_cut, hp, snap, device='cuda')
    pos, kw = _args(case, lr, k_cut, hp, snap)
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
        x, y = got[k].cpu(), want[k].cpu()
        assert torch.equal(torch.isnan(x), torch.isnan(y)), k
        assert torch.equal(x[~torch.isnan(x)], y[~torch.isnan(y)]), k


# --------------------------------------------------------------------------
# a packed round through ClientPack: the kernel against the slot loop
# --------------------------------------------------------------------------
def _packed_round(batched, monkeypatch):
    from fedtorch_amd.parameters import get_args
    from fedtorch_amd.nodes import Client
    from fedtorch_amd.trainings.packed import \
        train_and_validate_federated_packed
    monkeypatch.setattr(multiclient, '_BATCHED_ENABLED', batched)
    os.environ['FEDTORCH_SYNTH_SIZE'] = '200'
    torch.manual_seed(5)
    np.random.seed(5)
    args = get_args([
        '-d', 'synthetic', '-a', 'logistic_regression', '-f', 'true',
        '--iid_data', 'false',
        '--federated_type', 'fedavg', '--num_comms', '1',
        '--clients_per_rank', '4', '-b', '10', '--lr', '0.1',
        '--federated_sync_type', 'local_step', '--local_step', '3',
        '--online_client_rate', '1.0', '--in_momentum', 'true',
        '--in_momentum_factor', '0.9', '--weight_decay', '1e-3',
        '--stop_criteria', 'epoch', '--num_epochs', '8',
        '--on_cuda', 'true', '-j', '0', '--manual_seed', '7',
        '--checkpoint', '/tmp/ft_linround_gpu', '--debug', 'false'])
    client = Client(args, 0)
    client.initialize()
    client.initialize_dataset()
    client.load_local_dataset()
    client.gen_aux_models()
    pack = multiclient.ClientPack(client, 4)
    pack.build_loaders()
    assert pack.batched_eligible() == batched, pack.batched_blockers()
    assert pack.linear_layout()[2:] == (10, 60)
    # a non-trivial start: the convex models start from zero weights
    g = lc.gen('packed-start')
    client.model_server.copy_(torch.randn(client.arena.numel, generator=g)
                              .mul_(.1).cuda())
    w_off, b_off, K, F = pack.linear_layout()
    gap = torch.ones(client.arena.numel, dtype=torch.bool)
    gap[w_off:w_off + K * F] = False
    gap[b_off:b_off + K] = False
    client.model_server[gap.cuda()] = 0            # pad gaps stay zero
    rec = {}
    real_acc = pack.accumulate_partial

    def acc(server, weights):
        rec['replicas'] = pack.replicas.clone()
        return real_acc(server, weights)
    monkeypatch.setattr(pack, 'accumulate_partial', acc)
    def op(*a, **k):
        rec['operands'] = ([None if t is None or not torch.is_tensor(t)
                            else t.clone().cpu() for t in a], dict(k),
                           a[10])
        return _REAL_OP(*a, **k)
    monkeypatch.setattr(ops, 'linear_local_rounds', op)
    train_and_validate_federated_packed(client, pack)
    torch.cuda.synchronize()
    rec['in_mom'] = pack.in_mom.clone()
    rec['server'] = client.model_server.clone()
    return rec


def test_packed_round_kernel_against_slot_loop(monkeypatch):
    """C = 4, tau = 3, F = 60, K = 10 through real DeviceCachedLoaders: flag
    on (one launch) against flag off (the slot loop: library GEMMs, autograd,
    the fused SGD kernel).  Both are bounded against the float64 loop over
    the operands the batched round recorded; the kernel's error and the
    distance between the two stay within the bound of the random
    companions (the slot loop's own error is printed)."""
    off = _packed_round(False, monkeypatch)
    on = _packed_round(True, monkeypatch)
    assert 'operands' not in off
    pos, kw, k_cut = on['operands']
    X, Y, idx, steps, lr, server, replicas, in_mom, mom_init, snap = pos[:10]
    assert idx.shape == (4, 3, 10) and steps.tolist() == [3, 3, 3, 3]
    refs = {}
    for dt in (torch.float64, torch.float32):
        refs[dt] = lc.ref_rounds(
            X, Y, idx, steps, lr, server, replicas, in_mom, mom_init, None,
            0, kw['w_off'], kw['b_off'], kw['K'], kw['loss_kind'],
            kw['weight_decay'], kw['momentum'], kw['dampening'],
            kw['nesterov'], dtype=dt)
    ref = refs[torch.float64]
    for k in ('replicas', 'in_mom'):
        e32 = lc.err(refs[torch.float32][k], ref[k])
        tol = lc.bound(e32, ref[k].abs().max().item())
        e_on, e_off = lc.err(on[k], ref[k]), lc.err(off[k], ref[k])
        d = (on[k] - off[k]).abs().max().item()
        print('%s: kernel err %.3e  slot loop err %.3e  e32 %.3e  tol %.3e  '
              'on-off %.3e' % (k, e_on, e_off, e32, tol, d))
        assert e_on <= tol and d <= tol, k
