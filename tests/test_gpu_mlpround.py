# -*- coding: utf-8 -*-
"""mlp_local_rounds (hip/mlpround.h) on the GPU against the float64 step loop
of tests/mlpround_cases.py: the three shapes with operands cut out of
NaN-filled buffers, bounded by the fp32 CPU loop's own error; determinism,
launcher argument checks, graph capture, and a packed round through
ClientPack with the flag on against the slot loop.

Measured on an MI355X: see profiles/packed_mlp_notes.md."""
import math
import os

import numpy as np
import pytest
import torch

import linround_cases as lc
import mlpround_cases as mc
import fedtorch_amd.ops as ops
from fedtorch_amd.parallel import multiclient

pytestmark = pytest.mark.gpu

NAN = float('nan')
PAD = 96
_REAL_OP = ops.mlp_local_rounds
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
    return dict(layout=case['layout'], eps=case['eps'], wd_numel=wd_numel,
                weight_decay=hp['wd'], momentum=hp['m'],
                dampening=hp['damp'], nesterov=hp['nesterov'])


def run_cut(case, lr, k_cut, hp, snap, wd_numel):
    """the HIP path with every operand cut out of a NaN-filled (float) or
    plausible-but-wrong (int) buffer; asserts the guard zones afterwards"""
    M = case['X'].shape[0]
    fills = dict(X=NAN, Y=case['layout']['head'][2] - 1, idx=M - 1, steps=0,
                 lr=NAN, server=NAN, replicas=NAN, in_mom=NAN, mom_init=7,
                 snap=NAN)
    src = dict(case, lr=lr, snap=snap)
    v, bufs = {}, {}
    for k in KEYS:
        if src[k] is None:
            v[k] = None
        else:
            v[k], bufs[k] = _cut(src[k], fills[k])
    loss = ops.mlp_local_rounds(
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
                mom_init=v['mom_init'], snap=v['snap'], loss=loss)


def test_limits_match_the_extension():
    assert ops._C.mlp_round_max_batch() == ops.mlp_round_max_batch() \
        == ops.MLPROUND_MAXB
    assert ops._C.mlp_round_max_classes() == ops.mlp_round_max_classes() \
        == ops.MLPROUND_MAXK
    assert ops._C.mlp_round_max_layers() == ops.MLPROUND_MAXL


# --------------------------------------------------------------------------
# numerics and guards
# --------------------------------------------------------------------------
@pytest.mark.parametrize('shape', mc.SHAPES)
def test_against_float64_replay(shape):
    """bound: 8x the fp32 CPU replay's own error plus 16 fp32 ulps of the
    output's scale (lc.bound), fixed before the first GPU run"""
    case, lr, k_cut, hp, snap, wd_numel, ref, e32 = mc.case(*shape)
    got = run_cut(case, lr, k_cut, hp, snap, wd_numel)
    assert torch.equal(got['mom_init'].cpu(), ref['mom_init'])
    for k in mc.OUTPUTS:
        if ref[k] is None:
            assert got[k] is None
            continue
        assert lc.same_nan_pattern(got[k], ref[k]), k
        e, tol = lc.err(got[k], ref[k]), lc.bound(e32[k], mc.scale_of(ref[k]))
        print('%s %s: err %.3e  e32 %.3e  err/e32 %.2f  err/tol %.3f'
              % (shape, k, e, e32[k], e / e32[k] if e32[k] else 0.0, e / tol))
        assert e <= tol, (k, e, tol)
    # offline client 1: nothing written
    assert torch.isnan(got['replicas'][1]).all()
    assert torch.isnan(got['snap'][1]).all()
    assert not got['loss'][1].any()
    gap = mc.gap_mask(case['layout'], case['N'])
    if got['in_mom'] is not None:
        mom = got['in_mom'].cpu()
        assert torch.equal(mom[1], case['in_mom'][1])
        for c in (0, 2):                   # pad gaps of in_mom stay
            assert torch.equal(mom[c][gap], case['in_mom'][c][gap])
    for c in (0, 2):                       # pad gaps of replicas: server's
        assert torch.equal(got['replicas'][c].cpu()[gap],
                           case['server'][gap])


def test_single_row_step_stays_finite_and_in_bounds():
    """n = 1 (the twin refuses it; the launcher cannot see a device idx
    during capture): xh = 0, everything finite, guards intact"""
    case, lr, k_cut, hp, snap, wd_numel, _ref, _e = mc.case(*mc.SHAPES[1])
    case = dict(case, idx=case['idx'].clone())
    case['idx'][0, 1, 1:] = -1
    got = run_cut(case, lr, k_cut, hp, snap, wd_numel)
    for c in (0, 2):
        assert torch.isfinite(got['replicas'][c]).all()
        assert torch.isfinite(got['in_mom'][c]).all()
    assert torch.isfinite(got['loss']).all()


# --------------------------------------------------------------------------
# behaviour
# --------------------------------------------------------------------------
def _same(a, b):
    for k in ('replicas', 'in_mom', 'snap', 'loss', 'mom_init'):
        x, y = a[k].cpu(), b[k].cpu()
        assert torch.equal(torch.isnan(x), torch.isnan(y)), k
        assert torch.equal(x[~torch.isnan(x)], y[~torch.isnan(y)]), k


def test_two_runs_bit_identical():
    case, lr, k_cut, hp, snap, wd_numel, _ref, _e = mc.case(*mc.SHAPES[2])
    a = mc.call_op(ops, case, lr, k_cut, hp, snap, wd_numel, device='cuda')
    b = mc.call_op(ops, case, lr, k_cut, hp, snap, wd_numel, device='cuda')
    _same(a, b)


def _args(case, lr, k_cut, hp, snap, wd_numel):
    d = lambda t: t.clone().cuda()  # noqa: E731
    pos = [d(case['X']), d(case['Y']), d(case['idx']), d(case['steps']),
           d(lr), d(case['server']), d(case['replicas']), d(case['in_mom']),
           d(case['mom_init']), d(snap), k_cut]
    kw = _kw(case, hp, wd_numel)
    kw['layout'] = dict(blocks=list(kw['layout']['blocks']),
                        head=kw['layout']['head'])
    return pos, kw


def test_argument_checks_raise_before_launch():
    case, lr, k_cut, hp, snap, wd_numel, _r, _e = mc.case(*mc.SHAPES[1])
    X, Y, IDX, STEPS, LR, SRV, REP, MOM, MI, SNAP, KCUT = range(11)

    def bad(mutate, match):
        pos, kw = _args(case, lr, k_cut, hp, snap, wd_numel)
        mutate(pos, kw)
        before = [None if t is None or not torch.is_tensor(t) else t.clone()
                  for t in pos]
        with pytest.raises(RuntimeError, match=match):
            ops.mlp_local_rounds(*pos, **kw)
        torch.cuda.synchronize()
        for t, b in zip(pos, before):      # nothing was written
            if b is not None:
                assert torch.equal(torch.isnan(t), torch.isnan(b))
                assert torch.equal(t[~torch.isnan(t)], b[~torch.isnan(b)])

    def setp(i, fn):
        return lambda pos, kw: pos.__setitem__(i, fn(pos[i]))

    bad(setp(X, lambda t: t.double()), 'X must be fp32')
    bad(setp(Y, lambda t: t.long()), 'Y must be')
    bad(setp(Y, lambda t: t.float()), 'Y must be')
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
    bad(setp(SNAP, lambda t: t[:, :-64].contiguous()), 'snap must be')
    bad(setp(STEPS, lambda t: t + 9), 'steps holds')
    bad(setp(KCUT, lambda k: -1), 'k_cut')
    bad(setp(IDX, lambda t: t[:, :, :1].contiguous()), 'unsupported B=1')
    bad(setp(IDX, lambda t: torch.cat([t] * 5, 2).contiguous()),
        'unsupported B=80')

    def oob(pos, kw):
        pos[IDX][0, 0, 0] = case['X'].shape[0]
    bad(oob, 'idx holds row')

    def blk(i, v):
        def mutate(pos, kw):
            b = list(kw['layout']['blocks'][0])
            b[i] = v
            kw['layout']['blocks'][0] = tuple(b)
        return mutate
    bad(blk(1, 64), 'overlap')
    bad(blk(2, 10 ** 6), 'does not fit')
    bad(blk(0, -1), 'does not fit')
    bad(blk(4, 46), 'input has 45 features')
    bad(blk(5, 71), 'input has 71 features')      # the next block's input
    fc = case['layout']['head'][0]
    bad(lambda pos, kw: kw['layout'].__setitem__('head', (fc, 69, 10)),
        'head reads 69 features')
    bad(lambda pos, kw: kw['layout'].__setitem__('head', (fc, 70, 129)),
        'unsupported K=129')
    bad(lambda pos, kw: kw['layout'].__setitem__('blocks', []),
        'layout has 0 blocks')
    bad(lambda pos, kw: kw.__setitem__('wd_numel', case['N'] + 1), 'wd_numel')
    bad(lambda pos, kw: kw.__setitem__('eps', 0.0), 'eps')
    bad(lambda pos, kw: kw.__setitem__('dampening', 0.5), 'nesterov')


def test_graph_capture_replays():
    case, lr, k_cut, hp, snap, wd_numel, _r, _e = mc.case(*mc.SHAPES[1])
    want = mc.call_op(ops, case, lr, k_cut, hp, snap, wd_numel,
                      device='cuda')
    pos, kw = _args(case, lr, k_cut, hp, snap, wd_numel)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss = ops.mlp_local_rounds(*pos, **kw)
    # put the in/out operands back and replay
    pos[6].copy_(case['replicas'])
    pos[7].copy_(case['in_mom'])
    pos[8].copy_(case['mom_init'])
    pos[9].copy_(snap)
    g.replay()
    torch.cuda.synchronize()
    _same(dict(replicas=pos[6], in_mom=pos[7], mom_init=pos[8], snap=pos[9],
               loss=loss), want)


# --------------------------------------------------------------------------
# a packed round through ClientPack: the kernels against the slot loop
# --------------------------------------------------------------------------
def _packed_round(batched, monkeypatch):
    from fedtorch_amd.parameters import get_args
    from fedtorch_amd.nodes import Client
    from fedtorch_amd.trainings.packed import \
        train_and_validate_federated_packed
    monkeypatch.setattr(multiclient, '_BATCHED_MLP_ENABLED', batched)
    os.environ['FEDTORCH_SYNTH_SIZE'] = '200'
    torch.manual_seed(5)
    np.random.seed(5)
    args = get_args([
        '-d', 'mnist', '-a', 'mlp', '--mlp_hidden_size', '40',
        '--mlp_num_layers', '2', '-f', 'true',
        '--federated_type', 'fedavg', '--num_comms', '1',
        '--clients_per_rank', '4', '-b', '10', '--lr', '0.1',
        '--federated_sync_type', 'local_step', '--local_step', '3',
        '--online_client_rate', '1.0', '--in_momentum', 'true',
        '--in_momentum_factor', '0.9', '--weight_decay', '1e-3',
        '--stop_criteria', 'epoch', '--num_epochs', '8',
        # the seed: searched on the CPU for the ReLU precondition below
        '--on_cuda', 'true', '-j', '0', '--manual_seed', '20',
        '--checkpoint', '/tmp/ft_mlpround_gpu', '--debug', 'false'])
    client = Client(args, 0)
    client.initialize()
    client.initialize_dataset()
    client.load_local_dataset()
    client.gen_aux_models()
    pack = multiclient.ClientPack(client, 4)
    pack.build_loaders()
    assert pack.mlp_batched_eligible() == batched, pack.mlp_batched_blockers()
    assert not pack.batched_eligible()
    rec = {}
    real_acc = pack.accumulate_partial

    def acc(server, weights):
        rec['replicas'] = pack.replicas.clone()
        return real_acc(server, weights)
    monkeypatch.setattr(pack, 'accumulate_partial', acc)

    def op(*a, **k):
        rec['operands'] = ([None if t is None or not torch.is_tensor(t)
                            else t.clone().cpu() for t in a], dict(k))
        return _REAL_OP(*a, **k)
    monkeypatch.setattr(ops, 'mlp_local_rounds', op)
    train_and_validate_federated_packed(client, pack)
    torch.cuda.synchronize()
    rec['in_mom'] = pack.in_mom.clone()
    return rec


def test_packed_round_kernels_against_slot_loop(monkeypatch):
    """C = 4, tau = 3, MLP 784-40-40-10 through real DeviceCachedLoaders:
    flag on (the batched kernels) against flag off (the slot loop: library
    GEMMs, autograd, the fused SGD kernel).  Both are bounded against the
    float64 loop over the operands the batched round recorded; the kernels'
    error and the distance between the two stay within lc.bound (the slot
    loop's own error is printed).  The ReLU precondition of
    mlpround_cases.case is asserted for the recorded operands."""
    off = _packed_round(False, monkeypatch)
    on = _packed_round(True, monkeypatch)
    assert 'operands' not in off
    pos, kw = on['operands']
    X, Y, idx, steps, lr, server, replicas, in_mom, mom_init, snap = pos[:10]
    assert idx.shape == (4, 3, 10) and steps.tolist() == [3, 3, 3, 3]
    assert snap is None
    refs, pre = {}, {}
    for dt in (torch.float64, torch.float32):
        pre[dt] = []
        refs[dt] = mc.ref_rounds(
            X, Y, idx, steps, lr, server, replicas, in_mom, mom_init, None,
            0, kw['layout'], kw['eps'], kw['wd_numel'], kw['weight_decay'],
            kw['momentum'], kw['dampening'], kw['nesterov'], dtype=dt,
            pre=pre[dt])
    lo = min(y.abs().min().item() for y in pre[torch.float64])
    e = max((a.double() - b).abs().max().item()
            for a, b in zip(pre[torch.float32], pre[torch.float64]))
    assert lo > mc.MARGIN * e, (lo, e)
    ref = refs[torch.float64]
    for k in ('replicas', 'in_mom'):
        e32 = lc.err(refs[torch.float32][k], ref[k])
        tol = lc.bound(e32, ref[k].abs().max().item())
        e_on, e_off = lc.err(on[k], ref[k]), lc.err(off[k], ref[k])
        d = (on[k] - off[k]).abs().max().item()
        print('%s: kernel err %.3e  slot loop err %.3e  e32 %.3e  tol %.3e  '
              'on-off %.3e' % (k, e_on, e_off, e32, tol, d))
        assert e_on <= tol and e_off <= tol and d <= tol, k
