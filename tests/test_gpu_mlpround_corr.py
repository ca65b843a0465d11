# -*- coding: utf-8 -*-
"""The gradient corrections of mlp_local_rounds (hip/mlpround.h: delta / the
control pair / prox_mu in the batched backward kernels) on the GPU against
the float64 step loop of tests/mlpround_corr_cases.py: the nine (shape, kind)
cases with every operand cut out of NaN-filled buffers, bounded by the fp32
CPU loop's own error; the correction-free call, determinism, launcher
rejections, graph capture, and packed federations through ClientPack with
both flags on against the slot loop.

Measured on an MI355X: see profiles/packed_mlp_notes.md."""
import os

import numpy as np
import pytest
import torch

import linround_cases as lc
import mlpround_cases as mc
import mlpround_corr_cases as cc
import fedtorch_amd.ops as ops
from fedtorch_amd.parallel import multiclient
from test_gpu_mlpround import _cut, _guards_intact, _kw, _same

pytestmark = pytest.mark.gpu

NAN = float('nan')
_REAL_OP = ops.mlp_local_rounds
KEYS = ('X', 'Y', 'idx', 'steps', 'lr', 'server', 'replicas', 'in_mom',
        'mom_init', 'snap', 'delta', 'ctrl_server', 'ctrl_client')
INPUTS = ('X', 'Y', 'idx', 'steps', 'lr', 'server', 'delta', 'ctrl_server',
          'ctrl_client')


def run_cut(case, lr, k_cut, hp, snap, wd_numel, corr):
    """the HIP path with every operand, the corrections included, cut out
    of a NaN-filled (float) or plausible-but-wrong (int) buffer; asserts the
    guard zones and the inputs afterwards"""
    M = case['X'].shape[0]
    fills = dict(X=NAN, Y=case['layout']['head'][2] - 1, idx=M - 1, steps=0,
                 lr=NAN, server=NAN, replicas=NAN, in_mom=NAN, mom_init=7,
                 snap=NAN, delta=NAN, ctrl_server=NAN, ctrl_client=NAN)
    src = dict(case, lr=lr, snap=snap, delta=corr['delta'],
               ctrl_server=corr['ctrl_server'],
               ctrl_client=corr['ctrl_client'])
    v, bufs = {}, {}
    for k in KEYS:
        if src[k] is None:
            v[k] = None
        else:
            v[k], bufs[k] = _cut(src[k], fills[k])
    loss = ops.mlp_local_rounds(
        v['X'], v['Y'], v['idx'], v['steps'], v['lr'], v['server'],
        v['replicas'], v['in_mom'], v['mom_init'], v['snap'], k_cut,
        delta=v['delta'], ctrl_server=v['ctrl_server'],
        ctrl_client=v['ctrl_client'], prox_mu=corr['prox_mu'],
        **_kw(case, hp, wd_numel))
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert _guards_intact(b, fills[k]), 'guard zone of %s written' % k
    for k in INPUTS:                       # inputs unchanged, bit for bit
        if src[k] is not None:
            assert torch.equal(v[k].cpu().view(torch.int32),
                               src[k].view(torch.int32)), k
    assert loss.dtype == torch.float32 and loss.is_contiguous()
    assert loss.shape == case['idx'].shape[:2]
    return dict(replicas=v['replicas'], in_mom=v['in_mom'],
                mom_init=v['mom_init'], snap=v['snap'], loss=loss)


# --------------------------------------------------------------------------
# numerics and guards
# --------------------------------------------------------------------------
@pytest.mark.parametrize('shape,kind', cc.PAIRS)
def test_against_float64_replay(shape, kind):
    """bound: 8x the fp32 CPU replay's own error plus 16 fp32 ulps of the
    output's scale (lc.bound), the project's bound for these kernels"""
    case, lr, k_cut, hp, snap, wd_numel, corr, ref, e32 = cc.case(shape, kind)
    got = run_cut(case, lr, k_cut, hp, snap, wd_numel, corr)
    assert torch.equal(got['mom_init'].cpu(), ref['mom_init'])
    for k in mc.OUTPUTS:
        if ref[k] is None:
            assert got[k] is None
            continue
        assert lc.same_nan_pattern(got[k], ref[k]), k
        e, tol = lc.err(got[k], ref[k]), lc.bound(e32[k], mc.scale_of(ref[k]))
        print('%s %s %s: err %.3e  e32 %.3e  err/e32 %.2f  err/tol %.3f'
              % (shape, kind, k, e, e32[k], e / e32[k] if e32[k] else 0.0,
                 e / tol))
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


# --------------------------------------------------------------------------
# behaviour
# --------------------------------------------------------------------------
def test_no_correction_is_the_correction_free_call():
    """no correction given, and prox_mu = 0 with None tensors: bit-identical
    to each other (both run the kernels that know no correction)"""
    case, lr, k_cut, hp, snap, wd_numel, _ref, _e = mc.case(*mc.SHAPES[1])
    a = mc.call_op(ops, case, lr, k_cut, hp, snap, wd_numel, device='cuda')
    b = cc.call_op(ops, case, lr, k_cut, hp, snap, wd_numel, cc.no_corr(),
                   device='cuda')
    _same(a, b)


@pytest.mark.parametrize('kind', cc.KINDS)
def test_two_runs_bit_identical(kind):
    case, lr, k_cut, hp, snap, wd_numel, corr, _r, _e = \
        cc.case(cc.SHAPES[1], kind)
    a = cc.call_op(ops, case, lr, k_cut, hp, snap, wd_numel, corr,
                   device='cuda')
    b = cc.call_op(ops, case, lr, k_cut, hp, snap, wd_numel, corr,
                   device='cuda')
    _same(a, b)


def _args(case, lr, k_cut, hp, snap, wd_numel, corr):
    d = lambda t: t.clone().cuda()  # noqa: E731
    pos = [d(case['X']), d(case['Y']), d(case['idx']), d(case['steps']),
           d(lr), d(case['server']), d(case['replicas']), d(case['in_mom']),
           d(case['mom_init']), d(snap), k_cut]
    kw = _kw(case, hp, wd_numel)
    kw.update(cc.corr_kwargs(corr, 'cuda'))
    return pos, kw


def test_correction_checks_raise_before_launch():
    shape = cc.SHAPES[1]
    case, lr, k_cut, hp, snap, wd_numel, ctrl, _r, _e = cc.case(shape, 'ctrl')
    delta = cc.case(shape, 'delta')[6]

    def bad(corr, mutate, match):
        pos, kw = _args(case, lr, k_cut, hp, snap, wd_numel, corr)
        mutate(kw)
        before = [None if not torch.is_tensor(t) else t.clone() for t in pos]
        with pytest.raises(RuntimeError, match=match):
            ops.mlp_local_rounds(*pos, **kw)
        torch.cuda.synchronize()
        for t, b in zip(pos, before):      # nothing was written
            if b is not None:
                assert torch.equal(torch.isnan(t), torch.isnan(b))
                assert torch.equal(t[~torch.isnan(t)], b[~torch.isnan(b)])

    def setk(name, fn):
        return lambda kw: kw.__setitem__(name, fn(kw[name]))

    for corr, name in ((delta, 'delta'), (ctrl, 'ctrl_client')):   # [C, N]
        bad(corr, setk(name, lambda t: t.double()), name + ' must be')
        bad(corr, setk(name, lambda t: t.half()), name + ' must be')
        bad(corr, setk(name, lambda t: t[:-1].contiguous()),
            name + ' must be contiguous')
        bad(corr, setk(name, lambda t: t[:, :-64].contiguous()),
            name + ' must be contiguous')
        bad(corr, setk(name, lambda t: t[0].contiguous()),
            name + ' must be contiguous')
        bad(corr, setk(name, lambda t: t.t().contiguous().t()),
            name + ' must be contiguous')
        bad(corr, setk(name, lambda t: t.cpu()), 'GPU')
    name = 'ctrl_server'                                           # [N]
    bad(ctrl, setk(name, lambda t: t.double()), name + ' must be')
    bad(ctrl, setk(name, lambda t: t[:-1].contiguous()),
        name + ' must be contiguous')
    bad(ctrl, setk(name, lambda t: torch.stack([t] * 3)),
        name + ' must be contiguous')
    bad(ctrl, setk(name, lambda t: torch.stack([t, t], 1)[:, 0]),
        name + ' must be contiguous')
    bad(ctrl, setk(name, lambda t: t.cpu()), 'GPU')
    # half a pair, and both kinds of rows at once
    bad(ctrl, setk('ctrl_client', lambda t: None), 'come as a pair')
    bad(ctrl, setk('ctrl_server', lambda t: None), 'come as a pair')
    bad(ctrl, lambda kw: kw.__setitem__('delta', delta['delta'].cuda()),
        'delta and a control pair together')
    # the launcher's own pair check (an empty tensor is "absent")
    pos, kw = _args(case, lr, k_cut, hp, snap, wd_numel, ctrl)
    empty = torch.empty(0, device='cuda')
    flat = dict(kw)
    lay = ops._mlp_layout_flat(flat.pop('layout'))
    tail = (lay, flat['eps'], flat['wd_numel'], flat['weight_decay'],
            flat['momentum'], flat['dampening'], flat['nesterov'])
    with pytest.raises(RuntimeError, match='come as a pair, got only '
                       'ctrl_server'):
        ops._C.mlp_local_rounds(*pos, *tail, empty, kw['ctrl_server'], empty,
                                0.0)
    with pytest.raises(RuntimeError, match='delta and a control pair'):
        ops._C.mlp_local_rounds(*pos, *tail, delta['delta'].cuda(),
                                kw['ctrl_server'], kw['ctrl_client'], 0.0)
    torch.cuda.synchronize()
    assert torch.isnan(pos[6]).all()
    # prox_mu
    for mu in (-0.1, NAN, float('inf')):
        bad(cc.no_corr(), lambda kw, mu=mu: kw.__setitem__('prox_mu', mu),
            'prox_mu must be finite and >= 0')


def test_graph_capture_replays():
    case, lr, k_cut, hp, snap, wd_numel, corr, _r, _e = \
        cc.case(cc.SHAPES[1], 'ctrl')
    want = cc.call_op(ops, case, lr, k_cut, hp, snap, wd_numel, corr,
                      device='cuda')
    pos, kw = _args(case, lr, k_cut, hp, snap, wd_numel, corr)
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
# packed federations through ClientPack: the kernels against the slot loop
# --------------------------------------------------------------------------
# ftype -> (rounds, --manual_seed).  The seeds were searched on the CPU (the
# eager twin over the same model init, partitions and shuffles) for the ReLU
# precondition of mlpround_cases.case, which the test asserts.
FEDERATIONS = {'scaffold': (3, 424), 'fedgate': (3, 424), 'fedprox': (1, 8)}


def packed_federation(ftype, batched, monkeypatch, on_cuda=True, seed=None):
    """the arguments of test_gpu_mlpround._packed_round with the federated
    type, both MLP flags on or both off"""
    from fedtorch_amd.parameters import get_args
    from fedtorch_amd.nodes import Client
    rounds, seed0 = FEDERATIONS[ftype]
    seed = seed0 if seed is None else seed
    monkeypatch.setattr(multiclient, '_BATCHED_MLP_ENABLED', batched)
    monkeypatch.setattr(multiclient, '_BATCHED_MLP_CORR_ENABLED', batched)
    os.environ['FEDTORCH_SYNTH_SIZE'] = '200'
    torch.manual_seed(5)
    np.random.seed(5)
    args = get_args([
        '-d', 'mnist', '-a', 'mlp', '--mlp_hidden_size', '40',
        '--mlp_num_layers', '2', '-f', 'true',
        '--federated_type', ftype, '--fedprox_mu', '0.5',
        '--num_comms', str(rounds),
        '--clients_per_rank', '4', '-b', '10', '--lr', '0.1',
        '--federated_sync_type', 'local_step', '--local_step', '3',
        '--online_client_rate', '1.0', '--in_momentum', 'true',
        '--in_momentum_factor', '0.9', '--weight_decay', '1e-3',
        '--stop_criteria', 'epoch', '--num_epochs', '8',
        '--on_cuda', 'true' if on_cuda else 'false', '-j', '0',
        '--manual_seed', str(seed),
        '--checkpoint', '/tmp/ft_mlpround_corr_gpu', '--debug', 'false'])
    client = Client(args, 0)
    client.initialize()
    client.initialize_dataset()
    client.load_local_dataset()
    client.gen_aux_models()
    pack = multiclient.ClientPack(client, 4)
    pack.build_loaders()
    if not on_cuda:
        # the seed search: the cached loaders the GPU run builds, on the CPU
        from fedtorch_amd.components.datasets.device_cache import \
            DeviceCachedLoader
        for j, old in enumerate(pack.train_loaders):
            pack.train_loaders[j] = DeviceCachedLoader(
                old.dataset, args.batch_size,
                seed=int(args.manual_seed) * 1000003 + pack.global_id(j) * 8191,
                shuffle=True, device='cpu')
    assert pack.mlp_batched_eligible() == batched, pack.mlp_batched_blockers()
    assert not pack.batched_eligible()
    return cc.run_federation(client, pack, monkeypatch, real_op=_REAL_OP)


@pytest.mark.parametrize('ftype', sorted(FEDERATIONS))
def test_packed_federation_kernels_against_slot_loop(ftype, monkeypatch):
    """C = 4, tau = 3, MLP 784-40-40-10 through real DeviceCachedLoaders,
    three rounds (fedprox: one): both flags on (the batched kernels with the
    correction term) against both off (the slot loop: library GEMMs,
    autograd, the fused SGD kernel with the correction armed).  Both are
    bounded, in server and delta / ctrl / c, against the float64 replay of
    the whole federation over the operands the batched rounds recorded, and
    so is their distance; the ReLU precondition of mlpround_cases.case is
    asserted for those operands."""
    with monkeypatch.context() as m:
        off = packed_federation(ftype, False, m)
    with monkeypatch.context() as m:
        on = packed_federation(ftype, True, m)
    torch.cuda.synchronize()
    rounds = FEDERATIONS[ftype][0]
    assert len(off['calls']) == 0 and len(on['calls']) == rounds
    assert off['local_index'] == on['local_index'] == rounds * 4 * 3
    for r, (pos, kw) in enumerate(on['calls']):
        assert pos[2].shape == (4, 3, 10) and pos[3].tolist() == [3, 3, 3, 3]
        given = sorted(n for n in ('delta', 'ctrl_server', 'ctrl_client')
                       if kw.get(n) is not None)
        assert given == dict(fedprox=[], fedgate=['delta'],
                             scaffold=['ctrl_client', 'ctrl_server'])[ftype]
        assert (kw.get('prox_mu', 0.0) != 0) == (ftype == 'fedprox')
        for n in given:                    # live from the second round on
            assert bool(kw[n].any()) == (r > 0), (n, r)
    cc.assert_federations_agree(off, on, on, ftype)
