# -*- coding: utf-8 -*-
"""ops.mlp_local_rounds without a GPU: the eager twin against the float64
replay of mlpround_cases.py and against the real MLP module driven by
autograd and the fused optimizer, untouched rows and pad gaps, the twin's
errors, the eligibility rules of ClientPack.mlp_batched_eligible, and a
packed MLP federation trained once through the slot loop and once through
the batched round, both against a float64 replay."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import linround_cases as lc
import mlpround_cases as mc
import fedtorch_amd.ops as ops
from fedtorch_amd.components.datasets.device_cache import DeviceCachedLoader
from fedtorch_amd.parallel import multiclient

F32, F64 = torch.float32, torch.float64


def _assert_bounded(got, ref, e32, label=''):
    assert torch.equal(got['mom_init'].cpu(), ref['mom_init'])
    for k in mc.OUTPUTS:
        if ref[k] is None:
            assert got[k] is None or got[k].numel() == 0
            continue
        assert lc.same_nan_pattern(got[k], ref[k]), k
        e, tol = lc.err(got[k], ref[k]), lc.bound(e32[k], mc.scale_of(ref[k]))
        print('%s %s: err %.3e  e32 %.3e  err/e32 %.2f  err/tol %.3f'
              % (label, k, e, e32[k], e / e32[k] if e32[k] else 0.0, e / tol))
        assert e <= tol, (k, e, tol)


# --------------------------------------------------------------------------
# the eager twin against the float64 replay
# --------------------------------------------------------------------------
@pytest.mark.parametrize('shape', mc.SHAPES)
def test_twin_against_float64_replay(shape):
    case, lr, k_cut, hp, snap, wd_numel, ref, e32 = mc.case(*shape)
    got = mc.call_op(ops, case, lr, k_cut, hp, snap, wd_numel)
    _assert_bounded(got, ref, e32, str(shape))
    steps = case['steps'].tolist()
    for c in range(len(steps)):                 # snap: only when k_cut is due
        written = not bool(torch.isnan(got['snap'][c]).any())
        assert written == (1 <= k_cut <= steps[c]), (c, k_cut, steps[c])
    assert not got['loss'][1].any() and not got['loss'][2, 2:].any()
    assert (got['loss'][0] > 0).all()


def test_case_set_covers_the_edges():
    ks = [mc.case(*s) for s in mc.SHAPES]
    assert all(k[0]['steps'].tolist() == [3, 0, 2] for k in ks)
    valid = [sorted({int((k[0]['idx'][c, s] >= 0).sum())
                     for c in (0, 2) for s in range(mc.STEPS[c])})
             for k in ks]
    assert valid == [[3, 5], [2, 16], [17, 50]]
    assert [k[3]['m'] for k in ks] == [0.0, 0.9, 0.9]
    assert [k[3]['nesterov'] for k in ks] == [False, True, False]
    assert [k[3]['wd'] for k in ks] == [0.0, 5e-4, 5e-4]
    assert ks[1][5] < ks[1][0]['N'] and ks[2][5] == ks[2][0]['N']
    assert ks[1][0]['mom_init'].tolist() == [0, 1, 1]
    assert ks[2][0]['mom_init'].tolist() == [1, 0, 0]
    assert [k[2] for k in ks] == [3, 3, 1]     # inside c0 / beyond c2; first
    assert all(len(set(k[1][0].tolist())) == 3 for k in ks)   # lr changes


# --------------------------------------------------------------------------
# the twin against the real module: autograd + FusedSGD.step, the slot loop's
# ops
# --------------------------------------------------------------------------
def _module_case():
    """(model, arena, case, lr, hp, wd_numel): the (14, 33, 2, 1, 5) shape in
    the layout of a real Arena over MLP('adult'); pad gaps zero as in a real
    arena"""
    from fedtorch_amd.components.models.mlp import MLP
    from fedtorch_amd.parallel.arena import Arena
    model = MLP('adult', 1, 33, 0.0)
    arena = Arena(model)
    off = lambda n: arena.offsets[arena.names.index(n)]  # noqa: E731
    layout = dict(blocks=[(off('layers.0.0.weight'), off('layers.0.0.bias'),
                           off('layers.0.1.weight'), off('layers.0.1.bias'),
                           14, 33)], head=(off('fc.weight'), 33, 2))
    g = lc.gen('mlp-module')
    case = mc.make_case(g, 14, 33, 2, 1, 5, mc.STEPS, 22, m=0.9,
                        layout=layout, N=arena.numel, short=(0, 2, 3),
                        mom_init=[0, 1, 1])
    gap = mc.gap_mask(layout, arena.numel)
    case['server'][gap] = 0
    case['in_mom'][:, gap] = 0
    lr = torch.rand(3, 3, generator=g) * .05 + .01
    hp = dict(wd=5e-4, m=0.9, damp=0.0, nesterov=False)
    return model, arena, case, lr, hp, arena.wd_numel


def test_twin_against_the_real_module():
    from fedtorch_amd.components.optim.sgd import FusedSGD
    model, arena, case, lr, hp, wd_numel = _module_case()
    # the stock MLP's BatchNorm parameters are decayed like the rest
    assert wd_numel == arena.numel
    ref, r32, lo, e = mc.relu_margin(case, lr, 0, hp, None, wd_numel)
    assert lo > mc.MARGIN * e, (lo, e)
    e32 = {k: lc.err(r32[k], ref[k]) for k in ('replicas', 'in_mom', 'loss')}
    e32['snap'] = None
    twin = mc.call_op(ops, case, lr, 0, hp, None, wd_numel)
    _assert_bounded(twin, ref, e32, 'twin')

    opt = FusedSGD(arena, lr=0.1, in_momentum=0.9, weight_decay=hp['wd'])
    crit = nn.CrossEntropyLoss()
    mod = dict(replicas=case['replicas'].clone(),
               in_mom=case['in_mom'].clone(),
               mom_init=case['mom_init'].clone(), snap=None,
               loss=torch.zeros(3, 3))
    model.train()
    for c, ns in enumerate(mc.STEPS):
        if ns == 0:
            continue
        arena.load_flat(case['server'])
        opt.bind_state(in_buf=mod['in_mom'][c],
                       in_init=bool(case['mom_init'][c]))
        for s in range(ns):
            rows = case['idx'][c, s]
            rows = rows[rows >= 0].long()
            opt.zero_grad()
            loss = crit(model(case['X'][rows]), case['Y'][rows].long())
            loss.backward()
            opt.param_groups[0]['lr'] = float(lr[c, s])
            opt.step(apply_lr=True, apply_in_momentum=True,
                     apply_out_momentum=False)
            mod['loss'][c, s] = loss.item()
        mod['replicas'][c].copy_(arena.flat)
        mod['mom_init'][c] = 1
    _assert_bounded(mod, ref, e32, 'module')
    for k in ('replicas', 'in_mom', 'loss'):
        d = lc.err(twin[k], mod[k].double())
        assert d <= lc.bound(e32[k], mc.scale_of(ref[k])), (k, d)


# --------------------------------------------------------------------------
# what must stay untouched
# --------------------------------------------------------------------------
def test_offline_rows_and_pad_gaps_bit_untouched():
    case, lr, k_cut, hp, snap, wd_numel, _ref, _e = mc.case(*mc.SHAPES[1])
    got = mc.call_op(ops, case, lr, k_cut, hp, snap, wd_numel)
    # offline client 1: nothing written (NaN prefill, old momentum, flag)
    assert torch.isnan(got['replicas'][1]).all()
    assert torch.isnan(got['snap'][1]).all()
    assert torch.equal(got['in_mom'][1], case['in_mom'][1])
    assert case['mom_init'].tolist() == [0, 1, 1]
    assert got['mom_init'].tolist() == [1, 1, 1]
    assert not got['loss'][1].any()
    gap = mc.gap_mask(case['layout'], case['N'])
    assert gap.sum() > 64
    for c in (0, 2):
        assert torch.equal(got['replicas'][c][gap], case['server'][gap])
        assert torch.equal(got['in_mom'][c][gap], case['in_mom'][c][gap])
        assert not torch.equal(got['in_mom'][c][~gap],
                               case['in_mom'][c][~gap])
    assert torch.equal(got['snap'][0][gap], case['server'][gap])
    # without momentum neither in_mom nor mom_init is touched
    case, lr, k_cut, hp, snap, wd_numel, _ref, _e = mc.case(*mc.SHAPES[0])
    got = mc.call_op(ops, case, lr, k_cut, hp, snap, wd_numel)
    assert got['in_mom'] is None and got['mom_init'].tolist() == [0, 0, 0]


# --------------------------------------------------------------------------
# the twin's errors
# --------------------------------------------------------------------------
def _twin_raises(match, mutate):
    case, lr, k_cut, hp, snap, wd_numel, _ref, _e = mc.case(*mc.SHAPES[0])
    case = dict(case, idx=case['idx'].clone(),
                layout=dict(blocks=list(case['layout']['blocks']),
                            head=case['layout']['head']))
    mutate(case)
    with pytest.raises(ValueError, match=match):
        mc.call_op(ops, case, lr, k_cut, hp, snap, wd_numel)


def test_twin_raises_on_short_batches_and_bad_layouts():
    def one_row(case):
        case['idx'][2, 1, 1:] = -1
    _twin_raises('fewer than 2 samples', one_row)

    def blk(i, v):
        def mutate(case):
            b = list(case['layout']['blocks'][0])
            b[i] = v
            case['layout']['blocks'][0] = tuple(b)
        return mutate
    _twin_raises('overlap', blk(1, 64))               # bias inside the weight
    _twin_raises('does not fit', blk(2, 10 ** 6))     # gamma past the arena
    _twin_raises('input has 14 features', blk(4, 15))  # in != F
    _twin_raises('a layout block is',
                 lambda case: case['layout']['blocks'].__setitem__(
                     0, case['layout']['blocks'][0][:5]))

    def head(v):
        return lambda case: case['layout'].__setitem__('head', v)
    _twin_raises('head reads 32 features', head((2304, 32, 2)))
    _twin_raises('unsupported K=129', head((2304, 33, 129)))
    _twin_raises('layout has 0 blocks',
                 lambda case: case['layout'].__setitem__('blocks', []))


def test_limits_exported():
    assert ops.mlp_round_max_batch() == ops.MLPROUND_MAXB == 64
    assert ops.mlp_round_max_classes() == ops.MLPROUND_MAXK == 128


# --------------------------------------------------------------------------
# a packed federation on the CPU
# --------------------------------------------------------------------------
def _federation(extra=(), arch='mlp', cached=True, batch='10', seed=1):
    os.environ['FEDTORCH_SYNTH_SIZE'] = '200'
    from fedtorch_amd.parameters import get_args
    from fedtorch_amd.nodes import Client
    args = get_args([
        '-d', 'mnist', '-a', arch, '--mlp_hidden_size', '24',
        '--mlp_num_layers', '2', '-f', 'true',
        '--federated_type', 'fedavg', '--num_comms', '3',
        '--clients_per_rank', '4', '-b', batch, '--lr', '0.1',
        '--federated_sync_type', 'local_step', '--local_step', '3',
        '--online_client_rate', '0.75', '--in_momentum', 'true',
        '--in_momentum_factor', '0.9', '--weight_decay', '1e-3',
        '--lr_schedule_scheme', 'custom_multistep',
        '--lr_change_epochs', '1,2', '--lr_decay', '2',
        '--stop_criteria', 'epoch', '--num_epochs', '8',
        '--on_cuda', 'false', '-j', '0', '--manual_seed', '7',
        '--checkpoint', '/tmp/ft_mlpround', '--debug', 'false']
        + list(extra))
    client = Client(args, 0)
    client.initialize()
    client.initialize_dataset()
    client.load_local_dataset()
    client.gen_aux_models()
    pack = multiclient.ClientPack(client, 4)
    pack.build_loaders()
    if cached:
        for j, old in enumerate(pack.train_loaders):
            pack.train_loaders[j] = DeviceCachedLoader(
                old.dataset, client.args.batch_size, seed=100 * seed + j,
                shuffle=True, device='cpu')
    return client, pack


@pytest.fixture
def flag(monkeypatch):
    monkeypatch.setattr(multiclient, '_BATCHED_MLP_ENABLED', True)


def test_mlp_batched_eligible_truth_table(flag, monkeypatch):
    client, pack = _federation()
    assert pack.mlp_batched_blockers() == [] and pack.mlp_batched_eligible()
    # the linear path does not take an MLP, whatever its flag says
    assert pack.linear_layout() is None and not pack.batched_eligible()
    with monkeypatch.context() as m:
        m.setattr(multiclient, '_BATCHED_ENABLED', True)
        assert not pack.batched_eligible()
    layout = pack.mlp_layout()
    assert [b[4:] for b in layout['blocks']] == [(784, 24), (24, 24)]
    assert layout['head'][1:] == (24, 10) and pack.mlp_eps() == 1e-5
    flat, model = client.arena.flat, client.model
    for (w, b, g, be, fin, out), blk in zip(layout['blocks'], model.layers):
        assert flat[w:w + fin * out].data_ptr() == blk[0].weight.data_ptr()
        assert flat[b:b + out].data_ptr() == blk[0].bias.data_ptr()
        assert flat[g:g + out].data_ptr() == blk[1].weight.data_ptr()
        assert flat[be:be + out].data_ptr() == blk[1].bias.data_ptr()
    assert flat[layout['head'][0]:].data_ptr() == model.fc.weight.data_ptr()

    def blocked():
        return not pack.mlp_batched_eligible()

    with monkeypatch.context() as m:       # the flag
        m.setattr(multiclient, '_BATCHED_MLP_ENABLED', False)
        assert pack.mlp_batched_blockers() == [
            'FEDTORCH_PACKED_BATCHED_MLP is not set']
    for name, value in (('federated_type', 'fedprox'),
                        ('federated_type', 'scaffold'),
                        ('federated_type', 'fedgate'),
                        ('federated_sync_type', 'epoch'),
                        ('growing_batch_size', True), ('bf16', True)):
        with monkeypatch.context() as m:
            m.setattr(client.args, name, value, raising=False)
            assert blocked(), name
    with monkeypatch.context() as m:       # DRFA over fedavg is allowed
        m.setattr(client.args, 'federated_drfa', True, raising=False)
        assert not blocked()
    with monkeypatch.context() as m:       # a correction on the optimizer
        m.setattr(client.optimizer, '_prox_mu', 0.1)
        assert blocked()
    with monkeypatch.context() as m:
        m.setattr(client.optimizer, '_delta', client.arena.new_buffer())
        assert blocked()
    with monkeypatch.context() as m:       # a bf16 twin of the arena
        m.setattr(client.arena, 'half_flat',
                  client.arena.flat.to(torch.bfloat16))
        assert blocked()
    with monkeypatch.context() as m:       # noise (the robust variant)
        m.setattr(model, 'noise', torch.zeros(784))
        assert pack.mlp_layout() is None and blocked()
    with monkeypatch.context() as m:       # running statistics
        m.setattr(model.layers[1][1], 'track_running_stats', True)
        assert pack.mlp_layout() is None and blocked()
    with monkeypatch.context() as m:       # dropout
        m.setattr(model.layers[0][3], 'p', 0.5)
        assert pack.mlp_layout() is None and blocked()
    with monkeypatch.context() as m:       # a subclass is another model
        from fedtorch_amd.components.models.mlp import MLP
        m.setattr(model, '__class__', type('Other', (MLP,), {}))
        assert pack.mlp_layout() is None and blocked()
    with monkeypatch.context() as m:       # the arena holds other names
        names = list(client.arena.names)
        names[0] = 'other.weight'
        m.setattr(client.arena, 'names', names)
        assert blocked()
    with monkeypatch.context() as m:       # augmentation
        m.setattr(pack.train_loaders[2], '_aug', True)
        assert blocked()
    with monkeypatch.context() as m:       # not a DeviceCachedLoader
        loaders = list(pack.train_loaders)
        loaders[1] = [(None, None)]
        m.setattr(pack, 'train_loaders', loaders)
        assert blocked()
    with monkeypatch.context() as m:       # unequal batch sizes
        m.setattr(pack.train_loaders[3], 'batch_size', 5)
        assert blocked()
    for B in (1, 65):                      # B outside 2 .. 64
        with monkeypatch.context() as m:
            for ld in pack.train_loaders:
                m.setattr(ld, 'batch_size', B)
                m.setattr(ld, 'drop_last', True)
            assert any('batch size' in w for w in pack.mlp_batched_blockers())
    with monkeypatch.context() as m:       # a 1-sample last batch
        ld = pack.train_loaders[0]
        n = len(ld.x) // ld.batch_size * ld.batch_size + 1
        m.setattr(ld, 'x', torch.zeros(n, 784))
        assert blocked()
    with monkeypatch.context() as m:       # floating-point labels
        ld = pack.train_loaders[1]
        m.setattr(ld, 'y', ld.y.float())
        assert blocked()
    with monkeypatch.context() as m:       # more classes than the kernel has
        m.setattr(ops, 'MLPROUND_MAXK', 9)
        assert blocked()
    assert pack.mlp_batched_eligible()
    # the robust variant: noise and running statistics
    _c, rpack = _federation(arch='robust_mlp')
    assert rpack.mlp_layout() is None and not rpack.mlp_batched_eligible()
    # plain DataLoaders (no device cache)
    _c, dpack = _federation(cached=False)
    assert not dpack.mlp_batched_eligible()
    # a linear model is not an MLP
    _c, lpack = _federation(arch='logistic_regression')
    assert lpack.mlp_layout() is None
    assert lpack.mlp_batched_eligible() is False


def _train(batched, extra, monkeypatch, seed):
    """one packed federation of 3 rounds; returns the end state, the
    recorded operands of the batched calls and the weights of each round"""
    from fedtorch_amd.trainings.packed import \
        train_and_validate_federated_packed
    monkeypatch.setattr(multiclient, '_BATCHED_MLP_ENABLED', batched)
    torch.manual_seed(seed)
    np.random.seed(5)
    client, pack = _federation(extra, seed=seed)
    assert pack.mlp_batched_eligible() == batched, pack.mlp_batched_blockers()
    calls, weights = [], []
    real = ops.mlp_local_rounds

    def op(*a, **k):
        calls.append(([None if not torch.is_tensor(t) else t.clone()
                       for t in a], dict(k)))
        return real(*a, **k)
    monkeypatch.setattr(ops, 'mlp_local_rounds', op)
    lin = []
    monkeypatch.setattr(ops, 'linear_local_rounds',
                        lambda *a, **k: lin.append(1))
    real_acc = pack.accumulate_partial

    def acc(server, w):
        weights.append(list(w))
        return real_acc(server, w)
    monkeypatch.setattr(pack, 'accumulate_partial', acc)
    start = client.model_server.clone()
    torch.manual_seed(6)
    np.random.seed(6)
    train_and_validate_federated_packed(client, pack)
    a = client.args
    assert not lin and not a.out_momentum
    return dict(server=client.model_server.clone(),
                replicas=pack.replicas.clone(), in_mom=pack.in_mom.clone(),
                mom_init=list(pack.mom_init), local_index=a.local_index,
                epoch_=a.epoch_, seen=a.local_data_seen,
                lr=a.old_learning_rate, calls=calls, weights=weights,
                start=start, scale=a.lr_scale_at_sync,
                gens=[l._gen.get_state() for l in pack.train_loaders])


def _replay_federation(run, start, dtype, pre=None):
    """the federation over the recorded operands of the batched rounds, in
    `dtype`: local steps by mc.ref_rounds, then x -= scale * sum_j w_j
    (x - y_j) and the online clients adopt x"""
    server = start.to(dtype).clone()
    pos0 = run['calls'][0][0]
    replicas = pos0[6].to(dtype).clone()
    in_mom = pos0[7].to(dtype).clone()
    mom_init = pos0[8].clone()
    snap = None
    for (pos, kw), w in zip(run['calls'], run['weights']):
        X, Y, idx, steps, lr = pos[:5]
        has_snap = pos[9] is not None
        out = mc.ref_rounds(
            X, Y, idx, steps, lr, server, replicas, in_mom, mom_init,
            torch.zeros_like(replicas) if has_snap else None, pos[10]
            if has_snap else 0, kw['layout'], kw['eps'], kw['wd_numel'],
            kw['weight_decay'], kw['momentum'], kw['dampening'],
            kw['nesterov'], dtype=dtype, pre=pre)
        replicas, in_mom, mom_init = (out['replicas'], out['in_mom'],
                                      out['mom_init'])
        snap = out['snap']
        partial = torch.zeros_like(server)
        for j, wj in enumerate(w):
            partial += wj * (server - replicas[j])
        server = server - run['scale'] * partial
        for j, wj in enumerate(w):
            if wj != 0.0:
                replicas[j] = server
    return dict(server=server, replicas=replicas, in_mom=in_mom), snap


# seeds (model init and loader shuffles) for which the ReLU precondition of
# mlpround_cases.case holds over the run; searched on the CPU
FED_SEEDS = {False: 7, True: 13}


@pytest.mark.parametrize('drfa', [False, True])
def test_packed_mlp_federation_against_float64_replay(drfa, monkeypatch):
    """C = 4 with one client offline per round, tau = 3, 3 rounds, momentum
    0.9, weight decay, a multistep lr change inside the run; then DRFA over
    fedavg.  The slot loop (flag off) and the batched round (flag on: the
    eager twin here) both against the float64 replay of the operands the
    batched rounds recorded: at most 8x the fp32 replay's own error plus 16
    ulps of scale, and so is their mutual distance."""
    extra = ['--federated_drfa', 'true'] if drfa else []
    with monkeypatch.context() as m:
        slot = _train(False, extra, m, FED_SEEDS[drfa])
    with monkeypatch.context() as m:
        bat = _train(True, extra, m, FED_SEEDS[drfa])
    assert len(slot['calls']) == 0 and len(bat['calls']) == 3   # one a round
    assert slot['local_index'] == bat['local_index'] == 3 * 3 * 3
    assert slot['epoch_'] == bat['epoch_'] and slot['seen'] == bat['seen']
    assert slot['lr'] == bat['lr'] and slot['lr'] < 0.1   # the lr changed
    assert slot['mom_init'] == bat['mom_init']
    assert torch.equal(slot['start'], bat['start'])
    for g0, g1 in zip(slot['gens'], bat['gens']):
        assert torch.equal(g0, g1)
    for (pos, kw), w in zip(bat['calls'], bat['weights']):
        assert pos[3].tolist().count(3) == 3 and pos[3].tolist().count(0) == 1
        assert [x != 0 for x in w] == [s > 0 for s in pos[3].tolist()]
        assert (pos[9] is not None) == drfa
    for ws, wb in zip(slot['weights'], bat['weights']):
        assert np.allclose(ws, wb, rtol=1e-5, atol=0)
    p64, p32 = [], []
    r64, snap64 = _replay_federation(bat, bat['start'], F64, pre=p64)
    r32, _s = _replay_federation(bat, bat['start'], F32, pre=p32)
    # the precondition of mlpround_cases.case, for this run's operands
    lo = min(y.abs().min().item() for y in p64)
    e = max((a.double() - b).abs().max().item() for a, b in zip(p32, p64))
    assert lo > mc.MARGIN * e, (lo, e)
    for k in sorted(r64):
        e32 = lc.err(r32[k], r64[k])
        tol = lc.bound(e32, r64[k].abs().max().item())
        e_slot, e_bat = lc.err(slot[k], r64[k]), lc.err(bat[k], r64[k])
        d = (slot[k] - bat[k]).abs().max().item()
        print('%s: slot err %.3e  batched err %.3e  slot-batched %.3e  '
              'e32 %.3e  tol %.3e' % (k, e_slot, e_bat, d, e32, tol))
        assert e_slot <= tol, (k, e_slot, tol)
        assert e_bat <= tol, (k, e_bat, tol)
        assert d <= tol, (k, d, tol)
    assert lc.err(bat['server'], bat['start'].double()) > 1e-3   # it trained
