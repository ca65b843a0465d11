# -*- coding: utf-8 -*-
"""ops.linear_local_rounds without a GPU: the float64 reference of
linround_cases.py against autograd, the exact cases' precondition, the eager
twin against the reference, DeviceCachedLoader.index_batches, the
eligibility rules of ClientPack.batched_eligible, and a packed federation
trained once through the slot loop and once through the batched round."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import linround_cases as lc
import fedtorch_amd.ops as ops
from fedtorch_amd.components.datasets.device_cache import DeviceCachedLoader
from fedtorch_amd.parallel import multiclient

F32, F64 = torch.float32, torch.float64


# --------------------------------------------------------------------------
# the reference itself
# --------------------------------------------------------------------------
def _autograd_rounds(case, lr, hp):
    """nn.Linear + the loss modules + a hand-written copy of the fused-SGD
    twin's local branch, in float64; returns (replicas, in_mom, loss) of the
    online clients"""
    K, F = case['K'], case['X'].shape[1]
    w_off, b_off = case['w_off'], case['b_off']
    crit = nn.CrossEntropyLoss(reduction='mean') if case['loss_kind'] == 0 \
        else nn.MSELoss(reduction='mean')
    res = {}
    for c in range(len(case['steps'])):
        ns = int(case['steps'][c])
        if ns == 0:
            continue
        lin = nn.Linear(F, K).double()
        srv = case['server'].double()
        lin.weight.data.copy_(srv[w_off:w_off + K * F].view(K, F))
        lin.bias.data.copy_(srv[b_off:b_off + K])
        bufs = None
        if hp['m'] != 0:
            mo = case['in_mom'][c].double()
            bufs = [mo[w_off:w_off + K * F].view(K, F).clone(),
                    mo[b_off:b_off + K].clone()]
        init = bool(case['mom_init'][c])
        losses = []
        for s in range(ns):
            rows = case['idx'][c, s]
            rows = rows[rows >= 0].long()
            x = case['X'][rows].double()
            if case['loss_kind'] == 0:
                y = case['Y'][rows].long()
            else:
                y = case['Y'][rows].double().unsqueeze(1)
            lin.zero_grad()
            loss = crit(lin(x), y)
            loss.backward()
            losses.append(loss.item())
            for i, p in enumerate(lin.parameters()):
                d = p.grad.clone()
                if hp['wd'] != 0:
                    d.add_(p.data, alpha=hp['wd'])
                if hp['m'] != 0:
                    if not init:
                        bufs[i].copy_(d)
                    else:
                        bufs[i].mul_(hp['m']).add_(d, alpha=1 - hp['damp'])
                    d = d.add(bufs[i], alpha=hp['m']) if hp['nesterov'] \
                        else bufs[i].clone()
                p.data.add_(d, alpha=-float(lr[c, s]))
            init = True
        res[c] = (lin.weight.data.clone(), lin.bias.data.clone(), bufs,
                  losses)
    return res


@pytest.mark.parametrize('hp', [
    dict(wd=0.0, m=0.0, damp=0.0, nesterov=False),
    dict(wd=1e-2, m=0.9, damp=0.0, nesterov=False),
    dict(wd=1e-2, m=0.9, damp=0.0, nesterov=True),
    dict(wd=0.0, m=0.5, damp=0.25, nesterov=False)])
@pytest.mark.parametrize('loss_kind,K', [(0, 5), (1, 1)])
def test_reference_matches_autograd(loss_kind, K, hp):
    F, B, C, tau = 13, 6, 3, 4
    g = lc.gen('autograd', loss_kind, K)
    case = lc.make_case(g, F, K, B, C, tau, 40, loss_kind, [tau, 0, tau - 1],
                        integer=False, m=hp['m'])
    lr = torch.rand(C, tau, generator=g) * .1 + .05
    ref = lc._run_ref(case, lr, 0, hp)
    auto = _autograd_rounds(case, lr, hp)
    w, b = case['w_off'], case['b_off']
    for c, (W, bias, bufs, losses) in auto.items():
        r = ref['replicas'][c]
        assert torch.allclose(r[w:w + K * F].view(K, F), W, rtol=0,
                              atol=1e-13)
        assert torch.allclose(r[b:b + K], bias, rtol=0, atol=1e-13)
        if bufs is not None:
            mo = ref['in_mom'][c]
            assert torch.allclose(mo[w:w + K * F].view(K, F), bufs[0],
                                  rtol=0, atol=1e-13)
            assert torch.allclose(mo[b:b + K], bufs[1], rtol=0, atol=1e-13)
        n = len(losses)
        assert torch.allclose(ref['loss'][c, :n], torch.tensor(losses,
                              dtype=F64), rtol=0, atol=1e-13)
        assert not ref['loss'][c, n:].any()


@pytest.mark.parametrize('F,B,C,tau,lr_exp,wd,m', lc.EXACT_LS)
def test_exact_ls_cases_hold_in_fp32(F, B, C, tau, lr_exp, wd, m):
    """exact_case asserts the precondition; then the same loop in fp32 on
    the CPU must give the float64 result bit for bit"""
    case, lr, k_cut, hp, snap, ref = lc.exact_case(F, B, C, tau, lr_exp, wd,
                                                   m)
    r32 = lc._run_ref(case, lr, k_cut, hp, dtype=F32, snap=snap)
    for k in ('replicas', 'in_mom', 'snap', 'loss'):
        if ref[k] is None:
            continue
        assert r32[k].dtype == F32
        assert torch.equal(r32[k].double(), ref[k]) or (
            lc.same_nan_pattern(r32[k], ref[k])
            and lc.err(r32[k], ref[k]) == 0.0), k


@pytest.mark.parametrize('F,B,C,lr_exp,m', lc.EXACT_CE)
def test_exact_ce_cases_hold_in_fp32(F, B, C, lr_exp, m):
    case, lr, k_cut, hp, snap, ref = lc.exact_case(F, B, C, 1, lr_exp, 0.0,
                                                   m, loss_kind=0)
    r32 = lc._run_ref(case, lr, k_cut, hp, dtype=F32, snap=snap)
    for k in ('replicas', 'in_mom', 'snap'):
        if ref[k] is not None:
            assert lc.same_nan_pattern(r32[k], ref[k]), k
            assert lc.err(r32[k], ref[k]) == 0.0, k


# --------------------------------------------------------------------------
# the eager twin against the reference
# --------------------------------------------------------------------------
def _assert_exact(got, ref):
    for k in ('replicas', 'in_mom', 'snap'):
        if ref[k] is None:
            continue
        # NaN prefill: rows of offline clients, and snap rows not written
        assert lc.same_nan_pattern(got[k], ref[k]), k
        assert lc.err(got[k], ref[k]) == 0.0, k
    assert torch.equal(got['mom_init'].cpu(), ref['mom_init'])


@pytest.mark.parametrize('F,B,C,tau,lr_exp,wd,m', lc.EXACT_LS)
def test_twin_exact_ls(F, B, C, tau, lr_exp, wd, m):
    case, lr, k_cut, hp, snap, ref = lc.exact_case(F, B, C, tau, lr_exp, wd,
                                                   m)
    got = lc.call_op(ops, case, lr, k_cut, hp, snap)
    _assert_exact(got, ref)
    assert torch.equal(got['loss'].double(), ref['loss'])


def test_twin_offline_padding_mom_init_and_loss():
    """one offline client (its rows of replicas / in_mom / mom_init and the
    NaN-prefilled snap untouched), a short last batch, mom_init that differs
    between clients, per-step loss"""
    loss_kind, K, F, B, C, tau = 0, 10, 60, 16, 3, 3
    case, lr, k_cut, hp, snap, ref, e32 = lc.random_case(loss_kind, K, F, B,
                                                         C, tau)
    assert int(case['steps'][1]) == 0 and (case['idx'][0, tau - 1] < 0).any()
    assert case['mom_init'].tolist() == [0, 1, 0]
    got = lc.call_op(ops, case, lr, k_cut, hp, snap)
    # offline client 1: nothing written
    assert torch.isnan(got['replicas'][1]).all()
    assert torch.isnan(got['snap'][1]).all()
    assert torch.equal(got['in_mom'][1], case['in_mom'][1])
    assert got['mom_init'].tolist() == [1, 1, 1]
    assert not got['loss'][1].any()
    for k in ('replicas', 'in_mom', 'snap', 'loss'):
        assert lc.same_nan_pattern(got[k], ref[k]), k
        scale = ref[k][~torch.isnan(ref[k])].abs().max().item()
        assert lc.err(got[k], ref[k]) <= lc.bound(e32[k], scale), k
    # pad gaps: server's in replicas / snap, the old ones in in_mom
    gap = torch.ones(case['N'], dtype=torch.bool)
    gap[case['w_off']:case['w_off'] + K * F] = False
    gap[case['b_off']:case['b_off'] + K] = False
    for c in (0, 2):
        assert torch.equal(got['replicas'][c][gap], case['server'][gap])
        assert torch.equal(got['snap'][c][gap], case['server'][gap])
        assert torch.equal(got['in_mom'][c][gap], case['in_mom'][c][gap])


@pytest.mark.parametrize('which', ['first', 'last', 'beyond', 'off'])
def test_twin_k_cut(which):
    F, B, C, tau, lr_exp, wd, m = lc.EXACT_LS[2]
    case, lr, _k, hp, snap, _ref = lc.exact_case(F, B, C, tau, lr_exp, wd, m)
    k_cut = dict(first=1, last=tau, beyond=tau + 1, off=0)[which]
    ref = lc._run_ref(case, lr, k_cut, hp, snap=snap)
    got = lc.call_op(ops, case, lr, k_cut, hp, snap)
    _assert_exact(got, ref)
    steps = case['steps'].tolist()
    for c in range(C):
        written = not bool(torch.isnan(got['snap'][c]).any())
        assert written == (1 <= k_cut <= steps[c]), (c, k_cut, steps[c])
        if written and k_cut == 1:
            assert torch.equal(got['snap'][c], case['server'])


def test_limits_exported():
    assert ops.linear_round_max_floats(False) == ops.LINROUND_LDS_FLOATS
    assert ops.linear_round_max_floats(True) == ops.LINROUND_LDS_FLOATS // 2
    # MNIST logistic regression with momentum fits, CIFAR-10 only without
    assert ops.linear_round_lds_floats(784, 10, 50, True) \
        <= ops.LINROUND_LDS_FLOATS
    assert ops.linear_round_lds_floats(3072, 10, 50, False) \
        <= ops.LINROUND_LDS_FLOATS
    assert ops.linear_round_lds_floats(3072, 10, 50, True) \
        > ops.LINROUND_LDS_FLOATS


# --------------------------------------------------------------------------
# DeviceCachedLoader.index_batches
# --------------------------------------------------------------------------
def _dataset(n, shape=(3,), transform=None):
    from fedtorch_amd.components.datasets.sources import ArrayDataset
    g = lc.gen('ds', n)
    return ArrayDataset(torch.randn((n,) + shape, generator=g),
                        torch.randint(0, 5, (n,), generator=g),
                        transform=transform)


def _old_iter(ld):
    """DeviceCachedLoader.__iter__ as it was before index_batches"""
    n = len(ld.x)
    if ld.shuffle:
        perm = torch.randperm(n, generator=ld._gen).to(ld._device)
    else:
        perm = None
    for b in range(ld._nb):
        sl = slice(b * ld.batch_size, min((b + 1) * ld.batch_size, n))
        if perm is not None:
            ii = perm[sl]
            xb, yb = ld.x[ii], ld.y[ii]
        else:
            xb, yb = ld.x[sl], ld.y[sl]
        if ld._aug:
            xb = ld._augment(xb)
        yield xb, yb


@pytest.mark.parametrize('drop_last', [False, True])
@pytest.mark.parametrize('shuffle', [False, True])
def test_index_batches_match_iter(shuffle, drop_last):
    ds = _dataset(23)
    mk = lambda: DeviceCachedLoader(ds, 5, seed=11, shuffle=shuffle,  # noqa
                                    drop_last=drop_last, device='cpu')
    a, b, c = mk(), mk(), mk()
    for _epoch in range(2):
        batches = list(a)
        plan = list(b.index_batches())
        old = list(_old_iter(c))
        assert len(batches) == len(plan) == len(old) == len(a)
        for (xb, yb), ii, (xo, yo) in zip(batches, plan, old):
            assert ii.dtype == torch.int64
            assert torch.equal(xb, a.x[ii]) and torch.equal(yb, a.y[ii])
            assert torch.equal(xb, xo) and torch.equal(yb, yo)
        assert torch.equal(a._gen.get_state(), b._gen.get_state())
        assert torch.equal(a._gen.get_state(), c._gen.get_state())
    # an abandoned epoch draws one permutation, like a `break` in the loop
    next(iter(a)), next(b.index_batches(device='cpu')), next(_old_iter(c))
    assert torch.equal(a._gen.get_state(), b._gen.get_state())
    assert torch.equal(a._gen.get_state(), c._gen.get_state())


def test_iter_augment_branch_unchanged():
    from fedtorch_amd.components.datasets.sources import \
        _cifar_train_transform
    ds = _dataset(10, (3, 32, 32), _cifar_train_transform)
    a = DeviceCachedLoader(ds, 4, seed=3, shuffle=True, device='cpu')
    c = DeviceCachedLoader(ds, 4, seed=3, shuffle=True, device='cpu')
    assert a._aug
    for (xb, yb), (xo, yo) in zip(a, _old_iter(c)):
        assert torch.equal(xb, xo) and torch.equal(yb, yo)
    assert torch.equal(a._gen.get_state(), c._gen.get_state())


# --------------------------------------------------------------------------
# a packed federation on the CPU
# --------------------------------------------------------------------------
def _federation(extra=(), arch='logistic_regression', data='mnist',
                cached=True):
    os.environ['FEDTORCH_SYNTH_SIZE'] = '200'
    from fedtorch_amd.parameters import get_args
    from fedtorch_amd.nodes import Client
    args = get_args([
        '-d', data, '-a', arch, '-f', 'true',
        '--federated_type', 'fedavg', '--num_comms', '2',
        '--clients_per_rank', '4', '-b', '10', '--lr', '0.1',
        '--federated_sync_type', 'local_step', '--local_step', '3',
        '--online_client_rate', '0.75', '--in_momentum', 'true',
        '--in_momentum_factor', '0.9', '--weight_decay', '1e-3',
        '--lr_schedule_scheme', 'custom_multistep',
        '--lr_change_epochs', '1,2', '--lr_decay', '2',
        '--stop_criteria', 'epoch', '--num_epochs', '8',
        '--on_cuda', 'false', '-j', '0', '--manual_seed', '7',
        '--checkpoint', '/tmp/ft_linround', '--debug', 'false']
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
                old.dataset, client.args.batch_size, seed=100 + j,
                shuffle=True, device='cpu')
    return client, pack


@pytest.fixture
def flag(monkeypatch):
    monkeypatch.setattr(multiclient, '_BATCHED_ENABLED', True)


def test_batched_eligible_truth_table(flag, monkeypatch):
    client, pack = _federation()
    assert pack.batched_blockers() == [] and pack.batched_eligible()
    w_off, b_off, K, F = pack.linear_layout()
    assert (K, F) == (10, 784)
    assert client.arena.flat[w_off:w_off + K * F].data_ptr() \
        == client.model.fc.weight.data_ptr()
    assert client.arena.flat[b_off:b_off + K].data_ptr() \
        == client.model.fc.bias.data_ptr()

    def blocked(**kw):
        return not pack.batched_eligible()

    with monkeypatch.context() as m:       # the flag
        m.setattr(multiclient, '_BATCHED_ENABLED', False)
        assert blocked()
    for name, value in (('federated_type', 'fedprox'),
                        ('federated_sync_type', 'epoch'),
                        ('growing_batch_size', True), ('bf16', True)):
        with monkeypatch.context() as m:
            m.setattr(client.args, name, value, raising=False)
            assert blocked(), name
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
    with monkeypatch.context() as m:       # augmentation
        m.setattr(pack.train_loaders[2], '_aug', True)
        assert blocked()
    with monkeypatch.context() as m:       # not a DeviceCachedLoader
        loaders = list(pack.train_loaders)
        loaders[1] = [(None, None)]
        m.setattr(pack, 'train_loaders', loaders)
        assert blocked()
    with monkeypatch.context() as m:       # a 1-sample last batch
        ld = pack.train_loaders[0]
        n = len(ld.x) // ld.batch_size * ld.batch_size + 1
        m.setattr(ld, 'x', torch.zeros(n, 784))
        assert blocked()
    with monkeypatch.context() as m:       # over the LDS limit
        m.setattr(ops, 'LINROUND_LDS_FLOATS', 784 * 11)
        assert blocked()
    assert pack.batched_eligible()
    # robust variant / another model family
    _c, rpack = _federation(arch='robust_logistic_regression')
    assert rpack.linear_layout() is None and not rpack.batched_eligible()
    # plain DataLoaders (no device cache)
    _c, dpack = _federation(cached=False)
    assert not dpack.batched_eligible()


def _train(batched, extra, monkeypatch):
    from fedtorch_amd.trainings.packed import \
        train_and_validate_federated_packed
    monkeypatch.setattr(multiclient, '_BATCHED_ENABLED', batched)
    torch.manual_seed(5)
    np.random.seed(5)
    client, pack = _federation(extra)
    assert pack.batched_eligible() == batched
    calls = []
    real = ops.linear_local_rounds
    monkeypatch.setattr(ops, 'linear_local_rounds',
                        lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    torch.manual_seed(6)
    np.random.seed(6)
    train_and_validate_federated_packed(client, pack)
    a = client.args
    return dict(server=client.model_server.clone(),
                replicas=pack.replicas.clone(), in_mom=pack.in_mom.clone(),
                mom_init=list(pack.mom_init), local_index=a.local_index,
                epoch_=a.epoch_, seen=a.local_data_seen,
                lr=a.old_learning_rate, calls=len(calls),
                gens=[l._gen.get_state() for l in pack.train_loaders])


@pytest.mark.parametrize('drfa', [False, True])
def test_trajectory_batched_equals_slot_loop(drfa, monkeypatch):
    """C = 4 with one client offline per round, tau = 3, 2 rounds, momentum
    0.9, weight decay, a multistep lr change inside the run; then DRFA.

    torch.equal throughout: on the CPU the batched round runs the eager
    twin, which performs the slot loop's torch ops in the slot loop's order
    (F.linear, the loss functional, autograd's backward into a zeroed flat
    gradient, fused_sgd_step's eager branch over the whole arena row); the
    arena's pad gaps are zero, so putting them back changes nothing."""
    extra = ['--federated_drfa', 'true'] if drfa else []
    slot = _train(False, extra, monkeypatch)
    bat = _train(True, extra, monkeypatch)
    assert slot['calls'] == 0 and bat['calls'] == 2     # one per round
    assert slot['local_index'] == bat['local_index'] == 2 * 3 * 3
    assert slot['epoch_'] == bat['epoch_'] and slot['seen'] == bat['seen']
    assert slot['lr'] == bat['lr'] and slot['lr'] < 0.1   # the lr changed
    assert slot['mom_init'] == bat['mom_init']
    for k in ('server', 'replicas', 'in_mom'):
        assert torch.equal(slot[k], bat[k]), k
    assert slot['server'].abs().max() > 0
    for g0, g1 in zip(slot['gens'], bat['gens']):
        assert torch.equal(g0, g1)
