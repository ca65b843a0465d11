# -*- coding: utf-8 -*-
"""FedProx / SCAFFOLD / FedGATE for packed clients, without a GPU: the eager
twin of ops.linear_local_rounds with a gradient correction against the
float64 step loop, the two batched row ops, the eligibility rules of the
second opt-in, and packed federations on the CPU against a float64 replay of
the round structure (linround_corr_cases.replay_federation)."""
import multiprocessing as mp
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist

import linround_cases as lc
import linround_corr_cases as cc
import fedtorch_amd.ops as ops
from fedtorch_amd.components.datasets.device_cache import DeviceCachedLoader
from fedtorch_amd.parallel import multiclient

F64 = torch.float64


# --------------------------------------------------------------------------
# the eager twin against the float64 loop
# --------------------------------------------------------------------------
def _assert_exact(got, ref):
    for k in ('replicas', 'in_mom', 'snap'):
        if ref[k] is None:
            continue
        assert lc.same_nan_pattern(got[k], ref[k]), k
        assert lc.err(got[k], ref[k]) == 0.0, k
    assert torch.equal(got['mom_init'], ref['mom_init'])


@pytest.mark.parametrize('kind', cc.KINDS)
@pytest.mark.parametrize('F,B,tau,lr_exp,wd,m,mu', cc.EXACT_LS)
def test_twin_exact_ls(kind, F, B, tau, lr_exp, wd, m, mu):
    case, lr, k_cut, hp, snap, corr, ref = cc.exact_case(
        kind, F, B, tau, lr_exp, wd, m, mu)
    got = cc.call_op(ops, case, lr, k_cut, hp, snap, corr)
    _assert_exact(got, ref)
    assert torch.equal(got['loss'].double(), ref['loss'])
    # the correction took part
    plain = lc.call_op(ops, case, lr, k_cut, hp, snap)
    assert not torch.equal(plain['replicas'][0], got['replicas'][0])


@pytest.mark.parametrize('kind', cc.KINDS)
@pytest.mark.parametrize('F,B,lr_exp,m,mu', cc.EXACT_CE)
def test_twin_exact_ce_from_zero(kind, F, B, lr_exp, m, mu):
    case, lr, k_cut, hp, snap, corr, ref = cc.exact_case(
        kind, F, B, 1, lr_exp, 0.0, m, mu, loss_kind=0)
    got = cc.call_op(ops, case, lr, k_cut, hp, snap, corr)
    _assert_exact(got, ref)


@pytest.mark.parametrize('kind', cc.KINDS)
@pytest.mark.parametrize('loss_kind,K,F,B,C,tau', cc.RANDOM)
def test_twin_random(kind, loss_kind, K, F, B, C, tau):
    case, lr, k_cut, hp, snap, corr, ref, e32 = cc.random_case(
        kind, loss_kind, K, F, B, C, tau)
    got = cc.call_op(ops, case, lr, k_cut, hp, snap, corr)
    assert torch.equal(got['mom_init'], ref['mom_init'])
    for k in cc.OUTPUTS:
        assert lc.same_nan_pattern(got[k], ref[k]), k     # NaN rows unread
        scale = ref[k][~torch.isnan(ref[k])].abs().max().item()
        assert lc.err(got[k], ref[k]) <= lc.bound(e32[k], scale), k
    plain = lc.call_op(ops, case, lr, k_cut, hp, snap)
    assert (plain['replicas'][0] - got['replicas'][0]).abs().max() > 1e-4


def test_twin_rejects_bad_correction_sets():
    case, lr, k_cut, hp, snap, corr, _r, _e = cc.random_case('ctrl',
                                                             *cc.RANDOM[0])
    for bad, match in (
            (dict(corr, ctrl_client=None), 'pair'),
            (dict(corr, ctrl_server=None), 'pair'),
            (dict(corr, delta=corr['ctrl_client']), 'together')):
        with pytest.raises(RuntimeError, match=match):
            cc.call_op(ops, case, lr, k_cut, hp, snap, bad)


# --------------------------------------------------------------------------
# the two row ops
# --------------------------------------------------------------------------
@pytest.mark.parametrize('C,N', [(1, 64), (3, 192), (5, 1028)])
def test_row_ops_against_float64(C, N):
    t = cc.row_case(C, N)
    # FedGATE rows
    want, w32 = cc.ref_delta_rows(t), cc.ref_delta_rows(t, torch.float32)
    delta = t['state'].clone()
    ops.multi_delta_update(delta, t['server'], t['agg'], t['replicas'],
                           t['inv'])
    assert lc.same_nan_pattern(delta, want)        # offline rows untouched
    scale = want[~torch.isnan(want)].abs().max().item()
    assert lc.err(delta, want) <= lc.bound(lc.err(w32, want), scale)
    # SCAFFOLD rows
    (wc, wo), (c32, o32) = cc.ref_ctrl_rows(t), cc.ref_ctrl_rows(
        t, torch.float32)
    ctrl, out = t['state'].clone(), torch.full((N,), lc.NAN)
    ops.multi_scaffold_control_update(ctrl, t['ctrl_server'], t['server'],
                                      t['replicas'], t['inv'], t['weights'],
                                      out)
    assert lc.same_nan_pattern(ctrl, wc) and not torch.isnan(out).any()
    scale = wc[~torch.isnan(wc)].abs().max().item()
    assert lc.err(ctrl, wc) <= lc.bound(lc.err(c32, wc), scale)
    assert lc.err(out, wo) <= lc.bound(lc.err(o32, wo),
                                       wo.abs().max().item())


def test_row_ops_one_row_equal_the_single_row_ops():
    t = cc.row_case(1, 256, offline=())
    coef = float(t['inv'][0])
    a = t['state'].clone()
    ops.multi_delta_update(a, t['server'], t['agg'], t['replicas'], t['inv'])
    b = t['state'][0].clone()
    ops.delta_update(b, t['server'], t['agg'], t['replicas'][0], coef)
    assert torch.equal(a[0], b)
    ctrl, out = t['state'].clone(), torch.empty(256)
    ops.multi_scaffold_control_update(ctrl, t['ctrl_server'], t['server'],
                                      t['replicas'], t['inv'], t['weights'],
                                      out)
    new, diff = torch.empty(256), torch.empty(256)
    ops.scaffold_control_update(new, t['state'][0], t['ctrl_server'],
                                t['server'], t['replicas'][0], coef)
    ops.scaled_diff(new, t['state'][0], diff, float(t['weights'][0]))
    assert torch.equal(ctrl[0], new) and torch.equal(out, diff)


def test_row_ops_all_offline():
    t = cc.row_case(2, 64, offline=(0, 1))
    delta = t['state'].clone()
    ops.multi_delta_update(delta, t['server'], t['agg'], t['replicas'],
                           t['inv'])
    assert torch.isnan(delta).all()
    ctrl, out = t['state'].clone(), torch.full((64,), lc.NAN)
    ops.multi_scaffold_control_update(ctrl, t['ctrl_server'], t['server'],
                                      t['replicas'], t['inv'], t['weights'],
                                      out)
    assert torch.isnan(ctrl).all() and not out.any()


# --------------------------------------------------------------------------
# a packed federation on the CPU
# --------------------------------------------------------------------------
def _federation(extra=(), cached=True):
    os.environ['FEDTORCH_SYNTH_SIZE'] = '200'
    from fedtorch_amd.parameters import get_args
    from fedtorch_amd.nodes import Client
    args = get_args([
        '-d', 'mnist', '-a', 'logistic_regression', '-f', 'true',
        '--num_comms', '3',
        '--clients_per_rank', '4', '-b', '10', '--lr', '0.1',
        '--federated_sync_type', 'local_step', '--local_step', '3',
        '--online_client_rate', '0.75', '--in_momentum', 'true',
        '--in_momentum_factor', '0.9', '--weight_decay', '1e-3',
        '--lr_schedule_scheme', 'custom_multistep',
        '--lr_change_epochs', '1,2', '--lr_decay', '2',
        '--stop_criteria', 'epoch', '--num_epochs', '8',
        '--on_cuda', 'false', '-j', '0', '--manual_seed', '7',
        '--checkpoint', '/tmp/ft_linround_corr', '--debug', 'false']
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
def flags(monkeypatch):
    monkeypatch.setattr(multiclient, '_BATCHED_ENABLED', True)
    monkeypatch.setattr(multiclient, '_BATCHED_CORR_ENABLED', True)


@pytest.mark.parametrize('ftype', ['fedprox', 'scaffold', 'fedgate'])
def test_second_opt_in_truth_table(ftype, flags, monkeypatch):
    client, pack = _federation(['--federated_type', ftype])
    assert pack.batched_blockers() == [] and pack.batched_eligible()
    assert (pack.delta is not None) == (ftype == 'fedgate')
    assert (pack.ctrl is not None) == (ftype == 'scaffold')
    if pack.delta is not None:
        assert pack.delta.shape == pack.replicas.shape \
            and not pack.delta.any()
    if pack.ctrl is not None:
        assert pack.ctrl.shape == pack.replicas.shape and not pack.ctrl.any()
    with monkeypatch.context() as m:       # the second flag off: as before
        m.setattr(multiclient, '_BATCHED_CORR_ENABLED', False)
        assert pack.batched_blockers() == ['federated_type is not fedavg']
    with monkeypatch.context() as m:       # it needs the first flag
        m.setattr(multiclient, '_BATCHED_ENABLED', False)
        assert not pack.batched_eligible()
    for name in ('compressed', 'quantized'):   # FedCOMGATE and its kin
        with monkeypatch.context() as m:
            m.setattr(client.args, name, True)
            assert not pack.batched_eligible(), name
    for other in ('qsparse', 'apfl', 'fedadam'):
        with monkeypatch.context() as m:
            m.setattr(client.args, 'federated_type', other)
            assert not pack.batched_eligible(), other
    with monkeypatch.context() as m:       # a correction on the optimizer
        m.setattr(client.optimizer, '_prox_mu', 0.1)
        assert pack.batched_blockers() == [
            'a gradient correction is bound on the optimizer']
    with monkeypatch.context() as m:       # the remaining rules still hold
        m.setattr(client.args, 'growing_batch_size', True, raising=False)
        assert not pack.batched_eligible()
    assert pack.batched_eligible()


def test_fedavg_pack_has_no_algorithm_rows(flags):
    _client, pack = _federation(['--federated_type', 'fedavg'])
    assert pack.delta is None and pack.ctrl is None
    assert pack.batched_eligible()


def _run(extra, batched, monkeypatch, record=False):
    """one packed federation; returns (final state, meta, recording)"""
    monkeypatch.setattr(multiclient, '_BATCHED_ENABLED', batched)
    monkeypatch.setattr(multiclient, '_BATCHED_CORR_ENABLED', batched)
    torch.manual_seed(5)
    np.random.seed(5)
    client, pack = _federation(extra)
    assert pack.batched_eligible() == batched, pack.batched_blockers()
    return cc.run_federation(client, pack, monkeypatch, record=record)


CASES = {
    'fedprox': ['--federated_type', 'fedprox', '--fedprox_mu', '0.5'],
    'scaffold': ['--federated_type', 'scaffold'],
    'fedgate': ['--federated_type', 'fedgate'],
    'drfa-scaffold': ['--federated_type', 'scaffold', '--federated_drfa',
                      'true'],
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_packed_federation_against_float64_replay(name, monkeypatch):
    """3 rounds, C = 4, 3 of 4 clients online, tau = 3, momentum 0.9, weight
    decay, an lr change inside the run.  The slot loop, and the batched
    round with both flags on (the eager twin here), against the float64
    replay: the error of the final server and of delta / ctrl / c is at
    most 8x the fp32 replay's own error plus 16 ulps of scale."""
    extra = CASES[name]
    with monkeypatch.context() as m:
        slot, meta, rec = _run(extra, False, m, record=True)
    with monkeypatch.context() as m:
        bat, _meta, brec = _run(extra, True, m)
    assert len(rec['calls']) == 0 and len(brec['calls']) == 3     # one per round
    assert len(rec['rounds']) == 3
    for rnd in rec['rounds']:
        assert len(rnd['clients']) == 3 and rnd['n_sampled'] == 3
        assert all(len(s) == 3 for s in rnd['clients'].values())
    lrs = {s[2] for rnd in rec['rounds'] for st in rnd['clients'].values()
           for s in st}
    assert len(lrs) > 1                                  # the lr changed
    r64, entering = cc.replay_federation(rec, meta, F64)
    r32, _e = cc.replay_federation(rec, meta, torch.float32)
    if meta['ftype'] != 'fedprox':
        # round 1 starts from zero state; from round 2 on it must be live
        assert entering[0] == 0.0 and entering[1] > 1e-3 and entering[2] > 1e-3
    assert sorted(slot) == sorted(bat) == sorted(r64)
    for k in sorted(r64):
        e32 = lc.err(r32[k], r64[k])
        tol = lc.bound(e32, r64[k].abs().max().item())
        e_slot, e_bat = lc.err(slot[k], r64[k]), lc.err(bat[k], r64[k])
        d = (slot[k] - bat[k]).abs().max().item()
        print('%s %s: slot err %.3e  batched err %.3e  slot-batched %.3e  '
              'e32 %.3e  tol %.3e' % (name, k, e_slot, e_bat, d, e32, tol))
        assert e_slot <= tol, (k, e_slot, tol)
        assert e_bat <= tol, (k, e_bat, tol)
        assert d <= tol, (k, d, tol)
    # without the algorithm (plain FedAvg steps) the server is elsewhere
    plain, _e = cc.replay_federation(rec, meta, F64, correction=False)
    far = lc.err(slot['server'], plain['server'])
    tol = lc.bound(lc.err(r32['server'], r64['server']),
                   r64['server'].abs().max().item())
    assert far > 100 * tol, (far, tol)


# --------------------------------------------------------------------------
# what the packed trainer does not implement raises
# --------------------------------------------------------------------------
def _args(extra):
    from fedtorch_amd.parameters import get_args
    return get_args(['-d', 'mnist', '-a', 'logistic_regression', '-f', 'true',
                     '--clients_per_rank', '4', '--on_cuda', 'false',
                     '--checkpoint', '/tmp/ft_linround_corr', '--debug',
                     'false'] + list(extra))


@pytest.mark.parametrize('ftype', ['apfl', 'perfedme', 'perfedavg', 'afl',
                                   'qffl', 'qsparse', 'fedadam'])
def test_unsupported_type_raises(ftype):
    from fedtorch_amd.trainings.packed import check_packed_supported
    from fedtorch_amd.main import _dispatch
    args = _args(['--federated_type', ftype])
    with pytest.raises(ValueError, match='--federated_type %s' % ftype):
        check_packed_supported(args)
    with pytest.raises(ValueError, match='--clients_per_rank'):
        _dispatch(args)         # before a client is built


@pytest.mark.parametrize('flag', ['--compressed', '--quantized'])
def test_fedcomgate_raises(flag):
    from fedtorch_amd.trainings.packed import check_packed_supported
    args = _args(['--federated_type', 'fedgate', flag, 'true'])
    with pytest.raises(ValueError, match=flag + '.*--compressed false'):
        check_packed_supported(args)


def test_supported_types_pass_and_fedgate_is_dense_by_default():
    from fedtorch_amd.trainings.packed import check_packed_supported
    for ftype in ('fedavg', 'fedprox', 'scaffold', 'fedgate'):
        args = _args(['--federated_type', ftype])
        assert not args.compressed and not args.quantized
        check_packed_supported(args)


def test_trainer_raises_before_training():
    from fedtorch_amd.trainings.packed import \
        train_and_validate_federated_packed
    client, pack = _federation(['--federated_type', 'fedavg'])
    client.args.federated_type = 'qsparse'
    before = client.model_server.clone()
    with pytest.raises(ValueError, match='qsparse'):
        train_and_validate_federated_packed(client, pack)
    assert client.args.local_index == 0 and client.args.rounds_comm == 0
    assert torch.equal(client.model_server, before)


# --------------------------------------------------------------------------
# two processes over gloo
# --------------------------------------------------------------------------
def _worker_scaffold(rank, world, port, q):
    try:
        os.environ['MASTER_ADDR'] = '127.0.0.1'
        os.environ['MASTER_PORT'] = str(port)
        os.environ['FEDTORCH_SYNTH_SIZE'] = '300'
        dist.init_process_group('gloo', rank=rank, world_size=world)
        from fedtorch_amd.parameters import get_args
        from fedtorch_amd.nodes import Client
        from fedtorch_amd.trainings.packed import \
            train_and_validate_federated_packed
        from fedtorch_amd.parallel.multiclient import ClientPack
        args = get_args([
            '-d', 'mnist', '-a', 'logistic_regression', '-f', 'true',
            '--federated_type', 'scaffold', '--num_comms', '2',
            '--online_client_rate', '1.0', '--local_step', '2',
            '--federated_sync_type', 'local_step', '-b', '25',
            '--lr', '0.1', '--on_cuda', 'false', '--dist_backend', 'gloo',
            '-j', '0', '--clients_per_rank', '3', '--in_momentum', 'true',
            '--checkpoint', '/tmp/ft_ci_packed_scaffold', '--debug', 'false',
            '--manual_seed', '3'])
        client = Client(args, rank)
        client.initialize()
        client.initialize_dataset()
        client.load_local_dataset()
        client.gen_aux_models()
        pack = ClientPack(client, args.clients_per_rank)
        pack.build_loaders()
        train_and_validate_federated_packed(client, pack)
        ok = True
        for t in (client.model_server, client.model_server_control):
            rows = [torch.zeros_like(t) for _ in range(world)]
            dist.all_gather(rows, t.clone())
            ok = ok and all(torch.equal(rows[0], r) for r in rows)
            ok = ok and bool(torch.isfinite(t).all()) and bool(t.any())
        ok = ok and bool(pack.ctrl.any())
        q.put((rank, bool(ok)))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        import traceback
        traceback.print_exc()
        q.put((rank, False))
        raise


def test_two_proc_packed_scaffold():
    """2 ranks x 3 clients, 2 rounds: the server and the server control c
    end bitwise equal on both ranks, finite and non-zero."""
    world = 2
    ctx = mp.get_context('spawn')
    q = ctx.SimpleQueue()
    procs = [ctx.Process(target=_worker_scaffold, args=(r, world, 29991, q))
             for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get() for _ in range(world)]
    for p in procs:
        p.join(timeout=240)
        assert p.exitcode == 0
    assert all(ok for _, ok in results)
