# -*- coding: utf-8 -*-
"""Packed FedProx / SCAFFOLD / FedGATE federations of the stock MNIST `cnn`
through ClientPack on the GPU: both CNN flags on (the batched kernels with
the correction term, hip/cnnround.h) against both off (the slot loop), after
every round, against the float64 replay of the federation
(mlpround_corr_cases.replay_federation over cnnround_cases.ref_rounds).

Like test_gpu_packed_cnnround.py this builds on-GPU Clients, which change
process-wide state; `process_state` is that file's fixture."""
import random

import numpy as np
import pytest
import torch

import linround_cases as lc
import cnnround_cases as cc
import cnnround_corr_cases as kc
import mlpround_corr_cases as mcc
import fedtorch_amd.ops as ops
from fedtorch_amd.parallel import multiclient

pytestmark = pytest.mark.gpu

_REAL_OP = ops.cnn_local_rounds
ROUNDS, C = 3, 3
# --manual_seed per type: model init and loader shuffles for which the
# precondition of test_gpu_packed_cnnround.py (PACKED_MARGIN, its reasoning)
# holds over the three rounds; searched on the CPU (on_cuda=False)
SEEDS = {'fedprox': 124, 'scaffold': 111, 'fedgate': 111}
PACKED_MARGIN = 4.0


@pytest.fixture
def process_state(monkeypatch):
    """An on-GPU Client switches torch.backends.cudnn.benchmark on and
    reseeds every generator.  The test hands the process on as it found
    it."""
    monkeypatch.setattr(torch.backends.cudnn, 'benchmark',
                        torch.backends.cudnn.benchmark)
    rng = (torch.get_rng_state(), torch.cuda.get_rng_state(),
           np.random.get_state(), random.getstate())
    yield
    torch.cuda.synchronize()
    torch.set_rng_state(rng[0])
    torch.cuda.set_rng_state(rng[1])
    np.random.set_state(rng[2])
    random.setstate(rng[3])


def _ref_rounds(*a, dtype, pre=None):
    """mcc.ref_rounds_corr's signature (layout, eps, ...) for the CNN"""
    a, corr = list(a[:-1]), a[-1]
    del a[12]                              # eps
    with kc.corrected(corr, a[3], a[5], dtype):
        return cc.ref_rounds(*a, dtype=dtype, pre=pre)


def federation(ftype, batched, monkeypatch, on_cuda=True, seed=None):
    """a 3-round federation; returns mcc.run_federation's dict with the
    batched calls and `states`: server and delta / ctrl / c after each
    round"""
    from fedtorch_amd.parameters import get_args
    from fedtorch_amd.nodes import Client
    monkeypatch.setattr(multiclient, '_BATCHED_CNN_ENABLED', batched)
    monkeypatch.setattr(multiclient, '_BATCHED_CNN_CORR_ENABLED', batched)
    monkeypatch.setenv('FEDTORCH_SYNTH_SIZE', '210')
    torch.manual_seed(5)
    np.random.seed(5)
    seed = SEEDS[ftype] if seed is None else seed
    client = Client(get_args([
        '-d', 'mnist', '-a', 'cnn', '-f', 'true', '--federated_type', ftype,
        '--fedprox_mu', '0.5', '--num_comms', str(ROUNDS),
        '--clients_per_rank', str(C), '-b', '5', '--lr', '0.05',
        '--federated_sync_type', 'local_step', '--local_step', '3',
        '--online_client_rate', '1.0', '--in_momentum', 'true',
        '--in_momentum_factor', '0.9', '--weight_decay', '1e-3',
        '--stop_criteria', 'epoch', '--num_epochs', '8',
        '--on_cuda', 'true' if on_cuda else 'false', '-j', '0',
        '--manual_seed', str(seed),
        '--checkpoint', '/tmp/ft_cnnround_corr_gpu', '--debug', 'false']), 0)
    client.initialize()
    client.initialize_dataset()
    client.load_local_dataset()
    client.gen_aux_models()
    pack = multiclient.ClientPack(client, C)
    pack.build_loaders()
    if not on_cuda:        # the seed search: the loaders a GPU run builds
        from fedtorch_amd.components.datasets.device_cache import \
            DeviceCachedLoader
        for j, old in enumerate(pack.train_loaders):
            pack.train_loaders[j] = DeviceCachedLoader(
                old.dataset, 5, seed=seed * 1000003 + pack.global_id(j) * 8191,
                shuffle=True, device='cpu')
    assert pack.cnn_batched_eligible() == batched, pack.cnn_batched_blockers()
    calls, states = [], []
    keep = lambda t: None if not torch.is_tensor(t) \
        else t.detach().cpu().clone()  # noqa: E731

    def state():
        s = dict(server=client.model_server, delta=pack.delta, ctrl=pack.ctrl,
                 c=client.model_server_control if pack.ctrl is not None
                 else None)
        return {k: keep(v) for k, v in s.items() if v is not None}

    def op(*a, **k):
        calls.append(([keep(t) if torch.is_tensor(t) else t for t in a],
                      dict({n: keep(v) if torch.is_tensor(v) else v
                            for n, v in k.items()}, eps=None)))
        return _REAL_OP(*a, **k)
    real_sample = client.comm.sample_online_global

    def sample(total):                     # a round begins: the last one's end
        states.append(state())
        return real_sample(total)
    monkeypatch.setattr(ops, 'cnn_local_rounds', op)
    monkeypatch.setattr(client.comm, 'sample_online_global', sample)
    run = mcc.run_federation(client, pack, monkeypatch)
    return dict(run, calls=calls, states=states[1:] + [state()])


def check(off, on, label=''):
    """both runs and their distance, after every round, within lc.bound of
    the fp32 replay's error against the float64 replay of the federation over
    the operands the batched run recorded; the decision precondition first"""
    assert len(off['calls']) == 0 and len(on['calls']) == ROUNDS
    assert len(off['states']) == len(on['states']) == ROUNDS
    for r in range(1, ROUNDS + 1):
        part = dict(on, calls=on['calls'][:r], rounds=on['rounds'][:r])
        p64, p32 = [], []
        r64 = mcc.replay_federation(part, cc.F64, pre=p64)
        r32 = mcc.replay_federation(part, cc.F32, pre=p32)
        for what, (lo, e) in cc.margins(p64, p32).items():
            assert lo > PACKED_MARGIN * e, (what, r, lo, e)
        a, b = off['states'][r - 1], on['states'][r - 1]
        assert sorted(a) == sorted(b) == sorted(r64)
        for k in r64:
            tol = lc.bound(lc.err(r32[k], r64[k]), r64[k].abs().max().item())
            e_a, e_b = lc.err(a[k], r64[k]), lc.err(b[k], r64[k])
            d = (a[k] - b[k]).abs().max().item()
            print('%s round %d %s: slot loop %.3e  kernels %.3e  distance '
                  '%.3e  tol %.3e' % (label, r, k, e_a, e_b, d, tol))
            assert max(e_a, e_b, d) <= tol, (r, k, e_a, e_b, d, tol)


@pytest.mark.parametrize('ftype', sorted(SEEDS))
def test_packed_federation_kernels_against_slot_loop(ftype, process_state,
                                                     monkeypatch):
    """C = 3, tau = 3, B = 5, momentum 0.9, three rounds (delta and the
    controls are live from the second)."""
    monkeypatch.setattr(mcc, 'ref_rounds_corr', _ref_rounds)
    with monkeypatch.context() as m:
        off = federation(ftype, False, m)
    with monkeypatch.context() as m:
        on = federation(ftype, True, m)
    for r, (_pos, kw) in enumerate(on['calls'][1:]):
        for n in ('delta', 'ctrl_client'):
            assert kw.get(n) is None or bool(kw[n].any()), (n, r)
    check(off, on, ftype)
