# -*- coding: utf-8 -*-
"""A packed char-GRU round through ClientPack on the GPU with
FEDTORCH_PACKED_BATCHED_RNN on (ops.rnn_local_rounds, hip/rnnround.h, on the
trainer's real arena offsets, stacked windows, plan walk and per-client hidden
state), against the float64 step loop of test_gpu_rnnround.py over the
recorded operands.

Like test_gpu_packed_cnnround.py this builds an on-GPU Client, which switches
torch.backends.cudnn.benchmark on and reseeds every generator; the fixture
puts both back, and the file sorts behind the kernel tests."""
import random

import numpy as np
import pytest
import torch

import fedtorch_amd.ops as ops
from fedtorch_amd.parallel import multiclient
from test_gpu_rnnround import assert_bounded
from test_rnnround_cpu import _federation, cache_loaders

pytestmark = pytest.mark.gpu


@pytest.fixture
def process_state(monkeypatch):
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


def test_packed_round_against_float64_loop(process_state, monkeypatch):
    """C = 3, tau = 3, B = 30 over 66 windows per client (steps of 30, 30
    and 6 rows: the state resumes, then resets), stock vocabulary, H = 20,
    T = 6, momentum 0.9, one round"""
    from fedtorch_amd.trainings.packed import \
        train_and_validate_federated_packed
    monkeypatch.setattr(multiclient, '_BATCHED_RNN_ENABLED', True)
    torch.manual_seed(5)
    np.random.seed(5)
    client, pack = _federation(['--on_cuda', 'true', '--num_comms', '1'],
                               cached=False)
    cache_loaders(pack, 'cuda')
    assert pack.rnn_batched_eligible(), pack.rnn_batched_blockers()
    rec, real = {}, ops.rnn_local_rounds
    names = ('X', 'Y', 'idx', 'steps', 'lr', 'server', 'replicas', 'in_mom',
             'mom_init', 'snap', 'k_cut', 'hidden', 'hid_rows')

    def op(*a, **k):
        rec['case'] = {n: t.clone().cpu() for n, t in zip(names, a)
                       if torch.is_tensor(t)}
        rec['kw'] = dict(k)
        loss = real(*a, **k)
        rec['got'] = dict(loss=loss, replicas=a[6].clone(),
                          in_mom=a[7].clone(), mom_init=a[8].clone(),
                          hidden=a[11].clone(), hid_rows=a[12].clone())
        return loss
    monkeypatch.setattr(ops, 'rnn_local_rounds', op)
    train_and_validate_federated_packed(client, pack)
    torch.cuda.synchronize()
    case, kw = rec['case'], rec['kw']
    assert case['idx'].shape == (3, 3, 30)
    assert (case['idx'] >= 0).sum(2).tolist() == [[30, 30, 6]] * 3
    assert kw['layout']['encoder'][1:] == (86, 20) and kw['momentum'] == 0.9
    case['snap'] = torch.zeros_like(case['replicas'])       # no DRFA: unused
    rec['got']['snap'] = case['snap']
    assert_bounded(rec['got'], case, kw, 0)
