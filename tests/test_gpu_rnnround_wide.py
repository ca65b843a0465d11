# -*- coding: utf-8 -*-
"""rnn_wide_local_rounds (hip/rnnround_wide.h, 65 <= H <= 128) on the GPU
against the float64 CPU step loop of test_gpu_rnnround.py, bound 8 e32 +
16 ulp.  The shapes take every NT = ceil(H/16) in 5..8, one column past a
tile boundary (65, 97), full tiles (80, 112, 128), a second batch tile
(B = 17, 18) and T = 1, where no prefetch step exists."""
import numpy as np
import pytest
import torch

import fedtorch_amd.ops as ops
from fedtorch_amd.parallel import multiclient
from test_gpu_packed_rnnround import process_state  # noqa: F401
from test_gpu_rnnround import _same, assert_bounded, call_op, make_case
from test_rnnround_cpu import _federation, cache_loaders

pytestmark = pytest.mark.gpu

SHAPES = [(7, 65, 2, 1), (11, 80, 3, 5), (9, 97, 2, 17), (11, 112, 1, 18),
          (86, 128, 3, 18)]


def wide(case, kw, k_cut=2):
    return call_op(case, kw, k_cut, op=ops.rnn_wide_local_rounds)


@pytest.mark.parametrize('momentum', [0.0, 0.9])
@pytest.mark.parametrize('V,H,T,B', SHAPES)
def test_against_float64_loop(V, H, T, B, momentum):
    case, kw = make_case(V, H, T, B, momentum)
    assert_bounded(wide(case, kw), case, kw, 2)


def test_two_runs_bit_identical():
    case, kw = make_case(86, 128, 3, 18, 0.9)
    _same(wide(case, kw), wide(case, kw))


def test_graph_capture_replays():
    case, kw = make_case(11, 80, 3, 5, 0.9)
    want = wide(case, kw)
    d = {k: v.clone().cuda() for k, v in case.items()}
    inout = ('replicas', 'in_mom', 'mom_init', 'snap', 'hidden', 'hid_rows')
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss = ops.rnn_wide_local_rounds(
            d['X'], d['Y'], d['idx'], d['steps'], d['lr'], d['server'],
            d['replicas'], d['in_mom'], d['mom_init'], d['snap'], 2,
            d['hidden'], d['hid_rows'], **kw)
    for _ in range(3):                 # in/out operands back, then replay
        for k in inout:
            d[k].copy_(case[k])
        g.replay()
        torch.cuda.synchronize()
        _same(dict(d, loss=loss), want)


def test_limits_and_rejections():
    lim = ops.rnn_wide_round_limits()
    assert list(ops._C.rnn_wide_round_limits()) == [
        lim['B'], lim['Hmin'], lim['Hmax'], lim['V'], lim['K']]
    case, kw = make_case(11, 80, 3, 5, 0.9)
    enc = kw['layout']['encoder']
    for H in (64, 129):
        bad = dict(kw, layout=dict(kw['layout'], encoder=(enc[0], enc[1], H)))
        with pytest.raises(RuntimeError, match='rnn_wide_local_rounds: '
                                               'unsupported H=%d' % H):
            wide(case, bad)


def test_packed_round_against_float64_loop(process_state,  # noqa: F811
                                           monkeypatch):
    """test_gpu_packed_rnnround.py at H = 72 with both flags on: C = 3,
    tau = 3, steps of 30, 30 and 6 rows, T = 6, momentum 0.9, one round"""
    from fedtorch_amd.trainings.packed import \
        train_and_validate_federated_packed
    monkeypatch.setattr(multiclient, '_BATCHED_RNN_ENABLED', True)
    monkeypatch.setattr(multiclient, '_BATCHED_RNN_WIDE_ENABLED', True)
    torch.manual_seed(5)
    np.random.seed(5)
    client, pack = _federation(['--on_cuda', 'true', '--num_comms', '1',
                                '--rnn_hidden_size', '72'], cached=False)
    cache_loaders(pack, 'cuda')
    assert pack.rnn_batched_eligible(), pack.rnn_batched_blockers()
    rec, real = {}, ops.rnn_wide_local_rounds
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
    monkeypatch.setattr(ops, 'rnn_wide_local_rounds', op)
    train_and_validate_federated_packed(client, pack)
    torch.cuda.synchronize()
    case, kw = rec['case'], rec['kw']
    assert (case['idx'] >= 0).sum(2).tolist() == [[30, 30, 6]] * 3
    assert kw['layout']['encoder'][1:] == (86, 72) and kw['momentum'] == 0.9
    case['snap'] = torch.zeros_like(case['replicas'])       # no DRFA: unused
    rec['got']['snap'] = case['snap']
    assert_bounded(rec['got'], case, kw, 0)
