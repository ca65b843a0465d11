# -*- coding: utf-8 -*-
"""ops.rnn_wide_local_rounds (65 <= H <= 128) without a GPU: the eager twin
against the float64 step loop of test_gpu_rnnround.py, the H ranges of the two
ops, the truth table of the second opt-in and the packed trainer's route."""
import pytest
import torch

import fedtorch_amd.ops as ops
from fedtorch_amd.parallel import multiclient
from test_gpu_rnnround import assert_bounded, call_op, make_case
from test_rnnround_cpu import _federation


def test_twin_against_float64_loop():
    case, kw = make_case(7, 65, 2, 5, 0.9)
    got = call_op(case, kw, 2, device='cpu', op=ops.rnn_wide_local_rounds)
    assert_bounded(got, case, kw, 2)


@pytest.mark.parametrize('op,H', [('rnn_wide_local_rounds', 64),
                                  ('rnn_wide_local_rounds', 129),
                                  ('rnn_local_rounds', 65)])
def test_h_ranges(op, H):
    case, kw = make_case(7, 65, 2, 5, 0.9)
    enc = kw['layout']['encoder']
    kw['layout'] = dict(kw['layout'], encoder=(enc[0], enc[1], H))
    with pytest.raises(ValueError, match='%s: unsupported H=%d' % (op, H)):
        call_op(case, kw, 2, device='cpu', op=getattr(ops, op))
    assert ops.rnn_wide_round_limits() == dict(B=64, Hmin=65, Hmax=128,
                                               V=128, K=128)


def test_second_flag_truth_table(monkeypatch):
    _c, pack = _federation(['--rnn_hidden_size', '72'])
    monkeypatch.setattr(multiclient, '_BATCHED_RNN_ENABLED', True)
    assert not pack.rnn_batched_eligible() and not pack.rnn_batched_wide()
    assert pack.rnn_batched_blockers() == [
        'rnn_local_rounds: unsupported H=72 (1 <= H <= 64)']
    monkeypatch.setattr(multiclient, '_BATCHED_RNN_WIDE_ENABLED', True)
    assert pack.rnn_batched_blockers() == [] and pack.rnn_batched_wide()
    _c, narrow = _federation()                                   # H = 20
    assert narrow.rnn_batched_eligible() and not narrow.rnn_batched_wide()
    _c, prox = _federation(['--rnn_hidden_size', '72',
                            '--federated_type', 'fedprox'])
    assert not prox.rnn_batched_eligible()
    monkeypatch.setattr(multiclient, '_BATCHED_RNN_ENABLED', False)
    assert not pack.rnn_batched_eligible()       # the second flag alone


@pytest.mark.parametrize('H,route', [(20, 'rnn_local_rounds'),
                                     (72, 'rnn_wide_local_rounds')])
def test_trainer_route(monkeypatch, H, route):
    """both flags on, two rounds: one call per round of the op of the H"""
    from fedtorch_amd.trainings.packed import \
        train_and_validate_federated_packed
    monkeypatch.setattr(multiclient, '_BATCHED_RNN_ENABLED', True)
    monkeypatch.setattr(multiclient, '_BATCHED_RNN_WIDE_ENABLED', True)
    client, pack = _federation(['--rnn_hidden_size', str(H)])
    calls = []
    for name in ('rnn_local_rounds', 'rnn_wide_local_rounds'):
        def op(*a, _name=name, _real=getattr(ops, name), **k):
            calls.append(_name)
            return _real(*a, **k)
        monkeypatch.setattr(ops, name, op)
    train_and_validate_federated_packed(client, pack)
    assert calls == [route] * 2
    assert pack.hidden.shape == (3, 30, H)
    assert torch.isfinite(client.model_server).all()
