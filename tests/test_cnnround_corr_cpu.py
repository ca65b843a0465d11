# -*- coding: utf-8 -*-
"""The gradient corrections of ops.cnn_local_rounds without a GPU: the eager
twin against the corrected float64 step loop (tests/cnnround_corr_cases.py),
and the second opt-in FEDTORCH_PACKED_BATCHED_CNN_CORR of ClientPack."""
import pytest
import torch

import linround_cases as lc
import cnnround_cases as cc
import cnnround_corr_cases as kc
import fedtorch_amd.ops as ops
from fedtorch_amd.parallel import multiclient
from test_cnnround_cpu import _federation


@pytest.mark.parametrize('kind', kc.KINDS)
def test_twin_against_float64_replay(kind):
    """bound: 8x the fp32 CPU replay's own error plus 16 fp32 ulps of the
    output's scale (lc.bound)"""
    *args, corr, ref, e32 = kc.case(cc.SMALL, kind)
    got = cc.call_op(ops, *args, op=kc.with_corr(ops.cnn_local_rounds, corr))
    assert torch.equal(got['mom_init'], ref['mom_init'])
    for k in ('replicas', 'snap', 'loss'):
        assert lc.same_nan_pattern(got[k], ref[k]), k
        e, tol = lc.err(got[k], ref[k]), lc.bound(e32[k], cc.scale_of(ref[k]))
        assert e <= tol, (k, e, tol)
    # the correction is far outside that bound
    assert lc.err(cc.case(cc.SMALL)[6]['replicas'], ref['replicas']) > 5e-5


@pytest.mark.parametrize('ftype', ('fedprox', 'scaffold', 'fedgate'))
def test_cnn_corr_flag_truth_table(ftype, monkeypatch):
    monkeypatch.setattr(multiclient, '_BATCHED_CNN_ENABLED', True)
    client, pack = _federation(('--federated_type', ftype))
    # flag off: the slot loop, whatever the other paths' opt-ins say
    monkeypatch.setattr(multiclient, '_BATCHED_CORR_ENABLED', True)
    monkeypatch.setattr(multiclient, '_BATCHED_MLP_CORR_ENABLED', True)
    monkeypatch.setattr(multiclient, '_BATCHED_CNN_CORR_ENABLED', False)
    assert pack.cnn_batched_blockers() == ['federated_type is not fedavg']
    monkeypatch.setattr(multiclient, '_BATCHED_CNN_CORR_ENABLED', True)
    assert pack.cnn_batched_eligible()
    for name in ('quantized', 'compressed'):
        with monkeypatch.context() as m:
            m.setattr(client.args, name, True, raising=False)
            assert not pack.cnn_batched_eligible(), name
