# -*- coding: utf-8 -*-
"""Truth table of ops.gru.gru_stream_eligible without a GPU."""
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

import fedtorch_amd.ops as ops
from fedtorch_amd.ops import gru as fgru


@pytest.mark.parametrize('kw,want', [
    (dict(H=128), (True, False)),
    (dict(H=129), (False, True)),
    (dict(H=256), (False, True)),
    (dict(H=257), (False, False)),
    (dict(H=129, stream=False), (False, False)),
    (dict(H=129, narrow=False), (False, False)),
    (dict(H=256, cuda=False), (False, False)),         # CPU tensor
    (dict(H=256, layers=2), (False, False)),
])
def test_gru_stream_eligible_truth_table(monkeypatch, kw, want):
    """(gru_wide_eligible, gru_stream_eligible) of an otherwise eligible
    call, set up as in test_gru_cpu.py::test_gru_eligible_truth_table"""
    H = kw['H']
    monkeypatch.setattr(ops, '_C', SimpleNamespace())
    monkeypatch.setattr(ops, 'FORCE_EAGER', False)
    monkeypatch.setattr(fgru, '_GRU_ENABLED', kw.get('narrow', True))
    monkeypatch.setattr(fgru, '_GRU_WIDE_ENABLED', True)
    monkeypatch.setattr(fgru, '_GRU_STREAM_ENABLED', kw.get('stream', True))
    if kw.get('cuda', True):
        monkeypatch.setattr(fgru, '_kernels_active', lambda t:
                            ops.hip_available() and not ops.FORCE_EAGER)
    L = kw.get('layers', 1)
    gru = nn.GRU(H, H, num_layers=L, batch_first=True)
    x, h0 = torch.randn(4, 5, H), torch.zeros(L, 4, H)
    assert fgru.MAX_H_WIDE == 128 and fgru.MAX_H_STREAM == 256
    assert (fgru.gru_wide_eligible(gru, x, h0),
            fgru.gru_stream_eligible(gru, x, h0)) == want


@pytest.mark.parametrize('stream', [False, True])
def test_gru_seq_on_cpu_is_the_module(monkeypatch, stream):
    monkeypatch.setattr(fgru, '_GRU_ENABLED', True)
    monkeypatch.setattr(fgru, '_GRU_STREAM_ENABLED', stream)
    torch.manual_seed(0)
    gru = nn.GRU(8, 130, batch_first=True)
    x, h0 = torch.randn(2, 3, 8), torch.randn(1, 2, 130)
    assert not fgru.gru_stream_eligible(gru, x, h0)
    for got, want in zip(fgru.gru_seq(gru, x, h0), gru(x, h0)):
        assert torch.equal(got, want)
