# -*- coding: utf-8 -*-
"""Truth table of ops.gru.gru_wide_eligible without a GPU."""
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

import fedtorch_amd.ops as ops
from fedtorch_amd.ops import gru as fgru


@pytest.mark.parametrize('kw,want', [
    (dict(H=64), (True, False)),
    (dict(H=65), (False, True)),
    (dict(H=128), (False, True)),
    (dict(H=129), (False, False)),
    (dict(H=65, wide=False), (False, False)),
    (dict(H=65, narrow=False), (False, False)),
    (dict(H=128, cuda=False), (False, False)),         # CPU tensor
])
def test_gru_wide_eligible_truth_table(monkeypatch, kw, want):
    """(gru_eligible, gru_wide_eligible) of an otherwise eligible call, set
    up as in test_gru_cpu.py::test_gru_eligible_truth_table"""
    H = kw['H']
    monkeypatch.setattr(ops, '_C', SimpleNamespace())
    monkeypatch.setattr(ops, 'FORCE_EAGER', False)
    monkeypatch.setattr(fgru, '_GRU_ENABLED', kw.get('narrow', True))
    monkeypatch.setattr(fgru, '_GRU_WIDE_ENABLED', kw.get('wide', True))
    if kw.get('cuda', True):
        monkeypatch.setattr(fgru, '_kernels_active', lambda t:
                            ops.hip_available() and not ops.FORCE_EAGER)
    gru = nn.GRU(H, H, batch_first=True)
    x, h0 = torch.randn(4, 5, H), torch.zeros(1, 4, H)
    assert fgru.MAX_H == 64 and fgru.MAX_H_WIDE == 128
    assert (fgru.gru_eligible(gru, x, h0),
            fgru.gru_wide_eligible(gru, x, h0)) == want
