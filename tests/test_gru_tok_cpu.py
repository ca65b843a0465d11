# -*- coding: utf-8 -*-
"""Token path of ops.gru without a GPU: the truth table of gru_tok_eligible
and CharGRU on the CPU, which FEDTORCH_FUSED_GRU_TOKENS must not change."""
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import fedtorch_amd.ops as ops
from fedtorch_amd.components.models.rnn import CharGRU
from fedtorch_amd.ops import gru as fgru


@pytest.mark.parametrize('kw,want', [
    (dict(), True),
    (dict(H=65), True), (dict(H=128), True), (dict(H=129), False),
    (dict(H=65, wide=False), False),
    (dict(tokens=False), False),
    (dict(cuda=False), False),                          # CPU tensor
    (dict(tok=torch.zeros(4, 5, dtype=torch.int32)), False),
    (dict(tok=torch.zeros(4, 5, 1, dtype=torch.int64)), False),
    (dict(tok=torch.zeros(4, 0, dtype=torch.int64)), False),
    (dict(tok=torch.zeros(3, 5, dtype=torch.int64)), False),    # B of h0
    (dict(enc=dict(padding_idx=0)), False),
    (dict(enc=dict(max_norm=1.)), False), (dict(enc=dict(sparse=True)), False),
    (dict(enc=dict(scale_grad_by_freq=True)), False),
    (dict(enc_dtype=torch.bfloat16), True),
    (dict(enc_dtype=torch.float64), False),
    (dict(emb_dim=7), False),
    (dict(layers=2), False),
])
def test_gru_tok_eligible_truth_table(monkeypatch, kw, want):
    """an otherwise eligible call, set up as in test_gru_wide_cpu.py"""
    H = kw.get('H', 50)
    monkeypatch.setattr(ops, '_C', SimpleNamespace())
    monkeypatch.setattr(ops, 'FORCE_EAGER', False)
    monkeypatch.setattr(fgru, '_GRU_ENABLED', kw.get('narrow', True))
    monkeypatch.setattr(fgru, '_GRU_WIDE_ENABLED', kw.get('wide', True))
    monkeypatch.setattr(fgru, '_GRU_TOK_ENABLED', kw.get('tokens', True))
    if kw.get('cuda', True):
        monkeypatch.setattr(fgru, '_kernels_active', lambda t:
                            ops.hip_available() and not ops.FORCE_EAGER)
    gru = nn.GRU(H, H, kw.get('layers', 1), batch_first=True)
    enc = nn.Embedding(86, kw.get('emb_dim', H), **kw.get('enc', {}))
    enc = enc.to(kw.get('enc_dtype', torch.float32))
    tok = kw.get('tok', torch.zeros(4, 5, dtype=torch.int64))
    h0 = torch.zeros(gru.num_layers, 4, H)
    assert fgru.gru_tok_eligible(enc, gru, tok, h0) is want


def test_char_gru_cpu_unchanged_by_flag(monkeypatch):
    g = torch.Generator().manual_seed(5)
    x = torch.randint(0, 86, (10, 12), generator=g)
    y = torch.randint(0, 86, (10, 12), generator=g)
    runs = []
    for on in (False, True):
        for name in ('_GRU_ENABLED', '_GRU_WIDE_ENABLED', '_GRU_TOK_ENABLED'):
            monkeypatch.setattr(fgru, name, on)
        torch.manual_seed(0)
        model = CharGRU('shakespeare', 86, 50, 86, 10)
        logits = model(x)
        F.cross_entropy(logits, y).backward()
        runs.append([logits.detach(), model.hidden]
                    + [p.grad for p in model.parameters()])
    assert len(runs[0]) == 9
    for a, b in zip(*runs):
        assert torch.equal(a, b)
