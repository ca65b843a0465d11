# -*- coding: utf-8 -*-
"""GRU sequence path without a GPU: the float64 step-loop reference of
tests/gru_cases.py against torch.nn.GRU, the exactness preconditions of the
GPU exact cases, and the CPU behaviour of ops.gru (gru_seq is gru(x, h0),
CharGRU is unchanged, the truth table of gru_eligible)."""
import contextlib
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

import gru_cases as gc
import fedtorch_amd.ops as ops
from fedtorch_amd.components.models.rnn import CharGRU
from fedtorch_amd.ops import gru as fgru

F64 = torch.float64
_REAL_ACTIVE = fgru._kernels_active


@contextlib.contextmanager
def _flag(on):
    old = fgru._GRU_ENABLED
    fgru._GRU_ENABLED = on
    try:
        yield
    finally:
        fgru._GRU_ENABLED = old


# --------------------------------------------------------------------------
# the reference is the GRU of torch.nn
# --------------------------------------------------------------------------
@pytest.mark.parametrize('B,T,H,I', [(3, 5, 7, 4), (2, 1, 1, 3),
                                     (4, 6, 17, 17)])
def test_reference_matches_nn_gru(B, T, H, I):
    torch.manual_seed(B * 100 + T * 10 + H)
    gru = nn.GRU(I, H, batch_first=True).double()
    x = torch.randn(B, T, I, dtype=F64, requires_grad=True)
    h0 = torch.randn(1, B, H, dtype=F64, requires_grad=True)
    dout = torch.randn(B, T, H, dtype=F64)
    out, hn = gru(x, h0)
    params = (gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0,
              gru.bias_hh_l0)
    dx, dh0, dwi, dwh, dbi, dbh = torch.autograd.grad(
        out, (x, h0) + params, dout)

    with torch.no_grad():
        gx = x @ gru.weight_ih_l0.t() + gru.bias_ih_l0
        r_out, gates = gc.ref_fwd(gx, gru.weight_hh_l0, gru.bias_hh_l0,
                                  h0[0])
        g = gc.ref_bwd(dout, r_out, gates, gru.weight_hh_l0, h0[0])
        r_dx = g['dgx'] @ gru.weight_ih_l0
        r_dwi = g['dgx'].reshape(-1, 3 * H).t() @ x.reshape(-1, I)
        r_dbi = g['dgx'].sum((0, 1))

    def close(a, b):
        assert a.shape == b.shape
        assert torch.allclose(a, b, rtol=1e-12, atol=1e-13), \
            (a - b).abs().max().item()

    close(r_out, out)
    close(r_out[:, -1], hn[0])
    close(r_dx, dx)
    close(g['dh0'], dh0[0])
    close(r_dwi, dwi)
    close(g['dw'], dwh)
    close(r_dbi, dbi)
    close(g['db'], dbh)
    # q is what the n gate multiplies by r
    close(gates[:, :, 3],
          torch.stack([(h0[0] if t == 0 else out[:, t - 1]).detach()
                       @ gru.weight_hh_l0[2 * H:].t() + gru.bias_hh_l0[2 * H:]
                       for t in range(T)], dim=1).detach())


# --------------------------------------------------------------------------
# preconditions of the exact GPU cases
# --------------------------------------------------------------------------
@pytest.mark.parametrize('H', gc.MAP_H)
@pytest.mark.parametrize('B', gc.MAP_B)
def test_map_case_preconditions(B, H):
    gx, w, b, h0, out, gates = gc.map_case(B, H)
    for k in range(3):
        blk = w[k * H:(k + 1) * H]
        assert H == 1 or not torch.equal(blk, blk.t())
    for t in (w, b, h0):
        assert torch.equal(t, t.round())
        assert torch.equal(t.to(torch.bfloat16).to(F64), t)
    assert gc.fp32_exact(gx)
    # q = sum_k h0[b,k] w[2H+n,k] + b[2H+n]: exact in any order
    terms = torch.cat((h0.unsqueeze(1) * w[2 * H:].unsqueeze(0),
                       b[2 * H:].view(1, H, 1).expand(B, H, 1)), dim=2)
    assert gc.order_free_exact(terms, 2)
    q = gates[:, 0, 3]
    assert torch.equal(q, terms.sum(2)) and gc.fp32_exact(q)
    assert q.abs().max() > 0 or H == 1


@pytest.mark.parametrize('B,H', gc.TIME_BH)
@pytest.mark.parametrize('T', gc.TIME_T)
def test_time_case_preconditions(B, T, H):
    gx, w, b, h0, out = gc.time_case(B, T, H)
    r_out, gates = gc.ref_fwd(gx, w, b, h0)
    assert torch.equal(r_out, out) and gc.fp32_exact(out)
    assert gc.fp32_exact(gates)
    assert torch.equal(gates[:, :, :2], torch.full_like(gates[:, :, :2], .5))
    assert not gates[:, :, 2:].any()
    # rows and columns are told apart
    assert B == 1 or len({tuple(r.tolist()) for r in h0}) > 1


@pytest.mark.parametrize('B,H', gc.BWD_BH)
@pytest.mark.parametrize('T', gc.BWD_T)
def test_bwd_case_preconditions(B, T, H):
    trace = []
    dout, out, gates, w, h0, ref = gc.bwd_case(B, T, H, trace=trace)
    assert H == 1 or not torch.equal(w[:H], w[:H].t())
    assert torch.equal(w.to(torch.bfloat16).to(F64), w)
    for t in (dout, out, gates, w, h0):
        assert gc.fp32_exact(t)
    assert len(trace) == 13 * T
    for name, terms, value in trace:
        assert gc.fp32_exact(value), name
        if terms is not None:
            assert gc.fp32_exact(terms), name
            assert gc.order_free_exact(terms, 1), name
            assert torch.equal(terms.sum(1), value), name
    for name in ('dgx', 'dgh', 'dh0'):
        assert gc.fp32_exact(ref[name]), name
    assert ref['dh0'].abs().max() > 0 and ref['dgx'].abs().max() > 0


def test_random_case_tolerances():
    case = gc.random_case(17, 2, 17)
    assert case is gc.random_case(17, 2, 17)
    for name in ('out', 'gates', 'dgx', 'dgh', 'dh0', 'dw', 'db'):
        mag = case['ref'][name].abs().max().item()
        assert 0 < case['tol'][name] < 1e-4 * max(mag, 1.0), name
    assert gc.ulp32(1.0) == 2.0 ** -23 and gc.ulp32(1.5) == 2.0 ** -23
    assert gc.ulp32(0.75) == 2.0 ** -24 and gc.ulp32(0.0) == 0.0


# --------------------------------------------------------------------------
# CPU behaviour of ops.gru
# --------------------------------------------------------------------------
@pytest.mark.parametrize('on', [False, True])
def test_gru_seq_is_gru_on_cpu(on):
    torch.manual_seed(3)
    gru = nn.GRU(6, 9, batch_first=True)
    x = torch.randn(4, 5, 6)
    h0 = torch.randn(1, 4, 9)
    want_out, want_h = gru(x, h0)
    with _flag(on):
        assert not fgru.gru_eligible(gru, x, h0)
        out, h = fgru.gru_seq(gru, x, h0)
    assert out.dtype == want_out.dtype and torch.equal(out, want_out)
    assert h.shape == want_h.shape and torch.equal(h, want_h)
    g1 = torch.autograd.grad(want_out.sum(), gru.weight_hh_l0)[0]
    g2 = torch.autograd.grad(out.sum(), gru.weight_hh_l0)[0]
    assert torch.equal(g1, g2)


def _char_gru(seed=0):
    torch.manual_seed(seed)
    return CharGRU('shakespeare', 86, 50, 86, 10)


def test_char_gru_cpu_unchanged_by_flag():
    g = torch.Generator().manual_seed(5)
    batches = [torch.randint(0, 86, (10, 12), generator=g),
               torch.randint(0, 86, (10, 12), generator=g),
               torch.randint(0, 86, (7, 12), generator=g)]
    runs = []
    for on in (False, True):
        model = _char_gru()
        rec = []
        with _flag(on):
            for x in batches:
                y = model(x)
                assert y.shape == (x.size(0), 86, 12)
                assert model.hidden.shape == (1, x.size(0), 50)
                assert not model.hidden.requires_grad
                rec.append((y.detach().clone(), model.hidden.clone()))
        runs.append(rec)
    for (y0, h0), (y1, h1) in zip(*runs):
        assert torch.equal(y0, y1) and torch.equal(h0, h1)
    # the stock module gives the same: forward is gru(emb, hidden)
    model = _char_gru()
    emb = model.encoder(batches[0])
    out, h = model.gru(emb, torch.zeros(1, 10, 50))
    assert torch.equal(model.decoder(out).permute(0, 2, 1), runs[0][0][0])
    assert torch.equal(h, runs[0][0][1])


def test_char_gru_routes_through_gru_seq(monkeypatch):
    import importlib
    rnn = importlib.import_module('fedtorch_amd.components.models.rnn')
    seen = []

    def spy(gru, x, h0):
        seen.append((gru, tuple(x.shape), tuple(h0.shape),
                     h0.requires_grad))
        return gru(x, h0)

    monkeypatch.setattr(rnn, 'gru_seq', spy)
    model = _char_gru()
    model(torch.zeros(10, 4, dtype=torch.long))
    model(torch.zeros(10, 4, dtype=torch.long))
    assert seen == [(model.gru, (10, 4, 50), (1, 10, 50), False)] * 2


def _eligible_setup(monkeypatch, **kw):
    """a call for which everything but the named deviation is eligible; on a
    host without a GPU the extension counts as present and, with ``cuda``,
    _kernels_active does not ask the tensor where it lives"""
    monkeypatch.setattr(ops, '_C', SimpleNamespace())
    monkeypatch.setattr(ops, 'FORCE_EAGER', False)
    H = kw.pop('H', 50)
    gru = nn.GRU(H, H, kw.pop('layers', 1),
                 batch_first=kw.pop('batch_first', True),
                 bias=kw.pop('bias', True),
                 bidirectional=kw.pop('bidirectional', False))
    x = torch.randn(4, 5, H)
    h0 = torch.zeros(kw.pop('h0_shape', (1, 4, H)))
    assert not kw
    return gru, x, h0


def _eligible(monkeypatch, cuda=True, **kw):
    gru, x, h0 = _eligible_setup(monkeypatch, **kw)
    monkeypatch.setattr(
        fgru, '_kernels_active',
        (lambda t: ops.hip_available() and not ops.FORCE_EAGER) if cuda
        else _REAL_ACTIVE)
    return fgru.gru_eligible(gru, x, h0)


def test_gru_eligible_truth_table(monkeypatch):
    with _flag(True):
        assert _eligible(monkeypatch)
        assert _eligible(monkeypatch, H=64)
        assert _eligible(monkeypatch, H=1)
        assert not _eligible(monkeypatch, cuda=False)          # CPU tensor
        assert not _eligible(monkeypatch, layers=2)
        assert not _eligible(monkeypatch, bidirectional=True,
                             h0_shape=(2, 4, 50))
        assert not _eligible(monkeypatch, bidirectional=True)
        assert not _eligible(monkeypatch, batch_first=False)
        assert not _eligible(monkeypatch, bias=False)
        assert not _eligible(monkeypatch, H=65)
        assert not _eligible(monkeypatch, h0_shape=(1, 5, 50))
        assert not _eligible(monkeypatch, h0_shape=(4, 50))
        assert not _eligible(monkeypatch, h0_shape=(2, 4, 50))
        monkeypatch.setattr(ops, 'FORCE_EAGER', True)
        gru, x, h0 = nn.GRU(50, 50, batch_first=True), \
            torch.randn(4, 5, 50), torch.zeros(1, 4, 50)
        assert not fgru.gru_eligible(gru, x, h0)
    with _flag(False):
        assert not _eligible(monkeypatch)                      # flag off


def test_gru_eligible_needs_extension(monkeypatch):
    with _flag(True):
        gru, x, h0 = _eligible_setup(monkeypatch)
        monkeypatch.setattr(ops, '_C', None)
        monkeypatch.setattr(fgru, '_kernels_active',
                            lambda t: ops.hip_available()
                            and not ops.FORCE_EAGER)
        assert not fgru.gru_eligible(gru, x, h0)
