# -*- coding: utf-8 -*-
"""Token-input char-GRU on the GPU (gru_tok_fwd / gru_tok_wide_fwd,
gru_tok_grads, CharGRU with FEDTORCH_FUSED_GRU_TOKENS) against float64
references; references and tolerance of tests/gru_cases.py."""
import copy

import pytest
import torch
import torch.nn.functional as F

import gru_cases as gc
import fedtorch_amd.ops as ops
from fedtorch_amd.components.models.rnn import CharGRU
from fedtorch_amd.ops import gru as fgru

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64


def _dev(t, dtype=F32):
    return t.to(dtype).cuda().contiguous()


def _tokens(g, B, T, V, pattern):
    """'equal': one token everywhere; 'ends': random with rows 0 and V - 1
    present; 'oob': 'ends' with one token = V and one = -1"""
    if pattern == 'equal':
        return torch.full((B, T), V // 2, dtype=torch.int64)
    tok = torch.randint(0, V, (B, T), generator=g)
    flat = tok.view(-1)
    flat[0], flat[-1] = 0, V - 1
    if pattern == 'oob':
        flat[flat.numel() // 2] = V
        flat[-1] = -1
    return tok


def _gather(P, tok):
    """P[tok] with zero rows where the token is outside [0, V)"""
    ok = (tok >= 0) & (tok < P.size(0))
    return P[tok.clamp(0, P.size(0) - 1)] * ok.unsqueeze(-1).to(P.dtype)


@pytest.mark.parametrize('pattern', ['equal', 'ends', 'oob'])
@pytest.mark.parametrize('V', [1, 86])
@pytest.mark.parametrize('T', [1, 2, 3])
@pytest.mark.parametrize('B,H', [(1, 1), (17, 50), (16, 64), (17, 65),
                                 (3, 128)])
def test_fwd(B, H, T, V, pattern):
    g = gc.gen('tok fwd', B, H, T, V, pattern)
    k = H ** -0.5
    w = ((torch.rand(3 * H, H, generator=g) * 2 - 1) * k).to(F64)
    b = ((torch.rand(3 * H, generator=g) * 2 - 1) * k).to(F64)
    P = torch.randn(V, 3 * H, generator=g).to(F64)
    h0 = (torch.rand(B, H, generator=g) * 2 - 1).to(F64)
    tok = _tokens(g, B, T, V, pattern)
    wide = H > fgru.MAX_H
    tok_fwd = ops._C.gru_tok_wide_fwd if wide else ops._C.gru_tok_fwd
    flt_fwd = ops._C.gru_wide_fwd if wide else ops._C.gru_fwd
    Pd = gc.nan_framed(_dev(P))
    out, gates = tok_fwd(Pd, tok.cuda(), _dev(w), _dev(b), _dev(h0), True)
    assert out.shape == (B, T, H) and gates.shape == (B, T, 4, H)
    # the same arithmetic in the same order: bit equality
    want = flt_fwd(_gather(Pd, tok.cuda()).contiguous(), _dev(w), _dev(b),
                   _dev(h0), True)
    assert torch.equal(out, want[0]) and torch.equal(gates, want[1])
    gx = _gather(P.float().double(), tok)
    ref64, ref32 = (gc.ref_fwd(gx, w, b, h0, dt) for dt in (F64, F32))
    for got, r64, r32 in zip((out, gates), ref64, ref32):
        tol, _ = gc.tolerance(r64, r32)
        err = (got.double().cpu() - r64).abs().max().item()
        print('err %.3e tol %.3e' % (err, tol))
        assert err <= tol


@pytest.mark.parametrize('exact', [True, False])
@pytest.mark.parametrize('B,T,H,V', [(1, 1, 1, 1), (3, 5, 50, 86),
                                     (17, 3, 65, 17), (2, 130, 128, 33)])
def test_tok_grads(B, T, H, V, exact):
    """exact: integers in [-4, 4], every sum below 2^24 (at most 16 * 260),
    so fp32 == float64 whatever the order.  Else random fp32 values within
    the ordered-summation bound gamma_K sum |a_i b_i|, K = B T."""
    g = gc.gen('tok grads', B, T, H, V, exact)

    def val(*shape):
        if exact:
            return gc.ints(g, -4, 4, *shape)
        return torch.randn(*shape, generator=g).to(F32).to(F64)

    dgx, dgh = val(B, T, 3 * H), val(B, T, 3 * H)
    out, h0 = val(B, T, H), val(B, H)
    tok = _tokens(g, B, T, V, 'oob' if B * T > 1 else 'ends')
    R = B * T
    hp = torch.cat((h0.unsqueeze(1), out[:, :-1]), dim=1).reshape(R, H)
    ok = ((tok >= 0) & (tok < V)).view(R)
    a, x = dgh.reshape(R, 3 * H), dgx.reshape(R, 3 * H)[ok]

    def sums(a, hp, x):
        dP = torch.zeros(V, 3 * H, dtype=F64)
        return dP.index_add_(0, tok.view(R)[ok], x), a.t() @ hp, a.sum(0)

    want = sums(a, hp, x)
    got = ops._C.gru_tok_grads(_dev(dgx), _dev(dgh), _dev(out), _dev(h0),
                               tok.cuda(), V)
    u = 2.0 ** -24
    bound = sums(a.abs(), hp.abs(), x.abs())
    for name, gt, wt, bd in zip(('dP', 'dW_hh', 'db_hh'), got, want, bound):
        assert gt.shape == wt.shape, name
        if exact:
            assert torch.equal(gt.cpu(), wt.float()), name
        else:
            err = (gt.double().cpu() - wt).abs()
            assert bool((err <= R * u / (1 - R * u) * bd).all()), name
    if R < V:                    # rows no token selects: exact zeros
        unused = torch.ones(V, dtype=torch.bool)
        unused[tok.view(R)[ok]] = False
        assert unused.any() and not got[0][unused.cuda()].any()


def test_deterministic_and_graph_capture():
    B, T, H, V = 10, 50, 50, 86
    c = gc.random_case(B, T, H)
    P = _dev(torch.randn(V, 3 * H, generator=gc.gen('tok graph')))
    tok = _tokens(gc.gen('tok graph', 1), B, T, V, 'ends').cuda()
    w, b, h0, dout = (_dev(c[k]) for k in ('w', 'b', 'h0', 'dout'))

    def step():
        out, gates = ops._C.gru_tok_fwd(P, tok, w, b, h0, True)
        dgx, dgh, dh0 = ops._C.gru_bwd(dout, out, gates, w, h0)
        return (out, gates, dgx, dh0) + tuple(
            ops._C.gru_tok_grads(dgx, dgh, out, h0, tok, V))

    eager = step()
    for x, y in zip(eager, step()):
        assert torch.equal(x, y)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for _ in range(2):
        for t in outs:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(outs, eager):
            assert torch.equal(got, want)


def test_launcher_rejections():
    def z(*shape, **kw):
        return torch.zeros(*shape, device='cuda', **kw)

    B, T, V = 3, 2, 5
    for H, good, other in ((17, ops._C.gru_tok_fwd, ops._C.gru_tok_wide_fwd),
                           (65, ops._C.gru_tok_wide_fwd, ops._C.gru_tok_fwd)):
        P, tok = z(V, 3 * H), z(B, T, dtype=torch.int64)
        w, b, h0 = z(3 * H, H), z(3 * H), z(B, H)
        good(P, tok, w, b, h0, True)
        bad = [(P.double(), tok, w, b, h0), (P, tok.int(), w, b, h0),
               (P, tok, w.half(), b, h0),
               (z(V, 6 * H)[:, ::2], tok, w, b, h0),           # contiguity
               (P, z(T, B, dtype=torch.int64).t(), w, b, h0),
               (z(V, 3 * H + 1), tok, w, b, h0),               # shapes
               (P, tok.view(-1), w, b, h0), (P, tok, w, b, z(B + 1, H)),
               (P.cpu(), tok, w, b, h0), (P, tok.cpu(), w, b, h0),
               (z(0, 3 * H), tok, w, b, h0),                   # V = 0
               (P, z(0, T, dtype=torch.int64), w, b, z(0, H))]
        for args in bad:
            with pytest.raises(RuntimeError):
                good(*args, True)
        with pytest.raises(RuntimeError):                      # 64 | 65
            other(P, tok, w, b, h0, True)
    H = 17
    dg, out, h0 = z(B, T, 3 * H), z(B, T, H), z(B, H)
    tok = z(B, T, dtype=torch.int64)
    ops._C.gru_tok_grads(dg, dg, out, h0, tok, V)
    bad = [(dg.double(), dg, out, h0, tok, V), (dg, dg, out, h0, tok.int(), V),
           (dg, z(B, T, 6 * H)[:, :, ::2], out, h0, tok, V),
           (dg, dg, out, h0, z(T, B, dtype=torch.int64).t(), V),
           (dg, dg, out, h0, z(B, T + 1, dtype=torch.int64), V),
           (z(B, T, 3 * H + 3), dg, out, h0, tok, V),
           (dg.cpu(), dg, out, h0, tok, V), (dg, dg, out, h0, tok.cpu(), V),
           (dg, dg, out, h0, tok, 0),
           (z(B, T, 3 * 129), z(B, T, 3 * 129), z(B, T, 129), z(B, 129), tok,
            V)]
    for args in bad:
        with pytest.raises(RuntimeError):
            ops._C.gru_tok_grads(*args)
    torch.cuda.synchronize()


@pytest.mark.parametrize('H,tokens,want', [
    (50, True, ['gru_tok_fwd', 'gru_bwd', 'gru_tok_grads']),
    (50, False, ['gru_fwd', 'gru_bwd']),
    (128, True, ['gru_tok_wide_fwd', 'gru_wide_bwd', 'gru_tok_grads'])])
def test_char_gru_matches_float64_model(monkeypatch, H, tokens, want):
    """logits, the seven parameter gradients and the carried hidden state over
    two batches, within tolerance(float64 copy, fp32 CPU copy); the recorded
    ops._C calls of each batch are ``want``"""
    calls = []
    for name in ('gru_fwd', 'gru_bwd', 'gru_wide_fwd', 'gru_wide_bwd',
                 'gru_tok_fwd', 'gru_tok_wide_fwd', 'gru_tok_grads'):
        monkeypatch.setattr(
            ops._C, name, lambda *a, _f=getattr(ops._C, name), _n=name:
            (calls.append(_n), _f(*a))[1])
    monkeypatch.setattr(fgru, '_GRU_ENABLED', True)
    monkeypatch.setattr(fgru, '_GRU_WIDE_ENABLED', H > 64)
    monkeypatch.setattr(fgru, '_GRU_TOK_ENABLED', tokens)
    torch.manual_seed(11)
    m32 = CharGRU('shakespeare', 86, H, 86, 10)
    m64, mgpu = copy.deepcopy(m32).double(), copy.deepcopy(m32).cuda()
    m64.init_hidden(10)
    mgpu.init_hidden(10)
    g = torch.Generator().manual_seed(12)
    for step in range(2):
        x = torch.randint(0, 86, (10, 4), generator=g)
        y = torch.randint(0, 86, (10, 4), generator=g)
        res = []
        for m, dev in ((m64, 'cpu'), (m32, 'cpu'), (mgpu, 'cuda')):
            m.zero_grad(set_to_none=True)
            logits = m(x.to(dev))
            F.cross_entropy(logits, y.to(dev)).backward()
            r = {'logits': logits.detach(), 'hidden': m.hidden}
            r.update(('d ' + n, p.grad) for n, p in m.named_parameters())
            res.append(r)
        r64, r32, rg = res
        assert len(r64) == 9
        for name, ref in r64.items():
            tol, _ = gc.tolerance(ref, r32[name])
            err = (rg[name].double().cpu() - ref).abs().max().item()
            print('batch %d %s err %.3e tol %.3e' % (step, name, err, tol))
            assert err <= tol, (step, name, err, tol)
    assert calls == want * 2
