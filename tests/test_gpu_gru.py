# -*- coding: utf-8 -*-
"""GRU sequence kernels (hip/gru.h) on the GPU against the float64 step-loop
reference of tests/gru_cases.py: gru_fwd / gru_bwd exact cases (operand maps,
time indexing, backward, padding) and random companions, determinism,
launcher argument checks, and ops.gru.gru_seq / CharGRU at module level
(FEDTORCH_FUSED_GRU): numerics against a float64 CPU copy, routing, parameter
gradient dtypes, graph capture.

Measured on an MI355X, worst kernel error / e32 over the random cases (bound
4, plus the 16-ulp floor): see profiles/gru_notes.md."""
import contextlib
import copy
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import gru_cases as gc
import fedtorch_amd.ops as ops
from fedtorch_amd.components.models.rnn import CharGRU
from fedtorch_amd.ops import gru as fgru

pytestmark = pytest.mark.gpu

F32 = torch.float32
DT = gc.DTYPES
WDT = ['fp32', 'bf16']


@pytest.fixture
def calls(monkeypatch):
    """list of (name, args) of the recorded ops._C GRU calls"""
    rec = []
    for name in ('gru_fwd', 'gru_bwd'):
        fn = getattr(ops._C, name)
        monkeypatch.setattr(
            ops._C, name,
            lambda *a, _fn=fn, _n=name: (rec.append((_n, a)), _fn(*a))[1])
    return rec


@contextlib.contextmanager
def _flag(on):
    old = fgru._GRU_ENABLED
    fgru._GRU_ENABLED = on
    try:
        yield
    finally:
        fgru._GRU_ENABLED = old


def _dev(t, dtype=F32):
    return t.to(dtype).cuda().contiguous()


def _fwd(gx, w, b, h0, save=True, wdt='fp32', bdt=None):
    return ops._C.gru_fwd(_dev(gx), _dev(w, DT[wdt]), _dev(b, DT[bdt or wdt]),
                          _dev(h0), save)


def _within(got, want64, tol, e32, what):
    err = (got.detach().double().cpu() - want64).abs().max().item()
    print('%s: err %.3e  e32 %.3e  err/e32 %.3f  err/tol %.3f' % (
        what, err, e32, err / e32 if e32 else float('inf') if err else 0.0,
        err / tol if tol else float('inf') if err else 0.0))
    assert err <= tol, (what, err, tol)


# --------------------------------------------------------------------------
# exact cases
# --------------------------------------------------------------------------
@pytest.mark.parametrize('wdt', WDT)
@pytest.mark.parametrize('B', gc.MAP_B)
@pytest.mark.parametrize('H', gc.MAP_H)
def test_fwd_exact_operand_maps(H, B, wdt):
    gx, w, b, h0, out, gates = gc.map_case(B, H)
    got_out, got_g = _fwd(gx, w, b, h0, True, wdt)
    assert got_out.dtype == got_g.dtype == F32
    assert got_out.shape == (B, 1, H) and got_g.shape == (B, 1, 4, H)
    assert got_out.is_contiguous() and got_g.is_contiguous()
    assert torch.equal(got_g[:, :, 3].cpu(), gates[:, :, 3].float())
    # r and z come from the two other accumulator tiles.  Their arguments
    # are an exact integer plus gx, rounded once (<= 2^-24 |a|), and
    # |sigmoid'(a) a| < 0.23, so beyond the exp / division error (a few ulps
    # of 1/4 and of 1) they sit within 2^-26 of the reference: 2^-20 leaves
    # those some 15 ulps of 1.  n = tanh(gx_n + r q) is 1-Lipschitz in r q
    # (+ one rounding of an argument below |q| + 8), out = (1-z) n + z h0
    # with |n| <= 1, |h0| <= 4.
    err = (got_g.double().cpu() - gates).abs()
    er = err[:, :, :2].max().item()
    assert er <= 2.0 ** -20
    qmax = gates[:, :, 3].abs().max().item()
    en = err[:, :, 2].max().item()
    assert en <= 2.0 ** -20 * qmax + 2.0 ** -24 * (qmax + 8) + 2.0 ** -21
    assert (got_out.double().cpu() - out).abs().max().item() \
        <= 2.0 ** -20 * qmax + 2.0 ** -24 * (qmax + 8) + 2.0 ** -21 \
        + 5 * 2.0 ** -20 + 2.0 ** -21
    # without save_gates: the same out, an empty gates tensor
    out2, g2 = _fwd(gx, w, b, h0, False, wdt)
    assert g2.numel() == 0 and torch.equal(out2, got_out)


@pytest.mark.parametrize('T', gc.TIME_T)
@pytest.mark.parametrize('B,H', gc.TIME_BH)
def test_fwd_exact_time_indexing(B, H, T):
    gx, w, b, h0, out = gc.time_case(B, T, H)
    got_out, got_g = _fwd(gx, w, b, h0)
    assert got_out.shape == (B, T, H) and got_g.shape == (B, T, 4, H)
    assert torch.equal(got_out.cpu(), out.float())
    assert torch.equal(got_g[:, :, :2].cpu(), torch.full((B, T, 2, H), .5))
    assert not got_g[:, :, 2:].any()


@pytest.mark.parametrize('wdt', WDT)
@pytest.mark.parametrize('T', gc.BWD_T)
@pytest.mark.parametrize('B,H', gc.BWD_BH)
def test_bwd_exact(B, H, T, wdt):
    dout, out, gates, w, h0, ref = gc.bwd_case(B, T, H)
    dgx, dgh, dh0 = ops._C.gru_bwd(_dev(dout), _dev(out), _dev(gates),
                                   _dev(w, DT[wdt]), _dev(h0))
    for got, name, shape in ((dgx, 'dgx', (B, T, 3 * H)),
                             (dgh, 'dgh', (B, T, 3 * H)),
                             (dh0, 'dh0', (B, H))):
        assert got.dtype == F32 and got.shape == shape, name
        assert got.is_contiguous(), name
        assert torch.equal(got.cpu(), ref[name].float()), name


@pytest.mark.parametrize('wdt', WDT)
@pytest.mark.parametrize('B,T,H', gc.PAD_SHAPES)
def test_padding_never_read(B, T, H, wdt):
    g = gc.gen('pad', B, T, H)
    gx = torch.randn(B, T, 3 * H, generator=g)
    h0 = torch.rand(B, H, generator=g) * 2 - 1
    dout = torch.randn(B, T, H, generator=g)
    w = (torch.rand(3 * H, H, generator=g) * 2 - 1) / H ** .5
    b = (torch.rand(3 * H, generator=g) * 2 - 1) / H ** .5
    plain = [t.cuda() for t in (gx, w.to(DT[wdt]), b.to(DT[wdt]), h0, dout)]
    framed = [gc.nan_framed(t) for t in plain]
    for t, f in zip(plain, framed):
        assert torch.equal(t, f) and f.is_contiguous()

    def run(gx, w, b, h0, dout):
        out, gates = ops._C.gru_fwd(gx, w, b, h0, True)
        return (out, gates) + tuple(ops._C.gru_bwd(dout, out, gates, w, h0))

    want, got = run(*plain), run(*framed)
    for a, b_ in zip(want, got):
        assert not torch.isnan(b_).any() and not torch.isinf(b_).any()
        assert torch.equal(a, b_)


# --------------------------------------------------------------------------
# random companions
# --------------------------------------------------------------------------
@pytest.mark.parametrize('B,T,H', gc.RANDOM)
def test_random(B, T, H):
    c = gc.random_case(B, T, H)
    ref, tol, e32 = c['ref'], c['tol'], c['e32']
    out, gates = _fwd(c['gx'], c['w'], c['b'], c['h0'])
    h0 = _dev(c['h0'])
    dgx, dgh, dh0 = ops._C.gru_bwd(_dev(c['dout']), out, gates,
                                   _dev(c['w']), h0)
    got = dict(out=out, gates=gates, dgx=dgx, dgh=dgh, dh0=dh0,
               dw=fgru.hh_weight_grad(dgh, out, h0),
               db=fgru.hh_bias_grad(dgh))
    bad = []
    for name in ('out', 'gates', 'dgx', 'dgh', 'dh0', 'dw', 'db'):
        assert got[name].shape == ref[name].shape, name
        try:
            _within(got[name], ref[name], tol[name], e32[name],
                    '(%d,%d,%d) %s' % (B, T, H, name))
        except AssertionError as e:
            bad.append(e.args[0])
    assert not bad, bad


def test_random_bf16_weights():
    """bf16 w_hh / b_hh are widened while staged: the result is that of the
    fp32 kernel on the widened values, bit for bit"""
    B, T, H = 17, 2, 17
    c = gc.random_case(B, T, H)
    w16, b16 = c['w'].to(torch.bfloat16), c['b'].to(torch.bfloat16)
    a = _fwd(c['gx'], w16.double(), b16.double(), c['h0'])
    for wdt, bdt in (('bf16', 'bf16'), ('bf16', 'fp32'), ('fp32', 'bf16')):
        b_ = _fwd(c['gx'], w16.double(), b16.double(), c['h0'], True, wdt,
                  bdt)
        assert torch.equal(a[0], b_[0]) and torch.equal(a[1], b_[1])
    h0, dout = _dev(c['h0']), _dev(c['dout'])
    ga = ops._C.gru_bwd(dout, a[0], a[1], w16.float().cuda(), h0)
    gb = ops._C.gru_bwd(dout, a[0], a[1], w16.cuda(), h0)
    for x, y in zip(ga, gb):
        assert torch.equal(x, y)


def test_deterministic():
    c = gc.random_case(10, 50, 50)
    runs = []
    for _ in range(2):
        out, gates = _fwd(c['gx'], c['w'], c['b'], c['h0'])
        runs.append((out, gates) + tuple(ops._C.gru_bwd(
            _dev(c['dout']), out, gates, _dev(c['w']), _dev(c['h0']))))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# --------------------------------------------------------------------------
# launcher argument checks
# --------------------------------------------------------------------------
def _good(B=3, T=2, H=17):
    gx = torch.zeros(B, T, 3 * H, device='cuda')
    w = torch.zeros(3 * H, H, device='cuda')
    b = torch.zeros(3 * H, device='cuda')
    h0 = torch.zeros(B, H, device='cuda')
    return gx, w, b, h0


def test_fwd_argument_checks():
    B, T, H = 3, 2, 17
    gx, w, b, h0 = _good(B, T, H)
    ops._C.gru_fwd(gx, w, b, h0, False)
    bad = [
        (gx.double(), w, b, h0),                              # dtype
        (gx.half(), w, b, h0),
        (gx, w.half(), b, h0),
        (gx, w, b.double(), h0),
        (gx, w, b, h0.bfloat16()),
        (gx.transpose(0, 1), w, b, h0),                       # contiguity
        (torch.zeros(B, T, 6 * H, device='cuda')[:, :, ::2], w, b, h0),
        (gx, torch.zeros(H, 3 * H, device='cuda').t(), b, h0),
        (gx, w, torch.zeros(6 * H, device='cuda')[::2], h0),
        (gx, w, b, torch.zeros(H, B, device='cuda').t()),
        (gx, torch.zeros(3 * H + 1, H, device='cuda'), b, h0),  # shapes
        (gx, torch.zeros(3 * H, H + 1, device='cuda'), b, h0),
        (gx, w, torch.zeros(3 * H + 1, device='cuda'), h0),
        (torch.zeros(B, T, 3 * H + 1, device='cuda'), w, b, h0),
        (gx, w, b, torch.zeros(B + 1, H, device='cuda')),     # B mismatch
        (gx, w, b, torch.zeros(1, B, H, device='cuda')),
        (gx.cpu(), w, b, h0),                                 # device
        (gx, w.cpu(), b, h0),
        (gx, w, b.cpu(), h0),
        (gx, w, b, h0.cpu()),
        _good(B, T, 65),                                      # H limit
        (torch.zeros(0, T, 3 * H, device='cuda'), w, b,
         torch.zeros(0, H, device='cuda')),                   # empty
        (torch.zeros(B, 0, 3 * H, device='cuda'), w, b, h0),
    ]
    for args in bad:
        with pytest.raises(RuntimeError):
            ops._C.gru_fwd(*args, True)
    torch.cuda.synchronize()


def test_bwd_argument_checks():
    B, T, H = 3, 2, 17
    _, w, _, h0 = _good(B, T, H)
    out = torch.zeros(B, T, H, device='cuda')
    dout = torch.zeros(B, T, H, device='cuda')
    gates = torch.zeros(B, T, 4, H, device='cuda')
    ops._C.gru_bwd(dout, out, gates, w, h0)
    H65 = 65
    bad = [
        (dout.double(), out, gates, w, h0),                   # dtype
        (dout, out.half(), gates, w, h0),
        (dout, out, gates.double(), w, h0),
        (dout, out, gates, w.half(), h0),
        (dout, out, gates, w, h0.bfloat16()),
        (torch.zeros(T, B, H, device='cuda').transpose(0, 1), out, gates, w,
         h0),                                                 # contiguity
        (dout, torch.zeros(B, T, 2 * H, device='cuda')[:, :, ::2], gates, w,
         h0),
        (dout, out, torch.zeros(B, T, H, 4, device='cuda').transpose(2, 3),
         w, h0),
        (dout, out, gates, torch.zeros(H, 3 * H, device='cuda').t(), h0),
        (dout, out, gates, torch.zeros(3 * H + 1, H, device='cuda'), h0),
        (dout, out, torch.zeros(B, T, 3, H, device='cuda'), w, h0),
        (dout, out, torch.zeros(0, device='cuda'), w, h0),    # no gates
        (torch.zeros(B + 1, T, H, device='cuda'), out, gates, w, h0),
        (dout, out, gates, w, torch.zeros(B + 1, H, device='cuda')),
        (dout.cpu(), out, gates, w, h0),                      # device
        (dout, out.cpu(), gates, w, h0),
        (dout, out, gates.cpu(), w, h0),
        (dout, out, gates, w.cpu(), h0),
        (dout, out, gates, w, h0.cpu()),
        (torch.zeros(B, T, H65, device='cuda'),
         torch.zeros(B, T, H65, device='cuda'),
         torch.zeros(B, T, 4, H65, device='cuda'),
         torch.zeros(3 * H65, H65, device='cuda'),
         torch.zeros(B, H65, device='cuda')),                 # H limit
    ]
    for args in bad:
        with pytest.raises(RuntimeError):
            ops._C.gru_bwd(*args)
    torch.cuda.synchronize()


# --------------------------------------------------------------------------
# module level
# --------------------------------------------------------------------------
def _char_models():
    torch.manual_seed(11)
    m32 = CharGRU('shakespeare', 86, 50, 86, 10)
    m64 = copy.deepcopy(m32).double()
    m64.init_hidden(10)
    mgpu = copy.deepcopy(m32).cuda()
    mgpu.init_hidden(10)
    return m64, m32, mgpu


def test_char_gru_matches_float64_model(calls):
    """logits, every parameter gradient and the carried hidden state over two
    consecutive batches; e32 comes from the fp32 CPU copy of the model"""
    m64, m32, mgpu = _char_models()
    g = torch.Generator().manual_seed(12)
    bad = []
    with _flag(True):
        for step in range(2):
            x = torch.randint(0, 86, (10, 50), generator=g)
            y = torch.randint(0, 86, (10, 50), generator=g)
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
            assert rg['logits'].dtype == F32 and rg['hidden'].dtype == F32
            assert rg['hidden'].shape == (1, 10, 50)
            assert not rg['hidden'].requires_grad
            for name, want in r64.items():
                tol, e32 = gc.tolerance(want, r32[name])
                try:
                    _within(rg[name], want, tol, e32,
                            'batch %d %s' % (step, name))
                except AssertionError as e:
                    bad.append(e.args[0])
    assert [n for n, _ in calls] == ['gru_fwd', 'gru_bwd'] * 2
    assert not bad, bad


def _pair(H=50, B=4, T=5, dtype=F32):
    torch.manual_seed(H)
    gru = nn.GRU(H, H, batch_first=True).cuda().to(dtype)
    x = torch.randn(B, T, H, device='cuda')
    h0 = torch.randn(1, B, H, device='cuda')
    return gru, x, h0


def test_routing(calls):
    gru, x, h0 = _pair()
    with _flag(True):
        assert fgru.gru_eligible(gru, x, h0)
        out, hn = fgru.gru_seq(gru, x, h0)
        assert [n for n, _ in calls] == ['gru_fwd']
        assert calls[0][1][4] is True                 # training: save gates
        assert out.shape == (4, 5, 50) and hn.shape == (1, 4, 50)
        assert torch.equal(hn[0], out[:, -1])
        out.sum().backward()
        assert [n for n, _ in calls] == ['gru_fwd', 'gru_bwd']
        want_out, want_hn = gru(x, h0)
        assert torch.allclose(out, want_out, atol=1e-5)
        del calls[:]
        # eval without grad: one launch, no gates
        with torch.no_grad():
            out2, _ = fgru.gru_seq(gru, x, h0)
        assert [n for n, _ in calls] == ['gru_fwd']
        assert calls[0][1][4] is False
        assert torch.equal(out2, out)
        del calls[:]
        # bf16 autocast: still fp32 out / h_n
        with torch.autocast('cuda', dtype=torch.bfloat16):
            out3, hn3 = fgru.gru_seq(gru, x, h0)
        assert out3.dtype == hn3.dtype == F32 and torch.equal(out3, out)
        del calls[:]
        # H = 65: the library path
        gru65, x65, h65 = _pair(H=65)
        assert not fgru.gru_eligible(gru65, x65, h65)
        o65, hn65 = fgru.gru_seq(gru65, x65, h65)
        w65, whn65 = gru65(x65, h65)
        assert torch.equal(o65, w65) and torch.equal(hn65, whn65)
        assert calls == []
        # forced eager
        ops.FORCE_EAGER = True
        try:
            assert not fgru.gru_eligible(gru, x, h0)
            fgru.gru_seq(gru, x, h0)
        finally:
            ops.FORCE_EAGER = False
        assert calls == []
    with _flag(False):
        o, h = fgru.gru_seq(gru, x, h0)
        assert torch.equal(o, want_out) and torch.equal(h, want_hn)
    assert calls == []


def test_char_gru_routing(calls):
    _, _, mgpu = _char_models()
    x = torch.zeros(10, 50, dtype=torch.long, device='cuda')
    with _flag(True):
        mgpu(x)
        mgpu(x[:7])
        assert [n for n, _ in calls] == ['gru_fwd', 'gru_fwd']
        assert mgpu.hidden.shape == (1, 7, 50)
    del calls[:]
    with _flag(False):
        mgpu(x)
    assert calls == []


def test_bf16_parameters_get_bf16_grads():
    gru, x, h0 = _pair(H=50, B=5, T=3, dtype=torch.bfloat16)
    x.requires_grad_(True)
    with _flag(True):
        assert fgru.gru_eligible(gru, x, h0)
        out, _ = fgru.gru_seq(gru, x, h0)
        assert out.dtype == F32
        dout = torch.randn_like(out)
        out.backward(dout)
    for p in gru.parameters():
        assert p.grad.dtype == torch.bfloat16 and p.grad.shape == p.shape
    assert x.grad.dtype == F32
    # the Function itself returns bf16, rounded to nearest even from fp32
    w, b = gru.weight_hh_l0.detach(), gru.bias_hh_l0.detach()
    hh = h0[0].contiguous()
    with torch.no_grad():
        gx = F.linear(x.detach(), gru.weight_ih_l0.float(),
                      gru.bias_ih_l0.float())
        o, gates = ops._C.gru_fwd(gx, w, b, hh, True)
        assert torch.equal(o, out)
        ctx = SimpleNamespace(saved_tensors=(o, gates, w, hh),
                              needs_input_grad=(True, True, True, True, False),
                              b_dtype=b.dtype)
        dgx, dw, db, dh0, _ = fgru._GRUSeqFn.backward(ctx, dout)
        _, dgh, _ = ops._C.gru_bwd(dout, o, gates, w, hh)
    assert dw.dtype == db.dtype == torch.bfloat16
    assert torch.equal(dw, fgru.hh_weight_grad(dgh, o, hh).to(torch.bfloat16))
    assert torch.equal(db, fgru.hh_bias_grad(dgh).to(torch.bfloat16))
    assert torch.equal(dw, gru.weight_hh_l0.grad)
    assert torch.equal(db, gru.bias_hh_l0.grad)


def test_graph_capture():
    gru, x, h0 = _pair(H=50, B=10, T=50)
    x.requires_grad_(True)
    h0.requires_grad_(True)
    dout = torch.randn(10, 50, 50, device='cuda')
    leaves = (x, h0) + tuple(gru.parameters())

    def step():
        # nothing returned keeps the autograd graph alive (a surviving graph
        # would make the engine sync the capture stream with the stream the
        # leaves' AccumulateGrad nodes were made on)
        out, hn = fgru.gru_seq(gru, x, h0)
        grads = torch.autograd.grad(out, leaves, dout)
        return (out.detach(), hn.detach().clone()) + grads

    with _flag(True):
        eager = [t.clone() for t in step()]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                step()
        torch.cuda.current_stream().wait_stream(side)
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
