# -*- coding: utf-8 -*-
"""Streamed-weight GRU sequence kernels (hip/gru_stream.h, 129 <= H <= 256) on
the GPU against the float64 reference of tests/gru_cases.py, and gru_seq
under FEDTORCH_FUSED_GRU_STREAM.  Measured errors: profiles/gru_notes.md."""
import copy

import pytest
import torch
import torch.nn as nn

import gru_cases as gc
import fedtorch_amd.ops as ops
from fedtorch_amd.ops import gru as fgru

pytestmark = pytest.mark.gpu

F32 = torch.float32
WDT = ['fp32', 'bf16']
# NT = 9 and 16, a full tile and one column past it; 1 row, partial tiles;
# H = 144, 192, 256 take the 16-byte weight loads, the others element loads
BH = [(1, 129), (17, 144), (3, 145), (16, 192), (3, 193), (17, 241),
      (33, 256)]


def _dev(t, dtype=F32):
    return t.to(dtype).cuda().contiguous()


def _fwd(gx, w, b, h0, save=True, wdt='fp32'):
    dt = gc.DTYPES[wdt]
    return ops._C.gru_stream_fwd(_dev(gx), _dev(w, dt), _dev(b, dt),
                                 _dev(h0), save)


def _within(got, want64, tol, e32, what):
    err = (got.detach().double().cpu() - want64).abs().max().item()
    print('%s: err %.3e  e32 %.3e  err/e32 %.3f  err/tol %.3f' % (
        what, err, e32, err / e32 if e32 else 0.0, err / tol))
    return [] if err <= tol else [(what, err, tol)]


@pytest.mark.parametrize('wdt', WDT)
@pytest.mark.parametrize('B,H', BH)
def test_fwd_exact_operand_maps(B, H, wdt):
    gx, w, b, h0, out, gates = gc.map_case(B, H)
    got_out, got_g = _fwd(gx, w, b, h0, True, wdt)
    assert got_out.dtype == got_g.dtype == F32 and got_g.is_contiguous()
    assert got_out.shape == (B, 1, H) and got_g.shape == (B, 1, 4, H)
    assert torch.equal(got_g[:, :, 3].cpu(), gates[:, :, 3].float())
    # bounds derived in test_gpu_gru.py::test_fwd_exact_operand_maps
    err = (got_g.double().cpu() - gates).abs()
    assert err[:, :, :2].max().item() <= 2.0 ** -20
    qmax = gates[:, :, 3].abs().max().item()
    bn = 2.0 ** -20 * qmax + 2.0 ** -24 * (qmax + 8) + 2.0 ** -21
    assert err[:, :, 2].max().item() <= bn
    assert (got_out.double().cpu() - out).abs().max().item() \
        <= bn + 5 * 2.0 ** -20 + 2.0 ** -21
    out2, g2 = _fwd(gx, w, b, h0, False, wdt)
    assert g2.numel() == 0 and torch.equal(out2, got_out)


@pytest.mark.parametrize('B,T,H', [(17, 7, 161), (3, 2, 256)])
def test_fwd_exact_time_indexing(B, T, H):
    gx, w, b, h0, out = gc.time_case(B, T, H)
    got_out, got_g = _fwd(gx, w, b, h0)
    assert torch.equal(got_out.cpu(), out.float())
    assert torch.equal(got_g[:, :, :2].cpu(), torch.full((B, T, 2, H), .5))
    assert not got_g[:, :, 2:].any()


@pytest.mark.parametrize('B,H,T,wdt,frame', [
    (B, H, T, wdt, lambda t: t) for B, H in BH for T in (1, 2)
    for wdt in WDT] + [(17, 145, 2, 'bf16', gc.nan_framed)])
def test_bwd_exact(B, H, T, wdt, frame):
    dout, out, gates, w, h0, ref = gc.bwd_case(B, T, H)
    got = ops._C.gru_stream_bwd(
        *(frame(_dev(t)) for t in (dout, out, gates)),
        frame(_dev(w, gc.DTYPES[wdt])), frame(_dev(h0)))
    for t, name, shape in zip(got, ('dgx', 'dgh', 'dh0'),
                              ((B, T, 3 * H), (B, T, 3 * H), (B, H))):
        assert t.dtype == F32 and t.shape == shape and t.is_contiguous()
        assert torch.equal(t.cpu(), ref[name].float()), name


@pytest.mark.parametrize('B,T,H', [(10, 50, 256), (33, 7, 200)])
def test_random_and_deterministic(B, T, H):
    c = gc.random_case(B, T, H)
    h0, dout, w = _dev(c['h0']), _dev(c['dout']), _dev(c['w'])
    runs = []
    for _ in range(2):
        out, gates = _fwd(c['gx'], c['w'], c['b'], c['h0'])
        runs.append((out, gates) +
                    tuple(ops._C.gru_stream_bwd(dout, out, gates, w, h0)))
    got = dict(zip(('out', 'gates', 'dgx', 'dgh', 'dh0'), runs[0]),
               dw=fgru.hh_weight_grad(runs[0][3], out, h0),
               db=fgru.hh_bias_grad(runs[0][3]))
    bad = []
    for name, t in got.items():
        bad += _within(t, c['ref'][name], c['tol'][name], c['e32'][name],
                       '(%d,%d,%d) %s' % (B, T, H, name))
    assert not bad, bad
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_launchers_reject_before_launching():
    def z(*shape):
        return torch.zeros(*shape, device='cuda')

    def fwd(H, gx=None):
        return ops._C.gru_stream_fwd(z(3, 2, 3 * H) if gx is None else gx,
                                     z(3 * H, H), z(3 * H), z(3, H), True)

    def bwd(H):
        return ops._C.gru_stream_bwd(z(3, 2, H), z(3, 2, H), z(3, 2, 4, H),
                                     z(3 * H, H), z(3, H))

    fwd(129), bwd(129)
    for H in (128, 257):
        for fn in (fwd, bwd):
            with pytest.raises(RuntimeError, match='unsupported H'):
                fn(H)
    for gx in (z(3, 2, 387).double(), z(3, 2, 387).bfloat16(),
               z(3, 2, 774)[:, :, ::2], z(2, 3, 387).transpose(0, 1)):
        with pytest.raises(RuntimeError, match='gx must be'):
            fwd(129, gx)
    torch.cuda.synchronize()


def test_gru_seq_stream(monkeypatch):
    B, T, H = 10, 5, 256
    rec = []
    for name in ('gru_fwd', 'gru_bwd', 'gru_wide_fwd', 'gru_wide_bwd',
                 'gru_stream_fwd', 'gru_stream_bwd'):
        fn = getattr(ops._C, name)
        monkeypatch.setattr(
            ops._C, name,
            lambda *a, _fn=fn, _n=name: (rec.append(_n), _fn(*a))[1])
    monkeypatch.setattr(fgru, '_GRU_ENABLED', True)
    torch.manual_seed(H)
    g32 = nn.GRU(H, H, batch_first=True)
    x, h0, dout = torch.randn(B, T, H), torch.randn(1, B, H), \
        torch.randn(B, T, H)

    def run(gru, stream):
        monkeypatch.setattr(fgru, '_GRU_STREAM_ENABLED', stream)
        p = next(gru.parameters())
        xx = x.to(p.device, p.dtype).requires_grad_(True)
        hh = h0.to(p.device, p.dtype)
        assert fgru.gru_stream_eligible(gru, xx, hh) == (stream and p.is_cuda)
        out, hn = fgru.gru_seq(gru, xx, hh)
        grads = torch.autograd.grad(out, (xx,) + tuple(gru.parameters()),
                                    dout.to(p.device, p.dtype))
        return (out.detach(), hn.detach()) + grads

    want = run(copy.deepcopy(g32).double(), True)
    r32 = run(g32, True)
    ggpu = copy.deepcopy(g32).cuda()
    got = run(ggpu, True)
    assert rec == ['gru_stream_fwd', 'gru_stream_bwd']
    assert got[0].dtype == got[1].dtype == F32
    bad = []
    for name, g, w64, w32 in zip(
            ('out', 'h_n', 'dx', 'dw_ih', 'dw_hh', 'db_ih', 'db_hh'), got,
            want, r32):
        assert g.shape == w64.shape, name
        bad += _within(g, w64, *gc.tolerance(w64, w32), name)
    assert not bad, bad
    del rec[:]                  # the stream flag off: the library path
    off = run(ggpu, False)
    with torch.no_grad():
        stock = ggpu(x.cuda(), h0.cuda())
    assert rec == []
    assert torch.equal(off[0], stock[0]) and torch.equal(off[1], stock[1])
