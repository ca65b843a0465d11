# -*- coding: utf-8 -*-
"""Classifier-tail kernels (hip/head.h) on the GPU against the float64
references of tests/head_cases.py: head_fwd / head_bwd exact-integer cases
and random companions, determinism, launcher argument checks, the routing
of ops.head.pool_fc (FEDTORCH_FUSED_HEAD), graph capture, ce_topk_accum with
its tie rule, and the fused-metrics validation pass
(FEDTORCH_FUSED_METRICS)."""
import contextlib
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import head_cases as hc
import fedtorch_amd.ops as ops
from fedtorch_amd.components import metrics as ftm
from fedtorch_amd.logs.meter import define_val_tracker
from fedtorch_amd.ops import head
from fedtorch_amd.trainings import eval as ft_eval
from fedtorch_amd.trainings.eval_centered import do_validate_centered

pytestmark = pytest.mark.gpu

CL = torch.channels_last
F64 = torch.float64
DT = hc.DTYPES
OPS = ('head_fwd', 'head_bwd', 'ce_topk_accum')


@pytest.fixture
def calls(monkeypatch):
    """list of the names of the recorded ops._C head calls"""
    rec = []
    for name in OPS:
        fn = getattr(ops._C, name)
        monkeypatch.setattr(
            ops._C, name,
            lambda *a, _fn=fn, _n=name: (rec.append(_n), _fn(*a))[1])
    return rec


@contextlib.contextmanager
def _flags(head_on=None, metrics_on=None):
    old = head._HEAD_ENABLED, head._METRICS_ENABLED
    if head_on is not None:
        head._HEAD_ENABLED = head_on
    if metrics_on is not None:
        head._METRICS_ENABLED = metrics_on
    try:
        yield
    finally:
        head._HEAD_ENABLED, head._METRICS_ENABLED = old


def _empty():
    return torch.empty(0, device='cuda')


def _bias(b64, bdt):
    return _empty() if b64 is None or bdt is None else \
        b64.to(DT[bdt]).cuda()


def _within(got, want64, tol64, what):
    err = (got.detach().double().cpu() - want64).abs()
    worst = (err / tol64.clamp(min=1e-300)).max().item()
    print('%s: max err / tol = %.4f' % (what, worst))
    assert bool((err <= tol64).all()), (what, worst)


# --------------------------------------------------------------------------
# head_fwd
# --------------------------------------------------------------------------
_FULL = [(s, x, w, b) for s in hc.FWD_EXACT_FULL for x in ('bf16', 'fp32')
         for w in ('bf16', 'fp32') for b in ('bf16', 'fp32', None)]
_REST = [(s, 'bf16', 'fp32', 'fp32') for s in hc.FWD_EXACT_REST]


@pytest.mark.parametrize('shape,xdt,wdt,bdt', _FULL + _REST)
def test_head_fwd_exact(shape, xdt, wdt, bdt):
    x, w, b, logits, pooled = hc.fwd_exact_case(shape, bdt is not None)
    got_l, got_p = ops._C.head_fwd(
        hc.to_dev(x, DT[xdt], 'cuda', True), w.to(DT[wdt]).cuda(),
        _bias(b, bdt))
    assert got_l.dtype == got_p.dtype == torch.float32
    assert got_l.shape == logits.shape and got_p.shape == pooled.shape
    assert got_l.is_contiguous() and got_p.is_contiguous()
    assert torch.equal(got_p.cpu(), pooled.float())
    assert torch.equal(got_l.cpu(), logits.float())


@pytest.mark.parametrize('shape', hc.FWD_RANDOM)
@pytest.mark.parametrize('xdt,wdt,bdt', [('bf16', 'fp32', 'fp32'),
                                         ('bf16', 'bf16', 'bf16'),
                                         ('fp32', 'fp32', 'fp32')])
def test_head_fwd_random(shape, xdt, wdt, bdt):
    x, w, b, logits, pooled, tol_l, tol_p = hc.fwd_random_case(
        shape, DT[xdt], DT[wdt], DT[bdt])
    got_l, got_p = ops._C.head_fwd(
        hc.to_dev(x, DT[xdt], 'cuda', True), w.to(DT[wdt]).cuda(),
        b.to(DT[bdt]).cuda())
    _within(got_p, pooled, tol_p, 'pooled')
    _within(got_l, logits, tol_l, 'logits')


# --------------------------------------------------------------------------
# head_bwd
# --------------------------------------------------------------------------
@pytest.mark.parametrize('N', hc.BWD_N)
@pytest.mark.parametrize('shape', hc.BWD_SHAPES)
@pytest.mark.parametrize('xdt,wdt,bdt', [('bf16', 'bf16', 'bf16'),
                                         ('bf16', 'fp32', 'fp32'),
                                         ('fp32', 'bf16', 'fp32'),
                                         ('fp32', 'fp32', None)])
def test_head_bwd_exact(N, shape, xdt, wdt, bdt):
    C, H, W, K = shape
    dl, pooled, w, b, dx, dw, db = hc.bwd_exact_case(N, shape)
    wt, bt = w.to(DT[wdt]).cuda(), _bias(b, bdt)
    got_dx, got_dw, got_db = ops._C.head_bwd(
        dl.float().cuda(), pooled.float().cuda(), wt, bt, H, W,
        xdt == 'bf16', True)
    assert got_dx.dtype == DT[xdt] and got_dx.shape == (N, C, H, W)
    assert got_dx.is_contiguous(memory_format=CL)
    assert torch.equal(got_dx.cpu(), dx.float().to(DT[xdt]))
    assert got_dw.dtype == wt.dtype and got_dw.shape == wt.shape
    assert got_dw.is_contiguous() and got_dw.data_ptr() != wt.data_ptr()
    assert torch.equal(got_dw.cpu(), dw.float().to(DT[wdt]))
    if bdt is None:
        assert got_db is None
    else:
        assert got_db.dtype == bt.dtype and got_db.shape == bt.shape
        assert got_db.is_contiguous()
        assert torch.equal(got_db.cpu(), db.float().to(DT[bdt]))


def test_head_bwd_no_dx():
    dl, pooled, w, b, _dx, dw, _db = hc.bwd_exact_case(3, hc.BWD_SHAPES[0])
    C, H, W, K = hc.BWD_SHAPES[0]
    out = ops._C.head_bwd(dl.float().cuda(), pooled.float().cuda(),
                          w.float().cuda(), b.float().cuda(), H, W, True,
                          False)
    assert out[0] is None
    assert torch.equal(out[1].cpu(), dw.float())


@pytest.mark.parametrize('N', [3, 257])
@pytest.mark.parametrize('shape', hc.BWD_SHAPES)
@pytest.mark.parametrize('xdt,wdt', [('bf16', 'bf16'), ('fp32', 'fp32')])
def test_head_bwd_random(N, shape, xdt, wdt):
    C, H, W, K = shape
    dl, pooled, w, dx, dw, db, tol_dx, tol_dw, tol_db = hc.bwd_random_case(
        N, shape, DT[wdt])
    bt = torch.zeros(K, dtype=DT[wdt], device='cuda')
    got_dx, got_dw, got_db = ops._C.head_bwd(
        dl.float().cuda(), pooled.float().cuda(), w.to(DT[wdt]).cuda(), bt,
        H, W, xdt == 'bf16', True)
    _within(got_dx, dx, tol_dx + hc.half_ulp(dx, DT[xdt]), 'dx')
    _within(got_dw, dw, tol_dw + hc.half_ulp(dw, DT[wdt]), 'dw')
    _within(got_db, db, tol_db + hc.half_ulp(db, DT[wdt]), 'db')


# --------------------------------------------------------------------------
# determinism
# --------------------------------------------------------------------------
def test_determinism():
    N, C, H, W, K = 257, 64, 8, 8, 10
    g = hc.gen('determinism')
    x = torch.randn(N, C, H, W, generator=g).cuda().bfloat16().contiguous(
        memory_format=CL)
    w = torch.randn(K, C, generator=g).cuda()
    b = torch.randn(K, generator=g).cuda()
    dl = torch.randn(N, K, generator=g).cuda()
    z = torch.randn(N, K, generator=g).cuda()
    t = torch.randint(0, K, (N,), generator=g).cuda()
    runs = []
    for _ in range(2):
        logits, pooled = ops._C.head_fwd(x, w, b)
        dx, dw, db = ops._C.head_bwd(dl, pooled, w, b, H, W, True, True)
        acc = torch.zeros(4, dtype=F64, device='cuda')
        ops._C.ce_topk_accum(z, t, acc)
        runs.append((logits, pooled, dx, dw, db, acc))
    for a, b_ in zip(*runs):
        assert torch.equal(a, b_)


# --------------------------------------------------------------------------
# argument checks: every launcher refuses before any launch
# --------------------------------------------------------------------------
def test_argument_checks():
    N, C, H, W, K = 2, 16, 2, 2, 5
    x = torch.zeros(N, C, H, W, device='cuda').contiguous(memory_format=CL)
    w = torch.zeros(K, C, device='cuda')
    b = torch.zeros(K, device='cuda')
    ops._C.head_fwd(x, w, b)                      # the base case is fine
    bad_fwd = [
        (x.contiguous(), w, b),                               # NCHW
        (torch.zeros(N, 12, H, W, device='cuda').contiguous(
            memory_format=CL), torch.zeros(K, 12, device='cuda'), b),
        (x, torch.zeros(1025, C, device='cuda'), _empty()),   # K = 1025
        (x, torch.zeros(C, K, device='cuda').t(), b),         # strided w
        (x, w, torch.zeros(K + 1, device='cuda')),
        (x, w.double(), b),
        (x.cpu().contiguous(memory_format=CL), w, b),         # CPU operands
        (x, w.cpu(), b),
        (x, w, b.cpu()),
    ]
    for args in bad_fwd:
        with pytest.raises(RuntimeError):
            ops._C.head_fwd(*args)
    dl = torch.zeros(N, K, device='cuda')
    pooled = torch.zeros(N, C, device='cuda')
    ops._C.head_bwd(dl, pooled, w, b, H, W, True, True)
    bad_bwd = [
        (dl.cpu(), pooled, w, b, H, W, True, True),
        (dl, pooled.cpu(), w, b, H, W, True, True),
        (dl.bfloat16(), pooled, w, b, H, W, True, True),
        (dl[:, :4], pooled, w, b, H, W, True, True),
        (dl, pooled, torch.zeros(C, K, device='cuda').t(), b, H, W, True,
         True),
        (dl, pooled, w, b, 0, W, True, True),
        (torch.zeros(N, 1025, device='cuda'), pooled,
         torch.zeros(1025, C, device='cuda'), _empty(), H, W, True, True),
    ]
    for args in bad_bwd:
        with pytest.raises(RuntimeError):
            ops._C.head_bwd(*args)
    z = torch.zeros(N, K, device='cuda')
    t = torch.zeros(N, dtype=torch.int64, device='cuda')
    acc = torch.zeros(4, dtype=F64, device='cuda')
    ops._C.ce_topk_accum(z, t, acc)
    bad_ce = [
        (z, t.int(), acc),                                    # int32 targets
        (z, t, acc.float()),                                  # float32 acc
        (z, t, torch.zeros(3, dtype=F64, device='cuda')),     # wrong length
        (z, t, torch.zeros(5, dtype=F64, device='cuda')),
        (z.cpu(), t, acc), (z, t.cpu(), acc), (z, t, acc.cpu()),
        (torch.zeros(N, 1025, device='cuda'), t, acc),
        (z, t[:1], acc),
        (z.t(), torch.zeros(K, dtype=torch.int64, device='cuda'), acc),
    ]
    for args in bad_ce:
        with pytest.raises(RuntimeError):
            ops._C.ce_topk_accum(*args)
    torch.cuda.synchronize()
    assert acc.tolist()[3] == N                   # only the good call landed


# --------------------------------------------------------------------------
# routing
# --------------------------------------------------------------------------
def _fc_pair(N=5, C=64, HW=8, K=10):
    torch.manual_seed(17)
    fc = nn.Linear(C, K).cuda()
    g = hc.gen('routing', N, C, HW, K)
    x = torch.randn(N, C, HW, HW, generator=g).cuda().bfloat16().contiguous(
        memory_format=CL)
    dl = torch.randn(N, K, generator=g).cuda()
    return fc, x, dl


def test_pool_fc_routing(calls):
    fc, x, dl = _fc_pair()
    N, C, H, W = x.shape
    K = fc.out_features
    x.requires_grad_(True)
    with _flags(head_on=True):
        out = head.pool_fc(x, fc)
        assert calls == ['head_fwd']
        assert out.dtype == torch.float32
        out.backward(dl)
        assert calls == ['head_fwd', 'head_bwd']
    x64 = x.detach().double().cpu()
    w64, b64 = fc.weight.detach().double().cpu(), fc.bias.detach().double().cpu()
    dl64 = dl.double().cpu()
    logits, pooled = hc.ref_fwd(x64, w64, b64)
    dx, dw, db = hc.ref_bwd(dl64, pooled, w64, H, W)
    HW = H * W
    ap = x64.abs().sum(dim=(2, 3)) / HW
    _within(out, logits,
            (HW + C + 3) * hc.U * (ap @ w64.abs().t() + b64.abs()), 'logits')
    tol_dx = ((K + 3) * hc.U * (dl64.abs() @ w64.abs()) / HW)[
        :, :, None, None].expand(-1, -1, H, W)
    _within(x.grad, dx, tol_dx + hc.half_ulp(dx, torch.bfloat16), 'x.grad')
    # dw reads the kernel's own fp32 pooled: its error rides along
    tol_dw = (N + 2) * hc.U * (dl64.abs().t() @ ap) \
        + (HW + 2) * hc.U * (dl64.abs().t() @ ap)
    _within(fc.weight.grad, dw, tol_dw, 'fc.weight.grad')
    _within(fc.bias.grad, db, (N + 2) * hc.U * dl64.abs().sum(dim=0),
            'fc.bias.grad')
    assert x.grad.dtype == torch.bfloat16
    assert x.grad.is_contiguous(memory_format=CL)
    # needs_input_grad: a frozen input gets no dx kernel result
    del calls[:]
    with _flags(head_on=True):
        head.pool_fc(x.detach(), fc).backward(dl)
    assert calls == ['head_fwd', 'head_bwd']
    # flag off: the module calls, bit for bit, and no kernel
    del calls[:]
    with _flags(head_on=False), torch.no_grad(), \
            torch.autocast('cuda', dtype=torch.bfloat16):
        got = head.pool_fc(x, fc)
        want = fc(F.adaptive_avg_pool2d(x, 1).flatten(1))
    assert calls == []
    assert got.dtype == want.dtype == torch.bfloat16
    assert torch.equal(got, want)


@pytest.fixture(scope='module')
def resnet20():
    """seeded converted channels_last ResNet-20 as the training loop holds
    it (4-D weights in bf16, the stem's fp32; fc fp32 as under autocast)"""
    from fedtorch_amd.components.models.resnet import resnet
    from fedtorch_amd.ops.batchnorm import convert_to_fused_bn
    from fedtorch_amd.ops.stemconv import convert_stem
    torch.manual_seed(41)
    m = resnet(SimpleNamespace(arch='resnet20', data='cifar10')).cuda().to(
        memory_format=CL)
    convert_to_fused_bn(m)
    convert_stem(m)
    for p_ in m.parameters():
        if p_.dim() == 4 and p_ is not m.conv1.weight:
            p_.data = p_.data.bfloat16()
    return m


def _batch(n, seed):
    g = hc.gen('resnet_batch', n, seed)
    x = torch.randn(n, 3, 32, 32, generator=g).cuda().contiguous(
        memory_format=CL)
    return x, torch.randint(0, 10, (n,), generator=g).cuda()


def test_resnet20_routing(resnet20, calls):
    m = resnet20
    x, t = _batch(5, 0)
    with _flags(head_on=True):
        m.eval()
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
            out = m(x)
        assert calls == ['head_fwd']
        assert out.shape == (5, 10) and out.dtype == torch.float32
        del calls[:]
        m.train()
        with torch.autocast('cuda', dtype=torch.bfloat16):
            loss = F.cross_entropy(m(x), t)
        loss.backward()
        assert calls == ['head_fwd', 'head_bwd']
        assert m.fc.weight.grad.shape == m.fc.weight.shape
        assert m.fc.weight.grad.dtype == m.fc.weight.dtype
    m.zero_grad(set_to_none=True)
    del calls[:]
    with _flags(head_on=False):
        m.eval()
        with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
            m(x)
        m.train()
    assert calls == []


# --------------------------------------------------------------------------
# graph capture
# --------------------------------------------------------------------------
def test_graph_capture():
    fc, x, dl = _fc_pair(N=8)
    x.requires_grad_(True)

    def step():
        # nothing returned keeps the autograd graph alive: a surviving graph
        # holds the leaves' AccumulateGrad nodes, which remember the stream
        # they were made on, and the engine would then sync the capture
        # stream with that outside stream in the middle of the capture
        out = head.pool_fc(x, fc)
        gx, gw, gb = torch.autograd.grad(out, (x, fc.weight, fc.bias), dl)
        return out.detach(), gx, gw, gb

    with _flags(head_on=True):
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


# --------------------------------------------------------------------------
# ce_topk_accum
# --------------------------------------------------------------------------
def _acc():
    return torch.zeros(4, dtype=F64, device='cuda')


def _check(got, parts, factor=1.0, what=''):
    loss = sum(p[0] for p in parts)
    bound = sum(p[4] for p in parts)
    assert tuple(int(v) for v in got[1:]) == tuple(
        sum(p[i] for p in parts) for i in (1, 2, 3)), what
    err = abs(got[0] - loss)
    print('%s loss err / bound = %.4f' % (what, err / bound if bound else 0))
    assert err <= factor * bound, (what, got[0], loss, bound)


@pytest.mark.parametrize('dt', ['fp32', 'bf16'])
@pytest.mark.parametrize('K', hc.CE_K)
def test_ce_topk_grid(K, dt):
    for N in hc.CE_N:
        for s, o in hc.CE_DIST:
            z, t = hc.metric_case(K, N, s, o, DT[dt])
            acc = _acc()
            ops._C.ce_topk_accum(z.cuda(), t.cuda(), acc)
            _check(acc.tolist(), [hc.ref_metrics(z, t)],
                   what='K%d N%d s%g o%g %s' % (K, N, s, o, dt))


def test_ce_topk_ties_exercised():
    """bf16 at offset 100 ties constantly: the rule decides real cases"""
    z, t = hc.metric_case(62, 257, 4.0, 100.0, torch.bfloat16)
    assert not hc.tie_free(z, t)


def test_ce_topk_accumulates_and_resets(calls):
    m = head.MetricAccumulator('cuda')
    z1, t1 = hc.metric_case(10, 64, 4.0, 0.0, torch.float32)
    z2, t2 = hc.metric_case(10, 33, 1.0, 0.0, torch.bfloat16)
    m.update(z1.cuda(), t1.cuda())
    _check(m.result(), [hc.ref_metrics(z1, t1)])
    m.update(z2.cuda(), t2.cuda())
    _check(m.result(), [hc.ref_metrics(z1, t1), hc.ref_metrics(z2, t2)])
    assert calls == ['ce_topk_accum'] * 2
    m.reset()
    assert m.result() == (0.0, 0, 0, 0)


def test_ce_topk_ignored_targets():
    z, t = hc.mixed_target_case()
    acc = _acc()
    ops._C.ce_topk_accum(z.cuda(), t.cuda(), acc)
    before = acc.clone()
    _check(acc.tolist(), [hc.ref_metrics(z, t)])
    assert int(acc[3]) == t.numel() - 3
    ops._C.ce_topk_accum(z.cuda(), torch.full_like(t, -100).cuda(), acc)
    assert torch.equal(acc, before)
    ops._C.ce_topk_accum(z.cuda(), torch.full_like(t, 10).cuda(), acc)
    assert torch.equal(acc, before)


def test_ce_topk_tie_row():
    z, t = hc.tie_row_case(10)
    for dt in (torch.float32, torch.bfloat16):
        acc = _acc()
        ops._C.ce_topk_accum(z.to(dt).cuda(), t.cuda(), acc)
        assert tuple(int(v) for v in acc.tolist()[1:]) == (1, 5, 10)


@pytest.mark.parametrize('K', [5, 10, 1000])
def test_ce_topk_matches_stock(K):
    """tie-free fp32 logits: metrics.accuracy's counts and N * the mean
    CrossEntropyLoss within twice the bound"""
    N = 64
    z, t = hc.metric_case(K, N, 1.0, 0.0, torch.float32)
    assert hc.tie_free(z, t)
    zc, tc = z.cuda(), t.cuda()
    acc = _acc()
    ops._C.ce_topk_accum(zc, tc, acc)
    loss_sum, top1, top5, n = acc.tolist()
    p1, p5 = ftm.accuracy(zc, tc, topk=(1, 5))
    assert n == N
    assert top1 == round(p1 * N / 100.0) and top5 == round(p5 * N / 100.0)
    want = N * nn.CrossEntropyLoss()(zc, tc).item()
    bound = hc.ref_metrics(z, t)[4]
    assert abs(loss_sum - want) <= 2 * bound, (loss_sum, want, bound)


# --------------------------------------------------------------------------
# validation pass
# --------------------------------------------------------------------------
def _raise(*_a, **_k):
    raise AssertionError('metrics.accuracy called on the fused path')


def test_validate_centered_gpu(calls, monkeypatch):
    model, loader, args = hc.val_setup(on_cuda=True)
    with torch.no_grad():
        zs = torch.cat([model(x.cuda()) for x, _t in loader[:3]])
    ts = torch.cat([t for _x, t in loader[:3]])
    assert hc.tie_free(zs, ts)
    crit = nn.CrossEntropyLoss()
    off = define_val_tracker()
    with _flags(metrics_on=False):
        do_validate_centered(args, model, crit, (1, 5), None, loader, off)
    assert calls == []
    monkeypatch.setattr(ftm, 'accuracy', _raise)
    monkeypatch.setattr(ft_eval, 'accuracy', _raise)
    on = define_val_tracker()
    with _flags(metrics_on=True):
        do_validate_centered(args, model, crit, (1, 5), None, loader, on)
    assert calls == ['ce_topk_accum'] * 3      # 8, 8, 5; the 1 breaks
    loss_sum, top1, top5, n, bound = hc.ref_metrics(zs, ts)
    assert on['top1'].count == on['top5'].count == on['losses'].count == 21
    for name in ('top1', 'top5'):
        for field in ('sum', 'count', 'avg'):
            assert getattr(on[name], field) == getattr(off[name], field)
    assert on['top1'].sum == 100.0 * top1 and on['top5'].sum == 100.0 * top5
    print('loss on %.9f off %.9f ref %.9f bound %.3g' % (
        on['losses'].sum, off['losses'].sum, loss_sum, bound))
    assert abs(on['losses'].sum - loss_sum) <= bound
    assert abs(on['losses'].sum - off['losses'].sum) <= 2 * bound
    assert model.training


def test_validate_resnet20_both_flags(resnet20, calls, monkeypatch):
    m = resnet20
    args = SimpleNamespace(arch='resnet20', data='cifar10',
                           graph=SimpleNamespace(on_cuda=True),
                           channels_last=True)
    loader = [tuple(v.cpu() for v in _batch(5, s)) for s in (1, 2)]
    seen = []
    fwd = ops._C.head_fwd          # the recording wrapper of `calls`
    monkeypatch.setattr(
        ops._C, 'head_fwd',
        lambda *a: (lambda r: (seen.append(r[0]), r)[1])(fwd(*a)))
    monkeypatch.setattr(ftm, 'accuracy', _raise)
    monkeypatch.setattr(ft_eval, 'accuracy', _raise)
    tracker = define_val_tracker()
    with _flags(head_on=True, metrics_on=True), \
            torch.autocast('cuda', dtype=torch.bfloat16):
        do_validate_centered(args, m, nn.CrossEntropyLoss(), (1, 5), None,
                             loader, tracker)
    assert calls == ['head_fwd', 'ce_topk_accum'] * 2
    parts = [hc.ref_metrics(z, t) for z, (_x, t) in zip(seen, loader)]
    got = (tracker['losses'].sum, tracker['top1'].sum / 100.0,
           tracker['top5'].sum / 100.0, tracker['losses'].count)
    _check(got, parts, what='resnet20 validate')
    assert tracker['top1'].count == tracker['top5'].count == 10
    # a following training step, flags unchanged
    assert m.training
    x, t = _batch(5, 3)
    with _flags(head_on=True, metrics_on=True):
        with torch.autocast('cuda', dtype=torch.bfloat16):
            loss = F.cross_entropy(m(x), t)
        loss.backward()
    for name, p_ in m.named_parameters():
        assert p_.grad is not None and torch.isfinite(p_.grad).all().item(), \
            name
    m.zero_grad(set_to_none=True)
