# -*- coding: utf-8 -*-
"""rnn_local_rounds (hip/rnnround.h) on the GPU against a float64 CPU step
loop written here with plain torch ops and autograd.  Bound: the packed-round
bound 8 e32 + 16 ulp (linround_cases.bound), e32 the error of the same loop
in fp32 on the CPU, ulp of the tensor's largest magnitude."""
import pytest
import torch
import torch.nn.functional as Fn

import linround_cases as lc
import fedtorch_amd.ops as ops

pytestmark = pytest.mark.gpu

NAN = float('nan')
SHAPES = [(5, 3, 1, 1), (11, 17, 3, 5), (33, 64, 2, 16), (86, 50, 4, 18)]
OUT = ('replicas', 'in_mom', 'snap', 'hidden', 'loss')
HP = dict(weight_decay=1e-2, dampening=0.0, nesterov=False)


def make_case(V, H, T, B, momentum, seed=0):
    """C = 3, client 1 offline, steps 3 and 2, a short batch in the middle of
    client 0, one token outside [0, V), float operands cut out of NaN-filled
    buffers with NaN left in the offline client's rows"""
    g = torch.Generator().manual_seed(seed + 1000 * V + B)
    K, C, S, M = V + 2, 3, 3, 6 * B + 3
    lens = dict(decoder_b=K, w_hh=3 * H * H, encoder=V * H, b_ih=3 * H,
                decoder_w=K * H, b_hh=3 * H, w_ih=3 * H * H)
    off, N = {}, 2
    for k, n in lens.items():          # 3 pad floats between the tensors
        off[k] = N
        N += n + 3
    layout = dict(encoder=(off['encoder'], V, H), w_ih=off['w_ih'],
                  w_hh=off['w_hh'], b_ih=off['b_ih'], b_hh=off['b_hh'],
                  decoder=(off['decoder_w'], off['decoder_b'], K))

    def cut(shape, fill):
        big = torch.full((shape[0] + 2,) + tuple(shape[1:]), NAN)
        big[1:-1] = fill
        return big[1:-1]
    X = torch.randint(0, V, (M, T), generator=g, dtype=torch.int32)
    Y = torch.randint(0, K, (M, T), generator=g, dtype=torch.int32)
    short = 3 if B == 5 else max(B - 1, 1)
    idx = torch.full((C, S, B), -1, dtype=torch.int32)
    for c, ns in ((0, (B, short, B)), (2, (B, B))):
        for s, n in enumerate(ns):
            idx[c, s, :n] = torch.randperm(M, generator=g)[:n].int()
    X[idx[0, 0, 0], 0] = V                      # the out-of-range token
    rnd = lambda *s: torch.rand(*s, generator=g) - .5  # noqa: E731
    case = dict(
        X=X, Y=Y, idx=idx, steps=torch.tensor([3, 0, 2], dtype=torch.int32),
        lr=cut((C, S), .2 + .1 * torch.rand(C, S, generator=g)),
        server=cut((N,), .8 * rnd(N)), replicas=cut((C, N), rnd(C, N)),
        in_mom=cut((C, N), .1 * rnd(C, N)),
        mom_init=torch.tensor([1, 0, 0], dtype=torch.int32),
        snap=cut((C, N), rnd(C, N)), hidden=cut((C, B, H), rnd(C, B, H)),
        hid_rows=torch.tensor([B, 7, 0], dtype=torch.int32))
    for k in ('replicas', 'in_mom', 'snap', 'hidden'):
        case[k][1] = NAN
    kw = dict(HP, layout=layout, wd_numel=N // 2, momentum=momentum)
    return case, kw


def ref_rounds(case, kw, k_cut, dtype):
    """the contract of ops.rnn_local_rounds as a plain loop in `dtype`;
    returns the outputs, NaN where the op writes nothing"""
    f = lambda t: t.clone().to(dtype)  # noqa: E731
    server, lr = f(case['server']), case['lr'].to(dtype)
    out = {k: f(case[k]) for k in ('replicas', 'in_mom', 'snap', 'hidden')}
    out['loss'] = torch.zeros(case['lr'].shape, dtype=dtype)
    rows_kept, inits = case['hid_rows'].tolist(), case['mom_init'].tolist()
    enc, V, H = kw['layout']['encoder']
    dw, db, K = kw['layout']['decoder']
    spans = [(enc, (V, H)), (kw['layout']['w_ih'], (3 * H, H)),
             (kw['layout']['w_hh'], (3 * H, H)), (kw['layout']['b_ih'],
                                                  (3 * H,)),
             (kw['layout']['b_hh'], (3 * H,)), (dw, (K, H)), (db, (K,))]
    mom, wd = kw['momentum'], kw['weight_decay']
    T = case['X'].shape[1]
    for c, ns in enumerate(case['steps'].tolist()):
        if ns == 0:
            continue
        p = server.clone()
        for s in range(ns):
            if s + 1 == k_cut:
                out['snap'][c] = p
            rows = case['idx'][c, s]
            rows = rows[rows >= 0].long()
            n = len(rows)
            ts = [p[o:o + torch.Size(shp).numel()].view(shp).clone()
                  .requires_grad_(True) for o, shp in spans]
            E, w_ih, w_hh, b_ih, b_hh, w_d, b_d = ts
            tok = case['X'][rows].long()
            known = ((tok >= 0) & (tok < V)).unsqueeze(-1)
            gx = (E[tok.clamp(0, V - 1)] @ w_ih.t() + b_ih) * known
            h = out['hidden'][c, :n].clone() if rows_kept[c] == n \
                else torch.zeros(n, H, dtype=dtype)
            hs = []
            for t in range(T):
                xr, xz, xn = gx[:, t].chunk(3, 1)
                hr, hz, hn = (h @ w_hh.t() + b_hh).chunk(3, 1)
                r, z = torch.sigmoid(xr + hr), torch.sigmoid(xz + hz)
                h = (1 - z) * torch.tanh(xn + r * hn) + z * h
                hs.append(h)
            logits = torch.stack(hs, 1) @ w_d.t() + b_d
            l = Fn.cross_entropy(logits.reshape(n * T, K),
                                 case['Y'][rows].long().reshape(-1))
            gs = torch.autograd.grad(l, ts)
            out['loss'][c, s] = l.detach()
            out['hidden'][c, :n] = h.detach()
            rows_kept[c] = n
            for (o, shp), gt in zip(spans, gs):
                e = torch.arange(o, o + gt.numel())
                d = gt.reshape(-1) + wd * p[e] * (e < kw['wd_numel'])
                if mom != 0:
                    d = out['in_mom'][c, e] * mom + d if inits[c] else d
                    out['in_mom'][c, e] = d
                p[e] = p[e] - lr[c, s] * d
            inits[c] = 1
        out['replicas'][c] = p
    out['hid_rows'] = torch.tensor(
        rows_kept, dtype=torch.int32)
    out['mom_init'] = torch.tensor(
        [1 if (mom != 0 and n) else i for n, i in
         zip(case['steps'].tolist(), case['mom_init'].tolist())],
        dtype=torch.int32)
    return out


def call_op(case, kw, k_cut, device='cuda', op=None):
    d = {k: v.clone().to(device) for k, v in case.items()}
    loss = (op or ops.rnn_local_rounds)(
        d['X'], d['Y'], d['idx'], d['steps'], d['lr'], d['server'],
        d['replicas'], d['in_mom'], d['mom_init'], d['snap'], k_cut,
        d['hidden'], d['hid_rows'], **kw)
    if device == 'cuda':
        torch.cuda.synchronize()
    return dict(d, loss=loss)


def assert_bounded(got, case, kw, k_cut):
    ref = ref_rounds(case, kw, k_cut, torch.float64)
    r32 = ref_rounds(case, kw, k_cut, torch.float32)
    for k in OUT:
        if k == 'in_mom' and kw['momentum'] == 0:
            ref[k] = case[k].double()          # untouched without momentum
            r32[k] = case[k]
        assert lc.same_nan_pattern(got[k], ref[k]), k
        e32 = lc.err(r32[k], ref[k])
        live = ref[k][~torch.isnan(ref[k])]
        tol = lc.bound(e32, live.abs().max().item())
        e = lc.err(got[k], ref[k])
        print('%s: err %.3e  e32 %.3e  tol %.3e' % (k, e, e32, tol))
        assert e <= tol, k
    assert got['hid_rows'].cpu().tolist() == ref['hid_rows'].tolist()
    assert got['mom_init'].cpu().tolist() == ref['mom_init'].tolist()


@pytest.mark.parametrize('momentum', [0.0, 0.9])
@pytest.mark.parametrize('V,H,T,B', SHAPES)
def test_against_float64_loop(V, H, T, B, momentum):
    case, kw = make_case(V, H, T, B, momentum)
    assert_bounded(call_op(case, kw, 2), case, kw, 2)


def _same(a, b):
    for k in OUT + ('hid_rows', 'mom_init'):
        x, y = a[k].cpu(), b[k].cpu()
        assert torch.equal(torch.isnan(x), torch.isnan(y)), k
        assert torch.equal(x[~torch.isnan(x)], y[~torch.isnan(y)]), k


def test_two_runs_bit_identical():
    case, kw = make_case(86, 50, 4, 18, 0.9)
    _same(call_op(case, kw, 2), call_op(case, kw, 2))


def test_graph_capture_replays():
    case, kw = make_case(11, 17, 3, 5, 0.9)
    want = call_op(case, kw, 2)
    d = {k: v.clone().cuda() for k, v in case.items()}
    inout = ('replicas', 'in_mom', 'mom_init', 'snap', 'hidden', 'hid_rows')
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        loss = ops.rnn_local_rounds(
            d['X'], d['Y'], d['idx'], d['steps'], d['lr'], d['server'],
            d['replicas'], d['in_mom'], d['mom_init'], d['snap'], 2,
            d['hidden'], d['hid_rows'], **kw)
    for _ in range(3):                 # in/out operands back, then replay
        for k in inout:
            d[k].copy_(case[k])
        g.replay()
        torch.cuda.synchronize()
        _same(dict(d, loss=loss), want)


def test_limits_and_rejections():
    lim = ops.rnn_round_limits()
    assert list(ops._C.rnn_round_limits()) == [lim['B'], lim['H'], lim['V'],
                                               lim['K']]
    case, kw = make_case(11, 17, 3, 5, 0.9)

    def bad(mutate, match, device='cuda'):
        c, k = {n: v.clone() for n, v in case.items()}, dict(kw)
        k['layout'] = dict(k['layout'])
        mutate(c, k)
        with pytest.raises((RuntimeError, ValueError), match=match):
            call_op(c, k, 2, device=device)

    def lay(key, v):
        return lambda c, k: k['layout'].__setitem__(key, v)
    enc = kw['layout']['encoder']
    bad(lay('encoder', (enc[0], enc[1], 65)), 'unsupported H=65')
    bad(lay('encoder', (enc[0], 129, enc[2])), 'unsupported V=129')
    bad(lay('w_ih', kw['layout']['w_hh'] + 1), 'overlap')
    bad(lay('b_hh', 10 ** 7), 'does not fit')
    bad(lambda c, k: c.__setitem__(
        'idx', torch.cat([c['idx']] * 13, 2).contiguous()), 'unsupported B=65')
    bad(lambda c, k: c.__setitem__('X', c['X'].long()), 'X must be')
    bad(lambda c, k: c.__setitem__('hid_rows', c['hid_rows'].long()),
        'hid_rows must be')
    bad(lambda c, k: c['idx'].__setitem__((0, 0, 0), c['X'].shape[0]),
        'idx holds row')

    def hole(c, k):                    # valid rows that are no prefix
        c['idx'][0, 0, 1] = -1
    for k in ('replicas', 'in_mom', 'snap', 'hidden'):
        case[k][1] = 0.0               # the twin runs on finite operands
    bad(hole, 'not a prefix', device='cpu')
