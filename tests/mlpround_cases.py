# -*- coding: utf-8 -*-
"""Reference and case generator for ops.mlp_local_rounds (hip/mlpround.h):
a plain per-client step loop with a hand-written backward in any dtype
(float64 is the reference, float32 measures the format's own error), and
random-valued cases whose ReLU pre-activations stay clear of zero.  Shared
by test_mlpround_cpu.py and test_gpu_mlpround.py."""
import functools

import torch

import linround_cases as lc

F64 = torch.float64
F32 = torch.float32
NAN = float('nan')
OUTPUTS = ('replicas', 'in_mom', 'snap', 'loss')


# --------------------------------------------------------------------------
# layout
# --------------------------------------------------------------------------
def make_layout(F, H, K, L):
    """an arena-like layout in named_parameters order with pad gaps (64
    aligned, a leading gap as well): (layout, N)"""
    al = lambda n: (n + 63) // 64 * 64  # noqa: E731
    off, blocks, fin = 64, [], F
    for _i in range(L):
        w = off
        b = w + al(H * fin)
        g = b + al(H)
        be = g + al(H)
        off = be + al(H)
        blocks.append((w, b, g, be, fin, H))
        fin = H
    fc = off
    return dict(blocks=blocks, head=(fc, H, K)), fc + al(K * H)


def spans(layout):
    """[(start, end, kind)] of the parameter tensors"""
    out = []
    for w, b, g, be, fin, o in layout['blocks']:
        out += [(w, w + fin * o, 'w'), (b, b + o, 'b'), (g, g + o, 'g'),
                (be, be + o, 'be')]
    fc, H, K = layout['head']
    out.append((fc, fc + H * K, 'w'))
    return out


def gap_mask(layout, N):
    gap = torch.ones(N, dtype=torch.bool)
    for lo, hi, _k in spans(layout):
        gap[lo:hi] = False
    return gap


# --------------------------------------------------------------------------
# the reference: a plain step loop, backward written out
# --------------------------------------------------------------------------
def _sgd(p, buf, lo, hi, g, first, lr, wd, wd_numel, m, damp, nesterov):
    """the local branch of ops.fused_sgd_step on arena elements lo .. hi"""
    d = g.reshape(-1).clone()
    if wd != 0:
        nw = max(min(wd_numel, hi) - lo, 0)
        d[:nw] += wd * p[lo:lo + nw]
    if m != 0:
        if first:
            buf[lo:hi] = d
        else:
            buf[lo:hi] = m * buf[lo:hi] + (1 - damp) * d
        d = d + m * buf[lo:hi] if nesterov else buf[lo:hi].clone()
    p[lo:hi] -= lr * d


def ref_rounds(X, Y, idx, steps, lr, server, replicas, in_mom, mom_init,
               snap, k_cut, layout, eps, wd_numel, wd, m, damp, nesterov,
               dtype=F64, pre=None):
    """mlp_local_rounds as a plain loop in `dtype`.  Nothing is modified;
    returns dict(replicas, in_mom, mom_init, snap, loss) where untouched rows
    are copies of the inputs.  `pre`: a list that receives the pre-ReLU
    values y_i of the valid rows, one tensor per (client, step, block) in
    execution order."""
    C, T, _B = idx.shape
    out = dict(replicas=replicas.to(dtype).clone(),
               in_mom=None if in_mom is None else in_mom.to(dtype).clone(),
               mom_init=mom_init.clone(),
               snap=None if snap is None else snap.to(dtype).clone(),
               loss=torch.zeros((C, T), dtype=dtype))
    Xd = X.to(dtype)
    blocks = layout['blocks']
    fc, H, K = layout['head']
    for c in range(C):
        ns = int(steps[c])
        if ns <= 0:
            continue
        p = server.to(dtype).clone()
        buf = out['in_mom'][c] if m != 0 else None
        had = bool(mom_init[c]) if m != 0 else False
        for s in range(ns):
            if snap is not None and s + 1 == k_cut:
                out['snap'][c].copy_(p)
            rows = idx[c, s]
            rows = rows[rows >= 0].long()
            n = len(rows)
            y_ids = Y[rows].long()
            a = Xd[rows]
            saved = []
            for w, b, g, be, fin, o in blocks:
                W = p[w:w + fin * o].view(o, fin)
                z = a @ W.t() + p[b:b + o]
                mu = z.mean(0)
                var = ((z - mu) ** 2).mean(0)
                rstd = 1.0 / torch.sqrt(var + eps)
                xh = (z - mu) * rstd
                y = p[g:g + o] * xh + p[be:be + o]
                if pre is not None:
                    pre.append(y.clone())
                saved.append((a, xh, rstd, y))
                a = y.clamp(min=0)
            Wfc = p[fc:fc + H * K].view(K, H)
            z = a @ Wfc.t()
            lse = torch.logsumexp(z, 1)
            ar = torch.arange(n)
            out['loss'][c, s] = (lse - z[ar, y_ids]).sum() / n
            dl = torch.softmax(z, 1)
            dl[ar, y_ids] -= 1
            dl = dl / n
            grads = [(fc, fc + H * K, dl.t() @ a)]
            da = dl @ Wfc
            for (w, b, g, be, fin, o), (a_in, xh, rstd, y) in \
                    reversed(list(zip(blocks, saved))):
                W = p[w:w + fin * o].view(o, fin)
                dy = da * (y > 0).to(dtype)
                dg = (dy * xh).sum(0)
                dbe = dy.sum(0)
                dz = p[g:g + o] * rstd / n * (n * dy - dbe - xh * dg)
                grads += [(w, w + fin * o, dz.t() @ a_in),
                          (b, b + o, dz.sum(0)), (g, g + o, dg),
                          (be, be + o, dbe)]
                da = dz @ W
            first = m != 0 and not had
            for lo, hi, gr in grads:
                _sgd(p, buf, lo, hi, gr, first, float(lr[c, s]), wd,
                     wd_numel, m, damp, nesterov)
            had = True
        out['replicas'][c].copy_(p)
        if m != 0:
            out['mom_init'][c] = 1
    return out


# --------------------------------------------------------------------------
# cases
# --------------------------------------------------------------------------
# (F, H, K, L, B): hyper-parameters, the short batch, k_cut, wd_numel and the
# seed.  Every seed is checked by `case()` (the ReLU precondition below); the
# seeds were searched on the CPU for a margin of at least 80 where 64 is
# asserted (the largest shape has 72000 pre-ReLU values: few seeds qualify).
CASES = {
    (14, 33, 2, 1, 5): dict(
        hp=dict(wd=0.0, m=0.0, damp=0.0, nesterov=False), short=(0, 2, 3),
        k_cut=3, wd_part=False, mom_init=[0, 0, 0], seed=0),
    (45, 70, 10, 2, 16): dict(
        hp=dict(wd=5e-4, m=0.9, damp=0.0, nesterov=True), short=(2, 1, 2),
        k_cut=3, wd_part=True, mom_init=[0, 1, 1], seed=0),
    (257, 96, 62, 3, 50): dict(
        hp=dict(wd=5e-4, m=0.9, damp=0.0, nesterov=False), short=(0, 2, 17),
        k_cut=1, wd_part=False, mom_init=[1, 0, 0], seed=41018),
}
SHAPES = list(CASES)
STEPS = [3, 0, 2]          # C = 3: client 1 offline, unequal steps
EPS = 1e-5
MARGIN = 64.0


def make_case(g, F, H, K, L, B, steps, M, *, m, layout=None, N=None,
              short=None, mom_init=None):
    """operands of one call (CPU tensors, fp32 / int32).  Server weights are
    random with scale 1 / sqrt(fan_in) (zero weights would give constant
    columns and var = 0); pad gaps of server / in_mom are non-zero (they
    must pass through / stay).  `short` = (client, step, n): that step gets
    n valid rows, the rest padding."""
    if layout is None:
        layout, N = make_layout(F, H, K, L)
    C, T = len(steps), max(max(steps), 1)
    server = torch.randn(N, generator=g) * .1
    for lo, hi, kind in spans(layout):
        v = torch.randn(hi - lo, generator=g)
        if kind == 'w':
            fan_in = [blk[4] for blk in layout['blocks'] if blk[0] == lo]
            fan_in = fan_in[0] if fan_in else layout['head'][1]
            server[lo:hi] = v / fan_in ** .5
        elif kind == 'g':
            server[lo:hi] = 1 + .1 * v
        else:
            server[lo:hi] = .1 * v
    X = torch.randn(M, F, generator=g)
    Y = torch.randint(0, K, (M,), generator=g).to(torch.int32)
    idx = torch.full((C, T, B), -1, dtype=torch.int32)
    for c in range(C):
        for s in range(steps[c]):
            idx[c, s] = torch.randperm(M, generator=g)[:B]
    if short is not None:
        c, s, n = short
        idx[c, s, n:] = -1
    in_mom = torch.randn(C, N, generator=g) * .01 if m != 0 else None
    if mom_init is None:
        mom_init = [c % 2 for c in range(C)]
    return dict(X=X, Y=Y, idx=idx,
                steps=torch.tensor(steps, dtype=torch.int32), server=server,
                replicas=torch.full((C, N), NAN), in_mom=in_mom,
                mom_init=torch.tensor(mom_init, dtype=torch.int32), N=N,
                layout=layout, eps=EPS)


def run_ref(case, lr, k_cut, hp, snap, wd_numel, dtype=F64, pre=None):
    return ref_rounds(case['X'], case['Y'], case['idx'], case['steps'], lr,
                      case['server'], case['replicas'], case['in_mom'],
                      case['mom_init'], snap, k_cut, case['layout'],
                      case['eps'], wd_numel, hp['wd'], hp['m'], hp['damp'],
                      hp['nesterov'], dtype=dtype, pre=pre)


def relu_margin(case, lr, k_cut, hp, snap, wd_numel):
    """(ref64, ref32, smallest |y| of the float64 replay, largest error of
    the fp32 replay in y) over all pre-ReLU values of valid rows"""
    p64, p32 = [], []
    ref = run_ref(case, lr, k_cut, hp, snap, wd_numel, pre=p64)
    r32 = run_ref(case, lr, k_cut, hp, snap, wd_numel, dtype=F32, pre=p32)
    lo = min(y.abs().min().item() for y in p64)
    e = max((a.double() - b).abs().max().item() for a, b in zip(p32, p64))
    return ref, r32, lo, e


def build(F, H, K, L, B, seed):
    spec = CASES[(F, H, K, L, B)]
    g = lc.gen('mlp', F, H, K, L, B, seed)
    hp = spec['hp']
    case = make_case(g, F, H, K, L, B, STEPS, 3 * B + 7, m=hp['m'],
                     short=spec['short'], mom_init=spec['mom_init'])
    C, T = len(STEPS), max(STEPS)
    lr = torch.rand(C, T, generator=g) * .05 + .01      # changes per step
    snap = torch.full((C, case['N']), NAN)
    # wd on a prefix only: up to the middle of the head's weight
    fc, Hh, Kh = case['layout']['head']
    wd_numel = fc + (Hh * Kh) // 2 if spec['wd_part'] else case['N']
    return case, lr, spec['k_cut'], hp, snap, wd_numel


@functools.lru_cache(maxsize=None)
def case(F, H, K, L, B):
    """(case, lr, k_cut, hp, snap, wd_numel, ref64, e32) of a shape of CASES,
    computed once and shared: treat it as read-only.  e32: the largest error
    of the same loop in fp32 on the CPU, per output.

    Precondition, asserted here: ReLU makes the loss non-smooth, so every
    pre-ReLU value of a valid row lies farther from zero, in the float64
    replay, than 64 times the fp32 replay's largest error in the pre-ReLU
    values; then no rounding of fp32 size flips a mask."""
    seed = CASES[(F, H, K, L, B)]['seed']
    cs, lr, k_cut, hp, snap, wd_numel = build(F, H, K, L, B, seed)
    ref, r32, lo, e = relu_margin(cs, lr, k_cut, hp, snap, wd_numel)
    assert lo > MARGIN * e, ('a pre-ReLU value is too close to zero',
                             (F, H, K, L, B, seed), lo, e)
    e32 = {k: lc.err(r32[k], ref[k]) for k in OUTPUTS if ref[k] is not None}
    return cs, lr, k_cut, hp, snap, wd_numel, ref, e32


def scale_of(t):
    return t[~torch.isnan(t)].abs().max().item()


def call_op(ops, case, lr, k_cut, hp, snap, wd_numel, device='cpu'):
    """run ops.mlp_local_rounds on copies of the case's operands on `device`;
    returns dict like ref_rounds"""
    d = lambda t: None if t is None else t.clone().to(device)  # noqa: E731
    rep, mom, mi, sn = (d(case['replicas']), d(case['in_mom']),
                        d(case['mom_init']), d(snap))
    loss = ops.mlp_local_rounds(
        d(case['X']), d(case['Y']), d(case['idx']), d(case['steps']), d(lr),
        d(case['server']), rep, mom, mi, sn, k_cut, layout=case['layout'],
        eps=case['eps'], wd_numel=wd_numel, weight_decay=hp['wd'],
        momentum=hp['m'], dampening=hp['damp'], nesterov=hp['nesterov'])
    return dict(replicas=rep, in_mom=mom, mom_init=mi, snap=sn, loss=loss)
