# -*- coding: utf-8 -*-
"""References and case generators for ops.linear_local_rounds
(hip/linearround.h): a plain per-client step loop in any dtype (float64 is
the reference, float32 measures the format's own error), exact dyadic cases
with their precondition, and random-valued cases.  Shared by
test_linround_cpu.py and test_gpu_linround.py."""
import math
import zlib

import torch

F64 = torch.float64
NAN = float('nan')


def gen(*key):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(repr(key).encode()))
    return g


# --------------------------------------------------------------------------
# exactness precondition
# --------------------------------------------------------------------------
def ulp_exp(t):
    """smallest e >= 0 with t * 2^e integral for every element (t dyadic)"""
    t = t.double().reshape(-1)
    for e in range(0, 200):
        s = t * 2.0 ** e
        if bool((s == s.round()).all()):
            return e
    raise AssertionError('not dyadic')


class Exactness(object):
    """Collects the precondition of an exact case: every value, and every
    sum of absolute values of the terms of a summation, stays below 2^24
    times its dyadic denominator — then any summation order, fused or not,
    in fp32 gives the float64 result bit for bit."""

    def __init__(self):
        self.worst = 0.0

    def value(self, t):
        if t.numel():
            self.worst = max(self.worst,
                             t.abs().max().item() * 2.0 ** ulp_exp(t))
        return t

    def sum(self, terms, dim):
        if terms.numel():
            self.worst = max(
                self.worst,
                terms.abs().sum(dim).max().item() * 2.0 ** ulp_exp(terms))
        return terms.sum(dim)

    def ok(self):
        return self.worst < 2.0 ** 24


class _NoCheck(object):
    def value(self, t):
        return t

    def sum(self, terms, dim):
        return terms.sum(dim)


# --------------------------------------------------------------------------
# the reference: a plain step loop
# --------------------------------------------------------------------------
def sgd_update(p, g, buf, first, lr, wd, m, damp, nesterov, chk):
    """the local branch of ops.fused_sgd_step's eager twin on one tensor;
    returns (p, buf)"""
    d = chk.value(g + chk.value(wd * p)) if wd != 0 else g
    if m != 0:
        if first:
            buf = d.clone()
        else:
            buf = chk.value(chk.value(m * buf) + chk.value((1 - damp) * d))
        d = chk.value(d + chk.value(m * buf)) if nesterov else buf
    return chk.value(p - chk.value(lr * d)), buf


def ref_rounds(X, Y, idx, steps, lr, server, replicas, in_mom, mom_init,
               snap, k_cut, w_off, b_off, K, loss_kind, wd, m, damp,
               nesterov, dtype=F64, chk=None, check_loss=True):
    """linear_local_rounds as a plain loop in `dtype`.  Nothing is modified;
    returns dict(replicas, in_mom, mom_init, snap, loss) where untouched
    rows are copies of the inputs."""
    chk = chk or _NoCheck()
    none = _NoCheck()
    C, T, _B = idx.shape
    F = X.shape[1]
    nw = K * F
    out = dict(replicas=replicas.to(dtype).clone(),
               in_mom=None if in_mom is None else in_mom.to(dtype).clone(),
               mom_init=mom_init.clone(),
               snap=None if snap is None else snap.to(dtype).clone(),
               loss=torch.zeros((C, T), dtype=dtype))
    Xd = X.to(dtype)
    for c in range(C):
        ns = int(steps[c])
        if ns <= 0:
            continue
        p = server.to(dtype).clone()
        W = p[w_off:w_off + nw].view(K, F).clone()
        b = p[b_off:b_off + K].clone()
        had = bool(mom_init[c]) if m != 0 else False
        mW = mb = None
        if m != 0:
            mo = in_mom[c].to(dtype)
            mW = mo[w_off:w_off + nw].view(K, F).clone()
            mb = mo[b_off:b_off + K].clone()
        for s in range(ns):
            if snap is not None and s + 1 == k_cut:
                out['snap'][c].copy_(p)
                out['snap'][c][w_off:w_off + nw] = W.reshape(-1)
                out['snap'][c][b_off:b_off + K] = b
            rows = idx[c, s]
            rows = rows[rows >= 0].long()
            n = len(rows)
            x = Xd[rows]                                       # [n, F]
            z = chk.value(chk.sum(x[:, None, :] * W[None], 2) + b)
            if loss_kind == 0:
                y = Y[rows].long()
                lse = torch.logsumexp(z, 1)
                l = (lse - z[torch.arange(n), y]).sum() / n
                dz = torch.softmax(z, 1)
                dz[torch.arange(n), y] -= 1
                dz = chk.value(dz / n)
            else:
                d = chk.value(z - Y[rows].to(dtype)[:, None])
                lc = chk if check_loss else none
                l = lc.value(lc.sum((d * d).reshape(-1), 0) / n)
                dz = chk.value(2 * d / n)
            out['loss'][c, s] = l
            gW = chk.sum(dz[:, :, None] * x[:, None, :], 0)     # [K, F]
            gb = chk.sum(dz, 0)
            lr_s = float(lr[c, s])
            first = m != 0 and not had
            W, mW = sgd_update(W, gW, mW, first, lr_s, wd, m, damp,
                               nesterov, chk)
            b, mb = sgd_update(b, gb, mb, first, lr_s, wd, m, damp,
                               nesterov, chk)
            had = True
        p[w_off:w_off + nw] = W.reshape(-1)
        p[b_off:b_off + K] = b
        out['replicas'][c].copy_(p)
        if m != 0:
            out['in_mom'][c][w_off:w_off + nw] = mW.reshape(-1)
            out['in_mom'][c][b_off:b_off + K] = mb
            out['mom_init'][c] = 1
    return out


# --------------------------------------------------------------------------
# operands
# --------------------------------------------------------------------------
def layout(F, K):
    """an arena-like layout with pad gaps: (N, w_off, b_off)"""
    al = lambda n: (n + 63) // 64 * 64  # noqa: E731
    w_off = 64                          # a leading gap as well
    b_off = w_off + al(K * F)
    return b_off + al(K), w_off, b_off


def make_case(g, F, K, B, C, T, M, loss_kind, steps, *, integer, m,
              short_last=True):
    """operands of one call (CPU tensors, fp32 / int32).  `steps`: list of
    C step counts.  The last executed step of client 0 gets a short batch
    (-1 padding) when `short_last`.  Pad gaps of server / in_mom are
    non-zero (they must pass through / stay)."""
    N, w_off, b_off = layout(F, K)
    if integer:
        # sparse small integers: at most 3 non-zero features per row
        X = torch.zeros(M, F)
        for r in range(M):
            cols = torch.randint(0, F, (3,), generator=g)
            X[r, cols] = torch.randint(-1, 2, (3,), generator=g).float()
        X[:, F - 1] = torch.randint(-1, 2, (M,), generator=g).float()
        server = torch.randint(-1, 2, (N,), generator=g).float()
        in_mom = torch.randint(-1, 2, (C, N), generator=g).float()
    else:
        X = torch.randn(M, F, generator=g)
        server = torch.randn(N, generator=g) / F ** .5
        in_mom = torch.randn(C, N, generator=g) * .1
    if loss_kind == 0:
        Y = torch.randint(0, K, (M,), generator=g).to(torch.int32)
    elif integer:
        Y = torch.randint(-1, 2, (M,), generator=g).float()
    else:
        Y = torch.randn(M, generator=g)
    idx = torch.full((C, T, B), -1, dtype=torch.int32)
    for c in range(C):
        for s in range(steps[c]):
            idx[c, s] = torch.randint(0, M, (B,), generator=g)
    if short_last and steps[0] > 0 and B > 1:
        idx[0, steps[0] - 1, B // 2:] = -1
    mom_init = (torch.arange(C) % 2).to(torch.int32)   # differs per client
    return dict(X=X, Y=Y, idx=idx,
                steps=torch.tensor(steps, dtype=torch.int32),
                server=server, replicas=torch.full((C, N), NAN),
                in_mom=in_mom if m != 0 else None, mom_init=mom_init,
                N=N, w_off=w_off, b_off=b_off, K=K, loss_kind=loss_kind)


# exact least-squares cases: (F, B, C, tau, log2(1/lr), wd, momentum).
# B a power of two, lr and wd powers of two or zero, momentum 0 or 0.5.
# tau and lr are sized per shape so that `exact_case` can assert the
# precondition (the denominators grow by lr * 2 / B per step, and the loss
# squares them).
EXACT_LS = [
    (1, 2, 1, 3, 1, 0.0, 0.0),
    (1, 4, 3, 2, 1, 0.25, 0.5),
    (7, 4, 3, 3, 2, 0.0, 0.5),
    (7, 16, 5, 2, 1, 0.5, 0.0),
    (60, 16, 5, 2, 2, 0.0, 0.5),
    (60, 2, 1, 3, 1, 0.25, 0.0),
    (257, 64, 3, 2, 0, 0.0, 0.0),
    (257, 4, 5, 3, 2, 0.0, 0.5),
    (784, 16, 1, 2, 1, 0.0, 0.5),
    (784, 64, 5, 2, 0, 0.25, 0.0),
]
# exact softmax-CE cases at K = 2 from zero weights, one step:
# (F, B, C, log2(1/lr), momentum)
EXACT_CE = [(7, 4, 3, 2, 0.5), (257, 16, 1, 1, 0.0), (784, 64, 5, 3, 0.5)]


def _run_ref(case, lr, k_cut, hp, dtype=F64, chk=None, snap=None,
             check_loss=True):
    return ref_rounds(case['X'], case['Y'], case['idx'], case['steps'], lr,
                      case['server'], case['replicas'], case['in_mom'],
                      case['mom_init'], snap, k_cut, case['w_off'],
                      case['b_off'], case['K'], case['loss_kind'], hp['wd'],
                      hp['m'], hp['damp'], hp['nesterov'], dtype=dtype,
                      chk=chk, check_loss=check_loss)


def exact_case(F, B, C, tau, lr_exp, wd, m, loss_kind=1):
    """(case, lr, k_cut, hp, snap, ref64) of an exact case; asserts its
    precondition.  One client is offline when C > 1."""
    g = gen('exact', F, B, C, tau, loss_kind)
    K = 1 if loss_kind == 1 else 2
    steps = [tau if (c != 1) else 0 for c in range(C)]
    if C > 2:
        steps[2] = max(tau - 1, 1)
    case = make_case(g, F, K, B, C, tau, 3 * B + 5, loss_kind, steps,
                     integer=True, m=m)
    if loss_kind == 0:
        w, k = case['w_off'], case['K']
        case['server'][w:w + k * F] = 0
        case['server'][case['b_off']:case['b_off'] + k] = 0
        case['mom_init'].zero_()      # one step from a fresh buffer: buf = d
    lr = torch.full((C, tau), 2.0 ** -lr_exp)
    hp = dict(wd=wd, m=m, damp=0.0, nesterov=False)
    k_cut = tau
    snap = torch.full((C, case['N']), NAN)
    chk = Exactness()
    ref = _run_ref(case, lr, k_cut, hp, chk=chk, snap=snap,
                   check_loss=loss_kind == 1)
    assert chk.ok(), ('exact case leaves fp32', (F, B, C, tau, lr_exp),
                      math.log2(chk.worst))
    return case, lr, k_cut, hp, snap, ref


# random-valued companions: (loss_kind, K, F, B, C, tau)
RANDOM = [(0, 2, 60, 16, 3, 3), (0, 10, 257, 50, 3, 3),
          (0, 16, 784, 64, 2, 3), (1, 1, 90, 50, 3, 3)]


def random_case(loss_kind, K, F, B, C, tau):
    """(case, lr, k_cut, hp, snap, ref64, e32): e32 is the largest error of
    the same loop run in fp32 on the CPU, per output."""
    g = gen('random', loss_kind, K, F, B, C, tau)
    steps = [tau] * C
    if C > 1:
        steps[1] = 0
    case = make_case(g, F, K, B, C, tau, 4 * B + 3, loss_kind, steps,
                     integer=False, m=0.9)
    lr = (torch.rand(C, tau, generator=g) * .05 + .01)
    hp = dict(wd=1e-3, m=0.9, damp=0.0, nesterov=True)
    k_cut = 2
    snap = torch.full((C, case['N']), NAN)
    ref = _run_ref(case, lr, k_cut, hp, snap=snap)
    r32 = _run_ref(case, lr, k_cut, hp, dtype=torch.float32, snap=snap)
    e32 = {k: err(r32[k], ref[k]) for k in ('replicas', 'in_mom', 'snap',
                                            'loss')}
    return case, lr, k_cut, hp, snap, ref, e32


def err(got, want64):
    """largest absolute error over the elements the reference defines"""
    want = want64.double()
    live = ~torch.isnan(want)
    if not bool(live.any()):
        return 0.0
    return (got.double().cpu()[live] - want[live]).abs().max().item()


def same_nan_pattern(got, want):
    return torch.equal(torch.isnan(got.cpu()), torch.isnan(want))


def bound(e32, scale, mult=8.0, ulps=16.0):
    """tolerance of a random case: `mult` times the fp32 CPU loop's own
    error plus `ulps` fp32 ulps of the output's scale"""
    return mult * e32 + ulps * 2.0 ** -24 * scale


def call_op(ops, case, lr, k_cut, hp, snap, device='cpu'):
    """run ops.linear_local_rounds on copies of the case's operands on
    `device`; returns dict like ref_rounds"""
    d = lambda t: None if t is None else t.clone().to(device)  # noqa: E731
    rep, mom, mi, sn = (d(case['replicas']), d(case['in_mom']),
                        d(case['mom_init']), d(snap))
    loss = ops.linear_local_rounds(
        d(case['X']), d(case['Y']), d(case['idx']), d(case['steps']),
        d(lr), d(case['server']), rep, mom, mi, sn, k_cut,
        w_off=case['w_off'], b_off=case['b_off'], K=case['K'],
        loss_kind=case['loss_kind'], weight_decay=hp['wd'],
        momentum=hp['m'], dampening=hp['damp'], nesterov=hp['nesterov'])
    return dict(replicas=rep, in_mom=mom, mom_init=mi, snap=sn, loss=loss)
