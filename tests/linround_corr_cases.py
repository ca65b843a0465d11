# -*- coding: utf-8 -*-
"""References and case generators for the gradient-correction term of
ops.linear_local_rounds (delta / the control pair / prox_mu): the step loop
of linround_cases.ref_rounds with fused_sgd_step's corrections inserted in
front of the SGD update, exact dyadic cases and random-valued ones.  Shared
by test_linround_corr_cpu.py and test_gpu_linround_corr.py."""
import math

import torch

from linround_cases import (make_case, sgd_update, Exactness, bound, err,  # noqa: F401
                            gen, layout, _NoCheck, F64, NAN)

KINDS = ('delta', 'ctrl', 'prox')


def correct(g, p, p_srv, dl, cs, cc, mu, chk):
    """d = g ; d -= delta ; d += c - c_j ; d += mu (p - x): the order of
    ops.fused_sgd_step"""
    d = g
    if dl is not None:
        d = chk.value(d - dl)
    if cs is not None:
        d = chk.value(d + chk.value(cs - cc))
    if mu != 0:
        d = chk.value(d + chk.value(mu * chk.value(p - p_srv)))
    return d


def ref_rounds_corr(case, lr, k_cut, hp, corr, dtype=F64, chk=None, snap=None,
                    check_loss=True):
    """linear_local_rounds with a correction as a plain loop in `dtype`.
    corr: dict(delta [C, N] | None, ctrl_server [N] | None,
    ctrl_client [C, N] | None, prox_mu).  Only the weight / bias elements of
    the correction rows of online clients are touched.  Returns the dict of
    linround_cases.ref_rounds."""
    chk = chk or _NoCheck()
    none = _NoCheck()
    X, Y, idx, steps = case['X'], case['Y'], case['idx'], case['steps']
    server, in_mom, mom_init = case['server'], case['in_mom'], case['mom_init']
    w_off, b_off, K = case['w_off'], case['b_off'], case['K']
    loss_kind = case['loss_kind']
    wd, m, damp, nesterov = hp['wd'], hp['m'], hp['damp'], hp['nesterov']
    mu = corr.get('prox_mu', 0.0)
    C, T, _B = idx.shape
    F = X.shape[1]
    nw = K * F
    out = dict(replicas=case['replicas'].to(dtype).clone(),
               in_mom=None if in_mom is None else in_mom.to(dtype).clone(),
               mom_init=mom_init.clone(),
               snap=None if snap is None else snap.to(dtype).clone(),
               loss=torch.zeros((C, T), dtype=dtype))
    Xd = X.to(dtype)

    def wb(t):
        t = t.to(dtype)
        return (t[w_off:w_off + nw].view(K, F).clone(),
                t[b_off:b_off + K].clone())

    for c in range(C):
        ns = int(steps[c])
        if ns <= 0:
            continue
        p = server.to(dtype).clone()
        W, b = wb(p)
        W0, b0 = wb(p)
        dW = db = csW = csb = ccW = ccb = None
        if corr.get('delta') is not None:
            dW, db = wb(corr['delta'][c])
        if corr.get('ctrl_server') is not None:
            csW, csb = wb(corr['ctrl_server'])
            ccW, ccb = wb(corr['ctrl_client'][c])
        had = bool(mom_init[c]) if m != 0 else False
        mW = mb = None
        if m != 0:
            mW, mb = wb(in_mom[c])
        for s in range(ns):
            if snap is not None and s + 1 == k_cut:
                out['snap'][c].copy_(p)
                out['snap'][c][w_off:w_off + nw] = W.reshape(-1)
                out['snap'][c][b_off:b_off + K] = b
            rows = idx[c, s]
            rows = rows[rows >= 0].long()
            n = len(rows)
            x = Xd[rows]
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
                lc_ = chk if check_loss else none
                l = lc_.value(lc_.sum((d * d).reshape(-1), 0) / n)
                dz = chk.value(2 * d / n)
            out['loss'][c, s] = l
            gW = chk.sum(dz[:, :, None] * x[:, None, :], 0)
            gb = chk.sum(dz, 0)
            gW = correct(gW, W, W0, dW, csW, ccW, mu, chk)
            gb = correct(gb, b, b0, db, csb, ccb, mu, chk)
            lr_s = float(lr[c, s])
            first = m != 0 and not had
            W, mW = sgd_update(W, gW, mW, first, lr_s, wd, m, damp, nesterov,
                               chk)
            b, mb = sgd_update(b, gb, mb, first, lr_s, wd, m, damp, nesterov,
                               chk)
            had = True
        p[w_off:w_off + nw] = W.reshape(-1)
        p[b_off:b_off + K] = b
        out['replicas'][c].copy_(p)
        if m != 0:
            out['in_mom'][c][w_off:w_off + nw] = mW.reshape(-1)
            out['in_mom'][c][b_off:b_off + K] = mb
            out['mom_init'][c] = 1
    return out


def make_corr(g, case, kind, integer, mu):
    """the correction operands of `kind` for a case: values only where the
    kernel may read them — NaN in the pad gaps and in the rows of offline
    clients"""
    N, K = case['N'], case['K']
    F = case['X'].shape[1]
    C = case['idx'].shape[0]
    live = torch.zeros(N, dtype=torch.bool)
    live[case['w_off']:case['w_off'] + K * F] = True
    live[case['b_off']:case['b_off'] + K] = True

    def draw(*shape):
        if integer:
            t = torch.randint(-1, 2, shape + (N,), generator=g).float()
        else:
            t = torch.randn(shape + (N,), generator=g) * .1
        return torch.where(live, t, torch.full_like(t, NAN))

    def rows():
        t = draw(C)
        for c in range(C):
            if int(case['steps'][c]) <= 0:
                t[c] = NAN
        return t

    corr = dict(delta=None, ctrl_server=None, ctrl_client=None, prox_mu=0.0)
    if kind == 'delta':
        corr['delta'] = rows()
    elif kind == 'ctrl':
        corr['ctrl_server'] = draw()
        corr['ctrl_client'] = rows()
    elif kind == 'prox':
        corr['prox_mu'] = mu
    else:
        raise ValueError(kind)
    return corr


# exact least-squares cases (K = 1): (F, B, tau, log2(1/lr), wd, momentum, mu),
# C = 3 with client 1 offline and client 2 one step short; sized like
# linround_cases.EXACT_LS so that the precondition holds with a correction
# drawn from {-1, 0, 1} (it adds one unit per step to the gradient's range
# and nothing to its denominator; mu a power of two adds two bits).
EXACT_LS = [
    (1, 2, 3, 1, 0.0, 0.5, 0.5),
    (7, 16, 2, 1, 0.25, 0.5, 0.25),
    (257, 2, 3, 2, 0.0, 0.5, 0.5),
    (257, 16, 2, 1, 0.0, 0.0, 0.25),
    (784, 16, 2, 1, 0.0, 0.5, 0.5),
    (784, 2, 2, 1, 0.25, 0.0, 0.25),
]
# exact softmax-CE cases at K = 2 from zero weights, one step:
# (F, B, log2(1/lr), momentum, mu)
EXACT_CE = [(7, 2, 2, 0.5, 0.5), (257, 16, 1, 0.0, 0.25),
            (784, 16, 3, 0.5, 0.5)]


def exact_case(kind, F, B, tau, lr_exp, wd, m, mu, loss_kind=1):
    """(case, lr, k_cut, hp, snap, corr, ref64) of an exact case with a
    correction of `kind`; asserts its precondition."""
    C = 3
    g = gen('exact-corr', kind, F, B, tau, loss_kind)
    K = 1 if loss_kind == 1 else 2
    steps = [tau, 0, max(tau - 1, 1)]
    case = make_case(g, F, K, B, C, tau, 3 * B + 5, loss_kind, steps,
                     integer=True, m=m)
    if loss_kind == 0:
        w = case['w_off']
        case['server'][w:w + K * F] = 0
        case['server'][case['b_off']:case['b_off'] + K] = 0
    corr = make_corr(g, case, kind, True, mu)
    lr = torch.full((C, tau), 2.0 ** -lr_exp)
    hp = dict(wd=wd, m=m, damp=0.0, nesterov=False)
    k_cut = tau
    snap = torch.full((C, case['N']), NAN)
    chk = Exactness()
    ref = ref_rounds_corr(case, lr, k_cut, hp, corr, chk=chk, snap=snap,
                          check_loss=loss_kind == 1)
    assert chk.ok(), ('exact case leaves fp32', (kind, F, B, tau, lr_exp),
                      math.log2(chk.worst))
    return case, lr, k_cut, hp, snap, corr, ref


# random-valued companions: (loss_kind, K, F, B, C, tau), the shapes of
# linround_cases.RANDOM; momentum 0.9 with nesterov and weight decay
RANDOM = [(0, 2, 60, 16, 3, 3), (0, 10, 257, 50, 3, 3),
          (0, 16, 784, 64, 2, 3), (1, 1, 90, 50, 3, 3)]
OUTPUTS = ('replicas', 'in_mom', 'snap', 'loss')


def random_case(kind, loss_kind, K, F, B, C, tau):
    """(case, lr, k_cut, hp, snap, corr, ref64, e32): e32 is the largest
    error of the same loop run in fp32 on the CPU, per output."""
    g = gen('random-corr', kind, loss_kind, K, F, B, C, tau)
    steps = [tau] * C
    if C > 1:
        steps[1] = 0
    case = make_case(g, F, K, B, C, tau, 4 * B + 3, loss_kind, steps,
                     integer=False, m=0.9)
    corr = make_corr(g, case, kind, False, 0.1)
    lr = (torch.rand(C, tau, generator=g) * .05 + .01)
    hp = dict(wd=1e-3, m=0.9, damp=0.0, nesterov=True)
    k_cut = 2
    snap = torch.full((C, case['N']), NAN)
    ref = ref_rounds_corr(case, lr, k_cut, hp, corr, snap=snap)
    r32 = ref_rounds_corr(case, lr, k_cut, hp, corr, dtype=torch.float32,
                          snap=snap)
    e32 = {k: err(r32[k], ref[k]) for k in OUTPUTS}
    return case, lr, k_cut, hp, snap, corr, ref, e32


def corr_kwargs(corr, device='cpu'):
    d = lambda t: None if t is None else t.clone().to(device)  # noqa: E731
    return dict(delta=d(corr['delta']), ctrl_server=d(corr['ctrl_server']),
                ctrl_client=d(corr['ctrl_client']), prox_mu=corr['prox_mu'])


def call_op(ops, case, lr, k_cut, hp, snap, corr, device='cpu'):
    """run ops.linear_local_rounds with the correction on copies of the
    operands on `device`; returns dict like ref_rounds_corr"""
    d = lambda t: None if t is None else t.clone().to(device)  # noqa: E731
    rep, mom, mi, sn = (d(case['replicas']), d(case['in_mom']),
                        d(case['mom_init']), d(snap))
    loss = ops.linear_local_rounds(
        d(case['X']), d(case['Y']), d(case['idx']), d(case['steps']),
        d(lr), d(case['server']), rep, mom, mi, sn, k_cut,
        w_off=case['w_off'], b_off=case['b_off'], K=case['K'],
        loss_kind=case['loss_kind'], weight_decay=hp['wd'],
        momentum=hp['m'], dampening=hp['damp'], nesterov=hp['nesterov'],
        **corr_kwargs(corr, device))
    return dict(replicas=rep, in_mom=mom, mom_init=mi, snap=sn, loss=loss)


# --------------------------------------------------------------------------
# the two batched row ops
# --------------------------------------------------------------------------
def row_case(C, N, offline=(1,)):
    """operands of multi_delta_update / multi_scaffold_control_update: the
    rows of `offline` clients are NaN and their inv is 0"""
    g = gen('rows', C, N)
    t = dict(state=torch.randn(C, N, generator=g) * .1,
             ctrl_server=torch.randn(N, generator=g) * .1,
             server=torch.randn(N, generator=g),
             agg=torch.randn(N, generator=g) * .05,
             replicas=torch.randn(C, N, generator=g),
             inv=1.0 / (torch.rand(C, generator=g) * .3 + .05),
             weights=torch.rand(C, generator=g) * .5)
    for c in offline:
        if c < C:
            t['state'][c] = NAN
            t['replicas'][c] = NAN
            t['inv'][c] = 0
    return t


def ref_delta_rows(t, dtype=F64):
    out = t['state'].to(dtype).clone()
    s, a = t['server'].to(dtype), t['agg'].to(dtype)
    for c in range(out.shape[0]):
        if float(t['inv'][c]) != 0:
            out[c] += (s - a - t['replicas'][c].to(dtype)) \
                * t['inv'][c].to(dtype)
    return out


def ref_ctrl_rows(t, dtype=F64):
    """(ctrl rows, out)"""
    ctrl = t['state'].to(dtype).clone()
    s, cs = t['server'].to(dtype), t['ctrl_server'].to(dtype)
    out = torch.zeros_like(s)
    for c in range(ctrl.shape[0]):
        if float(t['inv'][c]) != 0:
            new = ctrl[c] - cs + (s - t['replicas'][c].to(dtype)) \
                * t['inv'][c].to(dtype)
            out += t['weights'][c].to(dtype) * (new - ctrl[c])
            ctrl[c] = new
    return ctrl, out


# --------------------------------------------------------------------------
# a packed federation: recording run and plain-loop replay
# --------------------------------------------------------------------------
def layout_meta(client, pack):
    w_off, b_off, K, F = pack.linear_layout()
    g = client.optimizer.param_groups[0]
    a = client.args
    assert not a.out_momentum and client.arena.wd_numel == client.arena.numel
    return dict(w_off=w_off, b_off=b_off, K=K, F=F, N=client.arena.numel,
                C=pack.C, total=pack.total_clients, wd=g['weight_decay'],
                m=g['in_momentum'] if a.in_momentum else 0.0,
                damp=g['dampening'], nesterov=g['nesterov'],
                mu=a.fedprox_mu, lr_scale=a.lr_scale_at_sync,
                ftype=a.federated_type)



def run_federation(client, pack, monkeypatch, record=False,
                   record_calls=False):
    """train_and_validate_federated_packed from a fixed non-trivial start;
    returns (final state on the CPU, meta, recording).  `record`: the slot
    loop's batches, lrs, weights and online counts per round, for
    replay_federation.  `record_calls`: operands (before) and replicas /
    in_mom (after) of every ops.linear_local_rounds call."""
    import numpy as np
    import fedtorch_amd.ops as ops
    from fedtorch_amd.trainings import packed
    meta = layout_meta(client, pack)
    dev = client.model_server.device
    g = gen('corr-start')
    start = torch.randn(meta['N'], generator=g) * .05
    gap = torch.ones(meta['N'], dtype=torch.bool)
    gap[meta['w_off']:meta['w_off'] + meta['K'] * meta['F']] = False
    gap[meta['b_off']:meta['b_off'] + meta['K']] = False
    start[gap] = 0                  # pad gaps zero as in a real arena
    client.model_server.copy_(start.to(dev))
    rec = dict(start=start.clone(), rounds=[], sampled=[], calls=[])
    cur = dict(j=None, steps=None, clients={})
    if record:
        real_load, real_run = packed.load_data_batch, pack.run_client
        real_acc = pack.accumulate_partial
        real_sample = client.comm.sample_online_global

        def load(args, x, y, tracker):
            if cur['j'] is not None:
                assert len(y) > 1
                cur['steps'].append(
                    (x.detach().cpu().clone(), y.detach().cpu().clone(),
                     client.optimizer.param_groups[0]['lr']))
            return real_load(args, x, y, tracker)

        def run_client(j, server_flat, fn):
            cur['j'], cur['steps'] = j, []
            tau = real_run(j, server_flat, fn)
            assert tau == len(cur['steps'])
            cur['clients'][j] = cur['steps']
            cur['j'] = None
            return tau

        def acc(server, weights):
            rec['rounds'].append(dict(clients=cur['clients'],
                                      weights=list(weights),
                                      n_sampled=len(rec['sampled'][-1])))
            cur['clients'] = {}
            return real_acc(server, weights)

        def sample(total):
            rec['sampled'].append(list(real_sample(total)))
            return rec['sampled'][-1]
        monkeypatch.setattr(packed, 'load_data_batch', load)
        monkeypatch.setattr(pack, 'run_client', run_client)
        monkeypatch.setattr(pack, 'accumulate_partial', acc)
        monkeypatch.setattr(client.comm, 'sample_online_global', sample)
    real_op = ops.linear_local_rounds

    def keep(t):
        return t.detach().cpu().clone() if torch.is_tensor(t) else t

    def op(*a, **k):
        call = dict(pos=[keep(t) for t in a] if record_calls else None,
                    kw={n: keep(v) for n, v in k.items()}
                    if record_calls else None)
        loss = real_op(*a, **k)
        if record_calls:
            call.update(replicas=keep(a[6]), in_mom=keep(a[7]))
        rec['calls'].append(call)
        return loss
    monkeypatch.setattr(ops, 'linear_local_rounds', op)
    torch.manual_seed(6)
    np.random.seed(6)
    packed.train_and_validate_federated_packed(client, pack)
    # the correction is cleared after the slot loop
    opt = client.optimizer
    assert opt._prox_mu == 0.0 and opt._delta is None \
        and opt._ctrl_server is None and opt._ctrl_client is None \
        and opt._server is None
    out = dict(server=keep(client.model_server))
    if pack.delta is not None:
        out['delta'] = keep(pack.delta)
    if pack.ctrl is not None:
        out['ctrl'] = keep(pack.ctrl)
        out['c'] = keep(client.model_server_control)
    return out, meta, rec


def replay_federation(rec, meta, dtype, correction=True):
    """sections 1-2 of the round structure (module docstring of
    trainings/packed.py) as a plain loop in `dtype` over the recorded
    batches, lrs, weights and online counts.  Returns (final state, the
    largest |correction state| entering each round)."""
    nochk = _NoCheck()
    N, C, K, F = meta['N'], meta['C'], meta['K'], meta['F']
    w_off, b_off, ftype = meta['w_off'], meta['b_off'], meta['ftype']
    x = rec['start'].to(dtype).clone()
    delta = torch.zeros(C, N, dtype=dtype)
    ctrl = torch.zeros(C, N, dtype=dtype)
    c = torch.zeros(N, dtype=dtype)
    mom = [None] * C
    entering = []
    for rnd in rec['rounds']:
        entering.append(max(delta.abs().max().item(),
                            ctrl.abs().max().item(), c.abs().max().item()))
        ys, taus, lrs = {}, {}, {}
        for j, steps in rnd['clients'].items():
            p = x.clone()
            for xb, yb, lr in steps:
                xb = xb.reshape(len(yb), -1).to(dtype)
                n = len(yb)
                W = p[w_off:w_off + K * F].view(K, F)
                z = xb @ W.t() + p[b_off:b_off + K]
                dz = torch.softmax(z, 1)
                dz[torch.arange(n), yb.long()] -= 1
                dz = dz / n
                d = torch.zeros(N, dtype=dtype)
                d[w_off:w_off + K * F] = (dz.t() @ xb).reshape(-1)
                d[b_off:b_off + K] = dz.sum(0)
                if correction and ftype == 'fedgate':
                    d = d - delta[j]
                elif correction and ftype == 'scaffold':
                    d = d + (c - ctrl[j])
                elif correction and ftype == 'fedprox':
                    d = d + meta['mu'] * (p - x)
                p, mom[j] = sgd_update(
                    p, d, mom[j], mom[j] is None, lr, meta['wd'], meta['m'],
                    meta['damp'], meta['nesterov'], nochk)
            ys[j], taus[j], lrs[j] = p, len(steps), steps[-1][2]
        w = rnd['weights']
        part = [j for j in sorted(ys) if w[j] != 0.0 and taus[j] > 0]
        partial = torch.zeros(N, dtype=dtype)
        for j in sorted(ys):
            partial += w[j] * (x - ys[j])
        if ftype == 'scaffold':
            b = torch.zeros(N, dtype=dtype)
            for j in part:
                new = ctrl[j] - c + (x - ys[j]) / (taus[j] * lrs[j])
                b += w[j] * (new - ctrl[j])
                ctrl[j] = new
            c = c + b * rnd['n_sampled'] / meta['total']
        if ftype == 'fedgate':
            for j in part:
                delta[j] += (x - partial - ys[j]) / (lrs[j] * taus[j])
        x = x - meta['lr_scale'] * partial
    out = dict(server=x)
    if ftype == 'fedgate':
        out['delta'] = delta
    if ftype == 'scaffold':
        out['ctrl'], out['c'] = ctrl, c
    return out, entering
