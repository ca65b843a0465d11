# -*- coding: utf-8 -*-
"""Reference and case generator for the gradient-correction term of
ops.mlp_local_rounds (delta / the control pair / prox_mu): the step loop of
mlpround_cases.ref_rounds, forward and backward as they stand there, with
fused_sgd_step's corrections put in front of its SGD update; random-valued
cases whose ReLU pre-activations stay clear of zero; and the recording run
and plain-loop replay of a packed MLP federation.  Shared by
test_mlpround_corr_cpu.py and test_gpu_mlpround_corr.py."""
import contextlib
import functools

import torch

import linround_cases as lc
import mlpround_cases as mc

F64, F32, NAN = mc.F64, mc.F32, mc.NAN
KINDS = ('delta', 'ctrl', 'prox')
OUTPUTS = mc.OUTPUTS
MU = 0.1


# --------------------------------------------------------------------------
# the reference: mlpround_cases.ref_rounds with a corrected gradient
# --------------------------------------------------------------------------
@contextlib.contextmanager
def _corrected_sgd(server, dl, cs, cc, mu):
    """while active, mc.ref_rounds updates with d = g ; d -= delta ;
    d += c - c_j ; d += mu (p - x) -- the order of ops.fused_sgd_step -- in
    place of g.  ref_rounds forms all gradients of a step before the first
    update, so p[lo:hi] is the pre-update value."""
    real = mc._sgd

    def sgd(p, buf, lo, hi, g, *rest):
        d = g.reshape(-1)
        if dl is not None:
            d = d - dl[lo:hi]
        if cs is not None:
            d = d + (cs[lo:hi] - cc[lo:hi])
        if mu != 0:
            d = d + mu * (p[lo:hi] - server[lo:hi])
        real(p, buf, lo, hi, d, *rest)
    mc._sgd = sgd
    try:
        yield
    finally:
        mc._sgd = real


def ref_rounds_corr(X, Y, idx, steps, lr, server, replicas, in_mom, mom_init,
                    snap, k_cut, layout, eps, wd_numel, wd, m, damp, nesterov,
                    corr, dtype=F64, pre=None):
    """mlp_local_rounds with a correction as a plain loop in `dtype`: one
    mc.ref_rounds call per client, with that client's correction row.  corr:
    dict(delta [C, N] | None, ctrl_server [N] | None, ctrl_client [C, N] |
    None, prox_mu).  The correction rows of offline clients are not touched.
    Returns the dict of mc.ref_rounds."""
    C = idx.shape[0]
    row = lambda t, c: None if t is None else t[c:c + 1]  # noqa: E731
    cast = lambda t: None if t is None else t.to(dtype)  # noqa: E731
    outs = []
    for c in range(C):
        online = int(steps[c]) > 0
        dl = cast(corr['delta'][c]) \
            if online and corr.get('delta') is not None else None
        cs = cc = None
        if online and corr.get('ctrl_server') is not None:
            cs, cc = cast(corr['ctrl_server']), cast(corr['ctrl_client'][c])
        with _corrected_sgd(server.to(dtype), dl, cs, cc,
                            corr.get('prox_mu', 0.0)):
            outs.append(mc.ref_rounds(
                X, Y, idx[c:c + 1], steps[c:c + 1], lr[c:c + 1], server,
                replicas[c:c + 1], row(in_mom, c), mom_init[c:c + 1],
                row(snap, c), k_cut, layout, eps, wd_numel, wd, m, damp,
                nesterov, dtype=dtype, pre=pre))
    return {k: None if outs[0][k] is None else torch.cat([o[k] for o in outs])
            for k in outs[0]}


def no_corr():
    return dict(delta=None, ctrl_server=None, ctrl_client=None, prox_mu=0.0)


def make_corr(g, case, kind, mu=MU):
    """the correction operands of `kind` for a case: random values of scale
    0.1 only where the kernels may read them -- NaN in the pad gaps and in
    the rows of offline clients"""
    N = case['N']
    C = case['idx'].shape[0]
    live = ~mc.gap_mask(case['layout'], N)

    def draw(*shape):
        t = torch.randn(shape + (N,), generator=g) * .1
        return torch.where(live, t, torch.full_like(t, NAN))

    def rows():
        t = draw(C)
        for c in range(C):
            if int(case['steps'][c]) <= 0:
                t[c] = NAN
        return t

    corr = no_corr()
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


# --------------------------------------------------------------------------
# cases
# --------------------------------------------------------------------------
# (F, H, K, L, B) -> hyper-parameters, the short batch (client, step, n),
# k_cut (inside the round of a client), whether wd covers only a prefix that
# ends inside the head's weight, mom_init and the seed per kind.  Every seed
# is checked by `case()` (the ReLU precondition of mlpround_cases.case, with
# its MARGIN); they were searched on the CPU for a margin of at least 80.
# The short steps keep at least 3 rows: BatchNorm over 2 rows normalises to
# +-1 up to eps and amplifies a rounding by up to 1 / sqrt(eps) = 316, which
# makes the fp32 replay's error a heavy-tailed estimate (in_mom of the second
# shape over 24 seeds: 5e-7 .. 0.3 at n = 2, 1.8e-7 .. 1.1e-6 at n = 5).  The
# two-row step is an edge of the forward and BatchNorm code, which
# test_gpu_mlpround.py covers at the same shape; the correction term does
# not depend on n.
CASES = {
    # one block: the head boundary is the only one; one column tile, K = 2
    (14, 33, 2, 1, 5): dict(
        hp=dict(wd=0.0, m=0.0, damp=0.0, nesterov=False), short=(0, 2, 3),
        k_cut=2, wd_part=False, mom_init=[0, 1, 0],
        seeds=dict(delta=0, ctrl=0, prox=0)),
    # partial tiles in F, H and K; a block boundary next to the head's
    (45, 70, 10, 2, 16): dict(
        hp=dict(wd=5e-4, m=0.9, damp=0.0, nesterov=True), short=(2, 1, 5),
        k_cut=3, wd_part=True, mom_init=[0, 1, 1],
        seeds=dict(delta=2, ctrl=0, prox=6)),
    # a middle block with a block on both sides
    (37, 40, 3, 3, 8): dict(
        hp=dict(wd=5e-4, m=0.9, damp=0.0, nesterov=False), short=(0, 1, 5),
        k_cut=1, wd_part=False, mom_init=[1, 0, 0],
        seeds=dict(delta=0, ctrl=3, prox=1)),
}
SHAPES = list(CASES)
STEPS = mc.STEPS           # C = 3: client 1 offline, unequal steps
PAIRS = [(s, k) for s in SHAPES for k in KINDS]


def run_ref(case, lr, k_cut, hp, snap, wd_numel, corr, dtype=F64, pre=None):
    return ref_rounds_corr(
        case['X'], case['Y'], case['idx'], case['steps'], lr, case['server'],
        case['replicas'], case['in_mom'], case['mom_init'], snap, k_cut,
        case['layout'], case['eps'], wd_numel, hp['wd'], hp['m'], hp['damp'],
        hp['nesterov'], corr, dtype=dtype, pre=pre)


def relu_margin(pre64, pre32):
    """(smallest |y| of the float64 replay, largest error of the fp32 replay
    in y) over the recorded pre-ReLU values of valid rows"""
    lo = min(y.abs().min().item() for y in pre64)
    e = max((a.double() - b).abs().max().item()
            for a, b in zip(pre32, pre64))
    return lo, e


def build(shape, kind, seed):
    F, H, K, L, B = shape
    spec = CASES[shape]
    g = lc.gen('mlp-corr', F, H, K, L, B, kind, seed)
    hp = spec['hp']
    case = mc.make_case(g, F, H, K, L, B, STEPS, 3 * B + 7, m=hp['m'],
                        short=spec['short'], mom_init=spec['mom_init'])
    C, T = len(STEPS), max(STEPS)
    lr = torch.rand(C, T, generator=g) * .05 + .01      # changes per step
    snap = torch.full((C, case['N']), NAN)
    fc, Hh, Kh = case['layout']['head']
    wd_numel = fc + (Hh * Kh) // 2 if spec['wd_part'] else case['N']
    corr = make_corr(g, case, kind)
    return case, lr, spec['k_cut'], hp, snap, wd_numel, corr


def margin_of(shape, kind, seed):
    """(ref64, ref32, lo, e) of a candidate seed: the seed search runs this"""
    cs, lr, k_cut, hp, snap, wd_numel, corr = build(shape, kind, seed)
    p64, p32 = [], []
    ref = run_ref(cs, lr, k_cut, hp, snap, wd_numel, corr, pre=p64)
    r32 = run_ref(cs, lr, k_cut, hp, snap, wd_numel, corr, dtype=F32,
                  pre=p32)
    return (ref, r32) + relu_margin(p64, p32)


@functools.lru_cache(maxsize=None)
def case(shape, kind):
    """(case, lr, k_cut, hp, snap, wd_numel, corr, ref64, e32) of a (shape,
    kind) pair, computed once and shared: treat it as read-only.  e32: the
    largest error of the same loop in fp32 on the CPU, per output.  Asserts
    the ReLU precondition of mlpround_cases.case, unchanged."""
    seed = CASES[shape]['seeds'][kind]
    cs, lr, k_cut, hp, snap, wd_numel, corr = build(shape, kind, seed)
    ref, r32, lo, e = margin_of(shape, kind, seed)
    assert lo > mc.MARGIN * e, ('a pre-ReLU value is too close to zero',
                                (shape, kind, seed), lo, e)
    e32 = {k: lc.err(r32[k], ref[k]) for k in OUTPUTS if ref[k] is not None}
    return cs, lr, k_cut, hp, snap, wd_numel, corr, ref, e32


def corr_kwargs(corr, device='cpu'):
    d = lambda t: None if t is None else t.clone().to(device)  # noqa: E731
    return dict(delta=d(corr['delta']), ctrl_server=d(corr['ctrl_server']),
                ctrl_client=d(corr['ctrl_client']), prox_mu=corr['prox_mu'])


def call_op(ops, case, lr, k_cut, hp, snap, wd_numel, corr, device='cpu'):
    """run ops.mlp_local_rounds with the correction on copies of the case's
    operands on `device`; returns dict like ref_rounds_corr"""
    d = lambda t: None if t is None else t.clone().to(device)  # noqa: E731
    rep, mom, mi, sn = (d(case['replicas']), d(case['in_mom']),
                        d(case['mom_init']), d(snap))
    loss = ops.mlp_local_rounds(
        d(case['X']), d(case['Y']), d(case['idx']), d(case['steps']), d(lr),
        d(case['server']), rep, mom, mi, sn, k_cut, layout=case['layout'],
        eps=case['eps'], wd_numel=wd_numel, weight_decay=hp['wd'],
        momentum=hp['m'], dampening=hp['damp'], nesterov=hp['nesterov'],
        **corr_kwargs(corr, device))
    return dict(replicas=rep, in_mom=mom, mom_init=mi, snap=sn, loss=loss)


# --------------------------------------------------------------------------
# a packed MLP federation: recording run and plain-loop replay
# --------------------------------------------------------------------------
STATE = ('server', 'delta', 'ctrl', 'c')


def run_federation(client, pack, monkeypatch, real_op=None):
    """train_and_validate_federated_packed over (client, pack); returns the
    end state on the CPU with the counters, the operands of every
    ops.mlp_local_rounds call (cloned before the call) and each round's
    weights and online count."""
    import fedtorch_amd.ops as ops
    from fedtorch_amd.trainings.packed import \
        train_and_validate_federated_packed
    keep = lambda t: t.detach().cpu().clone() \
        if torch.is_tensor(t) else t  # noqa: E731
    calls, rounds, sampled = [], [], []
    real = real_op or ops.mlp_local_rounds

    def op(*a, **k):
        calls.append(([keep(t) for t in a],
                      {n: keep(v) for n, v in k.items()}))
        return real(*a, **k)
    monkeypatch.setattr(ops, 'mlp_local_rounds', op)
    lin = []
    monkeypatch.setattr(ops, 'linear_local_rounds',
                        lambda *a, **k: lin.append(1))
    real_acc, real_sample = pack.accumulate_partial, \
        client.comm.sample_online_global

    def acc(server, w):
        # the round's own sample is the latest one (DRFA draws its second
        # set after the aggregation)
        rounds.append(dict(weights=list(w), n_sampled=len(sampled[-1])))
        return real_acc(server, w)

    def sample(total):
        sampled.append(list(real_sample(total)))
        return sampled[-1]
    monkeypatch.setattr(pack, 'accumulate_partial', acc)
    monkeypatch.setattr(client.comm, 'sample_online_global', sample)
    start = keep(client.model_server)
    train_and_validate_federated_packed(client, pack)
    # nothing stays bound on the shared optimizer
    opt = client.optimizer
    assert opt._prox_mu == 0.0 and opt._delta is None \
        and opt._ctrl_server is None and opt._ctrl_client is None \
        and opt._server is None
    a = client.args
    assert not lin and not a.out_momentum
    out = dict(server=keep(client.model_server), start=start, calls=calls,
               rounds=rounds, mom_init=list(pack.mom_init),
               local_index=a.local_index, epoch_=a.epoch_,
               seen=a.local_data_seen, lr=a.old_learning_rate,
               gens=[l._gen.get_state() for l in pack.train_loaders],
               meta=dict(ftype=a.federated_type, total=pack.total_clients,
                         scale=a.lr_scale_at_sync, mu=a.fedprox_mu))
    if pack.delta is not None:
        out['delta'] = keep(pack.delta)
    if pack.ctrl is not None:
        out['ctrl'] = keep(pack.ctrl)
        out['c'] = keep(client.model_server_control)
    return out


def replay_federation(run, dtype, pre=None):
    """the whole federation (module docstring of trainings/packed.py) as a
    plain loop in `dtype` over the recorded batches, lrs, weights and online
    counts of a batched run: local steps by ref_rounds_corr with the
    replay's own delta / controls, then the aggregation.  Returns the end
    state dict(server[, delta | ctrl, c])."""
    meta = run['meta']
    ftype = meta['ftype']
    pos0 = run['calls'][0][0]
    x = run['start'].to(dtype).clone()
    replicas = pos0[6].to(dtype).clone()
    in_mom = None if pos0[7] is None else pos0[7].to(dtype).clone()
    mom_init = pos0[8].clone()
    C, N = replicas.shape
    delta = torch.zeros(C, N, dtype=dtype)
    ctrl = torch.zeros(C, N, dtype=dtype)
    c = torch.zeros(N, dtype=dtype)
    for (pos, kw), rnd in zip(run['calls'], run['rounds']):
        X, Y, idx, steps, lr = pos[:5]
        has_snap = pos[9] is not None
        corr = no_corr()
        if ftype == 'fedgate':
            corr['delta'] = delta
        elif ftype == 'scaffold':
            corr.update(ctrl_server=c, ctrl_client=ctrl)
        elif ftype == 'fedprox':
            corr['prox_mu'] = meta['mu']
        out = ref_rounds_corr(
            X, Y, idx, steps, lr, x, replicas, in_mom, mom_init,
            torch.zeros_like(replicas) if has_snap else None,
            pos[10] if has_snap else 0, kw['layout'], kw['eps'],
            kw['wd_numel'], kw['weight_decay'], kw['momentum'],
            kw['dampening'], kw['nesterov'], corr, dtype=dtype, pre=pre)
        replicas, in_mom, mom_init = (out['replicas'], out['in_mom'],
                                      out['mom_init'])
        w, taus = rnd['weights'], steps.tolist()
        part = [j for j in range(C) if w[j] != 0.0 and taus[j] > 0]
        lrs = {j: float(lr[j, taus[j] - 1]) for j in part}
        partial = torch.zeros_like(x)
        for j in range(C):
            if w[j] != 0.0:
                partial += w[j] * (x - replicas[j])
        if ftype == 'scaffold':
            b = torch.zeros_like(x)
            for j in part:
                new = ctrl[j] - c + (x - replicas[j]) / (taus[j] * lrs[j])
                b += w[j] * (new - ctrl[j])
                ctrl[j] = new
            c = c + b * rnd['n_sampled'] / meta['total']
        if ftype == 'fedgate':
            for j in part:
                delta[j] += (x - partial - replicas[j]) / (lrs[j] * taus[j])
        x = x - meta['scale'] * partial
        for j in range(C):
            if w[j] != 0.0:
                replicas[j] = x
    out = dict(server=x)
    if ftype == 'fedgate':
        out['delta'] = delta
    if ftype == 'scaffold':
        out['ctrl'], out['c'] = ctrl, c
    return out


def assert_federations_agree(a, b, recorded, label=''):
    """runs `a` and `b` (end states of run_federation) against the float64
    replay of `recorded`'s operands: the ReLU precondition, then each run's
    error and their distance within lc.bound of the fp32 replay's error"""
    p64, p32 = [], []
    r64 = replay_federation(recorded, F64, pre=p64)
    r32 = replay_federation(recorded, F32, pre=p32)
    lo, e = relu_margin(p64, p32)
    assert lo > mc.MARGIN * e, (lo, e)
    for k in STATE:
        if k not in r64:
            assert k not in a and k not in b
            continue
        e32 = lc.err(r32[k], r64[k])
        tol = lc.bound(e32, r64[k].abs().max().item())
        e_a, e_b = lc.err(a[k], r64[k]), lc.err(b[k], r64[k])
        d = (a[k] - b[k]).abs().max().item()
        print('%s %s: err %.3e / %.3e  distance %.3e  e32 %.3e  tol %.3e'
              % (label, k, e_a, e_b, d, e32, tol))
        assert e_a <= tol, (k, e_a, tol)
        assert e_b <= tol, (k, e_b, tol)
        assert d <= tol, (k, d, tol)
