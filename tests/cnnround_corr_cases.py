# -*- coding: utf-8 -*-
"""The gradient-correction term of ops.cnn_local_rounds (delta / the control
pair / prox_mu) on the committed cases of cnnround_cases: its step loop with
fused_sgd_step's corrections put in front of the SGD update."""
import contextlib
import functools

import torch

import linround_cases as lc
import cnnround_cases as cc

KINDS = ('delta', 'ctrl', 'prox')
ROWS = ('delta', 'ctrl_server', 'ctrl_client')
MU = 1.0
# the scale of the correction rows.  1e-2 (about 1e-2 of the gradients')
# moves a conv1 decision of the mid case with a control pair to 47x the fp32
# replay's error, inside the 64x margin that `case()` asserts; the correction
# is scaled down for all cases instead of searching seeds.
SCALE = 2e-3


@contextlib.contextmanager
def corrected(corr, steps, server, dtype):
    """while active, cc.ref_rounds updates with d = g ; d -= delta[c] ;
    d += c - c_j[c] ; d += mu (p - x), the order of ops.fused_sgd_step.  It
    calls cc._sgd eight times per step, client by client, and forms all
    gradients of a step before the first call, so p[lo:hi] is pre-update."""
    real, x = cc._sgd, server.to(dtype)
    who = iter([c for c, n in enumerate(steps.tolist()) for _ in range(8 * n)])
    dl, cs, cj = (None if corr.get(k) is None else corr[k].to(dtype)
                  for k in ROWS)

    def sgd(p, buf, lo, hi, g, *rest):
        c, d = next(who), g.reshape(-1)
        if dl is not None:
            d = d - dl[c, lo:hi]
        if cs is not None:
            d = d + (cs[lo:hi] - cj[c, lo:hi])
        if corr.get('prox_mu', 0.0) != 0:
            d = d + corr['prox_mu'] * (p[lo:hi] - x[lo:hi])
        real(p, buf, lo, hi, d, *rest)
    cc._sgd = sgd
    try:
        yield
    finally:
        cc._sgd = real


def make_corr(case, kind):
    """the operands of `kind` from a fixed generator, NaN in the pad gaps and
    in the rows of offline clients: where no kernel may read"""
    g = lc.gen('cnn-corr', kind)
    C = case['idx'].shape[0]
    corr = dict(delta=None, ctrl_server=None, ctrl_client=None,
                prox_mu=MU if kind == 'prox' else 0.0)
    shapes = dict(delta=dict(delta=(C,)),
                  ctrl=dict(ctrl_server=(), ctrl_client=(C,)), prox={})[kind]
    for k, shp in shapes.items():
        t = torch.randn(shp + (case['N'],), generator=g) * SCALE
        t[..., cc.gap_mask(case['layout'], case['N'])] = cc.NAN
        if shp:
            t[case['steps'] <= 0] = cc.NAN
        corr[k] = t
    return corr


@functools.lru_cache(maxsize=None)
def case(geo, kind):
    """cc.case(geo)[:6] + (corr, ref64, e32), computed once and shared: treat
    it as read-only.  Asserts the decision precondition of cc.case, unchanged,
    for the corrected run."""
    args = cc.case(geo)[:6]
    corr = make_corr(args[0], kind)
    refs, pre = {}, {}
    for dt in (cc.F64, cc.F32):
        pre[dt] = []
        with corrected(corr, args[0]['steps'], args[0]['server'], dt):
            refs[dt] = cc.run_ref(*args, dtype=dt, pre=pre[dt])
    for what, (lo, e) in cc.margins(pre[cc.F64], pre[cc.F32]).items():
        assert lo > cc.MARGIN * e, (what, geo, kind, lo, e)
    ref = refs[cc.F64]
    e32 = {k: lc.err(refs[cc.F32][k], ref[k]) for k in cc.OUTPUTS
           if ref[k] is not None}
    return args + (corr, ref, e32)


def with_corr(op, corr, device='cpu'):
    """`op` with the correction operands as keywords"""
    kw = {k: v.clone().to(device) if torch.is_tensor(v) else v
          for k, v in corr.items()}
    return lambda *a, **k: op(*a, **k, **kw)
