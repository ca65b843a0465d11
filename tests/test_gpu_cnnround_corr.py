# -*- coding: utf-8 -*-
"""The gradient corrections of cnn_local_rounds (hip/cnnround.h: delta / the
control pair / prox_mu in the three backward kernels that update parameters)
on the GPU against the corrected float64 step loop of
tests/cnnround_corr_cases.py, with the machinery of test_gpu_cnnround.py.
Measured on an MI355X: see profiles/packed_cnn_notes.md."""
import pytest
import torch

import cnnround_cases as cc
import cnnround_corr_cases as kc
import fedtorch_amd.ops as ops
from test_gpu_cnnround import (NAN, _args, _assert_bounded, _cut,
                               _guards_intact, _same, run_cut)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('kind', kc.KINDS)
@pytest.mark.parametrize('geo', (cc.SMALL, cc.MID))
def test_against_float64_replay(geo, kind, monkeypatch):
    """The small geometry (plain conv weights, one tile everywhere) and the
    mid one (nhwc, several fc column tiles, two blocks of cnn_conv2_wrw_k per
    client, momentum, weight decay on a prefix).  Every operand is cut out of
    a NaN-filled buffer, the corrections with NaN in their pad gaps and in
    the offline client's rows: a stray read reaches an output.  Bound: 8x
    the fp32 CPU replay's own error plus 16 fp32 ulps of the output's scale
    (lc.bound), the project's bound for these kernels."""
    *args, corr, ref, e32 = kc.case(geo, kind)
    cut = {k: _cut(v, NAN) if torch.is_tensor(v) else (v, None)
           for k, v in corr.items()}
    real, kw = ops.cnn_local_rounds, {k: v for k, (v, _b) in cut.items()}
    monkeypatch.setattr(ops, 'cnn_local_rounds',
                        lambda *a, **k: real(*a, **k, **kw))
    got, off = run_cut(*args)
    for k, (v, buf) in cut.items():
        if buf is not None:
            assert _guards_intact(buf, NAN), k
            assert torch.equal(v.cpu().view(torch.int32),
                               corr[k].view(torch.int32)), k
    assert torch.equal(got['mom_init'].cpu(), ref['mom_init'])
    _assert_bounded(got, ref, e32, '%s %s' % (geo, kind), off=off)
    assert torch.isfinite(got['loss']).all()


def test_no_correction_is_the_correction_free_call():
    """all corrections None and prox_mu = 0: bit-identical to the call
    through the keyword set without them (the kernels that know none)"""
    args = cc.case(cc.MID)[:6]
    none = dict(delta=None, ctrl_server=None, ctrl_client=None, prox_mu=0.0)
    _same(cc.call_op(ops, *args, device='cuda'),
          cc.call_op(ops, *args, device='cuda',
                     op=kc.with_corr(ops.cnn_local_rounds, none)))


@pytest.mark.parametrize('change,match', [
    (lambda ctrl, delta: dict(ctrl, ctrl_client=None), 'come as a pair'),
    (lambda ctrl, delta: dict(ctrl, ctrl_server=None), 'come as a pair'),
    (lambda ctrl, delta: dict(ctrl, delta=delta),
     'delta and a control pair together'),
    (lambda ctrl, delta: dict(delta=delta[:, :-64].contiguous()),
     'delta must be contiguous'),
    (lambda ctrl, delta: dict(ctrl, ctrl_server=ctrl['ctrl_server'][:-1]
                              .contiguous()),
     'ctrl_server must be contiguous'),
    (lambda ctrl, delta: dict(prox_mu=-0.1),
     'prox_mu must be finite and >= 0'),
], ids=['no-client', 'no-server', 'delta+pair', 'delta-shape', 'ctrl-shape',
        'negative-mu'])
def test_correction_checks_raise_before_launch(change, match):
    *args, ctrl, _r, _e = kc.case(cc.MID, 'ctrl')
    ctrl = {k: v for k, v in ctrl.items() if torch.is_tensor(v)}
    corr = change(ctrl, kc.case(cc.MID, 'delta')[6]['delta'])
    pos, kw = _args(*args)
    with pytest.raises((RuntimeError, ValueError), match=match):
        kc.with_corr(ops.cnn_local_rounds, corr, 'cuda')(*pos, **kw)
    torch.cuda.synchronize()
    assert torch.isnan(pos[6]).all() and torch.isnan(pos[9]).all()
