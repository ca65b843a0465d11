# -*- coding: utf-8 -*-
"""CPU checks of tests/bn_cases.py, the reference and case generators of
tests/test_gpu_batchnorm.py: every case the GPU file parametrizes is built
here (the builders assert their preconditions: exact-sum limits,
representability, both signs present, zero-crossing margins), the
hand-written float64 BatchNorm is compared with torch's own under autograd,
and the bitmask packer with numpy's.  No GPU, no extension."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_cases as bc

F64 = torch.float64


def test_shape_grid_covers_the_kernel_paths():
    cl = [c for c in bc.CL_SHAPES]
    for dt in ('bf16', 'fp32'):
        cs = sorted({c[2] for c in cl if c[1] == dt})
        assert cs == [bc.VN[dt], 16, 32, 64, 256]
        for C in cs:
            rows = {bc.rows_of(c) for c in cl if c[1] == dt and c[2] == C}
            rp = bc.rows_per_pass(C, dt)
            assert {1, 3, rp - 1, rp + 1, 1024} <= rows
    # group counts 1 .. 64 (no butterfly at 64)
    assert {c[2] // bc.VN[c[1]] for c in cl} >= {1, 2, 4, 8, 16, 32, 64}
    # NCHW: vector and scalar path for both types; HW = 4 splits them
    hw = {(c[1], c[4] * c[5]) for c in bc.NCHW_SHAPES}
    for dt in ('bf16', 'fp32'):
        assert {(dt, 64), (dt, 49), (dt, 4), (dt, 1)} <= hw
    # the large cases: both grid caps bind and the last pass is ragged
    _l, dt, C, N, H, W = bc.CL_LARGE
    tasks = N * H * W * (C // bc.VN[dt])
    assert tasks > 256 * bc.BLOCK * 8 and tasks > 1024 * bc.BLOCK * 2
    assert tasks % (256 * bc.BLOCK) and tasks % (1024 * bc.BLOCK)
    assert N * H * W * C * 2 <= 8.6e6                    # bytes
    _l, dt, C, N, H, W = bc.NCHW_LARGE
    per_v = N * H * W // bc.VN[dt]
    work = -(-per_v // bc.BLOCK)
    assert work > 512 // C and work > 1024 // C
    assert per_v % ((512 // C) * bc.BLOCK) and per_v % ((1024 // C) * bc.BLOCK)
    # defer: both sides of the 64-block collapse, C = 256 on the far side
    blocks = {c: bc.defer_blocks(c) for c in bc.DEFER_CASES}
    assert min(blocks.values()) <= 64 < max(blocks.values())
    assert any(c[2] == 256 and b > 64 for c, b in blocks.items())
    # part: both sides of the 64-row switch, C up to 256
    assert {64, 65} <= set(bc.PART_B) and 256 in bc.PART_C


@pytest.mark.parametrize('case', bc.SHAPES + bc.LARGE, ids=bc.case_id)
def test_bwd_cases_meet_their_preconditions(case):
    flags = bc.BWD_FLAGS if case not in bc.LARGE else [(True, True)]
    for relu in sorted({f[0] for f in flags}):
        i, r, exact = bc.bwd_case(case, relu, True)
        assert exact == bc.is_pow2(bc.rows_of(case))
        assert torch.isfinite(r['dx']).all().item()
        b = bc.dx_bound(r, case[1])
        # a wrong kernel is off by O(1); the bound is far below that
        assert b.max().item() < 0.51 * bc.bf16_ulp(
            r['dx'].abs().max() + 1).item() + 1e-4
        if relu:
            # the mask changes the result: the test can tell it is applied
            _i, r0, _e = bc.bwd_case(case, False, True)
            assert not torch.equal(r['dx'], r0['dx'])
            assert not torch.equal(r['dbias'], r0['dbias'])


@pytest.mark.parametrize('case', bc.FWD_SHAPES + bc.LARGE, ids=bc.case_id)
def test_fwd_cases_meet_their_preconditions(case):
    flags = bc.FWD_FLAGS if case not in bc.LARGE else [(True,) * 4]
    for f in flags:
        i, r, E = bc.fwd_case(case, f)
        assert torch.isfinite(r['y']).all().item()
        assert E.max().item() < 1e-3
        assert (i['res'] is not None) == f[1]
        assert (i['w'] is not None) == f[2] and (i['rm0'] is not None) == f[3]
    for dt in ('bf16', 'fp32'):
        bc.fwd_one_row_case(dt)


@pytest.mark.parametrize('dt,C,B', bc.PART_CASES,
                         ids=['%s-C%d-B%d' % p for p in bc.PART_CASES])
def test_part_cases_meet_their_preconditions(dt, C, B):
    i, r, E, part = bc.part_case(dt, C, B)
    assert part.shape == (B, C, 2)
    assert bc.fp32_exact(part) and part.abs().max().item() < bc.EXACT
    assert torch.equal(part, part.round())               # integers


def test_part_flags_cover_the_collapse_cases():
    """with and without res, relu, affine and running statistics at every C
    on the far side of the 64-row switch"""
    for C in bc.PART_C:
        flags = [bc.part_flags(dt, C, B) for dt in ('bf16', 'fp32')
                 for B in (65, 100, 1000)]
        for k in range(4):
            assert {f[k] for f in flags} == {True, False}, (C, k)


@pytest.mark.parametrize('case', bc.DEFER_CASES, ids=bc.case_id)
def test_defer_cases_meet_their_preconditions(case):
    for relu in (False, True):
        i, r, coefs, bound, exact = bc.defer_case(case, relu)
        # the affine form reproduces dx: A*g + B + D*x
        dx = bc.vc(coefs[0]) * r['g'] + bc.vc(coefs[1]) + \
            bc.vc(coefs[2]) * i['x']
        assert torch.allclose(dx, r['dx'], rtol=0, atol=1e-11)
        assert bound.max().item() < 1e-4


# --------------------------------------------------------------------------
# the hand-written reference against torch's float64 BatchNorm + autograd
# --------------------------------------------------------------------------
AUTOGRAD_CASES = [('cl', 'fp32', 16, 4, 16, 16), ('cl', 'bf16', 8, 1, 1, 257),
                  ('nchw', 'fp32', 5, 3, 7, 7), ('nchw', 'bf16', 3, 5, 2, 2)]


@pytest.mark.parametrize('flags', bc.FWD_FLAGS,
                         ids=['relu%d-res%d-aff%d-trk%d' % f
                              for f in bc.FWD_FLAGS])
@pytest.mark.parametrize('case', AUTOGRAD_CASES, ids=bc.case_id)
def test_reference_matches_torch_autograd(case, flags):
    relu, has_res, affine, track = flags
    i, r, _E = bc.fwd_case(case, flags)
    C = case[2]
    x = i['x'].clone().requires_grad_(True)
    w = i['w'].clone().requires_grad_(True) if affine else None
    b = i['b'].clone().requires_grad_(True) if affine else None
    res = i['res'].clone().requires_grad_(True) if has_res else None
    rm = i['rm0'].clone() if track else None
    rv = i['rv0'].clone() if track else None
    out = F.batch_norm(x, rm, rv, w, b, True, i['mom'], i['eps'])
    if has_res:
        out = out + res
    if relu:
        out = torch.relu(out)
    dy = bc.ints(bc.gen('autograd', case, flags), -4, 4, *x.shape)
    out.backward(dy)

    def close(got, want, name):
        err = (got - want).abs().max().item()
        assert err <= 1e-12 * max(1.0, want.abs().max().item()), \
            '%s err %.3g' % (name, err)

    close(r['y'], out.detach(), 'y')
    if track:
        close(r['rm'], rm, 'running_mean')
        close(r['rv'], rv, 'running_var')
    rb = bc.ref_bwd(i['x'], dy, r['y'], r['mean'], r['ivar'], i['w'], relu)
    close(rb['dx'], x.grad, 'dx')
    if has_res:
        close(rb['dres'], res.grad, 'dres')
    if affine:
        close(rb['dweight'], w.grad, 'dgamma')
        close(rb['dbias'], b.grad, 'dbeta')
    assert rb['dbias'].shape == (C,)


def test_reference_one_row_matches_torch():
    """n = 1: torch refuses to train on one value per channel, so compare
    with the formulas' limit: y = relu(beta + res), mean = x, var = 0"""
    i, r, _E = bc.fwd_one_row_case('fp32')
    want = (bc.vc(i['b']) + i['res']).clamp_min(0)
    assert torch.allclose(r['y'], want, rtol=0, atol=1e-12)
    assert torch.equal(r['rm'], 0.75 * i['rm0'] + 0.25 * i['x'].view(-1))


# --------------------------------------------------------------------------
# the mask packer
# --------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(1, 8, 1, 1), (2, 16, 3, 5),
                                   (3, 64, 5, 7), (1, 256, 1, 3)])
def test_pack_mask_matches_numpy_packbits(shape):
    g = bc.gen('mask', shape)
    y = bc.ints(g, -2, 2, *shape)
    got = bc.pack_mask(y)
    flat = (y.permute(0, 2, 3, 1).reshape(-1) > 0).numpy()
    want = np.packbits(flat, bitorder='little')
    assert got.dtype == torch.uint8 and got.numel() * 8 == y.numel()
    assert np.array_equal(got.numpy(), want)
    # bit (e & 7) of byte (e >> 3), spelled out
    for e in (0, 7, y.numel() // 2 + 3, y.numel() - 1):
        assert ((int(got[e >> 3]) >> (e & 7)) & 1) == int(flat[e])
