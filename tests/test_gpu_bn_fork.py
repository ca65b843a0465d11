# -*- coding: utf-8 -*-
"""BN backward at a fork (hip/batchnorm.h bnh_fork_stats_k; launchers
bn_bwd_fork_stats + bn_bwd_part) against the path it replaces: the library's
`a + b` followed by the unchanged `bn_bwd`.

Bit for bit: g (also against that call's dres), dx, dweight, dbias.  bn_bwd
keeps its partial rows to itself, so the rows are checked three ways: their
count is the reduce grid's, they equal the rows the kernel writes when it is
handed the library's sum with b empty (the bn_bwd_stats_k arithmetic on the
same input), and dweight / dbias -- a deterministic function of the rows in
the unchanged dx kernel -- equal bn_bwd's.  Every operand is cut out of a
NaN-prefilled buffer, so a read outside an operand poisons a sum.

Against float64 (tests/bn_cases.py): integer inputs, power-of-two ivar and
weight, a + b exact in the element type (asserted): g, dweight, dbias and
the column sums of the rows are exact.

Module level: stem BNReLU + two BasicBlocks + one stride-2 BasicBlock with a
downsample; every gradient identical with FEDTORCH_BN_FORK's path on and
off, three fork launches, no elementwise add of two activation gradients."""
import zlib

import pytest
import torch
import torch.nn as nn

import fedtorch_amd.ops as ops

import bn_cases as bc

pytestmark = pytest.mark.gpu

DEV = 'cuda'
F64 = torch.float64
PAD = 64        # elements of NaN around every operand (keeps 16 B alignment)
RED_ITERS, RED_CAP = 8, 256          # bnh_red_grid


def _empty(dtype=torch.float32):
    return torch.empty(0, device=DEV, dtype=dtype)


def _cut(vals):
    """a copy of `vals` (same strides) that lives inside a NaN-filled
    buffer"""
    n = vals.numel()
    if vals.dtype == torch.uint8:
        buf = torch.full((n + 2 * PAD,), 255, dtype=torch.uint8, device=DEV)
    else:
        buf = torch.full((n + 2 * PAD,), float('nan'), dtype=vals.dtype,
                         device=DEV)
    out = buf[PAD:PAD + n].as_strided(vals.shape, vals.stride())
    out.copy_(vals)
    return out


def _nhwc(t4):
    """[N, C, H, W] values -> dense channels_last tensor"""
    N, C, H, W = t4.shape
    return t4.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def _grid(rows, C, dt):
    tasks = rows * (C // bc.VN[dt])
    return max(1, min(RED_CAP, -(-tasks // (bc.BLOCK * RED_ITERS)))), tasks


def _cap_rows(C, dt):
    """smallest row count at which the 256-block cap of the grid binds"""
    return bc.BLOCK * RED_ITERS * RED_CAP // (C // bc.VN[dt]) + 1


SHAPES = [(dt, C) for dt, cs in (('bf16', (8, 16, 64, 256)),
                                 ('fp32', (4, 16))) for C in cs]
VARIANTS = ('y', 'mask', 'norelu', 'b_empty')


def _kernel_cases():
    out = []
    for dt, C in SHAPES:
        for nhw in ((1, 1, 1), (3, 5, 7), (1, 1, _cap_rows(C, dt))):
            for v in VARIANTS:
                # the bitmask is bf16-only, and bn_bwd takes a 1x1 map (which
                # is also NCHW-contiguous) to its NCHW kernels, without one
                if v == 'mask' and (dt != 'bf16' or nhw == (1, 1, 1)):
                    continue
                out.append((dt, C) + nhw + (v,))
    return out


def _random_inputs(dt, C, N, H, W, variant):
    g = torch.Generator(device=DEV).manual_seed(
        zlib.crc32(repr((dt, C, N, H, W)).encode()))
    dtype = bc.DTYPES[dt]

    def act():
        return _cut(_nhwc(torch.randn(N, C, H, W, device=DEV, generator=g)
                          .to(dtype)))
    i = {'a': act(), 'b': act(), 'x': act(), 'y': act()}
    i['mean'] = _cut(torch.randn(C, device=DEV, generator=g))
    i['ivar'] = _cut(torch.rand(C, device=DEV, generator=g) + 0.5)
    i['w'] = _cut(torch.randn(C, device=DEV, generator=g))
    return _variant(i, variant)


def _variant(i, variant):
    i = dict(i)
    i['relu'] = variant != 'norelu'
    i['mask'] = _empty(torch.uint8)
    if variant == 'mask':
        i['mask'] = _cut(bc.pack_mask(i['y'].cpu().float()).to(DEV))
        i['y'] = _empty()
    elif variant == 'norelu':
        i['y'] = _empty()
    elif variant == 'b_empty':
        i['b'] = _empty()
    return i


def _fork(i):
    g, part = ops._C.bn_bwd_fork_stats(
        i['a'], i['b'], i['x'], i['y'], i['mask'], i['mean'], i['ivar'],
        i['relu'])
    dx, dw, db = ops._C.bn_bwd_part(g, i['x'], part, i['mean'], i['ivar'],
                                    i['w'])
    return g, part, dx, dw, db


def _parent(i):
    """(sum, dx, dweight, dbias, dres) of the path before the fork kernel"""
    s = i['a'] + i['b'] if i['b'].numel() else i['a']
    dx, dw, db, dres = ops._C.bn_bwd(
        s.contiguous() if s.shape[2] * s.shape[3] == 1 else s, i['x'],
        i['y'], i['mask'], i['mean'], i['ivar'], i['w'], i['relu'], True)
    return s, dx, dw, db, dres


def _eq(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if not torch.equal(got, want):
        bad = ((got != want) | (got != got)).nonzero()
        k = tuple(bad[0].tolist())
        raise AssertionError('%s: %d differ, first at %s: %r vs %r' % (
            what, bad.shape[0], k, got[k].item(), want[k].item()))


@pytest.mark.parametrize('case', _kernel_cases(),
                         ids=lambda c: '%s-C%d-%dx%dx%d-%s' % c)
def test_fork_matches_add_then_bn_bwd(case):
    dt, C, N, H, W, variant = case
    i = _random_inputs(*case)
    g, part, dx, dw, db = _fork(i)
    s, pdx, pdw, pdb, pdres = _parent(i)
    B, tasks = _grid(N * H * W, C, dt)
    if W > 1000:
        assert B == RED_CAP and tasks > bc.BLOCK * RED_ITERS * RED_CAP
    assert tuple(part.shape) == (B, C, 2)
    for t in (g, part, dx, dw, db):
        assert torch.isfinite(t).all().item()
    _eq(g, pdres, 'g vs dres')
    _eq(dx, pdx, 'dx')
    _eq(dw, pdw, 'dweight')
    _eq(db, pdb, 'dbias')
    assert g.is_contiguous(memory_format=torch.channels_last)
    j = dict(i, a=s, b=_empty())
    g2, part2 = ops._C.bn_bwd_fork_stats(
        j['a'], j['b'], j['x'], j['y'], j['mask'], j['mean'], j['ivar'],
        j['relu'])
    _eq(g2, g, 'g from the library sum')
    _eq(part2, part, 'partial rows from the library sum')


F64_CASES = [('cl', 'bf16', 16, 4, 16, 16), ('cl', 'bf16', 64, 3, 5, 7),
             ('cl', 'bf16', 256, 3, 5, 7), ('cl', 'bf16', 8, 4, 16, 16),
             ('cl', 'fp32', 4, 3, 5, 7), ('cl', 'fp32', 16, 4, 16, 16)]


@pytest.mark.parametrize(
    'case,variant',
    [(c, v) for c in F64_CASES for v in ('y', 'mask', 'norelu')
     if v != 'mask' or c[1] == 'bf16'],
    ids=lambda p: bc.case_id(p) if isinstance(p, tuple) else p)
def test_fork_against_float64(case, variant):
    _l, dt, C, N, H, W = case
    relu = variant != 'norelu'
    i64, r, _exact = bc.bwd_case(case, relu)
    dtype = bc.DTYPES[dt]
    k = bc.ints(bc.gen('fork', case), -3, 3, N, C, H, W)
    a64, b64 = i64['dy'] - k, k
    # the precondition of the comparison: operands and their sum are numbers
    # of the element type, so the kernel's one rounding changes nothing
    for t in (a64, b64, a64 + b64, i64['x'], i64['y']):
        assert torch.equal(t.to(dtype).double(), t)
    assert torch.equal(a64 + b64, i64['dy'])

    def act(t):
        return _cut(_nhwc(t.to(dtype).to(DEV)))
    i = _variant({'a': act(a64), 'b': act(b64), 'x': act(i64['x']),
                  'y': act(i64['y']),
                  'mean': _cut(i64['mean'].float().to(DEV)),
                  'ivar': _cut(i64['ivar'].float().to(DEV)),
                  'w': _cut(i64['w'].float().to(DEV))}, variant)
    g, part, _dx, dw, db = _fork(i)
    _eq(g.cpu().double(), r['g'], 'g')
    _eq(dw.cpu().double(), r['dweight'], 'dweight')
    _eq(db.cpu().double(), r['dbias'], 'dbias')
    cols = part.cpu().double().sum(0)
    _eq(cols[:, 0].contiguous(), r['dbias'], 'rows sum(g)')
    _eq(cols[:, 1].contiguous(), r['dweight'], 'rows sum(g*xhat)')


def test_fork_deterministic():
    i = _random_inputs('bf16', 64, 3, 5, 7, 'y')
    for u, v in zip(_fork(i), _fork(i)):
        assert torch.equal(u, v)
    i = _random_inputs('bf16', 16, 1, 1, _cap_rows(16, 'bf16'), 'mask')
    for u, v in zip(_fork(i), _fork(i)):
        assert torch.equal(u, v)


def test_fork_launchers_reject():
    i = _random_inputs('bf16', 16, 2, 4, 4, 'y')
    g, part, _dx, _dw, _db = _fork(i)

    def stats(**kw):
        j = dict(i, **kw)
        return ops._C.bn_bwd_fork_stats(
            j['a'], j['b'], j['x'], j['y'], j['mask'], j['mean'], j['ivar'],
            j['relu'])

    def dxp(**kw):
        j = dict(i, g=g, part=part)
        j.update(kw)
        return ops._C.bn_bwd_part(j['g'], j['x'], j['part'], j['mean'],
                                  j['ivar'], j['w'])
    nchw = i['x'].contiguous()
    nmask = i['x'].numel() // 8
    f32 = _nhwc(i['a'].float())
    bad = [
        lambda: stats(x=nchw),                          # layout of x
        lambda: stats(a=i['a'].contiguous()),           # layout of a
        lambda: stats(b=i['b'].contiguous()),           # layout of b
        lambda: stats(a=f32),                           # dtype mix
        lambda: stats(b=f32),
        lambda: stats(b=i['b'][:1]),                    # shape of b
        lambda: stats(y=_empty()),                      # relu without y/mask
        lambda: stats(mask=torch.zeros(nmask + 1, dtype=torch.uint8,
                                       device=DEV)),
        lambda: stats(mask=torch.zeros(nmask - 1, dtype=torch.uint8,
                                       device=DEV)),
        lambda: stats(mean=i['mean'][:8]),
        lambda: stats(ivar=i['ivar'].double()),
        lambda: dxp(x=nchw),
        lambda: dxp(g=f32),
        lambda: dxp(g=g.contiguous()),
        lambda: dxp(part=part[:0]),                     # 0 rows
        lambda: dxp(part=torch.zeros(257, 16, 2, device=DEV)),
        lambda: dxp(part=torch.zeros(1, 8, 2, device=DEV)),
        lambda: dxp(part=part.double()),
        lambda: dxp(w=i['w'][:8]),
    ]
    for k, fn in enumerate(bad):
        with pytest.raises(RuntimeError):
            fn()
            pytest.fail('call %d was accepted' % k)
    # fp32 x with a mask (the bitmask indexes 8 channels per byte)
    j = _random_inputs('fp32', 16, 2, 4, 4, 'y')
    with pytest.raises(RuntimeError):
        ops._C.bn_bwd_fork_stats(
            j['a'], j['b'], j['x'], _empty(),
            torch.zeros(nmask, dtype=torch.uint8, device=DEV),
            j['mean'], j['ivar'], True)
    torch.cuda.synchronize()


def test_fork_graph_capture_three_replays():
    i = _random_inputs('bf16', 32, 3, 5, 7, 'mask')
    fresh = [_random_inputs('bf16', 32, 3, 5, 7 + k, 'y') for k in (0, 1, 2)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _fork(i)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = _fork(i)
    for k in range(3):
        # new gradients in the captured operands before every replay
        i['a'].copy_(fresh[k]['b'][:, :, :, :7])
        i['b'].copy_(fresh[k]['x'][:, :, :, :7])
        graph.replay()
        torch.cuda.synchronize()
        for u, v in zip(outs, _fork(i)):
            assert torch.equal(u, v), 'replay %d' % k


# --------------------------------------------------------------------------
# module level
# --------------------------------------------------------------------------
class _Net(nn.Module):
    def __init__(self):
        super().__init__()
        from fedtorch_amd.components.models.resnet import BasicBlock
        from fedtorch_amd.ops.batchnorm import BNReLU
        from fedtorch_amd.ops.conv3x3 import NhwcConv1x1S2
        self.bn = BNReLU(32)
        self.b1 = BasicBlock(32, 32)
        self.b2 = BasicBlock(32, 32)
        self.b3 = BasicBlock(32, 64, 2, nn.Sequential(
            NhwcConv1x1S2(32, 64, kernel_size=1, stride=2, bias=False),
            nn.BatchNorm2d(64)))

    def forward(self, x):
        return self.b3(self.b2(self.b1(self.bn(x))))


def _module_step(fork, monkeypatch):
    with monkeypatch.context() as mp:
        return _module_step_patched(fork, mp)


def _module_step_patched(fork, monkeypatch):
    from fedtorch_amd.ops import batchnorm as bnm
    monkeypatch.setattr(bnm, '_FORK_ENABLED', fork)
    # the library convolutions that remain (stride-2 backward, 1x1
    # downsample) on their deterministic solvers: a weight gradient summed
    # with atomics differs from itself from run to run
    monkeypatch.setattr(torch.backends.cudnn, 'deterministic', True)
    calls = {'stats': 0, 'part': 0}
    real_stats, real_part = ops._C.bn_bwd_fork_stats, ops._C.bn_bwd_part

    def stats(*a):
        calls['stats'] += 1
        return real_stats(*a)

    def part(*a):
        calls['part'] += 1
        return real_part(*a)
    monkeypatch.setattr(ops._C, 'bn_bwd_fork_stats', stats)
    monkeypatch.setattr(ops._C, 'bn_bwd_part', part)
    torch.manual_seed(7)
    m = _Net()
    for mod in m.modules():
        if isinstance(mod, nn.BatchNorm2d):
            nn.init.normal_(mod.weight, 1.0, 0.2)
            nn.init.normal_(mod.bias, 0.0, 0.2)
    m = bnm.convert_to_fused_bn(m).cuda().to(memory_format=torch.channels_last)
    for p in m.parameters():
        if p.dim() == 4:
            p.data = p.data.bfloat16()
    m.train()
    x = torch.randn(2, 32, 16, 16, device=DEV).bfloat16().to(
        memory_format=torch.channels_last).requires_grad_(True)
    with torch.autocast('cuda', dtype=torch.bfloat16):
        out = m(x)
        loss = out.float().square().mean()
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU], record_shapes=True) as pr:
        loss.backward()
        torch.cuda.synchronize()
    adds = [e for e in pr.events()
            if e.name in ('aten::add', 'aten::add_')
            and e.input_shapes and len(e.input_shapes[0]) == 4]
    assert not bnm._FORK_TAGS, 'side table not drained'
    grads = [x.grad.clone()] + [p.grad.clone() for p in m.parameters()]
    return grads, calls, len(adds)


def test_fork_module_gradients_identical(monkeypatch):
    on, calls_on, adds_on = _module_step(True, monkeypatch)
    off, calls_off, adds_off = _module_step(False, monkeypatch)
    again, _c, _a = _module_step(False, monkeypatch)
    for k, (u, v) in enumerate(zip(off, again)):
        _eq(u, v, 'baseline not reproducible: gradient %d, fork off twice' % k)
    print('fork on: %r, %d activation adds; off: %r, %d' % (
        calls_on, adds_on, calls_off, adds_off))
    assert calls_on == {'stats': 3, 'part': 3}
    assert calls_off == {'stats': 0, 'part': 0}
    # the engine adds the two gradients of each of the three forks itself
    # when the path is off, and never when it is on
    assert adds_off == 3 and adds_on == 0
    assert len(on) == len(off)
    for k, (u, v) in enumerate(zip(on, off)):
        assert torch.isfinite(u).all().item()
        _eq(u, v, 'gradient %d' % k)
