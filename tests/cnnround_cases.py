# -*- coding: utf-8 -*-
"""Reference and case generator for ops.cnn_local_rounds (hip/cnnround.h):
a plain per-client step loop with a hand-written backward in any dtype
(float64 is the reference, float32 measures the format's own error) for
either order of the conv weights in the arena, and random-valued cases whose
ReLU and max-pool decisions stay clear of a tie.  Shared by
test_cnnround_cpu.py and test_gpu_cnnround.py."""
import functools

import torch
import torch.nn.functional as Fn

import linround_cases as lc

F64 = torch.float64
F32 = torch.float32
NAN = float('nan')
OUTPUTS = ('replicas', 'in_mom', 'snap', 'loss')
KINDS = ('conv1', 'conv2', 'fc1')


# --------------------------------------------------------------------------
# layout
# --------------------------------------------------------------------------
def dims(layout):
    """(Cin, S, C1, C2, H, K, S1, S2, F2)"""
    Cin, S = layout['image']
    C1, C2 = layout['conv1'][2], layout['conv2'][2]
    H, K = layout['fc1'][2], layout['fc2'][2]
    S1 = (S - 4) // 2
    S2 = (S1 - 4) // 2
    return Cin, S, C1, C2, H, K, S1, S2, C2 * S2 * S2


def make_layout(Cin, S, C1, C2, H, K, nhwc=(0, 0)):
    """an arena-like layout in named_parameters order with pad gaps (64
    aligned, a leading gap as well): (layout, N)"""
    al = lambda n: (n + 63) // 64 * 64  # noqa: E731
    S2 = ((S - 4) // 2 - 4) // 2
    sizes = [C1 * Cin * 25, C1, C2 * C1 * 25, C2, H * C2 * S2 * S2, H, K * H,
             K]
    offs, off = [], 64
    for n in sizes:
        offs.append(off)
        off += al(n)
    return dict(image=(Cin, S), conv1=(offs[0], offs[1], C1, nhwc[0]),
                conv2=(offs[2], offs[3], C2, nhwc[1]),
                fc1=(offs[4], offs[5], H), fc2=(offs[6], offs[7], K)), off


def tensors(layout):
    """[(start, end, shape, nhwc, fan_in)] of the eight parameter tensors:
    conv1 w, b, conv2 w, b, fc1 w, b, fc2 w, b; fan_in 0 for a bias"""
    Cin, _S, C1, C2, H, K, _S1, _S2, F2 = dims(layout)
    w1, b1, _c, n1 = layout['conv1']
    w2, b2, _c, n2 = layout['conv2']
    fw1, fb1, _h = layout['fc1']
    fw2, fb2, _k = layout['fc2']
    shp = [(w1, (C1, Cin, 5, 5), n1, 25 * Cin), (b1, (C1,), 0, 0),
           (w2, (C2, C1, 5, 5), n2, 25 * C1), (b2, (C2,), 0, 0),
           (fw1, (H, F2), 0, F2), (fb1, (H,), 0, 0),
           (fw2, (K, H), 0, H), (fb2, (K,), 0, 0)]
    out = []
    for lo, s, nhwc, fan in shp:
        n = 1
        for v in s:
            n *= v
        out.append((lo, lo + n, s, nhwc, fan))
    return out


def gap_mask(layout, N):
    gap = torch.ones(N, dtype=torch.bool)
    for lo, hi, _s, _n, _f in tensors(layout):
        gap[lo:hi] = False
    return gap


def get(p, t):
    """the tensor t of tensors() out of the arena row p, in its module shape
    ([co][ci][kh][kw] whatever the arena's order)"""
    lo, hi, shp, nhwc, _f = t
    if nhwc:
        co, ci, kh, kw = shp
        return p[lo:hi].view(co, kh, kw, ci).permute(0, 3, 1, 2)
    return p[lo:hi].view(shp)


def flat_of(g, t):
    """a module-shaped gradient in the arena's element order"""
    return (g.permute(0, 2, 3, 1) if t[3] else g).reshape(-1)


def reorder_index(layout, nhwc):
    """(layout with the conv order flags `nhwc`, index): row[index] is an
    arena row of `layout` in the element order of the new layout"""
    new = dict(layout, conv1=layout['conv1'][:3] + (nhwc[0],),
               conv2=layout['conv2'][:3] + (nhwc[1],))
    N = max(t[1] for t in tensors(layout))
    N = (N + 63) // 64 * 64
    ar = torch.arange(N)
    index = ar.clone()
    for t_old, t_new in zip(tensors(layout), tensors(new)):
        if len(t_old[2]) == 4:
            index[t_new[0]:t_new[1]] = flat_of(get(ar, t_old).contiguous(),
                                               t_new)
    return new, index


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


def windows(z):
    """[n, C, 2h, 2w] -> [n, C, h, w, 4]: the 2x2 windows in scan order"""
    n, C, hh, ww = z.shape
    return z.view(n, C, hh // 2, 2, ww // 2, 2).permute(0, 1, 2, 4, 3, 5) \
        .reshape(n, C, hh // 2, ww // 2, 4)


def unwindows(zw):
    n, C, h, w, _four = zw.shape
    return zw.view(n, C, h, w, 2, 2).permute(0, 1, 2, 4, 3, 5) \
        .reshape(n, C, 2 * h, 2 * w)


def relu_pool(z):
    """max-pool 2/2 of relu(z): (pooled, position of the FIRST maximum of the
    window in scan order, whether it is > 0)"""
    zw = windows(z)
    m, k = zw[..., 0], torch.zeros(zw.shape[:-1], dtype=torch.long)
    for q in (1, 2, 3):
        up = zw[..., q] > m
        m = torch.where(up, zw[..., q], m)
        k = torch.where(up, torch.full_like(k, q), k)
    on = m > 0
    return torch.where(on, m, torch.zeros_like(m)), k, on


def relu_pool_bwd(dp, k, on):
    """the gradient of relu_pool: to the first maximum, where it is > 0"""
    dzw = torch.zeros(dp.shape + (4,), dtype=dp.dtype)
    dzw.scatter_(-1, k.unsqueeze(-1), (dp * on.to(dp.dtype)).unsqueeze(-1))
    return unwindows(dzw)


def conv_fwd(x, W, b):
    n, _ci, hh, _ww = x.shape
    co = W.shape[0]
    cols = Fn.unfold(x, 5)                              # [n, ci 25, L]
    z = W.reshape(co, -1) @ cols + b[None, :, None]
    return z.view(n, co, hh - 4, hh - 4), cols


def conv_bwd(dz, cols, W, side):
    """(dW, db, dx); side: of the input"""
    n, co = dz.shape[:2]
    d = dz.reshape(n, co, -1)
    dW = (d @ cols.transpose(1, 2)).sum(0).view(W.shape)
    dx = Fn.fold(W.reshape(co, -1).t() @ d, (side, side), 5)
    return dW, d.sum((0, 2)), dx


def ref_rounds(X, Y, idx, steps, lr, server, replicas, in_mom, mom_init,
               snap, k_cut, layout, wd_numel, wd, m, damp, nesterov,
               dtype=F64, pre=None):
    """cnn_local_rounds as a plain loop in `dtype`.  Nothing is modified;
    returns dict(replicas, in_mom, mom_init, snap, loss) where untouched rows
    are copies of the inputs.  `pre`: a list that receives, per (client,
    step) in execution order, dict(conv1=z1, conv2=z2, fc1=y): the conv
    outputs and fc1's pre-activation of the valid rows."""
    C, T, _B = idx.shape
    out = dict(replicas=replicas.to(dtype).clone(),
               in_mom=None if in_mom is None else in_mom.to(dtype).clone(),
               mom_init=mom_init.clone(),
               snap=None if snap is None else snap.to(dtype).clone(),
               loss=torch.zeros((C, T), dtype=dtype))
    Xd = X.to(dtype)
    Cin, S, _C1, _C2, _H, _K, S1, _S2, F2 = dims(layout)
    ts = tensors(layout)
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
            W1, b1, W2, b2, Wf1, bf1, Wf2, bf2 = [get(p, t) for t in ts]
            x = Xd[rows].view(n, Cin, S, S)
            z1, cols1 = conv_fwd(x, W1, b1)
            p1, k1, on1 = relu_pool(z1)
            z2, cols2 = conv_fwd(p1, W2, b2)
            p2, k2, on2 = relu_pool(z2)
            f = p2.reshape(n, F2)
            y = f @ Wf1.t() + bf1
            if pre is not None:
                pre.append(dict(conv1=z1.clone(), conv2=z2.clone(),
                                fc1=y.clone()))
            a = y.clamp(min=0)
            z = a @ Wf2.t() + bf2
            lse = torch.logsumexp(z, 1)
            ar = torch.arange(n)
            out['loss'][c, s] = (lse - z[ar, y_ids]).sum() / n
            dl = torch.softmax(z, 1)
            dl[ar, y_ids] -= 1
            dl = dl / n
            dy = (dl @ Wf2) * (y > 0).to(dtype)
            dp2 = (dy @ Wf1).view(p2.shape)
            dW2, db2, dp1 = conv_bwd(relu_pool_bwd(dp2, k2, on2), cols2, W2,
                                     S1)
            dW1, db1, _dx = conv_bwd(relu_pool_bwd(dp1, k1, on1), cols1, W1,
                                     S)
            grads = [dW1, db1, dW2, db2, dy.t() @ f, dy.sum(0), dl.t() @ a,
                     dl.sum(0)]
            first = m != 0 and not had
            for t, gr in zip(ts, grads):
                gr = flat_of(gr, t) if gr.dim() == 4 else gr
                _sgd(p, buf, t[0], t[1], gr, first, float(lr[c, s]), wd,
                     wd_numel, m, damp, nesterov)
            had = True
        out['replicas'][c].copy_(p)
        if m != 0:
            out['mom_init'][c] = 1
    return out


# --------------------------------------------------------------------------
# cases
# --------------------------------------------------------------------------
# (Cin, S, C1, C2, H, K): B, the step counts, hyper-parameters, the short
# batch (client, step, n), the one-row step (client, step), k_cut, the order
# of the conv weights, whether weight decay covers a prefix only, and the
# seed.  Every seed is checked by `case()` (the precondition below); they
# were searched on the CPU.
SMALL = (1, 16, 3, 5, 7, 2)
MID = (3, 20, 5, 18, 33, 10)
STOCK = (1, 28, 20, 50, 512, 10)
CASES = {
    SMALL: dict(
        B=5, steps=[3, 0, 2],
        hp=dict(wd=0.0, m=0.0, damp=0.0, nesterov=False), short=(0, 2, 3),
        one=(2, 1), k_cut=3, nhwc=(0, 0), wd_part=False, mom_init=[0, 0, 0],
        seed=0),
    MID: dict(
        B=5, steps=[3, 0, 2],
        hp=dict(wd=5e-4, m=0.9, damp=0.0, nesterov=True), short=(0, 2, 3),
        one=(2, 1), k_cut=2, nhwc=(1, 1), wd_part=True, mom_init=[0, 1, 1],
        seed=2),
    STOCK: dict(
        B=3, steps=[0, 2],
        hp=dict(wd=5e-4, m=0.9, damp=0.0, nesterov=False), short=None,
        one=None, k_cut=2, nhwc=(0, 1), wd_part=False, mom_init=[1, 0],
        seed=43),
}
SHAPES = list(CASES)
MARGIN = 64.0


def make_case(g, geo, B, steps, M, *, m, nhwc=(0, 0), layout=None, N=None,
              short=None, one=None, mom_init=None):
    """operands of one call (CPU tensors, fp32 / int32).  Server weights are
    random with scale 1 / sqrt(fan_in), biases 0.1; pad gaps of server /
    in_mom are non-zero (they must pass through / stay).  `short` =
    (client, step, n): that step gets n valid rows, the rest padding; `one`
    = (client, step): a one-row step."""
    if layout is None:
        layout, N = make_layout(*geo, nhwc=nhwc)
    Cin, S = layout['image']
    K = layout['fc2'][2]
    C, T = len(steps), max(max(steps), 1)
    server = torch.randn(N, generator=g) * .1
    for lo, hi, _shp, _n, fan in tensors(layout):
        v = torch.randn(hi - lo, generator=g)
        server[lo:hi] = v / fan ** .5 if fan else .1 * v
    X = torch.randn(M, Cin * S * S, generator=g)
    Y = torch.randint(0, K, (M,), generator=g).to(torch.int32)
    idx = torch.full((C, T, B), -1, dtype=torch.int32)
    for c in range(C):
        for s in range(steps[c]):
            idx[c, s] = torch.randperm(M, generator=g)[:B]
    if short is not None:
        c, s, n = short
        idx[c, s, n:] = -1
    if one is not None:
        idx[one[0], one[1], 1:] = -1
    in_mom = torch.randn(C, N, generator=g) * .01 if m != 0 else None
    if mom_init is None:
        mom_init = [c % 2 for c in range(C)]
    return dict(X=X, Y=Y, idx=idx,
                steps=torch.tensor(steps, dtype=torch.int32), server=server,
                replicas=torch.full((C, N), NAN), in_mom=in_mom,
                mom_init=torch.tensor(mom_init, dtype=torch.int32), N=N,
                layout=layout)


def run_ref(case, lr, k_cut, hp, snap, wd_numel, dtype=F64, pre=None):
    return ref_rounds(case['X'], case['Y'], case['idx'], case['steps'], lr,
                      case['server'], case['replicas'], case['in_mom'],
                      case['mom_init'], snap, k_cut, case['layout'],
                      wd_numel, hp['wd'], hp['m'], hp['damp'],
                      hp['nesterov'], dtype=dtype, pre=pre)


def margins(p64, p32):
    """{kind: (smallest distance of a decision from a tie in the float64
    replay, largest error of the fp32 replay)} over the recorded steps: for a
    conv, a window's maximum from zero and, where it is positive, from the
    window's runner-up; for fc1, a pre-activation from zero"""
    out = {}
    for kind in KINDS:
        lo, e = float('inf'), 0.0
        for a, b in zip(p64, p32):
            z = a[kind]
            e = max(e, (b[kind].double() - z).abs().max().item())
            if kind == 'fc1':
                lo = min(lo, z.abs().min().item())
                continue
            top = windows(z).sort(-1, descending=True)[0]
            lo = min(lo, top[..., 0].abs().min().item())
            pos = top[..., 0] > 0
            if bool(pos.any()):
                lo = min(lo, (top[..., 0] - top[..., 1])[pos].min().item())
        out[kind] = (lo, e)
    return out


def decision_margin(case, lr, k_cut, hp, snap, wd_numel):
    """(ref64, ref32, margins)"""
    p64, p32 = [], []
    ref = run_ref(case, lr, k_cut, hp, snap, wd_numel, pre=p64)
    r32 = run_ref(case, lr, k_cut, hp, snap, wd_numel, dtype=F32, pre=p32)
    return ref, r32, margins(p64, p32)


def build(geo, seed):
    spec = CASES[geo]
    g = lc.gen('cnn', geo, seed)
    hp, B, steps = spec['hp'], spec['B'], spec['steps']
    case = make_case(g, geo, B, steps, 3 * B + 7, m=hp['m'],
                     nhwc=spec['nhwc'], short=spec['short'], one=spec['one'],
                     mom_init=spec['mom_init'])
    C, T = len(steps), max(steps)
    lr = torch.rand(C, T, generator=g) * .05 + .01      # changes per step
    snap = torch.full((C, case['N']), NAN)
    # wd on a prefix only: up to the middle of fc1's weight
    lo, hi = tensors(case['layout'])[4][:2]
    wd_numel = (lo + hi) // 2 if spec['wd_part'] else case['N']
    return case, lr, spec['k_cut'], hp, snap, wd_numel


@functools.lru_cache(maxsize=None)
def case(geo):
    """(case, lr, k_cut, hp, snap, wd_numel, ref64, e32) of a geometry of
    CASES, computed once and shared: treat it as read-only.  e32: the largest
    error of the same loop in fp32 on the CPU, per output.

    Precondition, asserted here: ReLU and max-pool make the loss non-smooth,
    so in the float64 replay every pool window's maximum lies farther from
    zero -- and, where it is positive, farther above the window's runner-up
    -- than 64 times the fp32 replay's largest error in that conv's outputs,
    and every fc1 pre-activation that far from zero; then no rounding of
    fp32 size flips a decision."""
    cs, lr, k_cut, hp, snap, wd_numel = build(geo, CASES[geo]['seed'])
    ref, r32, mg = decision_margin(cs, lr, k_cut, hp, snap, wd_numel)
    for kind, (lo, e) in mg.items():
        assert lo > MARGIN * e, ('a %s decision is too close to a tie' % kind,
                                 geo, lo, e)
    e32 = {k: lc.err(r32[k], ref[k]) for k in OUTPUTS if ref[k] is not None}
    return cs, lr, k_cut, hp, snap, wd_numel, ref, e32


def scale_of(t):
    return t[~torch.isnan(t)].abs().max().item()


def call_op(ops, case, lr, k_cut, hp, snap, wd_numel, device='cpu', op=None):
    """run ops.cnn_local_rounds on copies of the case's operands on `device`;
    returns dict like ref_rounds"""
    d = lambda t: None if t is None else t.clone().to(device)  # noqa: E731
    rep, mom, mi, sn = (d(case['replicas']), d(case['in_mom']),
                        d(case['mom_init']), d(snap))
    loss = (op or ops.cnn_local_rounds)(
        d(case['X']), d(case['Y']), d(case['idx']), d(case['steps']), d(lr),
        d(case['server']), rep, mom, mi, sn, k_cut, layout=case['layout'],
        wd_numel=wd_numel, weight_decay=hp['wd'], momentum=hp['m'],
        dampening=hp['damp'], nesterov=hp['nesterov'])
    return dict(replicas=rep, in_mom=mom, mom_init=mi, snap=sn, loss=loss)
