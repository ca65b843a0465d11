# -*- coding: utf-8 -*-
"""Arena op pack: the math hot paths of the framework.

Every op operates on FLAT arena tensors (see `fedtorch_amd/parallel/arena.py`)
and has two implementations:

* ``_C`` — the hand-written CDNA4 HIP kernel pack (gfx950), built in-tree by
  ``setup.py build_ext --inplace`` / ``__graft_entry__.build()``.  This is the
  path that runs on MI355X; ops FAIL LOUDLY if a CUDA tensor arrives and the
  extension is missing (no silent eager fallback on GPU).
* eager torch — used on CPU (tests, gloo plumbing config) and when the user
  passes ``--hip_kernels false``.

Math semantics follow the reference exactly (file:line cited per op).
"""
import torch

_C = None
_C_ERR = None
try:
    import importlib
    # NOTE: must go through importlib — a plain `from ... import _C` would
    # resolve to this module's own `_C = None` attribute, not the .so.
    _C = importlib.import_module('fedtorch_amd.ops._C')
except Exception as e:  # pragma: no cover - exercised only when not built
    _C_ERR = e

# users can force eager (``--hip_kernels false``); tests can flip it too.
FORCE_EAGER = False


def hip_available():
    return _C is not None


def _use_hip(*tensors):
    if FORCE_EAGER:
        return False
    if not any(t.is_cuda for t in tensors if isinstance(t, torch.Tensor)):
        return False
    if _C is None:
        raise RuntimeError(
            'fedtorch_amd HIP kernel pack (fedtorch_amd/ops/_C) is not built '
            'but a GPU tensor reached an arena op. Build it with '
            '`python setup.py build_ext --inplace` (or run '
            '__graft_entry__.build()). Original import error: %r' % (_C_ERR,))
    return True


# --------------------------------------------------------------------------
# fused dual-mode SGD step (reference `components/optimizers/sgd.py:67-128`)
# --------------------------------------------------------------------------

def fused_sgd_step(param, grad, *, lr, scale, weight_decay, in_momentum,
                   out_momentum, dampening, nesterov, apply_lr,
                   apply_in_momentum, apply_out_momentum,
                   in_buf=None, out_buf=None, first_in=False, first_out=False,
                   prox_mu=0.0, server=None, ctrl_server=None,
                   ctrl_client=None, delta=None, wd_numel=None,
                   half_param=None):
    """One pass over the arena: the reference's dual-use SGD step with the
    per-algorithm gradient corrections fused in.

    d = grad
    [fedgate]   d -= delta                      (`trainings/federated/main.py:116-119`)
    [scaffold]  d += ctrl_server - ctrl_client  (`main.py:120-122`)
    [fedprox]   d += prox_mu * (param - server) (`main.py:123-129`)
    [local]     d += weight_decay * param       (`sgd.py:96-97`, only if apply_lr;
                only the first `wd_numel` elements — BatchNorm params are
                packed at the arena tail and skip wd, matching the reference
                optimizer factory `components/optimizer.py:8-16`)
    [in mom]    buf = m*buf + (1-damp)*d ; d = nesterov ? d + m*buf : buf
                (first use: buf = d, `sgd.py:100-110`)
    [out mom]   likewise on the sync step       (`sgd.py:112-123`)
    param -= (apply_lr ? lr : scale) * d        (`sgd.py:125-128`)

    The reference applies corrections by mutating p.grad before step
    (`main.py:116-129`); fusing keeps one kernel and leaves `grad` unchanged.
    """
    if _use_hip(param, grad):
        return _C.fused_sgd_step(
            param, grad,
            in_buf if in_buf is not None else torch.empty(0, device=param.device),
            out_buf if out_buf is not None else torch.empty(0, device=param.device),
            delta if delta is not None else torch.empty(0, device=param.device),
            ctrl_server if ctrl_server is not None else torch.empty(0, device=param.device),
            ctrl_client if ctrl_client is not None else torch.empty(0, device=param.device),
            server if server is not None else torch.empty(0, device=param.device),
            float(lr), float(scale), float(weight_decay),
            float(in_momentum), float(out_momentum), float(dampening),
            bool(nesterov), bool(apply_lr), bool(apply_in_momentum),
            bool(apply_out_momentum), bool(first_in), bool(first_out),
            float(prox_mu),
            int(wd_numel) if wd_numel is not None else param.numel(),
            half_param if half_param is not None
            else torch.empty(0, device=param.device))

    d = grad
    if delta is not None:
        d = d - delta
    if ctrl_server is not None:
        d = d + (ctrl_server - ctrl_client)
    if prox_mu != 0.0 and server is not None:
        d = d + prox_mu * (param - server)
    if d is grad:
        d = grad.clone()
    if weight_decay != 0 and apply_lr:
        nw = wd_numel if wd_numel is not None else param.numel()
        d[:nw].add_(param[:nw], alpha=weight_decay)
    if in_momentum != 0 and apply_in_momentum:
        if first_in:
            in_buf.copy_(d)
        else:
            in_buf.mul_(in_momentum).add_(d, alpha=1 - dampening)
        if nesterov:
            d = d.add(in_buf, alpha=in_momentum)
        else:
            d = in_buf.clone()
    if out_momentum != 0 and apply_out_momentum:
        if first_out:
            out_buf.copy_(d)
        else:
            out_buf.mul_(out_momentum).add_(d, alpha=1 - dampening)
        if nesterov:
            d = d.add(out_buf, alpha=out_momentum)
        else:
            d = out_buf.clone()
    param.add_(d, alpha=-(lr if apply_lr else scale))
    if half_param is not None:  # refresh the bf16 compute copy
        half_param.copy_(param)


# --------------------------------------------------------------------------
# weighted model-diff + restore (reference `federated/fedavg.py:30-34`)
# --------------------------------------------------------------------------

def weighted_diff_restore(server, client, out, weight):
    """out = (server - client) * weight ; client = server — one pass."""
    if _use_hip(server, client, out):
        return _C.weighted_diff_restore(server, client, out, float(weight))
    torch.sub(server, client, out=out)
    out.mul_(weight)
    client.copy_(server)


def scaled_diff(a, b, out, weight):
    """out = (a - b) * weight (no restore)."""
    if _use_hip(a, b, out):
        return _C.scaled_diff(a, b, out, float(weight))
    torch.sub(a, b, out=out)
    out.mul_(weight)


def axpby(y, x, a=1.0, b=1.0):
    """y = b*y + a*x."""
    if _use_hip(y, x):
        return _C.axpby(y, x, float(a), float(b))
    y.mul_(b).add_(x, alpha=a)


# --------------------------------------------------------------------------
# adaptive quantization (reference `comms/utils/flow_utils.py:169-212`)
# --------------------------------------------------------------------------

def quantize(x, num_bits=8):
    """Adaptive min/max/mean quantization, exactly the reference formula:
    scale = (max-min)/(qmax-qmin) (0 -> 0.001), zp = clamp(int(qmin -
    (min-mean)/scale)), q = round(clamp(zp + (x-mean)/scale)).
    Returns (q int8/int16 tensor, info float32 [scale, zp, mean])."""
    qmin = -2.0 ** (num_bits - 1)
    qmax = 2.0 ** (num_bits - 1) - 1.0
    if _use_hip(x):
        return _C.quantize_adaptive(x, int(num_bits))
    min_val, max_val, mean_val = x.min(), x.max(), x.mean()
    scale = (max_val - min_val) / (qmax - qmin)
    if scale == 0.0:
        scale = torch.tensor(0.001, dtype=x.dtype, device=x.device)
    initial_zp = qmin - (min_val - mean_val) / scale
    zero_point = int(initial_zp.clamp(qmin, qmax).item())
    q = (zero_point + (x - mean_val) / scale).clamp_(qmin, qmax).round_()
    q = q.to(torch.int8 if num_bits == 8 else torch.int16)
    info = torch.stack([scale.float(),
                        torch.tensor(float(zero_point), device=x.device),
                        mean_val.float()]).to(x.device)
    return q, info


def dequantize(q, info):
    """x = scale * (q - zp) + mean (reference `flow_utils.py:208-212`)."""
    if _use_hip(q, info):
        return _C.dequantize(q, info)
    return info[0] * (q.float() - info[1]) + info[2]


def dequant_accumulate(qs, infos, out):
    """out = sum_k dequantize(qs[k], infos[k]) — fused over the gathered
    world (reference does list-of-dense + stack + sum,
    `federated/fedavg.py:53-54`). `qs`: [K, N] int8/16, `infos`: [K, 3]."""
    if _use_hip(qs, out):
        return _C.dequant_accumulate(qs, infos, out)
    out.zero_()
    for k in range(qs.shape[0]):
        out += infos[k, 0] * (qs[k].float() - infos[k, 1]) + infos[k, 2]


# --------------------------------------------------------------------------
# top-k compression (reference `flow_utils.py:218-237`)
# --------------------------------------------------------------------------

def topk_compress(x, k):
    """values+indices of the k largest |x| (reference keeps k = numel*r/2).
    Returns (v float32[k], i int32[k])."""
    if k <= 0:
        raise ValueError('Compression ratio is too low!')
    if _use_hip(x):
        return _C.topk_compress(x, int(k))
    _, idx = x.abs().topk(k)
    v = x[idx]
    return v, idx.to(torch.int32)


def scatter_accumulate(out, vs, idxs):
    """out = sum_k scatter(vs[k] at idxs[k]) — fused decompress-sum over the
    gathered compressed streams (reference materializes K dense tensors,
    `flow_utils.py:232-237` + `fedgate.py:79`).
    vs: [K, k] float32, idxs: [K, k] int32; out zeroed here."""
    if _use_hip(out, vs):
        return _C.scatter_accumulate(out, vs, idxs)
    out.zero_()
    for kk in range(vs.shape[0]):
        out.scatter_add_(0, idxs[kk].long(), vs[kk])


def multi_diff_accumulate(server, replicas, weights, out):
    """out = sum_c weights[c] * (server - replicas[c]) — ONE pass over the
    [C, N] replica arena (packed virtual clients)."""
    wsum = float(weights.sum())
    if _use_hip(server, replicas, out):
        return _C.multi_diff_accumulate(server, replicas, weights, out,
                                        wsum)
    torch.sum((server.unsqueeze(0) - replicas) * weights.view(-1, 1), dim=0,
              out=out)


def multi_delta_update(delta, server, agg, replicas, inv):
    """delta[c] += (server - agg - replicas[c]) * inv[c] for every row with
    inv[c] != 0 (the other rows are neither read nor written) — `delta_update`
    over the [C, N] rows of the packed clients in ONE pass; inv: [C] fp32,
    1 / (lr_c tau_c) or 0."""
    if _use_hip(delta, server, agg, replicas):
        return _C.multi_delta_update(delta, server, agg, replicas, inv)
    for c, coef in enumerate(inv.tolist()):
        if coef != 0.0:
            delta[c].add_(server - agg - replicas[c], alpha=coef)


def multi_scaffold_control_update(ctrl, ctrl_server, server, replicas, inv,
                                  weights, out):
    """For every row with inv[c] != 0, in client order:
    c+ = ctrl[c] - ctrl_server + (server - replicas[c]) * inv[c],
    out += weights[c] * (c+ - ctrl[c]), ctrl[c] = c+ ; out starts from zero.
    `scaffold_control_update` + the weighted control delta over the [C, N]
    rows of the packed clients in ONE pass; rows with inv[c] == 0 are left
    untouched and contribute nothing."""
    if _use_hip(ctrl, ctrl_server, server, replicas, out):
        return _C.multi_scaffold_control_update(ctrl, ctrl_server, server,
                                                replicas, inv, weights, out)
    out.zero_()
    for c, (coef, w) in enumerate(zip(inv.tolist(), weights.tolist())):
        if coef == 0.0:
            continue
        new = (ctrl[c] - ctrl_server).add_(server - replicas[c], alpha=coef)
        out.add_(new - ctrl[c], alpha=w)
        ctrl[c].copy_(new)


def fedadam_normalize(g, seg, v, beta, tau):
    """FedAdam server normalizer (reference `federated/fedavg.py:81-85`,
    arXiv:2003.00295): per-parameter-tensor v_p = beta*v_p +
    (1-beta)*||g_p||, then g_p /= (sqrt(v_p)+tau).  `seg`: int64 [P,2]
    arena (start,end) offsets; `v`: float32 [P] device-resident state.
    One kernel on GPU — zero host syncs (the reference loops P tensors
    with float(torch.norm(...)) each)."""
    if _use_hip(g, v):
        return _C.fedadam_normalize(g, seg, v, float(beta), float(tau))
    for p_i in range(v.numel()):
        s_, e_ = int(seg[p_i, 0]), int(seg[p_i, 1])
        gp = g[s_:e_]
        v[p_i] = beta * v[p_i] + (1.0 - beta) * torch.norm(gp)
        gp /= (torch.sqrt(v[p_i]) + tau)


def error_feedback_update(mem, grad, d, inv_weight):
    """mem += grad * inv_weight - d (reference `fedgate.py:81`,
    `qsparse.py:57`: `memory += grad/rank_weight - d`)."""
    if _use_hip(mem, grad, d):
        return _C.error_feedback_update(mem, grad, d, float(inv_weight))
    mem.add_(grad, alpha=inv_weight).sub_(d)


def delta_update(delta, server, agg, client, inv_lr_tau):
    """delta += (server - agg - client) * inv_lr_tau
    (reference `fedgate.py:104`: delta += (server - d - client)/(lr*tau))."""
    if _use_hip(delta, server, agg, client):
        return _C.delta_update(delta, server, agg, client, float(inv_lr_tau))
    delta.add_((server - agg - client), alpha=inv_lr_tau)


def scaffold_control_update(ctrl_new, ctrl_client, ctrl_server, server, client,
                            inv_lr_tau):
    """c+ = c - c_server + (w_server - w_client)/(tau*lr)
    (reference `scaffold.py:26-27`)."""
    if _use_hip(ctrl_new, ctrl_client):
        return _C.scaffold_control_update(ctrl_new, ctrl_client, ctrl_server,
                                          server, client, float(inv_lr_tau))
    ctrl_new.copy_(ctrl_client).sub_(ctrl_server).add_(server - client,
                                                       alpha=inv_lr_tau)


# --------------------------------------------------------------------------
# packed linear models: all clients' local steps of a round in ONE launch
# (hip/linearround.h)
# --------------------------------------------------------------------------

# LDS floats the kernel declares (159 KiB of a gfx950 CU's 160 KiB); kept
# equal to LINROUND_LDS_FLOATS of hip/linearround.h (a GPU test compares).
LINROUND_LDS_FLOATS = 40704
LINROUND_MAXK = 16


def linear_round_lds_floats(F, K, B, uses_momentum):
    """LDS floats one client needs: the resident [F + 1, K | 1] image of
    weight and bias (twice with momentum) plus B * (K + 2) of step scratch."""
    return (2 if uses_momentum else 1) * (F + 1) * (K | 1) + B * (K + 2)


def linear_round_max_floats(uses_momentum):
    """LDS floats left for one client's resident image (F + 1) * (K | 1);
    the step scratch B * (K + 2) comes off the same budget."""
    return LINROUND_LDS_FLOATS // (2 if uses_momentum else 1)


def linear_local_rounds(X, Y, idx, steps, lr, server, replicas, in_mom,
                        mom_init, snap, k_cut, *, w_off, b_off, K, loss_kind,
                        weight_decay, momentum, dampening, nesterov,
                        delta=None, ctrl_server=None, ctrl_client=None,
                        prox_mu=0.0):
    """All local SGD steps of a round, for every packed client of a linear
    model, in one call.

    X [M, F] f32, Y [M] (int32 class ids | f32 targets); idx [C, T, B] int32
    rows of X per sample, -1 = padding; steps [C] int32 (0 = offline, nothing
    of that client is read or written); lr [C, T] f32; server [N];
    replicas [C, N] (out); in_mom [C, N] or None/empty; mom_init [C] int32
    (in/out); snap [C, N] or None/empty: parameters BEFORE step k_cut
    (1-based), written when 1 <= k_cut <= steps[c].  weight [K, F] sits at
    `w_off`, bias [K] at `b_off` of the arena; every other element is copied
    through.  loss_kind 0 = softmax-CE (mean), 1 = MSE (mean, K == 1).
    The update is the local branch of `fused_sgd_step`, with its gradient
    corrections: delta [C, N] (d -= delta[c]), or the pair ctrl_server [N] /
    ctrl_client [C, N] (d += ctrl_server - ctrl_client[c]), and prox_mu
    (d += prox_mu * (p - server)).  Only the weight and bias elements of the
    correction rows of clients with steps > 0 are read.  in_mom / mom_init
    are touched only when momentum != 0.  Returns loss [C, T]: the mean loss
    of each executed step, 0 elsewhere."""
    dev = X.device
    if (ctrl_server is None) != (ctrl_client is None):
        raise RuntimeError('linear_local_rounds: ctrl_server and ctrl_client '
                           'come as a pair')
    if delta is not None and ctrl_server is not None:
        raise RuntimeError('linear_local_rounds: delta and a control pair '
                           'together are not supported (one correction '
                           'vector per client)')
    if in_mom is None:
        in_mom = torch.empty(0, device=dev)
    if snap is None:
        snap = torch.empty(0, device=dev)
    if _use_hip(X, server, replicas):
        return _C.linear_local_rounds(
            X, Y, idx, steps, lr, server, replicas, in_mom, mom_init, snap,
            int(k_cut), int(w_off), int(b_off), int(K), int(loss_kind),
            float(weight_decay), float(momentum), float(dampening),
            bool(nesterov),
            delta if delta is not None else torch.empty(0, device=dev),
            ctrl_server if ctrl_server is not None
            else torch.empty(0, device=dev),
            ctrl_client if ctrl_client is not None
            else torch.empty(0, device=dev),
            float(prox_mu))

    # eager twin: a per-client, per-step loop; the gradients come from
    # autograd over F.linear + the loss module's functional, the update from
    # the fused-SGD twin above over the whole row — the ops of the packed
    # slot loop, in its order.  Pad gaps (zero in a real arena, where the
    # whole-row update leaves them zero) are put back afterwards; those of
    # the correction rows are masked, never used.
    import torch.nn.functional as Fn
    C, T, _B = idx.shape
    Fdim = X.shape[1]
    nw = K * Fdim
    use_mom = momentum != 0
    loss = torch.zeros((C, T), dtype=torch.float32, device=dev)
    n_steps = steps.tolist()
    inits = mom_init.tolist()
    gap = torch.ones_like(server, dtype=torch.bool)
    gap[w_off:w_off + nw] = False
    gap[b_off:b_off + K] = False
    zero = torch.zeros_like(server)
    live = lambda t: torch.where(gap, zero, t)  # noqa: E731
    for c in range(C):
        if n_steps[c] <= 0:
            continue
        p = server.clone()
        grad = torch.zeros_like(p)
        corr = dict(prox_mu=prox_mu, server=server if prox_mu != 0 else None)
        if delta is not None:
            corr['delta'] = live(delta[c])
        if ctrl_server is not None:
            corr.update(ctrl_server=live(ctrl_server),
                        ctrl_client=live(ctrl_client[c]))
        mom_gaps = in_mom[c][gap].clone() if use_mom else None
        for s in range(n_steps[c]):
            if snap.numel() and s + 1 == k_cut:
                snap[c].copy_(torch.where(gap, server, p))
            rows = idx[c, s]
            rows = rows[rows >= 0].long()
            x = X[rows]
            w = p[w_off:w_off + nw].view(K, Fdim).clone().requires_grad_(True)
            b = p[b_off:b_off + K].clone().requires_grad_(True)
            with torch.enable_grad():
                out = Fn.linear(x, w, b)
                if loss_kind == 0:
                    l = Fn.cross_entropy(out, Y[rows].long())
                else:
                    l = Fn.mse_loss(out, Y[rows].unsqueeze(1))
                gw, gb = torch.autograd.grad(l, (w, b))
            loss[c, s] = l.detach()
            grad.zero_()
            grad[w_off:w_off + nw].copy_(gw.reshape(-1))
            grad[b_off:b_off + K].copy_(gb)
            fused_sgd_step(
                p, grad, lr=float(lr[c, s]), scale=1.0,
                weight_decay=weight_decay, in_momentum=momentum,
                out_momentum=0.0, dampening=dampening, nesterov=nesterov,
                apply_lr=True, apply_in_momentum=use_mom,
                apply_out_momentum=False,
                in_buf=in_mom[c] if use_mom else None,
                first_in=use_mom and not inits[c], **corr)
            if use_mom:
                inits[c] = 1
        replicas[c].copy_(torch.where(gap, server, p))
        if use_mom:
            in_mom[c][gap] = mom_gaps
            mom_init[c] = 1
    return loss


# --------------------------------------------------------------------------
# packed MLP: all clients' local steps batched per layer (hip/mlpround.h)
# --------------------------------------------------------------------------

# kept equal to MLPROUND_MAXB / _MAXK / _MAXL of hip/mlpround.h (a GPU test
# compares)
MLPROUND_MAXB = 64
MLPROUND_MAXK = 128
MLPROUND_MAXL = 8


def mlp_round_max_batch():
    """largest batch size B of ops.mlp_local_rounds (the smallest is 2)"""
    return MLPROUND_MAXB


def mlp_round_max_classes():
    """largest class count K of ops.mlp_local_rounds"""
    return MLPROUND_MAXK


def _mlp_layout_flat(layout):
    """[L, (w, b, gamma, beta, in, out) x L, fc, H, K] of a layout dict"""
    blocks = [tuple(int(v) for v in blk) for blk in layout['blocks']]
    head = tuple(int(v) for v in layout['head'])
    if any(len(blk) != 6 for blk in blocks) or len(head) != 3:
        raise ValueError('mlp_local_rounds: a layout block is (w_off, b_off, '
                         'gamma_off, beta_off, in, out), the head (fc_off, '
                         'H, K)')
    flat = [len(blocks)]
    for blk in blocks:
        flat.extend(blk)
    flat.extend(head)
    return flat


def _mlp_layout_check(layout, F, N):
    """the launcher's layout checks for the eager twin; returns the spans
    [(start, end)] of the parameter tensors in the arena"""
    who = 'mlp_local_rounds: '
    flat = _mlp_layout_flat(layout)
    L = flat[0]
    if not 1 <= L <= MLPROUND_MAXL:
        raise ValueError(who + 'layout has %d blocks (1 <= L <= %d)'
                         % (L, MLPROUND_MAXL))
    spans, prev = [], F
    for i, (w, b, g, be, fin, out) in enumerate(layout['blocks']):
        if fin != prev or out < 1:
            raise ValueError(who + 'layout block %d is [%d, %d] but its '
                             'input has %d features' % (i, out, fin, prev))
        spans += [(w, w + fin * out), (b, b + out), (g, g + out),
                  (be, be + out)]
        prev = out
    fc, H, K = layout['head']
    if H != prev:
        raise ValueError(who + 'layout head reads %d features but the last '
                         'block has %d' % (H, prev))
    if not 1 <= K <= MLPROUND_MAXK:
        raise ValueError(who + 'unsupported K=%d (1 <= K <= %d)'
                         % (K, MLPROUND_MAXK))
    spans.append((fc, fc + H * K))
    for lo, hi in spans:
        if lo < 0 or hi > N:
            raise ValueError(who + 'layout tensor [%d, %d) does not fit the '
                             'arena of %d' % (lo, hi, N))
    order = sorted(spans)
    for (_l0, h0), (l1, _h1) in zip(order, order[1:]):
        if h0 > l1:
            raise ValueError(who + 'layout tensors overlap at arena element '
                             '%d' % l1)
    return spans


def mlp_local_rounds(X, Y, idx, steps, lr, server, replicas, in_mom,
                     mom_init, snap, k_cut, *, layout, eps, wd_numel,
                     weight_decay, momentum, dampening, nesterov,
                     delta=None, ctrl_server=None, ctrl_client=None,
                     prox_mu=0.0):
    """All local SGD steps of a round, for every packed client of an MLP
    (`components/models/mlp.py` without noise), batched per layer.

    X [M, F] f32, Y [M] int32 class ids; idx [C, T, B] int32 rows of X per
    sample, -1 = padding, 2 <= B <= 64; steps [C] int32 (0 = offline, nothing
    of that client is read or written); lr [C, T] f32; server [N];
    replicas [C, N] (out); in_mom [C, N] or None/empty; mom_init [C] int32
    (in/out); snap [C, N] or None/empty: parameters BEFORE step k_cut
    (1-based), written when 1 <= k_cut <= steps[c].

    layout: dict(blocks=[(w_off, b_off, gamma_off, beta_off, in, out), ...],
    head=(fc_off, H, K)): the arena offsets and shapes of the L blocks
    Linear(in, out) + BatchNorm1d(out) + ReLU and of the bias-free head
    Linear(H, K), K <= 128.  BatchNorm uses the batch's statistics (biased
    variance, `eps`, affine).

    for every client c with steps[c] > 0:
      replicas[c] <- server                    (whole row, pad gaps included)
      for s in 0 .. steps[c]-1, rows r = idx[c, s, :] >= 0, n = #rows >= 2:
        [snap[c] <- replicas[c]   if s + 1 == k_cut]
        a_0 = X[r]
        z_i = a_i W_i^T + b_i ; mu, var over the n rows
        xh = (z - mu) rsqrt(var + eps) ; y_i = g_i xh + beta_i
        a_{i+1} = max(y_i, 0)
        logits = a_L Wfc^T ; loss[c, s] = mean CE(logits, Y[r])
        backward of exactly that ; d = grad ; [delta] d -= delta[c] ;
        [control pair] d += ctrl_server - ctrl_client[c] ;
        [prox_mu] d += prox_mu (p - server) ; d += wd p for arena index
        < wd_numel ; momentum / dampening / nesterov / first use
        (mom_init[c] == 0 at s == 0: buf = d) ; p -= lr[c, s] d
        -- the local branch of `fused_sgd_step` with its gradient
        corrections, in place in replicas[c] (and in_mom[c])
      mom_init[c] <- 1 (with momentum)

    delta [C, N], or the pair ctrl_server [N] / ctrl_client [C, N], and
    prox_mu >= 0 are constant over the call; only the parameter elements of
    the correction rows of clients with steps > 0 are read.  Pad gaps of in_mom stay as they were; in_mom / mom_init are touched only
    when momentum != 0.  Returns loss [C, T]: the mean loss of each executed
    step, 0 elsewhere.  The eager twin raises ValueError for an executed
    step with fewer than 2 valid rows; the HIP path cannot see a device idx
    and stays in bounds and finite there (n = 1 gives xh = 0)."""
    dev = X.device
    if (ctrl_server is None) != (ctrl_client is None):
        raise RuntimeError('mlp_local_rounds: ctrl_server and ctrl_client '
                           'come as a pair')
    if delta is not None and ctrl_server is not None:
        raise RuntimeError('mlp_local_rounds: delta and a control pair '
                           'together are not supported (one correction '
                           'vector per client)')
    if in_mom is None:
        in_mom = torch.empty(0, device=dev)
    if snap is None:
        snap = torch.empty(0, device=dev)
    if _use_hip(X, server, replicas):
        return _C.mlp_local_rounds(
            X, Y, idx, steps, lr, server, replicas, in_mom, mom_init, snap,
            int(k_cut), _mlp_layout_flat(layout), float(eps), int(wd_numel),
            float(weight_decay), float(momentum), float(dampening),
            bool(nesterov),
            delta if delta is not None else torch.empty(0, device=dev),
            ctrl_server if ctrl_server is not None
            else torch.empty(0, device=dev),
            ctrl_client if ctrl_client is not None
            else torch.empty(0, device=dev),
            float(prox_mu))

    # eager twin: a per-client, per-step loop; the gradients come from
    # autograd over F.linear / F.batch_norm / F.relu / F.cross_entropy, the
    # update from the fused-SGD twin above over the whole row — the ops of
    # the packed slot loop, in its order.  Pad gaps (zero in a real arena,
    # where the whole-row update leaves them zero) are put back afterwards;
    # those of the correction rows are masked, never used.
    import torch.nn.functional as Fn
    C, T, B = idx.shape
    N = server.numel()
    spans = _mlp_layout_check(layout, X.shape[1], N)
    if not 2 <= B <= MLPROUND_MAXB:
        raise ValueError('mlp_local_rounds: unsupported B=%d (2 <= B <= %d)'
                         % (B, MLPROUND_MAXB))
    if k_cut < 0:
        raise ValueError('mlp_local_rounds: k_cut is %d, expected >= 0'
                         % k_cut)
    if not (0 <= prox_mu < float('inf')):
        raise ValueError('mlp_local_rounds: prox_mu must be finite and >= 0, '
                         'got %r' % (prox_mu,))
    n_steps = steps.tolist()
    if max(n_steps) > T:
        raise ValueError('mlp_local_rounds: steps holds %d but idx has T=%d'
                         % (max(n_steps), T))
    for c in range(C):
        for s in range(n_steps[c]):
            if int((idx[c, s] >= 0).sum()) < 2:
                raise ValueError(
                    'mlp_local_rounds: step %d of client %d has fewer than 2 '
                    'samples (BatchNorm needs the batch statistics)' % (s, c))
    use_mom = momentum != 0
    loss = torch.zeros((C, T), dtype=torch.float32, device=dev)
    inits = mom_init.tolist()
    gap = torch.ones_like(server, dtype=torch.bool)
    for lo, hi in spans:
        gap[lo:hi] = False
    shapes = []                              # (offset, shape) in forward order
    for w, b, g, be, fin, out in layout['blocks']:
        shapes += [(w, (out, fin)), (b, (out,)), (g, (out,)), (be, (out,))]
    fc, H, K = layout['head']
    shapes.append((fc, (K, H)))
    zero = torch.zeros_like(server)
    live = lambda t: torch.where(gap, zero, t)  # noqa: E731
    for c in range(C):
        if n_steps[c] <= 0:
            continue
        p = server.clone()
        grad = torch.zeros_like(p)
        corr = dict(prox_mu=prox_mu, server=server if prox_mu != 0 else None)
        if delta is not None:
            corr['delta'] = live(delta[c])
        if ctrl_server is not None:
            corr.update(ctrl_server=live(ctrl_server),
                        ctrl_client=live(ctrl_client[c]))
        mom_gaps = in_mom[c][gap].clone() if use_mom else None
        for s in range(n_steps[c]):
            if snap.numel() and s + 1 == k_cut:
                snap[c].copy_(torch.where(gap, server, p))
            rows = idx[c, s]
            rows = rows[rows >= 0].long()
            ts = []
            for off, shp in shapes:
                n_el = 1
                for v in shp:
                    n_el *= v
                ts.append(p[off:off + n_el].view(shp).clone()
                          .requires_grad_(True))
            with torch.enable_grad():
                a = X[rows]
                for i in range(len(layout['blocks'])):
                    w_, b_, g_, be_ = ts[4 * i:4 * i + 4]
                    a = Fn.relu(Fn.batch_norm(Fn.linear(a, w_, b_), None,
                                              None, g_, be_, True, 0.1, eps))
                l = Fn.cross_entropy(Fn.linear(a, ts[-1]), Y[rows].long())
                gs = torch.autograd.grad(l, ts)
            loss[c, s] = l.detach()
            grad.zero_()
            for (off, _shp), gt in zip(shapes, gs):
                grad[off:off + gt.numel()].copy_(gt.reshape(-1))
            fused_sgd_step(
                p, grad, lr=float(lr[c, s]), scale=1.0,
                weight_decay=weight_decay, in_momentum=momentum,
                out_momentum=0.0, dampening=dampening, nesterov=nesterov,
                apply_lr=True, apply_in_momentum=use_mom,
                apply_out_momentum=False,
                in_buf=in_mom[c] if use_mom else None,
                first_in=use_mom and not inits[c], wd_numel=wd_numel,
                **corr)
            if use_mom:
                inits[c] = 1
        replicas[c].copy_(torch.where(gap, server, p))
        if use_mom:
            in_mom[c][gap] = mom_gaps
            mom_init[c] = 1
    return loss


# --------------------------------------------------------------------------
# packed CNN: all clients' local steps batched per layer (hip/cnnround.h)
# --------------------------------------------------------------------------

# kept equal to the CNNROUND_MAX* of hip/cnnround.h (a GPU test compares)
CNNROUND_MAXB = 64
CNNROUND_MAXK = 128
CNNROUND_MAXCIN = 4
CNNROUND_MAXS = 32
CNNROUND_MAXC1 = 24
CNNROUND_MAXC2 = 64
CNNROUND_MAXH = 4096


def cnn_round_limits():
    """the largest B, K, Cin, S, C1, C2, H of ops.cnn_local_rounds"""
    return dict(B=CNNROUND_MAXB, K=CNNROUND_MAXK, Cin=CNNROUND_MAXCIN,
                S=CNNROUND_MAXS, C1=CNNROUND_MAXC1, C2=CNNROUND_MAXC2,
                H=CNNROUND_MAXH)


def _cnn_layout_flat(layout):
    """[Cin, S, w1, b1, C1, nhwc1, w2, b2, C2, nhwc2, fw1, fb1, H, fw2, fb2,
    K] of a layout dict"""
    parts = [tuple(int(v) for v in layout[k])
             for k in ('image', 'conv1', 'conv2', 'fc1', 'fc2')]
    if [len(p) for p in parts] != [2, 4, 4, 3, 3]:
        raise ValueError('cnn_local_rounds: a layout is image=(Cin, S), '
                         'conv1 / conv2=(w_off, b_off, C, nhwc), fc1 / fc2='
                         '(w_off, b_off, out)')
    return [v for p in parts for v in p]


def cnn_layout_check(layout, F, N):
    """the launcher's layout checks (ValueError); returns the spans
    [(start, end)] of the eight parameter tensors in the arena, in the order
    conv1 w, b, conv2 w, b, fc1 w, b, fc2 w, b"""
    who = 'cnn_local_rounds: '
    (Cin, S, w1, b1, C1, n1, w2, b2, C2, n2, fw1, fb1, H, fw2, fb2,
     K) = _cnn_layout_flat(layout)
    if not (1 <= Cin <= CNNROUND_MAXCIN and 1 <= S <= CNNROUND_MAXS):
        raise ValueError(who + 'unsupported image (Cin=%d, S=%d), 1 <= Cin '
                         '<= %d, S <= %d' % (Cin, S, CNNROUND_MAXCIN,
                                             CNNROUND_MAXS))
    if S < 6 or (S - 4) % 2 or (S - 4) // 2 < 6 or ((S - 4) // 2 - 4) % 2:
        raise ValueError(who + 'S=%d does not pool evenly twice (S - 4 and '
                         '(S - 4) / 2 - 4 even, the last map at least 1x1)'
                         % S)
    S2 = ((S - 4) // 2 - 4) // 2
    F2 = C2 * S2 * S2
    if F != Cin * S * S:
        raise ValueError(who + 'X has %d features, the image (%d, %d, %d) '
                         'has %d' % (F, Cin, S, S, Cin * S * S))
    if not (1 <= C1 <= CNNROUND_MAXC1 and 1 <= C2 <= CNNROUND_MAXC2
            and 1 <= H <= CNNROUND_MAXH):
        raise ValueError(who + 'unsupported C1=%d C2=%d H=%d (C1 <= %d, C2 '
                         '<= %d, H <= %d)' % (C1, C2, H, CNNROUND_MAXC1,
                                              CNNROUND_MAXC2, CNNROUND_MAXH))
    if not 1 <= K <= CNNROUND_MAXK:
        raise ValueError(who + 'unsupported K=%d (1 <= K <= %d)'
                         % (K, CNNROUND_MAXK))
    if n1 not in (0, 1) or n2 not in (0, 1):
        raise ValueError(who + 'the nhwc flag of a conv must be 0 or 1')
    spans = [(w1, w1 + C1 * Cin * 25), (b1, b1 + C1),
             (w2, w2 + C2 * C1 * 25), (b2, b2 + C2),
             (fw1, fw1 + H * F2), (fb1, fb1 + H),
             (fw2, fw2 + K * H), (fb2, fb2 + K)]
    for lo, hi in spans:
        if lo < 0 or hi > N:
            raise ValueError(who + 'layout tensor [%d, %d) does not fit the '
                             'arena of %d' % (lo, hi, N))
    order = sorted(spans)
    for (_l0, h0), (l1, _h1) in zip(order, order[1:]):
        if h0 > l1:
            raise ValueError(who + 'layout tensors overlap at arena element '
                             '%d' % l1)
    return spans


def cnn_local_rounds(X, Y, idx, steps, lr, server, replicas, in_mom,
                     mom_init, snap, k_cut, *, layout, wd_numel,
                     weight_decay, momentum, dampening, nesterov):
    """All local SGD steps of a round, for every packed client of the
    LeNet-style CNN of `components/models/cnn.py`, batched per layer.

    X [M, Cin*S*S] f32, a row is one image in (c, h, w) order; Y [M] int32
    class ids; idx [C, T, B] int32 rows of X per sample, -1 = padding,
    1 <= B <= 64; steps [C] int32 (0 = offline, nothing of that client is
    read or written); lr [C, T] f32; server [N]; replicas [C, N] (out);
    in_mom [C, N] or None/empty; mom_init [C] int32 (in/out); snap [C, N] or
    None/empty: parameters BEFORE step k_cut (1-based), written when
    1 <= k_cut <= steps[c].

    layout: dict(image=(Cin, S), conv1=(w_off, b_off, C1, nhwc),
    conv2=(w_off, b_off, C2, nhwc), fc1=(w_off, b_off, H),
    fc2=(w_off, b_off, K)): the arena offsets and shapes.  Kernel size 5,
    stride 1, no padding and pool 2/2 are fixed.  `nhwc`: the conv weight's
    elements sit in the arena as [co][kh][kw][ci] (a channels_last parameter,
    `parallel/arena.py`), else as [co][ci][kh][kw].  Limits:
    `cnn_round_limits()`; S - 4 and S1 - 4 even, S2 >= 1.

    for every client c with steps[c] > 0:
      replicas[c] <- server                    (whole row, pad gaps included)
      for s in 0 .. steps[c]-1, rows r = idx[c, s, :] >= 0, n = #rows >= 1:
        [snap[c] <- replicas[c]   if s + 1 == k_cut]
        x  = X[r] as [n, Cin, S, S]
        p1 = maxpool2(relu(conv5(x,  W1) + b1))    S1 = (S - 4) / 2
        p2 = maxpool2(relu(conv5(p1, W2) + b2))    S2 = (S1 - 4) / 2
        a  = relu(flat(p2) Wf1^T + bf1)            flat (c2 * S2 + h) * S2 + w
        logits = a Wf2^T + bf2 ; loss[c, s] = mean CE(logits, Y[r])
        backward of exactly that (pool: the first maximum of a window in
        scan order; ReLU mask z > 0) ; d = grad ; d += wd p for arena index
        < wd_numel ; momentum / dampening / nesterov / first use
        (mom_init[c] == 0 at s == 0: buf = d) ; p -= lr[c, s] d
        -- the local branch of `fused_sgd_step`, in place in replicas[c]
        (and in_mom[c])
      mom_init[c] <- 1 (with momentum)

    Pad gaps of in_mom stay as they were; in_mom / mom_init are touched only
    when momentum != 0.  Returns loss [C, T]: the mean loss of each executed
    step, 0 elsewhere.  The eager twin raises ValueError for an executed
    step with no valid row; the HIP path cannot see a device idx and stays
    in bounds and finite there."""
    dev = X.device
    if in_mom is None:
        in_mom = torch.empty(0, device=dev)
    if snap is None:
        snap = torch.empty(0, device=dev)
    if _use_hip(X, server, replicas):
        return _C.cnn_local_rounds(
            X, Y, idx, steps, lr, server, replicas, in_mom, mom_init, snap,
            int(k_cut), _cnn_layout_flat(layout), int(wd_numel),
            float(weight_decay), float(momentum), float(dampening),
            bool(nesterov))

    # eager twin: a per-client, per-step loop; the gradients come from
    # autograd over F.conv2d / F.max_pool2d / F.relu / F.linear /
    # F.cross_entropy, the update from the fused-SGD twin above over the
    # whole row -- the ops of the packed slot loop, in its order.  Pad gaps
    # (zero in a real arena, where the whole-row update leaves them zero) are
    # put back afterwards.
    import torch.nn.functional as Fn
    who = 'cnn_local_rounds: '
    for name, t, dt in (('X', X, torch.float32), ('Y', Y, torch.int32),
                        ('idx', idx, torch.int32),
                        ('steps', steps, torch.int32),
                        ('lr', lr, torch.float32),
                        ('server', server, torch.float32),
                        ('replicas', replicas, torch.float32),
                        ('mom_init', mom_init, torch.int32)):
        if t.dtype != dt or not t.is_contiguous() or t.device != dev:
            raise ValueError(who + '%s must be contiguous %s on %s'
                             % (name, dt, dev))
    if X.dim() != 2 or idx.dim() != 3 or server.dim() != 1:
        raise ValueError(who + 'X is [M, F], idx [C, T, B], server [N]')
    C, T, B = idx.shape
    N = server.numel()
    M = X.shape[0]
    use_mom = momentum != 0
    for name, t in (('in_mom', in_mom if use_mom else None),
                    ('snap', snap if snap.numel() else None)):
        if t is not None and (t.dtype != torch.float32
                              or not t.is_contiguous() or t.device != dev):
            raise ValueError(who + '%s must be contiguous %s on %s'
                             % (name, torch.float32, dev))
    if nesterov and (not use_mom or dampening != 0):
        raise ValueError(who + 'nesterov needs a momentum and zero '
                         'dampening')
    want = [('Y', Y, (M,)), ('steps', steps, (C,)), ('lr', lr, (C, T)),
            ('replicas', replicas, (C, N)), ('mom_init', mom_init, (C,))]
    if use_mom:
        want.append(('in_mom', in_mom, (C, N)))
    if snap.numel():
        want.append(('snap', snap, (C, N)))
    for name, t, shp in want:
        if tuple(t.shape) != shp:
            raise ValueError(who + '%s must be %s, got %s'
                             % (name, list(shp), list(t.shape)))
    if not 1 <= B <= CNNROUND_MAXB:
        raise ValueError(who + 'unsupported B=%d (1 <= B <= %d)'
                         % (B, CNNROUND_MAXB))
    if k_cut < 0:
        raise ValueError(who + 'k_cut is %d, expected >= 0' % k_cut)
    if not 0 <= wd_numel <= N:
        raise ValueError(who + 'wd_numel is %d, the arena has %d'
                         % (wd_numel, N))
    spans = cnn_layout_check(layout, X.shape[1], N)
    n_steps = steps.tolist()
    if max(n_steps) > T:
        raise ValueError(who + 'steps holds %d but idx has T=%d'
                         % (max(n_steps), T))
    if int(idx.max()) >= M:
        raise ValueError(who + 'idx holds row %d but X has %d rows'
                         % (int(idx.max()), M))
    for c in range(C):
        for s in range(n_steps[c]):
            if int((idx[c, s] >= 0).sum()) < 1:
                raise ValueError(who + 'step %d of client %d has no sample'
                                 % (s, c))
    (Cin, S, _w1, _b1, C1, n1, _w2, _b2, C2, n2, _fw1, _fb1, H, _fw2, _fb2,
     K) = _cnn_layout_flat(layout)
    F2 = (spans[4][1] - spans[4][0]) // H
    # (4-D shape as stored, nhwc) per tensor, in the order of `spans`
    shapes = [((C1, Cin, 5, 5), n1), ((C1,), 0), ((C2, C1, 5, 5), n2),
              ((C2,), 0), ((H, F2), 0), ((H,), 0), ((K, H), 0), ((K,), 0)]
    loss = torch.zeros((C, T), dtype=torch.float32, device=dev)
    inits = mom_init.tolist()
    gap = torch.ones_like(server, dtype=torch.bool)
    for lo, hi in spans:
        gap[lo:hi] = False
    for c in range(C):
        if n_steps[c] <= 0:
            continue
        p = server.clone()
        grad = torch.zeros_like(p)
        mom_gaps = in_mom[c][gap].clone() if use_mom else None
        for s in range(n_steps[c]):
            if snap.numel() and s + 1 == k_cut:
                snap[c].copy_(torch.where(gap, server, p))
            rows = idx[c, s]
            rows = rows[rows >= 0].long()
            ts = []
            for (lo, hi), (shp, nhwc) in zip(spans, shapes):
                t = p[lo:hi].clone()
                if nhwc:
                    co, ci, kh, kw = shp
                    t = t.view(co, kh, kw, ci).permute(0, 3, 1, 2)
                else:
                    t = t.view(shp)
                ts.append(t.requires_grad_(True))
            with torch.enable_grad():
                a = X[rows].view(-1, Cin, S, S)
                a = Fn.max_pool2d(Fn.relu(Fn.conv2d(a, ts[0], ts[1])), 2, 2)
                a = Fn.max_pool2d(Fn.relu(Fn.conv2d(a, ts[2], ts[3])), 2, 2)
                a = Fn.relu(Fn.linear(a.reshape(-1, F2), ts[4], ts[5]))
                l = Fn.cross_entropy(Fn.linear(a, ts[6], ts[7]),
                                     Y[rows].long())
                gs = torch.autograd.grad(l, ts)
            loss[c, s] = l.detach()
            grad.zero_()
            for (lo, hi), (_shp, nhwc), gt in zip(spans, shapes, gs):
                if nhwc:
                    gt = gt.permute(0, 2, 3, 1)
                grad[lo:hi].copy_(gt.reshape(-1))
            fused_sgd_step(
                p, grad, lr=float(lr[c, s]), scale=1.0,
                weight_decay=weight_decay, in_momentum=momentum,
                out_momentum=0.0, dampening=dampening, nesterov=nesterov,
                apply_lr=True, apply_in_momentum=use_mom,
                apply_out_momentum=False,
                in_buf=in_mom[c] if use_mom else None,
                first_in=use_mom and not inits[c], wd_numel=wd_numel)
            if use_mom:
                inits[c] = 1
        replicas[c].copy_(torch.where(gap, server, p))
        if use_mom:
            in_mom[c][gap] = mom_gaps
            mom_init[c] = 1
    return loss


# --------------------------------------------------------------------------
# small host-side math (not perf-critical)
# --------------------------------------------------------------------------

def euclidean_proj_simplex(v, s=1):
    """Projection onto the simplex (reference `flow_utils.py:52-97`,
    Duchi et al. sort+cumsum algorithm). v: 1-D float tensor on any device."""
    assert s > 0
    n = v.numel()
    if bool((v.sum() == s).item()) and bool((v >= 0).all().item()):
        return v
    u, _ = torch.sort(v, descending=True)
    cssv = torch.cumsum(u, dim=0)
    arange = torch.arange(1, n + 1, device=v.device, dtype=v.dtype)
    nz = torch.nonzero(u * arange > (cssv - s), as_tuple=False)
    rho = nz[-1].squeeze() if len(nz) else torch.tensor(0, device=v.device)
    theta = (cssv[rho] - s) / (rho.to(v.dtype) + 1.0)
    return (v - theta).clamp(min=0)


def alpha_grad(local_flat, personal_flat, local_grad, personal_grad, alpha):
    """APFL adaptive-alpha gradient (reference `flow_utils.py:240-250`):
    grad_alpha = <w_p - w_l, alpha*g_p + (1-alpha)*g_l> + 0.02*alpha.
    One fused reduction over the arenas instead of a per-param loop."""
    if _use_hip(local_flat, personal_flat):
        ga = _C.alpha_grad(local_flat, personal_flat, local_grad,
                           personal_grad, float(alpha))
    else:
        dif = personal_flat - local_flat
        g = alpha * personal_grad + (1 - alpha) * local_grad
        ga = torch.dot(dif, g)
    return float(ga) + 0.02 * alpha


def blend(out, a, b, alpha):
    """out = alpha*a + (1-alpha)*b (APFL inference blend,
    reference `comms/utils/eval.py:31-39` blends logits; arena variant blends
    whatever flat buffer is handed in)."""
    if _use_hip(out, a, b):
        return _C.blend(out, a, b, float(alpha))
    torch.add(a.mul(alpha), b, alpha=1 - alpha, out=out)
