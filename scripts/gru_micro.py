# -*- coding: utf-8 -*-
"""Char-GRU sequence layer: FEDTORCH_FUSED_GRU off (nn.GRU, the library RNN
path) vs on (one F.linear + the persistent gru_fwd / gru_bwd kernels of
hip/gru.h).  With --hidden 65..128 --wide 1 the fused setting also turns on
FEDTORCH_FUSED_GRU_WIDE (gru_wide_fwd / gru_wide_bwd of hip/gru_wide.h), with
--hidden 129..256 --stream 1 FEDTORCH_FUSED_GRU_STREAM (gru_stream_fwd /
gru_stream_bwd of hip/gru_stream.h).
Needs a GPU.

(a) per call: forward + backward of the GRU layer alone (fp32, H = --hidden
    (default 50), T = 50, B in {10, 50, 128}; gradients of x, h0 and the
    four parameters).
(b) one full CharGRU train step each way (vocab 86, the same H, T = 50,
    B = 10): forward, cross-entropy, backward, SGD step.
(c) kernel launches per call of (a) and per step of (b), counted with the
    torch profiler (device-kernel events; memcpy / memset listed apart).

With --tokens 1 a third setting joins (b): "tokens", the fused path plus
FEDTORCH_FUSED_GRU_TOKENS (gru_tok_fwd + gru_tok_grads over the [V, 3H]
table, ops/gru.py::gru_tok_seq); its baseline is "fused", the path without
the third flag, in the same run.  Two more tables are printed:

(d) embedding + GRU layer, forward + backward (gradients of the embedding
    weight, h0 and the four GRU parameters), B in {10, 128}: stock / fused /
    tokens.
(e) gru_tok_grads alone against the cat + GEMM + sum it replaces
    (hh_weight_grad + hh_bias_grad; the library side gets no dP), B in
    {10, 128}, for 4, 8 and 16 waves per workgroup and the built-in choice.

All settings are warmed up first, then sampled alternately in ONE process:
each sample is device events around --iters repetitions, --samples samples
per setting; min / median / max are printed so the spread is visible."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fedtorch_amd import ops  # noqa: E402
from fedtorch_amd.components.models.rnn import CharGRU  # noqa: E402
from fedtorch_amd.ops import gru as fgru  # noqa: E402

H, T, V = 50, 50, 86
# name -> (FUSED_GRU, FUSED_GRU_TOKENS); --tokens 1 appends 'tokens'
SETTINGS = [('stock', (False, False)), ('fused', (True, False))]


def timed(fn, iters):
    """ms per call of fn over `iters` calls between two device events"""
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / iters


def report(tag, t, base=None):
    """every setting against `base`, or (default) against the one before it:
    fused against stock, tokens against fused"""
    for name in t:
        v = sorted(t[name])
        print('%s %-6s min %.4f median %.4f max %.4f ms (%d samples)' % (
            tag, name, v[0], statistics.median(v), v[-1], len(v)))
    names = list(t)
    for prev, name in zip(names, names[1:]):
        ref = base or prev
        s, f = t[ref], t[name]
        print('%s %s range [%.4f, %.4f] vs %s [%.4f, %.4f]: %s; '
              'median ratio %s/%s %.2f' % (
                  tag, name, min(f), max(f), ref, min(s), max(s),
                  'disjoint, below' if max(f) < min(s) else
                  'disjoint, above' if min(f) > max(s) else 'overlap',
                  ref, name, statistics.median(s) / statistics.median(f)))


def launches(fn):
    """(device kernels, memcpy/memset) of one call of fn, by the profiler"""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        kern = mem = 0
        for e in prof.events():
            if str(e.device_type).endswith('CUDA'):
                if e.name.lower().startswith(('memcpy', 'memset')):
                    mem += 1
                else:
                    kern += 1
        return kern, mem
    except Exception as e:  # the profiler is optional equipment
        return 'unavailable (%s)' % type(e).__name__, None


def set_flags(flag, a):
    fused, tokens = flag if isinstance(flag, tuple) else (flag, False)
    fgru._GRU_ENABLED = fused
    fgru._GRU_WIDE_ENABLED = fused and bool(a.wide)
    fgru._GRU_STREAM_ENABLED = fused and bool(a.stream)
    fgru._GRU_TOK_ENABLED = tokens


def compare(tag, call, a, settings=None, base=None):
    settings = settings or SETTINGS[:2]
    for _name, flag in settings:                 # warm up ALL first
        for _ in range(a.warmup):
            call(flag)
    t = {name: [] for name, _f in settings}
    for _ in range(a.samples):                   # alternate the settings
        for name, flag in settings:
            t[name].append(timed(lambda: call(flag), a.iters))
    report(tag, t, base)
    if a.launches:
        for name, flag in settings:
            print('%s %-6s launches per call: kernels %s, memcpy/memset %s'
                  % ((tag, name) + launches(lambda: call(flag))))


def layer(a):
    H = a.hidden
    for B in (10, 50, 128):
        torch.manual_seed(B)
        gru = nn.GRU(H, H, batch_first=True).cuda()
        x = torch.randn(B, T, H, device='cuda', requires_grad=True)
        h0 = torch.randn(1, B, H, device='cuda', requires_grad=True)
        dout = torch.randn(B, T, H, device='cuda')
        leaves = (x, h0) + tuple(gru.parameters())

        def call(flag):
            set_flags(flag, a)
            out, _hn = fgru.gru_seq(gru, x, h0)
            torch.autograd.grad(out, leaves, dout)

        compare('layer fwd+bwd B=%d ms/call' % B, call, a)


def train_step(a):
    B, H = 10, a.hidden
    torch.manual_seed(1)
    models, opts = {}, {}
    for name, _flag in SETTINGS:
        torch.manual_seed(2)
        models[name] = CharGRU('shakespeare', V, H, V, B).cuda()
        opts[name] = torch.optim.SGD(models[name].parameters(), lr=0.01)
    x = torch.randint(0, V, (B, T), device='cuda')
    y = torch.randint(0, V, (B, T), device='cuda')
    names = {flag: name for name, flag in SETTINGS}

    def call(flag):
        set_flags(flag, a)
        m, opt = models[names[flag]], opts[names[flag]]
        opt.zero_grad(set_to_none=True)
        F.cross_entropy(m(x), y).backward()
        opt.step()

    compare('CharGRU train step B=%d ms/step' % B, call, a, SETTINGS)


def embedding_layer(a):
    """(d): nn.Embedding + GRU layer, forward + backward"""
    H = a.hidden
    for B in (10, 128):
        torch.manual_seed(B)
        enc = nn.Embedding(V, H).cuda()
        gru = nn.GRU(H, H, batch_first=True).cuda()
        tok = torch.randint(0, V, (B, T), device='cuda')
        h0 = torch.randn(1, B, H, device='cuda', requires_grad=True)
        dout = torch.randn(B, T, H, device='cuda')
        leaves = (enc.weight, h0) + tuple(gru.parameters())

        def call(flag):
            set_flags(flag, a)
            out, _hn = fgru.gru_tok_seq(enc, gru, tok, h0)
            torch.autograd.grad(out, leaves, dout)

        compare('embedding+layer fwd+bwd B=%d ms/call' % B, call, a,
                SETTINGS)


def reduce_alone(a):
    """(e): gru_tok_grads against hh_weight_grad + hh_bias_grad"""
    H = a.hidden
    for B in (10, 128):
        torch.manual_seed(B)
        dgx = torch.randn(B, T, 3 * H, device='cuda')
        dgh = torch.randn(B, T, 3 * H, device='cuda')
        out = torch.randn(B, T, H, device='cuda')
        h0 = torch.randn(B, H, device='cuda')
        tok = torch.randint(0, V, (B, T), device='cuda')

        def call(waves):
            if waves is None:
                fgru.hh_weight_grad(dgh, out, h0)
                fgru.hh_bias_grad(dgh)
            else:
                ops._C.gru_tok_grads(dgx, dgh, out, h0, tok, V, waves)

        compare('reduce alone B=%d ms/call' % B, call, a,
                [('library', None), ('w4', 4), ('w8', 8), ('w16', 16),
                 ('auto', 0)], base='library')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--samples', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--launches', type=int, default=1)
    ap.add_argument('--hidden', type=int, default=H)
    ap.add_argument('--wide', type=int, default=0)
    ap.add_argument('--stream', type=int, default=0)
    ap.add_argument('--tokens', type=int, default=0)
    a = ap.parse_args()
    if a.tokens:
        SETTINGS.append(('tokens', (True, True)))
    covered = a.hidden <= fgru.MAX_H or \
        (a.wide and a.hidden <= fgru.MAX_H_WIDE) or \
        (a.stream and fgru.MAX_H_WIDE < a.hidden <= fgru.MAX_H_STREAM)
    if not covered or (a.tokens and a.hidden > fgru.MAX_H_WIDE):
        raise SystemExit('H = %d is the library path either way (--wide 1 '
                         'covers 65..128, --stream 1 129..256 without '
                         '--tokens)' % a.hidden)
    if not (torch.cuda.is_available() and ops.hip_available()):
        raise SystemExit('gru_micro needs a GPU and the built kernel pack')
    old = (fgru._GRU_ENABLED, fgru._GRU_WIDE_ENABLED, fgru._GRU_TOK_ENABLED,
           fgru._GRU_STREAM_ENABLED)
    try:
        if a.tokens:
            reduce_alone(a)
            embedding_layer(a)
        else:
            layer(a)
        train_step(a)
    finally:
        (fgru._GRU_ENABLED, fgru._GRU_WIDE_ENABLED, fgru._GRU_TOK_ENABLED,
         fgru._GRU_STREAM_ENABLED) = old
    print('GRU_MICRO_OK')


if __name__ == '__main__':
    main()
