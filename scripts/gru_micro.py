# -*- coding: utf-8 -*-
"""Char-GRU sequence layer: FEDTORCH_FUSED_GRU off (nn.GRU, the library RNN
path) vs on (one F.linear + the persistent gru_fwd / gru_bwd kernels of
hip/gru.h).  Needs a GPU.

(a) per call: forward + backward of the GRU layer alone (fp32, H = 50,
    T = 50, B in {10, 50, 128}; gradients of x, h0 and the four parameters).
(b) one full CharGRU train step each way (vocab 86, H = 50, T = 50, B = 10):
    forward, cross-entropy, backward, SGD step.
(c) kernel launches per call of (a) and per step of (b), counted with the
    torch profiler (device-kernel events; memcpy / memset listed apart).

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
SETTINGS = (('stock', False), ('fused', True))


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


def report(tag, t):
    for name in t:
        v = sorted(t[name])
        print('%s %-6s min %.4f median %.4f max %.4f ms (%d samples)' % (
            tag, name, v[0], statistics.median(v), v[-1], len(v)))
    s, f = t['stock'], t['fused']
    print('%s fused range [%.4f, %.4f] vs stock [%.4f, %.4f]: %s; '
          'median ratio stock/fused %.2f' % (
              tag, min(f), max(f), min(s), max(s),
              'disjoint, below' if max(f) < min(s) else
              'disjoint, above' if min(f) > max(s) else 'overlap',
              statistics.median(s) / statistics.median(f)))


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


def compare(tag, call, a):
    for _name, flag in SETTINGS:                 # warm up ALL first
        for _ in range(a.warmup):
            call(flag)
    t = {name: [] for name, _f in SETTINGS}
    for _ in range(a.samples):                   # alternate the settings
        for name, flag in SETTINGS:
            t[name].append(timed(lambda: call(flag), a.iters))
    report(tag, t)
    if a.launches:
        for name, flag in SETTINGS:
            print('%s %-6s launches per call: kernels %s, memcpy/memset %s'
                  % ((tag, name) + launches(lambda: call(flag))))


def layer(a):
    for B in (10, 50, 128):
        torch.manual_seed(B)
        gru = nn.GRU(H, H, batch_first=True).cuda()
        x = torch.randn(B, T, H, device='cuda', requires_grad=True)
        h0 = torch.randn(1, B, H, device='cuda', requires_grad=True)
        dout = torch.randn(B, T, H, device='cuda')
        leaves = (x, h0) + tuple(gru.parameters())

        def call(flag):
            fgru._GRU_ENABLED = flag
            out, _hn = fgru.gru_seq(gru, x, h0)
            torch.autograd.grad(out, leaves, dout)

        compare('layer fwd+bwd B=%d ms/call' % B, call, a)


def train_step(a):
    B = 10
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
        fgru._GRU_ENABLED = flag
        m, opt = models[names[flag]], opts[names[flag]]
        opt.zero_grad(set_to_none=True)
        F.cross_entropy(m(x), y).backward()
        opt.step()

    compare('CharGRU train step B=%d ms/step' % B, call, a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--samples', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--launches', type=int, default=1)
    a = ap.parse_args()
    if not (torch.cuda.is_available() and ops.hip_available()):
        raise SystemExit('gru_micro needs a GPU and the built kernel pack')
    old = fgru._GRU_ENABLED
    try:
        layer(a)
        train_step(a)
    finally:
        fgru._GRU_ENABLED = old
    print('GRU_MICRO_OK')


if __name__ == '__main__':
    main()
