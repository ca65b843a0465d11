# -*- coding: utf-8 -*-
"""Classifier tail: FEDTORCH_FUSED_HEAD / FEDTORCH_FUSED_METRICS off vs on
(needs a GPU).

(a) validate-style pass over the converted channels_last bf16 ResNet-20 in
    eval mode under no_grad + bf16 autocast, at N = 128 and 256: per batch
    the forward, the loss and the top-1/top-5 bookkeeping exactly as
    trainings/eval.py::do_validate does them (stock: inference() + the
    tracker update with their three .item() reads; fused metrics: one
    ce_topk_accum launch and no read), for the four flag settings none /
    head / metrics / both.  ms per batch.
(b) per call: pool + FC forward and backward (head_fwd + head_bwd) against
    the stock tail (adaptive_avg_pool2d + nn.Linear under autocast and their
    autograd backward) on the flagship shape N=256, 8x8x64 bf16 -> 10
    classes, launched eagerly and replayed from a graph of --gcalls calls.

All settings are warmed up first, then sampled alternately in ONE process:
each sample is device events around --iters repetitions, --samples samples
per setting; min / median / max are printed so the spread is visible."""
import argparse
import os
import statistics
import sys
from types import SimpleNamespace

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fedtorch_amd import ops  # noqa: E402
from fedtorch_amd.logs.logging import update_performancec_tracker  # noqa: E402
from fedtorch_amd.logs.meter import define_val_tracker  # noqa: E402
from fedtorch_amd.ops import head  # noqa: E402
from fedtorch_amd.trainings.eval import inference, inference_fused  # noqa: E402

CL = torch.channels_last
SETTINGS = (('none', False, False), ('head', True, False),
            ('metrics', False, True), ('both', True, True))


def build():
    from fedtorch_amd.components.models.resnet import resnet
    from fedtorch_amd.ops.batchnorm import convert_to_fused_bn
    from fedtorch_amd.ops.stemconv import convert_stem
    torch.manual_seed(41)
    m = resnet(SimpleNamespace(arch='resnet20', data='cifar10')).cuda().to(
        memory_format=CL)
    convert_to_fused_bn(m)
    convert_stem(m)
    for p in m.parameters():
        if p.dim() == 4 and p is not m.conv1.weight:
            p.data = p.data.bfloat16()
    return m.eval()


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
        print('%s %-8s min %.4f median %.4f max %.4f ms (%d samples)' % (
            tag, name, v[0], statistics.median(v), v[-1], len(v)))
    base = next(iter(t))
    for name in list(t)[1:]:
        print('%s %s range [%.4f, %.4f] vs %s [%.4f, %.4f]: %s' % (
            tag, name, min(t[name]), max(t[name]), base, min(t[base]),
            max(t[base]),
            'disjoint, below' if max(t[name]) < min(t[base]) else
            'disjoint, above' if min(t[name]) > max(t[base]) else 'overlap'))


def validate_pass(a):
    m = build()
    crit = nn.CrossEntropyLoss()
    metrics = (1, 5)
    for N in (128, 256):
        torch.manual_seed(42)
        x = torch.randn(N, 3, 32, 32, device='cuda').to(memory_format=CL)
        y = torch.randint(0, 10, (N,), device='cuda')
        macc = head.MetricAccumulator('cuda')
        tracker = define_val_tracker()

        def batch(head_on, metrics_on):
            head._HEAD_ENABLED = head_on
            with torch.no_grad(), torch.autocast('cuda',
                                                 dtype=torch.bfloat16):
                if metrics_on:
                    inference_fused(macc, m, crit, metrics, x, y)
                else:
                    loss, perf = inference(m, crit, metrics, x, y)
                    update_performancec_tracker(tracker, loss, perf, N)

        for _name, h, mt in SETTINGS:            # warm up ALL first
            for _ in range(a.warmup):
                batch(h, mt)
        macc.result()
        t = {name: [] for name, _h, _m in SETTINGS}
        for _ in range(a.samples):               # alternate the settings
            for name, h, mt in SETTINGS:
                t[name].append(timed(lambda: batch(h, mt), a.iters))
                macc.result()                    # the one read of a pass
        report('validate N=%d ms/batch' % N, t)


def per_call(a):
    N, C, HW, K = 256, 64, 8, 10
    torch.manual_seed(7)
    fc = nn.Linear(C, K).cuda()
    x = torch.randn(N, C, HW, HW, device='cuda').bfloat16().contiguous(
        memory_format=CL).requires_grad_(True)
    dl = torch.randn(N, K, device='cuda')
    dls = {torch.float32: dl, torch.bfloat16: dl.bfloat16()}  # no cast launch
    leaves = (x, fc.weight, fc.bias)

    def call(head_on):
        head._HEAD_ENABLED = head_on
        with torch.autocast('cuda', dtype=torch.bfloat16):
            out = head.pool_fc(x, fc)
        torch.autograd.grad(out, leaves, dls[out.dtype])

    def graphed(head_on):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                call(head_on)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(a.gcalls):
                call(head_on)
        g.replay()
        return g.replay

    for flag in (False, True):
        for _ in range(a.warmup):
            call(flag)
    t = {'stock': [], 'fused': []}
    for _ in range(a.samples):
        for name, flag in (('stock', False), ('fused', True)):
            t[name].append(timed(lambda: call(flag), a.iters))
    report('tail fwd+bwd N=256 eager ms/call', t)
    replays = {'stock': graphed(False), 'fused': graphed(True)}
    t = {'stock': [], 'fused': []}
    for _ in range(a.samples):
        for name in ('stock', 'fused'):
            t[name].append(timed(replays[name], a.iters) / a.gcalls)
    report('tail fwd+bwd N=256 graph ms/call', t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--samples', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--gcalls', type=int, default=20)
    a = ap.parse_args()
    if not (torch.cuda.is_available() and ops.hip_available()):
        raise SystemExit('head_micro needs a GPU and the built kernel pack')
    old = head._HEAD_ENABLED
    try:
        validate_pass(a)
        per_call(a)
    finally:
        head._HEAD_ENABLED = old
    print('HEAD_MICRO_OK')


if __name__ == '__main__':
    main()
