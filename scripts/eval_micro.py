# -*- coding: utf-8 -*-
"""Eval-mode ResNet-20 forward: FEDTORCH_MFMA_EVAL off vs on (needs a GPU).

Times the whole forward of the converted channels_last ResNet-20 in eval
mode under no_grad + bf16 autocast, the way trainings/eval.py::do_validate
runs it, at N=256 and at the validation batch size of the smoke() /
flagship federated configuration (`-b 128`; the eval loaders use
args.batch_size).  Both settings are warmed up first, then sampled
alternately in ONE process: each sample is device events around --iters
(>= 200) forwards, --samples (>= 5) samples per setting; min / median / max
are printed so the spread is visible.  Two weight states are measured: the
4-D weights already in bf16 (the bf16 compute twin of the hipGraph path) and
fp32 master weights that every forward casts.

--kernels additionally counts the kernels of ONE forward per setting with
the torch profiler (in this process, after the timing)."""
import argparse
import os
import statistics
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fedtorch_amd import ops  # noqa: E402
from fedtorch_amd.ops import conv3x3 as c3  # noqa: E402

CL = torch.channels_last
VAL_BATCH = 128   # smoke(): '-b 128'


def build(bf16_weights):
    from fedtorch_amd.components.models.resnet import resnet
    from fedtorch_amd.ops.batchnorm import convert_to_fused_bn
    from fedtorch_amd.ops.stemconv import convert_stem
    torch.manual_seed(41)
    m = resnet(SimpleNamespace(arch='resnet20', data='cifar10')).cuda().to(
        memory_format=CL)
    convert_to_fused_bn(m)
    convert_stem(m)
    g = torch.Generator().manual_seed(5)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            C = mod.num_features
            mod.running_mean.copy_((torch.randn(C, generator=g) * .2).cuda())
            mod.running_var.copy_((torch.rand(C, generator=g) + .5).cuda())
    if bf16_weights:
        for p in m.parameters():
            if p.dim() == 4 and p is not m.conv1.weight:
                p.data = p.data.bfloat16()
    return m.eval()


def forward(m, x, flag):
    c3._EVAL_ENABLED = flag
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16):
        return m(x)


def sample(m, x, flag, iters):
    """ms per forward over `iters` forwards between two device events"""
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(iters):
        forward(m, x, flag)
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / iters


def count_kernels(m, x, flag):
    from torch.profiler import ProfilerActivity, profile
    forward(m, x, flag)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        forward(m, x, flag)
        torch.cuda.synchronize()
    names = {}
    for ev in prof.events():
        if ev.device_type == torch.autograd.DeviceType.CUDA and \
                'memcpy' not in ev.name.lower() and \
                'memset' not in ev.name.lower():
            key = ev.name.split('(')[0].split('<')[0][:60]
            names[key] = names.get(key, 0) + 1
    return names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--samples', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--batches', default='256,%d' % VAL_BATCH)
    ap.add_argument('--kernels', action='store_true')
    a = ap.parse_args()
    if a.iters < 200 or a.samples < 5:
        ap.error('--iters >= 200 and --samples >= 5')
    if not (torch.cuda.is_available() and ops.hip_available()):
        raise SystemExit('eval_micro needs a GPU and the built kernel pack')
    old = c3._EVAL_ENABLED
    verdict = True
    try:
        for bf16_weights in (True, False):
            m = build(bf16_weights)
            for N in (int(b) for b in a.batches.split(',')):
                torch.manual_seed(42)
                x = torch.randn(N, 3, 32, 32, device='cuda').to(
                    memory_format=CL)
                outs = {}
                for flag in (False, True):       # warm up BOTH first
                    for _ in range(a.warmup):
                        outs[flag] = forward(m, x, flag)
                torch.cuda.synchronize()
                d = (outs[True].float() - outs[False].float()).abs().max()
                t = {False: [], True: []}
                for _ in range(a.samples):       # alternate off / on
                    for flag in (False, True):
                        t[flag].append(sample(m, x, flag, a.iters))
                tag = 'weights %s N=%d' % (
                    'bf16' if bf16_weights else 'fp32', N)
                for flag in (False, True):
                    v = sorted(t[flag])
                    print('%s flag %s: min %.4f median %.4f max %.4f ms/fwd '
                          '(%d samples x %d fwd)' % (
                              tag, 'on ' if flag else 'off', v[0],
                              statistics.median(v), v[-1], len(v), a.iters))
                below = max(t[True]) < min(t[False])
                verdict = verdict and below
                print('%s: on-range entirely below off-range: %s; '
                      'max |logit diff| on vs off %.4f' % (tag, below,
                                                           d.item()))
                if a.kernels:
                    for flag in (False, True):
                        try:
                            names = count_kernels(m, x, flag)
                        except Exception as e:   # profiler not available
                            print('%s flag %d kernels: not measured (%r)'
                                  % (tag, flag, e))
                            continue
                        print('%s flag %s: %d kernels per forward' % (
                            tag, 'on ' if flag else 'off',
                            sum(names.values())))
                        for k, n in sorted(names.items(),
                                           key=lambda kv: -kv[1]):
                            print('    %3d  %s' % (n, k))
    finally:
        c3._EVAL_ENABLED = old
    print('EVAL_MICRO default FEDTORCH_MFMA_EVAL=%d by the range rule'
          % verdict)
    print('EVAL_MICRO_OK')


if __name__ == '__main__':
    main()
