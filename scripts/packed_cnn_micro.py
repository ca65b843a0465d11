# -*- coding: utf-8 -*-
"""Packed CNN: time per federated round of the slot loop
(FEDTORCH_PACKED_BATCHED_CNN off: per client and step one eager forward,
backward and fused SGD launch) against the batched round (on: the clients'
steps batched per layer by ops.cnn_local_rounds, hip/cnnround.h).  Needs a
GPU.

Configuration: the stock LeNet-style `cnn` on synthetic MNIST, B = 50,
tau = 10, C in {16, 128} virtual clients on one rank, every client online,
momentum 0.9 on and off.

Every configuration runs in a process of its own (started from here, one at
a time): it builds the federation once, warms both paths up, then runs
--rounds rounds of each path ALTERNATELY; a round is timed wall-clock
between two device synchronisations (it includes the host's plan walk, the
aggregation and the replica re-sync, which both paths share).  The range of
each path is printed so the spread is visible.  The loaders, the counters
and the model carry on from round to round; both paths consume them alike.
--profile adds the device time per launch of each kernel of one batched
round (torch.profiler)."""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fedtorch_amd import ops  # noqa: E402
from fedtorch_amd.parallel import multiclient  # noqa: E402

B, TAU = 50, 10


def federation(C, momentum):
    from fedtorch_amd.parameters import get_args
    from fedtorch_amd.nodes import Client
    os.environ['FEDTORCH_SYNTH_SIZE'] = str(C * 500)
    torch.manual_seed(1)
    np.random.seed(1)
    argv = ['-d', 'mnist', '-a', 'cnn', '-f', 'true',
            '--federated_type', 'fedavg', '--num_comms', '1',
            '--clients_per_rank', str(C), '-b', str(B), '--lr', '0.05',
            '--federated_sync_type', 'local_step', '--local_step', str(TAU),
            '--online_client_rate', '1.0',
            '--in_momentum', 'true' if momentum else 'false',
            '--in_momentum_factor', '0.9', '--weight_decay', '1e-4',
            '--stop_criteria', 'epoch', '--num_epochs', '1000',
            '--on_cuda', 'true', '-j', '0', '--manual_seed', '7',
            '--checkpoint', '/tmp/ft_packed_cnn_micro', '--debug', 'false']
    client = Client(get_args(argv), 0)
    client.initialize()
    client.initialize_dataset()
    client.load_local_dataset()
    client.gen_aux_models()
    pack = multiclient.ClientPack(client, C)
    pack.build_loaders()
    # the slot loop ends a client's epoch on a 1-sample batch, which the
    # batched round does not reproduce: drop that sample for BOTH paths
    cut = 0
    for ld in pack.train_loaders:
        if len(ld.x) % ld.batch_size == 1:
            ld.x, ld.y = ld.x[:-1], ld.y[:-1]
            ld._nb = (len(ld.x) + ld.batch_size - 1) // ld.batch_size
            cut += 1
    if cut:
        print('  (%d client partitions shortened by one sample)' % cut)
    return client, pack


def one_round(client, pack, batched):
    from fedtorch_amd.trainings.packed import \
        train_and_validate_federated_packed
    multiclient._BATCHED_CNN_ENABLED = batched
    assert pack.cnn_batched_eligible() == batched, pack.cnn_batched_blockers()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    train_and_validate_federated_packed(client, pack)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def profile_round(client, pack):
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CPU,
                             ProfilerActivity.CUDA]) as prof:
        one_round(client, pack, True)
    for ev in prof.key_averages():
        if ('cnn_' in ev.key or 'mlp_' in ev.key) and '_k' in ev.key:
            total = getattr(ev, 'device_time_total',
                            getattr(ev, 'cuda_time_total', 0.0))
            print('    %-44s %4d launches  %9.1f us each  %9.2f ms total'
                  % (ev.key[:44], ev.count, total / max(ev.count, 1),
                     total / 1e3), flush=True)


def configuration(C, momentum, a):
    """one configuration, in this process"""
    if not (torch.cuda.is_available() and ops.hip_available()):
        raise SystemExit('packed_cnn_micro needs a GPU and the built kernel '
                         'pack')
    tag = 'cnn mnist B=%d tau=%d C=%d momentum=%s' % (
        B, TAU, C, 'on' if momentum else 'off')
    client, pack = federation(C, momentum)
    layout = pack.cnn_layout()
    print('  conv weight order: conv1 %s, conv2 %s' % tuple(
        'nhwc' if layout[k][3] else 'nchw' for k in ('conv1', 'conv2')))
    for _ in range(max(a.warmup, 1)):
        for batched in (False, True):
            one_round(client, pack, batched)
    t = {False: [], True: []}
    for _ in range(a.rounds):
        for batched in (False, True):
            t[batched].append(one_round(client, pack, batched))
    s, f = t[False], t[True]
    print('%s ms/round: slot loop [%.2f, %.2f] median %.2f | batched [%.2f, '
          '%.2f] median %.2f | %s; median ratio %.1f' % (
              tag, min(s), max(s), statistics.median(s), min(f), max(f),
              statistics.median(f),
              'disjoint, below' if max(f) < min(s) else
              'disjoint, above' if min(f) > max(s) else 'overlap',
              statistics.median(s) / statistics.median(f)), flush=True)
    if a.profile:
        profile_round(client, pack)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--clients', type=str, default='16,128')
    ap.add_argument('--momentum', type=str, default='on,off')
    ap.add_argument('--profile', action='store_true')
    ap.add_argument('--single', action='store_true',
                    help='run the one configuration named by --clients / '
                         '--momentum in this process')
    a = ap.parse_args()
    if a.single:
        configuration(int(a.clients), a.momentum == 'on', a)
        return
    for C in a.clients.split(','):
        for m in a.momentum.split(','):
            cmd = [sys.executable, os.path.abspath(__file__), '--single',
                   '--clients', C, '--momentum', m, '--rounds',
                   str(a.rounds), '--warmup', str(a.warmup)]
            if a.profile:
                cmd.append('--profile')
            subprocess.run(cmd, check=True)
    print('PACKED_CNN_MICRO_OK')


if __name__ == '__main__':
    main()
