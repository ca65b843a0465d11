# -*- coding: utf-8 -*-
"""Packed char-GRU: time per federated round of the slot loop
(FEDTORCH_PACKED_BATCHED_RNN off: per client and step the fused GRU sequence
kernels with token-gathered input gates, library decoder and loss, autograd,
one fused SGD launch) against the batched round (on: the clients' steps
batched per layer by ops.rnn_local_rounds, hip/rnnround.h).  Needs a GPU.

Configuration: the stock `rnn` (V = 86, H = 50, T = 50) on the synthetic
character stream, B = 10, tau = 10, momentum 0.9, C in {16, 128} virtual
clients on one rank, every client online, every client's windows in an
un-augmented DeviceCachedLoader (both paths read the same loaders).

Every configuration runs in a process of its own (started from here, one at
a time): it builds the federation once, warms both paths up, then runs
--rounds rounds of each path ALTERNATELY; a round is timed wall-clock between
two device synchronisations (it includes the host's plan walk, the
aggregation and the replica re-sync, which both paths share).  The full range
of each path is printed.  The two paths agree only up to the hidden state:
the slot loop threads the shared module's state through the clients, the
batched round carries one per client.

--hidden H runs the same at another hidden size; 65 <= H <= 128 times
ops.rnn_wide_local_rounds (hip/rnnround_wide.h, both opt-ins) against the
slot loop on the register-resident sequence kernels
(FEDTORCH_FUSED_GRU_WIDE)."""
import argparse
import os
import statistics
import subprocess
import sys
import time

os.environ['FEDTORCH_FUSED_GRU'] = '1'
os.environ['FEDTORCH_FUSED_GRU_TOKENS'] = '1'
os.environ['FEDTORCH_FUSED_GRU_WIDE'] = '1'     # read for 65 <= H <= 128 only

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fedtorch_amd import ops  # noqa: E402
from fedtorch_amd.parallel import multiclient  # noqa: E402

B, TAU = 10, 10


def federation(C, H):
    from fedtorch_amd.parameters import get_args
    from fedtorch_amd.nodes import Client
    from fedtorch_amd.components.datasets.device_cache import \
        DeviceCachedLoader
    from fedtorch_amd.components.datasets.sources import ArrayDataset
    torch.manual_seed(1)
    np.random.seed(1)
    argv = ['-d', 'shakespeare', '--iid_data', 'false', '-a', 'rnn',
            '--rnn_hidden_size', str(H),
            '-f', 'true', '--federated_type', 'fedavg', '--num_comms', '1',
            '--clients_per_rank', str(C), '-b', str(B), '--lr', '0.05',
            '--federated_sync_type', 'local_step', '--local_step', str(TAU),
            '--online_client_rate', '1.0', '--in_momentum', 'true',
            '--in_momentum_factor', '0.9', '--weight_decay', '1e-4',
            '--stop_criteria', 'epoch', '--num_epochs', '1000',
            '--on_cuda', 'true', '-j', '0', '--manual_seed', '7',
            '--checkpoint', '/tmp/ft_packed_rnn_micro', '--debug', 'false']
    client = Client(get_args(argv), 0)
    client.initialize()
    client.initialize_dataset()
    client.load_local_dataset()
    client.gen_aux_models()
    pack = multiclient.ClientPack(client, C)
    pack.build_loaders()
    for j, old in enumerate(pack.train_loaders):
        part = old.dataset
        ii = torch.as_tensor(list(part.indices))
        n = len(ii) - (len(ii) % B == 1)       # no 1-sample last batch
        pack.train_loaders[j] = DeviceCachedLoader(
            ArrayDataset(part.data.x[ii[:n]], part.data.y[ii[:n]]), B,
            seed=7 * 1000003 + j * 8191, shuffle=True, device='cuda')
    return client, pack


def one_round(client, pack, batched):
    from fedtorch_amd.trainings.packed import \
        train_and_validate_federated_packed
    multiclient._BATCHED_RNN_ENABLED = batched
    multiclient._BATCHED_RNN_WIDE_ENABLED = batched
    assert pack.rnn_batched_eligible() == batched, pack.rnn_batched_blockers()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    train_and_validate_federated_packed(client, pack)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def configuration(C, a):
    """one configuration, in this process"""
    if not (torch.cuda.is_available() and ops.hip_available()):
        raise SystemExit('packed_rnn_micro needs a GPU and the built kernel '
                         'pack')
    client, pack = federation(C, a.hidden)
    for _ in range(max(a.warmup, 1)):
        for batched in (False, True):
            one_round(client, pack, batched)
    t = {False: [], True: []}
    for _ in range(a.rounds):
        for batched in (False, True):
            t[batched].append(one_round(client, pack, batched))
    s, f = t[False], t[True]
    print('rnn shakespeare fedavg V=86 H=%d T=50 B=%d tau=%d C=%d momentum=on'
          ' ms/round: slot loop [%.2f, %.2f] median %.2f | batched [%.2f, '
          '%.2f] median %.2f | %s; median ratio %.1f' % (
              a.hidden, B, TAU, C, min(s), max(s), statistics.median(s),
              min(f), max(f),
              statistics.median(f),
              'disjoint, below' if max(f) < min(s) else
              'disjoint, above' if min(f) > max(s) else 'overlap',
              statistics.median(s) / statistics.median(f)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--clients', type=str, default='16,128')
    ap.add_argument('--hidden', type=int, default=50)
    ap.add_argument('--single', action='store_true',
                    help='run the one configuration named by --clients in '
                         'this process')
    a = ap.parse_args()
    if a.single:
        configuration(int(a.clients), a)
        return
    for C in a.clients.split(','):
        subprocess.run([sys.executable, os.path.abspath(__file__), '--single',
                        '--clients', C, '--rounds', str(a.rounds),
                        '--warmup', str(a.warmup), '--hidden',
                        str(a.hidden)], check=True)
    print('PACKED_RNN_MICRO_OK')


if __name__ == '__main__':
    main()
