# -*- coding: utf-8 -*-
"""A packed CNN round through ClientPack on the GPU: FEDTORCH_PACKED_BATCHED_CNN
on (ops.cnn_local_rounds, hip/cnnround.h, on the trainer's real arena offsets,
channels_last packing, stacked loader data and plan walk) against the slot
loop, both against the float64 step loop of tests/cnnround_cases.py.

This test builds an on-GPU Client, which sets torch.backends.cudnn.benchmark
and reseeds every generator for the whole process (utils/init_config.py).  It
puts both back (`process_state`), and it lives in a file of its own that
sorts with the other packed-round GPU tests (test_gpu_linround*,
test_gpu_mlpround*), behind the conv and kernel test files whose references
are library convolutions; the direct tests of the op are in
test_gpu_cnnround.py."""
import random

import numpy as np
import pytest
import torch

import linround_cases as lc
import cnnround_cases as cc
import fedtorch_amd.ops as ops
from fedtorch_amd.parallel import multiclient

pytestmark = pytest.mark.gpu

_REAL_OP = ops.cnn_local_rounds

# model init and loader shuffles for which the precondition below holds;
# searched on the CPU (the loaders' order is a function of the seed alone)
PACKED_SEED = 8
# the margin of a packed run, as in test_cnnround_cpu.py: every path is an
# fp32 evaluation within a small multiple of the fp32 replay's error e of
# the float64 values, so two of them can decide a ReLU or a pool window
# differently only where the float64 margin is below the sum of their
# errors; 4 e allows each path twice the replay's error.  (The 64x margin of
# cnnround_cases.case cannot hold over the 2.5 10^5 decisions of this round.)
PACKED_MARGIN = 4.0


@pytest.fixture
def process_state(monkeypatch):
    """An on-GPU Client changes the process: `init_config` switches
    torch.backends.cudnn.benchmark on (the library's exhaustive solver
    search) and reseeds every generator.  The test hands the process on as
    it found it."""
    monkeypatch.setattr(torch.backends.cudnn, 'benchmark',
                        torch.backends.cudnn.benchmark)
    rng = (torch.get_rng_state(), torch.cuda.get_rng_state(),
           np.random.get_state(), random.getstate())
    yield
    torch.cuda.synchronize()
    torch.set_rng_state(rng[0])
    torch.cuda.set_rng_state(rng[1])
    np.random.set_state(rng[2])
    random.setstate(rng[3])


def _packed_round(batched, monkeypatch, on_cuda=True, seed=None):
    from fedtorch_amd.parameters import get_args
    from fedtorch_amd.nodes import Client
    from fedtorch_amd.trainings.packed import \
        train_and_validate_federated_packed
    monkeypatch.setattr(multiclient, '_BATCHED_CNN_ENABLED', batched)
    monkeypatch.setenv('FEDTORCH_SYNTH_SIZE', '200')
    torch.manual_seed(5)
    np.random.seed(5)
    seed = PACKED_SEED if seed is None else seed
    args = get_args([
        '-d', 'mnist', '-a', 'cnn', '-f', 'true',
        '--federated_type', 'fedavg', '--num_comms', '1',
        '--clients_per_rank', '4', '-b', '5', '--lr', '0.05',
        '--federated_sync_type', 'local_step', '--local_step', '3',
        '--online_client_rate', '1.0', '--in_momentum', 'true',
        '--in_momentum_factor', '0.9', '--weight_decay', '1e-3',
        '--stop_criteria', 'epoch', '--num_epochs', '8',
        '--on_cuda', 'true' if on_cuda else 'false', '-j', '0',
        '--manual_seed', str(seed),
        '--checkpoint', '/tmp/ft_cnnround_gpu', '--debug', 'false'])
    client = Client(args, 0)
    client.initialize()
    client.initialize_dataset()
    client.load_local_dataset()
    client.gen_aux_models()
    pack = multiclient.ClientPack(client, 4)
    pack.build_loaders()
    if not on_cuda:        # the seed search: the loaders a GPU run builds
        from fedtorch_amd.components.datasets.device_cache import \
            DeviceCachedLoader
        for j, old in enumerate(pack.train_loaders):
            pack.train_loaders[j] = DeviceCachedLoader(
                old.dataset, args.batch_size,
                seed=seed * 1000003 + pack.global_id(j) * 8191,
                shuffle=True, device='cpu')
    assert pack.cnn_batched_eligible() == batched, pack.cnn_batched_blockers()
    assert not pack.batched_eligible() and not pack.mlp_batched_eligible()
    rec = {}
    real_acc = pack.accumulate_partial

    def acc(server, weights):
        rec['replicas'] = pack.replicas.clone()
        return real_acc(server, weights)
    monkeypatch.setattr(pack, 'accumulate_partial', acc)

    def op(*a, **k):
        rec['operands'] = ([None if t is None or not torch.is_tensor(t)
                            else t.clone().cpu() for t in a], dict(k))
        return _REAL_OP(*a, **k)
    monkeypatch.setattr(ops, 'cnn_local_rounds', op)
    train_and_validate_federated_packed(client, pack)
    if on_cuda:
        torch.cuda.synchronize()
    rec['in_mom'] = pack.in_mom.clone()
    return rec


def packed_replays(operands):
    """(ref64, ref32, margins) of a recorded batched round"""
    pos, kw = operands
    X, Y, idx, steps, lr, server, replicas, in_mom, mom_init = pos[:9]
    refs, pre = {}, {}
    for dt in (torch.float64, torch.float32):
        pre[dt] = []
        refs[dt] = cc.ref_rounds(
            X, Y, idx, steps, lr, server, replicas, in_mom, mom_init, None,
            0, kw['layout'], kw['wd_numel'], kw['weight_decay'],
            kw['momentum'], kw['dampening'], kw['nesterov'], dtype=dt,
            pre=pre[dt])
    return (refs[torch.float64], refs[torch.float32],
            cc.margins(pre[torch.float64], pre[torch.float32]))


def test_packed_round_kernels_against_slot_loop(process_state, monkeypatch):
    """C = 4, tau = 3, B = 5, the stock MNIST CNN through real
    DeviceCachedLoaders: flag on (the batched kernels) against flag off (the
    slot loop: library convolutions, autograd, the fused SGD kernel).  Both
    are bounded against the float64 loop over the operands the batched round
    recorded; the kernels' error and the distance between the two stay
    within lc.bound (the slot loop's own error is printed).  The decision
    precondition (PACKED_MARGIN) is asserted for the recorded operands."""
    off = _packed_round(False, monkeypatch)
    assert torch.backends.cudnn.benchmark      # what process_state undoes
    on = _packed_round(True, monkeypatch)
    assert 'operands' not in off
    pos, kw = on['operands']
    assert pos[2].shape == (4, 3, 5) and pos[3].tolist() == [3, 3, 3, 3]
    assert pos[9] is None
    assert kw['layout']['image'] == (1, 28)
    ref, r32, mg = packed_replays(on['operands'])
    for kind, (lo, e) in mg.items():
        assert lo > PACKED_MARGIN * e, (kind, lo, e)
    for k in ('replicas', 'in_mom'):
        e32 = lc.err(r32[k], ref[k])
        tol = lc.bound(e32, ref[k].abs().max().item())
        e_on, e_off = lc.err(on[k], ref[k]), lc.err(off[k], ref[k])
        d = (on[k] - off[k]).abs().max().item()
        print('%s: kernel err %.3e  slot loop err %.3e  e32 %.3e  tol %.3e  '
              'on-off %.3e' % (k, e_on, e_off, e32, tol, d))
        assert e_on <= tol and e_off <= tol and d <= tol, k
