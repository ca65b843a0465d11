# -*- coding: utf-8 -*-
"""Infra tests: checkpoint layout + resume, growing-batch sampler, flow
bookkeeping, tools parsers."""
import os
import types

import numpy as np
import torch

from fedtorch_amd.components.dataset import GrowingMinibatchSampler
from fedtorch_amd.trainings import flow


def test_growing_minibatch_sampler():
    data = list(range(1000))
    s = GrowingMinibatchSampler(data, num_epochs=3, base_batch_size=2,
                                rho=1.05, max_batch_size=64)
    batches = list(iter(s))
    sizes = [len(b) for b in batches]
    assert sizes[0] == 3  # int(2*1.05^0)+1
    assert all(a <= max(b, 64) for a, b in zip(sizes, sizes[1:] + [64]))
    assert max(sizes) <= 64
    # pool can run dry before the nominal iteration count (reference
    # semantics: batch list precomputed, pool sliced until empty)
    assert 0 < len(batches) <= s.num_iterations
    # consuming the sampler twice yields the same batches (idx_pool kept)
    batches2 = list(iter(s))
    assert [len(b) for b in batches2] == sizes


def _flow_args(**kw):
    base = dict(growing_batch_size=False, local_index=0, local_data_seen=0,
                num_batches_train_per_device_per_epoch=10,
                num_samples_per_epoch=100, stop_criteria='epoch',
                num_epochs=2, num_iterations_per_worker=50,
                federated_sync_type='epoch', num_epochs_per_comm=1,
                local_steps=[4] * 5, epoch=0, epoch_=0.0,
                client_epoch_total=0)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_flow_epoch_and_sync():
    a = _flow_args(local_index=25)
    flow.get_current_epoch(a)
    assert a.epoch_ == 2.5 and a.epoch == 2
    assert flow.get_current_local_step(a) == 4
    a.epoch = 99  # falls back to last entry
    assert flow.get_current_local_step(a) == 4
    assert flow.is_stop(a)

    a = _flow_args(federated_sync_type='local_step', local_index=8)
    assert flow.is_sync_fed(a)
    a.local_index = 7
    assert not flow.is_sync_fed(a)


def test_checkpoint_roundtrip(tmp_path, tiny_args):
    import torch.nn as nn
    from fedtorch_amd.logs.checkpoint import (
        init_checkpoint, save_to_checkpoint, maybe_resume_from_checkpoint)
    from fedtorch_amd.parallel.arena import Arena
    from fedtorch_amd.components.optim.sgd import FusedSGD

    args = tiny_args
    args.checkpoint = str(tmp_path)
    args.graph = types.SimpleNamespace(rank=0)
    args.debug = True
    args.timestamp = 'testrun'
    init_checkpoint(args)
    assert args.checkpoint_root.endswith('testrun')
    assert args.checkpoint_dir.endswith('testrun/0')

    torch.manual_seed(0)
    model = nn.Linear(5, 2)
    arena = Arena(model)
    opt = FusedSGD(arena, lr=0.1, in_momentum=0.9)
    g = torch.randn_like(arena.grad)
    opt.step(grad=g)
    args.best_epoch = [1.0]
    state = {'arguments': args, 'current_epoch': 1, 'local_index': 7,
             'global_index': 2, 'arch': 'x',
             'state_dict': model.state_dict(),
             'optimizer': opt.state_dict(), 'best_prec1': 55.0}
    save_to_checkpoint(state, True, dirname=args.checkpoint_root,
                       filename='checkpoint.pth.tar', save_all=False)
    assert os.path.exists(os.path.join(args.checkpoint_root,
                                       'checkpoint.pth.tar'))
    assert os.path.exists(os.path.join(args.checkpoint_root,
                                       'model_best.pth.tar'))

    # resume into a fresh model
    torch.manual_seed(1)
    model2 = nn.Linear(5, 2)
    arena2 = Arena(model2)
    opt2 = FusedSGD(arena2, lr=0.1, in_momentum=0.9)
    args2 = types.SimpleNamespace(
        resume=args.checkpoint_root, checkpoint_index=None,
        data=args.data, batch_size=args.batch_size,
        num_epochs=args.num_epochs,
        graph=types.SimpleNamespace(rank=0), best_epoch=[], local_index=0,
        best_prec1=0)
    maybe_resume_from_checkpoint(args2, model2, opt2)
    assert args2.local_index == 7
    assert args2.best_prec1 == 55.0
    assert torch.equal(model2.weight.data, model.weight.data)
    assert torch.allclose(opt2._in_buf, opt._in_buf)


def test_tools_parse_roundtrip(tmp_path):
    from fedtorch_amd.tools.load_console_records import (
        parse_record_for_test, parse_record_for_train, PAT_COMM)
    rec = tmp_path / 'record0'
    rec.write_text(
        '2026:09:13 10:00:00\tTest at batch: 12. Epoch: 1. Process: 0. '
        'Prec@1: 55.000 Prec@5: 90.000 Loss: 1.234 Comm: 3\n'
        '2026:09:13 10:00:05\tTest at batch: 24. Epoch: 2. Process: 0. '
        'Prec@1: 60.000 Prec@5: 92.000 Loss: 1.100 Comm: 4\n'
        '2026:09:13 10:00:06\tThis round communication time is: 0.125\n')
    df = parse_record_for_test(str(rec))
    assert len(df) == 2
    assert df['top1'].tolist() == [55.0, 60.0]
    assert df['time'].tolist() == [0.0, 5.0]


def test_bench_two_rank_cpu_contract():
    """The driver launches bench.py via torchrun with N ranks; verify the
    multi-rank path (gloo on CPU) emits the contract JSON from rank 0."""
    import json
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT='29881')
    out = subprocess.run(
        [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1',
         '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
         '--master-port', '29882', os.path.join(repo, 'bench.py'),
         '--gpus', '2', '--steps', '12', '--warmup', '2', '--batch', '16'],
        capture_output=True, text=True, timeout=600, cwd=repo, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, lines  # rank 0 only
    d = json.loads(lines[0])
    assert d['n_gpus'] == 2
    assert d['config']['global_batch'] == 32
    assert d['value'] > 0


def test_bench_dump_outputs_repeatable_cpu(tmp_path):
    """`--dump-outputs DIR` writes the state the last timed step left as
    fp32 .npy files; the same arguments give the same inputs, so two runs
    dump the same arrays (bit-exact on CPU).  `--steps` sets the number of
    timed steps, `ms_per_step` is reported, `--full` is accepted."""
    import json
    import os
    import subprocess
    import sys
    import numpy as np
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dumps = []
    for tag, extra in (('a', []), ('b', ['--full'])):
        dump = str(tmp_path / tag)
        out = subprocess.run(
            [sys.executable, os.path.join(repo, 'bench.py'), '--gpus', '1',
             '--steps', '11', '--warmup', '1', '--batch', '8',
             '--dump-outputs', dump] + extra,
            capture_output=True, text=True, timeout=600, cwd=repo)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
        assert len(lines) == 1, lines
        d = json.loads(lines[0])
        assert d['steps'] == 11
        assert d['ms_per_step'] > 0
        assert abs(d['value'] * d['ms_per_step'] - 8e3) < 8.0
        dumps.append({n: np.load(os.path.join(dump, n))
                      for n in sorted(os.listdir(dump))})
    a, b = dumps
    assert sorted(a) == ['bn_running_stats.npy', 'loss.npy', 'momentum.npy',
                         'params.npy']
    assert sorted(b) == sorted(a)
    for n in a:
        assert a[n].dtype == np.float32 and np.isfinite(a[n]).all(), n
        assert np.array_equal(a[n], b[n]), n
    assert np.abs(a['momentum.npy']).max() > 0  # training really stepped


def test_accuracy_and_per_class_oracle():
    """metrics vs hand-computed values (reference `metrics.py:50-91`)."""
    import torch
    from fedtorch_amd.components.metrics import accuracy, accuracy_per_class
    logits = torch.tensor([[0.9, 0.1, 0.0],
                           [0.1, 0.8, 0.1],
                           [0.2, 0.7, 0.1],
                           [0.3, 0.3, 0.4]])
    target = torch.tensor([0, 1, 0, 2])
    top1, top2 = accuracy(logits, target, topk=(1, 2))
    assert abs(top1 - 75.0) < 1e-5      # 3 of 4 correct
    assert abs(top2 - 100.0) < 1e-5     # sample 2's true class is 2nd
    acc, count = accuracy_per_class(logits, target, torch.tensor([0, 1, 2]))
    assert count.tolist() == [2.0, 1.0, 1.0]
    assert abs(acc[0].item() - 50.0) < 1e-4   # one of the two 0s right
    assert abs(acc[1].item() - 100.0) < 1e-4
    assert abs(acc[2].item() - 100.0) < 1e-4
    # rnn mode: argmax over flattened (seq) predictions
    r = accuracy(logits, target, topk=(1,), rnn=True)
    assert abs(r[0] - 75.0) < 1e-5


def test_checkpoint_best_and_epoch_copies(tmp_path):
    """save_to_checkpoint produces model_best + per-epoch copies exactly as
    the reference layout (`logs/checkpoint.py:68-82`)."""
    import os
    import torch
    from types import SimpleNamespace
    from fedtorch_amd.logs.checkpoint import save_to_checkpoint
    d = str(tmp_path / 'ck')
    args = SimpleNamespace(save_some_models=['2'])
    state = {'arguments': args, 'current_epoch': 1,
             'state_dict': {'w': torch.zeros(2)}, 'best_prec1': 10.0}
    save_to_checkpoint(state, True, d, 'checkpoint.pth.tar')
    assert os.path.exists(os.path.join(d, 'checkpoint.pth.tar'))
    assert os.path.exists(os.path.join(d, 'model_best.pth.tar'))
    assert not os.path.exists(os.path.join(d, 'checkpoint_epoch_1.pth.tar'))
    state['current_epoch'] = 2
    save_to_checkpoint(state, False, d, 'checkpoint.pth.tar')
    assert os.path.exists(os.path.join(d, 'checkpoint_epoch_2.pth.tar'))
    state['current_epoch'] = 3
    save_to_checkpoint(state, False, d, 'checkpoint.pth.tar', save_all=True)
    assert os.path.exists(os.path.join(d, 'checkpoint_epoch_3.pth.tar'))


def test_run_dist_command_mapping(capsys):
    """run_dist maps the reference's short flags (`run_mpi.py:25-105`) onto
    a torchrun command with the full parameter list."""
    import shlex
    from types import SimpleNamespace
    import run_dist
    ns = SimpleNamespace(
        num_epochs_per_comm=1, num_clients=4, dataset='cifar10',
        data_path='./data', batch_size=50, num_comms=3, lr_gamma=0.1,
        lr_mu=1, lr_sync=1.0, weight_decay=1e-4, iid=False, local_steps=10,
        on_cuda=False, federated=True, federated_type='fedgate',
        federated_drfa=False, drfa_gamma=0.1,
        federated_sync_type='local_step', online_client_rate=0.5,
        num_class_per_client=2, synthetic_params=[0.0, 0.0], quantized=True,
        compressed=False, compressed_ratio=1.0, unbalanced=False,
        fed_personal=False, fed_personal_alpha=0.0, fed_adaptive_alpha=False,
        sensitive_feature=9, quantized_bits=8, fedprox_mu=0.002, arch=None,
        tmp_dir='/tmp', bf16=False, master_port=29911, dry_run=True)
    assert run_dist.main(ns) == 0
    out = capsys.readouterr().out
    cmd = shlex.split(out.split('Running:\n', 1)[1].splitlines()[0])
    assert cmd[cmd.index('--nproc-per-node') + 1] == '4'
    joined = ' '.join(cmd)
    assert '--federated_type fedgate' in joined
    assert '--quantized True' in joined
    assert '--online_client_rate 0.5' in joined
    assert '--num_class_per_client 2' in joined
    assert '--local_step 10' in joined
    assert 'fedtorch_amd.main' in joined


def test_bench_four_rank_cpu_contract_with_settle():
    """8-GPU readiness: the driver may launch
    `torchrun --nproc-per-node 8 bench.py --gpus 8`.  Exercise the
    multi-rank path at world 4 on gloo INCLUDING the collective settle
    loop (all ranks must agree on the number of settle rounds or the
    sync collectives deadlock)."""
    import json
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT='29885',
               FEDTORCH_FORCE_SETTLE='1')
    out = subprocess.run(
        [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1',
         '--nproc-per-node', '4', '--master-addr', '127.0.0.1',
         '--master-port', '29886', os.path.join(repo, 'bench.py'),
         '--gpus', '4', '--steps', '10', '--warmup', '1', '--batch', '8'],
        capture_output=True, text=True, timeout=900, cwd=repo, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d['n_gpus'] == 4
    assert d['config']['global_batch'] == 32
    assert d['config']['parallelism'] == 'fedavg_dp4_tau10'
    assert d['value'] > 0


def test_reference_flag_surface_complete():
    """Every flag the reference's get_args defines exists in ours (the
    north star requires keeping the Client/get_args() surface).  The
    list is the reference `parameters.py` add_argument inventory
    (103 unique names), frozen here so the guard runs without the
    reference checkout."""
    REF_FLAGS = """avg_model base_batch_size blocks check_model_at_sync checkpoint checkpoint_index
    compressed compressed_ratio correct_wd debug densenet_bc_mode densenet_compression
    densenet_growth_rate dirichlet dist_backend drfa_gamma drop_rate eval_freq
    experiment fed_adaptive_alpha fed_personal fed_personal_alpha fed_personal_test fedadam_beta
    fedadam_tau federated_drfa federated_sync_type federated_type fedprox_mu growing_batch_size
    hostfile iid_data in_momentum in_momentum_factor is_distributed local_step
    local_step_warmup_per_interval local_step_warmup_period local_step_warmup_type log_dir lr lr_alpha
    lr_change_epochs lr_decay lr_fields lr_gamma lr_mu lr_onecycle_extra_low
    lr_onecycle_high lr_onecycle_low lr_onecycle_num_epoch lr_scale_at_sync lr_scale_indicators lr_scaleup
    lr_scaleup_type lr_schedule_scheme lr_warmup lr_warmup_epochs manual_seed max_batch_size
    mlp_hidden_size mlp_num_layers num_class_per_client num_comms num_epochs num_epochs_per_comm
    num_iterations on_cuda online_client_rate optimizer out_momentum out_momentum_factor
    partition_data per_class_acc perfedavg_beta perfedme_lambda pin_memory plot_dir
    pretrained qffl_q quantized quantized_bits reshuffle_per_epoch resume
    rnn_hidden_size rnn_seq_len save_all_models save_some_models sensitive_feature stop_criteria
    summary_freq synthetic_alpha synthetic_beta timestamp track_model_aggregation turn_off_local_step_from
    turn_on_local_step_from unbalanced use_nesterov vocab_size weight_decay wideresnet_widen_factor
    world""".split()
    from fedtorch_amd.parameters import get_args
    args = get_args(['-d', 'mnist', '-a', 'mlp', '--checkpoint', '/tmp/x'])
    ours = set(vars(args).keys())
    missing = sorted(set(REF_FLAGS) - ours)
    assert not missing, 'reference flags missing: %s' % missing


def test_client_api_surface():
    """The north star pins the reference's public Client API
    (README.md:59-71: initialize / initialize_dataset /
    load_local_dataset / gen_aux_models) and get_args."""
    from fedtorch_amd.nodes import Client
    from fedtorch_amd import parameters
    for m in ('initialize', 'initialize_dataset', 'load_local_dataset',
              'gen_aux_models'):
        assert callable(getattr(Client, m, None)), m
    assert callable(parameters.get_args)
    from fedtorch_amd.trainings.federated import train_and_validate_federated
    from fedtorch_amd.trainings.local_sgd import train_and_validate
    from fedtorch_amd.trainings.drfa import (
        train_and_validate_federated_drfa)
    from fedtorch_amd.trainings.apfl import (
        train_and_validate_federated_apfl)
    from fedtorch_amd.trainings.afl import train_and_validate_federated_afl
    assert all(callable(f) for f in (
        train_and_validate_federated, train_and_validate,
        train_and_validate_federated_drfa, train_and_validate_federated_apfl,
        train_and_validate_federated_afl))
