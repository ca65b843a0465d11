# -*- coding: utf-8 -*-
"""Packed federated training: C virtual clients per GPU rank
(--clients_per_rank; BASELINE config 5 runs DRFA with 128 virtual clients
on 8 ranks).  Aggregation math is identical to W*C one-client ranks: each
rank reduces its local clients' weighted diffs into ONE partial and a
single world all-reduce finishes the sum.

Algorithms: FedAvg, FedProx, SCAFFOLD and dense FedGATE, each optionally
DRFA lambda-weighted.  With x the server, y_j client j's replica after its
tau_j local steps, lr_j the lr of its last step, w_j its weight:

    partial = sum_j w_j (x - y_j) ; all_reduce ; x -= lr_scale_at_sync * partial
    fedgate   after the all-reduce (d = reduced partial, x before the update):
              delta_j += (x - d - y_j) / (lr_j tau_j)
    scaffold  before it: c_j+ = c_j - c + (x - y_j) / (tau_j lr_j),
              b = sum_j w_j (c_j+ - c_j), c_j <- c_j+ ; [partial | b] travel
              in one 2N all-reduce ; c += b |S| / N_tot
for the clients with w_j != 0 and tau_j > 0; the per-step gradient
corrections are those of `ops.fused_sgd_step`.
"""
import time

import torch

from fedtorch_amd import ops
from fedtorch_amd.components.scheduler import adjust_learning_rate
from fedtorch_amd.components.dataset import load_data_batch
from fedtorch_amd.trainings.flow import (
    get_current_epoch, is_sync_fed)
from fedtorch_amd.trainings.eval import inference
from fedtorch_amd.trainings.federated import amp
from fedtorch_amd.trainings.afl import lambda_dual_update
from fedtorch_amd.aggregation.federated import (
    distribute_model_server, distribute_model_server_control)
from fedtorch_amd.parallel.multiclient import PACKED_TYPES
from fedtorch_amd.logs.logging import log, logging_load_time
from fedtorch_amd.logs.meter import define_local_training_tracker


def _local_steps_fn(client, tracker):
    """Returns a closure running tau local steps on a given loader."""
    args = client.args

    def run(loader):
        steps = 0
        is_sync = False
        while not is_sync:
            for _input, _target in loader:
                steps += 1
                client.model.train()
                logging_load_time(tracker)
                args.local_index += 1
                args.local_data_seen += len(_target)
                get_current_epoch(args)
                adjust_learning_rate(args, client.optimizer,
                                     client.scheduler)
                _input, _target = load_data_batch(args, _input, _target,
                                                  tracker)
                if _input.size(0) == 1:
                    is_sync = is_sync_fed(args)
                    break
                client.optimizer.zero_grad()
                with amp(args):
                    loss, _ = inference(client.model, client.criterion,
                                        client.metrics, _input, _target,
                                        rnn=args.arch == 'rnn')
                loss.backward()
                client.optimizer.step(
                    apply_lr=True, apply_in_momentum=args.in_momentum,
                    apply_out_momentum=False)
                tracker['start_load_time'] = time.time()
                is_sync = is_sync_fed(args)
                if is_sync:
                    break
        return steps
    return run


def _apply_aggregate(client, server_flat, agg):
    """server -= lr_scale_at_sync * agg, with out momentum on the server
    state (one fused kernel)."""
    args = client.args
    g = client.optimizer.param_groups[0]
    out_m = g['out_momentum'] if args.out_momentum else 0.0
    if out_m != 0.0 and 'srv_out_mom' not in client.work:
        client.work['srv_out_mom'] = torch.zeros_like(server_flat)
        client.work['srv_out_init'] = False
    ops.fused_sgd_step(
        server_flat, agg, lr=0.0, scale=args.lr_scale_at_sync,
        weight_decay=0.0, in_momentum=0.0, out_momentum=out_m,
        dampening=0.0, nesterov=False, apply_lr=False,
        apply_in_momentum=False, apply_out_momentum=out_m != 0.0,
        out_buf=client.work.get('srv_out_mom'),
        first_out=out_m != 0.0 and not client.work.get('srv_out_init', True))
    if out_m != 0.0:
        client.work['srv_out_init'] = True


def _plan_local_rounds(client, pack, online):
    """The host's walk of a batched round, shared by the linear and the MLP
    path: the counters exactly as the slot loop moves them, client by client
    and step by step, with no GPU work: local_index, local_data_seen, epoch,
    the scheduled lr and the sync test, pulling each step's rows from the
    loader's index_batches() (a fresh epoch whenever one runs out, like the
    `while` / `for` pair of `_local_steps_fn`).  Returns (plan, idx [C, T, B]
    int32 rows of the stacked data, -1 = padding, lr [C, T], steps [C]) on
    the host; plan[j] is None for an offline client, else its list of
    (rows, lr)."""
    args = client.args
    _X, _Y, offs = pack.stacked_data()
    plan = [None] * pack.C
    for j in range(pack.C):
        if pack.global_id(j) not in online:
            continue
        plan[j] = []
        is_sync = False
        while not is_sync:
            for rows in pack.train_loaders[j].index_batches(device='cpu'):
                args.local_index += 1
                args.local_data_seen += len(rows)
                get_current_epoch(args)
                adjust_learning_rate(args, client.optimizer,
                                     client.scheduler)
                plan[j].append((rows, client.optimizer.param_groups[0]['lr']))
                is_sync = is_sync_fed(args)
                if is_sync:
                    break
    T = max([len(p) for p in plan if p] + [1])
    B = pack.train_loaders[0].batch_size
    idx = torch.full((pack.C, T, B), -1, dtype=torch.int32)
    lr = torch.zeros((pack.C, T), dtype=torch.float32)
    steps = torch.zeros(pack.C, dtype=torch.int32)
    for j, p in enumerate(plan):
        if not p:
            continue
        steps[j] = len(p)
        for s, (rows, lr_s) in enumerate(p):
            idx[j, s, :len(rows)] = rows + offs[j]
            lr[j, s] = lr_s
    return plan, idx, lr, steps


def _batched_local_rounds(client, pack, server, online, snap, k_cut,
                          mlp=False, cnn=False):
    """The local steps of ALL online local clients in one batched op call:
    ops.linear_local_rounds for a linear model (FEDTORCH_PACKED_BATCHED,
    `ClientPack.batched_eligible`), ops.mlp_local_rounds for an MLP
    (`mlp=True`: FEDTORCH_PACKED_BATCHED_MLP,
    `ClientPack.mlp_batched_eligible`), either with the gradient correction
    of the federated type (`ClientPack.batched_correction`);
    ops.cnn_local_rounds for the LeNet-style CNN (`cnn=True`:
    FEDTORCH_PACKED_BATCHED_CNN, `ClientPack.cnn_batched_eligible`, FedAvg
    only).

    The host first walks the counters (`_plan_local_rounds`).  `snap`:
    DRFA's [C, N] snapshot arena, row j receives client j's parameters before
    its step `k_cut`.  Returns (loss [C, T], steps per client, lr of each
    client's last step)."""
    args = client.args
    _X, _Y, _offs = pack.stacked_data()
    plan, idx, lr, steps = _plan_local_rounds(client, pack, online)
    g = client.optimizer.param_groups[0]
    momentum = g['in_momentum'] if args.in_momentum else 0.0
    dev = server.device
    mom_init = torch.tensor([int(b) for b in pack.mom_init],
                            dtype=torch.int32).to(dev)
    operands = (_X, _Y, idx.to(dev), steps.to(dev), lr.to(dev), server,
                pack.replicas, pack.in_mom if momentum != 0 else None,
                mom_init, snap, k_cut)
    sgd = dict(weight_decay=g['weight_decay'], momentum=momentum,
               dampening=g['dampening'], nesterov=g['nesterov'])
    corr = pack.batched_correction()
    if cnn:
        loss = ops.cnn_local_rounds(
            *operands, layout=pack.cnn_layout(),
            wd_numel=client.arena.wd_numel, **sgd)
    elif mlp:
        loss = ops.mlp_local_rounds(
            *operands, layout=pack.mlp_layout(), eps=pack.mlp_eps(),
            wd_numel=client.arena.wd_numel, **sgd, **corr)
    else:
        w_off, b_off, K, _F = pack.linear_layout()
        from fedtorch_amd.components.models.convex import LeastSquare
        loss = ops.linear_local_rounds(
            *operands, w_off=w_off, b_off=b_off, K=K,
            loss_kind=1 if isinstance(client.model, LeastSquare) else 0,
            **sgd, **corr)
    if pack.in_mom is not None:
        for j, p in enumerate(plan):
            if p:
                pack.mom_init[j] = True
    return (loss, [len(p) if p else 0 for p in plan],
            [p[-1][1] if p else 0.0 for p in plan])


def check_packed_supported(args):
    """Raise for what the packed trainer does not implement (it would
    otherwise train plain FedAvg under another algorithm's name)."""
    t = args.federated_type
    if t not in PACKED_TYPES:
        raise ValueError(
            '--federated_type {} is not implemented with --clients_per_rank '
            '> 1; the packed trainer runs {}'.format(
                t, ', '.join(PACKED_TYPES)))
    if t == 'fedgate' and (args.quantized or args.compressed):
        raise ValueError(
            'FedCOMGATE (--federated_type fedgate with --quantized / '
            '--compressed) is not implemented with --clients_per_rank > 1; '
            'pass --quantized false --compressed false for dense FedGATE')


def train_and_validate_federated_packed(client, pack, validate=False):
    """FedAvg / FedProx / SCAFFOLD / dense FedGATE (optionally DRFA
    lambda-weighted) over packed virtual clients."""
    args = client.args
    check_packed_supported(args)
    ftype = args.federated_type
    drfa = args.federated_drfa
    total = pack.total_clients
    log('packed federated training: {} ranks x {} virtual clients'.format(
        args.graph.n_nodes, pack.C), args.debug)
    tracker = define_local_training_tracker()
    tracker['start_load_time'] = time.time()
    server = client.model_server

    if drfa:
        lambda_vector = torch.full((total,), 1.0 / total)
        kth = torch.zeros_like(pack.replicas)
        kth_avg = torch.zeros_like(server)

    step_fn = _local_steps_fn(client, tracker)
    # linear models: one launch for all clients' local steps instead of the
    # slot loop (off unless FEDTORCH_PACKED_BATCHED=1 and the pack qualifies)
    batched = pack.batched_eligible()
    # MLP: the clients' steps batched per layer (off unless
    # FEDTORCH_PACKED_BATCHED_MLP=1 and the pack qualifies)
    batched_mlp = not batched and pack.mlp_batched_eligible()
    # CNN: likewise (off unless FEDTORCH_PACKED_BATCHED_CNN=1 and the pack
    # qualifies)
    batched_cnn = not batched and not batched_mlp \
        and pack.cnn_batched_eligible()
    log('packed local steps: {}'.format(
        'one batched launch per round' if batched
        else 'MLP layers batched over the clients' if batched_mlp
        else 'CNN layers batched over the clients' if batched_cnn
        else 'slot loop'),
        args.debug)
    batched = batched or batched_mlp or batched_cnn
    run_client = (lambda j, server_flat, fn: None) if batched \
        else pack.run_client
    if ftype == 'scaffold':
        ctrl_server = client.model_server_control
        pair = torch.zeros(2 * server.numel(), device=server.device)
    for n_c in range(args.num_comms):
        args.rounds_comm += 1
        args.comm_time.append(0.0)
        online = client.comm.sample_online_global(total)
        if ftype == 'scaffold':
            distribute_model_server_control(client.comm, server, ctrl_server,
                                            client.work)
        else:
            distribute_model_server(client.comm, server)
        if drfa:
            client.comm.broadcast(lambda_vector, src=0)
            k_cut = torch.randint(low=1, high=max(args.local_step, 2),
                                  size=(1,))
            client.comm.broadcast(k_cut, src=0)
            k_cut = int(k_cut[0])

        # weight denominator: DISTRIBUTED semantics — global client 0
        # (the server) counts even when not sampled (`fedavg.py:17-27`,
        # same rule as aggregation/federated.rank_weight)
        n_online = len(online) if 0 in online else len(online) + 1
        n_online = max(n_online, 1)
        weights = []
        taus, lrs = [0] * pack.C, [0.0] * pack.C
        for j in range(pack.C):
            gid = pack.global_id(j)
            if gid in online:
                if drfa:
                    w = float(lambda_vector[gid]) * total / n_online

                    def step_and_snapshot(loader, j=j):
                        steps = 0
                        is_sync = False
                        while not is_sync:
                            for _input, _target in loader:
                                steps += 1
                                if steps == k_cut:
                                    kth[j].copy_(client.arena.flat)
                                client.model.train()
                                args.local_index += 1
                                args.local_data_seen += len(_target)
                                get_current_epoch(args)
                                adjust_learning_rate(
                                    args, client.optimizer, client.scheduler)
                                _input, _target = load_data_batch(
                                    args, _input, _target, tracker)
                                if _input.size(0) == 1:
                                    is_sync = is_sync_fed(args)
                                    break
                                client.optimizer.zero_grad()
                                with amp(args):
                                    loss, _ = inference(
                                        client.model, client.criterion,
                                        client.metrics, _input, _target)
                                loss.backward()
                                client.optimizer.step(
                                    apply_lr=True,
                                    apply_in_momentum=args.in_momentum,
                                    apply_out_momentum=False)
                                is_sync = is_sync_fed(args)
                                if is_sync:
                                    break
                        return steps
                    taus[j] = run_client(j, server, step_and_snapshot)
                else:
                    w = 1.0 / n_online
                    taus[j] = run_client(j, server, step_fn)
                lrs[j] = client.optimizer.param_groups[0]['lr']
            else:
                w = 0.0
            weights.append(w)
        if batched:
            _loss, taus, lrs = _batched_local_rounds(
                client, pack, server, online, kth if drfa else None,
                k_cut if drfa else 0, mlp=batched_mlp, cnn=batched_cnn)

        partial = pack.accumulate_partial(server, weights)
        if ftype == 'scaffold':
            # [partial | weighted control delta] in one 2N all-reduce
            n = server.numel()
            pack.update_controls(server, weights, taus, lrs, pair[n:])
            pair[:n].copy_(partial)
            client.comm.all_reduce(pair)
            partial.copy_(pair[:n])
            # c += sum_j w_j (c_j+ - c_j) |S| / N: sign and factor as in
            # aggregation.federated.scaffold_aggregation
            ctrl_server.add_(pair[n:], alpha=len(online) / total)
        else:
            client.comm.all_reduce(partial)
        if ftype == 'fedgate':
            # before the server moves: delta_j uses the round's own server
            pack.update_delta(server, partial, weights, taus, lrs)
        _apply_aggregate(client, server, partial)
        client.arena.load_flat(server)
        # BN running stats: each rank contributes its pre-scaled partial
        # (sum over its online clients / total online) so the plain world
        # all-reduce gives the mean over ALL online clients even when
        # ranks have unequal online counts; then every client adopts the
        # mean (same end state as W*C one-client ranks)
        online_local = [j for j in range(pack.C)
                        if pack.global_id(j) in online]
        pack.partial_buffers(online_local, len(online))
        from fedtorch_amd.aggregation.federated import aggregate_bn_buffers
        aggregate_bn_buffers(args, client.comm, client.arena,
                             list(range(args.graph.n_nodes)),
                             work=client.work, prescaled=True)
        pack.adopt_buffers()
        for j in range(pack.C):
            # every client re-syncs at round end (its next round reloads
            # the server anyway; keeps replicas bounded in staleness)
            if weights[j] != 0.0:
                pack.replicas[j].copy_(server)

        if drfa:
            # kth average over online clients
            kth_avg.zero_()
            for j in range(pack.C):
                if weights[j] != 0.0:
                    kth_avg.add_(kth[j], alpha=1.0 / n_online)
            client.comm.all_reduce(kth_avg)
            # lambda update on a second sampled set
            online_l = client.comm.sample_online_global(total)
            loss_vec = torch.zeros(total)
            saved = client.arena.clone_flat()
            client.arena.load_flat(kth_avg)
            for j in range(pack.C):
                gid = pack.global_id(j)
                if gid not in online_l:
                    continue
                for _input, _target in pack.train_loaders[j]:
                    _input, _target = load_data_batch(args, _input, _target,
                                                      tracker)
                    if _input.size(0) == 1:
                        break
                    client.model.eval()
                    with torch.no_grad(), amp(args):
                        loss, _ = inference(client.model, client.criterion,
                                            client.metrics, _input, _target)
                    client.model.train()
                    loss_vec[gid] = loss.item() * (total / len(online_l))
                    break
            client.arena.load_flat(saved)
            client.comm.all_reduce(loss_vec)
            if args.graph.rank == 0:
                lambda_vector = lambda_dual_update(
                    args, lambda_vector, loss_vec,
                    step_scale=args.local_step)
        client.comm.flush_comm_time()
        log('packed round {} done (online {} of {}).'.format(
            n_c + 1, len(online), total), args.debug)
