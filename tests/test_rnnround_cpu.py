# -*- coding: utf-8 -*-
"""ops.rnn_local_rounds without a GPU: the eager twin against the real
CharGRU module and FusedSGD.step, the truth table of
ClientPack.rnn_batched_eligible, and the packed trainer's route with the flag
off and on."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import linround_cases as lc
import fedtorch_amd.ops as ops
from fedtorch_amd.components.datasets.device_cache import DeviceCachedLoader
from fedtorch_amd.components.datasets.sources import ArrayDataset
from fedtorch_amd.parallel import multiclient


def _module_rounds(case, dtype, V, H, B):
    """every client's steps on a CharGRU of its own with FusedSGD.step;
    returns (layout, N, wd_numel, replicas, in_mom, hidden, loss)"""
    from fedtorch_amd.components.models.rnn import CharGRU
    from fedtorch_amd.components.optim.sgd import FusedSGD
    from fedtorch_amd.parallel.arena import Arena
    crit = nn.CrossEntropyLoss()
    C, S = case['lr'].shape
    out = None
    for c in range(C):
        torch.manual_seed(11)
        model = CharGRU('shakespeare', V, H, V, B).to(dtype)
        model.init_hidden(B)           # in the module's dtype
        arena = Arena(model, dtype=dtype)
        if out is None:
            off = lambda n: arena.offsets[arena.names.index(n)]  # noqa: E731
            layout = dict(
                encoder=(off('encoder.weight'), V, H),
                w_ih=off('gru.weight_ih_l0'), w_hh=off('gru.weight_hh_l0'),
                b_ih=off('gru.bias_ih_l0'), b_hh=off('gru.bias_hh_l0'),
                decoder=(off('decoder.weight'), off('decoder.bias'), V))
            out = dict(layout=layout, N=arena.numel, wd_numel=arena.wd_numel,
                       server=arena.flat.detach().clone(),
                       replicas=torch.zeros(C, arena.numel, dtype=dtype),
                       in_mom=torch.zeros(C, arena.numel, dtype=dtype),
                       hidden=torch.full((C, B, H), float('nan'),
                                         dtype=dtype),   # rows >= n: open
                       loss=torch.zeros(C, S, dtype=dtype))
        opt = FusedSGD(arena, lr=0.1, in_momentum=0.9, weight_decay=1e-2)
        opt.bind_state(in_buf=out['in_mom'][c], in_init=False)
        model.train()
        for s in range(S):
            rows = case['idx'][c, s]
            rows = rows[rows >= 0].long()
            opt.zero_grad()
            loss = crit(model(case['X'][rows].long()), case['Y'][rows].long())
            loss.backward()
            opt.param_groups[0]['lr'] = float(case['lr'][c, s])
            opt.step(apply_lr=True, apply_in_momentum=True,
                     apply_out_momentum=False)
            out['loss'][c, s] = loss.detach()
        out['replicas'][c] = arena.flat.detach()
        n = model.hidden.size(1)
        out['hidden'][c, :n] = model.hidden[0]
    return out


def test_twin_against_the_chargru_module():
    """two clients, two steps each; client 0's second batch is short (the
    module re-initialises its hidden state), client 1 resumes from h_T.
    Bound: 8 e32 + 16 ulp, e32 the fp32 module's own error against the
    float64 module."""
    V, H, B, T, M = 12, 9, 4, 3, 20
    g = torch.Generator().manual_seed(4)
    idx = torch.full((2, 2, B), -1, dtype=torch.int32)
    for c, ns in enumerate(((B, 3), (B, B))):
        for s, n in enumerate(ns):
            idx[c, s, :n] = torch.randperm(M, generator=g)[:n].int()
    case = dict(X=torch.randint(0, V, (M, T), generator=g, dtype=torch.int32),
                Y=torch.randint(0, V, (M, T), generator=g, dtype=torch.int32),
                idx=idx, lr=.1 + .1 * torch.rand(2, 2, generator=g))
    ref = _module_rounds(case, torch.float64, V, H, B)
    m32 = _module_rounds(case, torch.float32, V, H, B)
    N = ref['N']
    got = dict(replicas=torch.zeros(2, N), in_mom=torch.zeros(2, N),
               hidden=torch.zeros(2, B, H))
    hid_rows = torch.zeros(2, dtype=torch.int32)
    got['loss'] = ops.rnn_local_rounds(
        case['X'], case['Y'], idx, torch.tensor([2, 2], dtype=torch.int32),
        case['lr'], m32['server'], got['replicas'], got['in_mom'],
        torch.zeros(2, dtype=torch.int32), None, 0, got['hidden'], hid_rows,
        layout=ref['layout'], wd_numel=ref['wd_numel'], weight_decay=1e-2,
        momentum=0.9, dampening=0.0, nesterov=False)
    assert hid_rows.tolist() == [3, B]
    for k in ('replicas', 'in_mom', 'hidden', 'loss'):
        e32 = lc.err(m32[k], ref[k])
        tol = lc.bound(e32, ref[k].nan_to_num().abs().max().item())
        assert lc.err(got[k], ref[k]) <= tol, k
    assert lc.err(got['replicas'][0], m32['server']) > 1e-4      # it moved


def _federation(extra=(), arch='rnn', cached=True, batch='30', T='6'):
    os.environ['FEDTORCH_SYNTH_SIZE'] = '400'
    from fedtorch_amd.parameters import get_args
    from fedtorch_amd.nodes import Client
    data = ['-d', 'shakespeare', '--iid_data', 'false'] if arch == 'rnn' \
        else ['-d', 'mnist']
    args = get_args(data + [
        '-a', arch, '--rnn_seq_len', T, '--rnn_hidden_size', '20',
        '-f', 'true', '--federated_type', 'fedavg', '--num_comms', '2',
        '--clients_per_rank', '3', '-b', batch, '--lr', '0.05',
        '--federated_sync_type', 'local_step', '--local_step', '3',
        '--online_client_rate', '1.0', '--in_momentum', 'true',
        '--in_momentum_factor', '0.9', '--weight_decay', '1e-3',
        '--stop_criteria', 'epoch', '--num_epochs', '8',
        '--on_cuda', 'false', '-j', '0', '--manual_seed', '7',
        '--checkpoint', '/tmp/ft_rnnround', '--debug', 'false']
        + list(extra))
    client = Client(args, 0)
    client.initialize()
    client.initialize_dataset()
    client.load_local_dataset()
    client.gen_aux_models()
    pack = multiclient.ClientPack(client, 3)
    pack.build_loaders()
    if cached:
        cache_loaders(pack, 'cpu')
    return client, pack


def cache_loaders(pack, device):
    """the clients' windows in un-augmented DeviceCachedLoaders"""
    for j, old in enumerate(pack.train_loaders):
        part = old.dataset
        ii = torch.as_tensor(list(part.indices))
        pack.train_loaders[j] = DeviceCachedLoader(
            ArrayDataset(part.data.x[ii], part.data.y[ii]), old.batch_size,
            seed=100 + j, shuffle=True, device=device)


def test_rnn_batched_eligible_truth_table(monkeypatch):
    client, pack = _federation()
    assert not pack.rnn_batched_eligible()                  # default OFF
    monkeypatch.setattr(multiclient, '_BATCHED_RNN_ENABLED', True)
    assert pack.rnn_batched_blockers() == [] and pack.rnn_batched_eligible()
    assert not pack.batched_eligible() and not pack.cnn_batched_eligible()
    layout, flat = pack.rnn_layout(), client.arena.flat
    assert layout['encoder'][1:] == (86, 20) and layout['decoder'][2] == 86
    assert flat[layout['w_hh']:].data_ptr() == \
        client.model.gru.weight_hh_l0.data_ptr()
    assert flat[layout['decoder'][1]:].data_ptr() == \
        client.model.decoder.bias.data_ptr()
    # the correction types stay in the slot loop; sync type; bf16
    for extra in (['--federated_type', 'fedprox'],
                  ['--federated_type', 'scaffold'],
                  ['--federated_sync_type', 'epoch'], ['--bf16', 'true']):
        assert not _federation(extra)[1].rnn_batched_eligible(), extra
    assert not _federation(cached=False)[1].rnn_batched_eligible()
    assert not _federation(batch='65')[1].rnn_batched_eligible()
    assert _federation(batch='64')[1].rnn_batched_eligible()
    # 66 windows: a batch of 13 leaves a 1-sample last batch
    assert not _federation(batch='13')[1].rnn_batched_eligible()
    _c, p2 = _federation()
    p2.train_loaders[1].batch_size = 8
    assert not p2.rnn_batched_eligible()
    _c, p3 = _federation()
    p3.train_loaders[2].x = p3.train_loaders[2].x[:, :-1]
    assert not p3.rnn_batched_eligible()
    monkeypatch.setattr(client.model, 'n_layers', 2)
    assert pack.rnn_layout() is None and not pack.rnn_batched_eligible()
    _c, other = _federation(arch='cnn', cached=False, batch='4')
    assert other.rnn_layout() is None and not other.rnn_batched_eligible()


def _train(monkeypatch, flag, veto=False):
    from fedtorch_amd.trainings.packed import \
        train_and_validate_federated_packed
    monkeypatch.setattr(multiclient, '_BATCHED_RNN_ENABLED', flag)
    torch.manual_seed(5)
    np.random.seed(5)
    client, pack = _federation()
    if veto:
        monkeypatch.setattr(pack, 'rnn_batched_eligible', lambda: False)
    calls, real = [], ops.rnn_local_rounds

    def op(*a, **k):
        calls.append([t.clone() if torch.is_tensor(t) else t for t in a])
        return real(*a, **k)
    monkeypatch.setattr(ops, 'rnn_local_rounds', op)
    train_and_validate_federated_packed(client, pack)
    return pack, calls, client.model_server.clone()


def test_flag_off_leaves_a_packed_round_unchanged(monkeypatch):
    """flag off: the slot loop, bit for bit what a pack gives that never
    qualifies; flag on: one op call per round on int32 windows, the short
    last batch of the 66-window partitions (30, 30, 6) inside the steps"""
    off, calls, server = _train(monkeypatch, False)
    assert not calls and off.hidden is None
    never, _calls, server_n = _train(monkeypatch, True, veto=True)
    assert torch.equal(off.replicas, never.replicas)
    assert torch.equal(off.in_mom, never.in_mom)
    assert torch.equal(server, server_n)
    on, calls, server_on = _train(monkeypatch, True)
    assert len(calls) == 2
    X, Y, idx, steps = calls[0][:4]
    assert X.dtype == Y.dtype == torch.int32 and X.shape == Y.shape == (198, 6)
    assert idx.shape == (3, 3, 30) and steps.tolist() == [3, 3, 3]
    assert (idx >= 0).sum(2).tolist() == [[30, 30, 6]] * 3
    assert calls[1][12].tolist() == [6, 6, 6]       # hid_rows after round 1
    assert on.hid_rows.tolist() == [6, 6, 6] and on.mom_init == [True] * 3
    assert torch.isfinite(server_on).all()
    assert (server_on - server).abs().max() < 0.05  # up to the hidden state
