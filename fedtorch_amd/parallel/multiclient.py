# -*- coding: utf-8 -*-
"""Virtual-client packing: C federated clients resident on ONE GPU rank.

The reference can only simulate many clients in its single-process
"centered" mode (`main_centered.py`).  On MI355X, 288 GB HBM3E holds
hundreds of ResNet-class replicas, so the packed mode is first-class: each
rank owns

* one nn.Module + arena for COMPUTE (clients time-share it),
* a ``[C, N]`` replica arena (one flat row per client),
* ``[C, N]`` momentum state (+ per-algorithm aux rows),
* per-client data partitions (global client id = rank*C + j).

A federated round runs each online local client's tau local steps on the
shared module (swap = one ``load_flat`` + momentum view bind), accumulates
the weighted diffs into ONE per-rank partial, and a single world all-reduce
finishes the aggregation — identical math to W*C one-client ranks
(`tests/test_multiclient.py` pins packed(2x2) == flat(4)).
"""
import os
from copy import copy

import torch

from fedtorch_amd import ops

# All online clients' local steps of a round in ONE launch for packed linear
# models (ops.linear_local_rounds, trainings/packed.py).  Opt-in:
# ``FEDTORCH_PACKED_BATCHED=1``; timings in profiles/packed_linear_notes.md.
_BATCHED_ENABLED = os.environ.get('FEDTORCH_PACKED_BATCHED', '0') == '1'
# The same launch for fedprox / scaffold / dense fedgate (the kernel's
# gradient-correction term).  A second opt-in on top of the first:
# ``FEDTORCH_PACKED_BATCHED_CORR=1``.
_BATCHED_CORR_ENABLED = \
    os.environ.get('FEDTORCH_PACKED_BATCHED_CORR', '0') == '1'

# Packed MLP clients: the local steps of all online clients batched per layer
# (ops.mlp_local_rounds, hip/mlpround.h).  Its own opt-in:
# ``FEDTORCH_PACKED_BATCHED_MLP=1``; timings in profiles/packed_mlp_notes.md.
_BATCHED_MLP_ENABLED = \
    os.environ.get('FEDTORCH_PACKED_BATCHED_MLP', '0') == '1'
# The same batched kernels for fedprox / scaffold / dense fedgate (their
# gradient-correction term).  A second opt-in on top of the MLP one:
# ``FEDTORCH_PACKED_BATCHED_MLP_CORR=1``.
_BATCHED_MLP_CORR_ENABLED = \
    os.environ.get('FEDTORCH_PACKED_BATCHED_MLP_CORR', '0') == '1'

# federated types the packed trainer implements
PACKED_TYPES = ('fedavg', 'fedprox', 'scaffold', 'fedgate')


# Packed CNN clients (the LeNet-style `cnn`): the local steps of all online
# clients batched per layer (ops.cnn_local_rounds, hip/cnnround.h).  Its own
# opt-in: ``FEDTORCH_PACKED_BATCHED_CNN=1``; timings in
# profiles/packed_cnn_notes.md.
_BATCHED_CNN_ENABLED = \
    os.environ.get('FEDTORCH_PACKED_BATCHED_CNN', '0') == '1'


class VirtualGraph(object):
    """graph facade so the dataset pipeline partitions over W*C clients."""

    def __init__(self, base, gid, total):
        self.rank = gid
        self.world = list(range(total))
        self.on_cuda = base.on_cuda
        self.blocks = getattr(base, 'blocks', str(total))

    @property
    def n_nodes(self):
        return len(self.world)

    @property
    def ranks(self):
        return list(range(self.n_nodes))

    @property
    def device(self):
        return 0


class ClientPack(object):
    """The C virtual clients of one GPU rank."""

    def __init__(self, client, clients_per_rank):
        """client: an initialized `Client` (model/arena/optimizer built)."""
        self.base = client
        self.args = client.args
        self.C = clients_per_rank
        self.rank = client.args.graph.rank
        self.world = client.args.graph.n_nodes
        self.total_clients = self.world * self.C
        arena = client.arena
        n = arena.numel
        dev = arena.flat.device
        # per-client state resident in HBM
        self.replicas = torch.zeros((self.C, n), device=dev)
        self.in_mom = torch.zeros((self.C, n), device=dev) \
            if client.optimizer.param_groups[0]['in_momentum'] else None
        self.mom_init = [False] * self.C
        # per-algorithm rows: FedGATE's gradient-tracking delta_j, SCAFFOLD's
        # client controls c_j (the server control is
        # client.model_server_control)
        t = getattr(client.args, 'federated_type', None)
        self.delta = torch.zeros((self.C, n), device=dev) \
            if t == 'fedgate' else None
        self.ctrl = torch.zeros((self.C, n), device=dev) \
            if t == 'scaffold' else None
        self.train_loaders = [None] * self.C
        self.partial = torch.zeros(n, device=dev)
        self._stacked = None  # (X, Y, row offsets), see stacked_data()
        # per-client BatchNorm running stats (the reference's centered mode
        # gives every ClientCentered its own module and therefore its own
        # BN buffers; the shared compute module must swap them per client)
        self.bufs = None
        if arena.buf_flat is not None:
            self.bufs = torch.zeros((self.C, arena.buf_flat.numel()),
                                    device=dev)
            for c in range(self.C):
                self.bufs[c].copy_(arena.buf_flat)
        for c in range(self.C):
            self.replicas[c].copy_(arena.flat)

    def global_id(self, j):
        return self.rank * self.C + j

    def build_loaders(self):
        """per-virtual-client data partitions over W*C clients.

        ONE partitioner is built (by the first local client) and shared
        by the rank's other virtual clients — building one per client
        gave every client a DIFFERENT index permutation (only the
        global-client-0 call shuffles before the broadcast), so chunks
        could OVERLAP across virtual clients.  Sharing mirrors the
        centered mode (`main_centered.py:20-25`) and keeps the broadcast
        count identical on every rank (one per rank, at j == 0)."""
        from fedtorch_amd.components.dataset import define_dataset
        per_client_data = self.args.data in ('emnist', 'emnist_full',
                                             'synthetic', 'shakespeare')
        part = None
        for j in range(self.C):
            args_j = copy(self.args)
            args_j.graph = VirtualGraph(self.args.graph, self.global_id(j),
                                        self.total_clients)
            if per_client_data:
                loaders = define_dataset(args_j, shuffle=True, test=False)
            elif part is None:
                loaders, part = define_dataset(args_j, shuffle=True,
                                               test=False,
                                               return_partitioner=True)
            else:
                loaders = define_dataset(args_j, shuffle=True, test=False,
                                         Partitioner=part)
            self.train_loaders[j] = loaders[0]
        # counters derived for the last one apply to all (equal splits)
        self.args.num_batches_train_per_device_per_epoch = \
            len(self.train_loaders[0])

    # ---- batched round of a linear model (trainings/packed.py) --------------
    def linear_layout(self):
        """(w_off, b_off, K, F) of the compute module's single ``fc`` layer
        in the arena, or None when the module is not a plain (non-robust)
        LogisticRegression / LeastSquare."""
        from fedtorch_amd.components.models.convex import (
            LogisticRegression, LeastSquare)
        model, arena = self.base.model, self.base.arena
        if type(model) not in (LogisticRegression, LeastSquare) \
                or model.noise is not None:
            return None
        if sorted(arena.names) != ['fc.bias', 'fc.weight']:
            return None
        w_off = arena.offsets[arena.names.index('fc.weight')]
        b_off = arena.offsets[arena.names.index('fc.bias')]
        K, F = model.fc.weight.shape
        return w_off, b_off, int(K), int(F)

    def batched_blockers(self):
        """Why this pack's rounds cannot run through
        ops.linear_local_rounds: a list of reasons, empty when they can."""
        from fedtorch_amd.components.datasets.device_cache import \
            DeviceCachedLoader
        from fedtorch_amd.components.models.convex import LeastSquare
        args, client = self.args, self.base
        why = []
        if not _BATCHED_ENABLED:
            why.append('FEDTORCH_PACKED_BATCHED is not set')
        layout = self.linear_layout()
        if layout is None:
            why.append('model is not a plain logistic regression / least '
                       'squares')
        why += self._run_blockers(
            self._batched_type_ok(_BATCHED_CORR_ENABLED))
        opt = client.optimizer
        loaders = self.train_loaders
        if not all(isinstance(l, DeviceCachedLoader) and not l._aug
                   for l in loaders):
            why.append('a local loader is not an un-augmented '
                       'DeviceCachedLoader')
        else:
            B = loaders[0].batch_size
            if any(l.batch_size != B for l in loaders):
                why.append('batch sizes differ between clients')
            # the slot loop's `break` on a 1-sample batch is not reproduced
            if any(not l.drop_last and len(l.x) % l.batch_size == 1
                   for l in loaders):
                why.append('a partition leaves a 1-sample last batch')
            if layout is not None:
                _w, _b, K, F = layout
                regress = isinstance(client.model, LeastSquare)
                for l in loaders:
                    if l.x[0].numel() != F:
                        why.append('loader rows do not have %d features' % F)
                        break
                    if not regress and l.y.is_floating_point():
                        why.append('class labels are not integers')
                        break
                mom = opt.param_groups[0]['in_momentum'] != 0 \
                    and bool(getattr(args, 'in_momentum', True))
                need = ops.linear_round_lds_floats(F, K, B, mom)
                if K > ops.LINROUND_MAXK or need > ops.LINROUND_LDS_FLOATS:
                    why.append('F=%d K=%d B=%d needs %d LDS floats (limit %d,'
                               ' K <= %d)' % (F, K, B, need,
                                              ops.LINROUND_LDS_FLOATS,
                                              ops.LINROUND_MAXK))
        return why

    def batched_eligible(self):
        return not self.batched_blockers()

    def _run_blockers(self, type_ok):
        """What every batched path refuses about the run: bf16, a federated
        type the path does not take (`type_ok`), a correction bound on the
        optimizer, the sync type, a growing batch size."""
        args, opt = self.args, self.base.optimizer
        why = []
        if getattr(self.base.arena, 'half_flat', None) is not None \
                or getattr(args, 'bf16', False):
            why.append('bf16 compute')
        if not type_ok:
            why.append('federated_type is not fedavg')
        if getattr(opt, '_prox_mu', 0.0) != 0.0 or any(
                getattr(opt, a, None) is not None
                for a in ('_server', '_ctrl_server', '_ctrl_client',
                          '_delta')):
            why.append('a gradient correction is bound on the optimizer')
        if getattr(args, 'federated_sync_type', None) != 'local_step':
            why.append('federated_sync_type is not local_step')
        if getattr(args, 'growing_batch_size', False):
            why.append('growing_batch_size')
        return why

    def _class_loader_blockers(self, min_b, max_b):
        """What the layer-batched classifier paths (MLP, CNN) refuse about
        the loaders: (reasons, whether every loader is an un-augmented
        DeviceCachedLoader -- only then can its rows be looked at)."""
        from fedtorch_amd.components.datasets.device_cache import \
            DeviceCachedLoader
        loaders = self.train_loaders
        if not all(isinstance(l, DeviceCachedLoader) and not l._aug
                   for l in loaders):
            return ['a local loader is not an un-augmented '
                    'DeviceCachedLoader'], False
        why = []
        B = loaders[0].batch_size
        if any(l.batch_size != B for l in loaders):
            why.append('batch sizes differ between clients')
        elif not min_b <= B <= max_b:
            why.append('batch size %d outside %d .. %d' % (B, min_b, max_b))
        # the slot loop's `break` on a 1-sample batch is not reproduced
        if any(not l.drop_last and len(l.x) % l.batch_size == 1
               for l in loaders):
            why.append('a partition leaves a 1-sample last batch')
        if any(l.y.is_floating_point() for l in loaders):
            why.append('class labels are not integers')
        return why, True

    def _batched_type_ok(self, corr_enabled):
        """fedavg always; fedprox / scaffold / dense fedgate when the path's
        gradient-correction opt-in is on"""
        args = self.args
        t = getattr(args, 'federated_type', None)
        if t == 'fedavg':
            return True
        return corr_enabled and t in ('fedprox', 'scaffold', 'fedgate') \
            and not (getattr(args, 'quantized', False)
                     or getattr(args, 'compressed', False))

    def batched_correction(self):
        """The gradient-correction operands of a batched round
        (ops.linear_local_rounds / ops.mlp_local_rounds) for the pack's
        federated type: what `arm_correction` binds client by client in the
        slot loop, as [C, N] rows."""
        t = getattr(self.args, 'federated_type', None)
        if t == 'fedgate':
            return dict(delta=self.delta)
        if t == 'scaffold':
            return dict(ctrl_server=self.base.model_server_control,
                        ctrl_client=self.ctrl)
        if t == 'fedprox':
            return dict(prox_mu=self.args.fedprox_mu)
        return {}

    # ---- batched round of an MLP (trainings/packed.py) ---------------------
    def mlp_layout(self):
        """The layout ops.mlp_local_rounds takes -- dict(blocks=[(w_off,
        b_off, gamma_off, beta_off, in, out), ...], head=(fc_off, H, K)) --
        of the compute module in the arena, or None when the module is not a
        plain MLP (no noise, BatchNorm on batch statistics, Dropout p = 0)
        whose parameters are exactly the arena's."""
        import torch.nn as nn
        from fedtorch_amd.components.models.mlp import MLP
        model, arena = self.base.model, self.base.arena
        if type(model) is not MLP or model.noise is not None:
            return None
        names = ['fc.weight']
        for i, blk in enumerate(model.layers):
            if len(blk) != 4 or not isinstance(blk[0], nn.Linear) \
                    or not isinstance(blk[1], nn.BatchNorm1d) \
                    or not isinstance(blk[2], nn.ReLU) \
                    or not isinstance(blk[3], nn.Dropout):
                return None
            if blk[1].track_running_stats or not blk[1].affine \
                    or blk[0].bias is None or blk[3].p != 0:
                return None
            names += ['layers.%d.%d.%s' % (i, k, w) for k in (0, 1)
                      for w in ('weight', 'bias')]
        if model.fc.bias is not None or len(model.layers) < 1 \
                or sorted(arena.names) != sorted(names):
            return None
        off = lambda n: arena.offsets[arena.names.index(n)]  # noqa: E731
        blocks = []
        for i, blk in enumerate(model.layers):
            out, fin = blk[0].weight.shape
            blocks.append((off('layers.%d.0.weight' % i),
                           off('layers.%d.0.bias' % i),
                           off('layers.%d.1.weight' % i),
                           off('layers.%d.1.bias' % i), int(fin), int(out)))
        K, H = model.fc.weight.shape
        return dict(blocks=blocks, head=(off('fc.weight'), int(H), int(K)))

    def mlp_eps(self):
        """the eps of the MLP's BatchNorm layers (one value, or None)"""
        eps = set(blk[1].eps for blk in self.base.model.layers)
        return eps.pop() if len(eps) == 1 else None

    def mlp_batched_blockers(self):
        """Why this pack's rounds cannot run through ops.mlp_local_rounds: a
        list of reasons, empty when they can."""
        why = []
        if not _BATCHED_MLP_ENABLED:
            why.append('FEDTORCH_PACKED_BATCHED_MLP is not set')
        layout = self.mlp_layout()
        if layout is None:
            why.append('model is not a plain MLP (no noise, BatchNorm on '
                       'batch statistics, Dropout p = 0) that fills the '
                       'arena')
        elif self.mlp_eps() is None:
            why.append('BatchNorm layers differ in eps')
        why += self._run_blockers(
            self._batched_type_ok(_BATCHED_MLP_CORR_ENABLED))
        reasons, cached = self._class_loader_blockers(2, ops.MLPROUND_MAXB)
        why += reasons
        if cached and layout is not None:
            F = layout['blocks'][0][4]
            if any(l.x[0].numel() != F for l in self.train_loaders):
                why.append('loader rows do not have %d features' % F)
            if layout['head'][2] > ops.MLPROUND_MAXK:
                why.append('K=%d classes (K <= %d)'
                           % (layout['head'][2], ops.MLPROUND_MAXK))
            if len(layout['blocks']) > ops.MLPROUND_MAXL:
                why.append('%d blocks (L <= %d)'
                           % (len(layout['blocks']), ops.MLPROUND_MAXL))
        return why

    def mlp_batched_eligible(self):
        return not self.mlp_batched_blockers()

    # ---- batched round of a CNN (trainings/packed.py) ----------------------
    def cnn_layout(self):
        """The layout ops.cnn_local_rounds takes -- dict(image=(Cin, S),
        conv1 / conv2=(w_off, b_off, C, nhwc), fc1 / fc2=(w_off, b_off, out))
        -- of the compute module in the arena, or None when the module is
        not exactly the LeNet-style CNN whose eight parameters are exactly
        the arena's.  `nhwc`: the arena packs that conv weight in
        channels_last element order (`Arena.cl`)."""
        from fedtorch_amd.components.models.cnn import CNN
        model, arena = self.base.model, self.base.arena
        if type(model) is not CNN:
            return None
        names = ['%s.%s' % (m, w) for m in ('conv1', 'conv2', 'fc1', 'fc2')
                 for w in ('weight', 'bias')]
        if sorted(arena.names) != sorted(names):
            return None
        for conv in (model.conv1, model.conv2):
            if conv.kernel_size != (5, 5) or conv.stride != (1, 1) \
                    or conv.padding != (0, 0) or conv.dilation != (1, 1) \
                    or conv.groups != 1:
                return None
        if model.conv2.in_channels != model.conv1.out_channels \
                or model.fc2.in_features != model.fc1.out_features:
            return None
        Cin, C1, C2 = (model.conv1.in_channels, model.conv1.out_channels,
                       model.conv2.out_channels)
        # the image side from fc1's features C2 * S2^2: S = 4 S2 + 12
        S2 = int(round((model.fc1.in_features / float(C2)) ** .5))
        if C2 * S2 * S2 != model.fc1.in_features or S2 < 1:
            return None
        at = lambda n: arena.names.index(n)  # noqa: E731
        off = lambda n: arena.offsets[at(n)]  # noqa: E731
        return dict(
            image=(int(Cin), 4 * S2 + 12),
            conv1=(off('conv1.weight'), off('conv1.bias'), int(C1),
                   int(bool(arena.cl[at('conv1.weight')]))),
            conv2=(off('conv2.weight'), off('conv2.bias'), int(C2),
                   int(bool(arena.cl[at('conv2.weight')]))),
            fc1=(off('fc1.weight'), off('fc1.bias'),
                 int(model.fc1.out_features)),
            fc2=(off('fc2.weight'), off('fc2.bias'),
                 int(model.fc2.out_features)))

    def cnn_batched_blockers(self):
        """Why this pack's rounds cannot run through ops.cnn_local_rounds: a
        list of reasons, empty when they can."""
        why = []
        if not _BATCHED_CNN_ENABLED:
            why.append('FEDTORCH_PACKED_BATCHED_CNN is not set')
        layout = self.cnn_layout()
        if layout is None:
            why.append('model is not the LeNet-style CNN (5x5 convs, 2x2 '
                       'pools, two Linear layers) that fills the arena')
        why += self._run_blockers(
            getattr(self.args, 'federated_type', None) == 'fedavg')
        reasons, cached = self._class_loader_blockers(1, ops.CNNROUND_MAXB)
        why += reasons
        if cached and layout is not None:
            Cin, S = layout['image']
            F = Cin * S * S
            if any(l.x[0].numel() != F for l in self.train_loaders):
                why.append('loader rows do not have %d features' % F)
            try:
                ops.cnn_layout_check(layout, F, self.base.arena.numel)
            except ValueError as e:
                why.append(str(e))
        return why

    def cnn_batched_eligible(self):
        return not self.cnn_batched_blockers()

    def stacked_data(self):
        """(X [M, F] fp32, Y [M] int32 labels | fp32 targets, offsets [C+1]):
        the clients' cached partitions stacked; client j's rows are
        offsets[j] .. offsets[j+1].  Built once, on first use."""
        if self._stacked is None:
            from fedtorch_amd.components.models.convex import LeastSquare
            regress = isinstance(self.base.model, LeastSquare)
            xs, ys, offs = [], [], [0]
            for l in self.train_loaders:
                xs.append(l.x.reshape(len(l.x), -1).float())
                ys.append(l.y.reshape(-1).float() if regress
                          else l.y.reshape(-1).to(torch.int32))
                offs.append(offs[-1] + len(l.x))
            self._stacked = (torch.cat(xs).contiguous(),
                             torch.cat(ys).contiguous(), offs)
        return self._stacked

    def run_client(self, j, server_flat, local_step_fn):
        """Swap in client j, run its local steps, swap out.
        local_step_fn(loader) -> local_steps performed."""
        client = self.base
        client.arena.load_flat(server_flat)
        if self.bufs is not None:
            client.arena.buf_flat.copy_(self.bufs[j])
        if self.in_mom is not None:
            client.optimizer.bind_state(in_buf=self.in_mom[j],
                                        in_init=self.mom_init[j])
        self.arm_correction(j, server_flat)
        try:
            steps = local_step_fn(self.train_loaders[j])
        finally:
            client.optimizer.clear_correction()
        if self.in_mom is not None:
            self.mom_init[j] = True
        self.replicas[j].copy_(client.arena.flat)
        if self.bufs is not None:
            self.bufs[j].copy_(client.arena.buf_flat)
        return steps

    def arm_correction(self, j, server_flat):
        """Bind client j's per-step gradient correction on the shared
        optimizer (the slot loop; `run_client` clears it afterwards)."""
        t = getattr(self.args, 'federated_type', None)
        opt = self.base.optimizer
        if t == 'fedgate':
            opt.set_correction(delta=self.delta[j])
        elif t == 'scaffold':
            opt.set_correction(ctrl_server=self.base.model_server_control,
                               ctrl_client=self.ctrl[j])
        elif t == 'fedprox':
            opt.set_correction(prox_mu=self.args.fedprox_mu,
                               server=server_flat)

    def partial_buffers(self, online_local, total_online):
        """Write this rank's PRE-SCALED partial of the global BN-stat mean
        (sum over ONLINE local clients / total_online) into the compute
        module's buffer arena.  Zeroed when no local client is online, so
        a plain world all-reduce of the buffer arena yields the mean over
        ALL online clients regardless of how they spread across ranks
        (ranks with more online clients weigh proportionally more)."""
        if self.bufs is None:
            return
        buf = self.base.arena.buf_flat
        if not online_local or total_online <= 0:
            buf.zero_()
            return
        torch.sum(self.bufs[list(online_local)], dim=0, out=buf)
        buf.div_(float(total_online))

    def adopt_buffers(self):
        """After the world-level BN-stat all-reduce every client adopts
        the global mean (mirrors all one-client ranks ending the round
        with identical buffers)."""
        if self.bufs is None:
            return
        self.bufs.copy_(self.base.arena.buf_flat.unsqueeze(0)
                        .expand_as(self.bufs))

    def accumulate_partial(self, server_flat, weights):
        """partial = sum_j weights[j] * (server - replica_j) — ONE batched
        kernel over the [C, N] replica arena; weights: list of per-local-
        client floats (0 for offline)."""
        w = torch.tensor(weights, dtype=torch.float32,
                         device=server_flat.device)
        ops.multi_diff_accumulate(server_flat, self.replicas, w,
                                  self.partial)
        return self.partial

    def _inv_lr_tau(self, weights, taus, lrs, device):
        """[C] fp32: 1 / (lr_j tau_j) of the clients that took part
        (w_j != 0 and tau_j > 0), 0 for the others."""
        return torch.tensor(
            [1.0 / (lr * tau) if w != 0.0 and tau > 0 else 0.0
             for w, tau, lr in zip(weights, taus, lrs)],
            dtype=torch.float32, device=device)

    def update_delta(self, server_flat, agg, weights, taus, lrs):
        """FedGATE: delta_j += (server - agg - y_j) / (lr_j tau_j) for the
        clients that took part; `agg` is the all-reduced partial and
        `server_flat` the server BEFORE the aggregate is applied."""
        ops.multi_delta_update(
            self.delta, server_flat, agg, self.replicas,
            self._inv_lr_tau(weights, taus, lrs, server_flat.device))

    def update_controls(self, server_flat, weights, taus, lrs, out):
        """SCAFFOLD: c_j+ = c_j - c + (server - y_j) / (tau_j lr_j) for the
        clients that took part, out = sum_j w_j (c_j+ - c_j), c_j <- c_j+."""
        dev = server_flat.device
        ops.multi_scaffold_control_update(
            self.ctrl, self.base.model_server_control, server_flat,
            self.replicas, self._inv_lr_tau(weights, taus, lrs, dev),
            torch.tensor(weights, dtype=torch.float32, device=dev), out)
        return out
