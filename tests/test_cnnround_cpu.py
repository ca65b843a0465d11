# -*- coding: utf-8 -*-
"""ops.cnn_local_rounds without a GPU: the float64 replay of
cnnround_cases.py against float64 autograd through the real CNN module and
the fused optimizer, the eager twin against the replay, untouched rows and
pad gaps, the twin's errors, the pool tie rule, the eligibility rules of
ClientPack.cnn_batched_eligible, and a packed CNN federation trained once
through the slot loop and once through the batched round, both against a
float64 replay."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import linround_cases as lc
import cnnround_cases as cc
import fedtorch_amd.ops as ops
from fedtorch_amd.components.datasets.device_cache import DeviceCachedLoader
from fedtorch_amd.parallel import multiclient

F32, F64 = torch.float32, torch.float64


def _assert_bounded(got, ref, e32, label=''):
    assert torch.equal(got['mom_init'].cpu(), ref['mom_init'])
    for k in cc.OUTPUTS:
        if ref[k] is None:
            assert got[k] is None or got[k].numel() == 0
            continue
        assert lc.same_nan_pattern(got[k], ref[k]), k
        e, tol = lc.err(got[k], ref[k]), lc.bound(e32[k], cc.scale_of(ref[k]))
        print('%s %s: err %.3e  e32 %.3e  err/e32 %.2f  err/tol %.3f'
              % (label, k, e, e32[k], e / e32[k] if e32[k] else 0.0, e / tol))
        assert e <= tol, (k, e, tol)


# --------------------------------------------------------------------------
# the reference against the real module in float64
# --------------------------------------------------------------------------
def _pack_layout(arena):
    at = lambda n: arena.names.index(n)  # noqa: E731
    off = lambda n: arena.offsets[at(n)]  # noqa: E731
    m = arena.module
    return dict(
        image=(m.conv1.in_channels, 28 if m.conv1.in_channels == 1 else 32),
        conv1=(off('conv1.weight'), off('conv1.bias'), 20,
               int(arena.cl[at('conv1.weight')])),
        conv2=(off('conv2.weight'), off('conv2.bias'), 50,
               int(arena.cl[at('conv2.weight')])),
        fc1=(off('fc1.weight'), off('fc1.bias'), 512),
        fc2=(off('fc2.weight'), off('fc2.bias'), m.num_classes))


@pytest.mark.parametrize('data,channels_last', [('mnist', False),
                                                ('mnist', True),
                                                ('cifar10', True)])
def test_reference_against_float64_autograd_of_the_module(data,
                                                          channels_last):
    """the hand-written backward, the pool rule and both weight orders:
    float64 autograd through CNN.forward with FusedSGD.step on a float64
    arena must agree with the float64 replay to rounding"""
    from fedtorch_amd.components.models.cnn import CNN
    from fedtorch_amd.components.optim.sgd import FusedSGD
    from fedtorch_amd.parallel.arena import Arena
    torch.manual_seed(3)
    model = CNN(data).double()
    if channels_last:
        model = model.to(memory_format=torch.channels_last)
    arena = Arena(model, dtype=F64)
    layout = _pack_layout(arena)
    assert layout['conv2'][3] == int(channels_last)
    assert layout['conv1'][3] == int(channels_last and data == 'cifar10')
    g = lc.gen('cnn-module', data, channels_last)
    steps = [2, 0]
    case = cc.make_case(g, None, 3, steps, 9, m=0.9, layout=layout,
                        N=arena.numel, short=(0, 1, 2), mom_init=[0, 1])
    gap = cc.gap_mask(layout, arena.numel)
    case['server'][gap] = 0
    case['in_mom'][:, gap] = 0
    lr = torch.rand(2, 2, generator=g) * .05 + .01
    hp = dict(wd=5e-4, m=0.9, damp=0.0, nesterov=True)
    ref = cc.run_ref(case, lr, 0, hp, None, arena.wd_numel)

    opt = FusedSGD(arena, lr=0.1, in_momentum=0.9, weight_decay=hp['wd'],
                   nesterov=True)
    crit = nn.CrossEntropyLoss()
    Cin, S = layout['image']
    in_mom = case['in_mom'].double()
    arena.load_flat(case['server'].double())
    opt.bind_state(in_buf=in_mom[0], in_init=False)
    model.train()
    for s in range(2):
        rows = case['idx'][0, s]
        rows = rows[rows >= 0].long()
        opt.zero_grad()
        x = case['X'][rows].double().view(-1, Cin, S, S)
        loss = crit(model(x), case['Y'][rows].long())
        loss.backward()
        opt.param_groups[0]['lr'] = float(lr[0, s])
        opt.step(apply_lr=True, apply_in_momentum=True,
                 apply_out_momentum=False)
        assert abs(loss.item() - ref['loss'][0, s].item()) < 1e-12
    scale = ref['replicas'][0].abs().max().item()
    assert lc.err(arena.flat, ref['replicas'][0]) < 1e-13 * max(scale, 1)
    assert lc.err(in_mom[0], ref['in_mom'][0]) < 1e-13
    assert lc.err(arena.flat, case['server'].double()) > 1e-4   # it moved


def test_pool_tie_goes_to_the_first_maximum():
    """a hand-made window with equal positive entries: the gradient goes to
    the first maximal element in scan order, as in F.max_pool2d's backward;
    a window whose maximum is <= 0 passes nothing"""
    z = torch.tensor([[[[1., 3., -1., 0.],
                        [3., 3., 0., -2.],
                        [2., 2., 5., 5.],
                        [2., 7., 5., 1.]]]], dtype=F64)
    p, k, on = cc.relu_pool(z)
    assert p.tolist() == [[[[3., 0.], [7., 5.]]]]
    assert k.tolist() == [[[[1, 1], [3, 0]]]]
    assert on.tolist() == [[[[True, False], [True, True]]]]
    dp = torch.tensor([[[[10., 20.], [30., 40.]]]], dtype=F64)
    dz = cc.relu_pool_bwd(dp, k, on)
    zt = z.clone().requires_grad_(True)
    torch.nn.functional.max_pool2d(torch.relu(zt), 2, 2).backward(dp)
    assert torch.equal(dz, zt.grad)
    assert dz.tolist() == [[[[0., 10., 0., 0.], [0., 0., 0., 0.],
                             [0., 0., 40., 0.], [0., 30., 0., 0.]]]]


# --------------------------------------------------------------------------
# the eager twin against the float64 replay
# --------------------------------------------------------------------------
@pytest.mark.parametrize('geo', cc.SHAPES)
def test_twin_against_float64_replay(geo):
    case, lr, k_cut, hp, snap, wd_numel, ref, e32 = cc.case(geo)
    got = cc.call_op(ops, case, lr, k_cut, hp, snap, wd_numel)
    _assert_bounded(got, ref, e32, str(geo))
    steps = case['steps'].tolist()
    for c in range(len(steps)):                 # snap: only when k_cut is due
        written = not bool(torch.isnan(got['snap'][c]).any())
        assert written == (1 <= k_cut <= steps[c]), (c, k_cut, steps[c])
    for c, ns in enumerate(steps):
        assert not got['loss'][c, ns:].any() and (got['loss'][c, :ns] > 0).all()


def test_case_set_covers_the_edges():
    ks = {g: cc.case(g) for g in cc.SHAPES}
    sm, mid, st = ks[cc.SMALL], ks[cc.MID], ks[cc.STOCK]
    for k in (sm, mid):
        assert k[0]['steps'].tolist() == [3, 0, 2]
        valid = sorted({int((k[0]['idx'][c, s] >= 0).sum())
                        for c in (0, 2) for s in range(k[0]['steps'][c])})
        assert valid == [1, 3, 5]              # one row, short, full
        assert len(set(k[1][0].tolist())) == 3                  # lr changes
    assert st[0]['steps'].tolist() == [0, 2] and st[0]['idx'].shape[2] == 3
    assert [k[3]['m'] for k in (sm, mid, st)] == [0.0, 0.9, 0.9]
    assert [k[3]['nesterov'] for k in (sm, mid, st)] == [False, True, False]
    assert mid[5] < mid[0]['N'] and st[5] == st[0]['N']        # wd prefix
    assert mid[0]['mom_init'].tolist() == [0, 1, 1]
    assert sm[2] == 3 and mid[2] == 2          # inside c0 / beyond c2; inside
    assert mid[0]['layout']['conv1'][3] == mid[0]['layout']['conv2'][3] == 1
    assert sm[0]['layout']['conv2'][3] == 0 and st[0]['layout']['conv2'][3]
    assert cc.dims(sm[0]['layout'])[6:8] == (6, 1)
    assert cc.dims(mid[0]['layout'])[6:8] == (8, 2)
    assert cc.MARGIN == 64.0


def test_weight_orders_agree():
    """the mid case in [co][ci][kh][kw] order gives the nhwc case's result,
    element for element (reference and twin)"""
    case, lr, k_cut, hp, snap, wd_numel, ref, e32 = cc.case(cc.MID)
    layout, index = cc.reorder_index(case['layout'], (0, 0))
    plain = dict(case, layout=layout, server=case['server'][index],
                 in_mom=case['in_mom'][:, index])
    # wd_numel cuts fc1's weight, behind both conv weights: the same prefix
    ref_p = cc.run_ref(plain, lr, k_cut, hp, snap, wd_numel)
    for k in ('replicas', 'in_mom', 'snap'):
        assert lc.same_nan_pattern(ref_p[k], ref[k][:, index])
        assert lc.err(ref_p[k], ref[k][:, index]) < 1e-13
    got = cc.call_op(ops, plain, lr, k_cut, hp, snap, wd_numel)
    for k in ('replicas', 'in_mom', 'snap'):
        tol = lc.bound(e32[k], cc.scale_of(ref[k]))
        assert lc.err(got[k], ref[k][:, index]) <= tol, k


# --------------------------------------------------------------------------
# what must stay untouched
# --------------------------------------------------------------------------
def test_offline_rows_and_pad_gaps_bit_untouched():
    case, lr, k_cut, hp, snap, wd_numel, _ref, _e = cc.case(cc.MID)
    got = cc.call_op(ops, case, lr, k_cut, hp, snap, wd_numel)
    assert torch.isnan(got['replicas'][1]).all()
    assert torch.isnan(got['snap'][1]).all()
    assert torch.equal(got['in_mom'][1], case['in_mom'][1])
    assert case['mom_init'].tolist() == [0, 1, 1]
    assert got['mom_init'].tolist() == [1, 1, 1]
    assert not got['loss'][1].any()
    gap = cc.gap_mask(case['layout'], case['N'])
    assert gap.sum() > 64
    for c in (0, 2):
        assert torch.equal(got['replicas'][c][gap], case['server'][gap])
        assert torch.equal(got['in_mom'][c][gap], case['in_mom'][c][gap])
        assert not torch.equal(got['in_mom'][c][~gap],
                               case['in_mom'][c][~gap])
    assert torch.equal(got['snap'][0][gap], case['server'][gap])
    # without momentum neither in_mom nor mom_init is touched
    case, lr, k_cut, hp, snap, wd_numel, _ref, _e = cc.case(cc.SMALL)
    got = cc.call_op(ops, case, lr, k_cut, hp, snap, wd_numel)
    assert got['in_mom'] is None and got['mom_init'].tolist() == [0, 0, 0]


# --------------------------------------------------------------------------
# the twin's errors
# --------------------------------------------------------------------------
def _twin_raises(match, mutate, geo=cc.SMALL):
    case, lr, k_cut, hp, snap, wd_numel, _ref, _e = cc.case(geo)
    case = dict(case, idx=case['idx'].clone(), layout=dict(case['layout']))
    args = dict(lr=lr, k_cut=k_cut, wd_numel=wd_numel, hp=dict(hp),
                snap=snap)
    mutate(case, args)
    with pytest.raises(ValueError, match=match):
        cc.call_op(ops, case, args['lr'], args['k_cut'], args['hp'],
                   args['snap'], args['wd_numel'])


def test_twin_raises_on_empty_steps_bad_layouts_and_limits():
    def empty(case, a):
        case['idx'][2, 1, :] = -1
    _twin_raises('has no sample', empty)

    def lay(key, i, v):
        def mutate(case, a):
            t = list(case['layout'][key])
            t[i] = v
            case['layout'][key] = tuple(t)
        return mutate
    _twin_raises('overlap', lay('conv1', 1, 64))      # bias inside the weight
    _twin_raises('does not fit', lay('fc2', 0, 10 ** 6))
    _twin_raises('does not fit', lay('conv2', 0, -1))
    _twin_raises('X has 256 features', lay('image', 0, 2))
    _twin_raises('does not pool evenly', lay('image', 1, 18))
    _twin_raises('does not pool evenly', lay('image', 1, 12))   # S2 = 0
    _twin_raises('unsupported image', lay('image', 1, 36))
    _twin_raises('unsupported image', lay('image', 0, 5))
    _twin_raises('unsupported C1=25', lay('conv1', 2, 25))
    _twin_raises('unsupported C1=3 C2=65', lay('conv2', 2, 65))
    _twin_raises('H=4097', lay('fc1', 2, 4097))
    _twin_raises('unsupported K=129', lay('fc2', 2, 129))
    _twin_raises('nhwc flag', lay('conv2', 3, 2))
    _twin_raises('a layout is', lambda case, a: case['layout'].__setitem__(
        'fc1', case['layout']['fc1'][:2]))
    _twin_raises('k_cut', lambda case, a: a.__setitem__('k_cut', -1))
    _twin_raises('wd_numel', lambda case, a: a.__setitem__(
        'wd_numel', case['N'] + 1))
    _twin_raises('steps holds',
                 lambda case, a: case.__setitem__('steps', case['steps'] + 9))
    _twin_raises('idx holds row', lambda case, a: case['idx'].__setitem__(
        (0, 0, 0), case['X'].shape[0]))
    _twin_raises('unsupported B=80', lambda case, a: case.__setitem__(
        'idx', torch.cat([case['idx']] * 16, 2).contiguous()))
    _twin_raises('lr must be', lambda case, a: a.__setitem__(
        'lr', a['lr'].double()))
    _twin_raises('Y must be', lambda case, a: case.__setitem__(
        'Y', case['Y'].long()))
    # the launcher's rules about the optimizer and the optional operands
    _twin_raises('nesterov needs', lambda case, a: a['hp'].update(
        nesterov=True))                               # small: no momentum
    _twin_raises('nesterov needs', lambda case, a: a['hp'].update(
        damp=0.5), geo=cc.MID)
    _twin_raises('in_mom must be', lambda case, a: case.__setitem__(
        'in_mom', case['in_mom'].double()), geo=cc.MID)
    _twin_raises('in_mom must be', lambda case, a: case.__setitem__(
        'in_mom', case['in_mom'].t().contiguous().t()), geo=cc.MID)
    _twin_raises('snap must be', lambda case, a: a.__setitem__(
        'snap', a['snap'].double()))
    _twin_raises('in_mom must be', lambda case, a: case.__setitem__(
        'in_mom', case['in_mom'][:-1].contiguous()), geo=cc.MID)


def test_limits_exported_and_admit_the_stock_models():
    lim = ops.cnn_round_limits()
    assert lim == dict(B=64, K=128, Cin=ops.CNNROUND_MAXCIN,
                       S=ops.CNNROUND_MAXS, C1=ops.CNNROUND_MAXC1,
                       C2=ops.CNNROUND_MAXC2, H=ops.CNNROUND_MAXH)
    for Cin, S, K in ((1, 28, 10), (1, 28, 62), (3, 32, 10), (3, 32, 100)):
        layout, N = cc.make_layout(Cin, S, 20, 50, 512, K)
        assert len(ops.cnn_layout_check(layout, Cin * S * S, N)) == 8


# --------------------------------------------------------------------------
# a packed federation on the CPU
# --------------------------------------------------------------------------
def _federation(extra=(), arch='cnn', cached=True, batch='2', seed=1,
                data='mnist'):
    os.environ['FEDTORCH_SYNTH_SIZE'] = '200'
    from fedtorch_amd.parameters import get_args
    from fedtorch_amd.nodes import Client
    args = get_args([
        '-d', data, '-a', arch, '--mlp_hidden_size', '24',
        '--mlp_num_layers', '2', '-f', 'true',
        '--federated_type', 'fedavg', '--num_comms', '3',
        '--clients_per_rank', '4', '-b', batch, '--lr', '0.05',
        '--federated_sync_type', 'local_step', '--local_step', '3',
        '--online_client_rate', '0.75', '--in_momentum', 'true',
        '--in_momentum_factor', '0.9', '--weight_decay', '1e-3',
        '--lr_schedule_scheme', 'custom_multistep',
        '--lr_change_epochs', '1,2', '--lr_decay', '2',
        '--stop_criteria', 'epoch', '--num_epochs', '8',
        '--on_cuda', 'false', '-j', '0', '--manual_seed', '7',
        '--checkpoint', '/tmp/ft_cnnround', '--debug', 'false']
        + list(extra))
    client = Client(args, 0)
    client.initialize()
    client.initialize_dataset()
    client.load_local_dataset()
    client.gen_aux_models()
    pack = multiclient.ClientPack(client, 4)
    pack.build_loaders()
    if cached:
        for j, old in enumerate(pack.train_loaders):
            pack.train_loaders[j] = DeviceCachedLoader(
                old.dataset, client.args.batch_size, seed=100 * seed + j,
                shuffle=True, device='cpu')
    return client, pack


@pytest.fixture
def flag(monkeypatch):
    monkeypatch.setattr(multiclient, '_BATCHED_CNN_ENABLED', True)


def test_cnn_batched_eligible_truth_table(flag, monkeypatch):
    client, pack = _federation()
    assert pack.cnn_batched_blockers() == [] and pack.cnn_batched_eligible()
    # the linear and the MLP path do not take a CNN, whatever their flags say
    assert pack.linear_layout() is None and not pack.batched_eligible()
    assert pack.mlp_layout() is None and not pack.mlp_batched_eligible()
    with monkeypatch.context() as m:
        m.setattr(multiclient, '_BATCHED_ENABLED', True)
        m.setattr(multiclient, '_BATCHED_MLP_ENABLED', True)
        assert not pack.batched_eligible()
        assert not pack.mlp_batched_eligible()
    layout = pack.cnn_layout()
    assert layout['image'] == (1, 28)
    assert layout['conv1'][2:] == (20, 0) and layout['conv2'][2:] == (50, 0)
    assert layout['fc1'][2] == 512 and layout['fc2'][2] == 10
    flat, model = client.arena.flat, client.model
    for key, mod in (('conv1', model.conv1), ('conv2', model.conv2),
                     ('fc1', model.fc1), ('fc2', model.fc2)):
        assert flat[layout[key][0]:].data_ptr() == mod.weight.data_ptr()
        assert flat[layout[key][1]:].data_ptr() == mod.bias.data_ptr()

    def blocked():
        return not pack.cnn_batched_eligible()

    with monkeypatch.context() as m:       # the flag
        m.setattr(multiclient, '_BATCHED_CNN_ENABLED', False)
        assert pack.cnn_batched_blockers() == [
            'FEDTORCH_PACKED_BATCHED_CNN is not set']
    for name, value in (('federated_type', 'fedprox'),
                        ('federated_type', 'scaffold'),
                        ('federated_type', 'fedgate'),
                        ('federated_sync_type', 'epoch'),
                        ('growing_batch_size', True), ('bf16', True)):
        with monkeypatch.context() as m:
            m.setattr(client.args, name, value, raising=False)
            assert blocked(), name
    with monkeypatch.context() as m:       # the corrections' opt-ins are not
        m.setattr(multiclient, '_BATCHED_CORR_ENABLED', True)    # this path's
        m.setattr(multiclient, '_BATCHED_MLP_CORR_ENABLED', True)
        m.setattr(client.args, 'federated_type', 'fedprox')
        assert blocked()
    with monkeypatch.context() as m:       # DRFA over fedavg is allowed
        m.setattr(client.args, 'federated_drfa', True, raising=False)
        assert not blocked()
    with monkeypatch.context() as m:       # a correction on the optimizer
        m.setattr(client.optimizer, '_prox_mu', 0.1)
        assert blocked()
    with monkeypatch.context() as m:
        m.setattr(client.optimizer, '_delta', client.arena.new_buffer())
        assert blocked()
    with monkeypatch.context() as m:       # a bf16 twin of the arena
        m.setattr(client.arena, 'half_flat',
                  client.arena.flat.to(torch.bfloat16))
        assert blocked()
    with monkeypatch.context() as m:       # a subclass is another model
        from fedtorch_amd.components.models.cnn import CNN
        m.setattr(model, '__class__', type('Other', (CNN,), {}))
        assert pack.cnn_layout() is None and blocked()
    with monkeypatch.context() as m:       # another kernel size
        m.setattr(model.conv2, 'kernel_size', (3, 3))
        assert pack.cnn_layout() is None and blocked()
    with monkeypatch.context() as m:       # the arena holds other names
        names = list(client.arena.names)
        names[0] = 'other.weight'
        m.setattr(client.arena, 'names', names)
        assert pack.cnn_layout() is None and blocked()
    with monkeypatch.context() as m:       # a channels_last conv2 weight
        cl = list(client.arena.cl)
        cl[client.arena.names.index('conv2.weight')] = True
        m.setattr(client.arena, 'cl', cl)
        assert pack.cnn_layout()['conv2'][3] == 1 and not blocked()
    with monkeypatch.context() as m:       # augmentation
        m.setattr(pack.train_loaders[2], '_aug', True)
        assert blocked()
    with monkeypatch.context() as m:       # not a DeviceCachedLoader
        loaders = list(pack.train_loaders)
        loaders[1] = [(None, None)]
        m.setattr(pack, 'train_loaders', loaders)
        assert blocked()
    with monkeypatch.context() as m:       # unequal batch sizes
        m.setattr(pack.train_loaders[3], 'batch_size', 5)
        assert blocked()
    for B, ok in ((1, True), (64, True), (0, False), (65, False)):
        with monkeypatch.context() as m:   # B outside 1 .. 64
            for ld in pack.train_loaders:
                m.setattr(ld, 'batch_size', B)
                m.setattr(ld, 'drop_last', True)
            assert any('batch size' in w
                       for w in pack.cnn_batched_blockers()) != ok
    with monkeypatch.context() as m:       # a 1-sample last batch
        ld = pack.train_loaders[0]
        n = len(ld.x) // ld.batch_size * ld.batch_size + 1
        m.setattr(ld, 'x', torch.zeros(n, 1, 28, 28))
        assert blocked()
    with monkeypatch.context() as m:       # floating-point labels
        ld = pack.train_loaders[1]
        m.setattr(ld, 'y', ld.y.float())
        assert blocked()
    with monkeypatch.context() as m:       # rows of another size
        ld = pack.train_loaders[1]
        m.setattr(ld, 'x', torch.zeros(len(ld.x), 1, 28, 27))
        assert any('features' in w for w in pack.cnn_batched_blockers())
    for name in ('CNNROUND_MAXK', 'CNNROUND_MAXC1', 'CNNROUND_MAXC2',
                 'CNNROUND_MAXH', 'CNNROUND_MAXS'):
        with monkeypatch.context() as m:   # the op's limits
            m.setattr(ops, name, 9)
            assert blocked(), name
    assert pack.cnn_batched_eligible()
    # plain DataLoaders (no device cache)
    _c, dpack = _federation(cached=False)
    assert not dpack.cnn_batched_eligible()
    # other models are not the CNN
    for arch in ('mlp', 'logistic_regression'):
        _c, opack = _federation(arch=arch)
        assert opack.cnn_layout() is None
        assert opack.cnn_batched_eligible() is False


def _train(batched, extra, monkeypatch, seed):
    """one packed federation of 3 rounds; returns the end state, the
    recorded operands of the batched calls and the weights of each round"""
    from fedtorch_amd.trainings.packed import \
        train_and_validate_federated_packed
    monkeypatch.setattr(multiclient, '_BATCHED_CNN_ENABLED', batched)
    torch.manual_seed(seed)
    np.random.seed(5)
    client, pack = _federation(extra, seed=seed)
    assert pack.cnn_batched_eligible() == batched, pack.cnn_batched_blockers()
    calls, weights, other = [], [], []
    real = ops.cnn_local_rounds

    def op(*a, **k):
        calls.append(([None if not torch.is_tensor(t) else t.clone()
                       for t in a], dict(k)))
        return real(*a, **k)
    monkeypatch.setattr(ops, 'cnn_local_rounds', op)
    for name in ('linear_local_rounds', 'mlp_local_rounds'):
        monkeypatch.setattr(ops, name, lambda *a, **k: other.append(1))
    real_acc = pack.accumulate_partial

    def acc(server, w):
        weights.append(list(w))
        return real_acc(server, w)
    monkeypatch.setattr(pack, 'accumulate_partial', acc)
    start = client.model_server.clone()
    torch.manual_seed(6)
    np.random.seed(6)
    train_and_validate_federated_packed(client, pack)
    a = client.args
    assert not other and not a.out_momentum
    return dict(server=client.model_server.clone(),
                replicas=pack.replicas.clone(), in_mom=pack.in_mom.clone(),
                mom_init=list(pack.mom_init), local_index=a.local_index,
                epoch_=a.epoch_, seen=a.local_data_seen,
                lr=a.old_learning_rate, calls=calls, weights=weights,
                start=start, scale=a.lr_scale_at_sync,
                gens=[l._gen.get_state() for l in pack.train_loaders])


def _replay_federation(run, start, dtype, pre=None):
    """the federation over the recorded operands of the batched rounds, in
    `dtype`: local steps by cc.ref_rounds, then x -= scale * sum_j w_j
    (x - y_j) and the online clients adopt x"""
    server = start.to(dtype).clone()
    pos0 = run['calls'][0][0]
    replicas = pos0[6].to(dtype).clone()
    in_mom = pos0[7].to(dtype).clone()
    mom_init = pos0[8].clone()
    snap = None
    for (pos, kw), w in zip(run['calls'], run['weights']):
        X, Y, idx, steps, lr = pos[:5]
        has_snap = pos[9] is not None
        out = cc.ref_rounds(
            X, Y, idx, steps, lr, server, replicas, in_mom, mom_init,
            torch.zeros_like(replicas) if has_snap else None, pos[10]
            if has_snap else 0, kw['layout'], kw['wd_numel'],
            kw['weight_decay'], kw['momentum'], kw['dampening'],
            kw['nesterov'], dtype=dtype, pre=pre)
        replicas, in_mom, mom_init = (out['replicas'], out['in_mom'],
                                      out['mom_init'])
        snap = out['snap']
        partial = torch.zeros_like(server)
        for j, wj in enumerate(w):
            partial += wj * (server - replicas[j])
        server = server - run['scale'] * partial
        for j, wj in enumerate(w):
            if wj != 0.0:
                replicas[j] = server
    return dict(server=server, replicas=replicas, in_mom=in_mom), snap


# The run makes about 2 10^5 ReLU / pool decisions (27 client steps of 2
# images, 3680 pool windows and 512 fc1 units each), far too many for every
# one to keep the 64x margin of cnnround_cases.case.  What the comparison
# needs is that no path decides differently from the float64 replay.  Every
# path here is an fp32 evaluation of the same expressions in another
# summation order, so each stays within a small multiple of the fp32
# replay's own error e of the float64 values; two of them can disagree about
# a decision only if its float64 margin is below the sum of their errors.
# FED_MARGIN = 4 allows each path twice the fp32 replay's error.  The seeds
# (model init and loader shuffles) were searched on the CPU for it.
FED_MARGIN = 4.0
FED_SEEDS = {False: 12, True: 4}


@pytest.mark.parametrize('drfa', [False, True])
def test_packed_cnn_federation_against_float64_replay(drfa, monkeypatch):
    """C = 4 with one client offline per round, tau = 3, 3 rounds, momentum
    0.9, weight decay, a multistep lr change inside the run; then DRFA over
    fedavg.  The slot loop (flag off) and the batched round (flag on: the
    eager twin here) both against the float64 replay of the operands the
    batched rounds recorded: at most 8x the fp32 replay's own error plus 16
    ulps of scale, and so is their mutual distance."""
    extra = ['--federated_drfa', 'true'] if drfa else []
    with monkeypatch.context() as m:
        slot = _train(False, extra, m, FED_SEEDS[drfa])
    with monkeypatch.context() as m:
        bat = _train(True, extra, m, FED_SEEDS[drfa])
    assert len(slot['calls']) == 0 and len(bat['calls']) == 3   # one a round
    assert slot['local_index'] == bat['local_index'] == 3 * 3 * 3
    assert slot['epoch_'] == bat['epoch_'] and slot['seen'] == bat['seen']
    assert slot['lr'] == bat['lr'] and slot['lr'] < 0.05   # the lr changed
    assert slot['mom_init'] == bat['mom_init']
    assert torch.equal(slot['start'], bat['start'])
    for g0, g1 in zip(slot['gens'], bat['gens']):
        assert torch.equal(g0, g1)
    for (pos, kw), w in zip(bat['calls'], bat['weights']):
        assert pos[3].tolist().count(3) == 3 and pos[3].tolist().count(0) == 1
        assert [x != 0 for x in w] == [s > 0 for s in pos[3].tolist()]
        assert (pos[9] is not None) == drfa
    for ws, wb in zip(slot['weights'], bat['weights']):
        assert np.allclose(ws, wb, rtol=1e-5, atol=0)
    p64, p32 = [], []
    r64, snap64 = _replay_federation(bat, bat['start'], F64, pre=p64)
    r32, _s = _replay_federation(bat, bat['start'], F32, pre=p32)
    for kind, (lo, e) in cc.margins(p64, p32).items():
        assert lo > FED_MARGIN * e, (kind, lo, e)
    for k in sorted(r64):
        e32 = lc.err(r32[k], r64[k])
        tol = lc.bound(e32, r64[k].abs().max().item())
        e_slot, e_bat = lc.err(slot[k], r64[k]), lc.err(bat[k], r64[k])
        d = (slot[k] - bat[k]).abs().max().item()
        print('%s: slot err %.3e  batched err %.3e  slot-batched %.3e  '
              'e32 %.3e  tol %.3e' % (k, e_slot, e_bat, d, e32, tol))
        assert e_slot <= tol, (k, e_slot, tol)
        assert e_bat <= tol, (k, e_bat, tol)
        assert d <= tol, (k, d, tol)
    assert lc.err(bat['server'], bat['start'].double()) > 1e-3   # it trained
