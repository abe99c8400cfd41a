"""GPU: one training step of the sparse layers and of the whole sparse encoder on the HIP path.

Fixture cases (tests/golden/sparse_train*.npz, generator tests/golden/make_golden_sparse_train.py): the forward in
training mode, the input gradient, dW (in full or as 64 projections), the BatchNorm gradients and the running
statistics after the step against the fp64 stand-in, by the rule of tests/lidar_teacher_ref.py: max |gpu - fp64| <=
4 x the stored fp32-vs-fp64 figure x max |fp64|.  Every measured ratio is printed.

The input-gradient kernel covers Cin in {16, 32, 64}: the 3 -> 16 layer has no input gradient (it raises when one is
required), so the encoder cases check the gradient of the rows after ``conv_input`` (``grad_stage0``), which has passed
through every other layer, instead of the gradient of the three-channel input rows the fixture also stores.

Edge shapes: seeded inputs at the row counts where the tiling can go wrong, against torch autograd over the same dense
masked computation on the CPU in fp64 (tests/sparse_train_ref.py); the bar is the same rule with the figure of the same
computation in fp32, and the seed is chosen by the fixture's mask-margin condition."""
import importlib

import numpy as np
import pytest
import torch

from tests import sparse_train_ref as ref
from tests.lidar_teacher_ref import MARGIN

pytestmark = pytest.mark.gpu
NORM = dict(type='BN1d', eps=1e-3, momentum=0.01)
GEN = ref.generator().gen


@pytest.fixture(scope='module')
def pkg():
    importlib.import_module('depth-from-motion_amd.build').build_hip()
    return importlib.import_module('depth-from-motion_amd')


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def make_layer(pkg, name, marked=True):
    kind, cin, cout, k, s, p, shape, full, count = GEN.LAYERS[name]
    m = pkg.make_sparse_convmodule(cin, cout, k, 'k', stride=s, padding=p, conv_type=kind, norm_cfg=NORM,
                                   order=('conv', 'norm', 'act') if full else ('conv', ))
    m.load_state_dict(ref.state_dict(f'layer.{name}'))
    m = m.cuda().train()
    if marked:
        pkg.enable_sparse_training(m)
    return m


def layer_input(pkg, name, grad):
    z, shape = ref.fixture(), GEN.LAYERS[name][6]
    feats = torch.from_numpy(z[f'layer.{name}.features']).cuda().requires_grad_(grad)
    coors = torch.from_numpy(z[f'layer.{name}.coors']).cuda()
    return feats, coors, pkg.SparseConvTensor(feats, coors, shape, 2)


def report(label, worst):
    print(f'{label}: worst ratio {max(worst):.3f} of {len(worst)} comparisons')


# ----------------------------------------------------------------------------------------------------------------------
# the fixture's cases
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(GEN.LAYERS))
def test_layer_step_matches_the_fixture(pkg, name):
    z, big, prefix = ref.fixture(), ref.side('layers'), f'layer.{name}'
    kind, cin, cout, k, s, p, shape, full, count = GEN.LAYERS[name]
    m = make_layer(pkg, name)
    needs = cin in (16, 32, 64)
    feats, coors, x = layer_input(pkg, name, needs)
    out = m(x)
    out.check_status()
    worst = []
    ref.compare_stage(z, f'{prefix}.stage', out, worst)
    volume = out.dense()
    assert volume.requires_grad
    (volume * ref.loss_weights(z[f'{prefix}.loss_seed'], volume.shape).cuda()).sum().backward()
    if needs:
        got, _ = ref.rows_in_key_order(feats.grad, coors, shape)
        ref.within(f'{name} grad_in', got, big[f'{prefix}.grad_in'], z[f'{prefix}.grad_in.err'], worst)
    else:
        assert feats.grad is None
        with pytest.raises(pkg.MfmaPathError, match='input gradient for Cin = 3'):
            m(layer_input(pkg, name, True)[2])
    ref.check_dw(name, m[0].weight.grad, z, big, prefix, '0.weight', worst)
    if full:
        bn = m[1]
        for key, got in (('grad.1.weight', bn.weight.grad), ('grad.1.bias', bn.bias.grad),
                         ('after.1.running_mean', bn.running_mean), ('after.1.running_var', bn.running_var)):
            ref.within(f'{name} {key}', got, z[f'{prefix}.{key}'], z[f'{prefix}.{key}.err'], worst)
        assert int(bn.num_batches_tracked) == 1
    report(name, worst)


@pytest.mark.parametrize('case', list(GEN.ENCODERS))
def test_encoder_step_matches_the_fixture(pkg, case):
    z, big, prefix = ref.fixture(), ref.side(case), f'enc.{case}'
    shape, batch = [int(s) for s in z[f'{prefix}.sparse_shape']], int(z[f'{prefix}.batch'])
    enc = pkg.CustomSparseEncoder(sparse_shape=shape, **GEN.ENCODER_CFG)
    enc.load_state_dict(ref.state_dict(prefix))
    enc = enc.cuda().train()
    pkg.enable_sparse_training(enc)
    feats = torch.from_numpy(z[f'{prefix}.features']).cuda()
    coors = torch.from_numpy(z[f'{prefix}.coors']).cuda()
    stages = enc.forward_stages(feats, coors, batch)
    enc.check_status()
    stages[0].features.retain_grad()
    worst = []
    ref.compare_stage(z, f'{prefix}.stage', stages[-1], worst)
    volume = stages[-1].dense()                                          # the gradient comes through dense()
    (volume * ref.loss_weights(z[f'{prefix}.loss_seed'], volume.shape).cuda()).sum().backward()
    got, _ = ref.rows_in_key_order(stages[0].features.grad, stages[0].indices, shape)
    ref.within(f'{case} grad_stage0', got, z[f'{prefix}.grad_stage0'], z[f'{prefix}.grad_stage0.err'], worst)
    for name, p in enc.named_parameters():
        assert p.grad is not None, name
        if p.dim() == 5:
            ref.check_dw(f'{case} {name}', p.grad, z, big, prefix, name, worst)
        else:
            ref.within(f'{case} grad.{name}', p.grad, z[f'{prefix}.grad.{name}'], z[f'{prefix}.grad.{name}.err'], worst)
    for name, b in enc.named_buffers():
        if name.endswith('num_batches_tracked'):
            assert int(b) == 1, name
        else:
            ref.within(f'{case} after.{name}', b, z[f'{prefix}.after.{name}'], z[f'{prefix}.after.{name}.err'], worst)
    report(case, worst)


def encoder_step(pkg, case):
    """a fresh encoder's forward (``output_volume_feat``) + backward -> every gradient, the buffers, the outputs"""
    z, prefix = ref.fixture(), f'enc.{case}'
    shape, batch = [int(s) for s in z[f'{prefix}.sparse_shape']], int(z[f'{prefix}.batch'])
    enc = pkg.CustomSparseEncoder(sparse_shape=shape, **GEN.ENCODER_CFG)
    enc.load_state_dict(ref.state_dict(prefix))
    enc = enc.cuda().train()
    pkg.enable_sparse_training(enc)
    spatial, volume = enc(torch.from_numpy(z[f'{prefix}.features']).cuda(), torch.from_numpy(z[f'{prefix}.coors']).cuda(),
                          batch)
    assert spatial.shape == (batch, volume.shape[1] * volume.shape[2], *volume.shape[3:])
    (volume * ref.loss_weights(z[f'{prefix}.loss_seed'], volume.shape).cuda()).sum().backward()
    out = {f'grad.{n}': p.grad for n, p in enc.named_parameters()}
    out.update({n: b for n, b in enc.named_buffers() if b.dtype == torch.float32})
    out['volume'] = volume
    return out


def test_two_runs_of_an_encoder_step_give_the_same_bits(pkg):
    a, b = encoder_step(pkg, 'enc_11_25_19'), encoder_step(pkg, 'enc_11_25_19')
    assert len(a) == 12 + 22 + 22 + 1
    for key in a:
        assert same_bits(a[key], b[key]), key


def test_a_marked_module_in_eval_mode_without_grad_gives_the_unmarked_bits(pkg):
    for name in ('subm_16_16', 'sp_s2_p1', 'sp_1x1'):
        plain, marked = make_layer(pkg, name, marked=False).eval(), make_layer(pkg, name).eval()
        with torch.no_grad():
            a, b = plain(layer_input(pkg, name, False)[2]), marked(layer_input(pkg, name, False)[2])
        assert not b.features.requires_grad and same_bits(a.dense(), b.dense()), name
        if name != 'sp_s2_p1':                                          # the row set is the input's: the rows themselves
            assert same_bits(a.features, b.features), name
        with pytest.raises(pkg.MfmaPathError, match='frozen-BN'):
            marked(layer_input(pkg, name, False)[2])                    # grad mode on: the weight needs a gradient


# ----------------------------------------------------------------------------------------------------------------------
# edge shapes
# ----------------------------------------------------------------------------------------------------------------------
SHAPE, BIG = [6, 12, 10], 1e30
# name: (conv_type, cin, cout, kernel, stride, padding, live rows, options)
EDGES = {f'rows_{n}': ('SubMConv3d', 16, 16, 3, 1, 1, n, {}) for n in (1, 15, 16, 17, 63, 64, 65, 255, 257, 511, 513)}
EDGES.update({
    'padding_rows_interleaved': ('SubMConv3d', 16, 16, 3, 1, 1, 65, dict(dead_every=3)),
    'empty_sample': ('SubMConv3d', 16, 16, 3, 1, 1, 65, dict(batch=3, empty=(1, ))),
    'tap_without_rows': ('SubMConv3d', 16, 16, 3, 1, 1, 40, dict(plane=2)),
    'ch_3_16': ('SubMConv3d', 3, 16, 3, 1, 1, 65, dict(dead_every=4)),
    'ch_32_64': ('SubMConv3d', 32, 64, 3, 1, 1, 65, dict(dead_every=4)),
    'ch_64_64': ('SubMConv3d', 64, 64, 3, 1, 1, 65, dict(dead_every=4)),
    'stride_2': ('SparseConv3d', 16, 32, 3, 2, 1, 65, dict(dead_every=3)),
    'stride_211_pad_011': ('SparseConv3d', 16, 16, 3, (2, 1, 1), (0, 1, 1), 40, dict(dead_every=3)),
    'stride_211_many_rows': ('SparseConv3d', 32, 32, 3, (2, 1, 1), (0, 1, 1), 300, {}),
    'conv_1x1': ('SparseConv3d', 64, 32, 1, 1, 0, 65, dict(dead_every=3)),
})


def edge_inputs(seed, cin, live, batch=2, empty=(), plane=None, dead_every=None):
    """``live`` unique cells (the last cell of sample 0 and the first cell of the next sample among them) in random
    order, with a row that does not exist (b = -1, values of 1e30) after every ``dead_every`` - 1 rows"""
    rng = np.random.default_rng(seed)
    d, h, w = SHAPE
    samples = [b for b in range(batch) if b not in empty]
    cells = set()
    if live >= 2 and plane is None:
        cells.update({(samples[0], d - 1, h - 1, w - 1), (samples[1], 0, 0, 0)})
    while len(cells) < live:
        cells.add((samples[int(rng.integers(0, len(samples)))], int(rng.integers(0, d)) if plane is None else plane,
                   int(rng.integers(0, h)), int(rng.integers(0, w))))
    coors = np.asarray(sorted(cells), dtype=np.int32)[rng.permutation(live)]
    feats = rng.normal(0, 1, (live, cin)).astype(np.float32)
    if dead_every:
        rows = live + live // (dead_every - 1) + 1
        slot = np.ones(rows, bool)
        slot[dead_every - 1::dead_every] = False
        slot[np.flatnonzero(slot)[live:]] = False
        all_coors, all_feats = np.full((rows, 4), -1, np.int32), np.full((rows, cin), BIG, np.float32)
        all_coors[slot], all_feats[slot] = coors, feats
        coors, feats = all_coors, all_feats
    return torch.from_numpy(feats), torch.from_numpy(coors)


@pytest.mark.parametrize('name', list(EDGES))
def test_edge_shapes_against_fp64_autograd(pkg, name):
    kind, cin, cout, k, s, p, live, opt = EDGES[name]
    batch = opt.get('batch', 2)
    rng = np.random.default_rng(99)
    kernel = (k, ) * 3
    weight = torch.from_numpy(rng.uniform(-1, 1, (*kernel, cin, cout)).astype(np.float32)) / (k ** 3 * cin) ** 0.5
    gamma = torch.from_numpy(rng.uniform(0.5, 1.5, cout).astype(np.float32))
    beta = torch.from_numpy(rng.uniform(-0.3, 0.3, cout).astype(np.float32))
    subm = kind == 'SubMConv3d'
    for seed in range(50):                                              # the fixture's mask-margin condition
        feats, coors = edge_inputs(seed, cin, live, **opt)
        r32, r64 = (ref.dense_step(t, feats, coors, SHAPE, batch, weight, gamma, beta, 1e-3, s, p, subm, 31)
                    for t in (torch.float32, torch.float64))
        pre = r64['pre'].abs()
        if torch.equal(r32['pre'] > 0, r64['pre'] > 0) and \
                float(pre.min() / pre.max()) > MARGIN * ref.figure(r32['pre'], r64['pre']):
            break
    else:
        raise AssertionError('no seed meets the mask-margin condition')
    if 'dead_every' in opt:
        assert (coors[:, 0] < 0).any() and int((coors[:, 0] >= 0).sum()) == live
    if name == 'tap_without_rows':
        assert not r64['dw'][0].any() and not r64['dw'][2].any() and r64['dw'][1].any()

    m = pkg.make_sparse_convmodule(cin, cout, k, 'e', stride=s, padding=p, conv_type=kind, norm_cfg=NORM)
    with torch.no_grad():
        m[0].weight.copy_(weight), m[1].weight.copy_(gamma), m[1].bias.copy_(beta)
    m = m.cuda().train()
    pkg.enable_sparse_training(m)
    needs = cin in (16, 32, 64)
    x = feats.cuda().requires_grad_(needs)
    out = m(pkg.SparseConvTensor(x, coors.cuda(), SHAPE, batch))
    out.check_status()
    assert int((out.indices[:, 0] >= 0).sum()) == r64['n']
    volume = out.dense()
    (volume * ref.loss_weights(31, volume.shape).cuda()).sum().backward()
    worst = []

    def check(label, got, key, want32=None, want64=None):
        a32, a64 = (r32[key], r64[key]) if want64 is None else (want32, want64)
        ref.within(f'{name} {label}', got, a64, ref.figure(a32, a64.double()), worst)

    check('volume', volume, 'volume')
    assert not volume.detach().cpu()[r64['volume'] == 0].any()          # inactive sites and ReLU zeros: exactly 0
    if needs:
        check('grad_in', x.grad, 'grad_in')
        assert not x.grad[coors.cuda()[:, 0] < 0].any()                # rows that do not exist: exactly 0
    check('dW', m[0].weight.grad, 'dw')
    check('grad_weight', m[1].weight.grad, 'dgamma')
    check('grad_bias', m[1].bias.grad, 'dbeta')
    check('running_mean', m[1].running_mean, None, 0.01 * r32['mean'], 0.01 * r64['mean'])
    check('running_var', m[1].running_var, None, 0.99 + 0.01 * r32['var'], 0.99 + 0.01 * r64['var'])
    assert int(m[1].num_batches_tracked) == 1
    report(name, worst)


def chain(pkg):
    """SubM 16 -> 16, strided 16 -> 32, SubM 32 -> 32, each with BatchNorm and ReLU, marked, in training mode"""
    torch.manual_seed(5)
    m = pkg.SparseSequential(pkg.make_sparse_convmodule(16, 16, 3, 'a', norm_cfg=NORM),
                             pkg.make_sparse_convmodule(16, 32, 3, 'b', stride=2, padding=1, conv_type='SparseConv3d',
                                                        norm_cfg=NORM),
                             pkg.make_sparse_convmodule(32, 32, 3, 'c', norm_cfg=NORM)).cuda().train()
    pkg.enable_sparse_training(m)
    return m


def chain_step(pkg, m, feats, coors, poison):
    """forward + backward of ``chain`` with an output gradient that is a function of the output COORDINATES; the rows
    that do not exist hold ``poison`` in the input and in the output gradient -> every gradient"""
    dead = coors[:, 0] < 0
    x = torch.where(dead[:, None], torch.full_like(feats, poison), feats).requires_grad_()
    for p in m.parameters():
        p.grad = None
    out = m(pkg.SparseConvTensor(x, coors, SHAPE, 2))
    i = out.indices.long()
    key = ((i[:, 0] * 7 + i[:, 1]) * 13 + i[:, 2]) * 11 + i[:, 3]
    g = torch.sin(key[:, None].float() * 0.37 + torch.arange(out.features.shape[1], device=x.device))
    odead = out.indices[:, 0] < 0
    assert odead.any()                                                   # the strided layer's fixed-capacity rows
    out.features.backward(torch.where(odead[:, None], torch.full_like(g, poison), g))
    grads = {n: p.grad.clone() for n, p in m.named_parameters()}
    grads['input'] = x.grad.clone()
    return grads, dead


def test_nan_in_rows_that_do_not_exist_reaches_no_gradient(pkg):
    m = chain(pkg)
    feats, coors = edge_inputs(3, 16, 120, dead_every=3)
    feats, coors = feats.cuda(), coors.cuda()
    clean, dead = chain_step(pkg, m, feats, coors, 0.0)
    dirty, _ = chain_step(pkg, m, feats, coors, float('nan'))
    assert dead.any() and len(clean) == 3 * 3 + 1
    for key in clean:
        assert torch.isfinite(dirty[key]).all(), key
        assert same_bits(clean[key], dirty[key]), key                   # the live rows: bit for bit
    assert not dirty['input'][dead].any() and dirty['input'][~dead].any()
    assert torch.equal(bits(dirty['input'][dead]), torch.zeros_like(bits(dirty['input'][dead])))   # +0, not -0


def test_all_rows_dead_gives_zero_gradients_and_keeps_the_running_statistics(pkg):
    m = chain(pkg)
    before = {n: b.clone() for n, b in m.named_buffers()}
    coors = torch.full((37, 4), -1, dtype=torch.int32).cuda()
    x = torch.full((37, 16), float('nan')).cuda().requires_grad_()
    out = m(pkg.SparseConvTensor(x, coors, SHAPE, 2))
    out.check_status()
    assert (out.indices[:, 0] < 0).all() and not out.features.detach().any()
    volume = out.dense()
    assert not volume.detach().any()
    (volume * 3.0).sum().backward()
    assert not x.grad.any() and torch.isfinite(x.grad).all()
    for n, p in m.named_parameters():
        assert p.grad is not None and not p.grad.any() and torch.isfinite(p.grad).all(), n
    for n, b in m.named_buffers():
        if n.endswith('num_batches_tracked'):
            assert int(b) == 1
        else:
            assert same_bits(b, before[n]), n                           # a live count of 0: unchanged


def test_batch_norm_over_live_counts_of_zero_and_one(pkg):
    st = importlib.import_module('depth-from-motion_amd.sparse_train')
    rng = np.random.default_rng(8)
    for c in (16, 32, 64):
        bn = torch.nn.BatchNorm1d(c, eps=1e-3, momentum=0.01).cuda().train()
        with torch.no_grad():
            bn.weight.uniform_(0.5, 1.5), bn.bias.uniform_(-0.3, 0.3)
            bn.running_mean.uniform_(-1, 1), bn.running_var.uniform_(0.5, 2)
        mean0, var0 = bn.running_mean.clone(), bn.running_var.clone()
        x = torch.from_numpy(rng.normal(0, 1, (5, c)).astype(np.float32)).cuda()
        x[[0, 1, 3, 4]] = float('nan')
        g = torch.ones(5, c).cuda()
        g[[0, 4]] = float('nan')
        for live, relu in ((0, True), (1, True), (1, False)):
            idx = torch.full((5, 4), -1, dtype=torch.int32).cuda()
            if live:
                idx[2] = torch.tensor([0, 1, 2, 3], dtype=torch.int32)
            xin = x.clone().requires_grad_()
            y = st.batch_norm_rows(xin, idx, bn, relu)
            y.backward(g)
            for t in (y, xin.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var):
                assert torch.isfinite(t).all()
            assert not y.detach()[[0, 1, 3, 4]].any() and not xin.grad.any()      # count 1: x - mean is 0, so is grad_x
            if live == 0:
                assert same_bits(bn.running_mean, mean0) and same_bits(bn.running_var, var0)
                assert not y.detach().any() and not bn.bias.grad.any() and not bn.weight.grad.any()
            else:
                want = bn.bias.detach().clamp_min(0) if relu else bn.bias.detach()
                assert same_bits(y.detach()[2], want)                              # xhat is exactly 0
                mom = torch.tensor(0.01, device='cuda')
                assert torch.equal(bn.running_mean, mean0 * (1 - mom) + x[2] * mom)
                assert torch.equal(bn.running_var, var0 * (1 - mom))               # M2 / max(1 - 1, 1) = 0
                assert torch.equal(bn.bias.grad, (want > 0).float() if relu else torch.ones_like(want))
                assert not bn.weight.grad.any()
                mean0, var0 = bn.running_mean.clone(), bn.running_var.clone()
            bn.weight.grad = bn.bias.grad = None
