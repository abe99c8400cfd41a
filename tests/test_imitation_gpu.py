"""GPU: the fused feature-imitation loss (csrc/imitation_loss.hip behind depth-from-motion_amd/imitation.py)
against tests/golden/imitation.npz -- the reference's own code -- for every case x dtype x layout, and against
an in-test restatement of the reference's ops (tests/imitation_util.py) where no fixture can go.

Bar: mask exact; loss, gradient and post-update buffers at rtol 1e-4, atol 1e-5.

The gradient has pred's dtype, in the reference's autograd as here, so the fixture records the reference's
gradient twice: from a fp32 ``pred`` leaf and from a bf16 one (the same unmodified function, the same values).
Each combination is held against the reference's gradient for its own pred dtype, at the one bar.  A bf16 value
cannot lie within rtol 1e-4 of a fp32 one in general (round-to-nearest with 8 significand bits moves a value by
up to 2^-8 relative), which is a property of the format and of the reference's own bf16 gradient just as much;
``test_fixture_gradient_bf16_is_one_rounding`` bounds the distance to the fp32 gradient by that figure.
"""
import importlib
import json
import os

import pytest
import torch

from tests import imitation_util as iu
from tests import util

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-4, atol=1e-5)
DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16}


@pytest.fixture(scope='module')
def pkg():
    importlib.import_module('depth-from-motion_amd.build').build_hip()
    return importlib.import_module('depth-from-motion_amd')


@pytest.fixture(scope='module')
def z():
    return iu.load()


def as_layout(x, dtype, channels_last):
    x = x.cuda().to(dtype)
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last if x.dim() == 4 else torch.channels_last_3d)
    return x


def make_layer(pkg, c, C):
    if c['normalize'] is None:
        return None
    layer = pkg.NormalizeLayer(c['normalize'], C).cuda()
    layer.scale.copy_(c['scale0'])
    if 'center0' in c:
        layer.center.copy_(c['center0'])
    return layer.train(c['training'])


def run_case(pkg, c, pd, td, pcl, tcl):
    C = c['pred'].shape[1]
    pred = as_layout(c['pred'], DTYPES[pd], pcl).requires_grad_(True)
    target = as_layout(c['target'], DTYPES[td], tcl)
    layer = make_layer(pkg, c, C)
    loss, info = pkg.imitation_reg_layer_loss(pred, target, dict(mode='inbox', loss_weight=c['loss_weight']),
                                              c['boxes'].cuda(), c['points'].cuda(), norm_layer=layer,
                                              training=c['training'])
    loss.backward()
    return pred, loss, info, layer


COMBOS = [(pd, td, pcl, tcl) for pd in DTYPES for td in DTYPES for pcl in (0, 1) for tcl in (0, 1)]
IDS = [f'{pd}{"cl" if pcl else "pl"}-{td}{"cl" if tcl else "pl"}' for pd, td, pcl, tcl in COMBOS]


@pytest.mark.parametrize('combo', COMBOS, ids=IDS)
@pytest.mark.parametrize('name', iu.CASES)
def test_fixture_mask_loss_buffers(pkg, z, name, combo):
    c = iu.case(z, name)
    pred, loss, info, layer = run_case(pkg, c, *combo)
    assert torch.equal(info['positives'].cpu(), c['positives'])
    assert int(info['num_positives']) == int(c['positives'].sum())
    print(name, combo, 'loss', float(loss), 'ref', c['loss'])
    assert loss.dtype == torch.float32
    assert abs(float(loss) - c['loss']) <= 1e-4 * abs(c['loss']) + 1e-5
    if layer is not None:
        assert torch.allclose(layer.scale.cpu(), c['scale1'], equal_nan=True, **TOL)
        if 'center1' in c:
            assert torch.allclose(layer.center.cpu(), c['center1'], equal_nan=True, **TOL)
        if name in ('e_miss', 'f_few', 'g_eval'):
            assert torch.equal(layer.scale.cpu(), c['scale0'])
    assert pred.grad.dtype == pred.dtype and pred.grad.stride() == pred.stride()


@pytest.mark.parametrize('combo', COMBOS, ids=IDS)
@pytest.mark.parametrize('name', iu.CASES)
def test_fixture_gradient(pkg, z, name, combo):
    """d loss / d pred against the reference's autograd for a ``pred`` leaf of the same dtype, at rtol 1e-4,
    atol 1e-5; zero exactly where the reference's is"""
    c = iu.case(z, name)
    pred, _, _, _ = run_case(pkg, c, *combo)
    got, ref = pred.grad.float().cpu(), (c['grad_bf16'].float() if combo[0] == 'bf16' else c['grad'])
    excess = ((got - ref).abs() / (TOL['atol'] + TOL['rtol'] * ref.abs())).max()
    print(name, combo, 'gradient error / bound', float(excess))
    assert torch.equal(got != 0, ref != 0) or name == 'd_nan'   # zero outside the positives
    assert torch.allclose(got, ref, **TOL)


@pytest.mark.parametrize('name', iu.CASES)
def test_fixture_gradient_bf16_is_one_rounding(pkg, z, name):
    """a bf16 gradient against the reference's fp32 one: within one round-to-nearest to 8 significand bits
    (2^-8 relative), and exactly 0 wherever the reference's is"""
    c = iu.case(z, name)
    pred, _, _, _ = run_case(pkg, c, 'bf16', 'f32', 1, 0)
    got, ref = pred.grad.float().cpu(), c['grad']
    assert torch.equal(got[ref == 0], torch.zeros_like(got[ref == 0]))
    assert bool(((got - ref).abs() <= ref.abs() * 2.0 ** -8 + 1e-30).all())


@pytest.mark.parametrize('name', ['a_3d', 'b_2d', 'c_cw_center_scale'])
def test_two_runs_are_bit_identical(pkg, z, name):
    c = iu.case(z, name)
    runs = []
    for _ in range(2):
        pred, loss, info, layer = run_case(pkg, c, 'bf16', 'f32', 1, 0)
        runs.append((loss.detach().clone(), info['stats'].clone(), pred.grad.clone(), layer.scale.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def restated_step(pkg, pred0, target, cells, kind, C, weight=1.0):
    layer = None if kind is None else pkg.NormalizeLayer(kind, C).cuda()
    pred = pred0.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    loss, positives = iu.restate(pred, target, cells, layer, weight)
    loss.backward()
    return loss, positives, pred.grad, layer


def compare_with_restatement(pkg, pred0, target, points, boxes, mode, kind, weight=1.0):
    C = pred0.shape[1]
    cells = None if mode == 'full' else iu.inbox_cells(points, boxes).cuda()
    rl, rpos, rgrad, rlayer = restated_step(pkg, pred0, target, cells, kind, C, weight)
    layer = None if kind is None else pkg.NormalizeLayer(kind, C).cuda()
    pred = pred0.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    loss, info = pkg.imitation_reg_layer_loss(pred, target, dict(mode=mode, loss_weight=weight),
                                              None if boxes is None else boxes.cuda(),
                                              None if points is None else points.cuda(), norm_layer=layer)
    loss.backward()
    assert torch.equal(info['positives'], rpos)
    print(mode, tuple(pred0.shape), 'positives', int(rpos.sum()), 'of', rpos.numel(), 'loss', float(loss), float(rl))
    assert torch.allclose(loss, rl, **TOL)
    assert torch.allclose(pred.grad.float(), rgrad.float(), **TOL)
    assert pred.grad.dtype == pred.dtype and pred.grad.stride() == pred.stride()
    if layer is not None:
        for (k, a), (_, b) in zip(layer.named_buffers(), rlayer.named_buffers()):
            assert torch.allclose(a, b, **TOL), k
    return int(rpos.sum())


def sparse_target(shape, seed, density=0.3):
    gen = torch.Generator().manual_seed(seed)
    t = torch.randn(shape, generator=gen)
    keep = torch.rand((shape[0], 1) + tuple(shape[2:]), generator=gen) < density
    return (t * keep).cuda()


@pytest.mark.parametrize('shape', [(1, 32, 5, 304, 288), (1, 64, 304, 288)], ids=['volume', 'bev'])
def test_config_k_size(pkg, shape):
    """config K's two pairs, about 40 seeded boxes under the 1e-3 m face margin, a sparse teacher target;
    student fp32 (the gradient bar is an fp32 bar: see test_fixture_gradient), channels-last, teacher planar"""
    points, boxes = iu.seeded_scene(31, 1, 304, 288, 0.2, 40, x0=2.0)
    assert iu.face_margin(points, boxes) > iu.MARGIN
    gen = torch.Generator().manual_seed(32)
    fmt = torch.channels_last_3d if len(shape) == 5 else torch.channels_last
    pred = torch.randn(shape, generator=gen).cuda().contiguous(memory_format=fmt)
    n = compare_with_restatement(pkg, pred, sparse_target(shape, 33), points, boxes, 'inbox', 'cw_scale')
    assert n > 100


@pytest.mark.parametrize('C', [8, 48, 96])
@pytest.mark.parametrize('nz', [0, 3])
def test_general_channel_counts(pkg, C, nz):
    points, boxes = iu.seeded_scene(41 + C, 2, 24, 20, 1.0, 3)
    shape = (2, C) + ((nz,) if nz else ()) + (24, 20)
    gen = torch.Generator().manual_seed(C)
    pred = torch.randn(shape, generator=gen).cuda()
    n = compare_with_restatement(pkg, pred, sparse_target(shape, C + 1, 0.6), points, boxes, 'inbox',
                                 'cw_center+scale', 0.5)
    assert n > 10


@pytest.mark.parametrize('kind', ['cw_scale', None])
def test_mode_full(pkg, kind):
    """'full' = every cell (the reference's branch cannot run: tests/test_imitation.py)"""
    shape = (2, 32, 3, 24, 20)
    gen = torch.Generator().manual_seed(3)
    pred = torch.randn(shape, generator=gen).cuda().contiguous(memory_format=torch.channels_last_3d)
    n = compare_with_restatement(pkg, pred, sparse_target(shape, 4, 0.5), None, None, 'full', kind)
    assert n > 500


def test_stereo_path_training_step_with_imitation_loss(pkg):
    """a small DfMStereoPath + ImitationLoss: backward of the summed imitation losses reaches volume_feat,
    bev_feat and the path's parameters, and matches the same step with the restatement in the kernel's place"""
    with open(os.path.join(util.GOLDEN, 'configs_dfm.json')) as f:
        model = json.load(f)['dfm_r34_1x8_kitti-3d-3class.py']['model']
    model = dict(model)
    model['depth_cfg'] = dict(model['depth_cfg'], num_bins=32)
    model['depth_head'] = dict(model['depth_head'], depth_cfg=dict(model['depth_head']['depth_cfg'], num_bins=32))
    model['voxel_cfg'] = dict(point_cloud_range=[2, -6.4, -3, 27.6, 6.4, 1], voxel_size=[0.2, 0.2, 0.2])
    H, W = 256, 512
    K = util.KITTI_P2.copy()
    results = []
    for fused in (True, False):
        torch.manual_seed(11)
        path = pkg.DfMStereoPath(model).cuda()
        gen = torch.Generator().manual_seed(7)

        def pyramid():
            return [torch.randn(1, c, H // s, W // s, generator=gen).cuda()
                    for c, s in ((3, 1), (64, 2), (128, 4), (128, 4), (128, 4))]
        meta = dict(ori_cam2img=K, cam2img=K.tolist(), cur2prevs=util.pose(0.5, 0.02, 0.0, -0.8)[None],
                    ori_shape=(H, W, 3), pad_shape=(H, W, 3), crop_offset=[0, 0], flip=False, scale_factor=[1.0])
        out = path(pyramid(), pyramid(), [meta])
        vol, bev = out['volume_feat'], out['bev_feat']
        vol.retain_grad()
        bev.retain_grad()
        assert vol.shape[-2:] == bev.shape[-2:]
        ny, nx = vol.shape[-2:]
        cfgs = [dict(lidar_feature_layer='spatial_features_2d', stereo_feature_layer='spatial_features_2d',
                     normalize='cw_scale', layer='conv2d', channel=bev.shape[1], kernel_size=1, use_relu=False,
                     mode='inbox', loss_weight=1.0),
                dict(lidar_feature_layer='volume_features', stereo_feature_layer='volume_features',
                     normalize='cw_scale', layer='conv3d', channel=vol.shape[1], kernel_size=1, use_relu=False,
                     mode='inbox', loss_weight=1.0)]
        torch.manual_seed(12)
        imi = pkg.ImitationLoss(cfgs).cuda().train()
        points, boxes = iu.seeded_scene(51, 1, ny, nx, 0.2, 6, x0=2.0)
        stereo = dict(spatial_features_2d=bev, volume_features=vol)
        lidar = dict(spatial_features_2d=sparse_target(bev.shape, 8), volume_features=sparse_target(vol.shape, 9))
        if fused:
            losses = imi(stereo, lidar, boxes.cuda(), points.cuda())
        else:
            cells = iu.inbox_cells(points, boxes).cuda()
            losses = []
            for cfg, conv in zip(cfgs, imi.conv_imitation):
                x = stereo[cfg['stereo_feature_layer']]
                p = conv(x.to(conv.weight.dtype))
                losses.append(iu.restate(p, lidar[cfg['lidar_feature_layer']], cells,
                                         imi.norm_imitation[cfg['stereo_feature_layer']], 1.0)[0])
        total = sum(losses)
        total.backward()
        grads = {n: p.grad.detach().float().clone() for n, p in path.named_parameters() if p.grad is not None}
        grads.update({'imi.' + n: p.grad.detach().float().clone() for n, p in imi.named_parameters()})
        results.append(([float(v) for v in losses], vol.grad.float().clone(), bev.grad.float().clone(), grads,
                        {k: v.clone() for k, v in imi.named_buffers()}))
    (l0, gv0, gb0, g0, b0), (l1, gv1, gb1, g1, b1) = results
    print('imitation losses', l0, l1)
    assert all(v > 0 for v in l0)
    for a, b in zip(l0, l1):
        assert abs(a - b) <= 1e-4 * abs(b) + 1e-5
    assert float(gv0.abs().max()) > 0 and float(gb0.abs().max()) > 0
    for a, b in ((gv0, gv1), (gb0, gb1)):
        assert float((a - b).norm()) <= 5e-3 * float(b.norm()) + 1e-12
    assert g0.keys() == g1.keys() and len(g0) > 50
    for n in g0:
        # (the convolutions' backward algorithms upstream are not run-to-run bit-stable: norm of the difference)
        err, ref = float((g0[n] - g1[n]).norm()), float(g1[n].norm())
        assert err <= 5e-3 * ref + 1e-12, (n, err, ref)
    for k in b0:
        assert torch.allclose(b0[k], b1[k], **TOL), k
