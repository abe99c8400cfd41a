"""Registry modules (DfMBackbone, FrustumToVoxel, OutdoorImVoxelNeck, DfMNeck,
DepthHead): constructor/registry/state_dict contract on CPU, and forward parity
on GPU against outputs of the REFERENCE modules (tests/golden/modules.npz, made
by make_golden.py with the same deterministic weights).
Tolerance for the conv/GN/BN stacks (MIOpen vs torch-CPU reduction order):
rtol 1e-3, atol 1e-4."""
import importlib
import os

import numpy as np
import pytest
import torch

from tests import util

CONV_TOL = dict(rtol=1e-3, atol=1e-4)
DEPTH_CFG = dict(mode='UD', num_bins=32, depth_min=2, depth_max=59.6, downsample_factor=4)


@pytest.fixture(scope='module')
def pkg():
    return importlib.import_module('depth-from-motion_amd')


@pytest.fixture(scope='module')
def mods():
    return importlib.import_module('depth-from-motion_amd.modules')


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(util.GOLDEN, 'modules.npz'))


def test_registry_builds_the_config_dicts(pkg):
    reg = importlib.import_module('depth-from-motion_amd.registry')
    assert {'DfMBackbone', 'FrustumToVoxel', 'DepthHead', 'OutdoorImVoxelNeck', 'DfMNeck'} <= set(
        reg.registered())
    # the dicts of configs/dfm/dfm_r34_1x8_kitti-3d-3class.py:118-145 (+ depth_cfg the detector injects)
    bb = reg.build_backbone(dict(type='DfMBackbone', in_channels=32, cv_channels=32, num_hg=1,
                                 cost_sample_factor=4,
                                 norm_cfg=dict(type='GN', num_groups=32, requires_grad=True)),
                            depth_cfg=dict(mode='UD', num_bins=288, depth_min=2, depth_max=59.6,
                                           downsample_factor=4))
    assert sum(p.numel() for p in bb.parameters()) == 1313344
    ft = reg.build_neck(dict(type='FrustumToVoxel', sem_atten_feat=True, stereo_atten_feat=False,
                             num_3dconvs=1, cv_channels=32, out_channels=32,
                             norm_cfg=dict(type='GN', num_groups=32, requires_grad=True)))
    # 27*64*32 + 2*32; the reference module under the mmcv stub has the same count
    # (SURVEY 8a quotes 55 392, which does not match the three state_dict tensors)
    assert sum(p.numel() for p in ft.parameters()) == 55360
    assert ft.cat_img_feature and ft.in_sem_channels == 32
    n1 = reg.build_neck(dict(type='OutdoorImVoxelNeck', in_channels=64, out_channels=256))
    assert sum(p.numel() for p in n1.parameters()) == 7523328
    n2 = reg.build_neck(dict(type='DfMNeck', in_channels=64, out_channels=256, num_frames=2))
    assert sum(p.numel() for p in n2.parameters()) == 15932160
    dh = reg.build_head(dict(type='DepthHead', with_convs=False,
                             depth_cfg=dict(mode='UD', num_bins=288, min_depth=2, max_depth=59.6),
                             depth_loss=dict(type='balanced_focal', loss_weight=1.0, fg_weight=5,
                                             bg_weight=1, alpha=1, gamma=2),
                             downsample_factor=4, num_views=1))
    assert len(list(dh.parameters())) == 0
    with pytest.raises(KeyError):
        reg.build(dict(type='NoSuchModule'))


def test_state_dict_keys_the_checkpoint_converter_pins(mods):
    """tools/model_converters/convert_dfm_checkpoints.py:34-63 and SURVEY 8b name these keys."""
    bb = mods.DfMBackbone(in_channels=32)
    keys = set(bb.state_dict())
    for k in ('dres0.conv.weight', 'dres0.gn.weight', 'dres0.gn.bias', 'hg_stereo.0.conv1.0.0.weight',
              'hg_stereo.0.conv5.0.weight', 'hg_stereo.0.conv6.1.bias', 'pred_stereo.0.0.conv.weight',
              'pred_stereo.0.1.weight', 'pred_mono.0.0.gn.weight', 'dres1_mono.conv.weight',
              'aggregate_cost.weight'):
        assert k in keys, k
    assert not any(k.endswith('conv.bias') for k in keys)  # bias='auto' under a norm
    ft = mods.FrustumToVoxel()
    assert set(ft.state_dict()) == {'voxel_convs.0.0.conv.weight', 'voxel_convs.0.0.gn.weight',
                                    'voxel_convs.0.0.gn.bias'}
    neck = mods.OutdoorImVoxelNeck(8, 16)
    for k in ('model.0.conv0.conv.weight', 'model.0.conv0.bn.running_mean',
              'model.0.conv0.bn.num_batches_tracked', 'model.1.bn.weight', 'model.5.conv.weight'):
        assert k in neck.state_dict(), k
    dn = mods.DfMNeck(4, 16, num_frames=2)
    for k in ('mono_layers.0.conv0.conv.weight', 'stereo_layers.1.conv.weight',
              'aggregate_layer.weight'):
        assert k in dn.state_dict(), k
    assert dn.state_dict()['stereo_layers.0.conv0.conv.weight'].shape[1] == 8


def _load(module, seed):
    module.load_state_dict(util.synthetic_state_dict(module, seed), strict=True)
    return module.eval().cuda()


@pytest.mark.gpu
def test_dfm_backbone_forward_vs_reference_module(mods, gold, monkeypatch):
    """fp32, the reference's default precision: every 3x3x3 convolution of the aggregation stacks runs the
    MFMA kernel in split precision (conv3d._ConvGFn in its split arithmetic: three bf16 launches accumulated in fp32) -- no
    torch / MIOpen convolution behind this comparison with the reference module's output"""
    import importlib
    cv = importlib.import_module('depth-from-motion_amd.conv3d')
    launched = {'n': 0}
    real = cv.conv3d_g_f32
    monkeypatch.setattr(cv, 'conv3d_g_f32', lambda *a, **k: (launched.__setitem__('n', launched['n'] + 1), real(*a, **k))[1])
    torch_convs = {'n': 0}
    real_torch = cv._torch_path
    monkeypatch.setattr(cv, '_torch_path', lambda *a, **k: (torch_convs.__setitem__('n', torch_convs['n'] + 1), real_torch(*a, **k))[1])
    m = _load(mods.DfMBackbone(in_channels=4, cv_channels=32, cost_sample_factor=4,
                               depth_cfg=DEPTH_CFG), 11)
    m.downsampled_depth = torch.from_numpy(gold['bb_depths'])
    meta = dict(ori_cam2img=util.KITTI_P2, cur2prevs=torch.from_numpy(util.pose(1.0, 0.05, 0.0, -0.9))[None],
                ori_shape=(375, 1242, 3), pad_shape=(16, 32, 3), crop_offset=[600, 150], flip=False,
                scale_factor=[1.0])
    with torch.no_grad():
        cost, sfeat, mfeat = m(torch.from_numpy(gold['bb_cur']).cuda(),
                               torch.from_numpy(gold['bb_prev']).cuda(), [meta])
    np.testing.assert_allclose(sfeat.cpu().numpy(), gold['bb_stereo'], **CONV_TOL)
    np.testing.assert_allclose(mfeat.cpu().numpy(), gold['bb_mono'], **CONV_TOL)
    np.testing.assert_allclose(cost.cpu().numpy(), gold['bb_cost'], **CONV_TOL)
    # dres1 (2 convolutions) + the hourglass (6) per branch, 3 launches each; dres0 / dres0_mono have 8 / 4
    # input channels here (in_channels=4) and the 32 -> 1 prediction heads are not 3x3x3 -> 32 k: torch
    # 6 launches each (three bf16 pieces per operand)
    assert launched['n'] >= 2 * 8 * 6, launched
    assert torch_convs['n'] <= 4, torch_convs


@pytest.mark.gpu
def test_frustum_to_voxel_module_vs_reference_module(mods, gold):
    z = np.load(os.path.join(util.GOLDEN, 'f2v_small.npz'))
    C = z['stereo'].shape[1]
    m = _load(mods.FrustumToVoxel(cv_channels=C, out_channels=8, in_sem_channels=C,
                                  norm_cfg=dict(type='GN', num_groups=4, requires_grad=True)), 21)
    m.coordinates_3d = torch.from_numpy(z['coordinates_3d'])
    m.depth_cfg = dict(depth_min=float(z['depth_min']), depth_max=float(z['depth_max']))
    metas = [{'cam2img': c.tolist(), 'pad_shape': tuple(z['pad_shape']) + (3,)} for c in z['cam2img']]
    with torch.no_grad():
        out = m(torch.from_numpy(z['stereo']).cuda(), torch.from_numpy(z['softmax']).cuda(), metas,
                torch.from_numpy(z['sem']).cuda())
    np.testing.assert_allclose(out.cpu().numpy(), gold['f2v_out'], **CONV_TOL)


@pytest.mark.gpu
def test_voxel_necks_vs_reference_modules(mods, gold):
    x = torch.from_numpy(gold['neck_x']).cuda()
    with torch.no_grad():
        a = _load(mods.OutdoorImVoxelNeck(in_channels=8, out_channels=16), 32)(x)[0]
        b = _load(mods.DfMNeck(in_channels=4, out_channels=16, num_frames=2), 33)(x)[0]
    np.testing.assert_allclose(a.cpu().numpy(), gold['imvoxel_out'], **CONV_TOL)
    np.testing.assert_allclose(b.cpu().numpy(), gold['dfmneck_out'], **CONV_TOL)
    with pytest.raises(AssertionError):
        mods.DfMNeck(in_channels=4, out_channels=16, num_frames=2).cuda()(x[:, :4])


@pytest.mark.gpu
def test_depth_head_module_matches_functional(mods, pkg):
    z = np.load(os.path.join(util.GOLDEN, 'depth_head_small.npz'))
    m = mods.DepthHead(depth_cfg=dict(mode='UD', num_bins=24, min_depth=2, max_depth=59.6),
                       with_convs=False, num_views=1).cuda()
    m.depth_samples = torch.from_numpy(z['depth_samples'])
    vol, soft, pred = m(torch.from_numpy(z['x']).cuda())
    assert np.array_equal(util.bits(vol.cpu().numpy()), util.bits(z['ref_vol']))
    np.testing.assert_allclose(pred.cpu().numpy(), z['ref_pred'], rtol=5e-6)


@pytest.mark.gpu
def test_baseline_config1_kitti_pair_d4_vs_reference_module(mods):
    """BASELINE.json configs[0]: one synthetic KITTI pair (375x1242 -> padded 384x1248), D=4
    planes, through DfMBackbone against the REFERENCE module's output on the same seeded features
    and weights (tests/golden/make_golden_r02.py::make_backbone_cfg1)."""
    import sys
    sys.path.insert(0, util.GOLDEN)
    from make_golden_r02 import CFG1, cfg1_inputs
    z = np.load(os.path.join(util.GOLDEN, 'backbone_cfg1.npz'))
    depth_cfg = dict(mode='UD', num_bins=16, depth_min=2, depth_max=59.6, downsample_factor=4)
    m = _load(mods.DfMBackbone(in_channels=CFG1['C'], cv_channels=32, num_hg=1,
                               cost_sample_factor=CFG1['csf'], depth_cfg=depth_cfg,
                               norm_cfg=dict(type='GN', num_groups=32, requires_grad=True)),
              CFG1['wseed'])
    cur, prev, depths, meta = cfg1_inputs()
    assert np.array_equal(depths.numpy(), z['depths'])
    m.downsampled_depth = depths
    with torch.no_grad():
        cost, sfeat, mfeat = m(cur.cuda(), prev.cuda(), [meta])
    assert cost.shape == (1, 1, 4, 96, 312) and sfeat.shape == (1, 32, 4, 96, 312)
    np.testing.assert_allclose(cost.cpu().numpy(), z['cost'], **CONV_TOL)
    np.testing.assert_allclose(sfeat[..., ::8, ::8].cpu().numpy(), z['stereo_s8'], **CONV_TOL)
    np.testing.assert_allclose(mfeat[..., ::8, ::8].cpu().numpy(), z['mono_s8'], **CONV_TOL)
    np.testing.assert_allclose(sfeat.abs().mean((0, 2, 3, 4)).cpu().numpy(), z['stereo_abs_mean'], rtol=1e-3)
    np.testing.assert_allclose(mfeat.abs().mean((0, 2, 3, 4)).cpu().numpy(), z['mono_abs_mean'], rtol=1e-3)


@pytest.mark.gpu
def test_bev_hourglass_and_spp_unet_neck_vs_reference_modules(mods):
    import sys
    sys.path.insert(0, util.GOLDEN)
    from make_golden_r02 import BEV_CFG, SPP_CFG, bev_spp_inputs
    z = np.load(os.path.join(util.GOLDEN, 'bev_spp.npz'))
    bev, feats = bev_spp_inputs()
    b = mods.BEVHourglass(**BEV_CFG)
    assert list(b.state_dict()) == list(z['bev_keys'])
    b = _load(b, 52)
    with torch.no_grad():
        pre, post = b(bev.cuda())
    np.testing.assert_allclose(pre.cpu().numpy(), z['bev_prehg'], **CONV_TOL)
    np.testing.assert_allclose(post.cpu().numpy(), z['bev_out'], **CONV_TOL)
    s = mods.SPPUNetNeck(**SPP_CFG)
    assert list(s.state_dict()) == list(z['spp_keys'])
    s = _load(s, 53)
    with torch.no_grad():
        stereo, sem = s([f.cuda() for f in feats])
    assert stereo.shape == (1, 12, 256, 256) and sem.shape == (1, 12, 64, 64)
    np.testing.assert_allclose(stereo[..., ::4, ::4].cpu().numpy(), z['spp_stereo_s4'], **CONV_TOL)
    np.testing.assert_allclose(sem.cpu().numpy(), z['spp_sem'], **CONV_TOL)
    np.testing.assert_allclose(stereo.abs().mean((0, 2, 3)).cpu().numpy(), z['spp_stereo_abs_mean'], rtol=1e-3)


@pytest.mark.gpu
def test_dfm_stereo_path_runs_the_training_config_end_to_end(pkg):
    """configs/dfm/dfm_r34_1x8_kitti-3d-3class.py's model dict (as extracted from the file):
    neck -> backbone_stereo -> depth_head -> feature_transformation -> BEVHourglass, plus the
    dense depth loss (dfm.py:348-356) and a backward pass through every HIP kernel of the path.
    Reduced image (128x256) and voxel range so the test stays small; channel widths, depth bins
    and module wiring are the config's."""
    import json
    with open(os.path.join(util.GOLDEN, 'configs_dfm.json')) as f:
        model = json.load(f)['dfm_r34_1x8_kitti-3d-3class.py']['model']
    model = dict(model)
    model['depth_cfg'] = dict(model['depth_cfg'], num_bins=32)          # D = 8 planes
    model['depth_head'] = dict(model['depth_head'],
                               depth_cfg=dict(model['depth_head']['depth_cfg'], num_bins=32))
    model['voxel_cfg'] = dict(point_cloud_range=[2, -6.4, -3, 27.6, 6.4, 1], voxel_size=[0.2, 0.2, 0.2])
    path = pkg.DfMStereoPath(model).cuda()
    H, W = 256, 512
    gen = torch.Generator().manual_seed(7)

    def pyramid():
        return [torch.randn(1, c, H // s, W // s, generator=gen).cuda()
                for c, s in ((3, 1), (64, 2), (128, 4), (128, 4), (128, 4))]
    K = util.KITTI_P2.copy()
    meta = dict(ori_cam2img=K, cam2img=K.tolist(), cur2prevs=util.pose(0.5, 0.02, 0.0, -0.8)[None],
                ori_shape=(H, W, 3), pad_shape=(H, W, 3), crop_offset=[0, 0], flip=False,
                scale_factor=[1.0])
    out = path(pyramid(), pyramid(), [meta])
    assert out['mono_stereo_costs'].shape == (1, 1, 8, H // 4, W // 4)
    assert out['upsample_costs'].shape == (1, 1, 32, H, W)
    assert out['volume_feat'].shape == (1, 32, 5, 64, 128)
    assert out['bev_feat'].shape == (1, 64, 64, 128)
    depth_img = (torch.rand(1, 1, H, W, generator=gen) * 60).cuda()
    depth_img[torch.rand(1, 1, H, W, generator=gen).cuda() < 0.8] = 0
    fg = (torch.rand(1, 1, H, W, generator=gen) < 0.3).float().cuda()
    loss = path.loss_dense_depth(out, depth_img, fg) + out['bev_feat'].square().mean()
    loss.backward()
    assert torch.isfinite(loss)
    grads = [p.grad for p in path.parameters() if p.requires_grad]
    assert all(g is not None and torch.isfinite(g).all() for g in grads)
    assert sum(float(g.abs().sum()) > 0 for g in grads) > 0.9 * len(grads)


@pytest.mark.gpu
def test_dfm_stereo_path_inference_bf16_ndhwc_matches_fp32(pkg, monkeypatch):
    """The same config path at inference in bf16 with the channels-last volume: every 3x3x3
    convolution in the MFMA kernels, GroupNorm(+residual) fused, the depth head fused into
    FrustumToVoxel (no upsample_costs tensor), against the fp32 / NCDHW run of the same weights."""
    import json
    cv = importlib.import_module('depth-from-motion_amd.conv3d')
    with open(os.path.join(util.GOLDEN, 'configs_dfm.json')) as f:
        model = json.load(f)['dfm_r34_1x8_kitti-3d-3class.py']['model']
    model = dict(model)
    model['depth_cfg'] = dict(model['depth_cfg'], num_bins=32)
    model['depth_head'] = dict(model['depth_head'],
                               depth_cfg=dict(model['depth_head']['depth_cfg'], num_bins=32))
    model['voxel_cfg'] = dict(point_cloud_range=[2, -6.4, -3, 27.6, 6.4, 1], voxel_size=[0.2, 0.2, 0.2])
    torch.manual_seed(5)
    path = pkg.DfMStereoPath(model).cuda().eval()
    H, W = 256, 512
    gen = torch.Generator().manual_seed(7)
    feats = [[torch.randn(1, c, H // s, W // s, generator=gen).cuda()
              for c, s in ((3, 1), (64, 2), (128, 4), (128, 4), (128, 4))] for _ in range(2)]
    K = util.KITTI_P2.copy()

    def meta():
        return dict(ori_cam2img=K, cam2img=K.tolist(), cur2prevs=util.pose(0.5, 0.02, 0.0, -0.8)[None],
                    ori_shape=(H, W, 3), pad_shape=(H, W, 3), crop_offset=[0, 0], flip=False,
                    scale_factor=[1.0])
    with torch.no_grad():
        ref = path(feats[0], feats[1], [meta()])
    assert ref['upsample_costs'] is None and isinstance(ref['upsample_costs_softmax'], pkg.LazyDepthDistribution)
    calls = {'g': 0, 'c32': 0}
    real_g, real_c = cv.conv3d_g, cv.conv3d_k3_c32
    monkeypatch.setattr(cv, 'conv3d_g', lambda *a, **k: (calls.__setitem__('g', calls['g'] + 1), real_g(*a, **k))[1])
    monkeypatch.setattr(cv, 'conv3d_k3_c32',
                        lambda *a, **k: (calls.__setitem__('c32', calls['c32'] + 1), real_c(*a, **k))[1])
    pb = path.to(torch.bfloat16)
    pb.backbone_stereo.volume_memory_format = torch.channels_last_3d
    with torch.no_grad():
        out = pb([t.bfloat16() for t in feats[0]], [t.bfloat16() for t in feats[1]], [meta()])
    # general kernel: 2 x 6 hourglass convolutions + the 3x3 2-D convolutions of SPPUNetNeck (2 x 7) and
    # BEVHourglass (7) as (1, 3, 3) kernels; 32 -> 32 kernel: dres1 x 2, pred.0 x 2, voxel_convs (2 halves);
    # dres0 (2 halves + mono) run inside the fused plane-sweep kernel (csrc/sweep_conv.hip)
    assert calls['g'] == 12 + 14 + 7 and calls['c32'] == 6, calls
    assert out['volume_feat'].shape == (1, 32, 5, 64, 128) and out['bev_feat'].shape == (1, 64, 64, 128)
    for key in ('mono_stereo_costs', 'volume_feat', 'bev_feat'):
        a, b = out[key].float().cpu().numpy(), ref[key].float().cpu().numpy()
        err = np.abs(a - b).mean() / (np.abs(b).mean() + 1e-6)
        assert err < 0.06, f'{key}: mean relative error {err:.3f}'


def _wide_inputs():
    gen = torch.Generator().manual_seed(60)   # tests/golden/make_golden_r02.py::wide_inputs
    return dict(hg=torch.randn(1, 32, 8, 12, 16, generator=gen),
                neck=torch.randn(1, 64, 10, 12, 12, generator=gen),
                dfmneck=torch.randn(1, 128, 10, 12, 12, generator=gen))


# 2x the largest values measured on MI355X in round 5 (max 0.0128 of full scale, rms 0.0088; the bar was
# rtol 5e-2 + 3 % of full scale before): bf16 activations through 6-8 convolution layers
BF16_MODULE_MAX, BF16_MODULE_RMS = 0.026, 0.018


def _close_bf16(got, ref, what='module'):
    """bf16 activations through 6-8 convolution layers against the reference module's fp32 output"""
    e_max, e_rms = util.bf16_end_to_end_error(got, ref, what)
    assert e_max <= BF16_MODULE_MAX and e_rms <= BF16_MODULE_RMS, (e_max, e_rms)


@pytest.mark.gpu
def test_wide_modules_mfma_path_vs_reference_modules(mods, monkeypatch):
    """hourglass(32), OutdoorImVoxelNeck(64 -> 256), DfMNeck(64 -> 256, 2 frames) at their real
    channel widths against the REFERENCE modules (tests/golden/modules_wide.npz):
    fp32 NCDHW (torch convolutions) within CONV_TOL, and bf16 channels_last_3d -- every 3x3x3
    convolution in the hand-written MFMA kernels, eval-mode BatchNorm folded into their epilogue --
    within the bf16 tolerance."""
    cv = importlib.import_module('depth-from-motion_amd.conv3d')
    calls = {'g': 0}
    real = cv.conv3d_g

    def counted(*a, **k):
        calls['g'] += 1
        return real(*a, **k)
    monkeypatch.setattr(cv, 'conv3d_g', counted)
    z = np.load(os.path.join(util.GOLDEN, 'modules_wide.npz'))
    x = _wide_inputs()
    cl = torch.channels_last_3d

    hg = _load(mods.hourglass(32, gn=True), 61)
    assert list(hg.state_dict().keys()) == list(z['hg_keys'])
    with torch.no_grad():
        y, pre, post = hg(x['hg'].cuda(), None, None)
    for got, key in ((y, 'hg_out'), (pre, 'hg_pre'), (post, 'hg_post')):
        np.testing.assert_allclose(got.cpu().numpy(), z[key], **CONV_TOL)
    assert calls['g'] == 0
    hgb = hg.to(torch.bfloat16)
    with torch.no_grad():
        y, pre, post = hgb(x['hg'].cuda().bfloat16().contiguous(memory_format=cl), None, None)
    assert calls['g'] == 6, 'all six convolutions of the hourglass run in the general MFMA kernel'
    for got, key in ((y, 'hg_out'), (pre, 'hg_pre'), (post, 'hg_post')):
        _close_bf16(got.float().cpu().numpy(), z[key])

    # hourglass(gn=False): BatchNorm3d instead of GroupNorm (conv_modules.py:42,113,126), eval mode
    hg = _load(mods.hourglass(32, gn=False), 64)
    assert list(hg.state_dict().keys()) == list(z['hgbn_keys'])
    with torch.no_grad():
        y, pre, post = hg(x['hg'].cuda(), None, None)
    for got, key in ((y, 'hgbn_out'), (pre, 'hgbn_pre'), (post, 'hgbn_post')):
        np.testing.assert_allclose(got.cpu().numpy(), z[key], **CONV_TOL)
    calls['g'] = 0
    hgb = hg.to(torch.bfloat16)
    with torch.no_grad():
        y, pre, post = hgb(x['hg'].cuda().bfloat16().contiguous(memory_format=cl), None, None)
    assert calls['g'] == 6
    for got, key in ((y, 'hgbn_out'), (pre, 'hgbn_pre'), (post, 'hgbn_post')):
        _close_bf16(got.float().cpu().numpy(), z[key])

    for cls, kw, seed, xin, key, nconv in (
            (mods.OutdoorImVoxelNeck, dict(in_channels=64, out_channels=256), 62, 'neck', 'imvoxel_out', 9),
            (mods.DfMNeck, dict(in_channels=64, out_channels=256, num_frames=2), 63, 'dfmneck', 'dfmneck_out', 18)):
        m = _load(cls(**kw), seed)
        with torch.no_grad():
            a = m(x[xin].cuda())[0]
        np.testing.assert_allclose(a.cpu().numpy(), z[key], **CONV_TOL)
        calls['g'] = 0
        mb = m.to(torch.bfloat16)
        with torch.no_grad():
            b = mb(x[xin].cuda().bfloat16().contiguous(memory_format=cl))[0]
        assert calls['g'] == nconv, f'{cls.__name__}: {calls["g"]} MFMA launches, expected {nconv}'
        _close_bf16(b.float().cpu().numpy(), z[key])


@pytest.mark.gpu
def test_res_module_trains_through_the_mfma_convolutions(mods):
    """training mode (batch statistics: torch BatchNorm3d) with the convolutions and their input
    gradients in the MFMA kernel, against the SAME bf16 module with torch's convolutions (MIOpen):
    identical rounding points except inside the convolutions.  A ReLU whose input rounds to the
    other side of zero flips a gradient entirely, so a small fraction of outliers is allowed."""
    cv = importlib.import_module('depth-from-motion_amd.conv3d')
    torch.manual_seed(3)
    m = mods.ResModule(64).cuda().train().to(torch.bfloat16)
    x = torch.randn(2, 64, 6, 10, 12, device='cuda').bfloat16().contiguous(memory_format=torch.channels_last_3d)
    gy = torch.randn(2, 64, 6, 10, 12, device='cuda').bfloat16().contiguous(memory_format=torch.channels_last_3d)

    def run():
        m.zero_grad()
        xi = x.clone().requires_grad_(True)
        y = m(xi)
        y.backward(gy)
        return (y.detach().float().cpu().numpy(), xi.grad.float().cpu().numpy(),
                m.conv0.conv.weight.grad.float().cpu().numpy())
    y, gx, gw = run()
    elig = cv.MfmaConv3dG.eligible
    cv.MfmaConv3dG.eligible = lambda self, t: False
    try:
        yr, gxr, gwr = run()
    finally:
        cv.MfmaConv3dG.eligible = elig

    def mostly_close(got, ref, frac):
        bad = np.abs(got - ref) > 5e-2 * np.abs(ref) + 0.03 * np.abs(ref).max()
        assert bad.mean() <= frac, f'{bad.mean():.4f} of the elements differ'
    mostly_close(y, yr, 0.0)
    mostly_close(gx, gxr, 0.01)
    mostly_close(gw, gwr, 0.01)


@pytest.mark.gpu
def test_2d_necks_at_config_widths_mfma_path_vs_torch_path(mods, monkeypatch):
    """SPPUNetNeck / BEVHourglass with the channel widths of configs/dfm/dfm_r34_1x8_kitti-3d-3class.py:
    the bf16 channels_last inference path (3x3 convolutions and up-convolutions in the MFMA kernel
    with a (1, 3, 3) kernel, eval-mode BatchNorm folded into its epilogue) against the same modules
    run in fp32 by torch (itself pinned to the reference modules at small widths by
    test_bev_hourglass_and_spp_unet_neck_vs_reference_modules)."""
    cv = importlib.import_module('depth-from-motion_amd.conv3d')
    calls = {'n': 0}
    real = cv.conv3d_g

    def counted(*a, **k):
        calls['n'] += 1
        return real(*a, **k)
    monkeypatch.setattr(cv, 'conv3d_g', counted)
    gn = dict(type='GN', num_groups=32, requires_grad=True)
    gen = torch.Generator().manual_seed(71)
    neck = _load(mods.SPPUNetNeck(in_channels=[3, 64, 128, 128, 128], start_level=2, sem_channels=[128, 32],
                                  stereo_channels=[32, 32], with_upconv=True, cat_img_feature=True, norm_cfg=gn), 72)
    H, W = 256, 512   # level-2..4 maps 64 x 128: one 64 x 64 SPP window row
    feats = [torch.randn(1, c, H // s, W // s, generator=gen).cuda() for c, s in
             ((3, 1), (64, 2), (128, 4), (128, 4), (128, 4))]
    with torch.no_grad():
        ref_st, ref_sem = neck(feats)
    assert calls['n'] == 0
    nb = neck.to(torch.bfloat16)
    with torch.no_grad():
        st, sem = nb([f.bfloat16() for f in feats])
    assert calls['n'] == 7, 'conv 512->64, 64->32, redir 64->64, 3->32 (padded), lastconv 32->32, rpnconv 512->128->32'
    _close_bf16(st.float().cpu().numpy(), ref_st.cpu().numpy())
    _close_bf16(sem.float().cpu().numpy(), ref_sem.cpu().numpy())
    # the fused tail of the SPP branches (csrc/spp_tail.hip) against the same steps as torch ops in bf16:
    # copied source channels bit for bit, interpolated branch channels to bf16 rounding
    import torch.nn.functional as F
    with torch.no_grad():
        cl = [f.bfloat16().contiguous(memory_format=torch.channels_last) for f in feats]
        fused = nb._spp_tail_fused(cl)
        assert fused is not None and fused.is_contiguous(memory_format=torch.channels_last)
        spp = [F.interpolate(b[1](p), tuple(cl[2].shape[2:]), mode='bilinear', align_corners=True)
               for b, p in zip(nb.spp_branches, nb._spp_pool(cl[-1]))]
        unfused = torch.cat((*cl[2:], *spp), 1)
    assert fused.shape == unfused.shape == (1, 512, H // 4, W // 4)
    assert torch.equal(fused[:, :384], unfused[:, :384])
    a, b = fused[:, 384:].float().cpu().numpy(), unfused[:, 384:].float().cpu().numpy()
    assert float(np.abs(b).mean()) > 0.1
    np.testing.assert_allclose(a, b, rtol=2.0 ** -6, atol=2.0 ** -6)

    bev = _load(mods.BEVHourglass(160, 64, norm_cfg=gn), 73)
    x = torch.randn(1, 160, 40, 48, generator=gen).cuda()
    with torch.no_grad():
        ref_pre, ref_post = bev(x)
    calls['n'] = 0
    bb = bev.to(torch.bfloat16)
    with torch.no_grad():
        pre, post = bb(x.bfloat16())
    assert calls['n'] == 7, 'compress_conv + the six (transposed) convolutions of hourglass2d'
    _close_bf16(pre.float().cpu().numpy(), ref_pre.cpu().numpy())
    _close_bf16(post.float().cpu().numpy(), ref_post.cpu().numpy())


@pytest.mark.gpu
def test_hip_graph_replay_of_the_2d_necks_is_the_same_tensor(mods):
    """graphs.GraphedCallable (hipGraph capture of the launch-bound 2-D necks): replays return what a
    plain call returns, bit for bit, for new input values and for a second input signature."""
    graphs = importlib.import_module('depth-from-motion_amd.graphs')
    gn = dict(type='GN', num_groups=32, requires_grad=True)
    bev = _load(mods.BEVHourglass(160, 64, norm_cfg=gn), 73).to(torch.bfloat16)
    g = graphs.GraphedCallable(lambda ts: bev(ts[0]))
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for shape in ((1, 160, 24, 32), (1, 160, 24, 32), (2, 160, 16, 24), (1, 160, 24, 32)):
            x = torch.randn(*shape, generator=gen).cuda().bfloat16().contiguous(memory_format=torch.channels_last)
            pre, post = g([x])
            rpre, rpost = bev(x)
            assert torch.equal(pre, rpre) and torch.equal(post, rpost)
    assert len(g._graphs) == 2
    x = torch.randn(1, 160, 24, 32, generator=gen).cuda().bfloat16().requires_grad_(True)
    assert g([x])[1].requires_grad        # autograd recording: plain call, no graph
