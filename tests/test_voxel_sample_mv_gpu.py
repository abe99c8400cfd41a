"""GPU: depth supervision of the multi-view detector on the HIP path (multiview_dfm.py:218-256, 296-304).

``voxel_sample_mv`` (one launch for all (sample, view) pairs) against the loop of single ``voxel_sample`` calls it
replaces -- exact equality, the condition under which ``MultiViewDfMMixin.feature_transformation`` may use it --
and against tests/golden/multiview_depth.npz, which the reference's own ``feature_transformation`` / ``DepthHead``
produced (tests/golden/make_golden_mvdepth.py).  Bars: fp32 bit-exact with the stored inverses
(test_point_sample_gpu.test_voxel_sample_bitexact_vs_reference_fixture); rtol 1e-4 / atol 1e-5 with the inverse
retaken on this host (test_voxel_sample_with_host_inverse_is_close); the backward bars of
test_voxel_sample_backward_vs_torch_grid_sample / _vs_the_oracle_operator; DESIGN.md section 2 for the depth head
(fp32 conv / norm stacks rtol 1e-3, atol 1e-4; one bf16 launch atol 2^-7 max|ref|)."""
import importlib
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import util

pytestmark = pytest.mark.gpu
CONV_TOL = dict(rtol=1e-3, atol=1e-4)
BF16_BAR = 2.0 ** -7
CL = torch.channels_last_3d


@pytest.fixture(scope='module')
def pkg():
    assert torch.cuda.is_available()
    return importlib.import_module('depth-from-motion_amd')


@pytest.fixture(scope='module')
def gm():
    """the fixture's generator: its constants and the img_metas it ran the reference with"""
    sys.path.insert(0, util.GOLDEN)
    try:
        return importlib.import_module('make_golden_mvdepth')
    finally:
        sys.path.remove(util.GOLDEN)


@pytest.fixture(scope='module')
def z():
    return np.load(os.path.join(util.GOLDEN, 'multiview_depth.npz'))


def volume_of(z, dtype=torch.float32, channels_last=False):
    vol = torch.from_numpy(z['volume_q'].astype(np.float32) / 16.0).cuda().to(dtype)   # exact in bf16 too
    return vol.contiguous(memory_format=CL) if channels_last else vol


def call_args(gm, z, td):
    """the arguments feature_transformation derives from img_metas (integration.py), for voxel_sample_mv"""
    metas = gm.metas(z['lidar2img'])
    return dict(
        proj_mats=z['lidar2img'], downsample_factor=gm.DS,
        img_scale_factors=[m.get('scale_factor', 1.0) if td else 1.0 for m in metas],
        img_crop_offsets=[m.get('img_crop_offset', 0) if td else 0 for m in metas],
        img_flips=[m.get('flip', False) if td else False for m in metas],
        img_pad_shape=gm.INPUT_SHAPE if td else gm.ORI_SHAPE,
        img_shapes=[[m['img_shape'][v][:2] for v in range(gm.NV)] for m in metas], num_views=gm.NV)


def batched(pkg, gm, z, vol, td, **kw):
    return pkg.voxel_sample_mv(vol, z['voxel_range'], z['voxel_size'], torch.from_numpy(z['depth_samples']),
                               **call_args(gm, z, td), **kw)


def looped(pkg, gm, z, vol, td):
    a = call_args(gm, z, td)
    outs = []
    for b in range(gm.B):
        for v in range(gm.NV):
            outs.append(pkg.voxel_sample(
                vol[b][None], z['voxel_range'], z['voxel_size'], torch.from_numpy(z['depth_samples']),
                torch.from_numpy(z['lidar2img'][b][v]), gm.DS, a['img_scale_factors'][b], a['img_crop_offsets'][b],
                a['img_flips'][b], a['img_pad_shape'], a['img_shapes'][b][v], aligned=True))
    return torch.cat(outs)


@pytest.mark.parametrize('td', [True, False], ids=['transform_depth', 'original_size'])
@pytest.mark.parametrize('channels_last', [False, True], ids=['ncdhw', 'ndhwc'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_batched_equals_looped_bit_for_bit(pkg, gm, z, dtype, channels_last, td):
    vol = volume_of(z, dtype, channels_last)
    want = looped(pkg, gm, z, vol, td)
    got = batched(pkg, gm, z, vol, td)
    assert got.shape == want.shape and got.dtype == dtype and got.is_contiguous()
    assert float(want.float().abs().sum()) > 0
    assert torch.equal(got, want)
    # the channels-last result (what MfmaConv3dTo1 reads) is the same tensor in another layout
    got_cl = batched(pkg, gm, z, vol, td, memory_format=CL)
    assert got_cl.is_contiguous(memory_format=CL) and torch.equal(got_cl, want)


@pytest.mark.parametrize('channels', [5, 12])
def test_channel_counts_outside_the_16_byte_blocks(pkg, gm, z, channels):
    """C not a multiple of 4 (fp32) / 8 (bf16): a channels-last volume goes through the element-wise kernel"""
    for dtype in (torch.float32, torch.bfloat16):
        vol = volume_of(z, dtype)[:, :channels].contiguous(memory_format=CL)
        want = looped(pkg, gm, z, vol, True)
        assert torch.equal(batched(pkg, gm, z, vol, True), want)
        assert torch.equal(batched(pkg, gm, z, vol, True, memory_format=CL), want)


@pytest.mark.parametrize('channels_last', [False, True], ids=['ncdhw', 'ndhwc'])
def test_fp32_bitexact_vs_reference_fixture(pkg, gm, z, channels_last):
    vol = volume_of(z, torch.float32, channels_last)
    got = batched(pkg, gm, z, vol, True, proj_invs=z['proj_inv'])   # the inverses taken where the fixture was made
    assert np.array_equal(util.bits(got.cpu().numpy()), util.bits(z['stereo_td1']))
    got = batched(pkg, gm, z, vol, False, proj_invs=z['proj_inv'])
    assert got.shape == (gm.B * gm.NV, gm.C) + z['stereo_td0'].shape[2:]
    kept = got[:, :gm.KEPT_CHANNELS_TD0].cpu().numpy()               # the fixture keeps channels 0..3 of this one
    assert np.array_equal(util.bits(kept), util.bits(z['stereo_td0']))


def test_device_resident_matrices_are_inverted_on_the_device(pkg, gm, z):
    """matrices staged on the device never come back to the host; dfm_camera_prepare's inverse (Gauss-Jordan in
    fp32) is close to torch.inverse, not bit-identical.  Bar, from the number format: a lattice point is a sum of
    four products of up to ~16 m each, every factor of the inverse a few fp32 roundings (2^-24 each) off ->
    <= 1e-5 of a voxel per axis; a trilinear sample moves by at most the largest difference between neighbouring
    voxels, 2 max|v|, per voxel of displacement and axis: atol = 3 * 2 max|v| * 1e-5; rtol 1e-4 as in
    test_voxel_sample_with_host_inverse_is_close."""
    vol = volume_of(z)
    a = call_args(gm, z, True)
    a['proj_mats'] = [torch.from_numpy(z['lidar2img'][b]).cuda() for b in range(gm.B)]
    got = pkg.voxel_sample_mv(vol, z['voxel_range'], z['voxel_size'], torch.from_numpy(z['depth_samples']), **a)
    np.testing.assert_allclose(got.cpu().numpy(), z['stereo_td1'], rtol=1e-4,
                               atol=3 * 2 * float(vol.abs().max()) * 1e-5)


class _Host(torch.nn.Module):
    """a detector-shaped host of the mixin: the volume comes from ``backbone_3d`` (as in the generator)"""

    def __init__(self, pkg, gm, z, td, volume):
        super().__init__()
        self.voxel_range, self.voxel_size = list(gm.VOXEL_RANGE), list(gm.VOXEL_SIZE)
        self.n_voxels, self.valid_sample, self.temporal_aggregate = list(gm.N_VOXELS), True, 'mean'
        self.transform_depth, self.depth_samples = td, torch.from_numpy(z['depth_samples'])
        self.with_backbone_3d, self.with_neck_3d, self.with_depth_head = True, False, True
        self.depth_head = pkg.registry.build_head(dict(
            type='DepthHead', depth_cfg=dict(gm.HEAD_DEPTH_CFG), in_channels=gm.C, with_convs=True,
            downsample_factor=gm.DS, num_views=gm.NV))
        self._volume = volume

    def backbone_3d(self, lifted):
        assert lifted.shape == self._volume.shape
        return [self._volume]
    backbone_3d.output_bev = False


@pytest.mark.parametrize('td', [True, False], ids=['transform_depth', 'original_size'])
def test_mixin_feature_transformation_vs_reference_fixture(pkg, gm, z, td):
    vol = volume_of(z)

    class Host(pkg.MultiViewDfMMixin, _Host):
        pass
    host = Host(pkg, gm, z, td, vol)
    feats = torch.randn(gm.B, gm.NV, gm.C, 6, 8, generator=torch.Generator().manual_seed(711)).cuda()
    volume_feat, stereo = host.feature_transformation(feats, gm.metas(z['lidar2img']), gm.NV, 1)
    assert volume_feat is vol
    # the switch is behaviour-neutral: the loop it replaced, bit for bit
    assert torch.equal(stereo, looped(pkg, gm, z, vol, td))
    ref = z['stereo_td1'] if td else z['stereo_td0']
    got = stereo[:, :ref.shape[1]].cpu().numpy()
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-5)   # the inverses are retaken on this host


def torch_voxel_sample_mv(ps, gm, z, volume, td):
    """the reference computation (point_fusion.py:366-408 inside the loop of multiview_dfm.py:220-256) in torch
    on the CPU, differentiable: the frustum lattice, the augmentations undone, the stored inverse, grid_sample"""
    metas = gm.metas(z['lidar2img'])
    pad = gm.INPUT_SHAPE if td else gm.ORI_SHAPE
    h_out, w_out = round(pad[0] / gm.DS), round(pad[1] / gm.DS)
    depths = torch.from_numpy(z['depth_samples'])[::gm.DS]
    rng, vsz = torch.from_numpy(z['voxel_range']), torch.from_numpy(z['voxel_size'])
    outs = []
    for b, m in enumerate(metas):
        sx, sy = ps._scale_xy(m.get('scale_factor', 1.0)) if td else (1.0, 1.0)
        cx, cy = ps._crop_xy(m.get('img_crop_offset', 0)) if td else (0.0, 0.0)
        for v in range(gm.NV):
            ds_, ys, xs = torch.meshgrid(depths, torch.arange(h_out, dtype=torch.float32) * gm.DS,
                                         torch.arange(w_out, dtype=torch.float32) * gm.DS, indexing='ij')
            if td and m.get('flip', False):
                xs = float(m['img_shape'][v][1]) - xs
            xs, ys = (xs + cx) / sx, (ys + cy) / sy
            hom = torch.stack([xs * ds_, ys * ds_, ds_, torch.ones_like(ds_)], -1).reshape(-1, 4)
            p3 = (hom @ torch.from_numpy(z['proj_inv'][b][v]).T)[:, :3]
            g = ((p3 - rng[:3]) / vsz - 0.5) / ((rng[3:] - rng[:3]) / vsz) * 2 - 1
            g = g.view(1, len(depths), h_out, w_out, 3)[..., [2, 1, 0]]
            outs.append(F.grid_sample(volume[b][None], g, mode='bilinear', padding_mode='zeros', align_corners=True))
    return torch.cat(outs)


@pytest.mark.parametrize('out_cl', [False, True], ids=['out_ncdhw', 'out_ndhwc'])
@pytest.mark.parametrize('channels_last', [False, True], ids=['ncdhw', 'ndhwc'])
def test_backward_vs_torch_autograd_of_the_reference_computation(pkg, gm, z, channels_last, out_cl):
    ps = importlib.import_module('depth-from-motion_amd.point_sample')
    rs = np.random.RandomState(5)
    v_cpu = torch.from_numpy(rs.randn(gm.B, gm.C, *gm.N_VOXELS).astype(np.float32)).requires_grad_(True)
    ref = torch_voxel_sample_mv(ps, gm, z, v_cpu, True)
    # (the torch restatement is the reference computation: it reproduces the fixture's forward)
    chk = torch_voxel_sample_mv(ps, gm, z, volume_of(z).cpu(), True)
    np.testing.assert_allclose(chk.numpy(), z['stereo_td1'], rtol=1e-4, atol=1e-5)
    g = torch.from_numpy(rs.randn(*ref.shape).astype(np.float32))
    ref.backward(g)
    want = v_cpu.grad.numpy()

    def run():
        v = v_cpu.detach().cuda()
        v = (v.contiguous(memory_format=CL) if channels_last else v).requires_grad_(True)
        out = batched(pkg, gm, z, v, True, proj_invs=z['proj_inv'], memory_format=CL if out_cl else torch.contiguous_format)
        out.backward(g.cuda())
        assert v.grad.shape == v.shape and v.grad.is_contiguous(memory_format=CL if channels_last else torch.contiguous_format)
        return out.detach(), v.grad.cpu().numpy()
    out, got = run()
    assert np.abs(want).max() > 0.5
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5 * np.abs(want).max())
    # adjoint identity <A v2, g> == <v2, A^T g> for an independent v2, A from the forward under test
    v2 = torch.from_numpy(rs.randn(*v_cpu.shape).astype(np.float32))
    lhs = float((batched(pkg, gm, z, v2.cuda(), True, proj_invs=z['proj_inv']).double().cpu() * g.double()).sum())
    rhs = float((v2.double() * torch.from_numpy(got).double()).sum())
    assert abs(lhs - rhs) <= 1e-4 * max(1.0, abs(lhs)), (lhs, rhs)
    # the views of a sample are summed with fp32 atomics: two runs agree within the same bar, not bit for bit
    _, again = run()
    np.testing.assert_allclose(again, got, rtol=1e-4, atol=1e-5 * np.abs(want).max())


def test_backward_bf16_channels_last(pkg, gm, z):
    """the fast path's layout: bf16 NDHWC volume and result; the gradient is the fp32 sum rounded once"""
    rs = np.random.RandomState(6)
    v32 = torch.from_numpy(rs.randn(gm.B, gm.C, *gm.N_VOXELS).astype(np.float32)).cuda().bfloat16()
    g = torch.from_numpy(rs.randn(gm.B * gm.NV, gm.C, 2, 6, 8).astype(np.float32)).cuda().bfloat16()
    a = v32.float().requires_grad_(True)
    batched(pkg, gm, z, a, True).backward(g.float())
    b = v32.contiguous(memory_format=CL).requires_grad_(True)
    batched(pkg, gm, z, b, True, memory_format=CL).backward(g)
    assert b.grad.dtype == torch.bfloat16 and b.grad.is_contiguous(memory_format=CL)
    want = a.grad
    assert float((b.grad.float() - want).abs().max()) <= BF16_BAR * float(want.abs().max())


def head_of(pkg, gm, loss_type):
    head = pkg.registry.build_head(dict(
        type='DepthHead', depth_cfg=dict(gm.HEAD_DEPTH_CFG), in_channels=gm.C, with_convs=True,
        depth_loss=dict(type=loss_type, loss_weight=1.0), downsample_factor=gm.DS, num_views=gm.NV))
    head.load_state_dict(util.synthetic_state_dict(head, gm.HEAD_SEED))
    return head.cuda()


@pytest.mark.parametrize('loss_type,key', [('ce', 'loss_ce'), ('gaussian_1.5', 'loss_gaussian')])
def test_depth_head_multiview_fp32_vs_reference_fixture(pkg, gm, z, loss_type, key):
    head = head_of(pkg, gm, loss_type)
    assert type(head.conv_depth).__name__ == 'MfmaConv3dTo1' and list(head.state_dict()) == ['conv_depth.weight']
    head.depth_samples = torch.from_numpy(z['depth_samples'])
    with torch.no_grad():
        vol, soft, pred = head(torch.from_numpy(z['stereo_td1']).cuda())
        loss = head.loss(pred.flatten(0, 1), vol.flatten(0, 1), torch.from_numpy(z['depth_img']).cuda().flatten(0, 1))
    assert vol.shape == z['head_vol'].shape and pred.shape == z['head_pred'].shape
    np.testing.assert_allclose(vol.cpu().numpy(), z['head_vol'], **CONV_TOL)
    np.testing.assert_allclose(soft.cpu().numpy(), z['head_soft'], **CONV_TOL)
    np.testing.assert_allclose(pred.cpu().numpy(), z['head_pred'], **CONV_TOL)
    np.testing.assert_allclose(float(loss), float(z[key]), **CONV_TOL)


def test_depth_head_bf16_ndhwc_runs_the_32_to_1_kernel(pkg, gm, z):
    cv = importlib.import_module('depth-from-motion_amd.conv3d')
    head = head_of(pkg, gm, 'ce').bfloat16()
    head.depth_samples = torch.from_numpy(z['depth_samples'])
    x = torch.from_numpy(z['stereo_td1']).cuda().bfloat16().contiguous(memory_format=CL)
    assert head.conv_depth.eligible(x), head.conv_depth.why_not(x)
    policy = cv.fallback_policy()
    cv.set_fallback_policy('raise')      # the kernel, or an error: never torch's convolution here
    try:
        with torch.no_grad():
            y = head.conv_depth(x)
            vol, soft, pred = head(x)
    finally:
        cv.set_fallback_policy(policy)
    ref = F.conv3d(x.float().cpu(), head.conv_depth.weight.detach().float().cpu(), padding=1)
    assert y.dtype == torch.bfloat16 and y.shape == ref.shape
    assert float((y.float().cpu() - ref).abs().max()) <= BF16_BAR * float(ref.abs().max())
    assert vol.shape == z['head_vol'].shape and vol.dtype == torch.bfloat16
    assert torch.isfinite(pred.float()).all()


def test_fast_path_with_a_depth_head_end_to_end(pkg, gm, z):
    """enable_fast_path(strict=True) on a MultiViewVoxelPath with a depth head; forward_with_depth and the loss"""
    from tests.test_voxel_sample_mv import DEPTH_CFG, DEPTH_HEAD, small_model
    small = pkg.MultiViewVoxelPath(small_model(True)).cuda().eval()
    rep = pkg.enable_fast_path(small, strict=True)       # 32 channels: conv_depth is the 32 -> 1 kernel's module
    assert 'depth_head' in rep['roots'] and small.depth_head.conv_depth.weight.dtype == torch.bfloat16
    with open(os.path.join(util.GOLDEN, 'configs_dfm.json')) as f:
        model = dict(json.load(f)['multiview-dfm_r101_dcn_2x16_waymoD5-3d-3class_camsync_10sweeps.py']['model'])
    model['anchor_generator'] = dict(model['anchor_generator'], ranges=[[-11.0, -15.0, -3.0, 11.0, 15.0, 3.0]])
    model['voxel_size'] = [1.0, 1.0, 0.5]
    model['depth_head'] = dict(DEPTH_HEAD, in_channels=128)   # two frames of 64 channels, concatenated
    model['depth_cfg'] = dict(DEPTH_CFG)
    path = pkg.MultiViewVoxelPath(model).cuda().eval()
    rep = pkg.enable_fast_path(path, strict=True)
    assert sorted(rep['roots']) == ['depth_head', 'neck_3d']
    sys.path.insert(0, util.GOLDEN)
    try:
        import make_golden as g1
    finally:
        sys.path.remove(util.GOLDEN)
    lidar2img = g1.waymo_like_cameras(5, 2, 77)
    meta = {'ori_lidar2img': [m for m in lidar2img], 'input_shape': (104, 156), 'img_shape': [(100, 150, 3)] * 10}
    feats = torch.randn(1, 10, 64, 26, 39, generator=torch.Generator().manual_seed(4)).cuda()
    with torch.no_grad():
        bev = path(feats, [dict(meta)], 5, 2)
        bev2, vol, soft, pred = path.forward_with_depth(feats, [dict(meta)], 5, 2)
        depth_img = torch.rand(1, 5, 104, 156, generator=torch.Generator().manual_seed(5)).cuda() * 14.0
        loss = path.loss_dense_depth(pred, vol, depth_img)
    assert torch.equal(bev, bev2) and bev.dtype == torch.float32 and bev.shape == (1, 256, 30, 22)
    assert vol.shape == soft.shape == (1, 5, 8, 104, 156) and pred.shape == (1, 5, 104, 156)
    assert torch.isfinite(pred.float()).all() and torch.isfinite(loss.float()) and float(loss) > 0
