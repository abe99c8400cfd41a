"""Generate tests/golden/multiview_depth.npz: depth supervision of the multi-view detector, by running the
REFERENCE's own code on PyTorch-CPU (same rules as make_golden.py: the reference's functions are lifted from
their files by AST or executed by path under ref_stubs, unmodified; only inputs and the outputs they produced
are stored).

Run in the build container only (needs the reference checkout):   python tests/golden/make_golden_mvdepth.py

(The name does not start with ``mv_``: tests/test_point_sample_oracle.py takes every ``mv_*.npz`` for a lifting case.)

Pinned here:
  * ``MultiViewDfM.feature_transformation`` with ``with_depth_head`` (multiview_dfm.py:218-256): its
    ``batch_stereo_feats`` for B = 2 samples x Nv = 5 Waymo-like cameras sampling a 32-channel 20 x 24 x 6 voxel
    volume, both samples rescaled, the second one flipped and cropped; ``transform_depth`` True (all 32 channels:
    they feed the depth head below) and False (the original-size lattice is 4x larger: channels 0..3 of the
    reference's result are kept).  The volume is handed to the method through its ``backbone_3d`` hook, so the
    reference's own loop, including the ``voxel_sample`` calls and both ``torch.cat``, produces the result.
  * ``DepthHead(with_convs=True, num_views=5)`` (dense_heads/depth_head.py): ``forward`` on that result and ``loss``
    for 'ce' and 'gaussian_1.5' against a seeded depth image.
The volume is stored as int8 sixteenths (exact in fp32 and in bf16); the host inverses of the projections are
stored so that a replay is bit-exact on any CPU (LAPACK's last bits differ between CPU models).
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as mg  # noqa: E402

B, NV, C = 2, 5, 32
N_VOXELS = (20, 24, 6)
VOXEL_RANGE = [-10.0, -12.0, -2.0, 10.0, 12.0, 2.0]
VOXEL_SIZE = [1.0, 1.0, 2.0 / 3.0]
ORI_SHAPE, INPUT_SHAPE = (48, 64), (24, 32)
DS = 4
DEPTH_CFG = dict(mode='UD', num_bins=8, depth_min=1.0, depth_max=13.0, downsample_factor=DS)
HEAD_DEPTH_CFG = dict(mode='UD', num_bins=8, min_depth=1.0, max_depth=13.0)
KEPT_CHANNELS_TD0 = 4
HEAD_SEED, GAUSSIAN = 41, 'gaussian_1.5'


def cameras():
    """waymo_like_cameras (made for 104 x 156 images) with the intrinsics scaled to the 48 x 64 originals"""
    cams = mg.waymo_like_cameras(NV, B, 700).reshape(B, NV, 4, 4)   # "frames" = the samples of the batch
    s = np.diag([64.0 / 156.0, 48.0 / 104.0, 1.0, 1.0]).astype(np.float32)
    return np.stack([[s @ m for m in cams[b]] for b in range(B)]).astype(np.float32)


def metas(lidar2img):
    out = []
    for b in range(B):
        m = {'ori_lidar2img': [x for x in lidar2img[b]], 'input_shape': INPUT_SHAPE,
             'ori_shape': ORI_SHAPE + (3,), 'img_shape': [(INPUT_SHAPE[0] - b, INPUT_SHAPE[1] - 2 * b, 3)] * NV}
        if b == 0:
            m['scale_factor'] = 0.5
        else:
            m['scale_factor'] = np.array([0.48, 0.52, 0.48, 0.52], np.float32)
            m['flip'] = True
            m['img_crop_offset'] = np.array([3.0, 2.0], np.float32)
        out.append(m)
    return out


def depth_samples():
    interval = (DEPTH_CFG['depth_max'] - DEPTH_CFG['depth_min']) / DEPTH_CFG['num_bins']
    d = torch.zeros(DEPTH_CFG['num_bins'], dtype=torch.float32)
    for i in range(DEPTH_CFG['num_bins']):
        d[i] = (i + 0.5) * interval + DEPTH_CFG['depth_min']      # DfM.prepare_depth, dfm.py:170-172
    return d


def main():
    g = mg.load_reference()
    rng = np.random.RandomState(710)
    volume_q = rng.randint(-64, 65, size=(B, C) + N_VOXELS).astype(np.int8)
    volume = torch.from_numpy(volume_q.astype(np.float32) / 16.0)
    lidar2img = cameras()
    depths = depth_samples()
    gen_self = SimpleNamespace(align_corner=False, custom_values=[])

    def grid_anchors(featmap_sizes, device='cpu'):
        a = g['aligned_anchors_single_range'](gen_self, featmap_sizes[0], VOXEL_RANGE, 1, sizes=[[0.0, 0.0, 0.0]],
                                              rotations=[0.0], device=device)
        return [a.reshape(-1, a.size(-1))]

    def backbone_3d(_lifted):
        return [volume]
    backbone_3d.output_bev = False
    feats = torch.randn(B, NV, 2, 6, 8, generator=torch.Generator().manual_seed(711))
    out = {}
    for td in (True, False):
        self_ = SimpleNamespace(
            anchor_generator=SimpleNamespace(grid_anchors=grid_anchors), n_voxels=list(N_VOXELS),
            valid_sample=True, temporal_aggregate='mean', with_backbone_3d=True, backbone_3d=backbone_3d,
            with_depth_head=True, with_neck_3d=False, transform_depth=td, voxel_range=VOXEL_RANGE,
            voxel_size=VOXEL_SIZE, depth_samples=depths.tolist(), depth_head=SimpleNamespace(downsample_factor=DS))
        vol_out, stereo = g['mv_feature_transformation'](self_, feats, metas(lidar2img), NV, 1)
        assert vol_out is volume
        out[f'stereo_td{int(td)}'] = stereo
        print('transform_depth', td, tuple(stereo.shape), 'nonzero', float((stereo != 0).float().mean()))

    import ref_stubs
    from tests import util
    ref_stubs.install()
    dh = ref_stubs.load_file('mmdet3d/models/dense_heads/depth_head.py', 'ref_depth_head')
    dh.dist = SimpleNamespace(get_rank=lambda: 1)   # the 'gaussian' branch asks the rank to print once
    losses = {}
    gen = torch.Generator().manual_seed(712)
    depth_img = torch.rand(B, NV, *INPUT_SHAPE, generator=gen) * 14.0   # some pixels outside (min, max)
    for loss_type in ('ce', GAUSSIAN):
        m = dh.DepthHead(depth_cfg=HEAD_DEPTH_CFG, in_channels=C, with_convs=True,
                         depth_loss=dict(type=loss_type, loss_weight=1.0), downsample_factor=DS, num_views=NV)
        m.load_state_dict(util.synthetic_state_dict(m, HEAD_SEED))
        m.depth_samples = depths
        with torch.no_grad():
            vol, soft, pred = m(out['stereo_td1'])
            losses[loss_type] = m.loss(pred.flatten(0, 1), vol.flatten(0, 1), depth_img.flatten(0, 1))
    np.savez_compressed(
        os.path.join(HERE, 'multiview_depth.npz'), volume_q=volume_q, lidar2img=lidar2img,
        proj_inv=np.stack([[torch.inverse(torch.from_numpy(m_)).numpy() for m_ in lidar2img[b]] for b in range(B)]),
        voxel_range=np.asarray(VOXEL_RANGE, np.float32), voxel_size=np.asarray(VOXEL_SIZE, np.float32),
        depth_samples=depths.numpy(), stereo_td1=out['stereo_td1'].numpy(),
        stereo_td0=out['stereo_td0'][:, :KEPT_CHANNELS_TD0].contiguous().numpy(),
        head_vol=vol.numpy(), head_soft=soft.numpy(), head_pred=pred.numpy(), depth_img=depth_img.numpy(),
        loss_ce=np.float32(losses['ce']), loss_gaussian=np.float32(losses[GAUSSIAN]))
    print('depth head', tuple(vol.shape), tuple(pred.shape), {k: float(v) for k, v in losses.items()},
          os.path.getsize(os.path.join(HERE, 'multiview_depth.npz')), 'bytes')


if __name__ == '__main__':
    if not os.path.isdir(mg.REF):
        sys.exit('reference not mounted; the fixture is committed, nothing to do')
    torch.set_num_threads(1)
    main()
