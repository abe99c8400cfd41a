"""Detector-level drop-in of the hot path.

The reference's detectors wire the path's modules together and inject attributes into them:

  DfM.__init__                mmdet3d/models/detectors/dfm.py:30-112 (attribute injection :82-100)
  DfM.extract_feat / forward  dfm.py:268-356
  MultiViewDfM.feature_transformation   mmdet3d/models/detectors/multiview_dfm.py:119-268

Three ways to use this package from there, all routed to the HIP kernels:

1. ``patch_reference()`` -- inside a real mmdet3d installation: re-registers the module
   classes (``DfMBackbone``, ``FrustumToVoxel``, ``DepthHead``, ``OutdoorImVoxelNeck``,
   ``DfMNeck``, ``BEVHourglass``, ``SPPUNetNeck``, and the loss ``IOU3DLoss``) under the same
   ``type`` names (force=True) so ``configs/dfm/*`` build them unchanged, rebinds the functions
   the reference modules call (``build_dfm_cost``, ``point_sample``, ``voxel_sample``, the NMS
   functions, ``diff_iou_rotated_3d`` and ``bbox_overlaps_nearest_3d`` where their modules are already
   imported), replaces ``MultiViewDfM.feature_transformation`` by
   ``MultiViewDfMMixin.feature_transformation`` and, where ``train_mixins`` is already imported,
   ``AnchorTrainMixin.anchor_target_3d`` by ``HipAnchorTrainMixin.anchor_target_3d`` and, where ``anchor3d_head`` is,
   ``Anchor3DHead.get_bboxes`` by ``HipAnchor3DHeadMixin.get_bboxes`` and ``loss_single`` of ``Anchor3DHead`` and
   of ``LIGAAnchor3DHead`` by ``HipAnchor3DLossMixin.loss_single``, and, where ``liga_atss_head`` is,
   ``LIGAATSSHead.get_targets`` by ``HipATSSTargetMixin.get_targets`` and ``LIGAATSSHead.loss`` by
   ``HipATSSLossMixin.loss``.  Where ``mmcv.ops`` is already imported its
   ``modulated_deform_conv2d`` is rebound and ``ModulatedDeformConv2dPack`` registered as ``'DCNv2'`` in mmcv's
   ``CONV_LAYERS``; likewise ``Voxelization``, ``SparseConvTensor``, ``SparseSequential`` and the layer types
   ``SubMConv3d`` / ``SparseConv3d`` of the LiDAR teacher (``LidarTeacher`` below), and
   ``DfM.extract_lidar_model_feat``; and ``depth_map_in_boxes_cpu`` / ``points_in_boxes_part`` / ``points_in_boxes_all``
   where the pipeline, the box structures and the detector hold them (``DfMDepthTargetMixin`` makes the depth loss's
   two target maps on the device when the loader did not supply them).
2. ``DfMStereoPath`` -- the KITTI student's path (neck -> backbone_stereo -> depth_head ->
   feature_transformation -> height compression -> backbone_3d) built from the ``model`` dict of
   ``configs/dfm/dfm_r34_1x8_kitti-3d-3class.py`` with the detector's attribute injection;
   usable without mmdet3d (this is what the tests and tools run).
3. ``MultiViewDfMMixin`` -- for a subclass ``class MultiViewDfM(MultiViewDfMMixin, RefMultiViewDfM)``.
"""
import importlib
import inspect
import sys
import types
from collections import namedtuple

import numpy as np
import torch
from torch import nn

from . import registry
from .fallback import REPLACED
from .box_nms import box3d_multiclass_nms, nms_bev, nms_normal_bev
from .iou3d_loss import diff_iou_rotated_3d
from .anchor_target import HipAnchorTrainMixin, bbox_overlaps_nearest_3d
from .bbox_decode import HipAnchor3DHeadMixin
from .anchor_loss import HipAnchor3DLossMixin
from .atss_target import HipATSSTargetMixin
from .atss_loss import HipATSSLossMixin
from .deform_conv import ModulatedDeformConv2dPack, modulated_deform_conv2d
from .sparse_conv import SparseConv3d, SparseConvTensor, SparseSequential, SubMConv3d, make_sparse_convmodule
from .voxelize import Voxelization
from . import kitti_eval as _kitti_eval
from . import depth_targets as _depth_targets
from . import optim as _optim
from ._launch import upload
from .geometry import prepare_coordinates_3d, prepare_depth
from .conv3d import MfmaConv3dTo1
from .graphs import GraphedCallable
from .plane_sweep import build_dfm_cost
from .streams import fork_join
from .point_sample import (mv_feature_transformation, point_sample, voxel_centers, voxel_sample,
                           voxel_sample_mv)


def inject_detector_attributes(detector, depth_cfg=None, voxel_cfg=None):
    """What DfM.__init__ writes onto its sub-modules after building them (dfm.py:82-100):
    ``backbone_stereo.downsampled_depth``, ``depth_head.depth_samples`` / ``.downsample_factor``,
    ``feature_transformation.depth_cfg`` / ``.coordinates_3d``.  ``detector`` is any object with
    those sub-modules as attributes (missing ones are skipped)."""
    if depth_cfg is not None:
        ds_factor = depth_cfg['downsample_factor']
        downsampled, depth = prepare_depth(depth_cfg)
        detector.downsampled_depth, detector.depth = downsampled, depth
        detector.depth_downsample_factor = ds_factor
        ft = getattr(detector, 'feature_transformation', None)
        if ft is not None and not inspect.ismethod(ft):   # (a method on the multi-view detectors)
            ft.depth_cfg = depth_cfg
        if getattr(detector, 'depth_head', None) is not None:
            if getattr(detector, 'backbone_stereo', None) is not None:   # (the multi-view path has none)
                detector.backbone_stereo.downsampled_depth = downsampled
            detector.depth_head.depth_samples = depth
            detector.depth_head.downsample_factor = ds_factor
    if voxel_cfg is not None:
        coords = prepare_coordinates_3d(voxel_cfg)
        detector.coordinates_3d = coords
        ft = getattr(detector, 'feature_transformation', None)
        if ft is not None:
            ft.coordinates_3d = coords
    return detector


def bev_view(vol):
    """``volume_feat.reshape(-1, C * Nz, Ny, Nx)`` (detectors/dfm.py: the voxel volume seen from above,
    height folded into the channels).  On the GPU the copy this reshape needs anyway (the volume is
    channels_last_3d) lands directly in NHWC, the layout BEVHourglass's 2-D convolutions run in."""
    B, C, nz, ny, nx = vol.shape
    if not vol.is_cuda:
        return vol.reshape(B, C * nz, ny, nx)
    return vol.permute(0, 3, 4, 1, 2).reshape(B, ny, nx, C * nz).permute(0, 3, 1, 2)


class DfMStereoPath(nn.Module):
    """The plane-sweep path of the ``DfM`` detector, built from its config ``model`` dict.

    ``forward(cur_feats, prev_feats, img_metas)`` takes the two image pyramids
    ``[img, *backbone(img)]`` (what dfm.py:281-284 hands to the neck) and returns what
    ``DfM.forward_train`` computes up to the detection head (dfm.py:268-322):
    ``dict(mono_stereo_costs, stereo_feats, mono_feats, upsample_costs, upsample_costs_softmax,
    depth_preds, volume_feat, bev_feat_prehg, bev_feat)``.  ``loss_dense_depth(out, depth_img,
    depth_fgmask_img)`` is dfm.py:348-356.
    """

    def __init__(self, model_cfg):
        super().__init__()
        cfg = {k: (dict(v) if isinstance(v, dict) else v) for k, v in model_cfg.items()}
        depth_cfg, voxel_cfg = cfg.get('depth_cfg'), cfg.get('voxel_cfg')
        self.neck = registry.build_neck(cfg['neck'])
        bs = cfg['backbone_stereo']
        if depth_cfg is not None:
            bs.update(depth_cfg=depth_cfg)                       # dfm.py:45-47
        self.backbone_stereo = registry.build_backbone(bs)
        ft = cfg.get('feature_transformation')
        if ft is not None:
            ft.update(cat_img_feature=self.neck.cat_img_feature,     # dfm.py:56-64
                      in_sem_channels=self.neck.sem_channels[-1])
            self.feature_transformation = registry.build_neck(ft)
        self.depth_head = registry.build_head(cfg['depth_head']) if cfg.get('depth_head') else None
        self.backbone_3d = registry.build_backbone(cfg['backbone_3d']) if cfg.get('backbone_3d') else None
        inject_detector_attributes(self, depth_cfg, voxel_cfg)
        # inference-time DepthHead -> FrustumToVoxel fusion; set False to get
        # the materialised upsample_costs / upsample_costs_softmax in eval mode as well
        self.fuse_depth_head = True
        # inference: replay the launch-bound 2-D necks (SPPUNetNeck, BEVHourglass) as hipGraphs
        # (graphs.py); opt-in -- the graphs keep static input / output buffers per input signature
        self.hip_graphs = False
        self._graphed = {}

    two_streams = True   # False: the previous frame's necks on the current stream too

    def _run_2d(self, name, module, tensors):
        """module(tensors) -- through a captured hipGraph when ``hip_graphs`` is on and nothing records
        gradients.  Each call site has its own graph (the outputs are static buffers: the neck's
        results for the current frame must survive its call on the previous frame)."""
        if not (self.hip_graphs and not torch.is_grad_enabled() and not self.training and tensors[0].is_cuda):
            return module(tensors) if name.startswith('neck') else module(tensors[0])
        g = self._graphed.get(name)
        if g is None:
            fn = (lambda ts: module(ts)) if name.startswith('neck') else (lambda ts: module(ts[0]))
            g = self._graphed[name] = GraphedCallable(fn)
        return g(tensors)

    def forward(self, cur_feats, prev_feats, img_metas):
        # the two frames' 2-D necks are independent calls of the same module: at inference (eval mode: no running
        # statistics to update, nothing recorded) the previous frame's runs on a side HIP stream
        (cur_stereo, cur_sem), (prev_stereo, _) = fork_join(
            lambda: self._run_2d('neck_cur', self.neck, list(cur_feats)),
            lambda: self._run_2d('neck_prev', self.neck, list(prev_feats)), cur_feats[0].device,
            fork=self.two_streams and not torch.is_grad_enabled() and not self.training)
        dev = cur_stereo.device
        for meta in img_metas:  # dfm.py:288-293: (N-1,4,4) tensors on the device
            meta['cur2prevs'] = torch.as_tensor(np.asarray(meta['cur2prevs'], dtype=np.float32)
                                                if not torch.is_tensor(meta['cur2prevs'])
                                                else meta['cur2prevs'], dtype=torch.float32).to(dev)
        costs, stereo_feats, mono_feats = self.backbone_stereo(cur_stereo, prev_stereo, img_metas)
        out = dict(mono_stereo_costs=costs, stereo_feats=stereo_feats, mono_feats=mono_feats,
                   cur_sem_feat=cur_sem)
        if self.depth_head is not None:
            # the depth head is fused into FrustumToVoxel's sampling kernel: the distribution is never
            # materialised.  Inference: upsample_costs is None.  Training: upsample_costs is the lazy
            # distribution, which DepthHead.loss (dfm.py:348-356) evaluates from the low-resolution cost;
            # the l1 losses differentiate depth_preds and keep the materialised head.
            fuse = (self.fuse_depth_head and hasattr(self, 'feature_transformation') and
                    not self.depth_head.with_convs and
                    (not torch.is_grad_enabled() or self.depth_head.depth_loss_type not in ('l1', 'purel1')))
            up, preds, soft = self.depth_head(costs, lazy=True) if fuse else \
                (lambda v, s, p: (v, p, s))(*self.depth_head(costs))
            out.update(upsample_costs=up, upsample_costs_softmax=soft, depth_preds=preds)
            if hasattr(self, 'feature_transformation'):
                vol = self.feature_transformation(stereo_feats, soft, img_metas, cur_sem)
                out['volume_feat'] = vol
                if self.backbone_3d is not None:
                    _, cv, nz, ny, nx = vol.shape
                    out['bev_feat_prehg'], out['bev_feat'] = self._run_2d('bev', self.backbone_3d, [bev_view(vol)])
        return out

    def loss_dense_depth(self, out, depth_img, depth_fgmask_img=None):
        if depth_fgmask_img is not None:
            depth_fgmask_img = depth_fgmask_img.flatten(start_dim=0, end_dim=1)
        return self.depth_head.loss(out['depth_preds'].flatten(start_dim=0, end_dim=1),
                                    out['upsample_costs'].flatten(start_dim=0, end_dim=1),
                                    depth_img.flatten(start_dim=0, end_dim=1),
                                    depth_fgmask_img=depth_fgmask_img)

    def depth_targets(self, points, gt_bboxes_3d, img_metas, projs=None):
        """``(depth_img, depth_fgmask_img)``, (B, 1, H, W) float32 and int32, of a batch -- what the pipeline step
        ``GenerateDepthMap(generate_fgmask=True)`` hands to ``forward_train``, made on the device from what reaches it
        anyway: ``points`` (the list of clouds the LiDAR teacher voxelizes: the pipeline's point filters keep
        ``rect_points`` in step with it, transforms_3d.py:1038-1039), ``gt_bboxes_3d`` (a list of box sets or objects
        with a ``.tensor``; on the host, where the loader leaves them, or on the device) and the metas' ``cam2img``,
        ``img_shape`` and ``pad_shape``.  ``projs``: the 3x4 projection of each sample, default ``cam2img[:3]`` --
        the reference projects with ``calib.P2``, a second copy of that
        matrix which the augmentations keep equal to it.  One memset and two launches of this package's kernels, no
        host wait (``depth_targets.counters()``)."""
        return depth_targets_from_metas(points, gt_bboxes_3d, img_metas, projs)


def _boxes_beside(boxes, device):
    """the first 7 columns of one sample's boxes as float32 on ``device``.  The loader leaves ``gt_bboxes_3d`` on the
    host (``DefaultFormatBundle3D`` wraps box objects ``cpu_only``) and the reference moves them itself where it needs
    them (dfm.py:480-483); here the copy is pinned and non-blocking, so the host does not wait for the stream"""
    t = getattr(boxes, 'tensor', boxes)
    if not torch.is_tensor(t):
        t = torch.as_tensor(np.asarray(t))
    t = t[:, :7]
    if t.device == device:
        return t
    if t.shape[0] == 0:
        return torch.empty((0, 7), dtype=t.dtype, device=device)
    return upload(t, device)


def depth_targets_from_metas(points, gt_bboxes_3d, img_metas, projs=None):
    """the arguments of ``generate_depth_targets`` read from ``img_metas``; every sample shares one ``pad_shape``.  With
    the clouds on a GPU, box sets that are still on the host are copied beside them"""
    points, boxes = list(points), list(gt_bboxes_3d)
    if points and torch.is_tensor(points[0]) and points[0].is_cuda:
        boxes = [_boxes_beside(b, points[0].device) for b in boxes]
    cam2imgs = [_depth_targets._host_matrix(meta['cam2img'], 'cam2img') for meta in img_metas]
    pads = {tuple(int(v) for v in tuple(meta['pad_shape'])[:2]) for meta in img_metas}
    if len(pads) != 1:
        raise ValueError(f'the samples of a batch share one pad_shape, got {sorted(pads)}')
    if projs is None:
        projs = cam2imgs
    return _depth_targets.generate_depth_targets(points, boxes, projs, cam2imgs,
                                                 [meta['img_shape'] for meta in img_metas], pads.pop())


class DfMDepthTargetMixin:
    """``forward_train`` of ``DfM`` (dfm.py:300-310) that makes ``depth_img`` / ``depth_fgmask_img`` on the device from
    ``points`` when the loader did not supply them (a train pipeline without ``GenerateDepthMap``, whose mask half needs
    mmcv's compiled ``points_in_boxes_cpu``), then defers to the host class:
    ``class FastDfM(DfMDepthTargetMixin, DfM)``.  What the loader supplied is left as it is."""

    def forward_train(self, img, img_metas, gt_bboxes_3d, gt_labels_3d, gt_bboxes=None, depth_img=None,
                      depth_fgmask_img=None, points=None, centers2d=None, **kwargs):
        if depth_img is None and points is not None and getattr(self, 'with_depth_head', True):
            depth_img, mask = depth_targets_from_metas(points, gt_bboxes_3d, img_metas)
            if depth_fgmask_img is None:
                depth_fgmask_img = mask
        return super().forward_train(img, img_metas, gt_bboxes_3d, gt_labels_3d, gt_bboxes=gt_bboxes,
                                     depth_img=depth_img, depth_fgmask_img=depth_fgmask_img, points=points,
                                     centers2d=centers2d, **kwargs)


class MultiViewDfMMixin:
    """``feature_transformation`` of ``MultiViewDfM`` (multiview_dfm.py:119-268) on the HIP path:
    one launch per batch lifts all (frame, view) feature maps into the voxel volume (sampling,
    valid-count reduction over views and frames, permute), then ``backbone_3d`` / ``neck_3d`` /
    the optional ``voxel_sample`` for the depth head run as in the reference.  The host class
    provides n_voxels, voxel_range, voxel_size, valid_sample, temporal_aggregate,
    transform_depth and the usual with_* properties."""

    def feature_transformation(self, batch_feats, img_metas, num_views, num_frames):
        # bf16 features: the volume is written channels-last, the layout the MFMA convolutions of
        # neck_3d read (no conversion copy); ``volume_memory_format`` on the host class overrides
        fast = getattr(self, 'fast_dtype', None)   # set by enable_fast_path(): lift in bf16 / NDHWC
        out_dtype = batch_feats.dtype
        if fast is not None and batch_feats.is_floating_point() and batch_feats.dtype != fast:
            batch_feats = batch_feats.to(fast)     # the view features, not the volume: Nv*F small maps
        fmt = getattr(self, 'volume_memory_format', None)
        if fmt is None:
            fmt = torch.channels_last_3d if batch_feats.dtype == torch.bfloat16 else torch.contiguous_format
        volume_feat = mv_feature_transformation(batch_feats, img_metas, num_views, num_frames,
                                                self.voxel_range, self.n_voxels,
                                                self.temporal_aggregate,
                                                valid_sample=getattr(self, 'valid_sample', True),
                                                memory_format=fmt)
        if getattr(self, 'with_backbone_3d', False):
            outputs = self.backbone_3d(volume_feat)
            volume_feat = outputs[0]
            if self.backbone_3d.output_bev:
                bev_feat = outputs[-1]
        batch_stereo_feats = None
        if getattr(self, 'with_depth_head', False):
            # every (sample, view) frustum in one launch, read from the volume where it lies and written at its
            # final offset: the bits of the reference's voxel_sample loop + torch.cat (multiview_dfm.py:220-256)
            td = self.transform_depth
            conv = getattr(self.depth_head, 'conv_depth', None)
            to1 = volume_feat.dtype == torch.bfloat16 and isinstance(conv, MfmaConv3dTo1)
            batch_stereo_feats = voxel_sample_mv(
                volume_feat, self.voxel_range, self.voxel_size,
                torch.as_tensor(self.depth_samples, dtype=torch.float32),
                [meta['ori_lidar2img'][:num_views] for meta in img_metas],
                self.depth_head.downsample_factor,
                [meta.get('scale_factor', 1.0) if td else 1.0 for meta in img_metas],
                [meta.get('img_crop_offset', 0) if td else 0 for meta in img_metas],
                [meta.get('flip', False) if td else False for meta in img_metas],
                [meta['input_shape'] if td else meta['ori_shape'][:2] for meta in img_metas],
                [[meta['img_shape'][v][:2] for v in range(num_views)] for meta in img_metas], num_views,
                # the layout the depth head's 32 -> 1 kernel reads; the values do not depend on it
                memory_format=torch.channels_last_3d if to1 else torch.contiguous_format)
        if getattr(self, 'with_neck_3d', False):
            if getattr(self, 'with_backbone_3d', False) and self.backbone_3d.output_bev:
                volume_feat = self.neck_3d(bev_feat)[1]
            else:
                volume_feat = self.neck_3d(volume_feat)[0]
        if fast is not None and volume_feat.dtype != out_dtype:
            # the caller's dtype at the path's exit (a (B, C_out, Ny, Nx) BEV map: small)
            volume_feat = volume_feat.to(out_dtype)
            if batch_stereo_feats is not None:
                batch_stereo_feats = batch_stereo_feats.to(out_dtype)
        out = (volume_feat, )
        if batch_stereo_feats is not None:
            out += (batch_stereo_feats, )
        return out


class DfMLidarTeacherMixin:
    """``extract_lidar_model_feat`` of ``DfM`` (dfm.py:373-382) on the HIP path, same signature, for a detector whose
    ``lidar_model`` holds this package's ``voxel_layer`` / ``voxel_encoder`` / ``middle_encoder`` / ``backbone`` (a
    ``LidarTeacher``, or the reference's VoxelNet built after ``patch_reference()``): batched voxelization with the
    batch size taken from the list, no ``.item()``."""

    @torch.no_grad()
    def extract_lidar_model_feat(self, points):
        lm = self.lidar_model
        if not hasattr(lm.voxel_layer, 'forward_batch'):   # a teacher built from mmcv's classes: the reference's method
            return REPLACED['DfM.extract_lidar_model_feat'](self, points)
        voxels, coors, num_points, _ = lm.voxel_layer.forward_batch(list(points))
        voxel_features = lm.voxel_encoder(voxels, num_points, coors)
        spatial_feat, volume_feat = lm.middle_encoder(voxel_features, coors, len(points))
        return volume_feat, lm.backbone(spatial_feat)


class DfMImitationMixin(DfMLidarTeacherMixin):
    """``extract_lidar_model_feat`` (from ``DfMLidarTeacherMixin``) and ``get_imitation_reg_layer_loss`` of ``DfM``
    (dfm.py:468-540) on the HIP path, for a subclass of the
    reference detector (``class FastDfM(DfMImitationMixin, DfM)``): one fused launch instead of
    ``points_in_boxes_part`` and the gather / normalise / reduce passes.  The host class provides
    ``bbox_head_3d.anchors``, ``norm_imitation`` and ``normalizer_clamp_value`` as the reference does; the
    second return value is the info dict of ``imitation_reg_layer_loss`` (no ``.item()`` logging values)."""

    def get_imitation_reg_layer_loss(self, features_preds, features_targets, imitation_cfg, gt_bboxes_3d):
        from .imitation import imitation_reg_layer_loss
        points = self.bbox_head_3d.anchors[0][:, :, :, 0, 0, :3]
        return imitation_reg_layer_loss(
            features_preds, features_targets, imitation_cfg, gt_bboxes_3d, points,
            norm_layer=self.norm_imitation[imitation_cfg['stereo_feature_layer']],
            normalizer_clamp_value=self.normalizer_clamp_value, training=self.training)


class LidarTeacher(nn.Module):
    """The frozen LiDAR teacher of the KITTI configs from their ``lidar_model`` dict (``type='VoxelNet'``:
    ``voxel_layer``, ``voxel_encoder=HardSimpleVFE``, ``middle_encoder=CustomSparseEncoder``,
    ``backbone=BEVHourglass``), without mmdet3d.  Submodule names are VoxelNet's (``voxel_layer``, ``voxel_encoder``,
    ``middle_encoder``, ``backbone``), so a teacher checkpoint's keys load as they are.

    ``forward(points_list)`` -> ``(volume_feat (B, C, D, H, W), bev_feat)``, what ``DfM.extract_lidar_model_feat``
    (dfm.py:373-382) returns: batched voxelization -> VFE -> sparse encoder -> BEV hourglass.  The batch size is the
    length of the list (the reference reads it back from ``coors[-1, 0].item()``), row counts stay on the device:
    NO host wait.  Forward only and always in eval mode, as the reference forces it (dfm.py:72-76, 111-116):
    parameters are frozen and ``train()`` leaves every module in ``eval()``."""

    def __init__(self, lidar_model_cfg):
        super().__init__()
        cfg = dict(lidar_model_cfg)
        kind = cfg.pop('type', 'VoxelNet')
        if kind != 'VoxelNet':
            raise KeyError(f'LidarTeacher builds a VoxelNet teacher, got type={kind!r}')
        for stage in ('neck', 'bbox_head'):
            if cfg.get(stage) is not None:
                raise NotImplementedError(f'LidarTeacher: lidar_model.{stage} is not None (the configs set it to None)')
        self.voxel_layer = Voxelization(**cfg['voxel_layer'])
        self.voxel_encoder = registry.build(cfg['voxel_encoder'])
        self.middle_encoder = registry.build(cfg['middle_encoder'])
        backbone = dict(cfg['backbone'])
        if (backbone.get('norm_cfg') or {}).get('type') == 'SyncBN':
            # eval only: a SyncBN is a BatchNorm2d here, under the same sub-module name ('bn') and keys
            backbone['norm_cfg'] = dict(backbone['norm_cfg'], type='BN')
        self.backbone = registry.build_backbone(backbone)
        if not getattr(self.middle_encoder, 'output_volume_feat', False):
            raise ValueError('LidarTeacher needs middle_encoder.output_volume_feat=True (the imitation loss reads the '
                             'volume features)')
        for param in self.parameters():
            param.requires_grad_(False)
        self.train(False)

    def train(self, mode=True):
        return super().train(False)   # the teacher is eval only

    @torch.no_grad()
    def forward(self, points_list):
        if isinstance(points_list, torch.Tensor):
            points_list = [points_list]
        voxels, coors, num_points, _ = self.voxel_layer.forward_batch(list(points_list))
        voxel_features = self.voxel_encoder(voxels, num_points, coors)
        spatial_feat, volume_feat = self.middle_encoder(voxel_features, coors, len(points_list))
        return volume_feat, self.backbone(spatial_feat)

    def check_status(self):
        """ONE host wait: raises ``DfmHipError`` when the last forward's index kernels reported a problem"""
        self.middle_encoder.check_status()


class MultiViewVoxelPath(MultiViewDfMMixin, nn.Module):
    """The multi-view path of ``MultiViewDfM`` from its config ``model`` dict (neck_3d,
    voxel_size, anchor_generator.ranges, temporal_aggregate, optionally depth_head + depth_cfg), without
    mmdet3d: voxel lifting + the 3-D neck.  ``forward(batch_feats (B, Nv*F, C, Hf, Wf), img_metas, num_views,
    num_frames)`` -> BEV feature (B, C_out, Ny, Nx).

    With a ``depth_head`` in the config (depth supervision, multiview_dfm.py:218-256, 296-304):
    ``forward_with_depth(...)`` -> (bev_feat, depth_volumes, depth_softmax, depth_preds), the last three
    (B, Nv, ...) as ``DepthHead.forward`` returns them, and ``loss_dense_depth(depth_preds, depth_volumes,
    depth_img)``."""

    def __init__(self, model_cfg):
        super().__init__()
        self.voxel_size = list(model_cfg['voxel_size'])
        self.voxel_range = list(model_cfg['anchor_generator']['ranges'][0])
        self.n_voxels = [round((self.voxel_range[3 + i] - self.voxel_range[i]) / self.voxel_size[i])
                         for i in range(3)]                      # multiview_dfm.py:54-61
        self.valid_sample = model_cfg.get('valid_sample', True)
        self.temporal_aggregate = model_cfg.get('temporal_aggregate', 'mean')
        self.transform_depth = model_cfg.get('transform_depth', True)
        self.neck_3d = registry.build_neck(dict(model_cfg['neck_3d']))
        self.with_neck_3d, self.with_backbone_3d, self.with_depth_head = True, False, False
        if model_cfg.get('depth_head'):
            depth_cfg = model_cfg.get('depth_cfg')
            if depth_cfg is None:
                raise KeyError("a model with a 'depth_head' needs 'depth_cfg' (dfm.py:79-92)")
            self.depth_head = registry.build_head(dict(model_cfg['depth_head']))
            self.with_depth_head = True
            inject_detector_attributes(self, depth_cfg)          # dfm.py:82-92
            self.depth_samples = self.depth                      # what feature_transformation samples at

    def forward(self, batch_feats, img_metas, num_views, num_frames):
        return self.feature_transformation(batch_feats, img_metas, num_views, num_frames)[0]

    def forward_with_depth(self, batch_feats, img_metas, num_views, num_frames):
        """-> (bev_feat, depth_volumes, depth_softmax, depth_preds): multiview_dfm.py:277-278, 297-298"""
        if not self.with_depth_head:
            raise RuntimeError("this MultiViewVoxelPath was built without a 'depth_head'")
        bev_feat, stereo_feat = self.feature_transformation(batch_feats, img_metas, num_views, num_frames)
        depth_volumes, depth_softmax, depth_preds = self.depth_head(stereo_feat)
        return bev_feat, depth_volumes, depth_softmax, depth_preds

    def loss_dense_depth(self, depth_preds, depth_volumes, depth_img):
        """multiview_dfm.py:299-303: depth_preds (B, Nv, H, W), depth_volumes (B, Nv, D, H, W), depth_img
        (B, Nv, H, W)"""
        return self.depth_head.loss(depth_preds.flatten(start_dim=0, end_dim=1),
                                    depth_volumes.flatten(start_dim=0, end_dim=1),
                                    depth_img.flatten(start_dim=0, end_dim=1))


# ---------------------------------------------------------------------------------------------
# patch_reference(): one table of named groups, three kinds of row, one applier per kind
# ---------------------------------------------------------------------------------------------
# (a) rebind the name ``attr`` of ``module`` to ``ours``; ``key``: where REPLACED keeps what was there (None: not kept)
Name = namedtuple('Name', 'module attr ours key load', defaults=(None, False))
# (b) rebind ``cls.method`` to ``mixin``'s, with every other function ``mixin`` defines (the helpers the method calls
# on ``self``); REPLACED['<cls>.<method>'] keeps what was there.  ``inherited``: ``cls`` need not define it itself
Method = namedtuple('Method', 'module cls method mixin inherited load', defaults=(False, False))
# (c) register ``ours`` as ``name`` (force=True) in the mmcv registry ``registry``, taken from the first of ``modules``
# that holds it (they hold the same object); ``key``: where REPLACED keeps the previous entry (None: not looked up)
Register = namedtuple('Register', 'modules registry name ours key load', defaults=(None, False))
# ``load``: the module may be imported for the purpose.  Otherwise a row applies only where its module is ALREADY
# imported: this package never drags in mmcv, mmdet or numba by itself.

_CONV_LAYER_MODULES = ('mmcv.cnn.bricks.registry', 'mmcv.cnn.bricks', 'mmcv.cnn')
_TEACHER_NAMES = dict(Voxelization=Voxelization, SparseConvTensor=SparseConvTensor, SparseSequential=SparseSequential,
                      SubMConv3d=SubMConv3d, SparseConv3d=SparseConv3d, make_sparse_convmodule=make_sparse_convmodule)


# the optimizer hook module holds torch's ``clip_grad`` MODULE and calls ``clip_grad.clip_grad_norm_``: it gets a
# namespace of its own in that place, torch's module is left as it is.
class _ClipGrad:
    clip_grad_norm_ = staticmethod(_optim.clip_grad_norm_)


def _rebind_clip_grad():
    hooks = _module('mmcv.runner.hooks.optimizer', True)
    if not hasattr(hooks, 'clip_grad'):
        return None
    hooks.clip_grad = _ClipGrad
    return 'functions', 'mmcv.runner.hooks.optimizer.clip_grad.clip_grad_norm_'


def _accept_staged_metas():
    # dfm.py:288-291 builds ``torch.tensor([img_meta['cur2prevs'] ...])``, which cannot take the device
    # tensors of a batch staged by data_geometry.stage_geometry: hand it host arrays (one 64-byte-per-
    # frame copy back; DfMStereoPath and the registered DfMBackbone read staged matrices in place)
    cls = getattr(_module('mmdet3d.models.detectors.dfm', True), 'DfM', None)
    extract_feat = getattr(cls, 'extract_feat', None)
    if extract_feat is None or getattr(extract_feat, '_dfm_staged_metas', False):
        return None
    cls.extract_feat = _extract_feat_with_staged_metas(extract_feat)
    return 'methods', 'DfM.extract_feat (accepts device-staged cur2prevs)'


def _rows(modules, names, **kwargs):
    """a Name row for every name in every module, module by module"""
    return [Name(m, attr, ours, **kwargs) for m in modules for attr, ours in names.items()]


PATCHES = {
    # the functions the reference's modules look up by name, and the files that define them
    'core': [Name(m, attr, ours, load=True) for m, attr, ours in (
        ('mmdet3d.models.backbones.dfm_backbone', 'build_dfm_cost', build_dfm_cost),
        ('mmdet3d.models.fusion_layers.point_fusion', 'point_sample', point_sample),
        ('mmdet3d.models.fusion_layers.point_fusion', 'voxel_sample', voxel_sample),
        ('mmdet3d.models.fusion_layers', 'point_sample', point_sample),
        ('mmdet3d.models.fusion_layers', 'voxel_sample', voxel_sample),
        ('mmdet3d.models.detectors.multiview_dfm', 'point_sample', point_sample),
        ('mmdet3d.models.detectors.multiview_dfm', 'voxel_sample', voxel_sample),
        ('mmdet3d.models.detectors.imvoxelnet', 'point_sample', point_sample))],
    # the BEV NMS functions (mmcv CUDA ops behind them in the reference) and every module that holds them by
    # name.  Not loaded: importing box3d_nms.py for this would drag in numba and mmcv.ops.
    'nms': _rows(('mmdet3d.core.post_processing.box3d_nms', 'mmdet3d.core.post_processing', 'mmdet3d.core',
                  'mmdet3d.models.dense_heads.anchor3d_head'),
                 dict(box3d_multiclass_nms=box3d_multiclass_nms, nms_bev=nms_bev, nms_normal_bev=nms_normal_bev)),
    # the reference's iou3d_loss.py holds mmcv's differentiable IoU by name (``from mmcv.ops import
    # diff_iou_rotated_3d``); its IOU3DLoss class itself is replaced through the registry.
    'iou': [Name('mmdet3d.models.losses.iou3d_loss', 'diff_iou_rotated_3d', diff_iou_rotated_3d)],
    # the KITTI evaluation: ``kitti_eval`` in every module that holds it by name, and ``rotate_iou_gpu_eval``
    # (numba.cuda in the reference) where it is defined.  The datasets import ``kitti_eval`` from
    # ``mmdet3d.core.evaluation`` at call time, so rebinding the names is enough.  Not loaded: eval.py imports numba.
    'kitti_eval': [
        *_rows(('mmdet3d.core.evaluation.kitti_utils.eval', 'mmdet3d.core.evaluation.kitti_utils',
                'mmdet3d.core.evaluation', 'mmdet3d.core'), dict(kitti_eval=_kitti_eval.kitti_eval)),
        Name('mmdet3d.core.evaluation.kitti_utils.rotate_iou', 'rotate_iou_gpu_eval', _kitti_eval.rotate_iou_eval)],
    # the depth loss's targets: ``depth_map_in_boxes_cpu`` where the pipeline holds it by name (its body calls mmcv's
    # compiled ``points_in_boxes_cpu``), and mmcv's ``points_in_boxes_part`` / ``_all`` where the box structures and
    # the detector imported them.
    'depth_targets': [
        *_rows(('mmdet3d.datasets.utils', 'mmdet3d.datasets.pipelines.transforms_3d'),
               dict(depth_map_in_boxes_cpu=_depth_targets.depth_map_in_boxes)),
        *_rows(('mmdet3d.core.bbox.structures.base_box3d', 'mmdet3d.models.detectors.dfm'),
               dict(points_in_boxes_part=_depth_targets.points_in_boxes_part,
                    points_in_boxes_all=_depth_targets.points_in_boxes_all))],
    # the optimizer step: ``FusedAdamW`` into mmcv's OPTIMIZERS registry (a config names it ``type='FusedAdamW'``),
    # and the clip of ``OptimizerHook.clip_grads``.  Loaded: the runner imports both modules anyway.
    'optimizer': [Register(('mmcv.runner.optimizer',), 'OPTIMIZERS', 'FusedAdamW', _optim.FusedAdamW, load=True),
                  _rebind_clip_grad],
    # the anchor head's target assignment: the modules that hold bbox_overlaps_nearest_3d by name, and
    # AnchorTrainMixin.anchor_target_3d of the reference's train_mixins.py.  Not loaded: these files import mmdet.
    'anchor_target': [
        *_rows(('mmdet3d.core.bbox.iou_calculators.iou3d_calculator', 'mmdet3d.core.bbox.iou_calculators',
                'mmdet3d.core.bbox', 'mmdet3d.core'), dict(bbox_overlaps_nearest_3d=bbox_overlaps_nearest_3d)),
        Method('mmdet3d.models.dense_heads.train_mixins', 'AnchorTrainMixin', 'anchor_target_3d', HipAnchorTrainMixin)],
    # the anchor head's inference side: Anchor3DHead.get_bboxes (inherited by LIGAAnchor3DHead).  Not loaded:
    # anchor3d_head.py imports mmdet.
    'anchor_head': [Method('mmdet3d.models.dense_heads.anchor3d_head', 'Anchor3DHead', 'get_bboxes',
                           HipAnchor3DHeadMixin)],
    # the anchor head's training side: loss_single of Anchor3DHead AND of LIGAAnchor3DHead (the subclass overrides
    # it, so both are rebound and each keeps its own).  Not loaded: both files import mmdet.
    'anchor_loss': [Method('mmdet3d.models.dense_heads.anchor3d_head', 'Anchor3DHead', 'loss_single',
                           HipAnchor3DLossMixin),
                    Method('mmdet3d.models.dense_heads.liga_anchor3d_head', 'LIGAAnchor3DHead', 'loss_single',
                           HipAnchor3DLossMixin)],
    # the 2-D ATSS head's target assignment: LIGAATSSHead inherits get_targets from mmdet's ATSSHead; the class gets
    # this package's method, the inherited one is kept.  mmdet's bbox_overlaps is rebound nowhere.  Not loaded:
    # liga_atss_head.py imports mmdet.
    'atss_target': [Method('mmdet3d.models.dense_heads.liga_atss_head', 'LIGAATSSHead', 'get_targets',
                           HipATSSTargetMixin, inherited=True)],
    # the 2-D ATSS head's loss: LIGAATSSHead inherits loss from mmdet's ATSSHead and overrides loss_single; the class
    # gets this package's loss (targets and all levels' terms without leaving the device), the inherited one is kept
    # and still finds the reference's loss_single.  A group of its own: 'atss_target' reports get_targets alone.  Not
    # loaded: liga_atss_head.py imports mmdet.
    'atss_loss': [Method('mmdet3d.models.dense_heads.liga_atss_head', 'LIGAATSSHead', 'loss', HipATSSLossMixin,
                         inherited=True)],
    # the backbone's deformable convolutions (the Waymo configs' ResNet-101 with dcn=dict(type='DCNv2')): mmcv's
    # function is rebound in the modules that hold it by name, and the Pack is registered as 'DCNv2' in mmcv's
    # CONV_LAYERS, which is where mmdet's ResNet builds its dcn layers from.  Not loaded: this package never imports
    # mmcv.
    'deform_conv': [
        *_rows(('mmcv.ops.modulated_deform_conv', 'mmcv.ops'), dict(modulated_deform_conv2d=modulated_deform_conv2d),
               key='modulated_deform_conv2d'),
        Register(_CONV_LAYER_MODULES, 'CONV_LAYERS', 'DCNv2', ModulatedDeformConv2dPack, key='DCNv2')],
    # the LiDAR teacher's ops: mmcv's Voxelization and spconv wrapper classes are rebound in the modules that hold
    # them by name, the layer types registered in mmcv's CONV_LAYERS (where make_sparse_convmodule builds them from),
    # and ``DfM.extract_lidar_model_feat``.  Not loaded: this package never imports mmcv or mmdet3d.
    'lidar_teacher': [
        *(Name(m, attr, ours, key=f'{m}.{attr}') for m in (
            'mmcv.ops', 'mmcv.ops.voxelize', 'mmcv.ops.sparse_conv', 'mmcv.ops.sparse_structure',
            'mmcv.ops.sparse_modules', 'mmdet3d.ops', 'mmdet3d.ops.sparse_block',
            'mmdet3d.models.middle_encoders.sparse_encoder', 'mmdet3d.models.detectors.voxelnet')
          for attr, ours in _TEACHER_NAMES.items()),
        Register(_CONV_LAYER_MODULES, 'CONV_LAYERS', 'SubMConv3d', SubMConv3d, key='CONV_LAYERS.SubMConv3d'),
        Register(_CONV_LAYER_MODULES, 'CONV_LAYERS', 'SparseConv3d', SparseConv3d, key='CONV_LAYERS.SparseConv3d'),
        Method('mmdet3d.models.detectors.dfm', 'DfM', 'extract_lidar_model_feat', DfMLidarTeacherMixin)],
    # the detectors themselves.  Loaded: patch_reference() is called to build them.
    'detectors': [Method('mmdet3d.models.detectors.multiview_dfm', 'MultiViewDfM', 'feature_transformation',
                         MultiViewDfMMixin, load=True),
                  _accept_staged_metas],
}


def _module(name, load):
    if not load:
        return sys.modules.get(name)
    try:
        return importlib.import_module(name)
    except ImportError:
        return None


def _apply_name(row):
    mod = _module(row.module, row.load)
    current = getattr(mod, row.attr, None)
    if current is None:
        return None
    if current is not row.ours:
        if row.key is not None:
            REPLACED[row.key] = current
        setattr(mod, row.attr, row.ours)
    return 'functions', f'{row.module}.{row.attr}'


def _apply_method(row):
    cls = getattr(_module(row.module, row.load), row.cls, None)
    if cls is None or not (hasattr(cls, row.method) if row.inherited else row.method in vars(cls)):
        return None
    ours = vars(row.mixin)
    if vars(cls).get(row.method) is not ours[row.method]:
        REPLACED[f'{cls.__name__}.{row.method}'] = getattr(cls, row.method)
        for name, fn in ours.items():
            if isinstance(fn, types.FunctionType):
                setattr(cls, name, fn)
    return 'methods', f'{row.cls}.{row.method}'


def _apply_register(row):
    for mod_name in row.modules:
        reg = getattr(_module(mod_name, row.load), row.registry, None)
        if reg is None:
            continue
        previous = reg.get(row.name) if row.key is not None else None
        if previous is not row.ours:
            if previous is not None:
                REPLACED[row.key] = previous
            reg.register_module(name=row.name, force=True, module=row.ours)
        return 'modules', f'{row.name} (mmcv {row.registry})'
    return None


_APPLIERS = {Name: _apply_name, Method: _apply_method, Register: _apply_register}


def apply_patches(group):
    """apply the rows of ``PATCHES[group]`` -> ``{'modules': [...], 'functions': [...], 'methods': [...]}``, what
    ``patch_reference()`` adds to its report for the group.  Applying a group again changes nothing and reports the
    same."""
    report = {'modules': [], 'functions': [], 'methods': []}
    for row in PATCHES[group]:
        done = row() if callable(row) else _APPLIERS[type(row)](row)
        if done is not None:
            report[done[0]].append(done[1])
    return report


def patch_reference(precision=None, strict=False):
    """Route a real mmdet3d (the reference fork) to the HIP path.  Call once after
    ``import mmdet3d`` and before building the model from ``configs/dfm/*``.  Returns a report
    dict {'modules': [...], 'functions': [...], 'methods': [...]}.  Raises ImportError when
    mmdet3d is not importable (this package never needs it otherwise).

    ``precision='bf16'``: every ``DfM`` / ``MultiViewDfM`` detector built afterwards is passed through
    ``enable_fast_path(detector, torch.bfloat16, strict=strict)`` at the end of its constructor, so
    the reference's fp32 pipeline reaches the MFMA kernels without another line of user code (the
    sampling / norm kernels run either way; without this switch the Mfma* convolutions of an fp32
    model run torch's convolution and say so once).  ``precision=None`` leaves models as built."""
    if precision not in (None, 'fp32', 'bf16'):
        raise ValueError(f'precision must be None, "fp32" or "bf16", got {precision!r}')
    report = {'modules': registry.register_into_mmdet3d(), 'functions': [], 'methods': []}
    for group in PATCHES:
        for kind, done in apply_patches(group).items():
            report[kind] += done
    if precision == 'bf16':
        report['methods'] += _fast_path_after_init(strict)
    return report


def _fast_path_after_init(strict):
    # every module of a detector is built inside DfM.__init__ (MultiViewDfM.__init__ calls it and
    # adds plain attributes only, multiview_dfm.py:36-65): converting at its end covers both
    cls = getattr(_module('mmdet3d.models.detectors.dfm', True), 'DfM', None)
    if cls is None:
        return []
    if not getattr(cls.__init__, '_dfm_fast', False):
        cls.__init__ = _init_then_fast_path(cls.__init__, strict)
        return ['DfM.__init__ -> enable_fast_path(bf16)']
    _patch_state['strict'] = bool(strict)   # patched before: the wrapper reads the strictness of the latest call
    return [f'DfM.__init__ already patched (strict={bool(strict)} from now on)']


def _extract_feat_with_staged_metas(extract_feat):
    def wrapped(self, img, img_metas, *args, **kwargs):
        for meta in img_metas:
            v = meta.get('cur2prevs')
            if torch.is_tensor(v):
                meta['cur2prevs'] = v.detach().cpu().numpy()
        return extract_feat(self, img, img_metas, *args, **kwargs)
    wrapped._dfm_staged_metas = True
    wrapped.__wrapped__ = extract_feat
    return wrapped


_patch_state = {'strict': False}  # the latest patch_reference(precision='bf16', strict=...) call decides


def _init_then_fast_path(init, strict):
    _patch_state['strict'] = bool(strict)

    def __init__(self, *args, **kwargs):
        init(self, *args, **kwargs)
        self.fast_path_report = enable_fast_path(self, torch.bfloat16, strict=_patch_state['strict'])
    __init__._dfm_fast = True
    __init__.__wrapped__ = init
    return __init__


# ---------------------------------------------------------------------------------------------
# the fast path, explicitly: bf16 / channels-last conversion of the path's modules inside a model
# ---------------------------------------------------------------------------------------------
def _map_tensors(obj, fn):
    if torch.is_tensor(obj):
        return fn(obj)
    if isinstance(obj, (list, tuple)):
        out = [_map_tensors(o, fn) for o in obj]
        return type(obj)(out) if not hasattr(obj, '_fields') else type(obj)(*out)
    return obj   # dicts are NOT entered: img_metas carry fp32 camera matrices / poses that must stay fp32


def _cast_hook(src, dst):
    """forward pre-hook: floating tensors of dtype ``src`` (or any floating dtype when src is None)
    among the positional / keyword arguments become ``dst``"""
    def cast(t):
        # feature maps and volumes only (>= 4-D): small fp32 geometry tensors pass through untouched
        if t.dim() >= 4 and t.is_floating_point() and t.dtype != dst and (src is None or t.dtype == src):
            return t.to(dst)
        return t

    def hook(module, args, kwargs):
        return _map_tensors(args, cast), {k: _map_tensors(v, cast) for k, v in kwargs.items()}
    return hook


def _is_norm(m):
    return isinstance(m, (nn.modules.batchnorm._BatchNorm, nn.GroupNorm))


def enable_fast_path(model, dtype=torch.bfloat16, strict=True, boundary_casts=True):
    """Route every convolution of the path inside ``model`` to the hand-written MFMA kernels.

    ``model``: a reference ``DfM`` / ``MultiViewDfM`` detector built after ``patch_reference()``, a
    ``DfMStereoPath`` / ``MultiViewVoxelPath``, or any ``nn.Module`` that contains this package's
    registered classes (the *path roots*: SPPUNetNeck, DfMBackbone, DepthHead, FrustumToVoxel,
    BEVHourglass, OutdoorImVoxelNeck, DfMNeck).  The reference pipeline runs fp32 / NCHW; the MFMA
    kernels take bf16 / channels-last.  This call

    * converts the convolution (and every other non-norm) parameter of the path roots to ``dtype``;
      GroupNorm / BatchNorm parameters and running statistics stay fp32 (the fused norm kernels and
      the folded epilogues read fp32);
    * sets ``DfMBackbone.volume_memory_format = channels_last_3d`` (the cost volume is built NDHWC)
      and marks a multi-view detector so its lifted voxel volume is written bf16 / NDHWC;
    * ``boundary_casts``: installs forward pre-hooks -- a path root casts floating inputs to ``dtype``;
      every OTHER child of a module that owns a path root (the 2-D backbone, the detection heads)
      casts ``dtype`` inputs back to the model's original floating dtype -- so the caller keeps feeding
      and receiving the tensors it did before;
    * ``strict`` (default True): every Mfma* module INSIDE ``model`` gets ``fallback_policy = 'raise'`` -- an
      input its kernel does not take (wrong dtype / layout, a shape no tiling fits) is an error there instead
      of a one-time warning and torch's convolution.  Per model: other models in the process keep the
      process-wide mode (fallback.set_fallback_policy; 'warn' by default).  ``strict=False`` leaves the
      modules' policy as it is.

    Returns a report dict(roots=[names], converted_parameters=n, cast_back=[names], dtype=...).
    Idempotent.  ``state_dict`` keys are unchanged; ``load_state_dict`` of an fp32 checkpoint casts
    on copy as usual."""
    from . import modules as _m
    path_classes = registry.path_classes()
    names = dict((m, n) for n, m in model.named_modules())
    roots, inside = [], set()
    for n, m in model.named_modules():
        if m in inside:
            continue
        if isinstance(m, path_classes):
            roots.append(m)
            inside.update(m.modules())
    orig = next((p.dtype for p in model.parameters() if p.is_floating_point() and p.dtype != dtype),
                torch.float32)
    converted = 0
    for root in roots:
        for sub in root.modules():
            if _is_norm(sub):
                continue
            for p in sub.parameters(recurse=False):
                if p.is_floating_point() and p.dtype != dtype:
                    p.data = p.data.to(dtype)
                    if p.grad is not None:
                        p.grad = None
                    converted += 1
            for k, b in sub.named_buffers(recurse=False):
                if b is not None and b.is_floating_point() and b.dtype != dtype:
                    setattr(sub, k, b.to(dtype))
        if isinstance(root, _m.DfMBackbone):
            root.volume_memory_format = torch.channels_last_3d
        if isinstance(root, _m.FrustumToVoxel) and not isinstance(model, DfMStereoPath):
            root.output_memory_format = torch.contiguous_format   # dfm.py:325-326 views the volume
    for m in model.modules():
        if isinstance(m, MultiViewDfMMixin) or \
                getattr(type(m), 'feature_transformation', None) is MultiViewDfMMixin.feature_transformation:
            m.fast_dtype = dtype
    cast_back = []
    if boundary_casts:
        for root in roots:
            if not root.__dict__.get('_dfm_fast_hook'):
                root.register_forward_pre_hook(_cast_hook(None, dtype), with_kwargs=True)
                root.__dict__['_dfm_fast_hook'] = True
        owners = [m for m in model.modules() if m not in inside and any(c in roots for c in m.children())]
        for owner in owners:
            for child in owner.children():
                if child in inside or any(sub in inside for sub in child.modules()):
                    continue
                if not child.__dict__.get('_dfm_fast_hook'):
                    child.register_forward_pre_hook(_cast_hook(dtype, orig), with_kwargs=True)
                    child.__dict__['_dfm_fast_hook'] = True
                cast_back.append(names.get(child, type(child).__name__))
    report = dict(roots=[names.get(r, type(r).__name__) for r in roots], converted_parameters=converted,
                  cast_back=cast_back, dtype=dtype, fallback_policy=None)
    if strict:
        from . import conv3d as _c
        kinds = (_c.MfmaConv3d, _c.MfmaConv3dG, _c.MfmaConvTranspose3d, _c.MfmaConv2d, _c.MfmaConvTranspose2d)
        n_strict = 0
        for root in roots:
            for sub in root.modules():
                if isinstance(sub, kinds):
                    sub.fallback_policy = 'raise'
                    n_strict += 1
        report['fallback_policy'] = f"'raise' on the {n_strict} Mfma* modules of this model"
    return report


__all__ = ['inject_detector_attributes', 'DfMStereoPath', 'MultiViewDfMMixin', 'MultiViewVoxelPath',
           'patch_reference', 'enable_fast_path', 'voxel_centers', 'HipAnchorTrainMixin']
