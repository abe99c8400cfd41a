"""depth-from-motion_amd -- MI355X (gfx950) native plane-sweep cost-volume path
of Depth-from-Motion.

The directory name carries a hyphen (it is the project name); import it as
``import dfm_amd`` (alias module at the repo root) or
``importlib.import_module('depth-from-motion_amd')``.

Everything numerical runs in hand-written HIP kernels behind the C ABI of
``include/dfm_hip.h`` (``lib/libdfm_hip.so``).  There is NO CPU or eager
PyTorch fallback: if the shared library is missing or no GPU is visible the
ops raise.
"""
from . import _capi  # noqa: F401
from . import modules, registry  # noqa: F401  (registers the module classes)
from .plane_sweep import build_dfm_cost, plane_sweep_grid  # noqa: F401
from .depth_head import LazyDepthDistribution, depth_head_forward, depth_head_statistics  # noqa: F401
from .group_norm import HipGroupNorm, group_norm  # noqa: F401
from .geometry import prepare_coordinates_3d, prepare_depth  # noqa: F401
from .frustum_to_voxel import frustum_to_voxel_sample  # noqa: F401
from .integration import (DfMDepthTargetMixin, DfMImitationMixin, DfMLidarTeacherMixin, DfMStereoPath,  # noqa: F401
                          LidarTeacher,
                          MultiViewDfMMixin, MultiViewVoxelPath, enable_fast_path, inject_detector_attributes,
                          patch_reference)
from .fallback import MfmaPathError, fallback_policy, set_fallback_policy  # noqa: F401
from .conv3d import set_fp32_mode  # noqa: F401
from .depth_head import depth_distribution_loss  # noqa: F401
from .imitation import (ImitationLoss, NormalizeLayer, imitation_reg_layer_loss,  # noqa: F401
                        reduce_imitation_statistics)
from .box_nms import box3d_multiclass_nms, box_iou_rotated, nms_bev, nms_normal_bev  # noqa: F401
from .iou3d_loss import (IOU3DLoss, diff_iou_rotated_2d, diff_iou_rotated_3d, iou3d_loss,  # noqa: F401
                         iou3d_loss_from_deltas)
from .anchor_target import (BboxOverlapsNearest3D, HipAnchorTrainMixin, anchor_target_3d,  # noqa: F401
                            bbox_overlaps_nearest_3d)
from .bbox_decode import (HipAnchor3DHeadMixin, anchor3d_get_bboxes, anchor_head_candidates,  # noqa: F401
                          delta_xyzwlhr_decode)
from .anchor_loss import HipAnchor3DLossMixin, anchor3d_loss  # noqa: F401
from .atss_target import BboxOverlaps2D, HipATSSTargetMixin, atss_target_2d, bbox_overlaps  # noqa: F401
from .atss_loss import HipATSSLossMixin, atss_loss_2d  # noqa: F401
from .deform_conv import (ModulatedDeformConv2d, ModulatedDeformConv2dPack, deform_sample,  # noqa: F401
                          modulated_deform_conv2d)
from .voxelize import HardSimpleVFE, Voxelization, hard_voxelize, hard_voxelize_batch  # noqa: F401
from .sparse_conv import (CustomSparseEncoder, SparseConv3d, SparseConvTensor, SparseSequential,  # noqa: F401
                          SubMConv3d, make_sparse_convmodule, sparse_conv_plan)
from .sparse_train import enable_sparse_training  # noqa: F401
from .kitti_eval import (bev_box_overlap, calculate_iou_partly, d3_box_overlap, do_eval, eval_class,  # noqa: F401
                         get_mAP11, get_mAP40, image_box_overlap, kitti_eval, rotate_iou_eval)
from .depth_targets import (GenerateDepthMap, depth_map_in_boxes, generate_depth_map,  # noqa: F401
                            generate_depth_targets, points_in_boxes_all, points_in_boxes_idmap, points_in_boxes_part)
from .data_geometry import (fold_ref_frame_matrices, select_ref_frames, stage_geometry,  # noqa: F401
                            video_cur2prevs)
from .point_sample import (mv_feature_transformation, point_sample, voxel_centers,  # noqa: F401
                           voxel_sample, voxel_sample_mv)
from .optim import FusedAdamW, clip_grad_norm_  # noqa: F401

__all__ = ['build_dfm_cost', 'plane_sweep_grid', 'point_sample', 'mv_feature_transformation',
           'voxel_centers', 'voxel_sample', 'voxel_sample_mv', 'frustum_to_voxel_sample', 'depth_head_forward', 'prepare_depth',
           'prepare_coordinates_3d', 'group_norm', 'HipGroupNorm', 'DfMStereoPath', 'MultiViewDfMMixin',
           'MultiViewVoxelPath', 'inject_detector_attributes', 'patch_reference', 'enable_fast_path', 'set_fallback_policy', 'set_fp32_mode',
           'fallback_policy', 'MfmaPathError', 'select_ref_frames', 'fold_ref_frame_matrices', 'video_cur2prevs',
           'stage_geometry', 'depth_distribution_loss',
           'depth_head_statistics', 'LazyDepthDistribution', 'ImitationLoss', 'NormalizeLayer',
           'imitation_reg_layer_loss', 'reduce_imitation_statistics', 'DfMImitationMixin', 'box3d_multiclass_nms',
           'nms_bev', 'nms_normal_bev', 'box_iou_rotated', 'diff_iou_rotated_3d', 'diff_iou_rotated_2d', 'iou3d_loss',
           'IOU3DLoss', 'iou3d_loss_from_deltas', 'bbox_overlaps_nearest_3d', 'BboxOverlapsNearest3D',
           'anchor_target_3d', 'HipAnchorTrainMixin', 'delta_xyzwlhr_decode', 'anchor_head_candidates',
           'anchor3d_get_bboxes', 'HipAnchor3DHeadMixin', 'bbox_overlaps', 'BboxOverlaps2D', 'atss_target_2d',
           'HipATSSTargetMixin', 'deform_sample', 'modulated_deform_conv2d', 'ModulatedDeformConv2d',
           'ModulatedDeformConv2dPack', 'hard_voxelize', 'hard_voxelize_batch', 'Voxelization', 'HardSimpleVFE',
           'SparseConvTensor', 'SubMConv3d', 'SparseConv3d', 'SparseSequential', 'make_sparse_convmodule',
           'CustomSparseEncoder', 'sparse_conv_plan', 'enable_sparse_training', 'LidarTeacher', 'DfMLidarTeacherMixin', 'rotate_iou_eval',
           'bev_box_overlap', 'd3_box_overlap', 'image_box_overlap', 'calculate_iou_partly', 'eval_class', 'get_mAP11',
           'get_mAP40', 'do_eval', 'kitti_eval', 'generate_depth_map', 'depth_map_in_boxes', 'generate_depth_targets',
           'points_in_boxes_part', 'points_in_boxes_all', 'points_in_boxes_idmap', 'GenerateDepthMap', 'DfMDepthTargetMixin',
           'FusedAdamW', 'clip_grad_norm_', 'anchor3d_loss', 'HipAnchor3DLossMixin', 'atss_loss_2d',
           'HipATSSLossMixin']
