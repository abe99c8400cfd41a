"""ctypes binding of lib/libdfm_hip.so (C ABI: include/dfm_hip.h and the headers it includes).

One hand-written table, ``_BINDING``, keyed by header file like the declarations it mirrors; ``STRUCTS`` names the
ctypes class of every descriptor struct.  Nothing is parsed here: tests/test_capi_binding.py parses the headers and
holds this module against them -- names, return types, every parameter's type, struct layouts, constants -- and
against the built library.

Loud by design: a missing library is an ImportError with the build command,
never a silent fallback.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('DFM_HIP_LIB', os.path.join(_HERE, 'lib', 'libdfm_hip.so'))

DFM_F32, DFM_BF16 = 0, 1


class SweepDesc(ctypes.Structure):
    """struct dfm_sweep_desc"""
    _fields_ = [
        ('batch', ctypes.c_int32),
        ('channels', ctypes.c_int32),
        ('h_in', ctypes.c_int32),
        ('w_in', ctypes.c_int32),
        ('num_depths', ctypes.c_int32),
        ('h_out', ctypes.c_int32),
        ('w_out', ctypes.c_int32),
        ('feat_sample_factor', ctypes.c_float),
        ('cost_sample_factor', ctypes.c_float),
        ('img_scale_factor', ctypes.c_float),
        ('crop_x', ctypes.c_float),
        ('crop_y', ctypes.c_float),
        ('org_w', ctypes.c_float),
        ('flip', ctypes.c_int32),
        ('dtype', ctypes.c_int32),
    ]


class SweepOpts(ctypes.Structure):
    """struct dfm_sweep_opts: launch options of ONE plane-sweep call (0 = library default)"""
    _fields_ = [(n, ctypes.c_int32) for n in (
        'kernel', 'lanes_per_workgroup', 'lds_kib', 'blocks_per_group', 'planes_per_workgroup',
        'bands_per_chunk', 'points_per_lane', 'pipeline', 'store_align_points', 'pair_stores',
        'unpack')] + [('reserved', ctypes.c_int32 * 1)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != 'reserved'}


class MvDesc(ctypes.Structure):
    """struct dfm_mv_desc"""
    _fields_ = [
        ('num_views', ctypes.c_int32),
        ('num_frames', ctypes.c_int32),
        ('channels', ctypes.c_int32),
        ('feat_h', ctypes.c_int32),
        ('feat_w', ctypes.c_int32),
        ('nx', ctypes.c_int32),
        ('ny', ctypes.c_int32),
        ('nz', ctypes.c_int32),
        ('num_points', ctypes.c_int64),
        ('scale_x', ctypes.c_float),
        ('scale_y', ctypes.c_float),
        ('crop_x', ctypes.c_float),
        ('crop_y', ctypes.c_float),
        ('flip', ctypes.c_int32),
        ('pad_h', ctypes.c_float),
        ('pad_w', ctypes.c_float),
        ('mode', ctypes.c_int32),
        ('aggregate', ctypes.c_int32),
        ('valid_sample', ctypes.c_int32),
        ('dtype', ctypes.c_int32),
        ('out_channels_last', ctypes.c_int32),
        ('feats_channels_last', ctypes.c_int32),
    ]


class F2vDesc(ctypes.Structure):
    """struct dfm_f2v_desc"""
    _fields_ = [(n, ctypes.c_int32) for n in (
        'batch', 'channels', 'd', 'h', 'w', 'ds', 'hs', 'ws', 'sem_channels', 'hsem', 'wsem', 'nz',
        'ny', 'nx')] + [(n, ctypes.c_float) for n in ('pad_h', 'pad_w', 'depth_min', 'depth_span')
                        ] + [('dtype', ctypes.c_int32), ('stereo_channels_last', ctypes.c_int32),
                           ('out_channels_last', ctypes.c_int32), ('stereo_atten', ctypes.c_int32),
                           ('no_sem_atten', ctypes.c_int32), ('sem_channels_last', ctypes.c_int32)]


class SppDesc(ctypes.Structure):
    """struct dfm_spp_desc"""
    _fields_ = [('batch', ctypes.c_int32), ('h', ctypes.c_int32), ('w', ctypes.c_int32),
                ('num_sources', ctypes.c_int32), ('source_channels', ctypes.c_int32 * 4),
                ('num_branches', ctypes.c_int32), ('in_channels', ctypes.c_int32),
                ('spp_channels', ctypes.c_int32), ('pooled_h', ctypes.c_int32 * 4),
                ('pooled_w', ctypes.c_int32 * 4), ('eps', ctypes.c_float)]


class VsDesc(ctypes.Structure):
    """struct dfm_vs_desc"""
    _fields_ = [('channels', ctypes.c_int32), ('nx', ctypes.c_int32), ('ny', ctypes.c_int32),
                ('nz', ctypes.c_int32), ('num_depths', ctypes.c_int32), ('h_out', ctypes.c_int32),
                ('w_out', ctypes.c_int32), ('downsample_factor', ctypes.c_float),
                ('scale_x', ctypes.c_float), ('scale_y', ctypes.c_float), ('crop_x', ctypes.c_float),
                ('crop_y', ctypes.c_float), ('flip', ctypes.c_int32), ('ori_w', ctypes.c_float),
                ('voxel_range', ctypes.c_float * 6), ('voxel_size', ctypes.c_float * 3),
                ('proj_inv', ctypes.c_float * 16), ('mode', ctypes.c_int32),
                ('dtype', ctypes.c_int32)]


VS_PAIR_FLOATS = 24  # DFM_VS_PAIR_FLOATS


class VsMvDesc(ctypes.Structure):
    """struct dfm_vs_mv_desc"""
    _fields_ = [(n, ctypes.c_int32) for n in ('batch', 'num_views', 'channels', 'nx', 'ny', 'nz', 'num_depths',
                                              'h_out', 'w_out')] + \
        [('downsample_factor', ctypes.c_float), ('voxel_range', ctypes.c_float * 6),
         ('voxel_size', ctypes.c_float * 3), ('dtype', ctypes.c_int32),
         ('volume_channels_last', ctypes.c_int32), ('out_channels_last', ctypes.c_int32)]


class DepthLossDesc(ctypes.Structure):
    """struct dfm_depth_loss_desc"""
    _fields_ = [(n, ctypes.c_int32) for n in ('batch', 'num_depths', 'h', 'w', 'target', 'focal')] + \
        [(n, ctypes.c_float) for n in ('min_depth', 'max_depth', 'interval', 'sigma', 'alpha', 'gamma')] + \
        [('dtype', ctypes.c_int32)]


class ImitationDesc(ctypes.Structure):
    """struct dfm_imitation_desc"""
    _fields_ = [(n, ctypes.c_int32) for n in (
        'batch', 'channels', 'nz', 'ny', 'nx', 'num_boxes', 'points_batch', 'mode', 'pred_dtype', 'target_dtype',
        'pred_channels_last', 'target_channels_last', 'center_len', 'scale_len')]


IMI_INBOX, IMI_FULL = 0, 1


class Conv3dDesc(ctypes.Structure):
    """struct dfm_conv3d_desc"""
    _fields_ = [('n', ctypes.c_int32), ('cin', ctypes.c_int32), ('cout', ctypes.c_int32),
                ('in_size', ctypes.c_int32 * 3), ('out_size', ctypes.c_int32 * 3),
                ('stride', ctypes.c_int32 * 3), ('padding', ctypes.c_int32 * 3),
                ('transposed', ctypes.c_int32 * 3), ('relu', ctypes.c_int32),
                ('in_channel_stride', ctypes.c_int32), ('kernel1', ctypes.c_int32 * 3)]


class Conv3dWgradDesc(ctypes.Structure):
    """struct dfm_conv3d_wgrad_desc"""
    _fields_ = [('n', ctypes.c_int32), ('a', ctypes.c_int32), ('b', ctypes.c_int32),
                ('g_size', ctypes.c_int32 * 3), ('x_size', ctypes.c_int32 * 3),
                ('stride', ctypes.c_int32 * 3), ('padding', ctypes.c_int32 * 3),
                ('g_stride', ctypes.c_int64 * 4), ('x_stride', ctypes.c_int64 * 4)]


DL_LINEAR, DL_HARD, DL_GAUSSIAN, DL_LAPLACIAN = 0, 1, 2, 3

OVERLAP_IOU, OVERLAP_IOF = 0, 1  # DFM_OVERLAP_*
ANCHOR_TARGET_MAX_SLOTS, ANCHOR_TARGET_MAX_BATCH = 8, 64  # DFM_ANCHOR_TARGET_MAX_*
SAMPLER_PSEUDO = 0  # DFM_SAMPLER_PSEUDO


class AnchorTargetDesc(ctypes.Structure):
    """struct dfm_anchor_target_desc"""
    _fields_ = [(n, ctypes.c_int32) for n in (
        'num_locations', 'num_slots', 'num_rotations', 'box_width', 'batch', 'num_classes', 'has_labels',
        'assign_per_class', 'match_low_quality', 'gt_max_assign_all', 'sampler', 'neg_iou_thr_is_range',
        'num_ignore_boxes')] + [('ignore_iof_thr', ctypes.c_float)] + \
        [(n, ctypes.c_float * ANCHOR_TARGET_MAX_SLOTS) for n in ('pos_iou_thr', 'neg_iou_thr', 'min_pos_iou')] + \
        [(n, ctypes.c_float) for n in ('dir_offset', 'dir_limit_offset', 'pos_weight')]


ANCHOR_HEAD_MAX_BATCH = 64  # DFM_ANCHOR_HEAD_MAX_BATCH
BBOX_CODE_MIN, BBOX_CODE_MAX = 7, 16  # the box widths dfm_delta_xyzwlhr_decode / dfm_anchor_head_candidates take


class AnchorHeadDesc(ctypes.Structure):
    """struct dfm_anchor_head_desc"""
    _fields_ = [(n, ctypes.c_int32) for n in (
        'batch', 'h', 'w', 'anchors_per_location', 'num_classes', 'box_code_size', 'nms_pre', 'dtype')] + \
        [(n, ctypes.c_int64 * 4) for n in ('cls_stride', 'reg_stride', 'dir_stride')]


ANCHOR_LOSS_MAX_CODE = 16  # DFM_ANCHOR_LOSS_MAX_CODE


class AnchorLossDesc(ctypes.Structure):
    """struct dfm_anchor_loss_desc"""
    _fields_ = [(n, ctypes.c_int32) for n in (
        'batch', 'h', 'w', 'anchors_per_location', 'num_classes', 'box_code_size', 'dtype', 'has_dir', 'with_iou',
        'diff_rad_by_sin', 'reserved')] + [(n, ctypes.c_float) for n in ('gamma', 'alpha', 'beta')] + \
        [('code_weight', ctypes.c_float * ANCHOR_LOSS_MAX_CODE)] + \
        [(n, ctypes.c_int64 * 4) for n in ('cls_stride', 'reg_stride', 'dir_stride', 'grad_cls_stride',
                                           'grad_reg_stride', 'grad_dir_stride')]


ATSS_MAX_LEVELS, ATSS_MAX_TOPK, ATSS_MAX_BATCH = 8, 16, 64  # DFM_ATSS_MAX_*
ATSS_THRESH_MEANSTD, ATSS_THRESH_RATIO = 0, 1  # DFM_ATSS_THRESH_*
ATSS_CODER_DELTA_XYWH = 0  # DFM_ATSS_CODER_DELTA_XYWH


class AtssTargetDesc(ctypes.Structure):
    """struct dfm_atss_target_desc"""
    _fields_ = [(n, ctypes.c_int32) for n in (
        'num_anchors', 'num_levels', 'batch', 'gt_width', 'topk', 'num_classes', 'thresh_mode', 'reg_width', 'coder',
        'sampler', 'num_ignore_boxes')] + [('ignore_iof_thr', ctypes.c_float), ('pos_weight', ctypes.c_float),
                                           ('target_means', ctypes.c_float * 4), ('target_stds', ctypes.c_float * 4)]


class AtssLossDesc(ctypes.Structure):
    """struct dfm_atss_loss_desc"""
    _fields_ = [(n, ctypes.c_int32) for n in (
        'batch', 'num_levels', 'num_anchors', 'num_classes', 'reg_class_agnostic', 'dtype', 'reg_dtype', 'reserved')] + \
        [('gamma', ctypes.c_float), ('alpha', ctypes.c_float), ('target_means', ctypes.c_float * 4),
         ('target_stds', ctypes.c_float * 4)] + \
        [(n, ctypes.c_int32 * ATSS_MAX_LEVELS) for n in ('h', 'w', 'row_offset', 'reserved_levels')] + \
        [(n, ctypes.c_int64 * (ATSS_MAX_LEVELS * 4)) for n in ('cls_stride', 'reg_stride', 'ctr_stride',
                                                               'grad_cls_stride', 'grad_reg_stride', 'grad_ctr_stride')]


class DeformDesc(ctypes.Structure):
    """struct dfm_deform_desc"""
    _fields_ = [(n, ctypes.c_int32) for n in (
        'n', 'cin', 'h', 'w', 'ho', 'wo', 'stride_h', 'stride_w', 'pad_h', 'pad_w', 'dil_h', 'dil_w', 'deform_groups',
        'mask_is_logit', 'dtype', 'om_dtype')] + [('offset_stride', ctypes.c_int64 * 4),
                                                  ('mask_stride', ctypes.c_int64 * 4)]


VOXEL_MAX_BATCH = 64  # DFM_VOXEL_MAX_BATCH


class VoxelDesc(ctypes.Structure):
    """struct dfm_voxel_desc"""
    _fields_ = [('batch', ctypes.c_int32), ('ndim', ctypes.c_int32), ('grid', ctypes.c_int32 * 3),
                ('max_num_points', ctypes.c_int32), ('max_voxels', ctypes.c_int32), ('lo', ctypes.c_float * 3),
                ('vs', ctypes.c_float * 3), ('offset', ctypes.c_int64 * (VOXEL_MAX_BATCH + 1))]


class SparseConvDesc(ctypes.Structure):
    """struct dfm_sparse_conv_desc"""
    _fields_ = [('batch', ctypes.c_int32), ('in_size', ctypes.c_int32 * 3), ('kernel', ctypes.c_int32 * 3),
                ('stride', ctypes.c_int32 * 3), ('padding', ctypes.c_int32 * 3), ('subm', ctypes.c_int32)]


class SparseConvPlan(ctypes.Structure):
    """struct dfm_sparse_conv_plan"""
    _fields_ = [('out_size', ctypes.c_int32 * 3), ('taps', ctypes.c_int32), ('out_rows', ctypes.c_int64),
                ('in_capacity', ctypes.c_int64), ('out_capacity', ctypes.c_int64)]


DEPTH_MAX_BATCH, DEPTH_CAM_DOUBLES = 64, 28  # DFM_DEPTH_MAX_BATCH, DFM_DEPTH_CAM_DOUBLES
PIB_PART, PIB_ALL, PIB_IDMAP = 0, 1, 2  # DFM_PIB_*


class DepthTargetsDesc(ctypes.Structure):
    """struct dfm_depth_targets_desc"""
    _fields_ = [(n, ctypes.c_int32) for n in ('batch', 'pad_h', 'pad_w', 'point_stride')] + \
        [('img_h', ctypes.c_int32 * DEPTH_MAX_BATCH), ('img_w', ctypes.c_int32 * DEPTH_MAX_BATCH),
         ('point_off', ctypes.c_int64 * (DEPTH_MAX_BATCH + 1)), ('box_off', ctypes.c_int64 * (DEPTH_MAX_BATCH + 1))]


OPTIM_THREADS, OPTIM_CHUNK, OPTIM_ZERO_GRADS = 256, 8192, 1  # DFM_OPTIM_*


class OptimTensor(ctypes.Structure):
    """struct dfm_optim_tensor: one row of the optimizer's multi-tensor table (the arrays are device addresses)"""
    _fields_ = [(n, ctypes.c_int64) for n in ('param', 'grad', 'exp_avg', 'exp_avg_sq', 'master', 'numel')] + \
        [('dtype', ctypes.c_int32), ('reserved', ctypes.c_int32)] + \
        [(n, ctypes.c_float) for n in ('decay', 'step_size', 'bc2_sqrt', 'lerp_weight', 'beta2', 'one_minus_beta2',
                                       'eps', 'reserved_f')]


# C struct name -> its ctypes mirror: every descriptor struct the headers define
STRUCTS = {
    'dfm_sweep_desc': SweepDesc, 'dfm_sweep_opts': SweepOpts, 'dfm_mv_desc': MvDesc, 'dfm_f2v_desc': F2vDesc,
    'dfm_spp_desc': SppDesc, 'dfm_vs_desc': VsDesc, 'dfm_vs_mv_desc': VsMvDesc,
    'dfm_depth_loss_desc': DepthLossDesc, 'dfm_imitation_desc': ImitationDesc, 'dfm_conv3d_desc': Conv3dDesc,
    'dfm_conv3d_wgrad_desc': Conv3dWgradDesc, 'dfm_anchor_target_desc': AnchorTargetDesc,
    'dfm_anchor_head_desc': AnchorHeadDesc, 'dfm_atss_target_desc': AtssTargetDesc, 'dfm_deform_desc': DeformDesc,
    'dfm_voxel_desc': VoxelDesc, 'dfm_sparse_conv_desc': SparseConvDesc, 'dfm_sparse_conv_plan': SparseConvPlan,
    'dfm_depth_targets_desc': DepthTargetsDesc, 'dfm_optim_tensor': OptimTensor,
    'dfm_anchor_loss_desc': AnchorLossDesc, 'dfm_atss_loss_desc': AtssLossDesc,
}

# DFM_SPARSE_STATUS_*: bits of the device status word of the sparse-convolution index kernels
SPARSE_STATUS = {1: 'a hash-table probe loop ran out of slots', 2: 'two input rows share one coordinate (duplicate)',
                 4: 'more output rows than the row bound', 8: 'a coordinate outside the grid or the batch'}
SPARSE_MAX_TAPS = 27  # DFM_SPARSE_MAX_TAPS
SPARSE_WGRAD_CHUNK, SPARSE_BN_CHUNK = 256, 256  # DFM_SPARSE_WGRAD_CHUNK, DFM_SPARSE_BN_CHUNK
KITTI_SAMPLE_POINTS, KITTI_LDS_DETS = 41, 128  # DFM_KITTI_SAMPLE_POINTS, DFM_KITTI_LDS_DETS

DFM_ERR_UNSUPPORTED = -2  # include/dfm_hip.h
BOX_NMS_MAX_N = 16384  # DFM_BOX_NMS_MAX_N


class DfmHipError(RuntimeError):
    pass


def _table(*rows):
    """(name, restype, argtypes) rows of one header -> {name: (restype, argtypes)}; a name bound twice raises (a dict
    literal would keep the last one and say nothing)"""
    table = {}
    for name, restype, argtypes in rows:
        if name in table:
            raise ValueError(f'{name} is bound twice in one header')
        table[name] = (restype, argtypes)
    return table


def _binding():
    """header file -> name -> (restype, argtypes) of every symbol that header declares: the whole binding, written by
    hand in the headers' order.  vp: a ``void *`` of the header (dtype-dependent memory, the stream), fp: a typed
    pointer (``float *``, ``int32_t *``, ...); both are c_void_p here.  A pointer to a descriptor struct is a
    POINTER to its class in STRUCTS."""
    P = ctypes.POINTER
    vp = fp = ctypes.c_void_p
    ci, i32, i64, sz, f32, f64 = (ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t, ctypes.c_float,
                                  ctypes.c_double)
    dp, op, mp, f2p, spp, pp = P(SweepDesc), P(SweepOpts), P(MvDesc), P(F2vDesc), P(SppDesc), P(vp)
    vsp, vmp, cp, wp, lp = P(VsDesc), P(VsMvDesc), P(Conv3dDesc), P(Conv3dWgradDesc), P(DepthLossDesc)
    ip, atp, ahp, adp, ddp = P(ImitationDesc), P(AnchorTargetDesc), P(AnchorHeadDesc), P(AtssTargetDesc), P(DeformDesc)
    vdp, sdp, plp, i32p, i64p = P(VoxelDesc), P(SparseConvDesc), P(SparseConvPlan), P(i32), P(i64)
    dtp, alp, slp = P(DepthTargetsDesc), P(AnchorLossDesc), P(AtssLossDesc)
    return {
        'dfm_hip.h': _table(
            ('dfm_version', ci, []),
            ('dfm_last_error', ctypes.c_char_p, []),
            ('dfm_profile_begin', ci, [ci]),
            ('dfm_profile_end', ci, [P(f64), P(ci)]),
            ('dfm_camera_prepare', ci, [fp, i32, i32, i32, fp, fp, vp]),
            ('dfm_plane_sweep_workspace_bytes', sz, [dp]),
            ('dfm_plane_sweep_fwd', ci, [dp, vp, vp, fp, fp, fp, fp, vp, vp, sz, vp]),
            ('dfm_plane_sweep_cl_workspace_bytes', sz, [dp]),
            ('dfm_plane_sweep_fwd_channels_last', ci, [dp, vp, vp, fp, fp, fp, fp, vp, vp, sz, vp]),
            ('dfm_plane_sweep_fwd_nhwc', ci, [dp, vp, vp, fp, fp, fp, fp, vp, vp, sz, vp]),
            ('dfm_plane_sweep_fwd_from_nhwc', ci, [dp, vp, vp, fp, fp, fp, fp, vp, vp, sz, vp]),
            ('dfm_plane_sweep_bwd', ci, [dp, vp, fp, fp, fp, fp, fp, fp, vp]),
            ('dfm_plane_sweep_grid', ci, [dp, i32, fp, fp, fp, fp, fp, fp, vp]),
            ('dfm_plane_sweep_last_kernel', ci, []),
            ('dfm_plane_sweep_bwd_last_kernel', ci, []),
            ('dfm_plane_sweep_fwd_opts', ci, [dp, vp, vp, fp, fp, fp, fp, vp, vp, sz, vp, op]),
            ('dfm_plane_sweep_bwd_opts', ci, [dp, vp, fp, fp, fp, fp, fp, fp, vp, op]),
            ('dfm_plane_sweep_bwd_channels_last', ci, [dp, vp, fp, fp, fp, fp, fp, fp, vp, sz, vp]),
            ('dfm_plane_sweep_bwd_cur_nhwc', ci, [dp, vp, fp, fp, fp, fp, fp, vp]),
            ('dfm_plane_sweep_bwd_prev_gather_workspace_bytes', sz, [dp]),
            ('dfm_plane_sweep_bwd_prev_gather', ci, [dp, vp, fp, fp, fp, fp, fp, vp, sz, vp]),
            ('dfm_plane_sweep_bwd_gather', ci, [dp, i32, vp, i32, fp, fp, fp, fp, fp, i32, vp, sz, vp]),
            ('dfm_plane_sweep_autotune', ci, [dp, vp, vp, fp, fp, fp, fp, vp, vp, sz, vp, op]),
            ('dfm_plane_sweep_tuning', ci, [dp, op]),
            ('dfm_plane_sweep_reset_tuning', None, []),
            ('dfm_store_probe', ci, [vp, i32, i32, i64, i32, i32, vp]),
            ('dfm_clock_probe', ci, [vp, i32, vp]),
            ('dfm_point_sample_mv_workspace_bytes', sz, [mp]),
            ('dfm_point_sample_mv_fwd', ci, [mp, vp, fp, fp, fp, vp, vp, vp, sz, vp]),
            ('dfm_frustum_to_voxel_workspace_bytes', sz, [f2p]),
            ('dfm_frustum_to_voxel_fwd', ci, [f2p, vp, vp, vp, fp, fp, vp, vp, sz, vp]),
            ('dfm_depth_head_fwd', ci, [i32, i32, i32, i32, i32, i32, vp, fp, vp, vp, vp, vp]),
            ('dfm_depth_head_stats_fwd', ci, [i32, i32, i32, i32, i32, i32, vp, fp, fp, fp, vp, vp]),
            ('dfm_frustum_to_voxel_fused_fwd', ci, [f2p, vp, vp, fp, fp, i32, vp, fp, fp, vp, vp, sz, vp]),
            ('dfm_frustum_to_voxel_bwd_workspace_bytes', sz, [f2p]),
            ('dfm_frustum_to_voxel_bwd', ci, [f2p, vp, vp, fp, fp, fp, fp, vp, sz, vp]),
            ('dfm_frustum_to_voxel_fused_bwd', ci, [f2p, vp, vp, fp, fp, i32, fp, fp, fp, fp, vp, sz, vp]),
            ('dfm_frustum_to_voxel_bwd_gather_workspace_bytes', sz, [f2p]),
            ('dfm_frustum_to_voxel_bwd_gather', ci, [f2p, vp, vp, vp, fp, fp, i32, fp, P(f32), fp, fp, fp, vp, sz,
                                                     vp]),
            ('dfm_frustum_to_voxel_bwd_gather_cl', ci, [f2p, vp, vp, vp, fp, fp, i32, fp, P(f32), fp, vp, fp, vp, sz,
                                                        vp]),
            ('dfm_point_sample_mv_fwd_batched', ci, [vp, i32, vp, fp, i32, fp, fp, vp, vp, vp]),
            ('dfm_point_sample_mv_bwd_workspace_bytes', sz, [mp]),
            ('dfm_point_sample_mv_bwd', ci, [mp, vp, fp, fp, fp, fp, vp, sz, vp]),
            ('dfm_depth_head_bwd', ci, [i32, i32, i32, i32, i32, i32, vp, fp, vp, vp, vp, fp, vp]),
            ('dfm_sweep_conv_weight_bytes', sz, []),
            ('dfm_sweep_conv_pack_weights', ci, [vp, vp, i32, vp, vp]),
            ('dfm_sweep_conv_stats_splits', ci, [dp, i32]),
            ('dfm_sweep_conv_fwd', ci, [dp, vp, vp, fp, fp, fp, fp, vp, vp, vp, fp, fp, i32, vp]),
            ('dfm_cost_gate_weight_bytes', sz, [i32]),
            ('dfm_cost_gate_pack_weights', ci, [vp, i32, i32, vp, vp]),
            ('dfm_cost_gate_fwd', ci, [i32, i32, i64, i32, vp, vp, vp, vp, vp]),
            ('dfm_conv3d_k3_c32_weight_bytes', sz, []),
            ('dfm_conv3d_k3_c32_pack_weights', ci, [vp, i32, i32, i32, i32, vp, vp]),
            ('dfm_conv3d_k3_c32_stats_splits', ci, [i32, i32, i32, i32, i32]),
            ('dfm_conv3d_k3_c32_fwd', ci, [i32, i32, i32, i32, vp, vp, fp, vp, i32, i32, i32, fp, vp]),
            ('dfm_conv3d_k3_c32_fwd_strided', ci, [i32, i32, i32, i32, vp, i32, vp, fp, vp, i32, i32, i32, fp, vp]),
            ('dfm_conv3d_k3_c32_fwd_slices', ci, [i32, i32, i32, i32, vp, i32, vp, vp, i32, i32, i32, vp]),
            ('dfm_conv3d_k3_c32_to1_fwd', ci, [i32, i32, i32, i32, vp, vp, vp, i32, i32, vp]),
            ('dfm_group_norm_coefficients', ci, [i32, i32, i32, f32, vp, i32, vp, vp, vp, vp]),
            ('dfm_conv3d_to1_norm_fwd', ci, [i32, i32, i32, i32, vp, vp, vp, i32, i32, i32, vp, i32, vp]),
            ('dfm_conv3d_to1_bwd_data', ci, [i32, i32, i32, i32, vp, vp, i32, vp, vp]),
            ('dfm_conv3d_to1_wgrad_workspace_bytes', sz, []),
            ('dfm_conv3d_to1_wgrad', ci, [i32, i32, i32, i32, vp, vp, vp, i32, vp, sz, vp]),
            ('dfm_bilinear_resize_bwd_nhwc', ci, [i32, i32, i32, i32, i32, i32, i32, vp, vp, fp, i32, vp, fp, i32, vp,
                                                  vp]),
            ('dfm_depth_pool_fwd', ci, [i64, i32, i64, i32, vp, vp, vp]),
            ('dfm_depth_pool_bwd', ci, [i64, i32, i64, i32, vp, vp, vp]),
            ('dfm_cost_gate_mfma_weight_bytes', sz, [i32]),
            ('dfm_cost_gate_mfma_pack_weights', ci, [vp, i32, i32, vp, vp]),
            ('dfm_cost_gate_mfma_fwd', ci, [i32, i32, i64, vp, vp, vp, vp, vp]),
            ('dfm_conv3d_g_weight_bytes', sz, [i32, i32]),
            ('dfm_conv3d_g_pack_weights', ci, [vp, i32, i32, i32, i32, i32, vp, vp]),
            ('dfm_conv3d_g_pack_weights_2d', ci, [vp, i32, i32, i32, i32, i32, vp, vp]),
            ('dfm_conv3d_g_fwd', ci, [cp, vp, vp, fp, fp, vp, vp, vp]),
            ('dfm_conv3d_g_fwd_f32', ci, [cp, vp, vp, vp, vp, vp]),
            ('dfm_conv3d_g_plan', ci, [cp, i64p]),
            ('dfm_conv3d_wgrad_workspace_bytes', sz, [wp]),
            ('dfm_conv3d_wgrad', ci, [wp, vp, vp, fp, vp, sz, vp]),
            ('dfm_conv3d_wgrad_to', ci, [wp, vp, vp, vp, i32, vp, sz, vp]),
            ('dfm_depth_loss_fwd', ci, [lp, vp, fp, fp, fp, vp, vp]),
            ('dfm_depth_loss_bwd', ci, [lp, vp, fp, fp, fp, vp, vp]),
            ('dfm_depth_loss_fused_fwd', ci, [lp, vp, i32, fp, fp, fp, vp, vp]),
            ('dfm_depth_loss_fused_bwd', ci, [lp, vp, i32, fp, fp, fp, fp, vp]),
            ('dfm_voxel_sample_fwd', ci, [vsp, vp, fp, vp, vp]),
            ('dfm_voxel_sample_bwd', ci, [vsp, vp, fp, fp, vp]),
            ('dfm_voxel_sample_mv_fwd', ci, [vmp, fp, vp, fp, vp, vp]),
            ('dfm_voxel_sample_mv_bwd', ci, [vmp, fp, vp, fp, fp, vp]),
            ('dfm_spp_tail_workspace_bytes', sz, [spp]),
            ('dfm_spp_tail_fwd', ci, [spp, pp, pp, pp, pp, pp, vp, vp, sz, vp]),
            ('dfm_group_norm_workspace_bytes', sz, [i32, i32, i64, i32]),
            ('dfm_group_norm_fwd', ci, [i32, i32, i64, i32, f32, i32, i32, vp, fp, fp, vp, fp, fp, vp, sz, vp]),
            ('dfm_group_norm_fwd_channels_last', ci, [i32, i32, i64, i32, f32, i32, i32, vp, fp, fp, vp, fp, fp, vp, sz,
                                                      vp]),
            ('dfm_group_norm_apply_channels_last', ci, [i32, i32, i64, i32, f32, i32, i32, vp, fp, fp, vp, fp, fp, fp,
                                                        i32, vp, sz, vp]),
            ('dfm_group_norm_fwd_channels_last_res', ci, [i32, i32, i64, i32, f32, i32, i32, vp, fp, fp, vp, vp, fp, fp,
                                                          vp, sz, vp]),
            ('dfm_group_norm_apply_channels_last_res', ci, [i32, i32, i64, i32, f32, i32, i32, vp, fp, fp, vp, vp, fp,
                                                            fp, fp, i32, vp, sz, vp]),
            ('dfm_group_norm_bwd', ci, [i32, i32, i64, i32, i32, i32, vp, vp, vp, fp, fp, fp, vp, fp, fp, vp, sz, vp]),
            ('dfm_group_norm_bwd_channels_last', ci, [i32, i32, i64, i32, i32, i32, vp, vp, vp, fp, fp, fp, vp, vp, fp,
                                                      fp, vp, sz, vp]),
            ('dfm_group_norm_bwd_channels_last_xmask', ci, [i32, i32, i64, i32, i32, vp, vp, fp, fp, fp, fp, vp, fp, fp,
                                                            vp, sz, vp]),
            ('dfm_batch_norm_workspace_bytes', sz, [i32, i64]),
            ('dfm_batch_norm_stats_channels_last', ci, [i32, i64, i32, vp, fp, vp, sz, vp]),
            ('dfm_batch_norm_apply_gathered_channels_last', ci, [i32, i64, i32, f32, i32, i32, vp, fp, fp, vp, fp, vp,
                                                                 fp, fp, fp, vp]),
            ('dfm_batch_norm_bwd_reduce_channels_last', ci, [i32, i64, i32, i32, vp, vp, vp, fp, fp, fp, fp, fp, vp, sz,
                                                             vp]),
            ('dfm_batch_norm_bwd_apply_channels_last', ci, [i32, i64, i32, i32, vp, vp, vp, fp, fp, fp, fp, fp, fp, vp,
                                                            vp, vp, sz, vp]),
            ('dfm_imitation_loss_workspace_bytes', sz, [ip]),
            ('dfm_imitation_loss_fwd', ci, [ip, vp, vp, fp, fp, fp, fp, fp, vp, vp, vp, sz, vp]),
            ('dfm_imitation_loss_bwd', ci, [ip, vp, vp, vp, fp, fp, fp, vp, vp]),
            ('dfm_box_nms_workspace_bytes', sz, [i32, i32]),
            ('dfm_box_nms_rotated', ci, [fp, i32, i32, vp, vp, i32, i32, f32, vp, vp, vp, sz, vp]),
            ('dfm_box_nms_aligned', ci, [fp, i32, vp, vp, i32, i32, f32, vp, vp, vp, sz, vp]),
            ('dfm_box_iou_rotated', ci, [fp, i32, fp, i32, i32, fp, vp]),
            ('dfm_diff_iou_rotated', ci, [fp, fp, i32, i32, fp, fp, fp, vp]),
            ('dfm_iou3d_loss_from_deltas', ci, [fp, fp, fp, vp, i32, i32, i32, fp, fp, vp]),
            ('dfm_nearest_bev_overlaps', ci, [fp, i32, fp, i32, i32, i32, i32, fp, vp]),
            ('dfm_anchor_target_workspace_bytes', sz, [i32, i32]),
            ('dfm_anchor_target_3d', ci, [atp, fp, fp, vp, i32p, vp, fp, fp, fp, vp, fp, vp, vp, sz, vp]),
        ),
        # the anchor head's maps -> boxes
        'dfm_hip_bbox_decode.h': _table(
            ('dfm_anchor_head_candidates_workspace_bytes', sz, [ahp]),
            ('dfm_anchor_head_candidates', ci, [ahp, vp, vp, vp, fp, fp, fp, fp, vp, vp, vp, sz, vp]),
            ('dfm_delta_xyzwlhr_decode', ci, [fp, fp, i32, i32, fp, vp]),
        ),
        # 2-D box overlaps and the 2-D ATSS head's training targets
        'dfm_hip_atss_target.h': _table(
            ('dfm_bbox_overlaps_2d', ci, [fp, i32, fp, i32, i32, i32, fp, vp]),
            ('dfm_atss_target_workspace_bytes', sz, [adp, i32]),
            ('dfm_atss_target_2d', ci, [adp, fp, i32p, vp, fp, i32p, vp, vp, fp, fp, fp, vp, vp, vp, sz, vp]),
        ),
        # the columns of the modulated deformable convolution and their backward
        'dfm_hip_deform_conv.h': _table(
            ('dfm_deform_sample_fwd', ci, [ddp, vp, vp, vp, vp, vp]),
            ('dfm_deform_conv_bwd_cols', ci, [ddp, vp, vp, vp, vp, fp, i64p, fp, i64p, fp, vp]),
        ),
        # hard voxelization and the sparse 3-D convolutions of the LiDAR teacher
        'dfm_hip_sparse_conv.h': _table(
            ('dfm_voxel_keys', ci, [vdp, fp, fp, vp]),
            ('dfm_voxel_heads', ci, [vdp, fp, fp, fp, fp, vp]),
            ('dfm_voxel_keep', ci, [vdp, fp, fp, fp, vp]),
            ('dfm_voxel_fill', ci, [vdp, fp, fp, fp, fp, fp, fp, fp, fp, fp, vp]),
            ('dfm_sparse_conv_out_shape', ci, [sdp, i64, plp]),
            ('dfm_sparse_conv_workspace_bytes', sz, [sdp, i64]),
            ('dfm_sparse_index_build', ci, [fp, i64, i32, i32p, fp, fp, i64, fp, vp]),
            ('dfm_sparse_subm_neighbours', ci, [fp, i64, i32, i32p, fp, fp, i64, fp, vp]),
            ('dfm_sparse_conv_out_rows', ci, [sdp, fp, i64, fp, fp, fp, fp, vp]),
            ('dfm_sparse_conv_neighbours', ci, [sdp, fp, i64, fp, fp, fp, vp]),
            ('dfm_sparse_conv_fwd', ci, [i32, i32, i32, fp, i64, fp, fp, i64, fp, fp, fp, i32, fp, vp]),
            ('dfm_sparse_dense', ci, [fp, fp, i64, i32, i32, i32p, fp, vp]),
        ),
        # the backward of the sparse convolutions and the BatchNorm over live rows
        'dfm_hip_sparse_train.h': _table(
            ('dfm_sparse_inverse_table', ci, [fp, i32, i64, i64, fp, vp]),
            ('dfm_sparse_conv_wgrad_workspace_bytes', sz, [i32, i32, i32, i64]),
            ('dfm_sparse_conv_wgrad', ci, [i32, i32, i32, fp, i64, fp, fp, i64, fp, fp, vp, sz, fp, vp]),
            ('dfm_sparse_bn_workspace_bytes', sz, [i64, i32]),
            ('dfm_sparse_bn_stats', ci, [fp, fp, i64, i32, fp, vp, sz, fp, vp]),
            ('dfm_sparse_bn_apply', ci, [fp, fp, i64, i32, fp, fp, fp, f32, i32, fp, vp]),
            ('dfm_sparse_bn_bwd_reduce', ci, [fp, fp, fp, i64, i32, fp, fp, fp, f32, i32, fp, vp, sz, fp, vp]),
            ('dfm_sparse_bn_bwd_apply', ci, [fp, fp, fp, i64, i32, fp, fp, fp, fp, f32, i32, fp, vp]),
            ('dfm_sparse_bn_running', ci, [fp, i32, f32, fp, fp, vp]),
            ('dfm_sparse_dense_bwd', ci, [fp, fp, i64, i32, i32, i32p, fp, vp]),
        ),
        # the KITTI evaluation's same-frame overlaps and its matching
        'dfm_hip_kitti_eval.h': _table(
            ('dfm_kitti_overlaps', ci, [i64, i64, i32, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, vp]),
            ('dfm_kitti_eval_workspace_bytes', sz, [i64, i32, i64, i32]),
            ('dfm_kitti_match', ci, [i32, i32, i32, i64, i32, i32, i32, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp,
                                     i64, i64, fp, fp, fp, fp, fp, fp, i64, vp, sz, vp]),
        ),
        # the depth loss's targets (LiDAR depth map, box-id mask) and box membership
        'dfm_hip_depth_targets.h': _table(
            ('dfm_depth_targets_workspace_bytes', sz, [dtp]),
            ('dfm_depth_scatter', ci, [dtp, fp, fp, vp, sz, vp]),
            ('dfm_depth_resolve', ci, [dtp, vp, fp, fp, fp, f32, f32, fp, fp, vp]),
            ('dfm_points_in_boxes', ci, [i32, i32, i64, i32, fp, fp, fp, vp]),
        ),
        # the optimizer step: the gradients' global norm, the clip and AdamW over one multi-tensor table
        'dfm_hip_optim.h': _table(
            ('dfm_grad_sqnorm', ci, [vp, i32, vp, i64, fp, vp]),
            ('dfm_adamw_step', ci, [vp, i32, vp, i64, fp, f32, fp, i32, vp]),
            ('dfm_grad_scale', ci, [vp, i32, vp, i64, fp, f32, fp, vp]),
        ),
        # the 3-D anchor head's loss_single: focal, smooth-L1, direction and IoU terms over the maps in place
        'dfm_hip_anchor_loss.h': _table(
            ('dfm_anchor3d_loss_workspace_bytes', sz, [alp]),
            ('dfm_anchor3d_loss_fwd', ci, [alp, vp, vp, vp, fp, fp, fp, fp, fp, fp, fp, fp, fp, vp, sz, vp]),
            ('dfm_anchor3d_loss_bwd', ci, [alp, vp, vp, vp, fp, fp, fp, fp, fp, fp, fp, fp, fp, vp, vp, vp, vp]),
        ),
        # the 2-D ATSS head's loss over all levels: focal, centerness-weighted GIoU and centerness terms; the maps and
        # their gradients come as HOST arrays of 3 L device pointers
        'dfm_hip_atss_loss.h': _table(
            ('dfm_atss_loss_workspace_bytes', sz, [slp]),
            ('dfm_atss_loss_fwd', ci, [slp, pp, fp, fp, fp, fp, fp, vp, sz, vp]),
            ('dfm_atss_loss_bwd', ci, [slp, pp, fp, fp, fp, fp, fp, pp, vp]),
        ),
    }


def _flatten(binding):
    """{header: {name: signature}} -> {name: signature}; a name bound under two headers raises"""
    flat, where = {}, {}
    for header, table in binding.items():
        for name, signature in table.items():
            if name in flat:
                raise ValueError(f'{name} is bound twice: under {where[name]} and under {header}')
            flat[name], where[name] = signature, header
    return flat


_BINDING = _binding()
SIGNATURES = _flatten(_BINDING)
EXPORTS = tuple(SIGNATURES)

_lib = None


def lib():
    """Load (once) and return the ctypes handle; raises if not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f'{LIB_PATH} not found: build it with '
            '`python -c "import __graft_entry__ as g; g.build()"` '
            '(hipcc --offload-arch=gfx950).  There is no CPU fallback.')
    h = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(h, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = h
    return h


def check(rc):
    if rc != 0:
        msg = lib().dfm_last_error().decode('utf-8', 'replace')
        raise DfmHipError(f'libdfm_hip error {rc}: {msg}')
