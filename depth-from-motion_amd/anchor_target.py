"""Nearest-BEV overlaps and the 3-D anchor head's training targets on the HIP path.

Mirror of ``bbox_overlaps_nearest_3d`` / ``BboxOverlapsNearest3D`` (mmdet3d/core/bbox/iou_calculators/
iou3d_calculator.py:9-55, 99-145) and of ``AnchorTrainMixin.anchor_target_3d`` (mmdet3d/models/dense_heads/
train_mixins.py:12-317) with what it runs per image and class slot: mmdet's ``MaxIoUAssigner`` over the
nearest-BEV overlaps, ``PseudoSampler``, ``DeltaXYZWLHRBBoxCoder.encode`` and ``get_direction_target``.  mmdet is
not a dependency: the semantics are those stated in include/dfm_hip.h.

The reference materialises a G x anchors overlap matrix per slot and image and walks it with well over a hundred
small launches and several device-to-host waits.  ``anchor_target_3d`` here is one call of
``dfm_anchor_target_3d`` for the whole batch and all slots: a memset of the (slots, sum G) scratch and two
launches, no overlap matrix in memory, nothing copied to the host.  Its outputs -- dense ``(B, A, ...)`` tensors
in the reference's final anchor order -- are what ``iou3d_loss_from_deltas`` takes as ``bbox_targets`` (one image:
``out[2][b]``); ``HipAnchorTrainMixin`` wraps them into the reference method's return tuple, which costs the one
small copy of the per-image counts.

GT boxes and anchors of any floating dtype or stride are converted to contiguous fp32.  CPU tensors are refused:
there is no CPU path.
"""
import ctypes

import torch

from . import _capi
from .fallback import run_reference
from ._launch import STREAM, WS, launch, require_gpu
from .registry import register_module

__all__ = ['bbox_overlaps_nearest_3d', 'BboxOverlapsNearest3D', 'anchor_target_3d', 'HipAnchorTrainMixin']

MAX_SLOTS, MAX_BATCH = _capi.ANCHOR_TARGET_MAX_SLOTS, _capi.ANCHOR_TARGET_MAX_BATCH


def _f32(t):
    return t.detach().to(torch.float32).contiguous()


def bbox_overlaps_nearest_3d(bboxes1, bboxes2, mode='iou', is_aligned=False, coordinate='lidar'):
    """Nearest-BEV IoU (or IoF) of two sets of 3-D boxes, ``(N, S)`` and ``(M, S)`` with ``S >= 7`` columns
    ``(x, y, z, dx, dy, dz, yaw, ...)`` -> ``(N, M)`` fp32, or ``(N,)`` when ``is_aligned`` (the reference
    function's signature, iou3d_calculator.py:99-145).  ``coordinate`` only selects the box class in the
    reference; the nearest-BEV box is the same for all three."""
    assert coordinate in ['camera', 'lidar', 'depth']
    require_gpu(bboxes1, 'bboxes1')
    require_gpu(bboxes2, 'bboxes2')
    if mode not in ('iou', 'iof'):
        raise ValueError(f"mode must be 'iou' or 'iof', got {mode!r}")
    if bboxes1.dim() != 2 or bboxes2.dim() != 2 or not bboxes1.size(-1) == bboxes2.size(-1) >= 7:
        raise ValueError(f'bbox_overlaps_nearest_3d takes (N, S) and (M, S) boxes with S >= 7, got '
                         f'{tuple(bboxes1.shape)} and {tuple(bboxes2.shape)}')
    n, m, width = bboxes1.shape[0], bboxes2.shape[0], bboxes1.shape[1]
    if is_aligned and n != m:
        raise ValueError(f'aligned overlaps need as many bboxes2 as bboxes1, got {n} and {m}')
    device = bboxes1.device
    out = torch.empty((n,) if is_aligned else (n, m), dtype=torch.float32, device=device)
    if out.numel():
        b1, b2 = _f32(bboxes1), _f32(bboxes2)
        launch('dfm_nearest_bev_overlaps', b1, n, b2, m, width,
               _capi.OVERLAP_IOF if mode == 'iof' else _capi.OVERLAP_IOU, int(bool(is_aligned)), out, STREAM)
    return out


@register_module(on_path=False)
class BboxOverlapsNearest3D(object):
    """``BboxOverlapsNearest3D`` of the reference (iou3d_calculator.py:9-55): built from
    ``dict(type='BboxOverlapsNearest3D')`` as the KITTI configs' ``iou_calculator``."""

    def __init__(self, coordinate='lidar'):
        assert coordinate in ['camera', 'lidar', 'depth']
        self.coordinate = coordinate

    def __call__(self, bboxes1, bboxes2, mode='iou', is_aligned=False):
        return bbox_overlaps_nearest_3d(bboxes1, bboxes2, mode, is_aligned, self.coordinate)

    def __repr__(self):
        return f'{self.__class__.__name__}(coordinate={self.coordinate}'


def _field(assigner, name, default):
    if isinstance(assigner, dict):
        return assigner.get(name, default)
    return getattr(assigner, name, default)


def _assigner_fields(assigners):
    """the MaxIoUAssigner fields of one assigner or a list of them (objects or config dicts), with mmdet's
    defaults: per-slot thresholds and the flags the slots must share"""
    if not isinstance(assigners, (list, tuple)):
        assigners = [assigners]
    pos = [_field(a, 'pos_iou_thr', None) for a in assigners]
    neg = [_field(a, 'neg_iou_thr', None) for a in assigners]
    if any(v is None for v in pos) or any(v is None for v in neg):
        raise ValueError('every assigner carries pos_iou_thr and neg_iou_thr (the MaxIoUAssigner fields)')
    min_pos = [_field(a, 'min_pos_iou', .0) for a in assigners]
    flags = {}
    for name, default in (('match_low_quality', True), ('gt_max_assign_all', True)):
        values = {bool(_field(a, name, default)) for a in assigners}
        if len(values) != 1:
            raise ValueError(f'the assigners of one head share {name}, got both settings')
        flags[name] = values.pop()
    return dict(pos=pos, neg=neg, min_pos=min_pos, ignore_iof_thr=max(float(_field(a, 'ignore_iof_thr', -1))
                                                                      for a in assigners), **flags)


def _gt_tensor(boxes, device):
    if not torch.is_tensor(boxes):
        boxes = boxes.tensor
    require_gpu(boxes, 'gt_bboxes')
    return _f32(boxes.to(device)).view(-1, boxes.shape[-1] if boxes.dim() > 1 else 7)


def anchor_target_3d(anchors, gt_bboxes_list, gt_labels_list, assigners, *, num_classes, assign_per_class,
                     dir_offset, dir_limit_offset, pos_weight, num_ignore_boxes=0, sampler='PseudoSampler'):
    """The training targets of every anchor for a batch, all class slots at once.

    ``anchors``: ``(..., C, R, 7)``, the anchors of ONE image as ``Anchor3DRangeGenerator(reshape_out=False)``
    lays them out, shared by every image; ``C`` class slots, one per assigner.  With a single assigner (not a
    list) every anchor is one slot that sees every GT box.  ``gt_bboxes_list``: per image a ``(G, 7)`` tensor
    or an object with ``.tensor``; ``gt_labels_list``: per image ``(G,)`` integer labels.  ``assigners``: one or
    a list of objects or dicts with the ``MaxIoUAssigner`` fields (``pos_iou_thr``, ``neg_iou_thr``,
    ``min_pos_iou``, ``match_low_quality``, ``gt_max_assign_all``, ``ignore_iof_thr``).

    Returns ``(labels, label_weights, bbox_targets, bbox_weights, dir_targets, dir_weights, counts)``: dense
    ``(B, A)`` / ``(B, A, 7)`` tensors, ``A`` = all anchors in the reference's final order ``(location, C, R)``,
    labels and direction bins int64, the rest fp32; ``counts`` ``(B, 2)`` int32 = positives and negatives per
    image, on the device.  Nothing is copied to the host.  A setting the kernel does not cover (an ignore
    threshold with ignore boxes, a tuple ``neg_iou_thr``, boxes that are not 7 wide, another sampler) raises
    ``DfmHipError`` from the C entry."""
    require_gpu(anchors, 'anchors')
    device = anchors.device
    f = _assigner_fields(assigners)
    if anchors.dim() < 3:
        raise ValueError(f'anchors are (..., C, R, 7), got {tuple(anchors.shape)}')
    width = anchors.shape[-1]
    if isinstance(assigners, (list, tuple)):
        slots, rotations = anchors.shape[-3], anchors.shape[-2]
        if len(assigners) != slots:
            raise ValueError(f'{len(assigners)} assigners for {slots} class slots of anchors')
        per_class = bool(assign_per_class)
    else:
        slots, rotations, per_class = 1, 1, False
    if slots > MAX_SLOTS:
        raise ValueError(f'{slots} class slots: at most {MAX_SLOTS}')
    a = _f32(anchors).view(-1, width)
    num_anchors = a.shape[0]
    batch = len(gt_bboxes_list)
    if gt_labels_list is not None and len(gt_labels_list) != batch:
        raise ValueError('gt_bboxes_list and gt_labels_list name different numbers of images')
    gts = [_gt_tensor(g, device) for g in gt_bboxes_list]
    for g in gts:
        if g.shape[0] and g.shape[1] != width:
            raise ValueError(f'GT boxes are {g.shape[1]} wide, anchors {width}')
    has_labels = gt_labels_list is not None
    if has_labels:
        for g, l in zip(gts, gt_labels_list):
            require_gpu(l, 'gt_labels')
            if l.shape[0] != g.shape[0]:
                raise ValueError('one label per GT box')
    tuple_neg = any(isinstance(v, (tuple, list)) for v in f['neg'])
    lib = _capi.lib()
    labels = torch.empty((batch, num_anchors), dtype=torch.int64, device=device)
    dir_targets = torch.empty((batch, num_anchors), dtype=torch.int64, device=device)
    label_weights = torch.empty((batch, num_anchors), dtype=torch.float32, device=device)
    dir_weights = torch.empty((batch, num_anchors), dtype=torch.float32, device=device)
    bbox_targets = torch.empty((batch, num_anchors, width), dtype=torch.float32, device=device)
    bbox_weights = torch.empty((batch, num_anchors, width), dtype=torch.float32, device=device)
    counts = torch.empty((batch, 2), dtype=torch.int32, device=device)
    for b0 in range(0, batch, MAX_BATCH):                      # (one call up to MAX_BATCH images)
        part = gts[b0:b0 + MAX_BATCH]
        nb = len(part)
        d = _capi.AnchorTargetDesc(
            num_locations=num_anchors // (slots * rotations), num_slots=slots, num_rotations=rotations,
            box_width=width, batch=nb, num_classes=int(num_classes), has_labels=int(has_labels),
            assign_per_class=int(per_class), match_low_quality=int(f['match_low_quality']),
            gt_max_assign_all=int(f['gt_max_assign_all']),
            sampler=_capi.SAMPLER_PSEUDO if sampler == 'PseudoSampler' else 1,
            neg_iou_thr_is_range=int(tuple_neg), num_ignore_boxes=int(num_ignore_boxes),
            ignore_iof_thr=f['ignore_iof_thr'], dir_offset=float(dir_offset),
            dir_limit_offset=float(dir_limit_offset), pos_weight=float(pos_weight))
        for c in range(slots):
            d.pos_iou_thr[c] = float(f['pos'][c])
            d.neg_iou_thr[c] = 0.0 if tuple_neg else float(f['neg'][c])
            d.min_pos_iou[c] = float(f['min_pos'][c])
        offsets = (ctypes.c_int32 * (nb + 1))()
        for i, g in enumerate(part):
            offsets[i + 1] = offsets[i] + g.shape[0]
        total = offsets[nb]
        gt = torch.cat(part) if total else a[:0]
        gl = None
        if has_labels and total:
            gl = torch.cat([l.detach().to(device=device, dtype=torch.int64).view(-1)
                            for l in gt_labels_list[b0:b0 + nb]]).contiguous()
        launch('dfm_anchor_target_3d', d, a, gt if total else None, gl, offsets, labels[b0:], label_weights[b0:],
               bbox_targets[b0:], bbox_weights[b0:], dir_targets[b0:], dir_weights[b0:], counts[b0:], WS, STREAM,
               ws_bytes=lib.dfm_anchor_target_workspace_bytes(slots, total))
    return labels, label_weights, bbox_targets, bbox_weights, dir_targets, dir_weights, counts


class HipAnchorTrainMixin(object):
    """``AnchorTrainMixin.anchor_target_3d`` (train_mixins.py:12-100) on the HIP path, for a head class
    ``class FastHead(HipAnchorTrainMixin, LIGAAnchor3DHead)`` (``patch_reference()`` rebinds the reference
    mixin's method to this one).  It reads ``self.bbox_assigner``, ``self.bbox_sampler``, ``self.bbox_coder``,
    ``self.train_cfg``, ``self.dir_offset``, ``self.dir_limit_offset``, ``self.assign_per_class`` and
    ``self.box_code_size`` as the reference does, and returns its tuple: six per-level lists of ``(B, n_level,
    ...)`` tensors, then ``num_total_pos`` and ``num_total_neg`` as Python ints with each image's count clamped
    to at least 1.  The counts are the only data read back from the device.

    A configuration the kernels do not cover (per-image anchor sets, per-class anchor lists, a sampler other
    than ``PseudoSampler``, an assigner that is no ``MaxIoUAssigner`` over nearest-BEV overlaps, ignore boxes
    with ``ignore_iof_thr > 0``, a tuple ``neg_iou_thr``, boxes that are not 7 wide) follows the package's
    fallback policy: 'warn' says so once and calls the reference method, 'raise' (``fallback_policy = 'raise'`` on
    the head, or ``set_fallback_policy('raise')``) makes it an ``MfmaPathError``; without a reference method to
    call it is an error either way."""

    def _anchor_target_unsupported(self, anchor_list, gt_bboxes_ignore_list, gt_labels_list, sampling):
        levels = anchor_list[0]
        if isinstance(levels[0], (list, tuple)):
            return 'per-class anchor lists (anchors of different feature map sizes)'
        if any(img is not anchor_list[0] and any(x is not y for x, y in zip(img, levels)) for img in anchor_list):
            return 'anchors that differ between the images'
        if sampling or type(getattr(self, 'bbox_sampler', None)).__name__ != 'PseudoSampler':
            return 'a sampler other than PseudoSampler'
        assigners = self.bbox_assigner if isinstance(self.bbox_assigner, (list, tuple)) else [self.bbox_assigner]
        for a in assigners:
            kind = a.get('type') if isinstance(a, dict) else type(a).__name__
            if kind != 'MaxIoUAssigner':
                return f'the assigner {kind}'
            calc = _field(a, 'iou_calculator', None)
            kind = calc.get('type') if isinstance(calc, dict) else type(calc).__name__
            if calc is not None and kind != 'BboxOverlapsNearest3D':
                return f'the IoU calculator {kind}'
            if isinstance(_field(a, 'neg_iou_thr', 0.), (tuple, list)):
                return 'a (low, high) neg_iou_thr'
            ignored = any(g is not None and len(g) > 0 for g in (gt_bboxes_ignore_list or []))
            if ignored and float(_field(a, 'ignore_iof_thr', -1)) > 0:
                return 'ignore boxes with ignore_iof_thr > 0'
        if type(getattr(self, 'bbox_coder', None)).__name__ not in ('DeltaXYZWLHRBBoxCoder', 'NoneType'):
            return f'the box coder {type(self.bbox_coder).__name__}'
        if levels[0].shape[-1] != 7:
            return f'{levels[0].shape[-1]}-wide boxes'
        if isinstance(self.bbox_assigner, (list, tuple)) and len(levels) > 1 and \
                any(l.shape[-3:] != levels[0].shape[-3:] for l in levels):
            return 'levels with different anchor sets per location'
        if gt_labels_list is None and getattr(self, 'assign_per_class', False):
            return 'assign_per_class without gt_labels'
        return None

    def anchor_target_3d(self, anchor_list, gt_bboxes_list, input_metas, gt_bboxes_ignore_list=None,
                         gt_labels_list=None, label_channels=1, num_classes=1, sampling=True):
        num_imgs = len(input_metas)
        assert len(anchor_list) == num_imgs
        why = self._anchor_target_unsupported(anchor_list, gt_bboxes_ignore_list, gt_labels_list, sampling)
        if why is not None:
            return run_reference(self, 'anchor_target_3d', why, 'anchor-target',
                                 (anchor_list, gt_bboxes_list, input_metas, gt_bboxes_ignore_list, gt_labels_list,
                                  label_channels, num_classes, sampling), mixin=HipAnchorTrainMixin)
        levels = anchor_list[0]
        code = getattr(self, 'box_code_size', levels[0].shape[-1])
        num_level_anchors = [l.view(-1, code).size(0) for l in levels]            # train_mixins.py:55-58
        anchors = torch.cat(list(levels)) if len(levels) > 1 else levels[0]
        train_cfg = self.train_cfg
        pos_weight = train_cfg['pos_weight'] if isinstance(train_cfg, dict) else train_cfg.pos_weight
        *dense, counts = anchor_target_3d(
            anchors, gt_bboxes_list, gt_labels_list, self.bbox_assigner, num_classes=num_classes,
            assign_per_class=getattr(self, 'assign_per_class', False), dir_offset=self.dir_offset,
            dir_limit_offset=self.dir_limit_offset, pos_weight=pos_weight)
        pos_neg = counts.clamp(min=1).sum(0).tolist()        # the one host read (train_mixins.py:86-87)
        out = []
        for t in dense:                                      # images_to_levels: (B, A, ...) split by level
            start, per_level = 0, []
            for n in num_level_anchors:
                per_level.append(t[:, start:start + n])
                start += n
            out.append(per_level)
        return (*out, int(pos_neg[0]), int(pos_neg[1]))
