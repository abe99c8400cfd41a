"""2-D box overlaps and the 2-D ATSS head's training targets on the HIP path.

Mirror of mmdet's ``bbox_overlaps`` / ``BboxOverlaps2D`` and of what ``ATSSHead.get_targets`` runs once per image for
the KITTI configs' ``bbox_head_2d = LIGAATSSHead``: ``LIGAATSSHead._get_target_single`` (mmdet3d/models/dense_heads/
liga_atss_head.py:399-483) -- ``anchor_inside_flags``, ``ATSS3DCenterAssigner.assign`` (mmdet3d/core/bbox/assigners/
atss_3dcenter_assigner.py:27-168), ``PseudoSampler``, ``DeltaXYWHBBoxCoder.encode``, ``unmap``.  mmdet is not a
dependency: the semantics are those stated in include/dfm_hip_atss_target.h.

The reference materialises an anchors x G overlap matrix and an anchors x G distance matrix per image and walks them
with a ``topk`` per level, a Python loop over the GT boxes, a G x anchors scatter and half a dozen ``nonzero``s, each
of which waits for the device.  ``atss_target_2d`` here is one call of ``dfm_atss_target_2d`` for the whole batch: a
memset of the per-anchor keys and three launches, neither matrix in memory, nothing copied to the host.
``HipATSSTargetMixin`` wraps its dense ``(B, A, ...)`` outputs into the reference method's return tuple, which costs
the one small copy of the per-image counts.

Boxes and anchors of any floating dtype or stride are converted to contiguous fp32.  CPU tensors are refused: there
is no CPU path.
"""
import ctypes

import torch

from . import _capi
from .fallback import run_reference
from ._launch import STREAM, WS, launch, require_gpu, upload
from .registry import register_module

__all__ = ['bbox_overlaps', 'BboxOverlaps2D', 'atss_target_2d', 'HipATSSTargetMixin']

MAX_LEVELS, MAX_TOPK, MAX_BATCH = _capi.ATSS_MAX_LEVELS, _capi.ATSS_MAX_TOPK, _capi.ATSS_MAX_BATCH


def _f32(t):
    return t.detach().to(torch.float32).contiguous()


def bbox_overlaps(bboxes1, bboxes2, mode='iou', is_aligned=False, eps=1e-6):
    """IoU (or IoF) of two sets of boxes ``(N, 4)`` and ``(M, 4)``, ``(x1, y1, x2, y2)`` -> ``(N, M)`` fp32, or
    ``(N,)`` when ``is_aligned`` (mmdet's signature, mmdet/core/bbox/iou_calculators/iou2d_calculator.py).  The
    kernel's ``eps`` is mmdet's default 1e-6; any other value raises."""
    require_gpu(bboxes1, 'bboxes1')
    require_gpu(bboxes2, 'bboxes2')
    if mode not in ('iou', 'iof'):
        raise ValueError(f"mode must be 'iou' or 'iof', got {mode!r}")
    if eps != 1e-6:
        raise ValueError(f'bbox_overlaps is built with eps = 1e-6, got {eps!r}')
    if bboxes1.dim() != 2 or bboxes2.dim() != 2 or bboxes1.size(-1) != 4 or bboxes2.size(-1) != 4:
        raise ValueError(f'bbox_overlaps takes (N, 4) and (M, 4) boxes, got {tuple(bboxes1.shape)} and '
                         f'{tuple(bboxes2.shape)}')
    n, m = bboxes1.shape[0], bboxes2.shape[0]
    if is_aligned and n != m:
        raise ValueError(f'aligned overlaps need as many bboxes2 as bboxes1, got {n} and {m}')
    out = torch.empty((n,) if is_aligned else (n, m), dtype=torch.float32, device=bboxes1.device)
    if out.numel():
        launch('dfm_bbox_overlaps_2d', _f32(bboxes1), n, _f32(bboxes2), m,
               _capi.OVERLAP_IOF if mode == 'iof' else _capi.OVERLAP_IOU, int(bool(is_aligned)), out, STREAM)
    return out


@register_module(on_path=False)
class BboxOverlaps2D(object):
    """mmdet's ``BboxOverlaps2D``: built from ``dict(type='BboxOverlaps2D')``, the default ``iou_calculator`` of
    ``ATSS3DCenterAssigner``.  As there, boxes wider than 4 columns (a score column) are cut to 4."""

    def __init__(self, scale=1., dtype=None):
        self.scale, self.dtype = scale, dtype

    def __call__(self, bboxes1, bboxes2, mode='iou', is_aligned=False):
        assert bboxes1.size(-1) in [0, 4, 5] and bboxes2.size(-1) in [0, 4, 5]
        return bbox_overlaps(bboxes1[..., :4], bboxes2[..., :4], mode, is_aligned)

    def __repr__(self):
        return f'{self.__class__.__name__}(scale={self.scale}, dtype={self.dtype})'


def atss_target_2d(anchors, num_level_anchors, gt_bboxes_list, gt_labels_list, *, topk, num_classes, pos_weight=-1,
                   inside_flags=None, target_means=(0., 0., 0., 0.), target_stds=(0.1, 0.1, 0.2, 0.2),
                   thresh_mode='meanstd', reg_width=4, coder='DeltaXYWHBBoxCoder', sampler='PseudoSampler',
                   ignore_iof_thr=-1, num_ignore_boxes=0):
    """The training targets of every anchor of the 2-D ATSS head for a batch.

    ``anchors``: ``(A, 4)``, the anchors of ONE image with the levels concatenated, shared by every image;
    ``num_level_anchors``: the level sizes, summing to ``A``.  ``gt_bboxes_list``: per image ``(G, 6)`` -- the 2-D
    box and the projected 3-D centre, ``append_3d_centers`` -- or ``(G, 4)``, the same width for every image;
    ``gt_labels_list``: per image ``(G,)`` integer labels, or None (every label 0).  ``inside_flags``: ``(B, A)``
    bool / uint8, the anchors that count for each image (mmdet's ``anchor_inside_flags``), or None: all of them.

    Returns ``(labels, label_weights, bbox_targets, bbox_weights, assigned_gt_inds, counts)``: dense ``(B, A)`` /
    ``(B, A, 4)`` tensors in the anchor order given, labels and assigned indices int64, the rest fp32; ``counts``
    ``(B, 2)`` int32 = positives and negatives per image, on the device.  Nothing is copied to the host.  It never
    falls back: a setting the kernels do not cover (the trailing keywords: ``thresh_mode='ratio'``, another
    regression width, coder or sampler, ignore boxes with ``ignore_iof_thr > 0``) raises ``DfmHipError`` from the C
    entry."""
    require_gpu(anchors, 'anchors')
    device = anchors.device
    if anchors.dim() != 2 or anchors.shape[1] != 4:
        raise ValueError(f'anchors are (A, 4), got {tuple(anchors.shape)}')
    a = _f32(anchors)
    num_anchors = a.shape[0]
    sizes = [int(n) for n in num_level_anchors]
    if not 1 <= len(sizes) <= MAX_LEVELS:
        raise ValueError(f'{len(sizes)} levels: 1 to {MAX_LEVELS}')
    if sum(sizes) != num_anchors or min(sizes) < 0:
        raise ValueError(f'the level sizes {sizes} do not sum to the {num_anchors} anchors')
    batch = len(gt_bboxes_list)
    if gt_labels_list is not None and len(gt_labels_list) != batch:
        raise ValueError('gt_bboxes_list and gt_labels_list name different numbers of images')
    gts = []
    for g in gt_bboxes_list:
        require_gpu(g, 'gt_bboxes')
        gts.append(_f32(g).view(-1, g.shape[-1] if g.dim() > 1 else 6))
    widths = {g.shape[1] for g in gts}
    if len(widths) > 1:
        raise ValueError(f'the GT boxes of one batch share their width, got {sorted(widths)}')
    width = widths.pop() if widths else 6
    if gt_labels_list is not None:
        for g, l in zip(gts, gt_labels_list):
            require_gpu(l, 'gt_labels')
            if l.shape[0] != g.shape[0]:
                raise ValueError('one label per GT box')
    inside = None
    if inside_flags is not None:
        require_gpu(inside_flags, 'inside_flags')
        if tuple(inside_flags.shape) != (batch, num_anchors):
            raise ValueError(f'inside_flags are (B, A) = {(batch, num_anchors)}, got {tuple(inside_flags.shape)}')
        inside = inside_flags.detach().ne(0).to(torch.uint8).contiguous()
    lib = _capi.lib()
    level_sizes = (ctypes.c_int32 * len(sizes))(*sizes)
    labels = torch.empty((batch, num_anchors), dtype=torch.int64, device=device)
    assigned = torch.empty((batch, num_anchors), dtype=torch.int64, device=device)
    label_weights = torch.empty((batch, num_anchors), dtype=torch.float32, device=device)
    bbox_targets = torch.empty((batch, num_anchors, 4), dtype=torch.float32, device=device)
    bbox_weights = torch.empty((batch, num_anchors, 4), dtype=torch.float32, device=device)
    counts = torch.empty((batch, 2), dtype=torch.int32, device=device)
    for b0 in range(0, batch, MAX_BATCH):                      # (one call up to MAX_BATCH images)
        part = gts[b0:b0 + MAX_BATCH]
        nb = len(part)
        d = _capi.AtssTargetDesc(
            num_anchors=num_anchors, num_levels=len(sizes), batch=nb, gt_width=width, topk=int(topk),
            num_classes=int(num_classes),
            thresh_mode=_capi.ATSS_THRESH_MEANSTD if thresh_mode == 'meanstd' else _capi.ATSS_THRESH_RATIO,
            reg_width=int(reg_width), coder=_capi.ATSS_CODER_DELTA_XYWH if coder == 'DeltaXYWHBBoxCoder' else 1,
            sampler=_capi.SAMPLER_PSEUDO if sampler == 'PseudoSampler' else 1,
            num_ignore_boxes=int(num_ignore_boxes), ignore_iof_thr=float(ignore_iof_thr),
            pos_weight=float(pos_weight))
        for c in range(4):
            d.target_means[c], d.target_stds[c] = float(target_means[c]), float(target_stds[c])
        offsets = (ctypes.c_int32 * (nb + 1))()
        for i, g in enumerate(part):
            offsets[i + 1] = offsets[i] + g.shape[0]
        total = offsets[nb]
        gt = torch.cat(part) if total else None
        gl = None
        if gt_labels_list is not None and total:
            gl = torch.cat([l.detach().to(device=device, dtype=torch.int64).view(-1)
                            for l in gt_labels_list[b0:b0 + nb]]).contiguous()
        launch('dfm_atss_target_2d', d, a, level_sizes, None if inside is None else inside[b0:b0 + nb], gt, offsets,
               gl, labels[b0:], label_weights[b0:], bbox_targets[b0:], bbox_weights[b0:], assigned[b0:], counts[b0:],
               WS, STREAM, ws_bytes=lib.dfm_atss_target_workspace_bytes(ctypes.byref(d), total))
    return labels, label_weights, bbox_targets, bbox_weights, assigned, counts


def _field(obj, name, default):
    if isinstance(obj, dict):
        return obj.get(name, default)
    return getattr(obj, name, default)


def _kind(obj):
    return obj.get('type') if isinstance(obj, dict) else type(obj).__name__


def head_dense_targets(head, anchor_list, valid_flag_list, gt_bboxes_list, img_metas, gt_labels_list):
    """``atss_target_2d`` for a head's lists, as ``HipATSSTargetMixin.get_targets`` and ``HipATSSLossMixin.loss`` (the
    next step of the same path) call it: the level-concatenated anchors of the first image, ``anchor_inside_flags`` of
    every image at once on the device, the head's assigner, coder and ``train_cfg`` read by attribute.  Returns
    ``(anchors (A, 4+), num_level_anchors, inside (B, A) bool, [labels, label_weights, bbox_targets, bbox_weights],
    counts (B, 2) int32)``, everything on the device; nothing is copied to the host."""
    levels = anchor_list[0]
    num_level_anchors = [l.size(0) for l in levels]
    anchors = torch.cat(list(levels)) if len(levels) > 1 else levels[0]
    require_gpu(anchors, 'anchors')
    train_cfg = head.train_cfg
    border = _field(train_cfg, 'allowed_border', -1)
    # anchor_inside_flags for every image at once, on the device
    inside = torch.stack([torch.cat(list(flags)) if len(flags) > 1 else flags[0] for flags in valid_flag_list])
    inside = inside.to(anchors.device).ne(0)
    if border >= 0:
        hw = upload(torch.tensor([[float(m['img_shape'][0]), float(m['img_shape'][1])] for m in img_metas],
                                 dtype=torch.float32), anchors.device)
        a = anchors.to(torch.float32)
        inside = inside & ((a[:, 0] >= -border) & (a[:, 1] >= -border))[None] & \
            (a[None, :, 2] < hw[:, 1:2] + border) & (a[None, :, 3] < hw[:, 0:1] + border)
    assigner = head.assigner
    width = 6 if _field(assigner, 'append_3d_centers', True) else 4
    coder = head.bbox_coder
    *dense, _, counts = atss_target_2d(
        anchors[:, :4], num_level_anchors, [g[:, :width] for g in gt_bboxes_list], gt_labels_list,
        topk=_field(assigner, 'topk', 9), num_classes=head.num_classes,
        pos_weight=_field(train_cfg, 'pos_weight', -1), inside_flags=inside,
        target_means=getattr(coder, 'means', (0., 0., 0., 0.)), target_stds=getattr(coder, 'stds', (1., 1., 1., 1.)))
    return anchors, num_level_anchors, inside, dense, counts


class HipATSSTargetMixin(object):
    """``ATSSHead.get_targets`` as ``LIGAATSSHead`` runs it (mmdet's method over ``LIGAATSSHead._get_target_single``,
    liga_atss_head.py:399-483) on the HIP path, for a head class ``class FastHead(HipATSSTargetMixin, LIGAATSSHead)``
    (``patch_reference()`` rebinds ``LIGAATSSHead.get_targets`` to this one).  It reads ``self.assigner``,
    ``self.sampler``, ``self.bbox_coder``, ``self.train_cfg.allowed_border``, ``self.train_cfg.pos_weight``,
    ``self.num_classes`` and ``self.num_reg_channel`` as the reference does, and returns its tuple: per-level lists
    of ``(B, n_level, ...)`` anchors, labels, label weights, bbox targets and bbox weights, then ``num_total_pos``
    and ``num_total_neg`` as Python ints with each image's count clamped to at least 1.  The counts are the only
    data read back from the device.  The anchors of the result are the input anchors with zero rows where the anchor
    does not count for the image (mmdet's ``unmap``).

    An image without any counting anchor gives all-zero weights here; the reference returns ``None`` for the whole
    batch in that case, after a host wait on ``inside_flags.any()``.

    A configuration the kernels do not cover (``thresh_mode='ratio'``, an assigner that is no
    ``ATSS3DCenterAssigner`` over ``BboxOverlaps2D``, ignore boxes with ``ignore_iof_thr > 0``, a regression width
    other than 4, a coder other than ``DeltaXYWHBBoxCoder``, a sampler other than ``PseudoSampler``, anchors that
    differ between the images, more than one anchor per location) follows the package's fallback policy: 'warn' says
    so once and calls the reference method, 'raise' (``fallback_policy = 'raise'`` on the head, or
    ``set_fallback_policy('raise')``) makes it an ``MfmaPathError``; without a reference method to call it is an
    error either way."""

    def _atss_target_unsupported(self, anchor_list, gt_bboxes_ignore_list):
        assigner = getattr(self, 'assigner', None)
        if _kind(assigner) != 'ATSS3DCenterAssigner':
            return f'the assigner {_kind(assigner)}'
        if _field(assigner, 'thresh_mode', 'meanstd') != 'meanstd':
            return f"thresh_mode={_field(assigner, 'thresh_mode', None)!r}"
        calc = _field(assigner, 'iou_calculator', None)
        if calc is not None and _kind(calc) != 'BboxOverlaps2D':
            return f'the IoU calculator {_kind(calc)}'
        ignored = any(g is not None and len(g) > 0 for g in (gt_bboxes_ignore_list or []))
        if ignored and float(_field(assigner, 'ignore_iof_thr', -1)) > 0:
            return 'ignore boxes with ignore_iof_thr > 0'
        if getattr(self, 'num_reg_channel', 4) not in (4, None):
            return f'{self.num_reg_channel} regression channels (num_extra_reg_channel > 0)'
        if type(getattr(self, 'bbox_coder', None)).__name__ != 'DeltaXYWHBBoxCoder':
            return f'the box coder {type(getattr(self, "bbox_coder", None)).__name__}'
        if type(getattr(self, 'sampler', None)).__name__ != 'PseudoSampler':
            return 'a sampler other than PseudoSampler'
        levels = anchor_list[0]
        if any(img is not levels and (len(img) != len(levels) or any(x is not y for x, y in zip(img, levels)))
               for img in anchor_list):
            return 'anchors that differ between the images'
        if getattr(self, 'num_anchors', 1) != 1:
            return f'{self.num_anchors} anchors per location'
        return None

    def get_targets(self, anchor_list, valid_flag_list, gt_bboxes_list, img_metas, gt_bboxes_ignore_list=None,
                    gt_labels_list=None, label_channels=1, unmap_outputs=True):
        num_imgs = len(img_metas)
        assert len(anchor_list) == len(valid_flag_list) == num_imgs
        why = self._atss_target_unsupported(anchor_list, gt_bboxes_ignore_list)
        if why is None and not unmap_outputs:
            why = 'unmap_outputs=False'
        if why is not None:
            return run_reference(self, 'get_targets', why, 'ATSS-target',
                                 (anchor_list, valid_flag_list, gt_bboxes_list, img_metas, gt_bboxes_ignore_list,
                                  gt_labels_list, label_channels, unmap_outputs), mixin=HipATSSTargetMixin)
        anchors, num_level_anchors, inside, dense, counts = head_dense_targets(
            self, anchor_list, valid_flag_list, gt_bboxes_list, img_metas, gt_labels_list)
        pos_neg = counts.clamp(min=1).sum(0).tolist()        # the one host read (mmdet: max(inds.numel(), 1))
        kept = anchors[None] * inside[..., None].to(anchors.dtype)                # unmap: zero rows outside
        out = []
        for t in (kept, *dense):                             # images_to_levels: (B, A, ...) split by level
            start, per_level = 0, []
            for n in num_level_anchors:
                per_level.append(t[:, start:start + n])
                start += n
            out.append(per_level)
        return (*out, int(pos_neg[0]), int(pos_neg[1]))
