"""Rotated / axis-aligned BEV non-maximum suppression and rotated-box IoU on the HIP path.

Mirror of ``box3d_multiclass_nms``, ``nms_bev`` and ``nms_normal_bev`` (mmdet3d/core/post_processing/
box3d_nms.py:8-128, 231-268, 274-288), the last step of ``Anchor3DHead.get_bboxes_single``, whose
``mmcv.ops.nms_rotated`` / ``nms`` are CUDA extensions; and of the ``box_iou_rotated`` op that
``BaseInstance3DBoxes.overlaps`` needs.  mmcv is not a dependency: the semantics are those stated in
include/dfm_hip.h (suppression by IoU strictly greater than the threshold, candidates visited in descending
score order, ``keep`` in that order; ties in score have no defined order in the reference -- here the sort is
stable, so equal scores keep their input order).

The reference loops over the classes in Python with a boolean index, a host sync and a launch pair each.
``box3d_multiclass_nms`` here filters and orders all classes with torch ops on the device (a masked, stable
argsort of ``scores.T``; the per-class counts stay a device tensor), then makes ONE mask launch and ONE reduce
launch for all classes (``dfm_box_nms_rotated`` / ``dfm_box_nms_aligned``); the only device-to-host copy is the
kept counts at the end.

Inputs: boxes of any floating dtype or stride are converted to contiguous fp32 (the kernels read fp32); scores
are only sorted and gathered, in their own dtype (bf16 scores are accepted as they are).  CPU tensors are
refused: there is no CPU path.
"""
import torch

from . import _capi
from ._launch import STREAM, WS, launch, require_gpu

__all__ = ['nms_bev', 'nms_normal_bev', 'box3d_multiclass_nms', 'box_iou_rotated', 'BOX_NMS_MAX_N']

BOX_NMS_MAX_N = _capi.BOX_NMS_MAX_N


def _boxes_f32(boxes):
    return boxes.detach().to(torch.float32).contiguous()


def _launch(boxes, order, counts, thresh, rotated, xyxyr):
    """boxes (num_boxes, 5) fp32; order (classes, n) int64; counts (classes) int32, all on one device.
    Returns (keep (classes, n) int64, kept_counts (classes) int32), both on the device, no sync."""
    lib = _capi.lib()
    device = boxes.device
    classes, n = order.shape
    if n > BOX_NMS_MAX_N:
        raise ValueError(f'{n} candidates per class: box NMS takes at most BOX_NMS_MAX_N = {BOX_NMS_MAX_N} '
                         '(cut them with nms_pre / pre_max_size)')
    keep = torch.empty((classes, n), dtype=torch.int64, device=device)
    kept = torch.zeros(classes, dtype=torch.int32, device=device)
    if n == 0 or classes == 0:
        return keep, kept
    nbytes = lib.dfm_box_nms_workspace_bytes(n, classes)
    if nbytes == 0:
        _capi.check(-1)
    tail = (order, counts, n, classes, float(thresh), keep, kept, WS, STREAM)
    if rotated:
        launch('dfm_box_nms_rotated', boxes, boxes.shape[0], int(xyxyr), *tail, ws_bytes=nbytes)
    else:
        launch('dfm_box_nms_aligned', boxes, boxes.shape[0], *tail, ws_bytes=nbytes)
    return keep, kept


def _single(boxes, scores, thresh, rotated, pre_max_size=None, post_max_size=None):
    require_gpu(boxes, 'boxes')
    require_gpu(scores, 'scores')
    order = torch.sort(scores, dim=0, descending=True, stable=True)[1]
    if pre_max_size is not None:
        order = order[:pre_max_size]
    n = order.shape[0]
    if n == 0:
        return order
    order = order.contiguous().view(1, n)
    counts = torch.full((1,), n, dtype=torch.int32, device=boxes.device)
    keep, kept = _launch(_boxes_f32(boxes), order, counts, thresh, rotated, xyxyr=True)
    keep = keep[0, :int(kept.item())]
    if post_max_size is not None:
        keep = keep[:post_max_size]
    return keep


def nms_bev(boxes, scores, thresh, pre_max_size=None, post_max_size=None):
    """box3d_nms.py:231-268.  boxes (N, 5) = (x1, y1, x2, y2, ry); the xyxyr -> xywhr conversion of the
    reference happens inside the kernel with the same fp32 operations.  Returns the kept indices (int64, into
    ``boxes``) in descending score order."""
    assert boxes.size(1) == 5, 'Input boxes shape should be [N, 5]'
    return _single(boxes, scores, thresh, True, pre_max_size, post_max_size)


def nms_normal_bev(boxes, scores, thresh):
    """box3d_nms.py:274-288.  boxes (N, 5); the IoU is that of the axis-aligned (x1, y1, x2, y2), the angle
    ignored, without a +1 offset.  Returns the kept indices in descending score order."""
    assert boxes.shape[1] == 5, 'Input boxes shape should be [N, 5]'
    return _single(boxes, scores, thresh, False)


def _cfg(cfg, name):
    return cfg[name] if isinstance(cfg, dict) else getattr(cfg, name)


def box3d_multiclass_nms(mlvl_bboxes, mlvl_bboxes_for_nms, mlvl_scores, score_thr, max_num, cfg,
                         mlvl_dir_scores=None, mlvl_attr_scores=None, mlvl_bboxes2d=None):
    """box3d_nms.py:8-128, same arguments and returns: ``(bboxes, scores, labels[, dir_scores][, attr_scores]
    [, bboxes2d])``, classes in ascending order, each class's boxes in descending score order, cut to the
    ``max_num`` best.  ``cfg`` supplies ``use_rotate_nms`` and ``nms_thr`` (attributes or keys).

    All classes go through one mask launch and one reduce launch; the result equals calling this module's
    ``nms_bev`` / ``nms_normal_bev`` once per class on the boolean-indexed candidates, as the reference does."""
    for name, t in (('mlvl_bboxes', mlvl_bboxes), ('mlvl_bboxes_for_nms', mlvl_bboxes_for_nms),
                    ('mlvl_scores', mlvl_scores)):
        require_gpu(t, name)
    assert mlvl_bboxes_for_nms.shape[1] == 5, 'Input boxes shape should be [N, 5]'
    num_classes = mlvl_scores.shape[1] - 1
    total = 0
    if mlvl_scores.shape[0] > 0 and num_classes > 0:
        cls_scores = mlvl_scores[:, :num_classes].t()                     # (C, N)
        valid = cls_scores > score_thr
        counts = valid.sum(dim=1, dtype=torch.int32)
        order = torch.sort(cls_scores.masked_fill(~valid, float('-inf')), dim=1, descending=True,
                           stable=True)[1].contiguous()
        keep, kept = _launch(_boxes_f32(mlvl_bboxes_for_nms), order, counts, _cfg(cfg, 'nms_thr'),
                             bool(_cfg(cfg, 'use_rotate_nms')), xyxyr=True)
        kept_host = kept.cpu().tolist()                                   # the one device-to-host copy
        total = sum(kept_host)
    if total:
        inds = torch.cat([keep[c, :k] for c, k in enumerate(kept_host) if k])
        labels = torch.repeat_interleave(torch.arange(num_classes, device=inds.device), kept.long(),
                                         output_size=total)
        bboxes = mlvl_bboxes[inds]
        scores = mlvl_scores[inds, labels]
        dir_scores = mlvl_dir_scores[inds] if mlvl_dir_scores is not None else None
        attr_scores = mlvl_attr_scores[inds] if mlvl_attr_scores is not None else None
        bboxes2d = mlvl_bboxes2d[inds] if mlvl_bboxes2d is not None else None
        if bboxes.shape[0] > max_num:
            _, top = scores.sort(descending=True)
            top = top[:max_num]
            bboxes, labels, scores = bboxes[top, :], labels[top], scores[top]
            if dir_scores is not None:
                dir_scores = dir_scores[top]
            if attr_scores is not None:
                attr_scores = attr_scores[top]
            if bboxes2d is not None:
                bboxes2d = bboxes2d[top]
    else:
        bboxes = mlvl_scores.new_zeros((0, mlvl_bboxes.size(-1)))
        scores = mlvl_scores.new_zeros((0, ))
        labels = mlvl_scores.new_zeros((0, ), dtype=torch.long)
        dir_scores = mlvl_scores.new_zeros((0, ))
        attr_scores = mlvl_scores.new_zeros((0, ))
        bboxes2d = mlvl_scores.new_zeros((0, 4))
    results = (bboxes, scores, labels)
    if mlvl_dir_scores is not None:
        results = results + (dir_scores, )
    if mlvl_attr_scores is not None:
        results = results + (attr_scores, )
    if mlvl_bboxes2d is not None:
        results = results + (bboxes2d, )
    return results


def box_iou_rotated(bboxes1, bboxes2, aligned=False):
    """Exact IoU of rotated boxes (cx, cy, w, h, angle in radians): ``(N, M)`` fp32, or ``(N,)`` between
    corresponding boxes when ``aligned`` (then M == N).  0 when either area is below 1e-14.  The IoU does not
    depend on whether the angle is counted clockwise or counter-clockwise (mirroring both boxes changes
    nothing)."""
    require_gpu(bboxes1, 'bboxes1')
    require_gpu(bboxes2, 'bboxes2')
    assert bboxes1.shape[-1] == 5 and bboxes2.shape[-1] == 5, 'boxes must be (N, 5) = (cx, cy, w, h, angle)'
    n, m = bboxes1.shape[0], bboxes2.shape[0]
    if aligned and n != m:
        raise ValueError(f'aligned IoU needs as many bboxes2 as bboxes1, got {n} and {m}')
    device = bboxes1.device
    out = torch.zeros((n,) if aligned else (n, m), dtype=torch.float32, device=device)
    if n == 0 or m == 0:
        return out
    b1, b2 = _boxes_f32(bboxes1), _boxes_f32(bboxes2)
    launch('dfm_box_iou_rotated', b1, n, b2, m, int(bool(aligned)), out, STREAM)
    return out
