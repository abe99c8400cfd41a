"""Differentiable rotated IoU and ``IOU3DLoss`` on the HIP path.

Mirror of ``mmdet3d/models/losses/iou3d_loss.py`` (``iou3d_loss``, ``IOU3DLoss``), whose
``mmcv.ops.diff_iou_rotated_3d`` is a CUDA extension, and of the IoU term of
``LIGAAnchor3DHead.loss_single`` (dense_heads/liga_anchor3d_head.py:210-224).  mmcv is not a dependency: the
semantics are those stated in include/dfm_hip.h -- box ``(x, y, z, dx, dy, dz, yaw)``, BEV rectangle centre
``(x, y)`` size ``(dx, dy)`` turned counter-clockwise by ``yaw``, z interval ``[z - dz/2, z + dz/2]``,
``IoU3D = I Z / (V1 + V2 - I Z)``; value and gradient 0 for empty boxes and for pairs that do not overlap (mmcv's
NaN from 0 / 0 is not reproduced).

``diff_iou_rotated_3d`` / ``diff_iou_rotated_2d`` make one launch (``dfm_diff_iou_rotated``) that returns the IoU
and both gradient rows; the backward is two broadcasts.  mmcv's path is about forty torch ops and a vertex-sort
kernel.  ``iou3d_loss_from_deltas`` is the head's call pattern in one launch (``dfm_iou3d_loss_from_deltas``):
gather the positive rows, decode prediction and target with ``DeltaXYZWLHRBBoxCoder.decode``, apply the
NaN-target rule, IoU, and the Jacobian row with respect to the prediction's deltas.

Inputs of any floating dtype or stride are converted to contiguous fp32 (the kernels compute in fp32); gradients
come back in the input's dtype.  CPU tensors are refused: there is no CPU path.  Nothing here copies from the
device to the host.
"""
import torch
import torch.nn as nn

from . import _capi
from ._launch import STREAM, launch, require_gpu
from .registry import register_module

__all__ = ['diff_iou_rotated_3d', 'diff_iou_rotated_2d', 'iou3d_loss', 'IOU3DLoss', 'iou3d_loss_from_deltas']


def _f32(t):
    return t.detach().to(torch.float32).contiguous()


class _DiffIoUFn(torch.autograd.Function):
    """one launch forward: the IoU and, when an input needs a gradient, both gradient rows (saved)"""

    @staticmethod
    def forward(ctx, box1, box2):
        device = box1.device
        width = box1.shape[-1]
        b1, b2 = _f32(box1).view(-1, width), _f32(box2).view(-1, width)
        n = b1.shape[0]
        iou = torch.zeros(n, dtype=torch.float32, device=device)
        want = any(ctx.needs_input_grad)
        g1 = torch.empty_like(b1) if want else None
        g2 = torch.empty_like(b2) if want else None
        if n:
            launch('dfm_diff_iou_rotated', b1, b2, n, width, iou, g1 if want else None, g2 if want else None, STREAM)
        if want:
            ctx.save_for_backward(g1, g2)
        ctx.shapes = (box1.shape, box1.dtype, box2.shape, box2.dtype)
        return iou.view(box1.shape[:-1])

    @staticmethod
    def backward(ctx, grad_iou):
        g1, g2 = ctx.saved_tensors
        s1, d1, s2, d2 = ctx.shapes
        g = grad_iou.detach().to(torch.float32).reshape(-1, 1)
        out1 = (g * g1).view(s1).to(d1) if ctx.needs_input_grad[0] else None
        out2 = (g * g2).view(s2).to(d2) if ctx.needs_input_grad[1] else None
        return out1, out2


def _diff_iou(box1, box2, width, name):
    require_gpu(box1, 'box1')
    require_gpu(box2, 'box2')
    if box1.shape != box2.shape or box1.dim() != 3 or box1.shape[-1] != width:
        raise ValueError(f'{name} takes two (B, N, {width}) tensors, got {tuple(box1.shape)} and '
                         f'{tuple(box2.shape)}')
    if not (box1.is_floating_point() and box2.is_floating_point()):
        raise TypeError(f'{name} takes floating-point boxes')
    return _DiffIoUFn.apply(box1, box2)


def diff_iou_rotated_3d(box3d1, box3d2):
    """IoU of corresponding rotated 3-D boxes: two ``(B, N, 7)`` tensors ``(x, y, z, dx, dy, dz, yaw)`` ->
    ``(B, N)`` fp32, differentiable with respect to both (mmcv.ops.diff_iou_rotated_3d's signature)."""
    return _diff_iou(box3d1, box3d2, 7, 'diff_iou_rotated_3d')


def diff_iou_rotated_2d(box1, box2):
    """IoU of corresponding rotated rectangles: two ``(B, N, 5)`` tensors ``(x, y, w, h, angle)`` -> ``(B, N)``
    fp32, differentiable with respect to both (mmcv.ops.diff_iou_rotated_2d's signature)."""
    return _diff_iou(box1, box2, 5, 'diff_iou_rotated_2d')


def _weight_reduce(loss, weight, reduction, avg_factor):
    """mmdet's ``weighted_loss`` rules (mmdet/models/losses/utils.py): ``avg_factor`` applies with 'mean' (an
    exact division; a device tensor costs no host sync), leaves 'none' alone and is an error with 'sum'"""
    if weight is not None:
        loss = loss * weight
    if avg_factor is None:
        if reduction == 'mean':
            return loss.mean()
        if reduction == 'sum':
            return loss.sum()
        if reduction != 'none':
            raise ValueError(f"reduction must be 'none', 'mean' or 'sum', got {reduction!r}")
        return loss
    if reduction == 'mean':
        return loss.sum() / avg_factor
    if reduction != 'none':
        raise ValueError('avg_factor can not be used with reduction="sum"')
    return loss


def iou3d_loss(pred, target, weight=None, reduction='mean', avg_factor=None):
    """``1 - IoU3D`` of ``pred`` and ``target``, two ``(N, 7)`` tensors, with the arguments and the results of
    the reference function (iou3d_loss.py:10-32 under mmdet's ``weighted_loss``): a NaN component of ``target``
    is replaced by ``pred``'s, so its gradient reaches ``pred`` through both arguments; the element-wise loss
    has shape ``(1, N)`` as the reference's has; with ``N == 0`` it is ``(pred - target).sum(1) * 0.`` -- the
    branch the reference wrote for that case but cannot reach behind its ``assert target.numel() > 0``, while
    ``loss_single`` calls it for an image without positives all the same."""
    require_gpu(pred, 'pred')
    require_gpu(target, 'target')
    target = torch.where(torch.isnan(target), pred, target)
    if pred.size(0) > 0:
        loss = 1 - diff_iou_rotated_3d(pred.unsqueeze(0), target.unsqueeze(0))
    else:
        loss = (pred - target).sum(1) * 0.
    return _weight_reduce(loss, weight, reduction, avg_factor)


@register_module(on_path=False)
class IOU3DLoss(nn.Module):
    """``IOU3DLoss`` of the reference (iou3d_loss.py:35-82): ``loss_weight * iou3d_loss(...)``; built from
    ``dict(type='IOU3DLoss', loss_weight=1.0)`` as the KITTI configs' ``loss_iou``."""

    def __init__(self, reduction='mean', loss_weight=1.0):
        super().__init__()
        assert reduction in ['none', 'sum', 'mean']
        self.reduction = reduction
        self.loss_weight = loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None, **kwargs):
        assert reduction_override in (None, 'none', 'mean', 'sum')
        reduction = reduction_override if reduction_override else self.reduction
        return self.loss_weight * iou3d_loss(pred, target, weight, reduction=reduction, avg_factor=avg_factor,
                                             **kwargs)


class _FromDeltasFn(torch.autograd.Function):
    """one launch forward: the per-row loss and its Jacobian row with respect to bbox_pred's deltas (saved)"""

    @staticmethod
    def forward(ctx, bbox_pred, anchors, bbox_targets, pos_inds):
        device = bbox_pred.device
        a, p, t = _f32(anchors), _f32(bbox_pred), _f32(bbox_targets)
        rows, size = p.shape
        num_pos = pos_inds.shape[0]
        loss = torch.ones(num_pos, dtype=torch.float32, device=device)
        want = ctx.needs_input_grad[0]
        jac = torch.empty((num_pos, 7), dtype=torch.float32, device=device) if want else None
        if num_pos:
            launch('dfm_iou3d_loss_from_deltas', a, p, t, pos_inds, rows, size, num_pos, loss,
                   jac, STREAM)
        if want:
            ctx.save_for_backward(jac, pos_inds)
        ctx.meta = (bbox_pred.shape, bbox_pred.dtype)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        jac, pos_inds = ctx.saved_tensors
        shape, dtype = ctx.meta
        grad = torch.zeros(shape, dtype=torch.float32, device=jac.device)
        # unique rows: a plain indexed store, no atomics
        grad[pos_inds, :7] = grad_loss.detach().to(torch.float32).reshape(-1, 1) * jac
        return grad.to(dtype), None, None, None


def iou3d_loss_from_deltas(anchors, bbox_pred, bbox_targets, pos_inds, bbox_weights=None):
    """The IoU term of ``loss_single`` before its reduction, in one launch: the ``(P,)`` fp32 loss

        iou3d_loss(decode(anchors[pos_inds], bbox_pred[pos_inds]),
                   decode(anchors[pos_inds], bbox_targets[pos_inds]), reduction='none')

    with ``decode = DeltaXYZWLHRBBoxCoder.decode``, differentiable with respect to ``bbox_pred``.
    ``anchors``, ``bbox_pred``, ``bbox_targets``: ``(R, S)``, ``S >= 7``, columns beyond 7 ignored;
    ``pos_inds``: ``(P,)`` int64, unique rows (what ``nonzero`` returns).  ``bbox_weights``: optional ``(P,)``
    per-row weights multiplied in.  Rows of ``bbox_pred`` outside ``pos_inds`` get exactly zero gradient."""
    for name, t in (('anchors', anchors), ('bbox_pred', bbox_pred), ('bbox_targets', bbox_targets),
                    ('pos_inds', pos_inds)):
        require_gpu(t, name)
    if not (anchors.dim() == 2 and anchors.shape == bbox_pred.shape == bbox_targets.shape and anchors.shape[1] >= 7):
        raise ValueError(f'anchors, bbox_pred and bbox_targets share one (R, S >= 7) shape, got '
                         f'{tuple(anchors.shape)}, {tuple(bbox_pred.shape)}, {tuple(bbox_targets.shape)}')
    if pos_inds.dim() != 1 or pos_inds.dtype != torch.int64:
        raise ValueError('pos_inds is a 1-D int64 tensor of row indices')
    loss = _FromDeltasFn.apply(bbox_pred, anchors, bbox_targets, pos_inds.contiguous())
    return loss if bbox_weights is None else loss * bbox_weights
