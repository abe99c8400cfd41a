"""The 2-D ATSS head's loss on the HIP path: every level of the batch in one call.

Mirror of mmdet's ``ATSSHead.loss`` as the KITTI configs' ``bbox_head_2d = LIGAATSSHead`` runs it: ``multi_apply`` of
``LIGAATSSHead.loss_single`` (mmdet3d/models/dense_heads/liga_atss_head.py:176-270) over the five FPN levels, with
``LIGAATSSHead.centerness_target`` (:380-397), ``DeltaXYWHBBoxCoder.decode``, ``FocalLoss``, ``GIoULoss`` and the
sigmoid ``CrossEntropyLoss``.  mmdet is not a dependency: the semantics are those stated in
include/dfm_hip_atss_loss.h (a part of include/dfm_hip.h).

Per level the reference permutes and copies the three maps, gathers the class-specific deltas, waits for the host
three times (``nonzero()``, the ``isnan().any()`` assert, ``GIoULoss``'s ``torch.any(weight > 0)``), gathers the
positive rows four times and decodes boxes three times; around the levels two ``reduce_mean(...).item()`` wait again,
and ``get_targets`` before them reads the counts.  ``atss_loss_2d`` is one ``autograd.Function`` over the 3 L maps: two
launches forward (``dfm_atss_loss_fwd``: the 3 L + 1 sums per workgroup, then their fixed-order sum) and one backward
(``dfm_atss_loss_bwd``: every element of the 3 L map gradients written once).  The maps are read in place (NCHW,
channels-last, any strides; ``cls_score`` / ``centerness`` fp32 or bf16, ``bbox_pred`` of its own dtype), the targets
are the dense tensors ``atss_target_2d`` returns, read where they lie.  ``HipATSSLossMixin.loss`` goes from the head's
maps and the GT boxes to the reference's loss dict without leaving the device: the targets' counts, the centerness
sum and both average factors (all-reduced when a process group is up) stay there.

CPU tensors are refused: there is no CPU path.
"""
import ctypes

import torch

from . import _capi
from .anchor_loss import dist_reduce_mean
from .atss_target import MAX_LEVELS, HipATSSTargetMixin, head_dense_targets
from .fallback import run_reference
from ._launch import DTYPES, STREAM, WS, launch, require_gpu

__all__ = ['atss_loss_2d', 'HipATSSLossMixin', 'counters']

_COUNTERS = {'kernel_launches': 0, 'memsets': 0, 'host_waits': 0}


def counters(reset=False):
    """kernel launches and memsets made by this module's C calls so far, and the times it waited for the host (none:
    the key is there so that a reader sees it is counted); ``reset=True`` zeroes them after reading.  A forward is
    two launches, a backward one, whatever the sizes, the number of levels and the number of positives."""
    out = dict(_COUNTERS)
    if reset:
        for k in _COUNTERS:
            _COUNTERS[k] = 0
    return out


def _pointer_table(tensors):
    """a HOST ``void *[len(tensors)]`` of device addresses, NULL for None; the array keeps the tensors alive"""
    arr = (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])
    arr.tensors = tuple(tensors)
    return arr


def _interleave(cls, reg, ctr):
    """three per-level lists -> the order of the C tables: (cls, reg, ctr) of level 0, of level 1, ..."""
    return [t for level in zip(cls, reg, ctr) for t in level]


def _desc(cls_scores, bbox_preds, centernesses, num_anchors, num_classes, reg_class_agnostic, gamma, alpha, means,
          stds):
    d = _capi.AtssLossDesc(batch=cls_scores[0].shape[0], num_levels=len(cls_scores), num_anchors=num_anchors,
                           num_classes=num_classes, reg_class_agnostic=int(bool(reg_class_agnostic)),
                           dtype=DTYPES[cls_scores[0].dtype], reg_dtype=DTYPES[bbox_preds[0].dtype], gamma=gamma,
                           alpha=alpha)
    d.target_means[:] = [float(v) for v in means]
    d.target_stds[:] = [float(v) for v in stds]
    offset = 0
    for l, (c, r, t) in enumerate(zip(cls_scores, bbox_preds, centernesses)):
        d.h[l], d.w[l], d.row_offset[l] = c.shape[2], c.shape[3], offset
        offset += c.shape[2] * c.shape[3]
        d.cls_stride[4 * l:4 * l + 4] = c.stride()
        d.reg_stride[4 * l:4 * l + 4] = r.stride()
        d.ctr_stride[4 * l:4 * l + 4] = t.stride()
    return d


class _AtssLossFn(torch.autograd.Function):
    """out (3 L + 1,) = (S_cls, S_box, S_ctr) of each level, then T; the backward is one launch over the saved inputs"""

    @staticmethod
    def forward(ctx, desc, targets, *maps):
        levels = desc.num_levels
        anchors, labels, label_weights, bbox_targets = targets
        out = torch.empty(3 * levels + 1, dtype=torch.float32, device=labels.device)
        launch('dfm_atss_loss_fwd', desc, _pointer_table(maps), anchors, labels, label_weights, bbox_targets, out, WS,
               STREAM, ws_bytes=_capi.lib().dfm_atss_loss_workspace_bytes(desc))
        ctx.rows = sum(m.shape[0] * m.shape[2] * m.shape[3] for m in maps[::3])
        if ctx.rows:
            _COUNTERS['kernel_launches'] += 2
        else:
            _COUNTERS['memsets'] += 1
        ctx.save_for_backward(*targets, *maps)
        ctx.desc = desc
        return out

    @staticmethod
    def backward(ctx, grad_out):
        targets, maps = ctx.saved_tensors[:4], ctx.saved_tensors[4:]
        desc = ctx.desc
        levels = desc.num_levels
        g = grad_out.detach().to(torch.float32)[:3 * levels].contiguous()      # T has no gradient
        grads = [torch.empty_like(m) if need else None for m, need in zip(maps, ctx.needs_input_grad[2:])]
        for kind, field in enumerate((desc.grad_cls_stride, desc.grad_reg_stride, desc.grad_ctr_stride)):
            for l in range(levels):
                t = grads[3 * l + kind]
                if t is not None:
                    field[4 * l:4 * l + 4] = t.stride()
        if ctx.rows and any(t is not None for t in grads):
            launch('dfm_atss_loss_bwd', desc, _pointer_table(maps), *targets, g, _pointer_table(grads), STREAM)
            _COUNTERS['kernel_launches'] += 1
        return (None, None, *grads)


def atss_loss_2d(cls_scores, bbox_preds, centernesses, anchors, labels, label_weights, bbox_targets, *, num_classes,
                 reg_class_agnostic=True, gamma=2.0, alpha=0.25, target_means=(0., 0., 0., 0.),
                 target_stds=(0.1, 0.1, 0.2, 0.2)):
    """The term sums of the 2-D ATSS head's loss for every level of a batch.

    ``cls_scores`` / ``bbox_preds`` / ``centernesses``: per-level lists (1 to 8 levels) of the ``(B, C, H, W)`` /
    ``(B, 4 or 4*C, H, W)`` / ``(B, 1, H, W)`` maps as the head returns them, one anchor per location, read in place
    whatever their strides; ``cls_scores`` and ``centernesses`` share one dtype, fp32 or bf16, ``bbox_preds`` have
    their own (the head calls ``.float()`` on them).  With ``reg_class_agnostic=False`` column ``s`` of class ``c`` is
    channel ``s * C + c`` and a row uses the class of its label.  ``anchors`` ``(A, 4)``: the anchors of one image with
    the levels concatenated, ``A = sum H*W``; ``labels`` ``(B, A)`` int64, ``label_weights`` ``(B, A)``,
    ``bbox_targets`` ``(B, A, 4)``: what ``atss_target_2d`` returns for those anchors (floating targets of another
    dtype or stride are converted to contiguous fp32).

    A row is positive iff ``0 <= label < num_classes``.  Returns ``(S_cls, S_box, S_ctr, T)``: three ``(L,)`` fp32
    tensors of unscaled per-level sums -- the focal term over all rows, ``ct * (1 - GIoU)`` and the centerness BCE
    over the positives, ``ct`` the centerness target -- differentiable with respect to all 3 L maps, and ``T``, the
    0-dim sum of ``ct`` over all positives, which depends on the targets only.  A level without a positive has
    ``S_box = S_ctr = 0`` exactly.  Two launches forward and one backward, whatever the sizes and the number of
    levels; nothing waits for the host.  This function never falls back: what the kernels do not do raises."""
    lists = [list(cls_scores), list(bbox_preds), list(centernesses)]
    levels = len(lists[0])
    if not 1 <= levels <= MAX_LEVELS or any(len(v) != levels for v in lists):
        raise ValueError(f'{[len(v) for v in lists]} maps: one of each kind per level, 1 to {MAX_LEVELS} levels')
    for name, t in [(n, m) for n, v in zip(('cls_scores', 'bbox_preds', 'centernesses'), lists) for m in v] + \
            [('anchors', anchors), ('labels', labels), ('label_weights', label_weights),
             ('bbox_targets', bbox_targets)]:
        require_gpu(t, name)
    cls, reg, ctr = lists
    num_classes = int(num_classes)
    reg_channels = 4 if reg_class_agnostic else 4 * num_classes
    batch = cls[0].shape[0]
    for l, (c, r, t) in enumerate(zip(cls, reg, ctr)):
        if any(m.dim() != 4 for m in (c, r, t)):
            raise ValueError('the head\'s maps are (B, channels, H, W)')
        if any(m.shape[0] != batch or m.shape[2:] != c.shape[2:] for m in (c, r, t)):
            raise ValueError(f'the maps of level {l} differ in batch or map size: ' +
                             ', '.join(str(tuple(m.shape)) for m in (c, r, t)))
        if num_classes < 1 or (c.shape[1], r.shape[1], t.shape[1]) != (num_classes, reg_channels, 1):
            raise ValueError(f'level {l}: {c.shape[1]} / {r.shape[1]} / {t.shape[1]} channels; one anchor per location '
                             f'with num_classes = {num_classes} and reg_class_agnostic = {bool(reg_class_agnostic)} '
                             f'needs {num_classes} / {reg_channels} / 1')
    if any(m.dtype != cls[0].dtype for m in cls + ctr) or cls[0].dtype not in DTYPES:
        raise TypeError('cls_scores and centernesses share one dtype, fp32 or bf16; got ' +
                        ', '.join(sorted({str(m.dtype) for m in cls + ctr})))
    if any(m.dtype != reg[0].dtype for m in reg) or reg[0].dtype not in DTYPES:
        raise TypeError('bbox_preds share one dtype, fp32 or bf16; got ' +
                        ', '.join(sorted({str(m.dtype) for m in reg})))
    rows = sum(c.shape[2] * c.shape[3] for c in cls)
    if anchors.dim() != 2 or tuple(anchors.shape) != (rows, 4):
        raise ValueError(f'anchors are (A, 4) with A = {rows}, the rows of the levels; got {tuple(anchors.shape)}')
    sizes = {'labels': batch * rows, 'label_weights': batch * rows, 'bbox_targets': batch * rows * 4}
    for name, t in (('labels', labels), ('label_weights', label_weights), ('bbox_targets', bbox_targets)):
        if t.numel() != sizes[name]:
            raise ValueError(f'{name} has {t.numel()} elements, {rows} anchors and a batch of {batch} need {sizes[name]}')
    desc = _desc(cls, reg, ctr, rows, num_classes, reg_class_agnostic, float(gamma), float(alpha), target_means,
                 target_stds)

    def f32(t):
        return t.detach().to(torch.float32).contiguous()
    targets = (f32(anchors), labels.detach().to(torch.int64).contiguous(), f32(label_weights), f32(bbox_targets))
    out = _AtssLossFn.apply(desc, targets, *_interleave(cls, reg, ctr))
    sums = out[:3 * levels].view(levels, 3)
    return sums[:, 0], sums[:, 1], sums[:, 2], out[3 * levels].detach()


class HipATSSLossMixin(object):
    """mmdet's ``ATSSHead.loss`` as ``LIGAATSSHead`` runs it, on the HIP path, for a head class
    ``class FastHead(HipATSSLossMixin, LIGAATSSHead)`` (``patch_reference()`` rebinds ``LIGAATSSHead.loss`` to this
    one).  Same signature, same result: a dict of three lists of L 0-dim tensors, ``loss_cls``, ``loss_bbox`` and
    ``loss_centerness``.  It builds the anchors and valid flags with the head's ``get_anchors``, the inside flags as
    ``HipATSSTargetMixin`` does, calls ``atss_target_2d`` and ``atss_loss_2d``, and forms on the device

        num_total_samples = max(reduce_mean(sum_images max(positives_i, 1)), 1)
        bbox_avg_factor   = max(reduce_mean(T), 1),   T = the sum of the centerness targets of all positives
        loss_cls[l]        = loss_cls.loss_weight        * S_cls[l] / num_total_samples
        loss_centerness[l] = loss_centerness.loss_weight * S_ctr[l] / num_total_samples
        loss_bbox[l]       = loss_bbox.loss_weight       * S_box[l] / bbox_avg_factor

    ``reduce_mean`` being an all-reduce of a device scalar divided by the world size when a process group is up.
    Nothing waits for the host: the reference's ``.item()`` of both factors, its ``nonzero()``, its NaN assert and the
    counts ``get_targets`` reads are not made.  It reads ``self.num_classes``, ``self.reg_class_agnostic``,
    ``self.bbox_coder`` (``means``, ``stds``), the loss modules ``self.loss_cls`` (``gamma``, ``alpha``),
    ``self.loss_bbox`` and ``self.loss_centerness`` (each ``loss_weight``) and what ``HipATSSTargetMixin`` reads.

    An image without any counting anchor contributes zero weights (``HipATSSTargetMixin``); the reference returns
    ``None`` for the whole batch there, after a host wait.

    What the kernels do not do -- ``reg_avg_factor`` other than 'default', ``num_extra_reg_channel > 0`` or a separate
    extra branch, a ``loss_cls`` that is not a sigmoid ``FocalLoss``, a ``loss_bbox`` that is not ``GIoULoss`` with
    ``reduction='mean'`` and ``eps=1e-6``, a ``loss_centerness`` that is not a sigmoid ``CrossEntropyLoss``, more than
    one anchor per location, more than 8 levels, and whatever ``HipATSSTargetMixin`` falls back for -- follows the
    package's fallback policy: 'warn' says so once and calls the reference ``loss`` (which finds the reference's own
    ``loss_single``), 'raise' makes it an ``MfmaPathError``; without a reference method to call it is an error either
    way."""

    def _atss_loss_unsupported(self, num_levels):
        if getattr(self, 'reg_avg_factor', 'default') != 'default':
            return f'reg_avg_factor={self.reg_avg_factor!r}'
        if getattr(self, 'num_reg_channel', 4) not in (4, None):
            return f'{self.num_reg_channel} regression channels (num_extra_reg_channel > 0)'
        if getattr(self, 'seperate_extra_reg_branch', False):
            return 'a separate extra regression branch'
        if not getattr(self, 'use_sigmoid_cls', True):
            return 'softmax classification (use_sigmoid_cls=False)'
        for name, want in (('loss_cls', 'FocalLoss'), ('loss_bbox', 'GIoULoss'), ('loss_centerness', 'CrossEntropyLoss')):
            module = getattr(self, name, None)
            if type(module).__name__ != want:
                return f'{name} = {type(module).__name__}, not {want}'
            if getattr(module, 'reduction', 'mean') != 'mean':
                return f'{name} with reduction={module.reduction!r}'
        if not getattr(self.loss_cls, 'use_sigmoid', True):
            return 'loss_cls = FocalLoss without use_sigmoid'
        if getattr(self.loss_bbox, 'eps', 1e-6) != 1e-6:
            return f'loss_bbox = GIoULoss with eps={self.loss_bbox.eps!r}'
        if not getattr(self.loss_centerness, 'use_sigmoid', False) or getattr(self.loss_centerness, 'use_mask', False):
            return 'loss_centerness = CrossEntropyLoss that is not the sigmoid one'
        if getattr(self.loss_centerness, 'class_weight', None) is not None:
            return 'loss_centerness = CrossEntropyLoss with class_weight'
        if getattr(self, 'num_anchors', 1) != 1:
            return f'{self.num_anchors} anchors per location'
        if num_levels > MAX_LEVELS:
            return f'{num_levels} levels (at most {MAX_LEVELS})'
        return None

    def loss(self, cls_scores, bbox_preds, centernesses, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore=None):
        args = (cls_scores, bbox_preds, centernesses, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore)
        why = self._atss_loss_unsupported(len(cls_scores))
        if why is None:
            featmap_sizes = [featmap.size()[-2:] for featmap in cls_scores]
            anchor_list, valid_flag_list = self.get_anchors(featmap_sizes, img_metas, device=cls_scores[0].device)
            why = HipATSSTargetMixin._atss_target_unsupported(self, anchor_list, gt_bboxes_ignore)
        if why is not None:
            return run_reference(self, 'loss', why, 'ATSS-loss', args, mixin=HipATSSLossMixin)
        anchors, _, _, dense, counts = head_dense_targets(self, anchor_list, valid_flag_list, gt_bboxes, img_metas,
                                                          gt_labels)
        labels, label_weights, bbox_targets, _ = dense
        coder = self.bbox_coder
        s_cls, s_box, s_ctr, total_ct = atss_loss_2d(
            cls_scores, bbox_preds, centernesses, anchors[:, :4], labels, label_weights, bbox_targets,
            num_classes=self.num_classes, reg_class_agnostic=getattr(self, 'reg_class_agnostic', True),
            gamma=self.loss_cls.gamma, alpha=self.loss_cls.alpha, target_means=getattr(coder, 'means', (0., 0., 0., 0.)),
            target_stds=getattr(coder, 'stds', (1., 1., 1., 1.)))
        num_total_pos = counts[:, 0].clamp(min=1).sum().to(torch.float32)     # mmdet: sum of max(pos_inds.numel(), 1)
        num_total_samples = dist_reduce_mean(num_total_pos).clamp(min=1.0)
        bbox_avg_factor = dist_reduce_mean(total_ct).clamp(min=1.0)
        return dict(loss_cls=list((s_cls * (float(self.loss_cls.loss_weight) / num_total_samples)).unbind(0)),
                    loss_bbox=list((s_box * (float(self.loss_bbox.loss_weight) / bbox_avg_factor)).unbind(0)),
                    loss_centerness=list(
                        (s_ctr * (float(self.loss_centerness.loss_weight) / num_total_samples)).unbind(0)))
