"""The 3-D anchor head's ``loss_single`` on the HIP path.

Mirror of ``Anchor3DHead.loss_single`` (mmdet3d/models/dense_heads/anchor3d_head.py:199-301) and of
``LIGAAnchor3DHead.loss_single`` (liga_anchor3d_head.py:130-226).  mmdet is not a dependency: the semantics are those
stated in include/dfm_hip_anchor_loss.h (a part of include/dfm_hip.h).

The reference permutes and copies the three maps, runs a Python focal loss over every class logit, waits for the host
twice (``labels.max().item()`` and ``nonzero()``), gathers the positive rows four times and reduces three times;
autograd walks all of it back.  ``anchor3d_loss`` is one ``autograd.Function``: two launches forward
(``dfm_anchor3d_loss_fwd``: the four term sums per workgroup, then their fixed-order sum times the scales) and one
backward (``dfm_anchor3d_loss_bwd``: every element of the three map gradients written once).  The maps are read in
place (NCHW, channels-last, any strides; fp32 or bf16), the targets are the dense tensors ``anchor_target_3d`` returns,
the average factors stay on the device inside ``scale``; nothing is copied to the host and nothing waits for it.
``HipAnchor3DLossMixin.loss_single`` has the reference method's signature and serves both head classes.

The reference's ``assert labels.max().item() <= num_classes`` is a wait for the host and is not made: a label outside
``[0, num_classes)`` -- ``num_classes`` itself, ``-1``, anything else -- is a row whose classes are all negative.
CPU tensors are refused: there is no CPU path.
"""

import torch

from . import _capi
from .fallback import run_reference
from ._launch import DTYPES, STREAM, WS, launch, require_gpu, upload

__all__ = ['anchor3d_loss', 'HipAnchor3DLossMixin', 'counters']

_COUNTERS = {'kernel_launches': 0, 'memsets': 0, 'host_waits': 0}


def counters(reset=False):
    """kernel launches and memsets made by this module's C calls so far, and the times it waited for the host (none:
    the key is there so that a reader sees it is counted); ``reset=True`` zeroes them after reading.  A forward is
    two launches, a backward one, whatever the sizes and the number of positives."""
    out = dict(_COUNTERS)
    if reset:
        for k in _COUNTERS:
            _COUNTERS[k] = 0
    return out


def _desc(cls_score, bbox_pred, dir_cls_preds, num_classes, code, gamma, alpha, beta, code_weight, diff_rad_by_sin,
          with_iou):
    batch, _, h, w = cls_score.shape
    d = _capi.AnchorLossDesc(batch=batch, h=h, w=w, anchors_per_location=cls_score.shape[1] // num_classes,
                             num_classes=num_classes, box_code_size=code, dtype=DTYPES[cls_score.dtype],
                             has_dir=dir_cls_preds is not None, with_iou=bool(with_iou),
                             diff_rad_by_sin=bool(diff_rad_by_sin), gamma=gamma, alpha=alpha, beta=beta)
    d.code_weight[:] = [1.0] * _capi.ANCHOR_LOSS_MAX_CODE
    if code_weight is not None:
        d.code_weight[:code] = [float(v) for v in code_weight]
    d.cls_stride[:] = cls_score.stride()
    d.reg_stride[:] = bbox_pred.stride()
    if dir_cls_preds is not None:
        d.dir_stride[:] = dir_cls_preds.stride()
    return d


class _Anchor3DLossFn(torch.autograd.Function):
    """out (4,) = scale * (S_cls, S_box, S_dir, S_iou); the backward is one launch over the saved inputs"""

    @staticmethod
    def forward(ctx, cls_score, bbox_pred, dir_cls_preds, targets, scale, desc):
        labels, label_weights, bbox_targets, bbox_weights, dir_targets, dir_weights, anchors = targets
        out = torch.empty(4, dtype=torch.float32, device=cls_score.device)
        launch('dfm_anchor3d_loss_fwd', desc, cls_score, bbox_pred, dir_cls_preds, labels, label_weights,
               bbox_targets, bbox_weights, dir_targets, dir_weights, anchors, scale, out, WS, STREAM,
               ws_bytes=_capi.lib().dfm_anchor3d_loss_workspace_bytes(desc))
        if cls_score.numel():
            _COUNTERS['kernel_launches'] += 2
        else:
            _COUNTERS['memsets'] += 1
        ctx.save_for_backward(cls_score, bbox_pred, dir_cls_preds, *targets, scale)
        ctx.desc = desc
        return out

    @staticmethod
    def backward(ctx, grad_out):
        cls_score, bbox_pred, dir_cls_preds, *targets, scale = ctx.saved_tensors
        desc = ctx.desc
        g = grad_out.detach().to(torch.float32).contiguous()
        grads = [torch.empty_like(m) if need and m is not None else None
                 for m, need in zip((cls_score, bbox_pred, dir_cls_preds), ctx.needs_input_grad[:3])]
        for field, t in zip((desc.grad_cls_stride, desc.grad_reg_stride, desc.grad_dir_stride), grads):
            if t is not None:
                field[:] = t.stride()
        if cls_score.numel() and any(t is not None for t in grads):
            launch('dfm_anchor3d_loss_bwd', desc, cls_score, bbox_pred, dir_cls_preds, *targets, scale, g, *grads,
                   STREAM)
            _COUNTERS['kernel_launches'] += 1
        return (*grads, None, None, None)


def anchor3d_loss(cls_score, bbox_pred, dir_cls_preds, labels, label_weights, bbox_targets, bbox_weights, dir_targets,
                  dir_weights, anchors=None, *, num_classes, scale, gamma=2.0, alpha=0.25, beta=1.0 / 9.0,
                  code_weight=None, diff_rad_by_sin=True, with_iou=False):
    """The four terms of ``loss_single`` of one level, for the whole batch.

    ``cls_score`` / ``bbox_pred`` / ``dir_cls_preds``: the ``(B, A*C, H, W)`` / ``(B, A*S, H, W)`` / ``(B, A*2, H, W)``
    maps as the head returns them, fp32 or bf16 (one dtype), read in place whatever their strides;
    ``dir_cls_preds=None``: a head without a direction classifier.  ``labels`` ``(B, N)`` int64, ``label_weights``
    ``(B, N)``, ``bbox_targets`` and ``bbox_weights`` ``(B, N, S)``, ``dir_targets`` ``(B, N)`` int64, ``dir_weights``
    ``(B, N)``: what ``anchor_target_3d`` returns for the level, ``N = H*W*A`` (any shape with those elements in that
    order; floating targets are converted to contiguous fp32).  ``anchors`` ``(N, S)``: needed with ``with_iou``
    only (``S == 7``).  ``scale``: a device tensor of four fp32 values ``loss_weight_i / avg_factor_i`` (class, box,
    direction, IoU; those of absent terms are not read).

    A row is positive iff ``0 <= label < num_classes``; any other label is a row whose classes are all negative (the
    reference's ``assert labels.max().item() <= num_classes`` would wait for the host and is not made).

    Returns ``(loss_cls, loss_bbox, loss_dir, loss_iou)``, 0-dim fp32 tensors, differentiable with respect to the
    three maps; the terms of an absent direction classifier or IoU term are exactly 0, as are ``loss_bbox``,
    ``loss_dir`` and ``loss_iou`` without a positive row.  Two launches forward and one backward, whatever the
    sizes; nothing waits for the host.  This function never falls back: what the kernels do not do raises."""
    maps = [('cls_score', cls_score), ('bbox_pred', bbox_pred)] + \
        ([('dir_cls_preds', dir_cls_preds)] if dir_cls_preds is not None else [])
    dense = [('labels', labels), ('label_weights', label_weights), ('bbox_targets', bbox_targets),
             ('bbox_weights', bbox_weights)]
    if dir_cls_preds is not None:
        dense += [('dir_targets', dir_targets), ('dir_weights', dir_weights)]
    if with_iou:
        if anchors is None:
            raise ValueError('with_iou needs the anchors')
        dense.append(('anchors', anchors))
    for name, t in maps + dense + [('scale', scale)]:
        require_gpu(t, name)
    if any(m.dim() != 4 for _, m in maps):
        raise ValueError('the head\'s maps are (B, channels, H, W)')
    if any(m.shape[0] != cls_score.shape[0] or m.shape[2:] != cls_score.shape[2:] for _, m in maps):
        raise ValueError('the maps of a level differ in batch or map size: ' +
                         ', '.join(str(tuple(m.shape)) for _, m in maps))
    if any(m.dtype != cls_score.dtype for _, m in maps) or cls_score.dtype not in DTYPES:
        raise TypeError('the maps share one dtype, fp32 or bf16; got ' + ', '.join(str(m.dtype) for _, m in maps))
    num_classes = int(num_classes)
    batch, channels, h, w = cls_score.shape
    if num_classes < 1 or channels % num_classes:
        raise ValueError(f'{channels} class channels are no multiple of num_classes = {num_classes}')
    per_loc = channels // num_classes
    if per_loc < 1 or bbox_pred.shape[1] % per_loc:
        raise ValueError(f'{per_loc} anchors per location do not divide the {bbox_pred.shape[1]} channels of bbox_pred')
    code = bbox_pred.shape[1] // per_loc
    if dir_cls_preds is not None and dir_cls_preds.shape[1] != per_loc * 2:
        raise ValueError(f'{per_loc} anchors per location: dir_cls_preds needs {per_loc * 2} channels, got '
                         f'{dir_cls_preds.shape[1]}')
    n = h * w * per_loc
    rows = batch * n
    sizes = {'labels': rows, 'label_weights': rows, 'bbox_targets': rows * code, 'bbox_weights': rows * code,
             'dir_targets': rows, 'dir_weights': rows, 'anchors': n * code}
    for name, t in dense:
        if t.numel() != sizes[name]:
            raise ValueError(f'{name} has {t.numel()} elements, a {h} x {w} map with {per_loc} anchors per location '
                             f'and a batch of {batch} needs {sizes[name]}')
    if scale.numel() != 4:
        raise ValueError('scale holds four values: class, box, direction, IoU')
    if code_weight is not None and len(code_weight) != code:
        raise ValueError(f'code_weight has {len(code_weight)} entries, the box code {code}')
    desc = _desc(cls_score, bbox_pred, dir_cls_preds, num_classes, code, float(gamma), float(alpha), float(beta),
                 code_weight, diff_rad_by_sin, with_iou)

    def f32(t):
        return t.detach().to(torch.float32).contiguous()

    def i64(t):
        return t.detach().to(torch.int64).contiguous()
    targets = (i64(labels), f32(label_weights), f32(bbox_targets), f32(bbox_weights),
               i64(dir_targets) if dir_cls_preds is not None else None,
               f32(dir_weights) if dir_cls_preds is not None else None, f32(anchors) if with_iou else None)
    out = _Anchor3DLossFn.apply(cls_score, bbox_pred, dir_cls_preds, targets, f32(scale), desc)
    return tuple(out.unbind(0))


def dist_reduce_mean(tensor):
    """``dist_reduce_mean`` of the reference (models/utils/common_utils.py): the mean over the ranks of a device
    scalar, an all-reduce when a process group is up, the tensor itself otherwise; nothing comes to the host"""
    dist = torch.distributed
    if not (dist.is_available() and dist.is_initialized()):
        return tensor
    tensor = tensor.clone()
    dist.all_reduce(tensor.div_(dist.get_world_size()), op=dist.ReduceOp.SUM)
    return tensor


def _on(host, device):
    """a small host tensor on ``device`` without a wait (a CPU ``device``: the tensor itself, for the host-side tests)"""
    return host if torch.device(device).type == 'cpu' else upload(host, device)


class HipAnchor3DLossMixin(object):
    """``Anchor3DHead.loss_single`` and ``LIGAAnchor3DHead.loss_single`` on the HIP path, for a head class
    ``class FastHead(HipAnchor3DLossMixin, LIGAAnchor3DHead)`` (``patch_reference()`` rebinds both reference classes'
    method to this one).  It reads ``self.num_classes``, ``self.box_code_size``, ``self.use_sigmoid_cls``,
    ``self.use_direction_classifier``, ``self.diff_rad_by_sin``, ``self.train_cfg['code_weight']`` and the loss modules
    ``self.loss_cls`` (``gamma``, ``alpha``), ``self.loss_bbox`` (``beta``), ``self.loss_dir``, ``self.loss_iou`` (each
    ``loss_weight`` and ``reduction``) by attribute, and returns the reference's tuple ``(loss_cls, loss_bbox,
    loss_dir[, loss_iou])``, ``loss_dir`` being ``None`` without a direction classifier.

    Average factors.  A head with ``normalizer_clamp_value`` (LIGAAnchor3DHead) divides the class term by
    ``avg + clamp`` and the others by ``max(avg, clamp)``, ``avg`` being ``num_total_samples`` or, with
    ``reduce_avg_factor``, its mean over the ranks (an all-reduce of a device scalar when a process group is up).
    Any other head divides every term by ``num_total_samples``; ``None`` means the batch size.

    What the kernels do not do -- softmax classification, a ``loss_cls`` that is not a sigmoid ``FocalLoss``, a
    ``loss_bbox`` that is not ``SmoothL1Loss``, a ``loss_dir`` that is not a softmax ``CrossEntropyLoss`` without
    ``class_weight``, a ``loss_iou`` that is neither ``None`` nor ``IOU3DLoss``, a ``reduction`` other than 'mean', a
    box code wider than 16 or, with ``loss_iou``, other than 7 -- follows the package's fallback policy: 'warn' says
    so once and calls the reference method, 'raise' makes it an ``MfmaPathError``; without a reference method to
    call it is an error either way."""

    def _loss_single_unsupported(self):
        if not getattr(self, 'use_sigmoid_cls', True):
            return 'softmax classification (use_sigmoid_cls=False)'
        losses = [('loss_cls', self.loss_cls, 'FocalLoss'), ('loss_bbox', self.loss_bbox, 'SmoothL1Loss')]
        if getattr(self, 'use_direction_classifier', True):
            losses.append(('loss_dir', self.loss_dir, 'CrossEntropyLoss'))
        if getattr(self, 'loss_iou', None) is not None:
            losses.append(('loss_iou', self.loss_iou, 'IOU3DLoss'))
        for name, module, want in losses:
            if type(module).__name__ != want:
                return f'{name} = {type(module).__name__}, not {want}'
            if getattr(module, 'reduction', 'mean') != 'mean':
                return f'{name} with reduction={module.reduction!r}'
        if not getattr(self.loss_cls, 'use_sigmoid', True):
            return 'loss_cls = FocalLoss without use_sigmoid'
        if getattr(self, 'use_direction_classifier', True):
            if getattr(self.loss_dir, 'use_sigmoid', False) or getattr(self.loss_dir, 'use_mask', False):
                return 'loss_dir = CrossEntropyLoss that is not the softmax one'
            if getattr(self.loss_dir, 'class_weight', None) is not None:
                return 'loss_dir = CrossEntropyLoss with class_weight'
        if self.box_code_size > _capi.BBOX_CODE_MAX:
            return f'a box code of {self.box_code_size} columns (at most {_capi.BBOX_CODE_MAX})'
        if getattr(self, 'loss_iou', None) is not None and self.box_code_size != 7:
            return f'loss_iou on a box code of {self.box_code_size} columns (7)'
        return None

    def _loss_single_scale(self, num_total_samples, batch, device):
        """the device tensor of ``loss_weight_i / avg_factor_i``"""
        with_dir = getattr(self, 'use_direction_classifier', True)
        iou = getattr(self, 'loss_iou', None)
        weights = [float(self.loss_cls.loss_weight), float(self.loss_bbox.loss_weight),
                   float(self.loss_dir.loss_weight) if with_dir else 0.0,
                   float(iou.loss_weight) if iou is not None else 0.0]
        if num_total_samples is None:
            num_total_samples = int(batch)
        clamp = getattr(self, 'normalizer_clamp_value', None)
        on_device = isinstance(num_total_samples, torch.Tensor) and num_total_samples.is_cuda
        if clamp is not None and getattr(self, 'reduce_avg_factor', False) and \
                torch.distributed.is_available() and torch.distributed.is_initialized():
            on_device = True
        if not on_device:                                     # host arithmetic in double, one small upload
            avg = float(num_total_samples)
            factors = [avg] * 4 if clamp is None else [avg + clamp] + [max(avg, float(clamp))] * 3
            host = torch.tensor([wt / f if wt else 0.0 for wt, f in zip(weights, factors)], dtype=torch.float32)
            return _on(host, device)
        if isinstance(num_total_samples, torch.Tensor):
            avg = num_total_samples.detach().to(device=device, dtype=torch.float32).reshape(())
        else:
            avg = _on(torch.tensor(float(num_total_samples), dtype=torch.float32), device)
        if clamp is None:
            factors = avg.expand(4)
        else:
            if getattr(self, 'reduce_avg_factor', False):
                avg = dist_reduce_mean(avg)
            factors = torch.stack([avg + clamp] + [torch.clamp(avg, min=clamp)] * 3)
        return _on(torch.tensor(weights, dtype=torch.float32), device) / factors

    def loss_single(self, cls_score, bbox_pred, dir_cls_preds, labels, label_weights, bbox_targets, bbox_weights,
                    dir_targets, dir_weights, anchors, num_total_samples):
        args = (cls_score, bbox_pred, dir_cls_preds, labels, label_weights, bbox_targets, bbox_weights, dir_targets,
                dir_weights, anchors, num_total_samples)
        why = self._loss_single_unsupported()
        if why is not None:
            return run_reference(self, 'loss_single', why, 'anchor-loss', args, mixin=HipAnchor3DLossMixin)
        with_dir = getattr(self, 'use_direction_classifier', True)
        with_iou = getattr(self, 'loss_iou', None) is not None
        train_cfg = getattr(self, 'train_cfg', None)
        code_weight = (train_cfg.get('code_weight', None) if hasattr(train_cfg, 'get') else
                       getattr(train_cfg, 'code_weight', None)) or None
        code = self.box_code_size
        if with_iou:                                           # (B, N, S) or (B * N, S), one set per image: the first
            anchors = anchors.reshape(-1, code)[:anchors.numel() // code // max(int(cls_score.shape[0]), 1)]
        scale = self._loss_single_scale(num_total_samples, cls_score.shape[0], cls_score.device)
        out = anchor3d_loss(cls_score, bbox_pred, dir_cls_preds if with_dir else None, labels, label_weights,
                            bbox_targets, bbox_weights, dir_targets, dir_weights, anchors if with_iou else None,
                            num_classes=self.num_classes, scale=scale, gamma=self.loss_cls.gamma,
                            alpha=self.loss_cls.alpha, beta=self.loss_bbox.beta, code_weight=code_weight,
                            diff_rad_by_sin=self.diff_rad_by_sin, with_iou=with_iou)
        losses = (out[0], out[1], out[2] if with_dir else None)
        return losses + (out[3],) if with_iou else losses
