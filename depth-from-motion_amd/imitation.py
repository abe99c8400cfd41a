"""LiDAR-teacher feature-imitation loss of DfM on the HIP path.

Mirror of ``DfM.get_imitation_reg_layer_loss`` / ``_init_imitation_layers`` / ``construct_feature_pairs``
(mmdet3d/models/detectors/dfm.py:213-262, 384-401, 455-540) and of ``NormalizeLayer`` /
``WeightedL2WithSigmaLoss`` (detectors/imitation_utils.py).  The reference builds the in-box mask with
``mmcv.ops.points_in_boxes_part``, gathers three ``(Npos, C)`` copies and reduces them with a dozen torch
passes; here one launch (``dfm_imitation_loss_fwd``) tests the boxes first, reads only the in-box columns of
the two feature tensors where they lie, and returns the positives mask and a statistics block

    stats = [count, S, sum_c t (C), sum_c |t| (C)]   (fp64; S = sum 0.5 (pred - t')^2 over the positives)

from which the loss and the ``NormalizeLayer`` buffer update follow by scalar / length-C device ops
(``reduce_imitation_statistics``; pure torch, runs on CPU tensors under gloo as well).  The ``(Npos, C)``
gather exists nowhere.  The backward is one dense pass (``dfm_imitation_loss_bwd``).

The LiDAR teacher's two feature tensors are inputs, as they are to the reference function;
``integration.LidarTeacher`` (hard voxelization and the sparse encoder on the HIP path, forward only, eval only)
produces them from the point clouds.  The 1x1 ``conv_imitation`` layers are library GEMMs.
"""
import ctypes

import torch
import torch.distributed as dist
import torch.nn as nn

from . import _capi
from ._launch import DTYPES, STREAM, WS, launch, require_gpu

__all__ = ['NormalizeLayer', 'ImitationLoss', 'imitation_reg_layer_loss', 'imitation_statistics',
           'reduce_imitation_statistics']


def _dist_on():
    return dist.is_available() and dist.is_initialized()


def _all_reduce(t, group=None):
    """SUM over the ranks; nothing to do in a single process without a process group (the reference calls
    dist.all_reduce unconditionally and cannot run there)"""
    if _dist_on():
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    return t


class NormalizeLayer(nn.Module):
    """imitation_utils.py:10-94: running centre / scale of the teacher's features at the positives.
    Same four types, buffers, forward and ``update`` arithmetic; pure torch."""

    def __init__(self, type, channel, momentum=0.99):
        super().__init__()
        self.channel = channel
        self.type = type
        self.momentum = momentum
        if type not in ('scale', 'cw_scale', 'center+scale', 'cw_center+scale'):
            raise ValueError('invalid normalization type')
        self.channel_wise = type.startswith('cw_')
        self.do_centering = 'center' in type
        self.do_scaling = True
        self.scaling_method = 'abs'
        n = channel if self.channel_wise else 1
        if self.do_centering:
            self.register_buffer('center', torch.ones(1, n))
        self.register_buffer('scale', torch.ones(1, n))

    def forward(self, inputs):
        x = inputs - self.center if self.do_centering else inputs
        x = x / self.scale
        if self.training:
            self.update(inputs)
        return x

    @torch.no_grad()
    def update(self, x, group=None):
        """the reference's update on an (N, C) tensor"""
        assert len(x.shape) == 2
        bsize = _all_reduce(torch.tensor(x.shape[0], dtype=torch.long, device=x.device), group)
        if bsize <= 10:
            return
        if self.do_centering:
            sum_x = _all_reduce(torch.sum(x, dim=0, keepdim=True), group)
            new_center = sum_x / torch.clamp(bsize, min=1)
            if not self.channel_wise:
                new_center = new_center.mean(dim=-1, keepdim=True)
            self.center *= self.momentum
            self.center += new_center * (1 - self.momentum)
            x = x - new_center
        sum_x = _all_reduce(torch.sum(x.abs(), dim=0, keepdim=True), group)
        new_scale = sum_x / torch.clamp(bsize, min=1)
        if not self.channel_wise:
            new_scale = new_scale.mean(dim=-1, keepdim=True)
        self.scale *= self.momentum
        self.scale += new_scale * (1 - self.momentum)

    @torch.no_grad()
    def _blend(self, name, new, ok):
        """buffer <- momentum * buffer + (1 - momentum) * new where ``ok`` (a device bool: the global count
        is above 10), untouched otherwise -- the reference's early return without a host sync"""
        buf = getattr(self, name)
        new = new.to(buf.dtype).view(1, -1)
        if not self.channel_wise:
            new = new.mean(dim=-1, keepdim=True)
        buf.copy_(torch.where(ok, buf * self.momentum + new * (1 - self.momentum), buf))
        return new


@torch.no_grad()
def reduce_imitation_statistics(stats, channels, batch_size, loss_weight=1.0, norm_layer=None,
                                normalizer_clamp_value=10, training=True, group=None, centered_abs_sum=None):
    """From one rank's statistics block to the loss scale and the buffer update.

    ``stats``: fp64 ``[count, S, sum t (C), sum |t| (C)]`` of this rank's positives (any device).
    Returns ``(loss_scale, normalizer)``: the loss is ``S * loss_scale`` with
    ``loss_scale = loss_weight / (C * B * normalizer)``, ``normalizer = clamp(mean over ranks of count,
    min=normalizer_clamp_value)`` (``dist_reduce_mean``, models/utils/common_utils.py:5-12).

    With ``training`` and a ``NormalizeLayer`` in training mode its buffers are updated as
    ``NormalizeLayer.update`` would from the gathered ``(Npos, C)`` targets, the "global count <= 10: leave
    them" rule included (as a device-side select).  ``centered_abs_sum(new_center (C,) fp32)`` must return
    this rank's fp64 ``sum |t - new_center|`` per channel; only the two centering types call it.

    Collectives (every rank issues them, with or without positives; none without a process group): one
    fp64 SUM carrying the count and the per-channel sums -- integers below 2^53 stay exact --, and a second
    one for the centering types only.
    """
    C = int(channels)
    stats = stats.to(torch.float64)
    update = bool(training) and isinstance(norm_layer, NormalizeLayer) and norm_layer.training
    world = dist.get_world_size(group) if _dist_on() else 1
    if update:
        first = stats[2:2 + C] if norm_layer.do_centering else stats[2 + C:2 + 2 * C]
        payload = torch.cat([stats[0:1], first])
    else:
        payload = stats[0:1].clone()
    _all_reduce(payload, group)
    count = payload[0]
    normalizer = torch.clamp((count / world).float(), min=normalizer_clamp_value)
    loss_scale = float(loss_weight) / (C * int(batch_size) * normalizer)
    if update:
        ok = count > 10
        bsize = torch.clamp(count, min=1)
        if norm_layer.do_centering:
            new_center = norm_layer._blend('center', payload[1:] / bsize, ok)
            # scale is measured on x - new_center
            second = centered_abs_sum(new_center.expand(1, C).reshape(C).float().contiguous()).to(torch.float64)
            abs_sum = _all_reduce(second.clone(), group)
        else:
            abs_sum = payload[1:]
        norm_layer._blend('scale', abs_sum / bsize, ok)
    return loss_scale, normalizer


def _layout(x):
    """(tensor as the kernel reads it, channels_last flag): NC[D]HW and N[D]HWC are read in place"""
    if x.is_contiguous():
        return x, 0
    fmt = torch.channels_last if x.dim() == 4 else torch.channels_last_3d
    if x.is_contiguous(memory_format=fmt):
        return x, 1
    return x.contiguous(), 0


def _vec(layer, name, device):
    """a NormalizeLayer buffer as the kernel takes it: fp32, length 1 or C (None: the layer has none); a copy,
    because the backward needs the value the forward used and the update that follows writes in place"""
    v = getattr(layer, name, None) if isinstance(layer, NormalizeLayer) else None
    if v is None:
        return None
    return v.detach().to(device=device, dtype=torch.float32).reshape(-1).clone()


def _desc(pred, target, p_cl, t_cl, points, boxes, mode, center, scale):
    d = _capi.ImitationDesc()
    d.batch, d.channels = pred.shape[0], pred.shape[1]
    d.nz = pred.shape[2] if pred.dim() == 5 else 1
    d.ny, d.nx = pred.shape[-2], pred.shape[-1]
    d.num_boxes = 0 if boxes is None else boxes.shape[1]
    d.points_batch = 1 if points is None else points.shape[0]
    d.mode = mode
    d.pred_dtype, d.target_dtype = DTYPES[pred.dtype], DTYPES[target.dtype]
    d.pred_channels_last, d.target_channels_last = p_cl, t_cl
    d.center_len = 0 if center is None else center.numel()
    d.scale_len = 0 if scale is None else scale.numel()
    return d


def _launch_fwd(desc, pred, target, points, boxes, center, scale, new_center, mask, stats):
    lib = _capi.lib()
    nbytes = lib.dfm_imitation_loss_workspace_bytes(ctypes.byref(desc))
    if nbytes == 0:
        _capi.check(-1)
    launch('dfm_imitation_loss_fwd', desc, pred, target, points, boxes, center, scale, new_center, mask, stats, WS,
           STREAM, ws_bytes=nbytes)


class _ImitationFn(torch.autograd.Function):
    """owns the two launches: S, the positives mask and the statistics block forward; the dense
    d S / d pred backward.  ``target`` gets no gradient (the teacher is frozen)."""

    @staticmethod
    def forward(ctx, pred, target, points, boxes, center, scale, desc):
        device = pred.device
        mshape = (pred.shape[0],) + tuple(pred.shape[2:])
        mask = torch.empty(mshape, dtype=torch.uint8, device=device)
        stats = torch.empty(2 + 2 * pred.shape[1], dtype=torch.float64, device=device)
        _launch_fwd(desc, pred, target, points, boxes, center, scale, None, mask, stats)
        ctx.save_for_backward(pred, target, mask, center, scale)
        ctx.desc = desc
        ctx.mark_non_differentiable(mask, stats)
        return stats[1].float(), mask, stats

    @staticmethod
    def backward(ctx, g_S, _g_mask, _g_stats):
        pred, target, mask, center, scale = ctx.saved_tensors
        coef = g_S.detach().to(torch.float32).reshape(1).contiguous()
        grad = torch.empty_like(pred)  # pred's own layout and dtype
        launch('dfm_imitation_loss_bwd', ctx.desc, pred, target, mask, center, scale, coef, grad, STREAM)
        return grad, None, None, None, None, None, None


def _pad_boxes(gt_boxes, device):
    """(B, T, 7) fp32 from a tensor or a ragged list of (T_b, >=7) tensors / box objects with ``.tensor``;
    the padding rows are zero-size boxes, which contain nothing"""
    if torch.is_tensor(gt_boxes):
        return gt_boxes[..., :7].to(device=device, dtype=torch.float32).contiguous()
    rows = [getattr(b, 'tensor', b)[..., :7].to(device=device, dtype=torch.float32) for b in gt_boxes]
    T = max([r.shape[0] for r in rows] + [0])
    out = torch.zeros((len(rows), T, 7), dtype=torch.float32, device=device)
    for i, r in enumerate(rows):
        out[i, :r.shape[0]] = r
    return out


def _prepare(features_preds, features_targets, mode, gt_boxes, points, norm_layer):
    require_gpu(features_preds, 'features_preds')
    require_gpu(features_targets, 'features_targets')
    if features_preds.dtype not in DTYPES or features_targets.dtype not in DTYPES:
        raise TypeError('features must be float32 or bfloat16')
    if features_preds.shape != features_targets.shape or features_preds.dim() not in (4, 5):
        raise ValueError(f'features must share one (B, C, [Nz,] Ny, Nx) shape, got {tuple(features_preds.shape)} '
                         f'and {tuple(features_targets.shape)}')
    device = features_preds.device
    pred, p_cl = _layout(features_preds)
    target, t_cl = _layout(features_targets.detach())
    if mode == 'inbox':
        boxes = _pad_boxes(gt_boxes, device)
        pts = points.detach().to(device=device, dtype=torch.float32)
        if pts.dim() == 3:
            pts = pts[None]
        pts = pts[..., :3].contiguous()
        if boxes.shape[0] != pred.shape[0] or tuple(pts.shape[1:3]) != tuple(pred.shape[-2:]):
            raise ValueError(f'gt_boxes {tuple(boxes.shape)} / points {tuple(pts.shape)} do not fit features '
                             f'{tuple(pred.shape)}')
        if boxes.shape[1] == 0:
            boxes = None
        kind = _capi.IMI_INBOX
    elif mode == 'full':
        boxes = pts = None
        kind = _capi.IMI_FULL
    else:
        raise ValueError('wrong imitation mode')
    center, scale = _vec(norm_layer, 'center', device), _vec(norm_layer, 'scale', device)
    return pred, target, pts, boxes, center, scale, _desc(pred, target, p_cl, t_cl, pts, boxes, kind, center, scale)


def imitation_statistics(features_preds, features_targets, mode, gt_boxes, points, norm_layer=None):
    """One forward launch: ``(S, mask, stats)`` -- S differentiable w.r.t. ``features_preds``, mask uint8
    ``(B, [Nz,] Ny, Nx)``, stats the fp64 block ``[count, S, sum t (C), sum |t| (C)]``."""
    pred, target, pts, boxes, center, scale, desc = _prepare(features_preds, features_targets, mode, gt_boxes,
                                                             points, norm_layer)
    return _ImitationFn.apply(pred, target, pts, boxes, center, scale, desc)


def imitation_reg_layer_loss(features_preds, features_targets, imitation_cfg, gt_boxes, points, norm_layer=None,
                             normalizer_clamp_value=10, training=True, group=None):
    """``DfM.get_imitation_reg_layer_loss`` (dfm.py:468-540): returns ``(loss, info)``.

    features_preds / features_targets: ``(B, C, [Nz,] Ny, Nx)``, each fp32 or bf16, each NC[D]HW or
    channels-last, read in place.  ``gt_boxes``: ``(B, T, 7)`` or a list of ``(T_b, 7)`` (x, y, z, sizes,
    yaw); ``points``: ``([1 or B,] Ny, Nx, 3)``, the reference's ``bbox_head_3d.anchors[0][:, :, :, 0, 0, :3]``.
    ``imitation_cfg`` supplies ``mode`` ('inbox' | 'full'; the reference's 'full' branch cannot run -- it ANDs a
    float tensor with a bool one -- and means "every cell" here) and ``loss_weight``.
    ``norm_layer``: the pair's ``NormalizeLayer`` (or ``nn.Identity`` / None); in ``training`` mode its buffers
    are updated from the kernel's statistics.

    ``info``: ``positives`` (bool mask), ``num_positives`` (device scalar, this rank), ``normalizer``,
    ``stats``.  The reference's logging-only ``rel_err`` median and its ``.item()`` calls (three host syncs a
    step) are deliberately left out: nothing here waits for the device.
    """
    if not isinstance(norm_layer, NormalizeLayer):
        norm_layer = None
    pred, target, pts, boxes, center, scale, desc = _prepare(features_preds, features_targets,
                                                             imitation_cfg['mode'], gt_boxes, points, norm_layer)
    S, mask, stats = _ImitationFn.apply(pred, target, pts, boxes, center, scale, desc)
    C = pred.shape[1]

    def centered_abs_sum(new_center):
        out = torch.empty(C, dtype=torch.float64, device=pred.device)
        _launch_fwd(desc, None, target, pts, boxes, center, scale, new_center, None, out)
        return out

    loss_scale, normalizer = reduce_imitation_statistics(
        stats, C, pred.shape[0], imitation_cfg.get('loss_weight', 1.0), norm_layer, normalizer_clamp_value,
        training, group, centered_abs_sum)
    loss = S * loss_scale
    return loss, dict(positives=mask.bool(), num_positives=stats[0], normalizer=normalizer, stats=stats)


class ImitationLoss(nn.Module):
    """``conv_imitation`` / ``norm_imitation`` of the DfM detector with the state-dict keys and constructor
    rules of ``_init_imitation_layers`` (dfm.py:213-262), so a detector checkpoint's entries load into it,
    and ``construct_feature_pairs`` + ``imitation_loss`` as ``forward``.

    A single cfg gives a bare ``conv_imitation`` module, several a ``ModuleList``; ``use_relu`` wraps the
    layer in a ``Sequential`` with a ReLU (and requires ``normalize=None``); ``normalize=None`` gives an
    ``nn.Identity``; ``layer`` is 'conv2d' | 'conv3d' | 'none' ('none' without ReLU is an ``nn.Identity`` --
    the reference raises an IndexError there).
    """

    def __init__(self, imitation_cfgs, normalizer_clamp_value=10):
        super().__init__()
        cfgs = imitation_cfgs if isinstance(imitation_cfgs, (list, tuple)) else [imitation_cfgs]
        self.imitation_cfgs = [dict(c) for c in cfgs]
        self.normalizer_clamp_value = normalizer_clamp_value
        convs = []
        self.norm_imitation = nn.ModuleDict()
        for cfg in self.imitation_cfgs:
            layers = []
            if cfg['layer'] in ('conv2d', 'conv3d'):
                conv = nn.Conv2d if cfg['layer'] == 'conv2d' else nn.Conv3d
                layers.append(conv(cfg['channel'], cfg['channel'], kernel_size=cfg['kernel_size'],
                                   padding=cfg['kernel_size'] // 2, stride=1, groups=1))
            elif cfg['layer'] != 'none':
                raise ValueError(f"invalid layer type {cfg['layer']}")
            if cfg.get('use_relu', False):
                layers.append(nn.ReLU())
                assert cfg.get('normalize') is None
            name = cfg['stereo_feature_layer']
            self.norm_imitation[name] = nn.Identity() if cfg.get('normalize') is None else \
                NormalizeLayer(cfg['normalize'], cfg['channel'])
            convs.append(nn.Identity() if not layers else layers[0] if len(layers) == 1 else nn.Sequential(*layers))
        self.conv_imitation = nn.ModuleList(convs) if len(convs) > 1 else convs[0]

    def forward(self, stereo_features, lidar_features, gt_boxes, points, group=None):
        """stereo_features / lidar_features: dicts keyed by the cfgs' ``stereo_feature_layer`` /
        ``lidar_feature_layer``; returns the list of losses in cfg order"""
        convs = [self.conv_imitation] if len(self.imitation_cfgs) == 1 else self.conv_imitation
        losses = []
        for cfg, conv in zip(self.imitation_cfgs, convs):
            x = stereo_features[cfg['stereo_feature_layer']]
            w = next(conv.parameters(), None)
            if w is not None and x.dtype != w.dtype:
                x = x.to(w.dtype)
            loss, _ = imitation_reg_layer_loss(
                conv(x), lidar_features[cfg['lidar_feature_layer']], cfg, gt_boxes, points,
                norm_layer=self.norm_imitation[cfg['stereo_feature_layer']],
                normalizer_clamp_value=self.normalizer_clamp_value, training=self.training, group=group)
            losses.append(loss)
        return losses
