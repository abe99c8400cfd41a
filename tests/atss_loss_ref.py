"""The 2-D ATSS head's loss as torch expressions, written from the formulas of include/dfm_hip_atss_loss.h: the
reference of tests/test_atss_loss*.py (run in fp64) and the baseline of tools/atss_loss_timing.py (run in fp32 on the
device: what a user of the package has without the fused kernels).

``level_terms`` is one level the way the head writes it -- permuted copies of the maps, a ``cat`` + ``gather`` for the
class-specific deltas, a focal loss of a dozen element-wise passes, ``nonzero``, indexed gathers, three box decodes,
the ``torch.any`` of GIoULoss -- differentiated by autograd; ``loss_terms`` runs it once per level over slices of the
dense targets, and ``loss_dict`` is the arithmetic of ``ATSSHead.loss`` around the levels, ``.item()`` included when
``host_factors`` is set (the baseline's two waits).
"""
import math

import torch

from tests.anchor_loss_ref import focal, rows_of

MAX_RATIO = abs(math.log(16 / 1000))
EPS = 1e-6


def delta2bbox(anchors, deltas, means, stds):
    """DeltaXYWHBBoxCoder.decode of (P, 4) rows without max_shape: dw and dh clamped to +-|log(16 / 1000)|"""
    e = deltas * deltas.new_tensor(list(stds)) + deltas.new_tensor(list(means))
    ew, eh = e[:, 2].clamp(-MAX_RATIO, MAX_RATIO), e[:, 3].clamp(-MAX_RATIO, MAX_RATIO)
    px, py = (anchors[:, 0] + anchors[:, 2]) * 0.5, (anchors[:, 1] + anchors[:, 3]) * 0.5
    pw, ph = anchors[:, 2] - anchors[:, 0], anchors[:, 3] - anchors[:, 1]
    gx, gy, gw, gh = px + pw * e[:, 0], py + ph * e[:, 1], pw * ew.exp(), ph * eh.exp()
    return torch.stack([gx - gw * 0.5, gy - gh * 0.5, gx + gw * 0.5, gy + gh * 0.5], 1)


def centerness_target(anchors, gt):
    """sqrt of the product of the two side ratios of the anchor centre inside ``gt``; 0 where the product is not > 0"""
    cx, cy = (anchors[:, 0] + anchors[:, 2]) * 0.5, (anchors[:, 1] + anchors[:, 3]) * 0.5
    l, t, r, b = cx - gt[:, 0], cy - gt[:, 1], gt[:, 2] - cx, gt[:, 3] - cy
    q = (torch.minimum(l, r) / torch.maximum(l, r)) * (torch.minimum(t, b) / torch.maximum(t, b))
    return torch.where(q > 0, q.clamp(min=0).sqrt(), torch.zeros_like(q))


def giou(p, g):
    """mmdet's bbox_overlaps(mode='giou', is_aligned=True, eps=1e-6) of (P, 4) rows"""
    area1, area2 = (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1]), (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
    wh = (torch.minimum(p[:, 2:], g[:, 2:]) - torch.maximum(p[:, :2], g[:, :2])).clamp(min=0)
    overlap = wh[:, 0] * wh[:, 1]
    union = (area1 + area2 - overlap).clamp(min=EPS)
    ewh = (torch.maximum(p[:, 2:], g[:, 2:]) - torch.minimum(p[:, :2], g[:, :2])).clamp(min=0)
    enclose = (ewh[:, 0] * ewh[:, 1]).clamp(min=EPS)
    return overlap / union - (enclose - union) / enclose


def level_terms(cls_score, bbox_pred, centerness, anchors, labels, label_weights, bbox_targets, *, num_classes,
                reg_class_agnostic=True, gamma=2.0, alpha=0.25, target_means=(0., 0., 0., 0.),
                target_stds=(0.1, 0.1, 0.2, 0.2), dtype=torch.float64):
    """(S_cls, S_box, S_ctr, T) of one level, 0-dim tensors of ``dtype``: ``anchors`` (n, 4) of the level, ``labels`` /
    ``label_weights`` (B, n), ``bbox_targets`` (B, n, 4)"""
    C = num_classes
    batch = cls_score.shape[0]
    labels = labels.reshape(-1)
    x = rows_of(cls_score.to(dtype), C).contiguous()
    t = (labels[:, None] == torch.arange(C, device=labels.device)[None]).to(dtype)
    s_cls = (focal(x, t, gamma, alpha) * label_weights.reshape(-1, 1).to(dtype)).sum()
    if reg_class_agnostic:
        reg = rows_of(bbox_pred.to(dtype), 4)
    else:
        reg = bbox_pred.to(dtype).permute(0, 2, 3, 1).reshape(-1, 4, C)
        reg = torch.cat([reg, torch.zeros_like(reg[:, :, :1])], dim=-1)
        reg = torch.gather(reg, 2, labels.clamp(0, C).reshape(-1, 1, 1).repeat(1, 4, 1)).squeeze(-1)
    ctr = centerness.to(dtype).permute(0, 2, 3, 1).reshape(-1)
    pos = ((labels >= 0) & (labels < C)).nonzero(as_tuple=False).reshape(-1)
    zero = reg.sum() * 0 + ctr.sum() * 0
    if len(pos) == 0:
        return s_cls, zero, zero, zero.detach()
    a = anchors.to(dtype).repeat(batch, 1)[pos]
    gt = delta2bbox(a, bbox_targets.reshape(-1, 4).to(dtype)[pos], target_means, target_stds)
    ct = centerness_target(a, gt)
    p = delta2bbox(a, reg[pos], target_means, target_stds)
    if not torch.any(ct > 0):
        s_box = (p * ct[:, None]).sum()
    else:
        s_box = (ct * (1 - giou(p, gt))).sum()
    z = ctr[pos]
    s_ctr = (z.clamp(min=0) - z * ct + torch.log1p(torch.exp(-z.abs()))).sum()
    return s_cls, s_box, s_ctr, ct.sum().detach()


def loss_terms(cls_scores, bbox_preds, centernesses, anchors, labels, label_weights, bbox_targets, **kw):
    """(S_cls (L,), S_box (L,), S_ctr (L,), T): ``level_terms`` once per level over slices of the dense (B, A, ...)
    targets, ``anchors`` (A, 4) with the levels concatenated"""
    out, start = [], 0
    for c, r, t in zip(cls_scores, bbox_preds, centernesses):
        n = c.shape[2] * c.shape[3]
        out.append(level_terms(c, r, t, anchors[start:start + n], labels[:, start:start + n],
                               label_weights[:, start:start + n], bbox_targets[:, start:start + n], **kw))
        start += n
    s_cls, s_box, s_ctr, ts = (torch.stack(v) for v in zip(*out))
    return s_cls, s_box, s_ctr, ts.sum()


def loss_dict(terms, num_total_pos, weights=(1.0, 2.0, 1.0), host_factors=False):
    """the arithmetic of ATSSHead.loss around the levels at world size 1: ``num_total_samples = max(num_total_pos, 1)``,
    ``bbox_avg_factor = max(T, 1)``; ``weights`` = the loss weights of (loss_cls, loss_bbox, loss_centerness).
    ``host_factors``: both factors go through ``.item()`` as in mmdet (two waits for the host)"""
    s_cls, s_box, s_ctr, total = terms
    if host_factors:
        samples = max(float(torch.as_tensor(num_total_pos, dtype=torch.float32, device=s_cls.device).item()), 1.0)
        factor = max(float(total.item()), 1.0)
    else:
        samples = torch.as_tensor(num_total_pos, dtype=s_cls.dtype, device=s_cls.device).clamp(min=1)
        factor = total.clamp(min=1)
    return dict(loss_cls=list((s_cls * weights[0] / samples).unbind(0)),
                loss_bbox=list((s_box * weights[1] / factor).unbind(0)),
                loss_centerness=list((s_ctr * weights[2] / samples).unbind(0)))
