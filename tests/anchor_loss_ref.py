"""The 3-D anchor head's loss_single as torch expressions, written from the formulas of
include/dfm_hip_anchor_loss.h: the reference of tests/test_anchor_loss*.py (run in fp64) and the baseline of
tools/anchor_loss_timing.py (run in fp32 on the device: what a user of the package has without the fused kernels).

``loss_terms`` is the whole computation the way the head writes it -- permuted copies of the maps, a focal loss of a
dozen element-wise passes, ``nonzero``, indexed gathers, three reductions -- differentiated by autograd.  The IoU term
is ``iou`` = a callable ``(anchors (P, 7), pred deltas (P, 7), target deltas (P, 7)) -> (P,) loss``: by default the
decode and the differentiable rotated IoU restated in torch by tests/golden/make_golden_iou3d.py (any dtype), for the
baseline the package's ``iou3d_loss_from_deltas``.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
from make_golden_iou3d import iou3d_pairs  # noqa: E402


def decode(anchors, deltas):
    """DeltaXYZWLHRBBoxCoder.decode of (P, 7) rows, as include/dfm_hip_bbox_decode.h states it"""
    xa, ya, za, wa, la, ha, ra = anchors.unbind(1)
    xt, yt, zt, wt, lt, ht, rt = deltas.unbind(1)
    za = za + ha / 2
    diagonal = torch.sqrt(la * la + wa * wa)
    hg = torch.exp(ht) * ha
    return torch.stack([xt * diagonal + xa, yt * diagonal + ya, zt * ha + za - hg / 2, torch.exp(wt) * wa,
                        torch.exp(lt) * la, hg, rt + ra], 1)


def iou_rows(anchors, pred, target):
    """1 - IoU3D of the decoded rows, a NaN component of the decoded target replaced by the prediction's"""
    p, t = decode(anchors, pred), decode(anchors, target)
    t = torch.where(torch.isnan(t), p, t)
    if p.shape[0] == 0:
        return p.sum(1) * 0
    return 1 - iou3d_pairs(p, t)


def rows_of(m, width):
    """(B, A * width, H, W) -> (B * H * W * A, width): the reference's permute(0, 2, 3, 1).reshape(-1, width)"""
    return m.permute(0, 2, 3, 1).reshape(-1, width)


def focal(x, t, gamma, alpha):
    p = torch.sigmoid(x)
    pt = (1 - p) * t + p * (1 - t)
    bce = torch.clamp(x, min=0) - x * t + torch.log1p(torch.exp(-x.abs()))
    return (alpha * t + (1 - alpha) * (1 - t)) * pt.pow(gamma) * bce


def smooth_l1(d, beta):
    a = d.abs()
    return torch.where(a < beta, 0.5 * a * a / beta, a - 0.5 * beta)


def loss_terms(cls_score, bbox_pred, dir_cls_preds, labels, label_weights, bbox_targets, bbox_weights, dir_targets,
               dir_weights, anchors=None, *, num_classes, gamma=2.0, alpha=0.25, beta=1.0 / 9.0, code_weight=None,
               diff_rad_by_sin=True, with_iou=False, iou=iou_rows, dtype=torch.float64):
    """(S_cls, S_box, S_dir, S_iou), 0-dim tensors of ``dtype``: the unscaled term sums, differentiable with respect to
    the maps; the sums of an absent direction classifier or IoU term are 0"""
    C = num_classes
    A = cls_score.shape[1] // C
    S = bbox_pred.shape[1] // A
    labels = labels.reshape(-1)
    x = rows_of(cls_score.to(dtype), C)
    t = (labels[:, None] == torch.arange(C, device=labels.device)[None]).to(dtype)
    s_cls = (focal(x, t, gamma, alpha) * label_weights.reshape(-1, 1).to(dtype)).sum()
    pos = ((labels >= 0) & (labels < C)).nonzero(as_tuple=False).reshape(-1)
    reg = rows_of(bbox_pred.to(dtype), S)
    p, tg = reg[pos], bbox_targets.reshape(-1, S).to(dtype)[pos]
    w = bbox_weights.reshape(-1, S).to(dtype)[pos]
    if code_weight is not None:
        w = w * w.new_tensor(list(code_weight))
    pd, td = p, tg
    if diff_rad_by_sin:
        pd = torch.cat([p[:, :6], torch.sin(p[:, 6:7]) * torch.cos(tg[:, 6:7]), p[:, 7:]], 1)
        td = torch.cat([tg[:, :6], torch.cos(p[:, 6:7]) * torch.sin(tg[:, 6:7]), tg[:, 7:]], 1)
    s_box = (smooth_l1(pd - td, beta) * w).sum()
    zero = s_box * 0
    s_dir = zero
    if dir_cls_preds is not None:
        d = rows_of(dir_cls_preds.to(dtype), 2)[pos]
        dt = (dir_targets.reshape(-1)[pos] != 0).long()
        picked = d.gather(1, dt[:, None])[:, 0]
        s_dir = ((torch.logsumexp(d, 1) - picked) * dir_weights.reshape(-1).to(dtype)[pos]).sum()
    s_iou = zero
    if with_iou:
        n = anchors.shape[0]
        s_iou = iou(anchors.to(dtype)[pos % n], p[:, :7], tg[:, :7]).sum()
    return s_cls, s_box, s_dir, s_iou
