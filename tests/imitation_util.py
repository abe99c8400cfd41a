"""Helpers of the feature-imitation tests: the fixture's cases, and an in-test restatement of the reference's
ops (dfm.py:468-540 + imitation_utils.py) in plain torch -- test infrastructure for the sizes and modes the
fixture cannot hold."""
import os

import numpy as np
import torch

from tests import util

CASES = ('a_3d', 'b_2d', 'c_scale', 'c_center_scale', 'c_cw_center_scale', 'c_none', 'd_nan', 'e_miss', 'f_few',
         'g_eval')
MARGIN = 1e-3


def load():
    return np.load(os.path.join(util.GOLDEN, 'imitation.npz'))


def case(z, name):
    """the case's tensors (CPU, fp32) and recorded results; ``grad`` / ``grad_bf16``: the reference's
    d loss / d pred for a fp32 / a bf16 ``pred`` leaf (a gradient has its leaf's dtype)"""
    g = lambda k: z[f'{name}/{k}']  # noqa: E731
    pred = torch.from_numpy(g('pred_q').astype(np.float32) / 16.0)
    target = torch.from_numpy(g('target_q').astype(np.float32) / 16.0)
    if f'{name}/target_nan' in z.files:
        nan = np.unpackbits(g('target_nan'))[:target.numel()].reshape(target.shape).astype(bool)
        target[torch.from_numpy(nan)] = float('nan')
    mshape = (pred.shape[0],) + tuple(pred.shape[2:])
    n = int(np.prod(mshape))
    out = dict(pred=pred, target=target, points=torch.from_numpy(g('points')), boxes=torch.from_numpy(g('boxes')),
               loss=float(g('loss')), grad=torch.from_numpy(g('grad')),
               grad_bf16=torch.from_numpy(g('grad_bf16')).view(torch.bfloat16),
               positives=torch.from_numpy(np.unpackbits(g('positives'))[:n].reshape(mshape).astype(bool)),
               training=bool(g('training')), normalize=str(g('normalize')) or None, loss_weight=float(g('loss_weight')))
    for k in ('scale0', 'center0', 'scale1', 'center1'):
        if f'{name}/{k}' in z.files:
            out[k] = torch.from_numpy(g(k))
    return out


def local_coords(points, boxes):
    px, py = (points[..., i][:, :, None] for i in range(2))
    x, y, _, xs, ys, _, yaw = (boxes[..., i][:, None, :] for i in range(7))
    a = -yaw
    dx, dy = px - x, py - y
    lx = dx * torch.cos(a) - dy * torch.sin(a)
    ly = dx * torch.sin(a) + dy * torch.cos(a)
    return lx, ly, xs / 2, ys / 2


def inbox_cells(points, boxes):
    """(B, Ny, Nx) bool: the stated box test with z forced to 0 on both sides (then the z test only rejects
    negative z sizes)"""
    B = boxes.shape[0]
    ny, nx = points.shape[-3:-1]
    p = points.reshape(-1, ny * nx, 3).float()
    if p.shape[0] == 1:
        p = p.expand(B, -1, -1)
    lx, ly, hx, hy = local_coords(p, boxes.float())
    zok = (boxes[..., 5] >= 0)[:, None, :]
    return (zok & (lx > -hx) & (lx < hx) & (ly > -hy) & (ly < hy)).any(-1).view(B, ny, nx)


def face_margin(points, boxes):
    ny, nx = points.shape[-3:-1]
    p = points.reshape(-1, ny * nx, 3).float()
    if p.shape[0] == 1:
        p = p.expand(boxes.shape[0], -1, -1)
    lx, ly, hx, hy = local_coords(p, boxes.float())
    return float(torch.minimum((lx.abs() - hx).abs(), (ly.abs() - hy).abs()).min())


def restate(pred, target, positives_cells, layer, loss_weight, clamp=10, training=True):
    """the reference's ops from `positives` on, in torch on the tensors' device: returns (loss, positives).
    ``layer``: a NormalizeLayer of this package (its forward / update are checked against the fixture on
    their own) or None; ``positives_cells`` (B, Ny, Nx) bool or None for mode='full'."""
    B = pred.shape[0]
    fp = pred.float().permute(0, *range(2, pred.dim()), 1)
    ft = target.float().permute(0, *range(2, target.dim()), 1)
    if positives_cells is None:
        positives = torch.ones(ft.shape[:-1], dtype=torch.bool, device=pred.device)
    elif ft.dim() == 5:
        positives = positives_cells.unsqueeze(1).repeat(1, ft.shape[1], 1, 1)
    else:
        positives = positives_cells
    positives = positives & torch.any(ft != 0, dim=-1)
    reg_weights = positives.float()
    reg_weights = reg_weights / torch.clamp(positives.sum().float(), min=clamp)
    pos_inds = reg_weights > 0
    pp, pt = fp[pos_inds], ft[pos_inds]
    if layer is not None:
        layer.train(training)
        pt = layer(pt)
    pt = torch.where(torch.isnan(pt), pp, pt)
    loss = (0.5 * (pp - pt) ** 2 * reg_weights[pos_inds].unsqueeze(-1)).mean(-1).sum() / B * loss_weight
    return loss, positives


def seeded_scene(seed, B, ny, nx, step, nboxes, x0=0.0):
    """points (1, ny, nx, 3) and boxes (B, nboxes + 1, 7) with the face margin, last row zero-size"""
    rng = np.random.RandomState(seed)
    ys = (torch.arange(ny, dtype=torch.float32) - ny / 2 + 0.5) * step
    xs = (torch.arange(nx, dtype=torch.float32) + 0.5) * step + x0
    yy, xx = torch.meshgrid(ys, xs, indexing='ij')
    points = torch.stack([xx, yy, torch.full_like(xx, -1.0)], dim=-1)[None]
    b = np.zeros((B, nboxes + 1, 7), np.float32)
    for i in range(B):
        for t in range(nboxes):
            for _ in range(1000):     # each box re-drawn on its own until it keeps the margin
                b[i, t] = [x0 + rng.uniform(2 * step, (nx - 2) * step), rng.uniform(-(ny / 2 - 2), ny / 2 - 2) * step,
                           rng.uniform(-2, 0), rng.uniform(3.2, 4.8), rng.uniform(1.5, 2.1), rng.uniform(1.4, 1.9),
                           rng.uniform(-7.5, 7.5)]
                if face_margin(points, torch.from_numpy(b[i:i + 1, t:t + 1])) > MARGIN:
                    break
            else:
                raise RuntimeError('no box with the face margin')
    boxes = torch.from_numpy(b)
    assert face_margin(points, boxes) > MARGIN
    return points, boxes
