"""Generate tests/golden/anchor_loss.npz: the 3-D anchor head's loss_single, both head classes.

Run in the build container only (needs the reference checkout):   python tests/golden/make_golden_anchor_loss.py

Executed unmodified, lifted by AST as make_golden_bbox_decode.py does (the files cannot be imported: they need mmcv /
mmdet): ``Anchor3DHead.loss_single`` and ``add_sin_difference`` (models/dense_heads/anchor3d_head.py),
``LIGAAnchor3DHead.loss_single`` (liga_anchor3d_head.py), ``dist_reduce_mean`` (models/utils/common_utils.py: no
process group here, so the identity), ``DeltaXYZWLHRBBoxCoder.decode`` and ``iou3d_loss`` / ``IOU3DLoss`` over the
stand-in for mmcv's ``diff_iou_rotated_3d`` of make_golden_iou3d.py.  Nothing of the reference is stored, only inputs
and the outputs it produced.

STAND-INS for mmdet's loss classes (mmdet is not installed), written from their documented formulas, reduction
'mean' with an ``avg_factor`` = ``loss.sum() / avg_factor`` times ``loss_weight``:
  FocalLoss         sigmoid focal loss in the binary_cross_entropy_with_logits form of py_sigmoid_focal_loss, the
                    (N,) weight broadcast over the classes; a label equal to num_classes is the background row
  SmoothL1Loss      0.5 d^2 / beta below beta, |d| - 0.5 beta from there
  CrossEntropyLoss  softmax cross entropy per row times the row weight

Everything runs in fp64 on the CPU from the stored fp32 inputs.  One set of maps and targets (B = 2, 5 x 6, 6 anchors
per location, C = 3: 360 rows, 41 positives) serves every case; ``nopos`` replaces the labels by background.
Per case: ``out`` = the returned tuple (NaN where the reference returns None or has no such term) and the gradients
of sum_i grad_out[i] * out[i] with respect to the three maps, stored as fp32 (relative 6e-8: under 1 % of the bounds
the tests hold them to).

Cases
  plain            Anchor3DHead, num_total_samples = 41, diff_rad_by_sin, no code_weight
  plain_cw         Anchor3DHead, num_total_samples = None (the batch size), code_weight, no diff_rad_by_sin
  plain_nodir      Anchor3DHead without a direction classifier
  liga             LIGAAnchor3DHead, normalizer_clamp_value = 10, reduce_avg_factor off, num_total_samples = 41
  liga_reduce      the same with reduce_avg_factor on and num_total_samples = 4 (below the clamp)
  liga_iou         liga with loss_iou
  liga_reduce_iou  liga_reduce with loss_iou
  nopos            liga without a positive row (with loss_iou the reference cannot run there: its iou3d_loss opens
                   with ``assert target.numel() > 0``; the stored IoU entry is the value of the branch behind that
                   assert, ``(pred - target).sum(1) * 0.`` reduced: 0)
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
import make_golden_iou3d as gi  # noqa: E402

B, H, W, A, C, S = 2, 5, 6, 6, 3, 7
GRAD_OUT = (0.3, 1.7, -2.0, 0.5)
CODE_WEIGHT = [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2]
WEIGHTS = dict(loss_cls=1.0, loss_bbox=2.0, loss_dir=0.2, loss_iou=1.0)    # config K's loss weights


class FocalLoss(object):
    """STAND-IN (see the module docstring)"""

    def __init__(self, gamma=2.0, alpha=0.25, loss_weight=1.0):
        self.use_sigmoid, self.gamma, self.alpha, self.reduction, self.loss_weight = True, gamma, alpha, 'mean', loss_weight

    def __call__(self, pred, target, weight=None, avg_factor=None):
        t = F.one_hot(target, pred.shape[1] + 1)[:, :pred.shape[1]].type_as(pred)
        p = pred.sigmoid()
        pt = (1 - p) * t + p * (1 - t)
        focal_weight = (self.alpha * t + (1 - self.alpha) * (1 - t)) * pt.pow(self.gamma)
        loss = F.binary_cross_entropy_with_logits(pred, t, reduction='none') * focal_weight
        loss = loss * weight.view(-1, 1)
        return self.loss_weight * (loss.sum() / avg_factor)


class SmoothL1Loss(object):
    """STAND-IN (see the module docstring)"""

    def __init__(self, beta=1.0 / 9.0, loss_weight=1.0):
        self.beta, self.reduction, self.loss_weight = beta, 'mean', loss_weight

    def __call__(self, pred, target, weight=None, avg_factor=None):
        diff = torch.abs(pred - target)
        loss = torch.where(diff < self.beta, 0.5 * diff * diff / self.beta, diff - 0.5 * self.beta)
        return self.loss_weight * ((loss * weight).sum() / avg_factor)


class CrossEntropyLoss(object):
    """STAND-IN (see the module docstring)"""

    def __init__(self, loss_weight=1.0):
        self.use_sigmoid, self.use_mask, self.class_weight = False, False, None
        self.reduction, self.loss_weight = 'mean', loss_weight

    def __call__(self, cls_score, label, weight=None, avg_factor=None):
        loss = F.cross_entropy(cls_score, label, reduction='none') * weight
        return self.loss_weight * (loss.sum() / avg_factor)


def load_reference():
    g = gi.load_reference()                                    # iou3d_loss, IOU3DLoss, decode
    g['dist_reduce_mean'] = mg.extract(mg.REF + 'models/utils/common_utils.py', ['dist_reduce_mean'],
                                       {'dist': torch.distributed})['dist_reduce_mean']
    plain, liga = dict(g), dict(g)
    mg.extract_method(mg.REF + 'models/dense_heads/anchor3d_head.py', 'Anchor3DHead', 'loss_single', plain)
    mg.extract_method(mg.REF + 'models/dense_heads/anchor3d_head.py', 'Anchor3DHead', 'add_sin_difference', plain)
    mg.extract_method(mg.REF + 'models/dense_heads/liga_anchor3d_head.py', 'LIGAAnchor3DHead', 'loss_single', liga)
    base = type('Anchor3DHead', (), dict(loss_single=plain['loss_single'],
                                         add_sin_difference=staticmethod(plain['add_sin_difference'])))
    sub = type('LIGAAnchor3DHead', (base,), dict(loss_single=liga['loss_single']))
    return g, base, sub


def make_head(g, klass, with_dir=True, with_iou=False, code_weight=None, diff_rad_by_sin=True, **attrs):
    head = klass()
    head.num_classes, head.box_code_size, head.use_sigmoid_cls = C, S, True
    head.use_direction_classifier, head.diff_rad_by_sin = with_dir, diff_rad_by_sin
    head.train_cfg = dict(code_weight=code_weight)
    head.loss_cls = FocalLoss(loss_weight=WEIGHTS['loss_cls'])
    head.loss_bbox = SmoothL1Loss(loss_weight=WEIGHTS['loss_bbox'])
    head.loss_dir = CrossEntropyLoss(loss_weight=WEIGHTS['loss_dir'])
    head.loss_iou = g['IOU3DLoss'](loss_weight=WEIGHTS['loss_iou']) if with_iou else None
    head.bbox_coder = types.SimpleNamespace(decode=g['decode'])
    for k, v in attrs.items():
        setattr(head, k, v)
    return head


def draw(rng):
    N = H * W * A
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    rows = []
    for y, x in zip(ys.ravel(), xs.ravel()):
        for c, zb in enumerate((-1.78, -0.6, -0.6)):
            for rot in (0.0, 1.57):
                rows.append([2.0 + 0.5 * x, -1.0 + 0.5 * y, zb, *gi.SIZES[c], rot])
    anchors = np.asarray(rows, np.float32)                                                  # (N, 7)
    labels = np.full((B, N), C, np.int64)
    pos = rng.choice(B * N, 41, replace=False)
    pos = np.union1d(pos, [B * N - 1])[-41:]                                                 # the last row among them
    labels.reshape(-1)[pos] = rng.randint(0, C, len(pos))
    label_weights = np.ones((B, N), np.float32)
    label_weights.reshape(-1)[rng.choice(B * N, 30, replace=False)] = 0
    label_weights.reshape(-1)[pos] = 1
    a64 = np.tile(anchors.astype(np.float64), (B, 1))
    gt = a64.copy()
    gt[:, 0:2] += rng.normal(0, 0.4, (B * N, 2))
    gt[:, 2] += rng.normal(0, 0.15, B * N)
    gt[:, 3:6] *= np.exp(rng.normal(0, 0.12, (B * N, 3)))
    gt[:, 6] += rng.normal(0, 0.25, B * N)
    enc = gi.encode(a64, gt)
    bbox_targets = np.zeros((B * N, S), np.float32)
    bbox_targets[pos] = enc[pos]
    bbox_weights = np.zeros((B * N, S), np.float32)
    bbox_weights[pos] = 1
    dir_targets = np.zeros(B * N, np.int64)
    dir_targets[pos] = rng.randint(0, 2, len(pos))
    dir_weights = np.zeros(B * N, np.float32)
    dir_weights[pos] = 1
    noise = np.where(rng.rand(B * N, S) < 0.5, rng.uniform(-1 / 9, 1 / 9, (B * N, S)), rng.normal(0, 0.3, (B * N, S)))
    rows_pred = rng.normal(0, 0.5, (B * N, S))
    rows_pred[pos] = bbox_targets[pos] + noise[pos]

    def to_map(rows_, width):                                   # (B * N, width) -> (B, A * width, H, W)
        return np.ascontiguousarray(rows_.reshape(B, H, W, A * width).transpose(0, 3, 1, 2)).astype(np.float32)
    cls = to_map(rng.normal(-2.0, 1.5, (B * N, C)), C)
    reg = to_map(rows_pred, S)
    dirs = to_map(rng.normal(0, 1, (B * N, 2)), 2)
    return dict(cls=cls, reg=reg, dir=dirs, labels=labels, label_weights=label_weights,
                bbox_targets=bbox_targets.reshape(B, N, S), bbox_weights=bbox_weights.reshape(B, N, S),
                dir_targets=dir_targets.reshape(B, N), dir_weights=dir_weights.reshape(B, N), anchors=anchors)


def run(head, z, labels, num_total_samples):
    t = lambda k: torch.from_numpy(z[k])  # noqa: E731
    maps = [t(k).double().requires_grad_(True) for k in ('cls', 'reg', 'dir')]
    anchors = t('anchors').double()[None].expand(B, -1, -1).reshape(-1, S)
    losses = head.loss_single(maps[0], maps[1], maps[2] if head.use_direction_classifier else None,
                              torch.from_numpy(labels), t('label_weights').double(), t('bbox_targets').double(),
                              t('bbox_weights').double(), t('dir_targets'), t('dir_weights').double(), anchors,
                              num_total_samples)
    out = np.full(4, np.nan)
    total = 0
    for i, v in enumerate(losses):
        if v is not None:
            out[i] = float(v)
            total = total + GRAD_OUT[i] * v
    wanted = [m for m in maps if head.use_direction_classifier or m is not maps[2]]
    grads = torch.autograd.grad(total, wanted, allow_unused=True)
    grads = [np.zeros(m.shape, np.float32) if gr is None else gr.numpy().astype(np.float32)
             for m, gr in zip(wanted, grads)]
    return out, grads


def main():
    g, plain, liga = load_reference()
    z = draw(np.random.RandomState(7))
    out = dict(z)
    out['grad_out'] = np.asarray(GRAD_OUT, np.float64)
    out['code_weight'] = np.asarray(CODE_WEIGHT, np.float64)
    for k, v in WEIGHTS.items():
        out[f'weight/{k}'] = np.float64(v)
    nopos = np.full_like(z['labels'], C)
    npos = int(((z['labels'] >= 0) & (z['labels'] < C)).sum())
    lg = dict(normalizer_clamp_value=10)
    cases = [
        ('plain', make_head(g, plain), z['labels'], npos),
        ('plain_cw', make_head(g, plain, code_weight=CODE_WEIGHT, diff_rad_by_sin=False), z['labels'], None),
        ('plain_nodir', make_head(g, plain, with_dir=False), z['labels'], npos),
        ('liga', make_head(g, liga, reduce_avg_factor=False, **lg), z['labels'], npos),
        ('liga_reduce', make_head(g, liga, reduce_avg_factor=True, **lg), z['labels'], 4),
        ('liga_iou', make_head(g, liga, with_iou=True, reduce_avg_factor=False, **lg), z['labels'], npos),
        ('liga_reduce_iou', make_head(g, liga, with_iou=True, reduce_avg_factor=True, **lg), z['labels'], 4),
        ('nopos', make_head(g, liga, reduce_avg_factor=False, **lg), nopos, npos),
    ]
    for name, head, labels, nts in cases:
        res, grads = run(head, z, labels, nts)
        out[f'{name}/out'] = res
        out[f'{name}/num_total_samples'] = np.float64(-1 if nts is None else nts)
        for k, gr in zip(('grad_cls', 'grad_reg', 'grad_dir'), grads):
            out[f'{name}/{k}'] = gr
        print(f'  {name}: {type(head).__name__}, num_total_samples {nts}, out {res.tolist()}')
    out['nopos/labels'] = nopos
    out['nopos/out'][3] = 0.0
    assert np.all(out['nopos/out'][1:] == 0) and all(not out[f'nopos/{k}'].any() for k in ('grad_reg', 'grad_dir'))
    path = os.path.join(HERE, 'anchor_loss.npz')
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 100 * 1000


if __name__ == '__main__':
    if not os.path.isdir(mg.REF):
        sys.exit('reference not mounted; the fixture is committed, nothing to do')
    torch.set_num_threads(1)
    main()
