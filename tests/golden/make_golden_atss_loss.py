"""Generate tests/golden/atss_loss.npz: the 2-D ATSS head's loss over all levels, from the reference's own code.

Run in the build container only (needs the reference checkout):   python tests/golden/make_golden_atss_loss.py

Executed unmodified, lifted by AST as make_golden_atss_target.py does (the file cannot be imported: it needs mmcv /
mmdet): ``LIGAATSSHead.loss_single`` (models/dense_heads/liga_atss_head.py:176-270) and
``LIGAATSSHead.centerness_target`` (:380-397).  Nothing of the reference is stored, only inputs and the outputs it
produced.

STAND-INS for symbols of packages that are not installed (mmdet 2.x, mmcv), each restating the published behaviour:
  * ``bbox2delta`` / ``delta2bbox`` behind ``DeltaXYWHBBoxCoder`` and ``multi_apply``: those of
    make_golden_atss_target.py (see its docstring), imported from it.
  * ``FocalLoss`` (mmdet/models/losses/focal_loss.py): ``py_sigmoid_focal_loss`` -- with p = sigmoid(x), t the one-hot
    label (the background label num_classes is the zero row) and pt = (1 - p) t + p (1 - t):
    binary_cross_entropy_with_logits(x, t) * (alpha t + (1 - alpha) (1 - t)) * pt^gamma, times the (N,) weight
    broadcast over the classes, summed and divided by ``avg_factor``, times ``loss_weight``: the stand-in of
    make_golden_anchor_loss.py, imported from it.
  * ``GIoULoss`` (mmdet/models/losses/iou_loss.py) with eps = 1e-6 and reduction 'mean': when no weight is positive
    ``(pred * weight[:, None]).sum()``; otherwise ``1 - bbox_overlaps(pred, target, mode='giou', is_aligned=True,
    eps)`` per row, where (mmdet/core/bbox/iou_calculators/iou2d_calculator.py) area = (x2 - x1) * (y2 - y1),
    overlap = prod(clamp(min(rb) - max(lt), min=0)), union = max(area1 + area2 - overlap, eps), ious = overlap / union,
    enclose = max(prod(clamp(max(rb) - min(lt), min=0)), eps), gious = ious - (enclose - union) / enclose; then the
    ``weighted_loss`` reduction: times the (N,) weight, summed, divided by ``avg_factor``; times ``loss_weight``.
  * ``CrossEntropyLoss(use_sigmoid=True)`` (mmdet/models/losses/cross_entropy_loss.py): for a (P,) prediction and a
    (P,) float label ``F.binary_cross_entropy_with_logits(pred, label, reduction='none')``, summed and divided by
    ``avg_factor``, times ``loss_weight``.  (mmdet writes ``label.float()``, the prediction's dtype in training; here
    the label takes the prediction's dtype, so that the fp64 run is not rounded to fp32 in the middle.)
  * the body of ``ATSSHead.loss`` (mmdet/models/dense_heads/atss_head.py) after ``get_targets``:
    ``num_total_samples = max(reduce_mean(num_total_pos), 1.0)``, ``multi_apply`` of ``loss_single`` over the levels
    (anchors, labels, label weights and bbox targets per level as ``images_to_levels`` splits the dense tensors),
    ``bbox_avg_factor = max(reduce_mean(sum of the levels' centerness sums), 1)``, ``losses_bbox`` divided by it;
    ``reduce_mean`` at world size 1 is the identity.

Targets come from tests/golden/atss_target.npz (what the reference's assigner produced), as the fp32 values the
kernels read: cases ``tiny``, ``five``, ``empty`` and ``rules``; C = 3, DeltaXYWHBBoxCoder means 0 and stds (0.1, 0.1,
0.2, 0.2), loss weights (1, 2, 1) as in the KITTI configs.  The maps are seeded draws: class logits N(-2, 1.5), centerness
logits N(0, 1), box deltas N(0, 1) except on the positive rows' own class, where they are the target deltas plus
N(0, 0.5) (x, y) and N(0, 0.8) (w, h) noise.  ``kinks`` is ``tiny`` with, on its first two positives, a predicted dw
whose decoded value lies well beyond the clamp (|e_2| = 6 > 4.135; the box, 62.5 anchors wide, is moved so that its
left side lies inside the target and the row's other three columns keep a gradient) and a predicted box moved 40
anchor widths away (a negative GIoU).

  tiny, kinks   32 x 48, strides (8, 16): 24 + 6 rows     B = 1, class-specific regression (12 box channels)
  tiny_agn      tiny with class-agnostic regression (its own box maps)
  five          64 x 256, strides 4 .. 64: 1364 rows      B = 2, class-agnostic
  empty         five's maps on the targets of `empty`     B = 2: image 1 has no GT, some levels have no positive
  rules         five's grid                               B = 1, class-specific

Every case runs twice, in fp64 (the maps and targets are the stored fp32 values cast up; the expected outputs and the
gradients of ``total = sum_{l, k} grad_out[l, k] * loss_k[l]`` with respect to every map, ``grad_out`` seeded and
stored) and in fp32 on the CPU.  Stored error figures, read by the GPU tests (nothing is written into a test), each the
largest over all cases of |fp32 - fp64| normalised per unit of |grad_S| = |grad_out[l, k] * loss_weight_k /
avg_factor_k|:
  fp32_loss_error       |fp32 - fp64| / |fp64| of any entry of the loss dict
  fp32_grad_cls_error   per unit of |grad_S_cls[l] * label_weight|
  fp32_grad_ctr_error   per unit of |grad_S_ctr[l]|
  fp32_grad_reg_error   per unit of |grad_S_box[l]| * ct * the decode's factor of the column: pw std_0, ph std_1,
                        gw std_2, gh std_3 (pw, ph the anchor's sides, gw, gh the predicted box's)
Draws stay away from the kinks (asserted; a positive row whose draw violates a guard is redrawn, no case is dropped):
no intersection or enclosing side within 1e-4 px of 0, no coordinate of a predicted box within 1e-4 px of its
target's, no |e_2|, |e_3| within 1e-4 of the clamp (the one beyond it in ``kinks`` is at 6), ct at least 1e-3.
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
import make_golden_anchor_loss as gl  # noqa: E402
import make_golden_atss_target as ag  # noqa: E402

C = 3
WEIGHTS = dict(loss_cls=1.0, loss_bbox=2.0, loss_centerness=1.0)
GUARD, CT_GUARD = 1e-4, 1e-3
MAX_RATIO = abs(np.log(16 / 1000))
FocalLoss, multi_apply, Coder = gl.FocalLoss, ag.multi_apply, ag.Coder


# ---------------------------------------------------------------------------------------------------------
# stand-ins (see the module docstring)
# ---------------------------------------------------------------------------------------------------------
def giou_aligned(b1, b2, eps):
    area1, area2 = (b1[:, 2] - b1[:, 0]) * (b1[:, 3] - b1[:, 1]), (b2[:, 2] - b2[:, 0]) * (b2[:, 3] - b2[:, 1])
    wh = (torch.min(b1[:, 2:], b2[:, 2:]) - torch.max(b1[:, :2], b2[:, :2])).clamp(min=0)
    overlap = wh[:, 0] * wh[:, 1]
    eps = area1.new_tensor([eps])
    union = torch.max(area1 + area2 - overlap, eps)
    ious = overlap / union
    ewh = (torch.max(b1[:, 2:], b2[:, 2:]) - torch.min(b1[:, :2], b2[:, :2])).clamp(min=0)
    enclose = torch.max(ewh[:, 0] * ewh[:, 1], eps)
    return ious - (enclose - union) / enclose


class GIoULoss(object):
    def __init__(self, eps=1e-6, loss_weight=1.0):
        self.eps, self.reduction, self.loss_weight = eps, 'mean', loss_weight

    def __call__(self, pred, target, weight=None, avg_factor=None):
        if weight is not None and not torch.any(weight > 0):
            return (pred * weight.unsqueeze(1)).sum()
        loss = (1 - giou_aligned(pred, target, self.eps)) * weight
        return self.loss_weight * (loss.sum() / avg_factor)


class CrossEntropyLoss(object):
    def __init__(self, loss_weight=1.0):
        self.use_sigmoid, self.use_mask, self.class_weight = True, False, None
        self.reduction, self.loss_weight = 'mean', loss_weight

    def __call__(self, cls_score, label, weight=None, avg_factor=None):
        loss = F.binary_cross_entropy_with_logits(cls_score, label.type_as(cls_score), reduction='none')
        return self.loss_weight * (loss.sum() / avg_factor)


def atss_head_loss(head, cls_scores, bbox_preds, centernesses, anchors, labels, label_weights, bbox_targets, sizes,
                   num_total_pos):
    """the body of ATSSHead.loss after get_targets, at world size 1"""
    split = lambda t: list(torch.split(t, sizes, dim=1))  # noqa: E731
    batch = labels.shape[0]
    anchor_list = split(anchors[None].expand(batch, -1, -1))
    num_total_samples = max(float(num_total_pos), 1.0)
    losses_cls, losses_bbox, loss_centerness, bbox_avg_factor = multi_apply(
        head.loss_single, anchor_list, cls_scores, bbox_preds, centernesses, split(labels), split(label_weights),
        split(bbox_targets), num_total_samples=num_total_samples)
    bbox_avg_factor = float(sum(bbox_avg_factor).clamp(min=1))
    losses_bbox = [x / bbox_avg_factor for x in losses_bbox]
    return dict(loss_cls=losses_cls, loss_bbox=losses_bbox, loss_centerness=loss_centerness), num_total_samples, \
        bbox_avg_factor


def make_head(g, agnostic):
    head = type('LIGAATSSHead', (), dict(loss_single=g['loss_single'], centerness_target=g['centerness_target']))()
    head.num_classes = head.cls_out_channels = C
    head.reg_class_agnostic, head.num_reg_channel, head.reg_avg_factor = agnostic, 4, 'default'
    head.loss_cls = FocalLoss(loss_weight=WEIGHTS['loss_cls'])
    head.loss_bbox = GIoULoss(loss_weight=WEIGHTS['loss_bbox'])
    head.loss_centerness = CrossEntropyLoss(loss_weight=WEIGHTS['loss_centerness'])
    head.bbox_coder = Coder()
    return head


def load_reference():
    g = {'torch': torch}
    for name in ('loss_single', 'centerness_target'):
        mg.extract_method(mg.REF + 'models/dense_heads/liga_atss_head.py', 'LIGAATSSHead', name, g)
    return g


# ---------------------------------------------------------------------------------------------------------
def level_shapes(grid):
    hw, strides = ag.GRIDS[grid]
    return [(-(-hw[0] // s), -(-hw[1] // s)) for s in strides]


def decode64(anchors, deltas):
    return ag.delta2bbox(torch.from_numpy(anchors).double(), torch.from_numpy(deltas).double(), Coder.means,
                         Coder.stds).numpy()


def kinks_of(anchors, target, pred):
    """the margins of positive rows (P, 4): smallest |side| of the intersection and the enclosing box, smallest
    coordinate distance of the two boxes, smallest distance of |e_2|, |e_3| from the clamp"""
    p, g = decode64(anchors, pred), decode64(anchors, target)
    inter = np.minimum(p[:, 2:], g[:, 2:]) - np.maximum(p[:, :2], g[:, :2])
    enclose = np.maximum(p[:, 2:], g[:, 2:]) - np.minimum(p[:, :2], g[:, :2])
    e = np.abs(pred[:, 2:].astype(np.float64) * np.asarray(Coder.stds[2:]))
    return np.minimum(np.minimum(np.abs(inter).min(1), np.abs(enclose).min(1)),
                      np.minimum(np.abs(p - g).min(1), np.abs(e - MAX_RATIO).min(1)))


def draw_maps(rng, shapes, batch, agnostic, anchors, labels, bbox_targets):
    """the three per-level map lists (fp32, NCHW) for dense targets (B, A) / (B, A, 4)"""
    A = anchors.shape[0]
    R = batch * A
    cls_rows = rng.normal(-2.0, 1.5, (R, C)).astype(np.float32)
    ctr_rows = rng.normal(0.0, 1.0, (R, 1)).astype(np.float32)
    width = 4 if agnostic else 4 * C
    reg_rows = rng.normal(0.0, 1.0, (R, width)).astype(np.float32)
    flat_labels, flat_targets = labels.reshape(-1), bbox_targets.reshape(-1, 4)
    for r in np.nonzero((flat_labels >= 0) & (flat_labels < C))[0]:
        cols = np.arange(4) if agnostic else np.arange(4) * C + flat_labels[r]
        for _ in range(200):
            d = (flat_targets[r] + rng.normal(0, 1, 4) * [0.5, 0.5, 0.8, 0.8]).astype(np.float32)
            if kinks_of(anchors[r % A][None], flat_targets[r][None], d[None])[0] >= GUARD:
                break
        else:
            raise RuntimeError('no draw satisfies the guards')
        reg_rows[r, cols] = d
    maps, start = ([], [], []), 0
    for h, w in shapes:
        n = h * w
        for dst, rows in zip(maps, (cls_rows, reg_rows, ctr_rows)):
            level = rows.reshape(batch, A, -1)[:, start:start + n]
            dst.append(np.ascontiguousarray(level.reshape(batch, h, w, -1).transpose(0, 3, 1, 2)))
        start += n
    return maps


def own_deltas(reg_maps, shapes, agnostic, labels):
    """(B * A, 4): each row's own-class deltas, from the maps"""
    rows = np.concatenate([m.transpose(0, 2, 3, 1).reshape(m.shape[0], h * w, -1)
                           for m, (h, w) in zip(reg_maps, shapes)], 1).reshape(-1, reg_maps[0].shape[1])
    if agnostic:
        return rows
    lab = np.clip(labels.reshape(-1), 0, C - 1)
    return np.stack([rows[np.arange(len(rows)), s * C + lab] for s in range(4)], 1)


def run(g, maps, agnostic, anchors, labels, label_weights, bbox_targets, sizes, num_total_pos, grad_out, dtype):
    head = make_head(g, agnostic)
    leaves = [[torch.from_numpy(m).to(dtype).requires_grad_(True) for m in kind] for kind in maps]
    losses, samples, factor = atss_head_loss(
        head, *leaves, torch.from_numpy(anchors).to(dtype), torch.from_numpy(labels),
        torch.from_numpy(label_weights).to(dtype), torch.from_numpy(bbox_targets).to(dtype), sizes, num_total_pos)
    out = torch.stack([torch.stack([v.reshape(()) for v in losses[k]])
                       for k in ('loss_cls', 'loss_bbox', 'loss_centerness')], 1)            # (L, 3)
    total = (out * torch.from_numpy(grad_out).to(dtype)).sum()
    flat = [m for kind in leaves for m in kind]
    grads = torch.autograd.grad(total, flat, allow_unused=True)
    grads = [torch.zeros_like(m) if gr is None else gr for m, gr in zip(flat, grads)]
    L = len(sizes)
    return out.detach().double().numpy(), [[gr.double().numpy() for gr in grads[k * L:(k + 1) * L]] for k in range(3)], \
        samples, factor


def main():
    g = load_reference()
    z = np.load(os.path.join(HERE, 'atss_target.npz'))
    assert int(z['num_classes']) == C and tuple(z['target_stds']) == Coder.stds and tuple(z['target_means']) == Coder.means
    rng = np.random.RandomState(2310)
    out = {}
    err = dict(loss=0.0, cls=0.0, reg=0.0, ctr=0.0)
    low = dict(kink=np.inf, ct=np.inf)
    drawn = {}

    def case(name, targets, grid, agnostic, maps_of=None, kinks=False):
        shapes = level_shapes(grid)
        sizes = [h * w for h, w in shapes]
        anchors = z[f'{targets}/anchors']
        labels = z[f'{targets}/labels']
        label_weights = z[f'{targets}/label_weights'].astype(np.float32)
        bbox_targets = z[f'{targets}/bbox_targets'].astype(np.float32)          # what the kernels read
        batch, A = labels.shape
        assert sum(sizes) == A == len(anchors) and z[f'{targets}/level_sizes'].tolist() == sizes
        pos = np.nonzero(((labels >= 0) & (labels < C)).reshape(-1))[0]
        if maps_of is None:
            maps = draw_maps(rng, shapes, batch, agnostic, anchors, labels, bbox_targets)
            if kinks:
                flat = labels.reshape(-1)
                first, second = pos[0], pos[1]
                lvl_rows = np.concatenate([[0], np.cumsum(sizes)])

                def poke(r, col, value, add=False):
                    b, n = divmod(r, A)
                    lv = int(np.searchsorted(lvl_rows, n, side='right') - 1)
                    y, x = divmod(n - lvl_rows[lv], shapes[lv][1])
                    ch = col if agnostic else col * C + flat[r]
                    maps[1][lv][b, ch, y, x] = value + (maps[1][lv][b, ch, y, x] if add else 0)
                poke(first, 2, 6.0 / Coder.stds[2])                       # e_2 = 6: beyond the clamp; the box is
                # exp(R) = 62.5 anchors wide: moved right by half of that, so that its left side lies inside the target
                # (a box that contains its target in x has no gradient in its x centre either)
                poke(first, 0, 0.5 * np.exp(MAX_RATIO) / Coder.stds[0], add=True)
                poke(second, 0, 40.0 / Coder.stds[0], add=True)           # 40 anchor widths to the right: disjoint
            drawn[name] = maps
            for kind, key in zip(maps, ('cls', 'reg', 'ctr')):
                for l, m in enumerate(kind):
                    out[f'{name}/{key}{l}'] = m
        else:
            maps = drawn[maps_of]
            out[f'{name}/maps_of'] = np.asarray(maps_of)
        grad_out = rng.uniform(0.5, 2.0, (len(sizes), 3)) * rng.choice([-1.0, 1.0], (len(sizes), 3))
        num_total_pos = int(z[f'{targets}/num_total_pos'])
        args = (g, maps, agnostic, anchors, labels, label_weights, bbox_targets, sizes, num_total_pos, grad_out)
        o64, g64, samples, factor = run(*args, torch.float64)
        o32, g32, _, _ = run(*args, torch.float32)
        # the guards
        a_rows = np.tile(anchors, (batch, 1))[pos]
        deltas = own_deltas(maps[1], shapes, agnostic, labels)[pos]
        gt = decode64(a_rows, bbox_targets.reshape(-1, 4)[pos])
        ct = np.zeros(0)
        if len(pos):
            margins = kinks_of(a_rows, bbox_targets.reshape(-1, 4)[pos], deltas)
            if kinks:
                e2 = np.abs(deltas[:, 2].astype(np.float64) * Coder.stds[2])
                assert (e2 > MAX_RATIO + 1).sum() == 1
                p = decode64(a_rows, deltas)
                assert ((np.minimum(p[:, 2], gt[:, 2]) - np.maximum(p[:, 0], gt[:, 0])) < -GUARD).sum() >= 1
            low['kink'] = min(low['kink'], margins.min())
            cx, cy = (a_rows[:, 0] + a_rows[:, 2]) / 2, (a_rows[:, 1] + a_rows[:, 3]) / 2
            lr = np.stack([cx - gt[:, 0], gt[:, 2] - cx], 1)
            tb = np.stack([cy - gt[:, 1], gt[:, 3] - cy], 1)
            ct = np.sqrt(lr.min(1) / lr.max(1) * tb.min(1) / tb.max(1))
            low['ct'] = min(low['ct'], ct.min())
        # the error figures
        nz = o64 != 0
        assert np.array_equal(nz, o32 != 0)
        err['loss'] = max(err['loss'], float((np.abs(o32 - o64)[nz] / np.abs(o64[nz])).max()))
        w = (WEIGHTS['loss_cls'] / samples, WEIGHTS['loss_bbox'] / factor, WEIGHTS['loss_centerness'] / samples)
        grad_s = np.abs(grad_out) * np.asarray(w)[None]                     # (L, 3)
        lw_rows = label_weights.reshape(batch, A)
        positive = ((labels >= 0) & (labels < C))
        own = own_deltas(maps[1], shapes, agnostic, labels).reshape(batch, A, 4).astype(np.float64)
        start = 0
        for l, (h, w_) in enumerate(shapes):
            n = h * w_
            to_rows = lambda m: m.transpose(0, 2, 3, 1).reshape(batch, n, -1)  # noqa: E731
            lw = lw_rows[:, start:start + n, None]
            d = np.abs(to_rows(g32[0][l]) - to_rows(g64[0][l]))
            assert not d[np.broadcast_to(lw == 0, d.shape)].any()
            live = np.broadcast_to(lw != 0, d.shape)
            if live.any():
                err['cls'] = max(err['cls'], float((d / np.where(lw != 0, lw, 1) / grad_s[l, 0])[live].max()))
            ps = positive[:, start:start + n]
            d = np.abs(to_rows(g32[2][l]) - to_rows(g64[2][l]))[..., 0]
            assert not d[~ps].any()
            if ps.any():
                err['ctr'] = max(err['ctr'], float((d[ps] / grad_s[l, 2]).max()))
                a = anchors[start:start + n].astype(np.float64)
                pw, ph = (a[:, 2] - a[:, 0])[None], (a[:, 3] - a[:, 1])[None]
                e = own[:, start:start + n] * np.asarray(Coder.stds)
                gw = pw * np.exp(np.clip(e[..., 2], -MAX_RATIO, MAX_RATIO))
                gh = ph * np.exp(np.clip(e[..., 3], -MAX_RATIO, MAX_RATIO))
                factors = np.stack([pw * Coder.stds[0] + 0 * gw, ph * Coder.stds[1] + 0 * gh, gw * Coder.stds[2],
                                    gh * Coder.stds[3]], -1)                # (B, n, 4)
                ct_rows = np.zeros((batch, A))
                ct_rows.reshape(-1)[pos] = ct
                g32r, g64r = to_rows(g32[1][l]), to_rows(g64[1][l])
                if not agnostic:
                    lab = np.clip(labels[:, start:start + n], 0, C - 1)
                    pick = lambda m: np.stack([np.take_along_axis(m[..., s * C:(s + 1) * C], lab[..., None], 2)[..., 0]  # noqa: E731
                                               for s in range(4)], -1)
                    others = np.abs(g32r).sum(-1) - np.abs(pick(g32r)).sum(-1)
                    assert not others[ps].any()
                    g32r, g64r = pick(g32r), pick(g64r)
                assert not g32r[~ps].any() and not g64r[~ps].any()
                unit = grad_s[l, 1] * ct_rows[:, start:start + n, None] * factors
                err['reg'] = max(err['reg'], float((np.abs(g32r - g64r)[ps] / unit[ps]).max()))
            start += n
        out[f'{name}/targets'] = np.asarray(targets)
        out[f'{name}/level_hw'] = np.asarray(shapes, np.int32)
        out[f'{name}/reg_class_agnostic'] = np.bool_(agnostic)
        out[f'{name}/grad_out'] = grad_out
        out[f'{name}/loss'] = o64                                           # (L, 3): loss_cls, loss_bbox, loss_centerness
        out[f'{name}/num_total_samples'] = np.float64(samples)
        out[f'{name}/bbox_avg_factor'] = np.float64(factor)
        for kind, key in zip(g64, ('grad_cls', 'grad_reg', 'grad_ctr')):
            for l, m in enumerate(kind):
                out[f'{name}/{key}{l}'] = m
        per_level = np.add.reduceat(positive.sum(0), np.concatenate([[0], np.cumsum(sizes)[:-1]]))
        print(f'  {name}: targets {targets}, B = {batch}, levels {sizes}, positives per level {per_level.tolist()}, '
              f'num_total_samples {samples}, bbox_avg_factor {factor:.4f}')
        return o64, per_level

    case('tiny', 'tiny', 'tiny', False)
    case('tiny_agn', 'tiny', 'tiny', True)
    o, _ = case('kinks', 'tiny', 'tiny', False, kinks=True)
    case('five', 'five', 'five', True)       # (64-px anchors and up on a 64 x 256 image: positives on the finest level)
    o, per_level = case('empty', 'empty', 'five', True, maps_of='five')
    assert (per_level == 0).any() and (per_level > 0).any()
    assert not o[per_level == 0][:, 1:].any()                               # a level without a positive: exactly 0
    case('rules', 'rules', 'five', False)
    print('smallest margins', {k: float(v) for k, v in low.items()})
    assert low['kink'] >= GUARD and low['ct'] >= CT_GUARD
    print({f'fp32_{k}_error': v for k, v in err.items()})
    out.update(fp32_loss_error=np.float64(err['loss']), fp32_grad_cls_error=np.float64(err['cls']),
               fp32_grad_reg_error=np.float64(err['reg']), fp32_grad_ctr_error=np.float64(err['ctr']),
               guard=np.float64(GUARD), ct_guard=np.float64(CT_GUARD), num_classes=np.int32(C),
               **{f'weight/{k}': np.float64(v) for k, v in WEIGHTS.items()})
    path = os.path.join(HERE, 'atss_loss.npz')
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 512 * 1024


if __name__ == '__main__':
    if not os.path.isdir(mg.REF):
        sys.exit('reference not mounted; the fixture is committed, nothing to do')
    torch.set_num_threads(1)
    main()
