"""Generate tests/golden/anchor_target.npz: nearest-BEV overlaps and the 3-D anchor head's training targets.

Run in the build container only (needs the reference checkout):   python tests/golden/make_golden_anchor_target.py

Executed unmodified, lifted by AST as make_golden.py does (the files cannot be imported: they need mmcv / mmdet):
  * ``AnchorTrainMixin`` whole -- ``anchor_target_3d``, ``anchor_target_3d_single``,
    ``anchor_target_single_assigner`` -- and ``get_direction_target`` (models/dense_heads/train_mixins.py);
  * ``DeltaXYZWLHRBBoxCoder.encode`` (core/bbox/coders/delta_xyzwhlr_bbox_coder.py:21-55);
  * ``bbox_overlaps_nearest_3d`` (core/bbox/iou_calculators/iou3d_calculator.py:99-145) with
    ``BaseInstance3DBoxes.bev`` / ``nearest_bev`` (core/bbox/structures/base_box3d.py:137-162) and ``limit_period``
    (core/bbox/structures/utils.py:11-25, its array-converter decorator taken off: tensors only here);
  * ``Anchor3DRangeGenerator`` (core/anchor/anchor_3d_generator.py:9-221, its registry decorator taken off).
Nothing of the reference is stored, only inputs and the outputs it produced.

STAND-INS for symbols of packages that are not installed (mmdet 2.x, mmcv), each restating the published behaviour:
  * ``bbox_overlaps`` (mmdet/core/bbox/iou_calculators/iou2d_calculator.py): boxes (x1, y1, x2, y2);
    area = (x2 - x1) (y2 - y1); lt = max of the top-left corners, rb = min of the bottom-right ones,
    wh = clamp(rb - lt, min=0), overlap = wh_x wh_y; union = area1 + area2 - overlap ('iou') or area1 ('iof'),
    union = max(union, eps = 1e-6); result overlap / union; (N, M), or (N,) when aligned.  In the boxes' dtype.
  * ``get_box_type``: returns a holder class (``tensor``, ``box_dim``) carrying the lifted ``bev`` and
    ``nearest_bev`` properties, which the LiDAR and depth box classes inherit unchanged.
  * ``MaxIoUAssigner`` (mmdet/core/bbox/assigners/max_iou_assigner.py): ``assign`` computes
    ``overlaps = iou_calculator(gt_bboxes, bboxes)`` (G, N) and calls ``assign_wrt_overlaps``: assigned = -1;
    per-anchor ``max / argmax = overlaps.max(dim=0)``, per-GT ``gt_max / gt_argmax = overlaps.max(dim=1)``;
    assigned = 0 where 0 <= max < neg_iou_thr; assigned = argmax + 1 where max >= pos_iou_thr; with
    match_low_quality, for i in range(G): if gt_max[i] >= min_pos_iou: assigned[overlaps[i] == gt_max[i]] = i + 1
    (gt_max_assign_all) or assigned[gt_argmax[i]] = i + 1.  Returns an ``AssignResult`` (gt_inds, max_overlaps,
    labels).  Ignore boxes are not restated: the cases have none (ignore_iof_thr = -1 as the configs set it).
  * ``PseudoSampler`` / ``SamplingResult`` (mmdet/core/bbox/samplers): pos_inds = nonzero(gt_inds > 0).unique(),
    neg_inds = nonzero(gt_inds == 0).unique(); pos_bboxes = bboxes[pos_inds], pos_assigned_gt_inds =
    gt_inds[pos_inds] - 1, pos_gt_bboxes = gt_bboxes[pos_assigned_gt_inds].
  * ``multi_apply`` (mmdet/core/utils/misc.py): map a function over zipped argument lists, transpose the results.
  * ``images_to_levels`` (mmdet/core/anchor/utils.py): stack the per-image targets, split dim 1 by level sizes.
  * ``mmcv.is_list_of``: every element of a list is of the given type.

Every case runs twice: in fp64 (anchors and GT boxes are the stored fp32 values cast up; the expected outputs) and
in fp32 on the CPU.  Stored error figures, read by the GPU tests (nothing is written into a test):
  fp32_overlap_error   largest |fp64 - fp32| of any overlap: every (slot, image) matrix of every case and the
                       standalone sets (matrix, aligned, iof)
  fp32_target_error    the same for the encoded bbox_targets

Discrete outputs must not depend on rounding.  Asserted for every case (a GT that violates a guard is redrawn, no
case is dropped):
  * every per-anchor maximum and every per-GT maximum is at least GUARD = 1e-5 from pos_iou_thr, neg_iou_thr and
    min_pos_iou of its slot;
  * the best and second-best GT of an anchor differ by at least GUARD unless they are equal in fp64;
  * for every positive, offset_rot / pi is at least DIR_GUARD = 1e-4 from an integer;
  * |r| of every box is at least 1e-3 from pi / 4 (the nearest-BEV swap);
  * the fp32 and fp64 runs agree on every label, weight, direction bin and count.

Cases.  Config K's anchor sizes, rotations, z and per-slot thresholds; the x / y ranges are scaled to the map at a
0.5 m stride starting at (2, -H/4): anchor centres are multiples of 0.5, exact in fp32.
  small      5 x 6   (180 anchors: under one block)        B = 1, G = 7 over the three classes
  odd        7 x 9   (378 anchors: no multiple of 64)      B = 1, G = 7
  posw       small's inputs with pos_weight = 2
  batch      40 x 36 (8640 anchors: several blocks)        B = 2, G = (9, 5); image 1 has no GT of class 2
  empty      40 x 36                                       B = 2, G = (6, 0): an image without any GT
  g70        40 x 36                                       B = 1, G = 70 of class 0: more than one LDS chunk
  shared     40 x 36 assign_per_class = False              B = 1, G = 7
  rules_all / rules_first   40 x 36, gt_max_assign_all = True / False, the same hand-placed GT boxes:
             low     a car whose maximum lies between min_pos_iou and pos_iou_thr: matched by the low-quality
                     rule only
             miss    a pedestrian whose maximum is below min_pos_iou: no positive
             band    (with them) anchors whose maximum lies in [neg_iou_thr, pos_iou_thr): ignored
             tie     a car exactly midway between two anchor centres, inside both anchors: both overlaps are the
                     same bits; both anchors are assigned with gt_max_assign_all, only the first without
             claim   two pedestrians whose maxima sit on one anchor: the later one wins, though the earlier one
                     overlaps more
             yaws in every quadrant, and |r| either side of pi / 4 (0.02 away)
"""
import ast
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402

GUARD = 1e-5
DIR_GUARD = 1e-4
SWAP_GUARD = 1e-3
SIZES = [[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]]
Z = [-1.78, -0.6, -0.6]
ROTATIONS = [0, 1.57]
THRESHOLDS = [dict(pos_iou_thr=0.6, neg_iou_thr=0.45, min_pos_iou=0.45),
              dict(pos_iou_thr=0.5, neg_iou_thr=0.35, min_pos_iou=0.35),
              dict(pos_iou_thr=0.5, neg_iou_thr=0.35, min_pos_iou=0.35)]
DIR_OFFSET, DIR_LIMIT_OFFSET = 0.7854, 0
STRIDE = 0.5


# ---------------------------------------------------------------------------------------------------------
# stand-ins (see the module docstring)
# ---------------------------------------------------------------------------------------------------------
def bbox_overlaps(bboxes1, bboxes2, mode='iou', is_aligned=False, eps=1e-6):
    assert mode in ('iou', 'iof')
    area1 = (bboxes1[..., 2] - bboxes1[..., 0]) * (bboxes1[..., 3] - bboxes1[..., 1])
    area2 = (bboxes2[..., 2] - bboxes2[..., 0]) * (bboxes2[..., 3] - bboxes2[..., 1])
    if is_aligned:
        lt = torch.max(bboxes1[..., :2], bboxes2[..., :2])
        rb = torch.min(bboxes1[..., 2:], bboxes2[..., 2:])
        wh = (rb - lt).clamp(min=0)
        overlap = wh[..., 0] * wh[..., 1]
        union = area1 + area2 - overlap if mode == 'iou' else area1
    else:
        lt = torch.max(bboxes1[..., :, None, :2], bboxes2[..., None, :, :2])
        rb = torch.min(bboxes1[..., :, None, 2:], bboxes2[..., None, :, 2:])
        wh = (rb - lt).clamp(min=0)
        overlap = wh[..., 0] * wh[..., 1]
        union = area1[..., None] + area2[..., None, :] - overlap if mode == 'iou' else area1[..., None]
    union = torch.max(union, union.new_tensor([eps]))
    return overlap / union


class AssignResult:
    def __init__(self, num_gts, gt_inds, max_overlaps, labels=None):
        self.num_gts, self.gt_inds, self.max_overlaps, self.labels = num_gts, gt_inds, max_overlaps, labels


class MaxIoUAssigner:
    def __init__(self, pos_iou_thr, neg_iou_thr, min_pos_iou=.0, gt_max_assign_all=True, ignore_iof_thr=-1,
                 match_low_quality=True, iou_calculator=None):
        self.pos_iou_thr, self.neg_iou_thr, self.min_pos_iou = pos_iou_thr, neg_iou_thr, min_pos_iou
        self.gt_max_assign_all, self.ignore_iof_thr = gt_max_assign_all, ignore_iof_thr
        self.match_low_quality, self.iou_calculator = match_low_quality, iou_calculator
        self.seen = []                                    # the overlap matrices, for the guards

    def assign(self, bboxes, gt_bboxes, gt_bboxes_ignore=None, gt_labels=None):
        assert gt_bboxes_ignore is None
        overlaps = self.iou_calculator(gt_bboxes, bboxes)
        self.seen.append(overlaps)
        return self.assign_wrt_overlaps(overlaps, gt_labels)

    def assign_wrt_overlaps(self, overlaps, gt_labels=None):
        num_gts, num_bboxes = overlaps.size(0), overlaps.size(1)
        assigned_gt_inds = overlaps.new_full((num_bboxes, ), -1, dtype=torch.long)
        assert num_gts > 0 and num_bboxes > 0             # (the mixin does not call it otherwise)
        max_overlaps, argmax_overlaps = overlaps.max(dim=0)
        gt_max_overlaps, gt_argmax_overlaps = overlaps.max(dim=1)
        assert isinstance(self.neg_iou_thr, float)
        assigned_gt_inds[(max_overlaps >= 0) & (max_overlaps < self.neg_iou_thr)] = 0
        pos_inds = max_overlaps >= self.pos_iou_thr
        assigned_gt_inds[pos_inds] = argmax_overlaps[pos_inds] + 1
        if self.match_low_quality:
            for i in range(num_gts):
                if gt_max_overlaps[i] >= self.min_pos_iou:
                    if self.gt_max_assign_all:
                        max_iou_inds = overlaps[i, :] == gt_max_overlaps[i]
                        assigned_gt_inds[max_iou_inds] = i + 1
                    else:
                        assigned_gt_inds[gt_argmax_overlaps[i]] = i + 1
        assigned_labels = None
        if gt_labels is not None:
            assigned_labels = assigned_gt_inds.new_full((num_bboxes, ), -1)
            pos = torch.nonzero(assigned_gt_inds > 0, as_tuple=False).squeeze()
            if pos.numel() > 0:
                assigned_labels[pos] = gt_labels[assigned_gt_inds[pos] - 1]
        return AssignResult(num_gts, assigned_gt_inds, max_overlaps, labels=assigned_labels)


class SamplingResult:
    def __init__(self, pos_inds, neg_inds, bboxes, gt_bboxes, assign_result):
        self.pos_inds, self.neg_inds = pos_inds, neg_inds
        self.pos_bboxes, self.neg_bboxes = bboxes[pos_inds], bboxes[neg_inds]
        self.pos_assigned_gt_inds = assign_result.gt_inds[pos_inds] - 1
        self.pos_gt_bboxes = gt_bboxes[self.pos_assigned_gt_inds, :]


class PseudoSampler:
    def sample(self, assign_result, bboxes, gt_bboxes, **kwargs):
        pos_inds = torch.nonzero(assign_result.gt_inds > 0, as_tuple=False).squeeze(-1).unique()
        neg_inds = torch.nonzero(assign_result.gt_inds == 0, as_tuple=False).squeeze(-1).unique()
        return SamplingResult(pos_inds, neg_inds, bboxes, gt_bboxes, assign_result)


def multi_apply(func, *args, **kwargs):
    from functools import partial
    pfunc = partial(func, **kwargs) if kwargs else func
    return tuple(map(list, zip(*map(pfunc, *args))))


def images_to_levels(target, num_levels):
    target = torch.stack(target, 0)
    level_targets, start = [], 0
    for n in num_levels:
        level_targets.append(target[:, start:start + n])
        start += n
    return level_targets


# ---------------------------------------------------------------------------------------------------------
# the reference, lifted
# ---------------------------------------------------------------------------------------------------------
def lift(path, names, glb):
    for node in ast.parse(open(path).read()).body:
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)) and node.name in names:
            node.decorator_list = []
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, 'exec'), glb)
    return glb


def load_reference():
    mmcv = types.SimpleNamespace(is_list_of=lambda seq, kind: isinstance(seq, list) and
                                 all(isinstance(x, kind) for x in seq))
    g = {'torch': torch, 'np': np, 'mmcv': mmcv, 'bbox_overlaps': bbox_overlaps, 'multi_apply': multi_apply,
         'images_to_levels': images_to_levels}
    lift(mg.REF + 'core/bbox/structures/utils.py', ['limit_period'], g)
    box = {}
    for name in ('bev', 'nearest_bev'):
        mg.extract_method(mg.REF + 'core/bbox/structures/base_box3d.py', 'BaseInstance3DBoxes', name, g)
        box[name] = property(g.pop(name))

    def init(self, tensor, box_dim=7):
        self.tensor, self.box_dim = tensor, box_dim
    holder = type('Boxes', (), dict(__init__=init, **box))
    g['get_box_type'] = lambda coordinate: (holder, None)
    lift(mg.REF + 'core/bbox/iou_calculators/iou3d_calculator.py', ['bbox_overlaps_nearest_3d'], g)
    lift(mg.REF + 'models/dense_heads/train_mixins.py', ['AnchorTrainMixin', 'get_direction_target'], g)
    mg.extract_method(mg.REF + 'core/bbox/coders/delta_xyzwhlr_bbox_coder.py', 'DeltaXYZWLHRBBoxCoder', 'encode', g)
    lift(mg.REF + 'core/anchor/anchor_3d_generator.py', ['Anchor3DRangeGenerator'], g)
    return g


def make_anchors(g, H, W):
    """(1, H, W, 3, 2, 7) fp32 and the ranges used"""
    x0, y0 = 2.0, -H / 4
    ranges = [[x0, y0, z, x0 + STRIDE * (W - 1), y0 + STRIDE * (H - 1), z] for z in Z]
    gen = g['Anchor3DRangeGenerator'](ranges=ranges, sizes=SIZES, rotations=ROTATIONS, reshape_out=False)
    anchors = gen.grid_anchors([(H, W)], device='cpu')[0]
    assert anchors.shape == (1, H, W, 3, 2, 7) and anchors.dtype == torch.float32
    xs = anchors[0, 0, :, 0, 0, 0].double().numpy()
    assert np.array_equal(xs, x0 + STRIDE * np.arange(W)), 'anchor centres are not exact multiples of the stride'
    return anchors


def make_head(g, dtype, per_class=True, assign_all=True, pos_weight=-1):
    calc = lambda a, b, mode='iou', is_aligned=False: g['bbox_overlaps_nearest_3d'](a, b, mode, is_aligned)  # noqa
    head = g['AnchorTrainMixin']()
    head.bbox_assigner = [MaxIoUAssigner(gt_max_assign_all=assign_all, iou_calculator=calc, **t) for t in THRESHOLDS]
    head.bbox_sampler = PseudoSampler()
    head.bbox_coder = types.SimpleNamespace(encode=g['encode'])
    head.train_cfg = types.SimpleNamespace(pos_weight=pos_weight)
    head.dir_offset, head.dir_limit_offset = DIR_OFFSET, DIR_LIMIT_OFFSET
    head.assign_per_class, head.box_code_size = per_class, 7
    return head


def run(g, anchors, gts, labels, dtype, **cfg):
    """the reference method in ``dtype`` -> (dict of (B, A, ...) arrays + counts, the head)"""
    head = make_head(g, dtype, **cfg)
    B = len(gts)
    a = anchors.to(dtype)
    res = head.anchor_target_3d([[a] for _ in range(B)], [torch.from_numpy(x).to(dtype) for x in gts],
                                [dict() for _ in range(B)], gt_labels_list=[torch.from_numpy(x) for x in labels],
                                num_classes=3, sampling=False)
    names = ('labels', 'label_weights', 'bbox_targets', 'bbox_weights', 'dir_targets', 'dir_weights')
    out = {n: r[0].numpy() for n, r in zip(names, res[:6])}
    pos = out['bbox_weights'][:, :, 0] > 0
    neg = (out['label_weights'] > 0) & ~pos
    out['counts'] = np.stack([pos.sum(1), neg.sum(1)], 1).astype(np.int32)
    out['num_total_pos'], out['num_total_neg'] = np.int64(res[6]), np.int64(res[7])
    assert res[6] == np.maximum(out['counts'][:, 0], 1).sum() and res[7] == np.maximum(out['counts'][:, 1], 1).sum()
    return out, head


# ---------------------------------------------------------------------------------------------------------
# guards
# ---------------------------------------------------------------------------------------------------------
def swap_margin(yaw):
    yaw = np.asarray(yaw, np.float64)
    return np.abs(np.abs(yaw - np.floor(yaw / np.pi + 0.5) * np.pi) - np.pi / 4)


def bad_gts(g, anchors, gt, label, per_class):
    """indices of the GT boxes of one image that violate a guard (fp64)"""
    bad = set(np.nonzero(swap_margin(gt[:, 6]) < SWAP_GUARD)[0].tolist())
    a64 = anchors.double()
    for c, thr in enumerate(THRESHOLDS):
        idx = np.nonzero(label == c)[0] if per_class else np.arange(len(gt))
        if len(idx) == 0:
            continue
        ov = g['bbox_overlaps_nearest_3d'](torch.from_numpy(gt[idx]).double(), a64[..., c, :, :].reshape(-1, 7))
        ov = ov.numpy()
        for t in thr.values():
            close = np.abs(ov.max(1) - t) < GUARD                              # a GT's maximum
            bad.update(idx[close].tolist())
            close = np.abs(ov.max(0) - t) < GUARD                              # an anchor's maximum: blame its GT
            bad.update(idx[ov.argmax(0)[close]].tolist())
        if len(idx) > 1:
            order = np.sort(ov, 0)
            near = (order[-1] - order[-2] < GUARD) & (order[-1] != order[-2])
            bad.update(idx[ov.argmax(0)[near]].tolist())
        # direction bins of the pairs that can become positive: the argmax pairs and the per-GT maxima
        flat = a64[..., c, :, :].reshape(-1, 7).numpy()
        for k, i in enumerate(idx):
            cand = np.nonzero((ov[k] == ov[k].max()) | ((ov.argmax(0) == k) & (ov[k] >= thr['pos_iou_thr'])))[0]
            rot = (gt[i, 6].astype(np.float64) - flat[cand, 6]) + flat[cand, 6] - DIR_OFFSET
            off = (rot - np.floor(rot / (2 * np.pi) + DIR_LIMIT_OFFSET) * 2 * np.pi) / np.pi
            if np.any(np.abs(off - np.round(off)) < DIR_GUARD):
                bad.add(int(i))
    return sorted(bad)


def draw_gt(rng, anchors, c):
    """a GT box of class c near a random anchor of its slot"""
    _, H, W, _, R, _ = anchors.shape
    a = anchors[0, rng.randint(H), rng.randint(W), c, rng.randint(R)].double().numpy()
    scale = min(SIZES[c][0], SIZES[c][1])
    box = a.copy()
    box[0:2] += rng.uniform(-0.22, 0.22, 2) * min(1.0, scale)
    box[2] += rng.normal(0, 0.1)
    box[3:6] *= rng.uniform(0.85, 1.15, 3)
    box[6] += rng.normal(0, 0.25) + rng.randint(-1, 2) * np.pi
    return box.astype(np.float32)


def scene(g, rng, anchors, classes, per_class=True, fixed=None):
    """GT boxes (fp32) and labels of one image: ``fixed`` hand-placed rows first (never redrawn), then one drawn
    box per entry of ``classes``; drawn boxes that violate a guard are redrawn"""
    fixed_boxes, fixed_labels = fixed if fixed is not None else (np.zeros((0, 7), np.float32), np.zeros(0, np.int64))
    label = np.concatenate([fixed_labels, np.asarray(classes, np.int64)])
    if len(label) == 0:
        return np.zeros((0, 7), np.float32), label
    gt = np.concatenate([fixed_boxes] + [draw_gt(rng, anchors, c)[None] for c in classes]).astype(np.float32)
    for _ in range(500):
        bad = bad_gts(g, anchors, gt, label, per_class)
        if not bad:
            return gt, label
        redraw = [i for i in bad if i >= len(fixed_labels)]
        assert redraw, f'a hand-placed GT violates a guard: {bad}'
        for i in redraw:
            gt[i] = draw_gt(rng, anchors, int(label[i]))
    raise RuntimeError('no scene satisfies the guards')


# ---------------------------------------------------------------------------------------------------------
# the hand-placed GT boxes of the rules cases
# ---------------------------------------------------------------------------------------------------------
def rules_gts(g, anchors):
    _, H, W, _, _, _ = anchors.shape
    calc = g['bbox_overlaps_nearest_3d']

    def centre(h, w, c, r=0):
        return anchors[0, h, w, c, r].double().numpy()
    rows, labels = [], []
    # low: a car 0.2 m off an anchor centre, inside it and smaller: IoU 0.556, between 0.45 and 0.6
    a = centre(5, 6, 0)
    rows.append([a[0] + 0.21, a[1] + 0.09, a[2], 3.07, 1.13, 1.5, math.pi + 0.3])
    labels.append(0)
    # miss: a pedestrian a quarter of a stride off in both axes and smaller: maximum below 0.35
    a = centre(30, 8, 1)
    rows.append([a[0] + 0.25, a[1] + 0.25, a[2], 0.6, 0.5, 1.7, -2.0])
    labels.append(1)
    # tie: a car midway between two anchor centres (next to each other along x), inside both anchors, the pair
    # chosen so that the two fp32 overlaps are the same bits
    tie = None
    for h in range(12, H - 4):
        for w in range(20, W - 5):
            a, b = centre(h, w, 0), centre(h, w + 1, 0)
            box = np.array([(a[0] + b[0]) / 2, a[1], a[2], 3.25, 1.0, 1.5, -0.3], np.float32)
            assert float(box[0]) == (a[0] + b[0]) / 2
            pair = anchors[0, h, w:w + 2, 0, 0]
            o32 = calc(torch.from_numpy(box)[None], pair)[0]
            o64 = calc(torch.from_numpy(box)[None].double(), pair.double())[0]
            if o32[0] == o32[1] and o64[0] == o64[1] and tie is None:
                tie = box
    assert tie is not None, 'no exactly tied anchor pair'
    rows.append(tie.tolist())
    labels.append(0)
    # claim: two pedestrians around one anchor; the earlier one overlaps more, the later one wins
    a = centre(33, 25, 1)
    rows.append([a[0] + 0.03, a[1], a[2], 0.8, 0.6, 1.73, 0.05])
    rows.append([a[0] - 0.08, a[1] + 0.02, a[2], 0.8, 0.6, 1.73, math.pi - 0.1])
    labels += [1, 1]
    # yaws either side of pi / 4, in the quadrants the others miss
    a = centre(20, 4, 2)
    rows.append([a[0] + 0.05, a[1] - 0.04, a[2], 1.7, 0.6, 1.7, math.pi / 4 - 0.02])
    a = centre(24, 30, 2, 1)
    rows.append([a[0] - 0.05, a[1] + 0.03, a[2], 1.8, 0.62, 1.75, math.pi / 4 + 0.02])
    a = centre(10, 30, 2, 1)
    rows.append([a[0] + 0.02, a[1] + 0.06, a[2], 1.8, 0.58, 1.7, -math.pi / 2 - 0.2])
    labels += [2, 2, 2]
    return np.asarray(rows, np.float32), np.asarray(labels, np.int64)


def check_rules(out_all, out_first, gt, label, anchors):
    """the hand-placed boxes do what the docstring says (fp64 outputs of the two rules cases)"""
    A = out_all['labels'].shape[1]
    flat = anchors.reshape(-1, 7).double().numpy()

    def positives_of(out, i):
        """anchors whose encoded target decodes to GT i"""
        pos = np.nonzero(out['bbox_weights'][0, :, 0] > 0)[0]
        rg = out['bbox_targets'][0, pos, 6] + flat[pos, 6]
        xg = out['bbox_targets'][0, pos, 0] * np.hypot(flat[pos, 3], flat[pos, 4]) + flat[pos, 0]
        hit = (np.abs(rg - gt[i, 6]) < 1e-6) & (np.abs(xg - gt[i, 0]) < 1e-6)
        return pos[hit]
    assert len(positives_of(out_all, 0)) >= 1                      # low: matched ...
    assert len(positives_of(out_all, 1)) == 0                      # miss: not matched
    t_all, t_first = positives_of(out_all, 2), positives_of(out_first, 2)
    assert len(t_all) == 2 and len(t_first) == 1 and t_first[0] == t_all.min(), (t_all, t_first)
    claimed = ((33 * 36 + 25) * 3 + 1) * 2                         # claim: the anchor both pedestrians sit on
    for o in (out_all, out_first):                                 # the later one wins (0.77 against 0.93)
        assert claimed in positives_of(o, 4) and claimed not in positives_of(o, 3)
    ignored = (out_all['label_weights'][0] == 0)
    assert ignored.sum() > 0 and np.all(out_all['labels'][0][ignored] == 3)           # band
    quadrants = set((np.floor(gt[:, 6] / (np.pi / 2)).astype(int) % 4).tolist())
    assert quadrants == {0, 1, 2, 3} and np.any(gt[:, 6] < 0) and np.any(gt[:, 6] > np.pi), quadrants
    assert A == 8640


# ---------------------------------------------------------------------------------------------------------
def main():
    g = load_reference()
    rng = np.random.RandomState(4011)
    out = {}
    err = dict(overlap=0.0, target=0.0)
    grids = {k: make_anchors(g, *k) for k in ((5, 6), (7, 9), (40, 36))}

    def case(name, hw, gts, labels, **cfg):
        anchors = grids[hw]
        r64, h64 = run(g, anchors, gts, labels, torch.float64, **cfg)
        r32, h32 = run(g, anchors, gts, labels, torch.float32, **cfg)
        for a64, a32 in zip(h64.bbox_assigner, h32.bbox_assigner):
            for o64, o32 in zip(a64.seen, a32.seen):
                err['overlap'] = max(err['overlap'], float((o64 - o32.double()).abs().max()))
        for k in ('labels', 'label_weights', 'bbox_weights', 'dir_targets', 'dir_weights', 'counts',
                  'num_total_pos', 'num_total_neg'):
            assert np.array_equal(r64[k], r32[k]), (name, k)
        err['target'] = max(err['target'], float(np.abs(r64['bbox_targets'] - r32['bbox_targets']).max()))
        assert r64['labels'].dtype == np.int64 and r64['dir_targets'].dtype == np.int64
        offsets = np.concatenate([[0], np.cumsum([len(x) for x in gts])]).astype(np.int32)
        out[f'{name}/anchors'] = anchors.numpy()
        out[f'{name}/gt_boxes'] = np.concatenate(gts).astype(np.float32).reshape(-1, 7)
        out[f'{name}/gt_labels'] = np.concatenate(labels).astype(np.int64)
        out[f'{name}/gt_offsets'] = offsets
        out[f'{name}/assign_per_class'] = np.int32(cfg.get('per_class', True))
        out[f'{name}/gt_max_assign_all'] = np.int32(cfg.get('assign_all', True))
        out[f'{name}/pos_weight'] = np.float64(cfg.get('pos_weight', -1))
        for k, v in r64.items():
            out[f'{name}/{k}'] = v.astype(np.float32) if k in ('label_weights', 'bbox_weights', 'dir_weights') else v
        print(f'  {name}: A = {r64["labels"].shape[1]}, G = {np.diff(offsets).tolist()}, counts '
              f'{r64["counts"].tolist()}, ignored {int((r64["label_weights"] == 0).sum())}')
        return r64

    a = grids[(5, 6)]
    gt, lb = scene(g, rng, a, [0, 0, 0, 1, 1, 2, 2])
    perm = rng.permutation(7)                                # the classes interleaved
    gt, lb = gt[perm], lb[perm]
    r = case('small', (5, 6), [gt], [lb])
    assert r['counts'][0, 0] > 0
    r2 = case('posw', (5, 6), [gt], [lb], pos_weight=2)
    assert set(np.unique(r2['label_weights']).tolist()) >= {1.0, 2.0}
    gt, lb = scene(g, rng, grids[(7, 9)], [1, 0, 2, 1, 0, 2, 1])
    case('odd', (7, 9), [gt], [lb])
    big = grids[(40, 36)]
    g1, l1 = scene(g, rng, big, [0, 1, 2, 0, 1, 2, 0, 1, 2])
    g2, l2 = scene(g, rng, big, [0, 1, 0, 1, 0])
    r = case('batch', (40, 36), [g1, g2], [l1, l2])
    assert np.all(r['counts'][:, 0] > 0)
    g3, l3 = scene(g, rng, big, [2, 1, 0, 1, 2, 0])
    r = case('empty', (40, 36), [g3, np.zeros((0, 7), np.float32)], [l3, np.zeros(0, np.int64)])
    assert r['counts'][1].tolist() == [0, 8640]
    g4, l4 = scene(g, rng, big, [0] * 70)
    case('g70', (40, 36), [g4], [l4])
    g5, l5 = scene(g, rng, big, [0, 1, 2, 1, 0, 2, 1], per_class=False)
    case('shared', (40, 36), [g5], [l5], per_class=False)
    fixed = rules_gts(g, big)
    g6, l6 = scene(g, rng, big, [0, 1, 2], fixed=fixed)
    r_all = case('rules_all', (40, 36), [g6], [l6], assign_all=True)
    r_first = case('rules_first', (40, 36), [g6], [l6], assign_all=False)
    check_rules(r_all, r_first, g6.astype(np.float64), l6, big)

    # standalone overlaps: a matrix, its aligned diagonal block, iof; and hand-computed pairs
    calc = g['bbox_overlaps_nearest_3d']
    b1 = np.stack([draw_gt(rng, big, int(c)) for c in rng.randint(0, 3, 130)])
    b2 = b1[:37].copy()
    b2[:, 0:2] += rng.uniform(-0.6, 0.6, (37, 2)).astype(np.float32)
    b2[:, 3:5] *= rng.uniform(0.8, 1.2, (37, 2)).astype(np.float32)
    b2[:, 6] += rng.normal(0, 0.2, 37).astype(np.float32)
    keep = (swap_margin(b1[:, 6]) > SWAP_GUARD)
    keep[:37] &= swap_margin(b2[:, 6]) > SWAP_GUARD
    assert keep.all(), 'a standalone box sits on the swap threshold: change the seed'
    hand1 = np.asarray([[0, 0, 0, 2, 2, 1, 0], [0, 0, 0, 4, 2, 1, math.pi / 2], [3, 1, 0, 4, 2, 1, 0.7],
                        [3, 1, 0, 4, 2, 1, 0.8], [0, 0, 0, 4, 2, 1, math.pi + 0.1], [0, 0, 0, 2, 2, 1, 0],
                        [0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 4, 2, 1, -math.pi / 2 + 0.1]], np.float32)
    hand2 = np.asarray([[1, 0, 0, 2, 2, 1, 0], [0, 0, 0, 4, 2, 1, 0], [3, 1, 0, 4, 2, 1, 0],
                        [3, 1, 0, 4, 2, 1, 0], [0, 0, 0, 4, 2, 1, 0], [5, 0, 0, 2, 2, 1, 0],
                        [0, 0, 0, 0, 0, 0, 0], [0, 0, 5, 2, 4, 3, 0]], np.float32)
    for tag, x, y in (('overlaps', b1, b2), ('hand', hand1, hand2)):
        out[f'{tag}/boxes1'], out[f'{tag}/boxes2'] = x, y
        n = len(y)
        for key, kw, xs in (('iou', dict(mode='iou'), x), ('iof', dict(mode='iof'), x),
                            ('aligned_iou', dict(mode='iou', is_aligned=True), x[:n]),
                            ('aligned_iof', dict(mode='iof', is_aligned=True), x[:n])):
            v64 = calc(torch.from_numpy(xs).double(), torch.from_numpy(y).double(), **kw)
            v32 = calc(torch.from_numpy(xs), torch.from_numpy(y), **kw)
            err['overlap'] = max(err['overlap'], float((v64 - v32.double()).abs().max()))
            out[f'{tag}/{key}'] = v64.numpy()
    print('  hand iou', np.round(out['hand/aligned_iou'], 6).tolist(), 'iof', np.round(out['hand/aligned_iof'], 6).tolist())

    print('fp32_overlap_error', err['overlap'], 'fp32_target_error', err['target'])
    out.update(fp32_overlap_error=np.float64(err['overlap']), fp32_target_error=np.float64(err['target']),
               guard=np.float64(GUARD), dir_guard=np.float64(DIR_GUARD), dir_offset=np.float64(DIR_OFFSET),
               dir_limit_offset=np.float64(DIR_LIMIT_OFFSET), num_classes=np.int32(3),
               thresholds=np.asarray([[t['pos_iou_thr'], t['neg_iou_thr'], t['min_pos_iou']] for t in THRESHOLDS]))
    path = os.path.join(HERE, 'anchor_target.npz')
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    if not os.path.isdir(mg.REF):
        sys.exit('reference not mounted; the fixture is committed, nothing to do')
    torch.set_num_threads(1)
    main()
