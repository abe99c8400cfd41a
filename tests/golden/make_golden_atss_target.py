"""Generate tests/golden/atss_target.npz: 2-D box overlaps and the 2-D ATSS head's training targets.

Run in the build container only (needs the reference checkout):   python tests/golden/make_golden_atss_target.py

Executed unmodified, lifted by AST as make_golden_anchor_target.py does (the files cannot be imported: they need
mmcv / mmdet):
  * ``ATSS3DCenterAssigner.assign`` (core/bbox/assigners/atss_3dcenter_assigner.py:27-168);
  * ``LIGAATSSHead._get_target_single`` and ``LIGAATSSHead.centerness_target`` (models/dense_heads/
    liga_atss_head.py:380-483); the latter only to record the centerness targets of the positives.
Nothing of the reference is stored, only inputs and the outputs it produced.

STAND-INS for symbols of packages that are not installed (mmdet 2.x, mmcv), each restating the published behaviour:
  * ``bbox_overlaps``, ``PseudoSampler`` / ``SamplingResult``, ``multi_apply``, ``images_to_levels``: those of
    make_golden_anchor_target.py (see its docstring), imported from it.
  * ``AssignResult`` (mmdet/core/bbox/assigners/assign_result.py): a holder of num_gts, gt_inds, max_overlaps, labels.
  * ``anchor_inside_flags`` (mmdet/core/anchor/utils.py): with allowed_border >= 0, valid_flags & x1 >= -ab &
    y1 >= -ab & x2 < img_w + ab & y2 < img_h + ab for img_shape[:2] = (img_h, img_w); otherwise the valid flags.
  * ``unmap`` (mmdet/core/utils/misc.py): a tensor of ``count`` rows filled with ``fill``, the data written to the
    rows where the flags are set.
  * ``bbox2delta`` / ``delta2bbox`` (mmdet/core/bbox/coder/delta_xywh_bbox_coder.py), the body of
    ``DeltaXYWHBBoxCoder.encode`` / ``decode``: px = (x1 + x2) * 0.5, pw = x2 - x1 (gt alike), deltas
    ((gx - px) / pw, (gy - py) / ph, log(gw / pw), log(gh / ph)), then (deltas - means) / stds; the decode is its
    inverse with dw, dh clamped to +-|log(16 / 1000)|.
  * the body of ``ATSSHead.get_targets`` (mmdet/models/dense_heads/atss_head.py): concatenate each image's levels,
    ``multi_apply`` of ``_get_target_single``, None when an image has no inside anchor, num_total_pos / neg = sum of
    max(count, 1), ``images_to_levels`` of the five dense lists; and ``get_num_level_anchors_inside``: the inside
    flags split by level and summed.  Here it also asks ``_get_target_single`` for its assign result
    (``return_sampling_results=True``) to record ``assigned_gt_inds``.
  * valid flags as ``AnchorGenerator.valid_flags`` gives them: per level the first min(ceil(pad_h / stride), feat_h)
    rows and min(ceil(pad_w / stride), feat_w) columns.

Anchors are plain data: squares of side 16 * stride centred on (x * stride, y * stride), y-major, one per location
(AnchorGenerator(ratios=[1.0], octave_base_scale=16, scales_per_octave=1), centre offset 0), feature maps of
ceil(image / stride).

Every case runs twice: in fp64 (anchors and GT boxes are the stored fp32 values cast up; the expected outputs) and in
fp32 on the CPU.  Stored error figures, read by the GPU tests (nothing is written into a test):
  fp32_target_error    largest |fp64 - fp32| of any encoded bbox target of any case
  fp32_overlap_error   the same for the standalone overlap sets (matrix, aligned, iou, iof)

Discrete outputs must not depend on rounding.  Asserted for every case from an independent fp64 restatement of the
assignment in numpy (``analyse``; its assignment must equal the reference's), a GT that violates a guard is redrawn
(hand-placed ones never are) and no case is dropped:
  * per (image, GT, level) with more counting anchors than k_l: the k_l-th and (k_l + 1)-th smallest distance differ
    by at least CUT_GUARD = 1e-3 px;
  * every candidate's iou is at least GUARD = 1e-5 from its GT's threshold;
  * every candidate's min(l, t, r, b) is at least INSET_GUARD = 1e-3 from 0.01;
  * an anchor's best and second-best claiming GT differ by at least GUARD in iou unless they are equal in fp64, in
    which case the reference must have taken the lower index;
  * the fp32 and fp64 runs agree on every discrete output.

Cases (topk = 9):
  tiny     32 x 48, strides (8, 16): 24 + 6 anchors        B = 1, G = 3: level 2 has 6 < 9 anchors, k_l = 6, N = 15
  odd      56 x 72, (8, 16, 32): 63 + 20 + 6 = 89           B = 1, G = 5: no multiple of 64
  five     64 x 256, (4, 8, 16, 32, 64): 1364               B = 2, G = (12, 5)
  posw     tiny's inputs with pos_weight = 2
  empty    five's grid                                      B = 2, G = (6, 0): an image without GT
  g70      five's grid                                      B = 1, G = 70
  border   five's grid, B = 2, G = (6, 6): img_shape (60, 250) and (64, 256), valid flags from pad shapes (64, 192)
           and (64, 256), allowed_border = 16.  (With allowed_border = 0 no 16 * stride anchor lies inside a
           64 x 256 image and the reference returns None; 16 is below half the finest anchor's side, so the finest
           level counts in part, differently per image, and the coarser levels not at all: k_l = 0 there.)
  valid    five's grid, B = 2, G = (6, 6): the same valid flags with allowed_border = -1: image 0 counts 3 of the 4
           coarsest anchors (k_l = 3) and three quarters of every other level
  centre4  five's grid, B = 1, G = 6: (G, 4) boxes, the box centres as the points
  rules    five's grid, B = 1, hand-placed GTs:
           off     3-D centre outside its 2-D box: candidates, no positive
           twin    two identical boxes with different labels: the lower index wins every anchor
           claim   two overlapping GTs that both claim one anchor: the later one wins by its higher iou
           small   a 6 x 6 px box: positives only from the finest level
"""
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
import make_golden_anchor_target as at  # noqa: E402

GUARD, CUT_GUARD, INSET_GUARD = 1e-5, 1e-3, 1e-3
TOPK, NUM_CLASSES = 9, 3
MEANS, STDS = (0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2)
bbox_overlaps, PseudoSampler, multi_apply, images_to_levels = (at.bbox_overlaps, at.PseudoSampler, at.multi_apply,
                                                               at.images_to_levels)


# ---------------------------------------------------------------------------------------------------------
# stand-ins (see the module docstring)
# ---------------------------------------------------------------------------------------------------------
class AssignResult:
    def __init__(self, num_gts, gt_inds, max_overlaps, labels=None):
        self.num_gts, self.gt_inds, self.max_overlaps, self.labels = num_gts, gt_inds, max_overlaps, labels


def anchor_inside_flags(flat_anchors, valid_flags, img_shape, allowed_border=0):
    img_h, img_w = img_shape[:2]
    if allowed_border >= 0:
        return valid_flags & (flat_anchors[:, 0] >= -allowed_border) & (flat_anchors[:, 1] >= -allowed_border) & \
            (flat_anchors[:, 2] < img_w + allowed_border) & (flat_anchors[:, 3] < img_h + allowed_border)
    return valid_flags


def unmap(data, count, inds, fill=0):
    if data.dim() == 1:
        ret = data.new_full((count, ), fill)
        ret[inds.type(torch.bool)] = data
    else:
        ret = data.new_full((count, ) + data.size()[1:], fill)
        ret[inds.type(torch.bool), :] = data
    return ret


def bbox2delta(proposals, gt, means, stds):
    px, py = (proposals[..., 0] + proposals[..., 2]) * 0.5, (proposals[..., 1] + proposals[..., 3]) * 0.5
    pw, ph = proposals[..., 2] - proposals[..., 0], proposals[..., 3] - proposals[..., 1]
    gx, gy = (gt[..., 0] + gt[..., 2]) * 0.5, (gt[..., 1] + gt[..., 3]) * 0.5
    gw, gh = gt[..., 2] - gt[..., 0], gt[..., 3] - gt[..., 1]
    deltas = torch.stack([(gx - px) / pw, (gy - py) / ph, torch.log(gw / pw), torch.log(gh / ph)], dim=-1)
    return deltas.sub_(deltas.new_tensor(means).unsqueeze(0)).div_(deltas.new_tensor(stds).unsqueeze(0))


def delta2bbox(rois, deltas, means, stds, wh_ratio_clip=16 / 1000):
    d = deltas * deltas.new_tensor(stds).view(1, -1) + deltas.new_tensor(means).view(1, -1)
    max_ratio = abs(math.log(wh_ratio_clip))
    dw, dh = d[:, 2].clamp(-max_ratio, max_ratio), d[:, 3].clamp(-max_ratio, max_ratio)
    px, py = (rois[:, 0] + rois[:, 2]) * 0.5, (rois[:, 1] + rois[:, 3]) * 0.5
    pw, ph = rois[:, 2] - rois[:, 0], rois[:, 3] - rois[:, 1]
    gw, gh, gx, gy = pw * dw.exp(), ph * dh.exp(), px + pw * d[:, 0], py + ph * d[:, 1]
    return torch.stack([gx - gw * 0.5, gy - gh * 0.5, gx + gw * 0.5, gy + gh * 0.5], dim=-1)


class Coder:
    means, stds = MEANS, STDS

    def encode(self, bboxes, gt_bboxes):
        return bbox2delta(bboxes, gt_bboxes, self.means, self.stds)

    def decode(self, bboxes, deltas):
        return delta2bbox(bboxes, deltas, self.means, self.stds)


def get_num_level_anchors_inside(self, num_level_anchors, inside_flags):
    return [int(flags.sum()) for flags in torch.split(inside_flags, num_level_anchors)]


def get_targets(self, anchor_list, valid_flag_list, gt_bboxes_list, img_metas, gt_bboxes_ignore_list=None,
                gt_labels_list=None, label_channels=1, unmap_outputs=True):
    num_imgs = len(img_metas)
    assert len(anchor_list) == len(valid_flag_list) == num_imgs
    num_level_anchors = [anchors.size(0) for anchors in anchor_list[0]]
    num_level_anchors_list = [num_level_anchors] * num_imgs
    anchor_list = [torch.cat(a) for a in anchor_list]
    valid_flag_list = [torch.cat(v) for v in valid_flag_list]
    if gt_bboxes_ignore_list is None:
        gt_bboxes_ignore_list = [None for _ in range(num_imgs)]
    if gt_labels_list is None:
        gt_labels_list = [None for _ in range(num_imgs)]
    (all_anchors, all_labels, all_label_weights, all_bbox_targets, all_bbox_weights, pos_inds_list, neg_inds_list,
     assign_results) = multi_apply(self._get_target_single, anchor_list, valid_flag_list, num_level_anchors_list,
                                   gt_bboxes_list, gt_bboxes_ignore_list, gt_labels_list, img_metas,
                                   label_channels=label_channels, unmap_outputs=unmap_outputs,
                                   return_sampling_results=True)
    if any([labels is None for labels in all_labels]):
        return None
    num_total_pos = sum([max(inds.numel(), 1) for inds in pos_inds_list])
    num_total_neg = sum([max(inds.numel(), 1) for inds in neg_inds_list])
    lists = [images_to_levels(t, num_level_anchors) for t in (all_anchors, all_labels, all_label_weights,
                                                             all_bbox_targets, all_bbox_weights)]
    self.seen = (assign_results, pos_inds_list)
    return (*lists, num_total_pos, num_total_neg)


# ---------------------------------------------------------------------------------------------------------
# the reference, lifted
# ---------------------------------------------------------------------------------------------------------
def load_reference():
    g = {'torch': torch, 'AssignResult': AssignResult, 'anchor_inside_flags': anchor_inside_flags, 'unmap': unmap}
    mg.extract_method(mg.REF + 'core/bbox/assigners/atss_3dcenter_assigner.py', 'ATSS3DCenterAssigner', 'assign', g)
    for name in ('_get_target_single', 'centerness_target'):
        mg.extract_method(mg.REF + 'models/dense_heads/liga_atss_head.py', 'LIGAATSSHead', name, g)
    return g


def make_head(g, width, pos_weight=-1, allowed_border=-1):
    assigner = type('ATSS3DCenterAssigner', (), dict(assign=g['assign']))()
    assigner.topk, assigner.ignore_iof_thr, assigner.thresh_mode = TOPK, -1, 'meanstd'
    assigner.append_3d_centers, assigner.iou_calculator = width == 6, bbox_overlaps
    head = type('LIGAATSSHead', (), dict(_get_target_single=g['_get_target_single'], get_targets=get_targets,
                                         centerness_target=g['centerness_target'],
                                         get_num_level_anchors_inside=get_num_level_anchors_inside))()
    head.assigner, head.sampler, head.bbox_coder = assigner, PseudoSampler(), Coder()
    head.train_cfg = types.SimpleNamespace(allowed_border=allowed_border, pos_weight=pos_weight)
    head.num_classes, head.num_reg_channel = NUM_CLASSES, 4
    return head


# ---------------------------------------------------------------------------------------------------------
# plain data: anchors and valid flags
# ---------------------------------------------------------------------------------------------------------
def make_anchors(hw, strides):
    levels = []
    for s in strides:
        fh, fw = -(-hw[0] // s), -(-hw[1] // s)
        ys, xs = np.meshgrid(np.arange(fh) * s, np.arange(fw) * s, indexing='ij')
        c = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)
        levels.append(np.concatenate([c - 8 * s, c + 8 * s], 1).astype(np.float32))
    return levels


def make_valid(hw, strides, pad_hw):
    flags = []
    for s in strides:
        fh, fw = -(-hw[0] // s), -(-hw[1] // s)
        vh, vw = min(-(-pad_hw[0] // s), fh), min(-(-pad_hw[1] // s), fw)
        f = np.zeros((fh, fw), bool)
        f[:vh, :vw] = True
        flags.append(f.ravel())
    return flags


GRIDS = {'tiny': ((32, 48), (8, 16)), 'odd': ((56, 72), (8, 16, 32)), 'five': ((64, 256), (4, 8, 16, 32, 64))}


# ---------------------------------------------------------------------------------------------------------
# the guards: an fp64 restatement of the assignment
# ---------------------------------------------------------------------------------------------------------
def iou64(a, b):
    """(n, 4) against one box (4,), fp64, mmdet's formula"""
    area1, area2 = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]), (b[2] - b[0]) * (b[3] - b[1])
    w = np.clip(np.minimum(a[:, 2], b[2]) - np.maximum(a[:, 0], b[0]), 0, None)
    h = np.clip(np.minimum(a[:, 3], b[3]) - np.maximum(a[:, 1], b[1]), 0, None)
    return w * h / np.maximum(area1 + area2 - w * h, 1e-6)


def analyse(anchors, level_sizes, inside, gt):
    """-> (assigned (A,) int64, bad GT indices, candidate lists per GT, smallest margins) of one image"""
    a = anchors.astype(np.float64)
    gt = gt.astype(np.float64)
    A, G = len(a), len(gt)
    cx, cy = (a[:, 0] + a[:, 2]) / 2, (a[:, 1] + a[:, 3]) / 2
    claims = np.full((A, G), -np.inf)
    bad, cands = set(), []
    margins = dict(cut=np.inf, thr=np.inf, inset=np.inf, claim=np.inf)
    starts = np.concatenate([[0], np.cumsum(level_sizes)])
    for g in range(G):
        px, py = (gt[g, 4], gt[g, 5]) if gt.shape[1] == 6 else ((gt[g, 0] + gt[g, 2]) / 2, (gt[g, 1] + gt[g, 3]) / 2)
        d = np.sqrt((cx - px) ** 2 + (cy - py) ** 2)
        cand = []
        for l in range(len(level_sizes)):
            idx = np.arange(starts[l], starts[l + 1])[inside[starts[l]:starts[l + 1]]]
            k = min(TOPK, len(idx))
            order = idx[np.argsort(d[idx], kind='stable')]
            cand += order[:k].tolist()
            if len(idx) > k > 0:
                gap = d[order[k]] - d[order[k - 1]]
                margins['cut'] = min(margins['cut'], gap)
                if gap < CUT_GUARD:
                    bad.add(g)
        cand = np.asarray(cand, np.int64)
        cands.append(cand)
        if len(cand) <= 1:
            continue
        iou = iou64(a[cand], gt[g, :4])
        thr = iou.mean() + iou.std(ddof=1)
        inset = np.minimum(np.minimum(cx[cand] - gt[g, 0], cy[cand] - gt[g, 1]),
                           np.minimum(gt[g, 2] - cx[cand], gt[g, 3] - cy[cand]))
        m_thr, m_in = np.abs(iou - thr).min(), np.abs(inset - 0.01).min()
        margins['thr'], margins['inset'] = min(margins['thr'], m_thr), min(margins['inset'], m_in)
        if m_thr < GUARD or m_in < INSET_GUARD:
            bad.add(g)
        pos = (iou >= thr) & (inset > 0.01)
        claims[cand[pos], g] = iou[pos]
    assigned = np.zeros(A, np.int64)
    if G:
        assigned = np.where(np.isfinite(claims.max(1)), claims.argmax(1) + 1, 0).astype(np.int64)   # lowest index
    assigned[~inside] = -1
    if G > 1:
        order = np.sort(claims, 1)
        both = np.isfinite(order[:, -2])
        gap = order[both, -1] - order[both, -2]
        if gap.size and (gap > 0).any():
            margins['claim'] = min(margins['claim'], gap[gap > 0].min())
        near = both.copy()
        near[both] = (gap < GUARD) & (gap > 0)
        for i in np.nonzero(near)[0]:
            bad.add(int(np.argsort(claims[i], kind='stable')[-2:].max()))    # blame the later of the two
    return assigned, sorted(bad), cands, margins


def draw_gt(rng, hw, width):
    """a GT box in an image of hw.  In the two small images every anchor (128 px and up) contains any box that lies
    inside the image, so a level's overlaps would all be equal and nothing could pass mean + std: there the boxes
    are drawn larger than the image, as the projection of a close object is"""
    H, W = hw
    if W < 128:
        bw, bh = rng.uniform(2.0 * W, 4.0 * W), rng.uniform(2.0 * H, 5.0 * H)
        x1, y1 = rng.uniform(0.1 * W, 0.9 * W) - bw / 2, rng.uniform(0.1 * H, 0.9 * H) - bh / 2
    else:
        bw, bh = rng.uniform(max(12.0, 0.08 * W), 0.45 * W), rng.uniform(max(10.0, 0.2 * H), 0.8 * H)
        x1, y1 = rng.uniform(-0.1 * bw, W - 0.9 * bw), rng.uniform(-0.1 * bh, H - 0.9 * bh)
    box = [x1, y1, x1 + bw, y1 + bh]
    if width == 6:
        box += [x1 + bw * rng.uniform(0.3, 0.7), y1 + bh * rng.uniform(0.3, 0.7)]
    return np.asarray(box, np.float32)


def scene(rng, anchors, level_sizes, inside, hw, count, width=6, fixed=None):
    """GT boxes (fp32) and labels of one image; drawn boxes that violate a guard are redrawn, hand-placed never"""
    fixed = np.zeros((0, width), np.float32) if fixed is None else fixed
    if len(fixed) + count == 0:
        return np.zeros((0, width), np.float32), np.zeros(0, np.int64)
    gt = np.concatenate([fixed] + [draw_gt(rng, hw, width)[None] for _ in range(count)]).astype(np.float32)
    labels = rng.randint(0, NUM_CLASSES, len(gt)).astype(np.int64)
    for _ in range(500):
        bad = analyse(anchors, level_sizes, inside, gt)[1]
        if not bad:
            return gt, labels
        redraw = [i for i in bad if i >= len(fixed)]
        assert redraw, f'a hand-placed GT violates a guard: {bad}'
        for i in redraw:
            gt[i] = draw_gt(rng, hw, width)
    raise RuntimeError('no scene satisfies the guards')


# ---------------------------------------------------------------------------------------------------------
# the hand-placed GT boxes of the rules case
# ---------------------------------------------------------------------------------------------------------
def rules_gts(anchors, level_sizes):
    inside = np.ones(len(anchors), bool)
    off = [40.3, 20.2, 80.6, 50.4, 121.37, 29.81]                   # the point lies 40 px right of the box
    twin = [100.3, 10.2, 150.7, 44.9, 126.43, 26.57]
    small = [217.5, 49.3, 223.5, 55.3, 220.4, 52.3]               # holds one finest-level centre, (220, 52), and no
    first = [160.2, 8.3, 200.4, 40.1, 181.3, 25.2]                # centre of a coarser level
    for dx in np.arange(2.0, 14.0, 0.7):                          # claim: slide a larger box over the first one
        for dy in np.arange(0.5, 6.0, 0.7):
            second = [160.2 + dx, 8.3 + dy, 212.9 + dx, 47.6 + dy, 183.4 + dx, 26.1 + dy]
            gt = np.asarray([off, twin, twin, first, second, small], np.float32)
            assigned, bad, cands, _ = analyse(anchors, level_sizes, inside, gt)
            if bad:
                continue
            a64 = anchors.astype(np.float64)
            for i in np.nonzero(assigned == 5)[0]:                # won by the later box: did the first claim it too?
                if i not in cands[3]:
                    continue
                iou = iou64(a64[cands[3]], gt[3, :4].astype(np.float64))
                thr = iou.mean() + iou.std(ddof=1)
                mine = iou64(a64[i:i + 1], gt[3, :4].astype(np.float64))[0]
                cxy = ((a64[i, 0] + a64[i, 2]) / 2, (a64[i, 1] + a64[i, 3]) / 2)
                inset = min(cxy[0] - gt[3, 0], cxy[1] - gt[3, 1], gt[3, 2] - cxy[0], gt[3, 3] - cxy[1])
                if mine >= thr and inset > 0.01:
                    return gt, np.asarray([0, 1, 2, 0, 1, 2], np.int64), int(i)
    raise RuntimeError('no placement gives a doubly claimed anchor')


# ---------------------------------------------------------------------------------------------------------
def main():
    g = load_reference()
    rng = np.random.RandomState(2209)
    out, err = {}, dict(target=0.0, overlap=0.0)
    low = dict(cut=np.inf, thr=np.inf, inset=np.inf, claim=np.inf)

    def run(levels, valid, gts, labels, metas, dtype, **cfg):
        head = make_head(g, gts[0].shape[1], **cfg)
        B = len(gts)
        res = head.get_targets([[torch.from_numpy(l).to(dtype) for l in levels] for _ in range(B)],
                               [[torch.from_numpy(v) for v in valid[b]] for b in range(B)],
                               [torch.from_numpy(x).to(dtype) for x in gts], metas,
                               gt_labels_list=[torch.from_numpy(x) for x in labels])
        assert res is not None
        names = ('anchors_out', 'labels', 'label_weights', 'bbox_targets', 'bbox_weights')
        r = {n: torch.cat(v, 1).numpy() for n, v in zip(names, res[:5])}
        assign_results, pos_inds = head.seen
        flat = torch.cat([torch.from_numpy(l).to(dtype) for l in levels])
        inside = [anchor_inside_flags(flat, torch.cat([torch.from_numpy(v) for v in valid[b]]),
                                      metas[b]['img_shape'][:2], head.train_cfg.allowed_border) for b in range(B)]
        r['assigned_gt_inds'] = np.stack([unmap(ar.gt_inds, flat.shape[0], ins, fill=-1).numpy()
                                          for ar, ins in zip(assign_results, inside)])
        r['inside'] = np.stack([i.numpy() for i in inside]).astype(np.uint8)
        pos = r['assigned_gt_inds'] > 0
        r['counts'] = np.stack([pos.sum(1), (r['assigned_gt_inds'] == 0).sum(1)], 1).astype(np.int32)
        r['num_total_pos'], r['num_total_neg'] = np.int64(res[5]), np.int64(res[6])
        cent = [head.centerness_target(flat[pos[b]], torch.from_numpy(r['bbox_targets'][b][pos[b]]))
                for b in range(B) if pos[b].any()]
        r['centerness'] = torch.cat(cent).numpy() if cent else np.zeros(0, np.float64)
        return r

    def case(name, grid, gts, labels, valid=None, img_shapes=None, allowed_border=-1, pos_weight=-1):
        hw, strides = GRIDS[grid]
        levels = make_anchors(hw, strides)
        B = len(gts)
        valid = valid if valid is not None else [make_valid(hw, strides, hw) for _ in range(B)]
        metas = [dict(img_shape=(*(img_shapes[b] if img_shapes else hw), 3)) for b in range(B)]
        cfg = dict(allowed_border=allowed_border, pos_weight=pos_weight)
        r64 = run(levels, valid, gts, labels, metas, torch.float64, **cfg)
        r32 = run(levels, valid, gts, labels, metas, torch.float32, **cfg)
        for k in ('labels', 'label_weights', 'bbox_weights', 'assigned_gt_inds', 'counts', 'inside', 'num_total_pos',
                  'num_total_neg'):
            assert np.array_equal(r64[k], r32[k]), (name, k)
        err['target'] = max(err['target'], float(np.abs(r64['bbox_targets'] - r32['bbox_targets']).max()))
        flat, sizes = np.concatenate(levels), [len(l) for l in levels]
        for b in range(B):                                        # the guards, and the restatement agrees
            assigned, bad, cands, m = analyse(flat, sizes, r64['inside'][b] != 0, gts[b])
            assert not bad, (name, b, bad)
            assert np.array_equal(assigned, r64['assigned_gt_inds'][b]), (name, b)
            for k in low:
                low[k] = min(low[k], m[k])
            if name == 'tiny':
                out['tiny/candidates'] = np.stack(cands, 1).astype(np.int64)          # (N, G)
        assert np.array_equal(r64['counts'][:, 0], (r64['bbox_weights'][:, :, 0] > 0).sum(1))
        assert r64['labels'].dtype == np.int64 and r64['assigned_gt_inds'].dtype == np.int64
        out[f'{name}/anchors'] = flat
        out[f'{name}/level_sizes'] = np.asarray(sizes, np.int32)
        out[f'{name}/gt_boxes'] = np.concatenate(gts).astype(np.float32)
        out[f'{name}/gt_labels'] = np.concatenate(labels).astype(np.int64)
        out[f'{name}/gt_offsets'] = np.concatenate([[0], np.cumsum([len(x) for x in gts])]).astype(np.int32)
        out[f'{name}/valid_flags'] = np.stack([np.concatenate(v) for v in valid]).astype(np.uint8)
        out[f'{name}/img_shapes'] = np.asarray([m['img_shape'][:2] for m in metas], np.int32)
        out[f'{name}/allowed_border'] = np.int32(allowed_border)
        out[f'{name}/pos_weight'] = np.float64(pos_weight)
        for k, v in r64.items():
            out[f'{name}/{k}'] = v.astype(np.float32) if k in ('label_weights', 'bbox_weights') else v
        print(f'  {name}: A = {len(flat)}, G = {[len(x) for x in gts]}, counts {r64["counts"].tolist()}, '
              f'counting {(r64["inside"] != 0).sum(1).tolist()}')
        return r64

    def drawn(grid, counts, width=6, valid=None, img_shapes=None, allowed_border=-1, areas=None):
        hw, strides = GRIDS[grid]
        levels = make_anchors(hw, strides)
        flat, sizes = np.concatenate(levels), [len(l) for l in levels]
        gts, labels = [], []
        for b, n in enumerate(counts):
            v = np.concatenate(valid[b]) if valid is not None else np.ones(len(flat), bool)
            shape = img_shapes[b] if img_shapes else hw
            inside = anchor_inside_flags(torch.from_numpy(flat), torch.from_numpy(v), shape, allowed_border).numpy()
            for _ in range(200):                                  # an image with GT boxes has a positive
                gt, lb = scene(rng, flat, sizes, inside, areas[b] if areas else hw, n, width)
                if n == 0 or (analyse(flat, sizes, inside, gt)[0] > 0).any():
                    break
            else:
                raise RuntimeError('no scene with a positive')
            gts.append(gt)
            labels.append(lb)
        return gts, labels

    gts, lbs = drawn('tiny', [3])
    r = case('tiny', 'tiny', gts, lbs)
    assert r['counts'][0, 0] > 0
    r2 = case('posw', 'tiny', gts, lbs, pos_weight=2)
    assert set(np.unique(r2['label_weights']).tolist()) == {1.0, 2.0}
    r = case('odd', 'odd', *drawn('odd', [5]))
    assert r['counts'][0, 0] > 0
    r = case('five', 'five', *drawn('five', [12, 5]))
    assert np.all(r['counts'][:, 0] > 0)
    r = case('empty', 'five', *drawn('five', [6, 0]))
    assert r['counts'][1].tolist() == [0, 1364]
    case('g70', 'five', *drawn('five', [70]))
    hw, strides = GRIDS['five']
    valid = [make_valid(hw, strides, (64, 192)), make_valid(hw, strides, (64, 256))]
    shapes = [(60, 250), (64, 256)]
    kw = dict(valid=valid, img_shapes=shapes, allowed_border=16)
    r = case('border', 'five', *drawn('five', [6, 6], areas=[(60, 192), (64, 256)], **kw), **kw)
    counting = (r['inside'] != 0)
    assert not np.array_equal(counting[0], counting[1]) and 0 < counting[0, :1024].sum() < counting[1, :1024].sum()
    assert counting[:, 1024:].sum() == 0 and np.all(r['counts'][:, 0] > 0)
    kw = dict(valid=valid, img_shapes=shapes, allowed_border=-1)
    r = case('valid', 'five', *drawn('five', [6, 6], areas=[(60, 192), (64, 256)], **kw), **kw)
    assert (r['inside'][0, 1360:] != 0).sum() == 3 and np.all(r['counts'][:, 0] > 0)
    r = case('centre4', 'five', *drawn('five', [6], width=4))
    assert r['counts'][0, 0] > 0
    levels = make_anchors(hw, strides)
    gt, lb, claimed = rules_gts(np.concatenate(levels), [len(l) for l in levels])
    r = case('rules', 'five', [gt], [lb])
    out['rules/claim_anchor'] = np.int64(claimed)
    a = r['assigned_gt_inds'][0]
    assert not (a == 1).any() and (a == 2).any() and not (a == 3).any()            # off; twin: the lower index
    assert a[claimed] == 5 and (a == 4).any()                                      # claim: the later box wins it
    assert (a == 6).any() and np.nonzero(a == 6)[0].max() < 1024                   # small: the finest level only

    # standalone overlaps: a random 130 x 37 set and eight hand-computed pairs
    def boxes(n):
        x1, y1 = rng.uniform(0, 200, n), rng.uniform(0, 50, n)
        return np.stack([x1, y1, x1 + rng.uniform(4, 80, n), y1 + rng.uniform(4, 40, n)], 1).astype(np.float32)
    b1 = boxes(130)
    b2 = (b1[:37] + rng.uniform(-6, 6, (37, 4))).astype(np.float32)
    hand1 = np.asarray([[0, 0, 2, 2], [0, 0, 2, 2], [0, 0, 4, 4], [1, 1, 3, 3], [0, 0, 2, 2], [0, 0, 0, 0],
                        [0, 0, 2, 2], [0, 0, 2, 2]], np.float32)
    hand2 = np.asarray([[1, 0, 3, 2], [0, 1, 2, 3], [1, 1, 3, 3], [0, 0, 4, 4], [5, 5, 6, 6], [0, 0, 0, 0],
                        [0, 0, 2, 2], [1, 1, 3, 3]], np.float32)
    for tag, x, y in (('overlaps', b1, b2), ('hand', hand1, hand2)):
        out[f'{tag}/boxes1'], out[f'{tag}/boxes2'] = x, y
        n = len(y)
        for key, kw, xs in (('iou', dict(mode='iou'), x), ('iof', dict(mode='iof'), x),
                            ('aligned_iou', dict(mode='iou', is_aligned=True), x[:n]),
                            ('aligned_iof', dict(mode='iof', is_aligned=True), x[:n])):
            v64 = bbox_overlaps(torch.from_numpy(xs).double(), torch.from_numpy(y).double(), **kw)
            v32 = bbox_overlaps(torch.from_numpy(xs), torch.from_numpy(y), **kw)
            err['overlap'] = max(err['overlap'], float((v64 - v32.double()).abs().max()))
            out[f'{tag}/{key}'] = v64.numpy()
    print('  hand iou', np.round(out['hand/aligned_iou'], 6).tolist(), 'iof', np.round(out['hand/aligned_iof'], 6).tolist())
    print('smallest margins', {k: float(v) for k, v in low.items()})
    assert low['cut'] >= CUT_GUARD and low['thr'] >= GUARD and low['inset'] >= INSET_GUARD and low['claim'] >= GUARD
    print('fp32_overlap_error', err['overlap'], 'fp32_target_error', err['target'])
    out.update(fp32_overlap_error=np.float64(err['overlap']), fp32_target_error=np.float64(err['target']),
               guard=np.float64(GUARD), cut_guard=np.float64(CUT_GUARD), inset_guard=np.float64(INSET_GUARD),
               topk=np.int32(TOPK), num_classes=np.int32(NUM_CLASSES), target_means=np.asarray(MEANS),
               target_stds=np.asarray(STDS), **{f'margin_{k}': np.float64(v) for k, v in low.items()})
    path = os.path.join(HERE, 'atss_target.npz')
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 512 * 1024


if __name__ == '__main__':
    if not os.path.isdir(mg.REF):
        sys.exit('reference not mounted; the fixture is committed, nothing to do')
    torch.set_num_threads(1)
    main()
