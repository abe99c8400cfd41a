"""Generate tests/golden/box_nms.npz: BEV non-maximum suppression and rotated-box IoU.

Run in the build container only (needs the reference checkout):   python tests/golden/make_golden_box_nms.py

Executed unmodified, lifted from core/post_processing/box3d_nms.py by AST as make_golden.py does (the file
itself cannot be imported: it needs numba and mmcv.ops): ``box3d_multiclass_nms``, ``nms_bev`` and
``nms_normal_bev``.  Nothing of the reference is stored, only inputs and the outputs it produced.

STAND-INS: ``mmcv.ops.nms_rotated`` and ``mmcv.ops.nms`` are CUDA ops of a package that is not installed.  The
functions of those names below are fp64 numpy restatements of the semantics include/dfm_hip.h states: exact IoU
by convex clipping (axis-aligned IoU without +1 for ``nms``), candidates visited in descending score order
(stable), a candidate dropped when an earlier kept one has IoU strictly greater than the threshold, indices
returned in that order.  The IoU function is written once and run in fp64 (the expected values) and in numpy
float32 (to measure what fp32 arithmetic costs); it follows the kernel's algorithm step by step (midpoint
translation, centre-distance rejection, Sutherland-Hodgman in the first box's axes, shoelace) and is checked
against hand-computed overlaps in tests/test_box_nms.py.

Decidability in fp32: a scene is accepted only when no pair of its boxes has an fp64 IoU (rotated or axis-
aligned) within GUARD_BAND of a threshold the scene is used with; boxes of offending pairs are moved and the
scene checked again.  ``fp32_iou_error`` is the largest |fp64 - float32| IoU over every pair of every scene, in
both argument orders, and of the stored IoU matrix; the generator asserts GUARD_BAND >= 4 * fp32_iou_error and
stores both numbers.

Scenes (boxes (N, 5) = x1, y1, x2, y2, ry in fp32; scores (N, C + 1), all distinct):
  dense      N=4096 C=3   KITTI-like clusters with dense overlaps (config K: nms_thr 0.25, score_thr 0.1,
                          max_num 500; and max_num 50, which cuts)
  sparse     N=300  C=3   few overlaps; class 1 has no candidate above score_thr; pre / post_max_size cuts
  n65        N=65   C=1   one chain of overlapping boxes: suppression crosses the 64-bit word boundary
  n1 / n0    N=1 / 0
  special    N=48   C=2   identical boxes, zero-area boxes, edge-touching boxes, boxes at +-75 m
Per scene: ``keep_rot`` / ``keep_aligned`` = nms_bev / nms_normal_bev on class 0's scores (all N boxes);
``mc_rot_*`` / ``mc_aligned_*`` = box3d_multiclass_nms with mlvl_bboxes = the row index, so that the returned
boxes ARE the kept indices, plus the labels.  ``iou_boxes1/2`` (cx, cy, w, h, angle) and ``iou`` (fp64 matrix).
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402

GUARD_BAND = 1e-4
NMS_THR = 0.25


# ---------------------------------------------------------------------------------------------------------
# the IoU, once, in any float dtype
# ---------------------------------------------------------------------------------------------------------
def _push(qx, qy, n, px, py, emit, nout):
    """append (px, py) to the FRONT of the first nout slots where emit"""
    e = emit[:, None]
    qx[:, 1:nout] = np.where(e, qx[:, 0:nout - 1], qx[:, 1:nout])
    qy[:, 1:nout] = np.where(e, qy[:, 0:nout - 1], qy[:, 1:nout])
    qx[:, 0] = np.where(emit, px, qx[:, 0])
    qy[:, 0] = np.where(emit, py, qy[:, 0])
    n += emit


def _clip(px, py, n, sx, sy, off, nin):
    """clip to off - (sx x + sy y) >= 0: at most nin vertices in, nin + 1 out"""
    d = off[:, None] - (sx * px[:, :nin] + sy * py[:, :nin])
    qx, qy = np.zeros_like(px), np.zeros_like(py)
    m = np.zeros_like(n)
    for i in range(nin):
        act = i < n
        wrap = (i + 1 == n) | (i + 1 == nin)
        i1 = i + 1 if i + 1 < nin else 0
        xn = np.where(wrap, px[:, 0], px[:, i1])
        yn = np.where(wrap, py[:, 0], py[:, i1])
        dn = np.where(wrap, d[:, 0], d[:, i1])
        in_c, in_n = d[:, i] >= 0, dn >= 0
        _push(qx, qy, m, px[:, i], py[:, i], act & in_c, nin + 1)
        t = d[:, i] / (d[:, i] - dn)
        ix = px[:, i] + t * (xn - px[:, i])
        iy = py[:, i] + t * (yn - py[:, i])
        _push(qx, qy, m, ix, iy, act & (in_c != in_n), nin + 1)
    return qx, qy, m


def rbox_iou(a, b, dtype=np.float64):
    """IoU of rotated boxes a[k], b[k] ((P, 5) = cx, cy, w, h, angle), evaluated in ``dtype``"""
    a, b = np.asarray(a).astype(dtype), np.asarray(b).astype(dtype)
    half, eps = dtype(0.5), dtype(1e-14)
    out = np.zeros(a.shape[0], dtype)
    area_a, area_b = a[:, 2] * a[:, 3], b[:, 2] * b[:, 3]
    mx, my = (a[:, 0] + b[:, 0]) * half, (a[:, 1] + b[:, 1]) * half
    ax, ay, bx, by = a[:, 0] - mx, a[:, 1] - my, b[:, 0] - mx, b[:, 1] - my
    ddx, ddy = bx - ax, by - ay
    r = half * np.sqrt(a[:, 2] * a[:, 2] + a[:, 3] * a[:, 3]) + half * np.sqrt(b[:, 2] * b[:, 2] + b[:, 3] * b[:, 3])
    go = ~((area_a < eps) | (area_b < eps)) & ~(ddx * ddx + ddy * ddy > r * r)
    if not go.any():
        return out
    a, b, ax, ay, bx, by = a[go], b[go], ax[go], ay[go], bx[go], by[go]
    ca, sa, cb, sb = np.cos(a[:, 4]), np.sin(a[:, 4]), np.cos(b[:, 4]), np.sin(b[:, 4])
    hwb, hhb = b[:, 2] * half, b[:, 3] * half
    P = a.shape[0]
    px, py = np.zeros((P, 8), dtype), np.zeros((P, 8), dtype)
    for k in range(4):
        lx = hwb if k in (0, 3) else -hwb
        ly = hhb if k < 2 else -hhb
        wx = bx + (lx * cb - ly * sb)
        wy = by + (lx * sb + ly * cb)
        ux, uy = wx - ax, wy - ay
        px[:, k] = ux * ca + uy * sa
        py[:, k] = uy * ca - ux * sa
    n = np.full(P, 4, np.int64)
    hwa, hha = a[:, 2] * half, a[:, 3] * half
    one, zero = dtype(1), dtype(0)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        px, py, n = _clip(px, py, n, one, zero, hwa, 4)
        px, py, n = _clip(px, py, n, -one, zero, hwa, 5)
        px, py, n = _clip(px, py, n, zero, one, hha, 6)
        px, py, n = _clip(px, py, n, zero, -one, hha, 7)
    acc = np.zeros(P, dtype)
    for i in range(8):
        wrap = (i + 1 == n) | (i + 1 == 8)
        i1 = i + 1 if i + 1 < 8 else 0
        xn = np.where(wrap, px[:, 0], px[:, i1])
        yn = np.where(wrap, py[:, 0], py[:, i1])
        acc = acc + np.where(i < n, px[:, i] * yn - xn * py[:, i], zero)
    inter = half * np.abs(acc)
    out[go] = inter / (a[:, 2] * a[:, 3] + b[:, 2] * b[:, 3] - inter)
    return out


def abox_iou(a, b, dtype=np.float64):
    """IoU of axis-aligned boxes a[k], b[k] ((P, >=4) = x1, y1, x2, y2), no +1 offset"""
    a, b = np.asarray(a).astype(dtype), np.asarray(b).astype(dtype)
    area_a, area_b = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]), (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    iw = np.maximum(np.minimum(a[:, 2], b[:, 2]) - np.maximum(a[:, 0], b[:, 0]), 0)
    ih = np.maximum(np.minimum(a[:, 3], b[:, 3]) - np.maximum(a[:, 1], b[:, 1]), 0)
    inter = iw * ih
    with np.errstate(divide='ignore', invalid='ignore'):
        iou = inter / (area_a + area_b - inter)
    return np.where((area_a < 1e-14) | (area_b < 1e-14), 0, iou).astype(dtype)


def near_pairs(b1, b2, rotated, upper):
    """index pairs whose IoU can be non-zero (a superset; every other pair is exactly 0 in any dtype)"""
    b1, b2 = np.asarray(b1, np.float64), np.asarray(b2, np.float64)
    if rotated:
        r1, r2 = 0.5 * np.hypot(b1[:, 2], b1[:, 3]), 0.5 * np.hypot(b2[:, 2], b2[:, 3])
        d = np.hypot(b1[:, None, 0] - b2[None, :, 0], b1[:, None, 1] - b2[None, :, 1])
        near = d <= 1.01 * (r1[:, None] + r2[None, :]) + 1e-6
    else:
        near = (np.minimum(b1[:, None, 2], b2[None, :, 2]) >= np.maximum(b1[:, None, 0], b2[None, :, 0])) & \
               (np.minimum(b1[:, None, 3], b2[None, :, 3]) >= np.maximum(b1[:, None, 1], b2[None, :, 1]))
    if upper:
        near = np.triu(near, 1)
    return np.nonzero(near)


def iou_matrix(b1, b2, rotated, dtype=np.float64, upper=False):
    """(N, M) IoU; with ``upper`` only the entries j > i (the rest 0)"""
    i, j = near_pairs(b1, b2, rotated, upper)
    out = np.zeros((len(b1), len(b2)), dtype)
    fn = rbox_iou if rotated else abox_iou
    out[i, j] = fn(np.asarray(b1)[i], np.asarray(b2)[j], dtype)
    return out


def greedy(iou_upper, thr):
    """keep list over candidates already in visiting order; iou_upper[i, j] for j > i"""
    n = iou_upper.shape[0]
    removed = np.zeros(n, bool)
    keep = []
    for i in range(n):
        if removed[i]:
            continue
        keep.append(i)
        removed[i + 1:] |= iou_upper[i, i + 1:] > thr
    return np.asarray(keep, np.int64)


def _stand_in(boxes, scores, thr, rotated):
    order = torch.sort(scores, dim=0, descending=True, stable=True)[1]
    b = boxes[order].double().numpy()
    keep = order[torch.from_numpy(greedy(iou_matrix(b, b, rotated, upper=True), thr))]
    return torch.cat([boxes[keep], scores[keep, None]], dim=1), keep


def nms_rotated(boxes, scores, iou_threshold, labels=None):
    """fp64 STAND-IN for mmcv.ops.nms_rotated (see the module docstring): boxes (n, 5) = cx, cy, w, h, angle"""
    return _stand_in(boxes, scores, iou_threshold, True)


def nms(boxes, scores, iou_threshold, offset=0):
    """fp64 STAND-IN for mmcv.ops.nms: boxes (n, 4) = x1, y1, x2, y2, offset 0"""
    assert offset == 0
    return _stand_in(boxes, scores, iou_threshold, False)


# ---------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------
def to_xywhr(bev):
    """nms_bev's conversion (box3d_nms.py:259-262) in the dtype of ``bev`` (fp32)"""
    return np.stack([(bev[:, 0] + bev[:, 2]) / 2, (bev[:, 1] + bev[:, 3]) / 2, bev[:, 2] - bev[:, 0],
                     bev[:, 3] - bev[:, 1], bev[:, 4]], axis=-1)


def to_xyxyr(xywhr):
    x, y, w, h, r = (xywhr[:, i] for i in range(5))
    return np.stack([x - w / 2, y - h / 2, x + w / 2, y + h / 2, r], axis=-1).astype(np.float32)


def distinct_scores(rng, n, cols):
    """(n, cols) fp32 in (0, 1), distinct over the WHOLE matrix: box3d_multiclass_nms's max_num cut sorts the
    kept scores of all classes together, and ties have no defined order"""
    s = ((rng.permutation(n * cols) + 0.5) / max(n * cols, 1)).astype(np.float32).reshape(n, cols)
    assert len(np.unique(s)) == n * cols
    return s


SIZES = np.array([[3.9, 1.6], [0.8, 0.6], [1.76, 0.6]])


def clustered(rng, n, clusters, spread):
    centres = np.stack([rng.uniform(2, 68, clusters), rng.uniform(-38, 38, clusters)], axis=1)
    yaw = rng.uniform(-np.pi, np.pi, clusters)
    kind = rng.randint(0, 3, clusters)
    which = np.sort(rng.randint(0, clusters, n))
    xy = centres[which] + rng.normal(0, spread, (n, 2))
    wh = SIZES[kind[which]] * rng.uniform(0.8, 1.25, (n, 2))
    r = yaw[which] + rng.normal(0, 0.15, n) + (rng.rand(n) < 0.2) * np.pi / 2
    return to_xyxyr(np.concatenate([xy, wh, r[:, None]], axis=1))


def in_band(bev, thresholds):
    """boxes that take part in a pair whose fp64 IoU lies within GUARD_BAND of a threshold"""
    bad = set()
    for rotated, b in ((True, to_xywhr(bev)), (False, bev)):
        i, j = near_pairs(b, b, rotated, True)
        v = (rbox_iou if rotated else abox_iou)(b[i], b[j])
        for thr in thresholds:
            hit = np.abs(v - thr) <= GUARD_BAND
            bad.update(j[hit].tolist())
    return sorted(bad)


def settle(rng, bev, thresholds, movable=None):
    for _ in range(200):
        bad = in_band(bev, thresholds)
        if not bad:
            return bev
        if movable is not None and not set(bad) <= movable:
            raise RuntimeError('a fixed box is within the guard band')
        print('   ', len(bad), 'boxes within the guard band: moved')
        for k in bad:
            d = rng.uniform(-0.25, 0.25, 2).astype(np.float32)
            bev[k, [0, 2]] += d[0]
            bev[k, [1, 3]] += d[1]
    raise RuntimeError('no decidable scene')


def fp32_error(bev):
    """largest |fp64 - fp32| IoU over every pair of the scene, both argument orders, both IoU kinds"""
    worst = 0.0
    for rotated, b in ((True, to_xywhr(bev)), (False, bev)):
        fn = rbox_iou if rotated else abox_iou
        i, j = near_pairs(b, b, rotated, False)
        if len(i):
            worst = max(worst, float(np.abs(fn(b[i], b[j]) - fn(b[i], b[j], np.float32)).max()))
    return worst


def special_boxes():
    rows = []
    rows += [[10, 5, 4, 2, 0.3]] * 6                                   # identical
    rows += [[20, -5, 0, 2, 0.1], [20, -5, 3, 0, 0.1], [20.2, -5, 3.9, 1.6, 0.1], [20.4, -5.1, 3.9, 1.6, 0.1],
             [30, 0, 0, 0, 0]]                                         # zero area beside real boxes
    for k in range(6):                                                 # edge-touching, axis-aligned: a row
        rows.append([40 + 2 * k, 10, 2, 2, 0])
    for k in range(5):                                                 # edge-touching, rotated by 90 degrees
        rows.append([40 + 4 * k, 20, 2, 4, np.pi / 2])
    for sx in (-1, 1):                                                 # +-75 m
        for sy in (-1, 1):
            for k in range(6):
                rows.append([sx * 75 - 0.35 * k, sy * 75 + 0.2 * k, 3.9, 1.6, 0.4 * k])
    rows += [[0, 0, 4, 4, np.pi / 4], [0, 0, 4, 4, 0]]                 # the octagon
    return np.asarray(rows, np.float64)


def run_scene(g, name, bev, scores, score_thr, max_nums, extra=None):
    out = {f'{name}/boxes': bev, f'{name}/scores': scores, f'{name}/score_thr': np.float32(score_thr)}
    tb, ts = torch.from_numpy(bev), torch.from_numpy(scores)
    n = bev.shape[0]
    if n:
        out[f'{name}/keep_rot'] = g['nms_bev'](tb, ts[:, 0], NMS_THR).numpy()
        out[f'{name}/keep_aligned'] = g['nms_normal_bev'](tb, ts[:, 0], NMS_THR).numpy()
        for key, (pre, post) in (extra or {}).items():
            out[f'{name}/{key}'] = g['nms_bev'](tb, ts[:, 0], NMS_THR, pre, post).numpy()
    index = torch.arange(n, dtype=torch.float32)[:, None]
    for rot, tag in ((True, 'rot'), (False, 'aligned')):
        cfg = SimpleNamespace(use_rotate_nms=rot, nms_thr=NMS_THR)
        for max_num in max_nums:
            b, s, lab = g['box3d_multiclass_nms'](index, tb, ts, score_thr, max_num, cfg)
            idx = b[:, 0].long()
            assert torch.equal(s, ts[idx, lab])
            out[f'{name}/mc_{tag}_{max_num}_idx'] = idx.numpy()
            out[f'{name}/mc_{tag}_{max_num}_labels'] = lab.numpy()
            print(f'  {name}: multiclass {tag} max_num {max_num}: {len(idx)} kept,', 'per class',
                  np.bincount(lab.numpy(), minlength=scores.shape[1] - 1).tolist())
    return out


def main():
    g = {'torch': torch, 'nms_rotated': nms_rotated, 'nms': nms}
    mg.extract(mg.REF + 'core/post_processing/box3d_nms.py', ['box3d_multiclass_nms', 'nms_bev', 'nms_normal_bev'], g)
    rng = np.random.RandomState(4096)
    out, worst = {}, 0.0
    thr = [NMS_THR]

    print('dense')
    dense = settle(rng, clustered(rng, 4096, 160, 0.7), thr)
    out.update(run_scene(g, 'dense', dense, distinct_scores(rng, 4096, 4), 0.1, (500, 50)))
    worst = max(worst, fp32_error(dense))

    print('sparse')
    sparse = settle(rng, clustered(rng, 300, 150, 0.5), thr)
    s = distinct_scores(rng, 300, 4)
    s[:, 1] *= 0.09                                                    # class 1: nothing above score_thr 0.1
    assert len(np.unique(s)) == s.size
    out.update(run_scene(g, 'sparse', sparse, s, 0.1, (500, 20), extra={'keep_rot_pre100_post10': (100, 10),
                                                                         'keep_rot_pre100': (100, None),
                                                                         'keep_rot_post5': (None, 5)}))
    worst = max(worst, fp32_error(sparse))

    print('n65')
    chain = np.zeros((65, 5))
    chain[:, 0] = 10 + 1.1 * np.arange(65)                             # neighbours overlap well above 0.25
    chain[:, 1] = 3
    chain[:, 2:4] = [3.9, 1.6]
    chain[:, 4] = 0.05 * np.arange(65) % 0.4
    n65 = settle(rng, to_xyxyr(chain), thr)
    s = np.zeros((65, 2), np.float32)
    s[:, 0] = (65 - np.arange(65)) / 128.0                             # exact in bf16 as well; chain order
    out.update(run_scene(g, 'n65', n65, s, 0.0, (500,)))
    worst = max(worst, fp32_error(n65))

    print('n1 / n0')
    out.update(run_scene(g, 'n1', to_xyxyr(np.array([[5.0, 1, 3.9, 1.6, 0.7]])), np.array([[0.6, 0]], np.float32),
                         0.1, (500,)))
    out.update(run_scene(g, 'n0', np.zeros((0, 5), np.float32), np.zeros((0, 4), np.float32), 0.1, (500,)))

    print('special')
    sp = special_boxes()
    special = to_xyxyr(sp)
    assert not in_band(special, thr), 'the special boxes must be decidable as they are'
    out.update(run_scene(g, 'special', special, distinct_scores(rng, len(sp), 3), 0.1, (500,)))
    worst = max(worst, fp32_error(special))

    # the IoU matrix: the head of the dense scene (whole clusters) and the special boxes, against a shifted window
    b1 = np.concatenate([to_xywhr(dense[:150]), sp.astype(np.float32)]).astype(np.float32)
    b2 = np.concatenate([sp.astype(np.float32), to_xywhr(dense[40:170])]).astype(np.float32)
    iou = iou_matrix(b1, b2, True)
    worst = max(worst, float(np.abs(iou - iou_matrix(b1, b2, True, np.float32)).max()))
    out.update(iou_boxes1=b1, iou_boxes2=b2, iou=iou)
    print('IoU matrix', iou.shape, 'non-zero', int((iou > 0).sum()), 'max', iou.max())

    print('fp32_iou_error', worst, 'guard band', GUARD_BAND)
    assert GUARD_BAND >= 4 * worst, (GUARD_BAND, worst)
    out.update(fp32_iou_error=np.float64(worst), guard_band=np.float64(GUARD_BAND), nms_thr=np.float32(NMS_THR))
    path = os.path.join(HERE, 'box_nms.npz')
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    if not os.path.isdir(mg.REF):
        sys.exit('reference not mounted; the fixture is committed, nothing to do')
    torch.set_num_threads(1)
    main()
