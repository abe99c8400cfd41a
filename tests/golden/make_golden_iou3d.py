"""Generate tests/golden/iou3d.npz: the differentiable rotated 3-D IoU and IOU3DLoss.

Run in the build container only (needs the reference checkout):   python tests/golden/make_golden_iou3d.py

Executed unmodified, lifted by AST as make_golden.py does (the files cannot be imported: they need mmcv / mmdet):
``iou3d_loss`` and ``IOU3DLoss`` (models/losses/iou3d_loss.py) and ``DeltaXYZWLHRBBoxCoder.decode``
(core/bbox/coders/delta_xyzwhlr_bbox_coder.py:58-91).  Nothing of the reference is stored, only inputs and the
outputs it produced.

STAND-INS for the two symbols of packages that are not installed:
  * ``weighted_loss`` (mmdet/models/losses/utils.py): the decorator that adds ``weight``, ``reduction`` and
    ``avg_factor`` to an element-wise loss -- multiply by the weight; without ``avg_factor`` reduce by 'none' |
    'mean' | 'sum'; with it 'mean' is ``loss.sum() / avg_factor`` (an exact division, no epsilon), 'none' is
    untouched and 'sum' raises ValueError.
  * ``mmcv.ops.diff_iou_rotated_3d``: ``diff_iou_rotated_3d`` below, a torch restatement of the semantics
    include/dfm_hip.h states -- box (x, y, z, dx, dy, dz, yaw), BEV rectangle centre (x, y) size (dx, dy) turned
    counter-clockwise by yaw, z interval [z - dz/2, z + dz/2], IoU3D = I Z / (V1 + V2 - I Z) with I the exact
    area of the rectangles' intersection, Z = max(0, min zmax - max zmin), V = dx dy dz; 0 (and zero gradient)
    when a BEV area or a volume is below 1e-14 or I or Z is 0.  It is written once for any dtype (both boxes
    relative to the midpoint of their centres, Sutherland-Hodgman in the first box's axes, shoelace, as the
    box-NMS stand-in) and differentiated by autograd.  Run in fp64 it gives the expected values and gradients;
    run in fp32 on the CPU it measures what fp32 arithmetic costs.  The fp64 gradient is checked here against
    central differences (step 1e-6, agreement asserted at 1e-7) and the values against hand-computed overlaps
    in tests/test_iou3d_loss.py.

The reference's ``iou3d_loss`` opens with ``assert target.numel() > 0``, which makes its own ``P == 0`` branch
unreachable (LIGAAnchor3DHead.loss_single calls it for an image without positives all the same).  The P = 0 case
stored here is what that branch's expression ``(pred - target).sum(1) * 0.`` gives under the reduction; the
generator asserts that the reference raises there.

Error figures, stored next to the data and read by the GPU tests (nothing is written into a test):
  fp32_iou_error / fp32_grad_error            largest |fp64 - fp32| of the stand-in's IoU / of any gradient
                                              component over every pair of every scene (general, aligned, special,
                                              the decoded pairs of the head cases)
  fp32_head_loss_error / fp32_head_grad_error the same for decode + loss from fp32 deltas (per-row loss; gradient
                                              with respect to bbox_pred), where fp32 rounds the decoded centres

General position.  The gradient is undefined on a set of measure zero; a pair whose gradient is stored is
accepted only when every corner of each rectangle is at least GUARD = 1e-3 m from every edge line of the other
(parallel edges are then that far apart as well), and both top faces, both bottom faces and Z itself are at least
GUARD apart / away from 0.  Offending second boxes are moved and the pair checked again; no pair is dropped.

Scenes (boxes fp32):
  general  1024 pairs  KITTI-sized, centres to +-75 m, every yaw quadrant, ~90 % overlapping
  aligned    64 pairs  equal yaw
  special  values only: identical, contained, z-disjoint, BEV-disjoint, zero-size, edge-touching, the hand cases
  head     R = 600 anchors of config K's three classes (two rotations); targets encode boxes near the anchors,
           predictions are the targets plus noise.  Cases p257, p1, p0, nan (p257's rows with one NaN target
           component: yaw, z or the width delta in turn).  Per case: pos_inds, the decoded fp32 boxes, the
           reference's per-row loss, its reduced loss with a tensor avg_factor, the gradients of both with
           respect to bbox_pred (the per-row one through the stored row weights); and for p257 / nan the
           IOU3DLoss results on the decoded fp32 boxes (every reduction, weight, float / tensor avg_factor,
           gradients to pred and target).
"""
import ast
import functools
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402

GUARD = 1e-3
EPS = 1e-14


# ---------------------------------------------------------------------------------------------------------
# the IoU, once, in any float dtype, differentiable
# ---------------------------------------------------------------------------------------------------------
def _push(qx, qy, n, px, py, emit):
    """(px, py) appended to the FRONT of the vertex list where emit"""
    e = emit[:, None]
    qx = torch.where(e, torch.cat([px[:, None], qx[:, :-1]], 1), qx)
    qy = torch.where(e, torch.cat([py[:, None], qy[:, :-1]], 1), qy)
    return qx, qy, n + emit.long()


def _clip(px, py, n, sx, sy, off, nin):
    """clip to off - (sx x + sy y) >= 0: at most nin vertices in, nin + 1 out"""
    d = off[:, None] - (sx * px[:, :nin] + sy * py[:, :nin])
    qx, qy, m = torch.zeros_like(px), torch.zeros_like(py), torch.zeros_like(n)
    for i in range(nin):
        act = i < n
        wrap = (i + 1 == n) | (i + 1 == nin)
        i1 = i + 1 if i + 1 < nin else 0
        xn = torch.where(wrap, px[:, 0], px[:, i1])
        yn = torch.where(wrap, py[:, 0], py[:, i1])
        dn = torch.where(wrap, d[:, 0], d[:, i1])
        in_c, in_n = d[:, i] >= 0, dn >= 0
        qx, qy, m = _push(qx, qy, m, px[:, i], py[:, i], act & in_c)
        cross = act & (in_c != in_n)
        t = d[:, i] / torch.where(cross, d[:, i] - dn, torch.ones_like(dn))    # (no 0 / 0 in a masked row)
        qx, qy, m = _push(qx, qy, m, px[:, i] + t * (xn - px[:, i]), py[:, i] + t * (yn - py[:, i]), cross)
    return qx, qy, m


def bev_intersection(a, b):
    """area of the intersection of the rectangles a[k], b[k] ((P, 5) = cx, cy, w, h, angle), in their dtype"""
    half = 0.5
    mx, my = (a[:, 0] + b[:, 0]) * half, (a[:, 1] + b[:, 1]) * half
    ax, ay, bx, by = a[:, 0] - mx, a[:, 1] - my, b[:, 0] - mx, b[:, 1] - my
    ddx, ddy = bx - ax, by - ay
    r = half * torch.sqrt(a[:, 2] * a[:, 2] + a[:, 3] * a[:, 3]) + \
        half * torch.sqrt(b[:, 2] * b[:, 2] + b[:, 3] * b[:, 3])
    near = ~(ddx * ddx + ddy * ddy > r * r)
    ca, sa, cb, sb = torch.cos(a[:, 4]), torch.sin(a[:, 4]), torch.cos(b[:, 4]), torch.sin(b[:, 4])
    hwb, hhb = b[:, 2] * half, b[:, 3] * half
    xs, ys = [], []
    for k in range(4):
        lx = hwb if k in (0, 3) else -hwb
        ly = hhb if k < 2 else -hhb
        wx = bx + (lx * cb - ly * sb)
        wy = by + (lx * sb + ly * cb)
        ux, uy = wx - ax, wy - ay
        xs.append(ux * ca + uy * sa)
        ys.append(uy * ca - ux * sa)
    zero = torch.zeros_like(ax)
    px, py = torch.stack(xs + [zero] * 4, 1), torch.stack(ys + [zero] * 4, 1)
    n = torch.full((a.shape[0],), 4, dtype=torch.long, device=a.device)
    hwa, hha = a[:, 2] * half, a[:, 3] * half
    px, py, n = _clip(px, py, n, 1.0, 0.0, hwa, 4)
    px, py, n = _clip(px, py, n, -1.0, 0.0, hwa, 5)
    px, py, n = _clip(px, py, n, 0.0, 1.0, hha, 6)
    px, py, n = _clip(px, py, n, 0.0, -1.0, hha, 7)
    acc = zero
    for i in range(8):
        wrap = (i + 1 == n) | (i + 1 == 8)
        i1 = i + 1 if i + 1 < 8 else 0
        xn = torch.where(wrap, px[:, 0], px[:, i1])
        yn = torch.where(wrap, py[:, 0], py[:, i1])
        acc = acc + torch.where(i < n, px[:, i] * yn - xn * py[:, i], zero)
    return torch.where(near, half * acc.abs(), zero)


def iou3d_pairs(a, b):
    """IoU3D of the boxes a[k], b[k] ((P, 7) = x, y, z, dx, dy, dz, yaw), in their dtype"""
    zero = torch.zeros_like(a[:, 0])
    area_a, area_b = a[:, 3] * a[:, 4], b[:, 3] * b[:, 4]
    vol_a, vol_b = area_a * a[:, 5], area_b * b[:, 5]
    inter = bev_intersection(a[:, [0, 1, 3, 4, 6]], b[:, [0, 1, 3, 4, 6]])
    z = torch.minimum(a[:, 2] + a[:, 5] * 0.5, b[:, 2] + b[:, 5] * 0.5) - \
        torch.maximum(a[:, 2] - a[:, 5] * 0.5, b[:, 2] - b[:, 5] * 0.5)
    ok = ~((area_a < EPS) | (area_b < EPS) | (vol_a < EPS) | (vol_b < EPS)) & (inter > 0) & (z > 0)
    w = inter * z
    union = torch.where(ok, vol_a + vol_b - w, torch.ones_like(w))
    return torch.where(ok, w / union, zero)


def diff_iou_rotated_3d(box3d1, box3d2):
    """STAND-IN for mmcv.ops.diff_iou_rotated_3d (see the module docstring): (B, N, 7) x 2 -> (B, N)"""
    return iou3d_pairs(box3d1.reshape(-1, 7), box3d2.reshape(-1, 7)).reshape(box3d1.shape[:-1])


def weighted_loss(loss_func):
    """STAND-IN for mmdet's decorator (see the module docstring)"""
    @functools.wraps(loss_func)
    def wrapper(pred, target, weight=None, reduction='mean', avg_factor=None, **kwargs):
        loss = loss_func(pred, target, **kwargs)
        if weight is not None:
            loss = loss * weight
        if avg_factor is None:
            if reduction == 'mean':
                loss = loss.mean()
            elif reduction == 'sum':
                loss = loss.sum()
            elif reduction != 'none':
                raise ValueError(reduction)
        elif reduction == 'mean':
            loss = loss.sum() / avg_factor
        elif reduction != 'none':
            raise ValueError('avg_factor can not be used with reduction="sum"')
        return loss
    return wrapper


def values_and_grads(a, b, dtype):
    """(iou, d iou / d a, d iou / d b) of the stand-in evaluated in ``dtype``, returned as fp64 numpy"""
    ta = torch.from_numpy(np.asarray(a)).to(dtype).requires_grad_(True)
    tb = torch.from_numpy(np.asarray(b)).to(dtype).requires_grad_(True)
    iou = iou3d_pairs(ta, tb)
    ga, gb = torch.autograd.grad(iou.sum(), (ta, tb))
    return iou.detach().double().numpy(), ga.double().numpy(), gb.double().numpy()


def central_differences(a, b, step=1e-6):
    a, b = torch.from_numpy(a).double(), torch.from_numpy(b).double()
    ga, gb = torch.zeros_like(a), torch.zeros_like(b)
    with torch.no_grad():
        for k in range(7):
            d = torch.zeros(7, dtype=torch.float64)
            d[k] = step
            ga[:, k] = (iou3d_pairs(a + d, b) - iou3d_pairs(a - d, b)) / (2 * step)
            gb[:, k] = (iou3d_pairs(a, b + d) - iou3d_pairs(a, b - d)) / (2 * step)
    return ga.numpy(), gb.numpy()


# ---------------------------------------------------------------------------------------------------------
# general position
# ---------------------------------------------------------------------------------------------------------
def _corner_line_gap(o, x):
    """smallest distance of a corner of rectangle o[k] to an edge line of rectangle x[k] (fp64 numpy, (P, 7))"""
    gap = np.full(o.shape[0], np.inf)
    co, so, cx, sx = np.cos(o[:, 6]), np.sin(o[:, 6]), np.cos(x[:, 6]), np.sin(x[:, 6])
    for lx, ly in ((1, 1), (-1, 1), (-1, -1), (1, -1)):
        wx = o[:, 0] + lx * o[:, 3] / 2 * co - ly * o[:, 4] / 2 * so - x[:, 0]
        wy = o[:, 1] + lx * o[:, 3] / 2 * so + ly * o[:, 4] / 2 * co - x[:, 1]
        u, v = wx * cx + wy * sx, wy * cx - wx * sx
        for d in (u - x[:, 3] / 2, u + x[:, 3] / 2, v - x[:, 4] / 2, v + x[:, 4] / 2):
            gap = np.minimum(gap, np.abs(d))
    return gap


def degenerate(a, b):
    """pairs (fp32 boxes) that are NOT in general position"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    gap = np.minimum(_corner_line_gap(a, b), _corner_line_gap(b, a))
    top = np.abs((a[:, 2] + a[:, 5] / 2) - (b[:, 2] + b[:, 5] / 2))
    bot = np.abs((a[:, 2] - a[:, 5] / 2) - (b[:, 2] - b[:, 5] / 2))
    z = np.abs(np.minimum(a[:, 2] + a[:, 5] / 2, b[:, 2] + b[:, 5] / 2) -
               np.maximum(a[:, 2] - a[:, 5] / 2, b[:, 2] - b[:, 5] / 2))
    return ~((gap >= GUARD) & (top >= GUARD) & (bot >= GUARD) & (z >= GUARD))


SIZES = np.array([[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]])


def draw_second(rng, a, far, same_yaw):
    """a second box near (or, where ``far``, away from) each first box"""
    n = a.shape[0]
    b = a.copy()
    b[:, 0:2] += rng.normal(0, 0.25, (n, 2)) * a[:, 3:5].mean(1, keepdims=True)
    b[:, 2] += rng.normal(0, 0.3, n)
    b[:, 3:6] *= rng.uniform(0.8, 1.25, (n, 3))
    if not same_yaw:
        b[:, 6] += rng.normal(0, 0.4, n) + rng.randint(0, 4, n) * (rng.rand(n) < 0.3) * np.pi / 2
    away = rng.rand(n) < 0.5
    b[:, 0] += np.where(far & away, rng.uniform(4, 20, n), 0)
    b[:, 2] += np.where(far & ~away, rng.uniform(2.5, 4, n), 0)
    return b


def pairs_scene(rng, n, same_yaw):
    kind = rng.randint(0, 3, n)
    a = np.concatenate([rng.uniform(-75, 75, (n, 2)), rng.uniform(-2, 1, (n, 1)),
                        SIZES[kind] * rng.uniform(0.8, 1.25, (n, 3)), rng.uniform(-np.pi, np.pi, (n, 1))], 1)
    a = a.astype(np.float32)
    far = rng.rand(n) < 0.1
    b = draw_second(rng, a.astype(np.float64), far, same_yaw).astype(np.float32)
    for _ in range(200):
        bad = degenerate(a, b)
        if not bad.any():
            return a, b
        print('   ', int(bad.sum()), 'pairs not in general position: second box moved')
        b[bad] = draw_second(rng, a[bad].astype(np.float64), far[bad], same_yaw).astype(np.float32)
    raise RuntimeError('no scene in general position')


def special_pairs():
    s2 = np.sqrt(2.0)
    rows = [
        ([0, 0, 0, 1, 1, 1, 0], [0.5, 0, 0, 1, 1, 1, 0]),                          # offset unit cubes: 1/3
        ([0, 0, 0, 1, 1, 1, 0], [0, 0, 0, 1, 1, 1, np.pi / 4]),                     # the octagon
        ([0, 0, 0, 2, 2, 2, 0.3], [0, 0, 1, 2, 2, 2, 0.3]),                         # half z overlap: 1/3
        ([0, 0, 0, 4, 4, 4, 0.3], [0, 0, 0, 2, 2, 2, 0.3]),                         # containment: 1/8
        ([10, 5, -1, 3.9, 1.6, 1.56, 0.3], [10, 5, -1, 3.9, 1.6, 1.56, 0.3]),       # identical
        ([-70, 60, -1, 3.9, 1.6, 1.56, -2.1], [-70, 60, -1, 3.9, 1.6, 1.56, -2.1]),  # identical, far out
        ([20, -5, 0, 4, 2, 1.5, 0.7], [20.2, -5.1, 0.1, 1, 0.5, 0.5, 1.9]),         # contained, turned
        ([5, 5, 0, 3.9, 1.6, 1.5, 0.2], [5.3, 5.1, 1.5, 3.9, 1.6, 1.5, 0.4]),       # z-disjoint: faces touch
        ([5, 5, 0, 3.9, 1.6, 1.5, 0.2], [5.3, 5.1, 4.0, 3.9, 1.6, 1.5, 0.4]),       # z-disjoint
        ([5, 5, 0, 3.9, 1.6, 1.5, 0.2], [15, 5, 0, 3.9, 1.6, 1.5, 0.4]),            # BEV-disjoint, far
        ([5, 5, 0, 2, 2, 1.5, 0], [7.5, 5, 0, 2, 2, 1.5, 0]),                       # BEV-disjoint, circles meet
        ([5, 5, 0, 0, 1.6, 1.5, 0.2], [5, 5, 0, 3.9, 1.6, 1.5, 0.2]),               # zero dx
        ([5, 5, 0, 3.9, 1.6, 0, 0.2], [5, 5, 0, 3.9, 1.6, 1.5, 0.2]),               # zero dz
        ([5, 5, 0, 3.9, 1.6, 1.5, 0.2], [5, 5, 0, 0, 0, 0, 0]),                     # zero-size second box
        ([0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0]),                             # both empty
        ([40, 10, 0, 2, 2, 2, 0], [42, 10, 0, 2, 2, 2, 0]),                         # edge-touching
        ([0, 0, 0, s2, s2, 1, np.pi / 4], [0, 0, 0, 2, 2, 1, 0]),                   # inscribed diamond: 1/2
    ]
    a = np.asarray([r[0] for r in rows], np.float32)
    b = np.asarray([r[1] for r in rows], np.float32)
    return a, b


# ---------------------------------------------------------------------------------------------------------
# the head
# ---------------------------------------------------------------------------------------------------------
def lift(path, names, glb):
    """exec the named top-level functions / classes of a reference file; only the registry decorator of a
    class is taken off (the function keeps ``@weighted_loss``, resolved to the stand-in above)"""
    for node in ast.parse(open(path).read()).body:
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)) and node.name in names:
            if isinstance(node, ast.ClassDef):
                node.decorator_list = []
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, 'exec'), glb)
    return glb


def load_reference():
    g = {'torch': torch, 'nn': torch.nn, 'diff_iou_rotated_3d': diff_iou_rotated_3d, 'weighted_loss': weighted_loss}
    lift(mg.REF + 'models/losses/iou3d_loss.py', ['iou3d_loss', 'IOU3DLoss'], g)
    mg.extract_method(mg.REF + 'core/bbox/coders/delta_xyzwhlr_bbox_coder.py', 'DeltaXYZWLHRBBoxCoder', 'decode', g)
    return g


def encode(anchors, boxes):
    """the inverse of decode (fp64 numpy; only used to make plausible targets)"""
    xa, ya, za, wa, la, ha, ra = (anchors[:, i] for i in range(7))
    xg, yg, zg, wg, lg, hg, rg = (boxes[:, i] for i in range(7))
    diag = np.sqrt(la ** 2 + wa ** 2)
    return np.stack([(xg - xa) / diag, (yg - ya) / diag, ((zg + hg / 2) - (za + ha / 2)) / ha, np.log(wg / wa),
                     np.log(lg / la), np.log(hg / ha), rg - ra], 1)


def head_inputs(rng):
    pos = np.stack([rng.uniform(2, 59.6, 100), rng.uniform(-30.4, 30.4, 100)], 1)
    rows = []
    for p in pos:
        for c, zb in enumerate((-1.78, -0.6, -0.6)):
            for rot in (0.0, 1.57):
                rows.append([p[0], p[1], zb, *SIZES[c], rot])
    anchors = np.asarray(rows, np.float32)                                  # (600, 7)
    R = anchors.shape[0]
    a64 = anchors.astype(np.float64)
    gt = a64.copy()
    gt[:, 0:2] += rng.normal(0, 0.4, (R, 2))
    gt[:, 2] += rng.normal(0, 0.15, R)
    gt[:, 3:6] *= np.exp(rng.normal(0, 0.12, (R, 3)))
    gt[:, 6] += rng.normal(0, 0.25, R)
    targets = encode(a64, gt).astype(np.float32)
    return anchors, targets


def draw_pred(rng, targets):
    sigma = np.array([0.1, 0.1, 0.1, 0.08, 0.08, 0.08, 0.12])
    return (targets.astype(np.float64) + rng.normal(0, 1, targets.shape) * sigma).astype(np.float32)


def nan_targets(targets, pos):
    """one NaN component in the first three of every four positive rows: yaw, z, the width delta in turn (a NaN
    height delta would make z and dz of the two boxes equal: a pair on the measure-zero set)"""
    t = targets.copy()
    for k, col in enumerate((6, 2, 3)):
        t[pos[k::4], col] = np.nan
    return t


def decoded(g, anchors, deltas, pos, dtype):
    f = lambda x: torch.from_numpy(x).to(dtype)  # noqa: E731
    return g['decode'](f(anchors)[pos], f(deltas)[pos])


def head_pairs(g, anchors, pred, targets, pos):
    """the decoded fp32 boxes of the positives, the target's NaN components replaced as iou3d_loss does"""
    p = decoded(g, anchors, pred, pos, torch.float32)
    t = decoded(g, anchors, targets, pos, torch.float32)
    return p.numpy(), t.numpy(), torch.where(torch.isnan(t), p, t).numpy()


def run_head_case(g, anchors, pred, targets, pos, row_w, dtype):
    """the reference pipeline of loss_single's IoU term in ``dtype``: per-row loss, reduced loss with a tensor
    avg_factor, and the gradients of (row_w . per-row loss) and of the reduced loss with respect to bbox_pred"""
    f = lambda x: torch.from_numpy(x).to(dtype)  # noqa: E731
    a, t = f(anchors), f(targets)
    bp = f(pred).requires_grad_(True)
    loss_fn = g['IOU3DLoss'](loss_weight=1.0)
    pi = torch.from_numpy(pos)
    args = (g['decode'](a[pi], bp[pi]), g['decode'](a[pi], t[pi]))
    avg = torch.clamp(torch.tensor(float(len(pos)), dtype=dtype), min=10)
    if len(pos) == 0:
        try:
            loss_fn(*args, weight=None, avg_factor=avg)
            raise RuntimeError('the reference was expected to refuse P = 0')
        except AssertionError:
            pass
        rows = (args[0] - args[1]).sum(1) * 0.                             # the branch behind the assert
        reduced = rows.sum() / avg
    else:
        rows = loss_fn(*args, weight=None, reduction_override='none').reshape(-1)
        reduced = loss_fn(*args, weight=None, avg_factor=avg)
    g_rows, = torch.autograd.grad((rows * f(row_w)).sum(), bp, retain_graph=True)
    g_red, = torch.autograd.grad(reduced, bp)
    return [x.detach().double().numpy() for x in (rows, reduced, g_rows, g_red)] + [float(avg)]


def run_module_case(g, pred_boxes, target_boxes, weight, out, tag):
    """IOU3DLoss on decoded fp32 boxes, evaluated in fp64: every reduction, weight, float / tensor avg_factor"""
    def fresh():
        p = torch.from_numpy(pred_boxes).double().requires_grad_(True)
        t = torch.from_numpy(target_boxes).double().requires_grad_(True)
        return p, t
    w = torch.from_numpy(weight).double()
    for red in ('none', 'mean', 'sum'):
        p, t = fresh()
        out[f'{tag}/{red}'] = g['IOU3DLoss'](reduction=red)(p, t).detach().numpy()
        out[f'{tag}/{red}_weight'] = g['IOU3DLoss'](reduction=red)(p, t, weight=w).detach().numpy()
    p, t = fresh()
    out[f'{tag}/mean_avg_float'] = g['IOU3DLoss']()(p, t, weight=w, avg_factor=37.5).detach().numpy()
    out[f'{tag}/none_avg_float'] = g['IOU3DLoss']()(p, t, avg_factor=37.5, reduction_override='none').detach().numpy()
    try:
        g['IOU3DLoss'](reduction='sum')(p, t, avg_factor=37.5)
        raise RuntimeError('sum with avg_factor was expected to raise')
    except ValueError:
        pass
    loss = g['IOU3DLoss'](loss_weight=2.0)(p, t, weight=w, avg_factor=torch.tensor(37.5, dtype=torch.float64))
    gp, gt = torch.autograd.grad(loss, (p, t), allow_unused=True)
    out[f'{tag}/w2_mean_avg_tensor'] = loss.detach().numpy()
    out[f'{tag}/w2_mean_avg_tensor_grad_pred'] = gp.numpy()
    out[f'{tag}/w2_mean_avg_tensor_grad_target'] = torch.nan_to_num(gt, nan=0.0).numpy()


def main():
    g = load_reference()
    rng = np.random.RandomState(3007)
    out = {}
    iou_err = grad_err = 0.0

    def pairs(name, a, b, with_grads):
        nonlocal iou_err, grad_err
        v64, ga64, gb64 = values_and_grads(a, b, torch.float64)
        v32, ga32, gb32 = values_and_grads(a, b, torch.float32)
        assert np.isfinite(v64).all() and np.isfinite(ga64).all() and np.isfinite(gb64).all(), name
        assert np.isfinite(v32).all() and np.isfinite(ga32).all() and np.isfinite(gb32).all(), name
        iou_err = max(iou_err, float(np.abs(v64 - v32).max()))
        if with_grads:
            assert not degenerate(a, b).any(), name
            e = max(float(np.abs(ga64 - ga32).max()), float(np.abs(gb64 - gb32).max()))
            grad_err = max(grad_err, e)
            fa, fb = central_differences(a, b)
            fd = max(float(np.abs(fa - ga64).max()), float(np.abs(fb - gb64).max()))
            print(f'  {name}: {len(a)} pairs, {int((v64 > 0).sum())} overlap, IoU max {v64.max():.3f}, |grad| max '
                  f'{max(np.abs(ga64).max(), np.abs(gb64).max()):.3f}, fp32 grad error {e:.3g}, '
                  f'central differences within {fd:.3g}')
            assert fd < 1e-7, (name, fd)
        return v64, ga64, gb64

    print('general')
    a, b = pairs_scene(rng, 1024, False)
    v, ga, gb = pairs('general', a, b, True)
    assert 0.85 < (v > 0).mean() < 0.95
    out.update({'general/boxes1': a, 'general/boxes2': b, 'general/iou': v, 'general/grad1': ga, 'general/grad2': gb})

    print('aligned')
    a, b = pairs_scene(rng, 64, True)
    assert np.array_equal(a[:, 6], b[:, 6])
    v, ga, gb = pairs('aligned', a, b, True)
    out.update({'aligned/boxes1': a, 'aligned/boxes2': b, 'aligned/iou': v, 'aligned/grad1': ga, 'aligned/grad2': gb})

    print('special')
    a, b = special_pairs()
    v, _, _ = pairs('special', a, b, False)
    print('  special IoU', np.round(v, 6).tolist())
    out.update({'special/boxes1': a, 'special/boxes2': b, 'special/iou': v})

    print('head')
    anchors, targets = head_inputs(rng)
    R = anchors.shape[0]
    p257 = np.sort(rng.permutation(R)[:257]).astype(np.int64)
    cases = {'p257': (p257, targets), 'p1': (p257[100:101], targets), 'p0': (p257[:0], targets),
             'nan': (p257, nan_targets(targets, p257))}
    pred = draw_pred(rng, targets)
    for _ in range(200):
        bad = np.zeros(R, bool)
        for pos, tg in cases.values():
            if len(pos):
                p, _, t = head_pairs(g, anchors, pred, tg, pos)
                bad[pos[degenerate(p, t)]] = True
        if not bad.any():
            break
        print('   ', int(bad.sum()), 'rows not in general position: prediction drawn again')
        pred[bad] = draw_pred(rng, targets[bad])
    else:
        raise RuntimeError('no head scene in general position')
    # the rows outside every pos_inds: predictions that are not near their (zero) targets
    rest = np.setdiff1d(np.arange(R), p257)
    pred[rest] = rng.normal(0, 0.3, (len(rest), 7)).astype(np.float32)
    targets[rest] = 0
    cases['nan'] = (p257, nan_targets(targets, p257))
    row_w = rng.uniform(0.5, 1.5, R).astype(np.float32)
    out.update({'head/anchors': anchors, 'head/bbox_pred': pred, 'head/row_weights': row_w})
    loss_err = hgrad_err = 0.0
    for name, (pos, tg) in cases.items():
        rw = row_w[:len(pos)]
        r64 = run_head_case(g, anchors, pred, tg, pos, rw, torch.float64)
        r32 = run_head_case(g, anchors, pred, tg, pos, rw, torch.float32)
        if len(pos):
            loss_err = max(loss_err, float(np.abs(r64[0] - r32[0]).max()))
            hgrad_err = max(hgrad_err, float(np.abs(r64[2] - r32[2]).max()), float(np.abs(r64[3] - r32[3]).max()))
            p, t_raw, t = head_pairs(g, anchors, pred, tg, pos)
            pairs(f'head/{name}', p, t, True)
            out.update({f'head/{name}/pred_boxes': p, f'head/{name}/target_boxes': t_raw})
        assert np.isfinite(r64[2]).all() and np.isfinite(r64[3]).all()
        out.update({f'head/{name}/pos_inds': pos, f'head/{name}/bbox_targets': tg, f'head/{name}/loss_rows': r64[0],
                    f'head/{name}/loss_reduced': r64[1], f'head/{name}/grad_rows': r64[2],
                    f'head/{name}/grad_reduced': r64[3], f'head/{name}/avg_factor': np.float64(r64[4])})
        print(f'  head/{name}: P = {len(pos)}, reduced loss {float(r64[1]):.6f}, |grad| max {np.abs(r64[2]).max():.3f}')
    weight = rng.uniform(0.5, 1.5, 257).astype(np.float32)
    out['head/module_weight'] = weight
    for name in ('p257', 'nan'):
        run_module_case(g, out[f'head/{name}/pred_boxes'], out[f'head/{name}/target_boxes'], weight, out,
                        f'head/{name}/module')

    print('fp32_iou_error', iou_err, 'fp32_grad_error', grad_err)
    print('fp32_head_loss_error', loss_err, 'fp32_head_grad_error', hgrad_err)
    out.update(fp32_iou_error=np.float64(iou_err), fp32_grad_error=np.float64(grad_err),
               fp32_head_loss_error=np.float64(loss_err), fp32_head_grad_error=np.float64(hgrad_err),
               guard=np.float64(GUARD))
    path = os.path.join(HERE, 'iou3d.npz')
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    if not os.path.isdir(mg.REF):
        sys.exit('reference not mounted; the fixture is committed, nothing to do')
    torch.set_num_threads(1)
    main()
