"""Generate tests/golden/depth_targets.npz: the depth loss's targets (``depth_img``, ``depth_fgmask_img``) and the
box-membership operators.

Run in the build container only (needs the reference checkout):   python tests/golden/make_golden_depth_targets.py

Executed from the reference, lifted from their files by AST or executed by path, unmodified (same rules as
ref_stubs.py and the other generators; only inputs and the results they produced are stored):
  * ``GenerateDepthMap`` (datasets/pipelines/transforms_3d.py, the class with its registry decorator taken off), its
    ``__call__`` on an ``input_dict`` and its ``__repr__``;
  * ``Calibration.rect_to_img`` (core/camera/calibration.py, the whole file; an instance is made without a calib file
    and given ``P2``);
  * ``points_img2cam`` (core/bbox/structures/utils.py) UNDER ITS DECORATOR ``array_converter``
    (core/utils/array_converter.py, the whole file): with numpy arguments the decorator makes FP32 tensors, so the
    reference unprojects in FP32;
  * ``depth_map_in_boxes_cpu``, ``points_in_boxes_cpu_idmap`` and ``check_numpy_to_torch`` (datasets/utils.py).

STAND-IN: mmcv is not installed, so ``mmcv.ops.points_in_boxes_cpu`` alone is a numpy FP32 restatement of mmcv's
documented rule (cz = z + z_size/2; reject if |pz - cz| > z_size/2; a = -yaw; lx = dx cos a - dy sin a,
ly = dx sin a + dy cos a; inside iff |lx| < x_size/2 and |ly| < y_size/2, strict), returning the (B, N, M) int32 0/1
tensor the caller transposes.  ``points_in_boxes_part`` / ``_all`` of the membership case are the same restatement.

Every comparison the tests make is bit-exact, so the reference itself must be stable on the inputs.  For every case
but ``exact`` this file asserts, in FP64, and redraws from its fixed seed until all hold:
  * every finite u, v is at least 1e-9 from a half-integer (the image edges -0.5 and w - 0.5 are half-integers);
  * each float(depth) and each FP32 unprojected coordinate is unchanged when its FP64 source moves by 4 ulp;
  * each (pixel point, box) pair is at least 1e-4 m from the box's surface (the largest of the three signed face
    distances |l| - half size is at least 1e-4 from 0), with the box-local coordinates taken in FP64;
  * the reference's FP32 unprojection and the FP64 one differ by less than 5e-5 m (``img2cam_fp32_deviation`` stores
    the largest difference seen): half the face margin, so neither arithmetic can move a point across a face.
The ``exact`` case uses P = [[64,0,16,0],[0,64,8,0],[0,0,1,0]] and dyadic coordinates: every intermediate value is exact
in FP32 and in FP64, ties and points on a face included.

Maps are stored sparsely (flat indices and values of the non-zero pixels, the bit patterns for the depths).
"""
import ast
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference/mmdet3d/'
OUT = os.path.join(HERE, 'depth_targets.npz')
FACE_MARGIN, HALF_MARGIN, ULPS = 1e-4, 1e-9, 4


# ---------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------
def points_in_boxes_cpu(points, boxes):
    """numpy FP32 STAND-IN for mmcv.ops.points_in_boxes_cpu (see the module docstring): (B, N, M) int32"""
    p = points.detach().numpy().astype(np.float32)
    b = boxes.detach().numpy().astype(np.float32)
    two = np.float32(2)
    px, py, pz = (p[..., k][:, :, None] for k in range(3))
    x, y, z, xs, ys, zs, yaw = (b[..., k][:, None, :] for k in range(7))
    cz = z + zs / two
    a = -yaw
    dx, dy = px - x, py - y
    lx = dx * np.cos(a) - dy * np.sin(a)
    ly = dx * np.sin(a) + dy * np.cos(a)
    inside = ~(np.abs(pz - cz) > zs / two) & (lx > -xs / two) & (lx < xs / two) & (ly > -ys / two) & (ly < ys / two)
    return torch.from_numpy(inside.astype(np.int32))


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _lift(path, names, glb, keep_decorators=False):
    """exec the named top-level functions / classes of a reference file in ``glb``"""
    tree = ast.parse(open(path).read())
    found = []
    for node in tree.body:
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)) and node.name in names:
            if not keep_decorators:
                node.decorator_list = []
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, 'exec'), glb)
            found.append(node.name)
    assert sorted(found) == sorted(names), (path, found)
    return glb


def load_reference():
    ac = _load(REF + 'core/utils/array_converter.py', '_ref_array_converter')
    calib = _load(REF + 'core/camera/calibration.py', '_ref_calibration')
    g = {'torch': torch, 'np': np, 'array_converter': ac.array_converter}
    _lift(REF + 'core/bbox/structures/utils.py', ['points_img2cam'], g, keep_decorators=True)
    g['points_in_boxes_cpu'] = points_in_boxes_cpu
    _lift(REF + 'datasets/utils.py', ['check_numpy_to_torch', 'depth_map_in_boxes_cpu', 'points_in_boxes_cpu_idmap'], g)
    _lift(REF + 'datasets/pipelines/transforms_3d.py', ['GenerateDepthMap'], g)
    g['Calibration'] = calib.Calibration
    return g


def make_calib(g, P):
    c = object.__new__(g['Calibration'])
    c.P2 = P
    return c


def reference_maps(g, points, boxes, P, cam2img, img_shape, pad_shape):
    d = dict(cam2img=cam2img, points=types.SimpleNamespace(tensor=torch.from_numpy(points)), calib=make_calib(g, P),
             pad_shape=tuple(pad_shape), img_shape=tuple(img_shape),
             gt_bboxes_3d=types.SimpleNamespace(tensor=torch.from_numpy(boxes)))
    with np.errstate(all='ignore'):
        out = g['GenerateDepthMap'](generate_fgmask=True)(d)
    assert out['depth_img'].dtype == np.float32 and out['depth_fgmask_img'].dtype == np.int32
    assert out['depth_img'].shape == out['depth_fgmask_img'].shape == tuple(pad_shape[:2])
    return out['depth_img'], out['depth_fgmask_img']


# ---------------------------------------------------------------------------------------------------------
# the stability conditions, FP64
# ---------------------------------------------------------------------------------------------------------
def _moved(a, ulps):
    lo = hi = a
    for _ in range(ulps):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
    return lo, hi


def _f32_stable(a):
    lo, hi = _moved(a, ULPS)
    a32 = a.astype(np.float32)
    return bool(np.all((lo.astype(np.float32) == a32) & (hi.astype(np.float32) == a32)))


def local64(pts, boxes):
    """the largest signed face distance (N, M) of FP64 points against FP32 boxes, box-local coordinates in FP64"""
    b = boxes.astype(np.float64)
    px, py, pz = (pts[:, k][:, None] for k in range(3))
    x, y, z, xs, ys, zs, yaw = (b[:, k][None] for k in range(7))
    a = -yaw
    dx, dy = px - x, py - y
    lx, ly = dx * np.cos(a) - dy * np.sin(a), dx * np.sin(a) + dy * np.cos(a)
    return np.maximum(np.maximum(np.abs(lx) - xs / 2, np.abs(ly) - ys / 2), np.abs(pz - (z + zs / 2)) - zs / 2)


def stable(g, points, boxes, P, cam2img, img_shape, pad_shape, depth_img):
    """(ok, reason, FP32-vs-FP64 deviation of the unprojection) of one sample"""
    x, y, z = (points[:, k].astype(np.float64) for k in range(3))
    X, Y, Z = -y, -z, x
    with np.errstate(all='ignore'):
        h = [X * P[r, 0] + Y * P[r, 1] + Z * P[r, 2] + P[r, 3] for r in range(3)]
        u, v = h[0] / Z, h[1] / Z
    depth = h[2] - P[2, 3]
    for c in (u, v):
        c = c[np.isfinite(c)]
        if c.size and np.min(np.abs((c - 0.5) - np.round(c - 0.5))) < HALF_MARGIN:
            return False, 'a pixel coordinate within 1e-9 of a half-integer', 0.0
    if not _f32_stable(depth):
        return False, 'a depth within 4 ulp of an FP32 rounding boundary', 0.0
    mask = depth_img > 0
    if not mask.any():
        return True, '', 0.0
    iy, ix = np.nonzero(mask)
    d = depth_img[mask].astype(np.float64)
    pad = np.eye(4)
    pad[:cam2img.shape[0], :cam2img.shape[1]] = cam2img
    inv = np.linalg.inv(pad)
    homo = np.stack([ix * d, iy * d, d, np.ones_like(d)], 1)
    cam = homo @ inv.T
    pts = np.stack([cam[:, 2], -cam[:, 0], -cam[:, 1]], 1)
    if not _f32_stable(pts):
        return False, 'an unprojected coordinate within 4 ulp of an FP32 rounding boundary', 0.0
    ref = g['points_img2cam'](np.stack([ix, iy, depth_img[mask]], 1), cam2img)      # the reference: FP32 inside
    deviation = float(np.max(np.abs(np.stack([ref[:, 2], -ref[:, 0], -ref[:, 1]], 1) - pts)))
    if deviation >= FACE_MARGIN / 2:
        return False, f'the FP32 unprojection is {deviation:.2e} m from the FP64 one', deviation
    if boxes.shape[0] and np.min(np.abs(local64(pts, boxes))) < FACE_MARGIN:
        return False, 'a pixel point within 1e-4 m of a box surface', deviation
    return True, '', deviation


# ---------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------
KITTI_P2 = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791],
                     [0.0, 0.0, 1.0, 0.002745884]])


def augmented(scale, crop_x, crop_y):
    """KITTI's P2 after a resize by ``scale`` and a crop at (crop_x, crop_y): a non-zero fourth column"""
    P = KITTI_P2.copy()
    P[:2] *= scale
    P[0] -= crop_x * P[2]
    P[1] -= crop_y * P[2]
    return P


def cam4(P):
    return np.vstack([P, [0.0, 0.0, 0.0, 1.0]])


def frustum_points(rng, n, P, img_shape, zmin, zmax, spill=1.15):
    """n pseudo-LiDAR points (n, 4) FP32 whose projections cover the image and spill over its edges"""
    Z = rng.uniform(zmin, zmax, n)
    u = (rng.uniform(-0.5, 0.5, n) * spill + 0.5) * img_shape[1]
    v = (rng.uniform(-0.5, 0.5, n) * spill + 0.5) * img_shape[0]
    X = (u * Z - P[0, 2] * Z - P[0, 3]) / P[0, 0]
    Y = (v * Z - P[1, 2] * Z - P[1, 3]) / P[1, 1]
    return np.stack([Z, -X, -Y, rng.uniform(0, 1, n)], 1).astype(np.float32)


def boxes_on(rng, points, m, size_lo, size_hi):
    """m LiDAR boxes (m, 7) FP32 centred on points of the cloud, every second one rotated; box 1 overlaps box 0"""
    rows = []
    for k in range(m):
        c = points[rng.integers(0, len(points)), :3].astype(np.float64)
        size = rng.uniform(size_lo, size_hi, 3)
        if k == 1:
            c = rows[0][:3] + np.array([0.3 * rows[0][3], 0.1, 0.5 * rows[0][5]])       # inside box 0
        yaw = rng.uniform(-3.5, 3.5) if k % 2 == 0 else 0.0
        rows.append(np.array([c[0], c[1], c[2] - size[2] / 2, size[0], size[1], size[2], yaw]))
    return np.array(rows, dtype=np.float32).reshape(m, 7)


def settle(g, draw, what):
    """draw() -> a list of samples (points, boxes, P, cam2img, img_shape, pad_shape); redrawn until every sample is
    stable.  Returns the samples, their reference maps and the largest FP32 deviation"""
    for attempt in range(200):
        samples = draw()
        maps, worst, reason = [], 0.0, ''
        for s in samples:
            depth, mask = reference_maps(g, *s)
            ok, reason, dev = stable(g, *s, depth)
            worst = max(worst, dev)
            if not ok:
                break
            maps.append((depth, mask))
        else:
            print(f'{what}: settled at attempt {attempt}, FP32 deviation {worst:.2e} m')
            return samples, maps, worst
        print(f'{what}: attempt {attempt} redrawn ({reason})')
    raise AssertionError(f'{what}: the conditions did not settle')


def sparse(store, key, depth, mask):
    idx = np.nonzero(depth.reshape(-1).view(np.uint32))[0]
    store[f'{key}/depth_idx'] = idx.astype(np.int32)
    store[f'{key}/depth_bits'] = depth.reshape(-1).view(np.uint32)[idx]
    idx = np.nonzero(mask.reshape(-1))[0]
    store[f'{key}/mask_idx'] = idx.astype(np.int32)
    store[f'{key}/mask_val'] = mask.reshape(-1)[idx].astype(np.int32)


def put(store, key, sample, maps):
    points, boxes, P, cam2img, img_shape, pad_shape = sample
    store[f'{key}/points'], store[f'{key}/boxes'], store[f'{key}/P'] = points, boxes, P
    store[f'{key}/cam2img'] = cam2img
    store[f'{key}/img_shape'] = np.array(img_shape, dtype=np.int64)
    store[f'{key}/pad_shape'] = np.array(pad_shape, dtype=np.int64)
    sparse(store, key, *maps)


def exact_case():
    """see the module docstring; every pixel named here is reserved: no filler point lands on it"""
    P = np.array([[64.0, 0, 16, 0], [0, 64.0, 8, 0], [0, 0, 1.0, 0]])
    h, w, n = 16, 32, 5000
    rng = np.random.default_rng(7)

    def at(u, v, Z):              # the pseudo-LiDAR point that projects to (u, v) at depth Z, all dyadic
        return [Z, -(u - 16) * Z / 64, -(v - 8) * Z / 64, 0.0]
    special = {
        # ties: even k stays, odd k goes up; -0.5 -> -0 (kept, column / row 0); w - 0.5 -> w (dropped)
        10: at(4.5, 3, 2.0), 11: at(5.5, 3, 2.0), 12: at(-0.5, 5, 2.0), 13: at(w - 0.5, 5, 2.0),
        14: at(9, 2.5, 4.0), 15: at(9, 3.5, 4.0), 16: at(11, -0.5, 4.0), 17: at(11, h - 0.5, 4.0),
        # Z = 0 (u = +-inf), X = Z = 0 (0 / 0), Z < 0 inside the image (depth -2 is written, gets no id)
        20: [0.0, 1.0, 1.0, 0.0], 21: [0.0, 0.0, 1.0, 0.0], 22: at(24, 8, -2.0),
        # five points on pixel (20, 12), depths not monotonic: the last one stays
        30: at(20, 12, 8.0), 31: at(20.25, 12, 2.0), 32: at(19.75, 11.75, 16.0), 33: at(20, 12.25, 1.0),
        34: at(20, 12, 4.0),
        # two points on pixel (26, 2), 4900 indices apart (different workgroups)
        50: at(26, 2, 8.0), 4950: at(26, 2, 2.0),
        # on a face at yaw 0 (outside), inside, in the plane of a box with dz = 0 (held: |pz - cz| > 0 does not
        # reject it) and 1/64 m above that plane (not held)
        60: at(16, 8, 4.0), 61: at(17, 8, 4.0), 62: at(12, 8, 1.0), 63: at(12, 7, 1.0),
    }
    # pixel (16, 8) depth 4 -> point (4, 0, 0): on the face x = 4 of box 0 (x in [2, 4]) and on the face y = 0 of box 1
    # pixel (17, 8) depth 4 -> point (4, -1/16, 0): box 1 spans x in [2.5, 4.5], y in [-0.5, 0], z in [-1, 1]: inside
    # pixel (12, 8) depth 1 -> point (1, 1/16, 0), pixel (12, 7) -> (1, 1/16, 1/64): box 2 has dz = 0 at z = 0
    boxes = np.array([[3.0, 0.5, -1.0, 2.0, 2.0, 2.0, 0.0], [3.5, -0.25, -1.0, 2.0, 0.5, 2.0, 0.0],
                      [1.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0], [8.0, 0.0, -2.0, 4.0, 8.0, 4.0, 0.0]], dtype=np.float32)
    reserved = {(4, 3), (5, 3), (6, 3), (0, 5), (9, 2), (9, 4), (11, 0), (24, 8), (20, 12), (26, 2), (16, 8), (17, 8),
                (12, 8), (12, 7)}
    pts = np.zeros((n, 4))
    for i in range(n):
        if i in special:
            pts[i] = special[i]
            continue
        while True:
            Z = float(rng.choice([0.5, 1.0, 2.0, 4.0, 8.0, 16.0]))
            u, v = rng.integers(-8, 8 * (w + 1)) / 8.0, rng.integers(-8, 8 * (h + 1)) / 8.0
            if (int(np.round(u)), int(np.round(v))) not in reserved:
                break
        pts[i] = at(u, v, Z)
    pts32 = pts.astype(np.float32)
    assert np.array_equal(pts32.astype(np.float64), pts)
    return pts32, boxes, P, cam4(P), (h, w, 3), (h, w, 3)


def membership_case(rng):
    """(2, 515, 3) x (2, 5, 7), overlapping boxes; points at least 1e-4 m from every box surface"""
    for _ in range(200):
        boxes = np.zeros((2, 5, 7))
        for b in range(2):
            for k in range(5):
                boxes[b, k] = [rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(-1, 0), rng.uniform(3, 7),
                               rng.uniform(2, 5), rng.uniform(1.5, 3), rng.uniform(-4, 4)]
        boxes[1, 4, 3:6] = 0.0                                        # a zero-size padding row
        boxes32 = boxes.astype(np.float32)
        points = np.stack([rng.uniform(-5, 5, (2, 515)), rng.uniform(-5, 5, (2, 515)), rng.uniform(-1.5, 3, (2, 515))],
                          -1).astype(np.float32)
        if all(np.min(np.abs(local64(points[b].astype(np.float64), boxes32[b]))) >= FACE_MARGIN for b in range(2)):
            inside = points_in_boxes_cpu(torch.from_numpy(points), torch.from_numpy(boxes32)).numpy()
            part = np.where(inside.any(-1), inside.argmax(-1), -1).astype(np.int32)
            idmap = np.where(inside.any(-1), 4 - inside[..., ::-1].argmax(-1), -1).astype(np.int32)
            assert (part != idmap).sum() >= 20 and (part == -1).sum() >= 20 and inside[1, :, 4].sum() == 0
            return points, boxes32, inside, part, idmap
    raise AssertionError('membership: the conditions did not settle')


def main():
    g = load_reference()
    rng = np.random.default_rng(20261020)
    store, worst = {}, 0.0

    def random_draw():
        P = augmented(1.03, 597.0, 163.0)
        img, pad = (30, 61, 3), (32, 64, 3)
        pts = frustum_points(rng, 300, P, pad, 5.0, 40.0)            # over the pad band as well: dropped there
        boxes = np.array([[14.0, 0.1, -1.6, 9.0, 1.3, 2.6, 0.3], [27.0, -0.2, -2.2, 12.0, 2.4, 3.6, 0.0],
                          [30.0, 0.1, -1.8, 7.0, 1.6, 2.8, -0.2]]) + np.r_[rng.normal(0, 0.2, 6), 0.0]
        return [(pts, boxes.astype(np.float32), P, cam4(P), img, pad)]
    samples, maps, dev = settle(g, random_draw, 'random')
    worst = max(worst, dev)
    put(store, 'random', samples[0], maps[0])
    assert (maps[0][1] == 1).any() and (maps[0][1] == 2).any() and (maps[0][1] == 3).any()
    assert not maps[0][0][30:].any() and not maps[0][0][:, 61:].any() and (maps[0][0] > 0).sum() > 100

    sample = exact_case()
    depth, mask = reference_maps(g, *sample)
    put(store, 'exact', sample, (depth, mask))
    # what the case is there to show, read off the reference's own result
    assert depth[3, 4] == 2 and depth[3, 6] == 2 and depth[3, 5] == 0 and depth[5, 0] == 2 and depth[2, 9] == 4
    assert depth[4, 9] == 4 and depth[0, 11] == 4 and depth[8, 24] == -2 and mask[8, 24] == 0
    assert depth[12, 20] == 4 and depth[2, 26] == 2 and mask[8, 16] == 0 and mask[8, 17] == 2
    assert mask[8, 12] == 3 and mask[7, 12] == 0
    assert depth[8, 16] == 4 and depth[8, 17] == 4 and depth[8, 12] == 1 and (mask == 4).any()
    inv32 = torch.inverse(torch.tensor(cam4(sample[2]), dtype=torch.float32)).numpy()
    assert np.array_equal(inv32.astype(np.float64), np.linalg.inv(cam4(sample[2])))          # exact in both

    P = augmented(1.0, 600.0, 170.0)
    some_boxes = np.array([[10.0, 0, -1, 4, 2, 2, 0.1], [20.0, 0, -1, 4, 2, 2, 0], [15.0, 0, -1, 30, 4, 3, 0]],
                          dtype=np.float32)
    for key, n, bx in (('empty/none', 0, some_boxes[:0]), ('empty/no_points', 0, some_boxes),
                       ('empty/no_boxes', 100, some_boxes[:0])):
        def draw(n=n, bx=bx):
            pts = frustum_points(rng, n, P, (8, 16), 5.0, 30.0).reshape(n, 4)
            return [(pts, bx, P, cam4(P), (8, 16, 3), (8, 16, 3))]
        samples, maps, dev = settle(g, draw, key)
        put(store, key, samples[0], maps[0])
        assert not maps[0][1].any() and bool(maps[0][0].any()) == (n > 0)

    def batch_draw():
        out = []
        for b, (n, m) in enumerate(zip((0, 257, 5000), (2, 0, 7))):
            Pb = augmented(1.0 + 0.02 * b, 590.0 + 8 * b, 160.0 + 5 * b)
            img, pad = ((32, 64, 3), (29, 64, 3), (31, 57, 3))[b], (32, 64, 3)
            pts = frustum_points(rng, n, Pb, pad, 4.0, 45.0).reshape(n, 4)
            src = pts if n else frustum_points(rng, 50, Pb, pad, 4.0, 45.0)
            cam2img = (cam4(Pb), Pb[:, :3].copy(), Pb.copy())[b]                     # 4x4, 3x3, 3x4
            out.append((pts, boxes_on(rng, src, m, 3.0, 14.0), Pb, cam2img, img, pad))
        return out
    samples, maps, dev = settle(g, batch_draw, 'batch')
    worst = max(worst, dev)
    for b in range(3):
        put(store, f'batch/{b}', samples[b], maps[b])
    assert (maps[2][1] > 0).sum() > 50 and len(np.unique(maps[2][1])) >= 4

    def config_draw():
        Pc = augmented(1.0, 0.0, 55.0)
        img, pad = (320, 1242, 3), (320, 1280, 3)
        pts = frustum_points(rng, 20000, Pc, (320, 1280), 3.0, 60.0, spill=1.05)
        return [(pts, boxes_on(rng, pts, 12, 1.5, 6.0), Pc, cam4(Pc), img, pad)]
    samples, maps, dev = settle(g, config_draw, 'config')
    worst = max(worst, dev)
    put(store, 'config', samples[0], maps[0])
    assert (maps[0][0] > 0).sum() > 15000 and len(np.unique(maps[0][1])) >= 4

    points, boxes, inside, part, idmap = membership_case(rng)
    store.update({'membership/points': points, 'membership/boxes': boxes, 'membership/all': inside.astype(np.int32),
                  'membership/part': part, 'membership/idmap': idmap})
    store['img2cam_fp32_deviation'] = np.float64(worst)
    store['repr'] = np.array(repr(g['GenerateDepthMap'](generate_fgmask=True)))
    np.savez_compressed(OUT, **store)
    size = os.path.getsize(OUT)
    print(f'{OUT}: {size} bytes, FP32 unprojection deviation {worst:.2e} m')
    assert size < 1024 * 1024


if __name__ == '__main__':
    main()
