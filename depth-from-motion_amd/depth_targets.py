"""The depth loss's targets on the HIP path: the LiDAR depth map, the box-id mask, and box membership.

Mirror of the reference's pipeline step ``GenerateDepthMap(generate_fgmask=True)``
(``mmdet3d/datasets/pipelines/transforms_3d.py:55-118``) with ``Calibration.rect_to_img``
(``core/camera/calibration.py:230-240``), ``depth_map_in_boxes_cpu`` / ``points_in_boxes_cpu_idmap``
(``datasets/utils.py:403-455``) and ``points_img2cam`` (``core/bbox/structures/utils.py:217-248``), and of mmcv's
``points_in_boxes_part`` / ``points_in_boxes_all``, compiled operators that do not exist on this platform.

  * ``depth_img``: the LiDAR points projected into the augmented image; where several points round to one pixel the
    one with the highest index stays, as the reference's fancy-index assignment lets it.
  * ``depth_fgmask_img``: for every pixel with ``depth > 0`` the 1-based id of the highest-indexed ground-truth box
    that holds the pixel's unprojected point, else 0.

On device tensors a batch is ONE memset and TWO launches of this package's kernels and NO host wait
(include/dfm_hip_depth_targets.h states the arithmetic): ``counters()`` keeps count of those -- not of torch's copies
around them (the small table upload; for B > 1 the concatenation of the clouds and of the boxes).
On numpy arrays and CPU tensors the same arithmetic runs in numpy -- a loader
worker has no GPU.  The results are integers and copied floats: the two paths agree bit for bit wherever the point is
not within rounding distance of a half-integer pixel coordinate or of a box face.

One deliberate deviation: ``points_img2cam`` is decorated with ``array_converter``, which turns numpy arguments into
FP32 tensors, so the reference unprojects a pixel with an FP32 inverse and an FP32 product.  Here the inverse is taken
in FP64 on the host and the product runs in FP64; the unprojected point is rounded to FP32 once.  The two differ by some
1e-5 m at KITTI ranges, which moves a pixel across a box face only if it lies that close to it.
"""
import numpy as np
import torch

from . import _capi
from ._launch import STREAM, Workspace, launch, require_gpu, upload

__all__ = ['generate_depth_map', 'depth_map_in_boxes', 'generate_depth_targets', 'points_in_boxes_part',
           'points_in_boxes_all', 'points_in_boxes_idmap', 'GenerateDepthMap', 'counters']

MAX_BATCH = _capi.DEPTH_MAX_BATCH
MAX_POINTS = 2 ** 32 - 2    # the key's index word holds index + 1
MAX_BOXES = 2 ** 31 - 2     # the int32 id holds index + 1

_COUNTERS = {'kernel_launches': 0, 'memsets': 0, 'host_waits': 0}


def counters(reset=False):
    """kernel launches, device memsets and host waits (device-to-host copies, each of which waits for the stream) made
    by this module so far; ``reset=True`` zeroes them after reading"""
    out = dict(_COUNTERS)
    if reset:
        for k in _COUNTERS:
            _COUNTERS[k] = 0
    return out


# ---------------------------------------------------------------------------------------------------------
# arguments
# ---------------------------------------------------------------------------------------------------------
def _host_matrix(m, name):
    """a small matrix as FP64 numpy; a device tensor is copied to the host, which waits for its stream (counted)"""
    if torch.is_tensor(m):
        if m.is_cuda:
            _COUNTERS['host_waits'] += 1
        m = m.detach().cpu().numpy()
    m = np.asarray(m, dtype=np.float64)
    if m.ndim != 2:
        raise ValueError(f'{name} is a matrix, got shape {m.shape}')
    return m


def _proj(m):
    m = _host_matrix(m, 'proj')
    if m.shape[0] < 3 or m.shape[1] != 4:
        raise ValueError(f'proj is the 3x4 projection (or a 4x4 matrix whose first three rows are), got {m.shape}')
    return np.ascontiguousarray(m[:3])


def _inv_cam2img(m):
    """points_img2cam's inverse (utils.py:239-241): cam2img padded to 4x4 with the identity, inverted in FP64"""
    m = _host_matrix(m, 'cam2img')
    if m.shape[0] > 4 or m.shape[1] > 4:
        raise ValueError(f'cam2img is at most 4x4, got {m.shape}')
    pad = np.eye(4, dtype=np.float64)
    pad[:m.shape[0], :m.shape[1]] = m
    try:
        return np.linalg.inv(pad)
    except np.linalg.LinAlgError:
        raise ValueError('cam2img is singular: a depth pixel cannot be unprojected') from None


def _shape2(s, name):
    s = tuple(int(v) for v in tuple(s)[:2])
    if len(s) != 2 or s[0] < 0 or s[1] < 0:
        raise ValueError(f'{name} is (height, width, ...), got {s}')
    return s


def _check_shapes(img_shape, pad_shape):
    img, pad = _shape2(img_shape, 'img_shape'), _shape2(pad_shape, 'pad_shape')
    if pad[0] <= 0 or pad[1] <= 0:
        raise ValueError(f'pad_shape must be positive, got {pad}')
    if img[0] > pad[0] or img[1] > pad[1]:
        raise ValueError(f'img_shape {img} does not fit pad_shape {pad}: a kept point would land outside the map')
    return img, pad


def _box_tensor(boxes):
    """a (M, >=7) array of LiDAR boxes, or an object that holds one as ``.tensor`` (LiDARInstance3DBoxes)"""
    return boxes.tensor if hasattr(boxes, 'tensor') and not torch.is_tensor(boxes) else boxes


def _check_points(p, name='points'):
    if p.ndim != 2 or p.shape[1] < 3:
        raise ValueError(f'{name} is (N, >=3) with x, y, z first, got {tuple(p.shape)}')
    if p.dtype not in (np.float32, torch.float32):
        raise TypeError(f'{name} must be float32 (the LiDAR cloud as the pipeline holds it), got {p.dtype}')
    if p.shape[0] > MAX_POINTS:
        raise ValueError(f'{name}: {p.shape[0]} points, the key of a pixel holds the point index in 32 bits '
                         f'(at most {MAX_POINTS})')


def _check_boxes(b, name='boxes'):
    if b.ndim != 2 or b.shape[1] < 7:
        raise ValueError(f'{name} is (M, >=7) = x, y, z, x_size, y_size, z_size, yaw, got {tuple(b.shape)}')
    if b.dtype not in (np.float32, torch.float32):
        raise TypeError(f'{name} must be float32, got {b.dtype}')
    if b.shape[0] > MAX_BOXES:
        raise ValueError(f'{name}: {b.shape[0]} boxes, the int32 id holds at most {MAX_BOXES}')


def _is_device(t):
    return torch.is_tensor(t) and t.is_cuda


def _as_numpy(t):
    return t.detach().numpy() if torch.is_tensor(t) else np.asarray(t)


# ---------------------------------------------------------------------------------------------------------
# the numpy path: the kernels' operations in the kernels' order and precision.  Every FP64 and FP32 operation is
# correctly rounded on both sides but for cos / sin of the yaw: numpy's float32 cos / sin and the device's cosf / sinf
# may differ in the last ulp, so the two paths agree on a point unless it lies within that rounding of a box face
# ---------------------------------------------------------------------------------------------------------
def _dot4(a, b, c, d, m):
    return ((a * m[0] + b * m[1]) + c * m[2]) + d * m[3]


def _rectify_np(points):
    """pseudo-LiDAR (N, >=3) FP32 -> rectified camera (N, 3) FP64: homo @ pseudo2cam_T (transforms_3d.py:69-76)"""
    x, y, z = (points[:, k].astype(np.float64) for k in range(3))
    with np.errstate(all='ignore'):
        return np.stack([((x * 0.0 + y * -1.0) + z * 0.0) + 0.0, ((x * 0.0 + y * 0.0) + z * -1.0) + 0.0,
                         ((x * 1.0 + y * 0.0) + z * 0.0) + 0.0], 1)


def _scatter_np(rect, proj, img, pad):
    """rectified points (N, 3) FP64 -> depth map pad FP32: rect_to_img, np.round, the image test, highest index wins"""
    X, Y, Z = rect[:, 0], rect[:, 1], rect[:, 2]
    one = np.float64(1.0)
    with np.errstate(all='ignore'):
        h0, h1, h2 = (_dot4(X, Y, Z, one, proj[r]) for r in range(3))
        u, v = h0 / Z, h1 / Z
        depth = (h2 - proj[2, 3]).astype(np.float32)
        ru, rv = np.rint(u), np.rint(v)
        keep = np.isfinite(u) & np.isfinite(v) & (rv >= 0) & (rv < img[0]) & (ru >= 0) & (ru < img[1])
    idx = np.nonzero(keep)[0]
    keys = np.zeros(pad[0] * pad[1], dtype=np.uint64)
    lin = rv[idx].astype(np.int64) * pad[1] + ru[idx].astype(np.int64)
    key = ((idx.astype(np.uint64) + np.uint64(1)) << np.uint64(32)) | depth[idx].view(np.uint32).astype(np.uint64)
    np.maximum.at(keys, lin, key)
    return (keys & np.uint64(0xffffffff)).astype(np.uint32).view(np.float32).reshape(pad)


def _pt_boxes_np(boxes, ratio=1.0, distance=0.0):
    """csrc/box_membership.h pt_box on (M, 7) FP32: centre x, y, cz, half sizes, cos / sin of -yaw, all FP32"""
    b = np.ascontiguousarray(boxes[:, :7], dtype=np.float32)
    two = np.float32(2.0)
    h = (b[:, 3:6] * np.float32(ratio) + np.float32(distance)) / two
    a = -b[:, 6]
    return b[:, 0], b[:, 1], b[:, 2] + h[:, 2], h[:, 0], h[:, 1], h[:, 2], np.cos(a), np.sin(a)


def _inside_np(pts, pb):
    """(N, M) bool: pt_in_box of every FP32 point against every box"""
    x, y, cz, hx, hy, hz, ca, sa = pb
    px, py, pz = (pts[:, k:k + 1] for k in range(3))
    with np.errstate(all='ignore'):
        dx, dy = px - x[None], py - y[None]
        lx = dx * ca[None] - dy * sa[None]
        ly = dx * sa[None] + dy * ca[None]
        return ~(np.abs(pz - cz[None]) > hz[None]) & (lx > -hx[None]) & (lx < hx[None]) & (ly > -hy[None]) & \
            (ly < hy[None])


def _highest_np(inside):
    n, m = inside.shape
    if m == 0:
        return np.full(n, -1, dtype=np.int32)
    return np.where(inside, np.arange(m, dtype=np.int32)[None], np.int32(-1)).max(1).astype(np.int32)


def _lowest_np(inside):
    n, m = inside.shape
    if m == 0:
        return np.full(n, -1, dtype=np.int32)
    first = np.where(inside, np.arange(m, dtype=np.int32)[None], np.int32(m)).min(1)
    return np.where(first == m, -1, first).astype(np.int32)


def _fgmask_np(depth_img, boxes, inv, ratio, distance):
    out = np.zeros(depth_img.shape, dtype=np.int32)
    with np.errstate(invalid='ignore'):
        mask = depth_img > 0
    if boxes.shape[0] == 0 or not mask.any():
        return out
    iy, ix = np.nonzero(mask)
    d = depth_img[mask].astype(np.float64)
    hx, hy, one = ix.astype(np.float64) * d, iy.astype(np.float64) * d, np.float64(1.0)
    cx, cy, cz = (_dot4(hx, hy, d, one, inv[r]) for r in range(3))
    pts = np.stack([cz, -cx, -cy], 1).astype(np.float32)
    pb = _pt_boxes_np(boxes, ratio, distance)
    ids = np.empty(len(pts), dtype=np.int32)
    for s in range(0, len(pts), 65536):
        ids[s:s + 65536] = _highest_np(_inside_np(pts[s:s + 65536], pb))
    out[mask] = ids + 1
    return out


# ---------------------------------------------------------------------------------------------------------
# the batch
# ---------------------------------------------------------------------------------------------------------
def _desc(sizes, box_counts, stride, imgs, pad):
    d = _capi.DepthTargetsDesc()
    d.batch, d.pad_h, d.pad_w, d.point_stride = len(sizes), pad[0], pad[1], stride
    for b, (n, m, img) in enumerate(zip(sizes, box_counts, imgs)):
        d.img_h[b], d.img_w[b] = img
        d.point_off[b + 1] = d.point_off[b] + n
        d.box_off[b + 1] = d.box_off[b] + m
    return d


def _cat(parts, width, device):
    parts = [p for p in parts if p.shape[0]]
    if not parts:
        return None
    t = parts[0] if len(parts) == 1 else torch.cat(parts)
    return t.contiguous() if width is None else t[:, :width].contiguous()


def _keys(desc, device):
    nbytes = _capi.lib().dfm_depth_targets_workspace_bytes(desc)
    if nbytes == 0:
        _capi.check(-1)
    index = device.index if device.index is not None else torch.cuda.current_device()
    with torch.cuda.device(index):
        return Workspace.get(index, torch.cuda.current_stream(index).cuda_stream, nbytes), nbytes


def _device_batch(points_list, boxes_list, projs, invs, imgs, pad, want_depth, want_mask, ratio, distance,
                  depth_in=None):
    """the launches of one batch: scatter (unless ``depth_in`` is given) and resolve"""
    B = len(imgs)
    device = depth_in.device if depth_in is not None else points_list[0].device
    sizes = [int(p.shape[0]) for p in points_list] if points_list is not None else [0] * B
    counts = [int(b.shape[0]) for b in boxes_list] if boxes_list is not None else [0] * B
    stride = int(points_list[0].shape[1]) if points_list is not None else 3
    d = _desc(sizes, counts, stride, imgs, pad)
    cam = np.zeros((B, _capi.DEPTH_CAM_DOUBLES), dtype=np.float64)
    for b in range(B):
        if projs is not None:
            cam[b, :12] = projs[b].reshape(-1)
        cam[b, 12:] = (invs[b] if invs is not None else np.eye(4)).reshape(-1)
    cam_d = upload(torch.from_numpy(cam), device)
    keys = None
    if depth_in is None:
        points = _cat(points_list, None, device)
        keys, nbytes = _keys(d, device)
        launch('dfm_depth_scatter', d, points, cam_d, keys, nbytes, STREAM)
        _COUNTERS['memsets'] += 1
        _COUNTERS['kernel_launches'] += int(points is not None)
    boxes = _cat(boxes_list, 7, device) if want_mask else None
    depth = torch.empty((B, 1) + pad, dtype=torch.float32, device=device) if want_depth else None
    mask = torch.empty((B, 1) + pad, dtype=torch.int32, device=device) if want_mask else None
    launch('dfm_depth_resolve', d, keys, depth_in, cam_d, boxes, float(ratio), float(distance), depth, mask, STREAM)
    _COUNTERS['kernel_launches'] += 1
    return depth, mask


def generate_depth_targets(points_list, boxes_list, projs, cam2imgs, img_shapes, pad_shape, generate_fgmask=True,
                           expand_ratio=1.0, expand_distance=0.):
    """The two maps of a batch: ``(depth_img (B, 1, H, W) float32, depth_fgmask_img (B, 1, H, W) int32)`` with
    ``(H, W) = pad_shape[:2]`` -- the shapes ``loss_dense_depth`` flattens; the mask is ``None`` with
    ``generate_fgmask=False``.

    ``points_list``: B clouds ``(N_b, >=3)`` float32 in the pseudo-LiDAR frame (x forward, y left, z up; what the
    detector's ``points`` argument holds);  ``boxes_list``: B box sets ``(M_b, >=7)`` float32 or objects with such a
    ``.tensor``;  ``projs``: B 3x4 projections (the reference's ``calib.P2``);  ``cam2imgs``: B intrinsics, up to 4x4;
    ``img_shapes``: B ``(h, w, ...)``, a point outside is dropped;  ``pad_shape``: the maps' size.
    Device tensors run the kernels: one memset and two launches of the package's own, no host wait.
    Numpy arrays and CPU tensors run the numpy
    path and return CPU tensors."""
    B = len(points_list)
    if B == 0 or not (len(projs) == len(img_shapes) == B) or \
            (generate_fgmask and not (len(boxes_list) == len(cam2imgs) == B)):
        raise ValueError('points_list, boxes_list, projs, cam2imgs and img_shapes hold one entry per sample, at least '
                         'one')
    if B > MAX_BATCH:
        raise ValueError(f'{B} samples in one call, at most {MAX_BATCH} (DFM_DEPTH_MAX_BATCH)')
    boxes_list = [_box_tensor(b) for b in boxes_list] if generate_fgmask else None
    for p in points_list:
        _check_points(p)
    for b in boxes_list or ():
        _check_boxes(b)
    if len({int(p.shape[1]) for p in points_list}) != 1:
        raise ValueError('every cloud of a batch has the same number of columns')
    shapes = [_check_shapes(s, pad_shape) for s in img_shapes]
    imgs, pad = [s[0] for s in shapes], shapes[0][1]
    projs = [_proj(p) for p in projs]
    invs = [_inv_cam2img(c) for c in cam2imgs] if generate_fgmask else None
    on_device = [_is_device(t) for t in list(points_list) + list(boxes_list or ())]
    if all(on_device):
        devices = sorted({str(t.device) for t in list(points_list) + list(boxes_list or ())})
        if len(devices) != 1:
            raise RuntimeError(f'points and boxes of one batch live on one GPU, got {", ".join(devices)}: '
                               'depth-from-motion_amd has no cross-device kernels')
        return _device_batch(points_list, boxes_list, projs, invs, imgs, pad, True, generate_fgmask, expand_ratio,
                             expand_distance)
    if any(on_device):
        raise RuntimeError('points and boxes of one batch live either all on the GPU (the kernels) or all on the host '
                           '(the numpy path)')
    depth = np.stack([_scatter_np(_rectify_np(_as_numpy(p)), projs[b], imgs[b], pad)
                      for b, p in enumerate(points_list)])
    mask = None
    if generate_fgmask:
        mask = np.stack([_fgmask_np(depth[b], _as_numpy(boxes_list[b]), invs[b], expand_ratio, expand_distance)
                         for b in range(B)])
        mask = torch.from_numpy(mask[:, None])
    return torch.from_numpy(depth[:, None]), mask


def _like(result, template):
    """a (H, W) CPU tensor as numpy when the caller gave numpy"""
    return result if torch.is_tensor(template) else result.numpy()


def generate_depth_map(points, proj, img_shape, pad_shape):
    """``depth_img`` ``(H, W)`` float32 of one cloud ``(N, >=3)`` float32 (pseudo-LiDAR frame): transforms_3d.py:92-103
    with ``proj`` for ``calib.P2``.  A device tensor runs the kernels; numpy gives numpy, a CPU tensor a CPU tensor."""
    depth, _ = generate_depth_targets([points], None, [proj], None, [img_shape], pad_shape, generate_fgmask=False)
    return _like(depth[0, 0], points)


def depth_map_in_boxes(depth_img, boxes, cam2img, expand_ratio=1.0, expand_distance=0.):
    """``depth_map_in_boxes_cpu`` (datasets/utils.py:403-427), same signature: ``(H, W)`` int32, 1 + the highest index
    of a box that holds the pixel's point, 0 for none and wherever ``depth_img > 0`` does not hold."""
    boxes = _box_tensor(boxes)
    if depth_img.ndim != 2:
        raise ValueError(f'depth_img is (H, W), got {tuple(depth_img.shape)}')
    if depth_img.dtype not in (np.float32, torch.float32):
        raise TypeError(f'depth_img must be float32, got {depth_img.dtype}')
    _check_boxes(boxes)
    pad = tuple(int(v) for v in depth_img.shape)
    inv = _inv_cam2img(cam2img)
    if _is_device(depth_img) != _is_device(boxes):
        raise RuntimeError('depth_img and boxes live either both on the GPU (the kernel) or both on the host (the '
                           'numpy path)')
    if _is_device(depth_img):
        _, mask = _device_batch(None, [boxes], None, [inv], [pad], pad, False, True, expand_ratio, expand_distance,
                                depth_in=depth_img.contiguous())
        return mask[0, 0]
    out = _fgmask_np(np.ascontiguousarray(_as_numpy(depth_img)), _as_numpy(boxes), inv, expand_ratio, expand_distance)
    return _like(torch.from_numpy(out), depth_img)


# ---------------------------------------------------------------------------------------------------------
# box membership
# ---------------------------------------------------------------------------------------------------------
def _points_in_boxes(points, boxes, mode):
    if points.ndim != 3 or points.shape[2] != 3:
        raise ValueError(f'points must have 3 dimensions (B, N, 3), but got {tuple(points.shape)}')
    if boxes.ndim != 3 or boxes.shape[2] != 7:
        raise ValueError(f'boxes dimension should be 7 (B, M, 7), but got unexpected shape {tuple(boxes.shape)}')
    if boxes.shape[0] != points.shape[0]:
        raise ValueError(f'Points and boxes should have the same batch size, but got {boxes.shape[0]} and '
                         f'{points.shape[0]}')
    if points.dtype not in (np.float32, torch.float32) or boxes.dtype not in (np.float32, torch.float32):
        raise TypeError(f'points and boxes must be float32, got {points.dtype} and {boxes.dtype}')
    B, N, M = int(points.shape[0]), int(points.shape[1]), int(boxes.shape[1])
    if M > MAX_BOXES:
        raise ValueError(f'{M} boxes, the int32 index holds at most {MAX_BOXES}')
    shape = (B, N, M) if mode == _capi.PIB_ALL else (B, N)
    if _is_device(points) != _is_device(boxes):
        raise RuntimeError('points and boxes live either both on the GPU (the kernel) or both on the host (the numpy '
                           'path)')
    if _is_device(points):
        require_gpu(boxes, 'boxes')
        out = torch.empty(shape, dtype=torch.int32, device=points.device)
        if out.numel():
            launch('dfm_points_in_boxes', mode, B, N, M, points.contiguous(), boxes.contiguous() if M else None, out,
                   STREAM)
            _COUNTERS['kernel_launches'] += 1
        return out
    p, bx = _as_numpy(points), _as_numpy(boxes)
    out = np.empty(shape, dtype=np.int32)
    for b in range(B):
        inside = _inside_np(p[b], _pt_boxes_np(bx[b]))
        out[b] = inside.astype(np.int32) if mode == _capi.PIB_ALL else \
            (_lowest_np(inside) if mode == _capi.PIB_PART else _highest_np(inside))
    return torch.from_numpy(out) if torch.is_tensor(points) else out


def points_in_boxes_part(points, boxes):
    """mmcv's ``points_in_boxes_part``: ``(B, N)`` int32, the lowest index of a box ``(B, M, 7)`` that holds the point
    ``(B, N, 3)``, -1 for none (LiDAR boxes: bottom centre, yaw about z)."""
    return _points_in_boxes(points, boxes, _capi.PIB_PART)


def points_in_boxes_all(points, boxes):
    """mmcv's ``points_in_boxes_all``: ``(B, N, M)`` int32, 1 where the box holds the point, else 0."""
    return _points_in_boxes(points, boxes, _capi.PIB_ALL)


def points_in_boxes_idmap(points, boxes):
    """``(B, N)`` int32: the HIGHEST index of a box that holds the point, -1 for none -- what
    ``points_in_boxes_cpu_idmap`` (datasets/utils.py:430-455) makes of mmcv's ``points_in_boxes_cpu``."""
    return _points_in_boxes(points, boxes, _capi.PIB_IDMAP)


# ---------------------------------------------------------------------------------------------------------
# the pipeline step
# ---------------------------------------------------------------------------------------------------------
class GenerateDepthMap(object):
    """Generate depth map by projecting LiDAR points: the reference's pipeline step (transforms_3d.py:55-118), same
    constructor, ``__call__(input_dict)`` contract and ``__repr__``.  Reads ``cam2img``, ``rect_points`` (rectified
    camera points) or else ``points`` (an object whose ``.tensor`` is the pseudo-LiDAR cloud), ``calib`` (its ``P2``;
    absent: ``cam2img[:3]``), ``pad_shape``, ``img_shape`` and, for the mask, ``gt_bboxes_3d``; writes ``depth_img``
    (float32) and ``depth_fgmask_img`` (int32) as numpy arrays.  A loader worker has no GPU: this runs the numpy
    path."""

    def __init__(self, generate_fgmask=True):
        self.generate_fgmask = generate_fgmask

    def __call__(self, input_dict):
        cam2img = input_dict['cam2img']
        if 'rect_points' in input_dict:
            rect = np.asarray(input_dict['rect_points'], dtype=np.float64)[:, :3]
        else:
            pts = input_dict['points']
            pts = pts.tensor if hasattr(pts, 'tensor') else pts
            rect = _rectify_np(np.asarray(_as_numpy(pts.cpu() if torch.is_tensor(pts) else pts), dtype=np.float32))
        calib = input_dict.get('calib')
        proj = _proj(calib.P2 if calib is not None else cam2img)
        img, pad = _check_shapes(input_dict['img_shape'], input_dict['pad_shape'])
        input_dict['depth_img'] = _scatter_np(rect, proj, img, pad)
        if self.generate_fgmask:
            boxes = _box_tensor(input_dict['gt_bboxes_3d'])
            boxes = _as_numpy(boxes.cpu() if torch.is_tensor(boxes) else boxes)[:, :7].astype(np.float32)
            input_dict['depth_fgmask_img'] = _fgmask_np(input_dict['depth_img'], boxes, _inv_cam2img(cam2img), 1.0, 0.)
        return input_dict

    def __repr__(self):
        repr_str = self.__class__.__name__
        repr_str += f'(generate_fgmask={self.generate_fgmask}.'
        return repr_str
