"""Hard voxelization of the LiDAR teacher on the HIP path.

Mirror of mmcv's ``Voxelization`` (the deterministic hard mode, ``max_num_points > 0``) as the KITTI configs' frozen
teacher uses it: ``voxel_layer=dict(max_num_points=5, voxel_size=[0.05, 0.05, 0.1], max_voxels=(40000, 40000))``.
The semantics are those of the reference's in-tree ``points_to_voxel(..., reverse_index=True)``
(core/voxel/voxel_generator.py), stated in include/dfm_hip_sparse_conv.h: all three results are bit-identical to it,
and the same bits run after run.

The per-point and per-voxel work is four HIP kernels (``dfm_voxel_keys / heads / keep / fill``); between them torch
runs one stable sort, two prefix sums and one prefix maximum -- all of fixed size, so nothing waits for the device.

Host waits: ``hard_voxelize_batch`` none (the row count stays on the device, unused rows carry batch index -1);
``hard_voxelize`` and ``Voxelization.forward`` ONE, the read of the row count ``M`` their mmcv-shaped results are
sliced to.  CPU tensors are refused: there is no CPU path.
"""
import numpy as np
import torch
from torch import nn

from . import _capi
from ._launch import STREAM, launch, require_gpu
from .registry import register_module

__all__ = ['hard_voxelize', 'hard_voxelize_batch', 'Voxelization', 'HardSimpleVFE', 'voxel_grid_size']


def voxel_grid_size(voxel_size, point_cloud_range):
    """cells along (x, y, z): ``round((hi - lo) / voxel_size)`` in fp32, as the reference computes it"""
    r = np.asarray(point_cloud_range, dtype=np.float32)
    vs = np.asarray(voxel_size, dtype=np.float32)
    if r.shape != (6,) or vs.shape != (3,):
        raise ValueError('voxel_size is 3 numbers and point_cloud_range 6, got '
                         f'{voxel_size!r} and {point_cloud_range!r}')
    grid = np.round((r[3:] - r[:3]) / vs).astype(np.int32)
    if not (vs > 0).all() or not (grid >= 1).all():
        raise ValueError(f'voxel_size {voxel_size!r} over point_cloud_range {point_cloud_range!r} gives the grid '
                         f'{grid.tolist()}')
    return tuple(int(g) for g in grid)


def _desc(sizes, ndim, voxel_size, point_cloud_range, max_num_points, max_voxels):
    if not 1 <= len(sizes) <= _capi.VOXEL_MAX_BATCH:
        raise ValueError(f'a batch of {len(sizes)} clouds: 1 to {_capi.VOXEL_MAX_BATCH}')
    if max_num_points < 1 or max_voxels < 1:
        raise ValueError('hard voxelization needs max_num_points >= 1 and max_voxels >= 1 '
                         '(dynamic voxelization is not built)')
    d = _capi.VoxelDesc(batch=len(sizes), ndim=ndim, max_num_points=max_num_points, max_voxels=max_voxels)
    grid = voxel_grid_size(voxel_size, point_cloud_range)
    lo = np.asarray(point_cloud_range, dtype=np.float32)[:3]
    vs = np.asarray(voxel_size, dtype=np.float32)
    for j in range(3):
        d.grid[j], d.lo[j], d.vs[j] = grid[j], float(lo[j]), float(vs[j])
    total = 0
    for b in range(_capi.VOXEL_MAX_BATCH + 1):
        d.offset[b] = total
        if b < len(sizes):
            total += sizes[b]
    return d


def hard_voxelize_batch(points_list, voxel_size, point_cloud_range, max_num_points, max_voxels):
    """A list of ``B`` clouds ``(N_b, ndim)`` fp32 -> ``(voxels (R, max_num_points, ndim) fp32, coors (R, 4) int32
    (b, z, y, x), num_points (R,) int32, count)`` with ``R = B * max_voxels`` fixed-capacity rows: the first ``count``
    (a 0-d int64 tensor ON THE DEVICE) are the voxels of sample 0 in first-appearance order, then sample 1's, ...;
    every row past them has batch index -1 (and coordinates -1), zero points and ``num_points`` 0.  No host wait."""
    if not isinstance(points_list, (list, tuple)) or not points_list:
        raise TypeError('points_list is a non-empty list of (N, ndim) tensors')
    ndim = points_list[0].shape[-1]
    for p in points_list:
        require_gpu(p, 'points')
        if p.dim() != 2 or p.shape[1] != ndim or p.dtype != torch.float32:
            raise ValueError(f'every cloud is (N, {ndim}) float32, got {tuple(p.shape)} {p.dtype}')
    sizes = [int(p.shape[0]) for p in points_list]
    d = _desc(sizes, ndim, voxel_size, point_cloud_range, int(max_num_points), int(max_voxels))
    device = points_list[0].device
    rows, n = len(sizes) * int(max_voxels), sum(sizes)
    voxels = torch.zeros((rows, int(max_num_points), ndim), dtype=torch.float32, device=device)
    coors = torch.full((rows, 4), -1, dtype=torch.int32, device=device)
    num_points = torch.zeros((rows,), dtype=torch.int32, device=device)
    if n == 0:
        return voxels, coors, num_points, torch.zeros((), dtype=torch.int64, device=device)
    points = points_list[0] if len(points_list) == 1 else torch.cat([p for p in points_list if p.shape[0]])
    points = points.contiguous()
    key = torch.empty((n,), dtype=torch.int64, device=device)
    launch('dfm_voxel_keys', d, points, key, STREAM)
    sorted_key, perm = torch.sort(key, stable=True)
    first = torch.empty((n,), dtype=torch.int32, device=device)
    head = torch.empty((n,), dtype=torch.int64, device=device)
    launch('dfm_voxel_heads', d, sorted_key, perm, first, head, STREAM)
    first_scan = torch.cumsum(first, 0, dtype=torch.int64)
    head_scan = torch.cummax(head, 0).values
    keep = torch.empty((n,), dtype=torch.int32, device=device)
    launch('dfm_voxel_keep', d, first, first_scan, keep, STREAM)
    keep_scan = torch.cumsum(keep, 0, dtype=torch.int64)
    launch('dfm_voxel_fill', d, points, sorted_key, perm, head_scan, keep, keep_scan, voxels, coors, num_points,
           STREAM)
    return voxels, coors, num_points, keep_scan[-1]


def hard_voxelize(points, voxel_size, point_cloud_range, max_num_points, max_voxels):
    """One cloud ``(N, ndim)`` -> ``(voxels (M, max_num_points, ndim), coors (M, 3) int32 (z, y, x), num_points (M,)
    int32)``: the reference's ``points_to_voxel(points, voxel_size, point_cloud_range, max_num_points, True,
    max_voxels)`` bit for bit.  ONE host wait: the read of ``M``."""
    voxels, coors, num_points, count = hard_voxelize_batch([points], voxel_size, point_cloud_range, max_num_points,
                                                           max_voxels)
    m = int(count)   # the one host read: mmcv's result is sliced to the voxel count
    return voxels[:m], coors[:m, 1:].contiguous(), num_points[:m]


@register_module(on_path=False)
class Voxelization(nn.Module):
    """mmcv's ``Voxelization`` (same constructor), hard mode.  ``forward(points (N, ndim))`` -> ``(voxels (M,
    max_num_points, ndim), coors (M, 3) int32 z, y, x, num_points (M,) int32)``; ``max_voxels`` is ``(training,
    testing)`` or one number.  ONE host wait per call (the slice to ``M``); ``forward_batch(points_list)`` is
    ``hard_voxelize_batch`` with the module's settings and waits for nothing."""

    def __init__(self, voxel_size, point_cloud_range, max_num_points, max_voxels=20000, deterministic=True):
        super().__init__()
        if max_num_points == -1 or max_voxels == -1:
            raise NotImplementedError('dynamic voxelization (max_num_points = -1) is not built on the HIP path')
        self.voxel_size, self.point_cloud_range = list(voxel_size), list(point_cloud_range)
        self.max_num_points = int(max_num_points)
        self.max_voxels = tuple(max_voxels) if isinstance(max_voxels, (tuple, list)) else (max_voxels, max_voxels)
        self.deterministic = deterministic   # this path is deterministic either way
        gx, gy, gz = voxel_grid_size(voxel_size, point_cloud_range)
        self.grid_size = torch.tensor([gx, gy, gz])
        self.pcd_shape = [1, gy, gx]   # mmcv: [*grid_size[:2], 1][::-1]

    def _max_voxels(self):
        return int(self.max_voxels[0] if self.training else self.max_voxels[1])

    def forward(self, points):
        return hard_voxelize(points, self.voxel_size, self.point_cloud_range, self.max_num_points, self._max_voxels())

    def forward_batch(self, points_list):
        return hard_voxelize_batch(points_list, self.voxel_size, self.point_cloud_range, self.max_num_points,
                                   self._max_voxels())

    def __repr__(self):
        return (f'{type(self).__name__}(voxel_size={self.voxel_size}, point_cloud_range={self.point_cloud_range}, '
                f'max_num_points={self.max_num_points}, max_voxels={self.max_voxels}, '
                f'deterministic={self.deterministic})')


@register_module(on_path=False)
class HardSimpleVFE(nn.Module):
    """The reference's ``HardSimpleVFE`` (voxel_encoders/voxel_encoder.py): the mean of a voxel's points over its first
    ``num_features`` features -- a plain torch mirror (the sum runs in slot order).  It divides by ``num_points`` on
    live rows only: a row with ``num_points = 0`` (the fixed-capacity padding of ``hard_voxelize_batch``) stays exactly
    zero instead of 0 / 0."""

    def __init__(self, num_features=4):
        super().__init__()
        self.num_features = num_features
        self.fp16_enabled = False

    def forward(self, features, num_points, coors=None):
        # the points of a voxel are added one after the other, in point order: the same bits on every device and run
        total = features[:, 0, :self.num_features]
        for i in range(1, features.shape[1]):
            total = total + features[:, i, :self.num_features]
        live = num_points > 0
        count = torch.where(live, num_points, torch.ones_like(num_points)).to(features.dtype).view(-1, 1)
        return torch.where(live.view(-1, 1), total / count, torch.zeros_like(total)).contiguous()
