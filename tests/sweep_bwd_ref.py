"""fp64 reference of the plane sweep's backward -- TEST INFRASTRUCTURE, NOT PRODUCT.

The adjoint of the two ``F.grid_sample`` calls of ``build_dfm_cost`` (reference dfm_backbone.py:296-311;
bilinear, zeros padding, ``align_corners=True``) in plain numpy, and the problems the backward tests run:
tests/test_sweep_bwd_ref.py checks this file against torch's CPU autograd, tests/test_sweep_bwd_exact_gpu.py
checks the HIP kernels against this file.

Positions.  The oracle's fp32 normalised grids (``orc.sweep_params`` / ``orc.plane_sweep_grid``) are
un-normalised in fp32 exactly as ATen does, ``((g + 1) / 2) * (size - 1)``: the forward kernels and
``dfm_plane_sweep_grid`` are pinned bit for bit to these positions, and an fp64 un-normalisation would move a
position by a coordinate ulp, i.e. a weight by about 1e-5.  Everything after that is fp64: the corner
``floor(x)``, the fractions, the four weights ``(1 - fy | fy) * (1 - fx | fx)``, the in-bounds masks, and the
sums (``np.add.at`` into float64 maps).  A non-finite position contributes nothing.

Per map element the reference returns
    grad : sum_k w_k g_k
    A    : sum_k w_k |g_k|   (the same pass on |grad|: what every rounding-error bound is proportional to)
    n    : the number of in-bounds taps that land there (zero-weight taps included, as in ATen)
"""
import functools

import numpy as np

from oracle import dfm_oracle as orc
from tests import util

U = 2.0 ** -24  # fp32 unit roundoff (round to nearest)


def positions(grid, H, W):
    """(x, y) fp32 sample positions of a normalised fp32 grid (N, 2): ATen's grid_sampler_unnormalize with
    align_corners=True, in fp32, op by op"""
    grid = np.ascontiguousarray(grid, np.float32)
    one, two = np.float32(1.0), np.float32(2.0)
    x = ((grid[:, 0] + one) / two) * np.float32(W - 1)
    y = ((grid[:, 1] + one) / two) * np.float32(H - 1)
    assert x.dtype == np.float32 and y.dtype == np.float32
    return x, y


def adjoint(x, y, g, H, W):
    """x, y (N,) fp32 positions, g (C, N) gradient of the sampled values -> (grad (C, H, W) f64, A (C, H, W) f64,
    n (H, W) int64, oob: number of taps outside the map among the finite positions)"""
    C, N = g.shape
    fin = np.isfinite(x) & np.isfinite(y)
    x64 = np.where(fin, x, np.float32(0)).astype(np.float64)
    y64 = np.where(fin, y, np.float32(0)).astype(np.float64)
    xw, yn = np.floor(x64), np.floor(y64)
    fx, fy = x64 - xw, y64 - yn
    gt = np.ascontiguousarray(g.T, np.float64)      # (N, C): one row per sample
    grad = np.zeros((H * W, C), np.float64)
    A = np.zeros((H * W, C), np.float64)
    n = np.zeros(H * W, np.int64)
    oob = 0
    for dy in (0, 1):
        for dx in (0, 1):
            ix, iy = xw + dx, yn + dy
            ok = fin & (ix >= 0) & (ix <= W - 1) & (iy >= 0) & (iy <= H - 1)
            oob += int((fin & ~ok).sum())
            w = ((fy if dy else 1.0 - fy) * (fx if dx else 1.0 - fx))[ok]
            idx = (iy[ok] * W + ix[ok]).astype(np.int64)
            contrib = gt[ok] * w[:, None]
            np.add.at(grad, idx, contrib)
            np.add.at(A, idx, np.abs(contrib))
            np.add.at(n, idx, 1)
    to_map = lambda a: np.ascontiguousarray(a.T).reshape(C, H, W)
    return to_map(grad), to_map(A), n.reshape(H, W), oob


# ---------------------------------------------------------------------------------------------------------
# geometry cases (shared by every kernel that accepts them) and problems (geometry x shape)
# ---------------------------------------------------------------------------------------------------------
def _geometry(name, shape):
    """-> dict(P (B,4,4), T (B,4,4), flip, crop, scale, depths (D,))"""
    B, D = shape['B'], shape['D']
    P = np.stack([util.KITTI_P2] * B).copy()
    if shape['center'] or name == 'zplane':
        # the principal point in the middle of the image region the maps cover (small maps: forward motion then
        # zooms about their centre instead of sweeping every sample off the map)
        P[:, 0, 2], P[:, 1, 2] = shape['W'] * shape['fsf'] / 2.0, shape['H'] * shape['fsf'] / 2.0
    T = util.random_poses(B, seed=11)
    g = dict(flip=False, crop=(0, 0), scale=1.0, depths=util.depth_planes(D))
    if name == 'plain':
        pass
    elif name == 'aug':              # flip + crop (7, 55) + scale 0.97
        g.update(flip=True, crop=(7, 55), scale=0.97)
    elif name == 'scale103':         # scale 1.03 (run at cost_sample_factor 8: a pose whose disparities differ
        g.update(scale=1.03)         # from plane to plane, so that the few lattice points reach many pixels)
        T[:] = util.pose(1.0, 0.3, 0.2, -0.8)
    elif name == 'batch2':           # two samples: different intrinsics (principal point) and poses
        assert B == 2
        P[1, 0, 2] += 3.5
        P[1, 1, 2] -= 2.25
        T = np.stack([util.pose(1.5, 0.08, 0.0, -0.5), util.pose(-1.0, -0.06, 0.0, -1.3)])
    elif name == 'forward':          # strong forward motion
        T[:, 2, 3] = -4.0
    elif name == 'zplane':           # plane 1 at z = 0 in the previous camera, plane 0 behind it, the rest in front
        P[:, :3, 3] = 0.0
        P[:, 0, 0] = P[:, 1, 1] = 720.0
        g['depths'] = np.concatenate([np.array([1.0, 2.0], np.float32), g['depths'][2:]])
        T[:] = np.eye(4, dtype=np.float32)
        T[:, 2, 3] = -float(g['depths'][1])
        T[:, 0, 3] = 0.3
    elif name == 'outside':          # a lateral pose that throws every prev sample out of the map
        T[:] = util.pose(0.0, 500.0, 0.0, 0.0)
    elif name == 'lateral':          # sideways motion only: prev samples stay in their rows (maps of 3 / 4 rows)
        T[:] = util.pose(0.0, 0.5, 0.0, 0.0)
    else:
        raise KeyError(name)
    g.update(P=P.astype(np.float32), T=T.astype(np.float32))
    return g


GEOMETRIES = ('plain', 'aug', 'scale103', 'batch2', 'forward', 'zplane', 'outside')


def _shape(B, C, H, W, D, fsf, csf, center=False):
    return dict(B=B, C=C, H=H, W=W, D=D, fsf=fsf, csf=csf, center=center)


# shapes, the smallest that reach the kernels' edges (which kernel takes which: tests/test_sweep_bwd_exact_gpu.py)
SHAPES = {
    'tiny_dense': _shape(2, 5, 12, 40, 3, 4, 1),        # scatter kernel, forced
    'tiny_strided': _shape(2, 5, 12, 40, 3, 4, 2),
    'tiny_csf8': _shape(2, 5, 16, 48, 9, 4, 8, center=True),
    'rows3': _shape(1, 4, 3, 64, 3, 4, 1),              # h_in < 4: no LDS slab of four rows
    'wide2560': _shape(1, 2, 4, 2560, 2, 1, 1),         # four rows of 2560 do not fit the LDS budget
    'dense': _shape(2, 6, 23, 61, 5, 4, 1),             # tile kernel: hw = 1403 (no multiple of 256), C = 4 + 2
    'dense8': _shape(1, 8, 12, 40, 4, 4, 1),            # ... channels-last gradient volumes: whole 16-byte runs
    'deep33': _shape(1, 3, 10, 48, 33, 4, 1),           # several depth chunks, a partial last one
    'wide1280': _shape(1, 4, 8, 1280, 3, 1, 1),         # two-channel passes (CW = 2)
    'wide1280_csf4': _shape(1, 4, 8, 1280, 6, 1, 4),    # ... two bands per lattice row
    'strided8': _shape(2, 8, 32, 128, 7, 1, 4, center=True),   # tile kernel, strided lattice
    'strided8_csf8': _shape(2, 8, 32, 128, 7, 1, 8, center=True),
    'k32': _shape(2, 32, 64, 256, 11, 1, 4),            # window and gather kernels: config K in small
    'k32_csf2': _shape(2, 32, 32, 128, 5, 1, 2),
    'k32_csf8': _shape(2, 32, 64, 256, 11, 1, 8),
    'k64_csf2': _shape(1, 64, 20, 64, 5, 1, 2),
    'k32_partial': _shape(1, 32, 20, 64, 6, 1, 4, center=True),   # 5 x 16 lattice: the last workgroup holds one tile of four
    'k64_csf8': _shape(1, 64, 40, 128, 9, 1, 8, center=True),   # 5 x 16 lattice at cost_sample_factor 8
    'k64_partial_csf2': _shape(1, 64, 10, 32, 4, 1, 2),  # 5 x 16 lattice, overlapping windows
}

# problem name -> (geometry, shape)
PROBLEMS = {}
for _g in ('plain', 'aug', 'batch2', 'forward', 'zplane', 'outside'):
    PROBLEMS[f'tiny_dense-{_g}'] = (_g, 'tiny_dense')
    PROBLEMS[f'tiny_strided-{_g}'] = (_g, 'tiny_strided')
    PROBLEMS[f'dense-{_g}'] = (_g, 'dense')
    PROBLEMS[f'strided8-{_g}'] = (_g, 'strided8')
    PROBLEMS[f'k32-{_g}'] = (_g, 'k32')
PROBLEMS['tiny_csf8-scale103'] = ('scale103', 'tiny_csf8')
PROBLEMS['strided8_csf8-scale103'] = ('scale103', 'strided8_csf8')
PROBLEMS['k32_csf8-scale103'] = ('scale103', 'k32_csf8')
PROBLEMS['rows3-lateral'] = ('lateral', 'rows3')
PROBLEMS['wide2560-lateral'] = ('lateral', 'wide2560')
PROBLEMS['dense8-aug'] = ('aug', 'dense8')
PROBLEMS['deep33-plain'] = ('plain', 'deep33')
PROBLEMS['deep33-aug'] = ('aug', 'deep33')
PROBLEMS['wide1280-lateral'] = ('lateral', 'wide1280')
PROBLEMS['wide1280-aug'] = ('aug', 'wide1280')
PROBLEMS['wide1280_csf4-aug'] = ('aug', 'wide1280_csf4')
PROBLEMS['k32_csf2-plain'] = ('plain', 'k32_csf2')
PROBLEMS['k32_csf2-aug'] = ('aug', 'k32_csf2')
PROBLEMS['k64_csf2-aug'] = ('aug', 'k64_csf2')
PROBLEMS['k32_partial-plain'] = ('plain', 'k32_partial')
PROBLEMS['k64_csf8-scale103'] = ('scale103', 'k64_csf8')
PROBLEMS['k64_partial_csf2-aug'] = ('aug', 'k64_partial_csf2')

IMG_SHAPE = (375, 1242)


@functools.lru_cache(maxsize=None)
def problem(name):
    """the inputs of one problem: shape, camera geometry and the gradient volume (B, 2C, D, h_out, w_out), fp32 with
    full mantissas (``gout``) and rounded to bf16 (``gout16``: exact in both dtypes).  Cached; do not modify."""
    geom, shape = PROBLEMS[name]
    k = dict(SHAPES[shape])
    k.update(_geometry(geom, k))
    k['name'], k['geom'], k['img_shape'] = name, geom, IMG_SHAPE
    k['h_out'], k['w_out'] = round(k['H'] / k['csf']), round(k['W'] / k['csf'])   # dfm_backbone.py:242-243
    k['Pinv'] = util.host_inverse(k['P'])
    rng = np.random.RandomState(sum(name.encode()) % 10007)
    k['gout'] = rng.randn(k['B'], 2 * k['C'], k['D'], k['h_out'], k['w_out']).astype(np.float32)
    k['gout16'] = orc.bf16_round(k['gout'])
    for a in ('gout', 'gout16', 'P', 'T', 'Pinv', 'depths'):
        k[a].setflags(write=False)
    return k


def grids(k, b):
    """the oracle's normalised fp32 grids of sample b: (cur (N, 2), prev (N, 2)), N = D * h_out * w_out"""
    prm = orc.sweep_params(k['H'], k['W'], k['D'], k['fsf'], k['csf'], k['P'][b], k['Pinv'][b], k['T'][b],
                           k['img_shape'], k['flip'], k['crop'], k['scale'])
    return orc.plane_sweep_grid(prm, k['depths'])


@functools.lru_cache(maxsize=None)
def reference(name, bf16=False):
    """fp64 gradients of both maps for one problem: dict of ``grad``, ``A`` (2, B, C, H, W) f64 -- index 0 the cur
    map, 1 the prev map -- ``n`` (2, B, H, W) and ``oob`` (2,) (taps outside the map).  Asserts the input
    conditions every backward test relies on, so that no test passes on an empty problem.  Cached; read-only."""
    k = problem(name)
    B, C, H, W = k['B'], k['C'], k['H'], k['W']
    gout = (k['gout16'] if bf16 else k['gout']).astype(np.float64)
    grad = np.zeros((2, B, C, H, W), np.float64)
    A = np.zeros((2, B, C, H, W), np.float64)
    n = np.zeros((2, B, H, W), np.int64)
    oob = np.zeros(2, np.int64)
    for b in range(B):
        for half, grid in enumerate(grids(k, b)):
            x, y = positions(grid, H, W)
            g = gout[b, half * C:(half + 1) * C].reshape(C, -1)
            grad[half, b], A[half, b], n[half, b], o = adjoint(x, y, g, H, W)
            oob[half] += o
    ref = dict(grad=grad, A=A, n=n, oob=oob)
    check_input_conditions(k, ref)
    for a in ref.values():
        a.setflags(write=False)
    return ref


def check_input_conditions(k, ref):
    """a problem is worth running when the gradient is not small, a good part of the prev map receives something
    (none of it in the case built to be all outside) and both maps have taps that fall off the map"""
    name = k['name']
    covered = float((ref['n'][1] > 0).mean())
    if k['geom'] == 'outside':
        assert covered == 0.0 and float(np.abs(ref['grad'][1]).max()) == 0.0, name
    else:
        assert covered >= 0.2, f'{name}: only {covered:.3f} of the prev map receives a contribution'
        assert float(np.abs(ref['grad'][1]).max()) > 0.1, name
    assert float(np.abs(ref['grad'][0]).max()) > 0.1, name
    assert ref['oob'][0] >= 1 and ref['oob'][1] >= 1, f'{name}: out-of-bounds taps (cur, prev) = {tuple(ref["oob"])}'
