"""tests/golden/depth_targets.npz read once for tests/test_depth_targets.py and tests/test_depth_targets_gpu.py: the
cases by name, their sparse maps made dense.  The arrays are shared between the tests and never written to."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'depth_targets.npz')
SINGLE = ('random', 'exact', 'empty/none', 'empty/no_points', 'empty/no_boxes', 'config')
BATCH = ('batch/0', 'batch/1', 'batch/2')


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def case(key):
    """dict(points, boxes, P, cam2img, img_shape, pad_shape, depth (H, W) float32, mask (H, W) int32) of one sample"""
    z = fixture()
    c = {k: z[f'{key}/{k}'] for k in ('points', 'boxes', 'P', 'cam2img')}
    c['img_shape'] = tuple(int(v) for v in z[f'{key}/img_shape'])
    c['pad_shape'] = tuple(int(v) for v in z[f'{key}/pad_shape'])
    h, w = c['pad_shape'][:2]
    bits = np.zeros(h * w, dtype=np.uint32)
    bits[z[f'{key}/depth_idx']] = z[f'{key}/depth_bits']
    mask = np.zeros(h * w, dtype=np.int32)
    mask[z[f'{key}/mask_idx']] = z[f'{key}/mask_val']
    c['depth'], c['mask'] = bits.view(np.float32).reshape(h, w), mask.reshape(h, w)
    return c


def same_bits(a, b):
    """two float32 arrays hold the same bit patterns (a NaN equals itself, -0 differs from 0)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and \
        np.array_equal(a.view(np.uint32), b.view(np.uint32))
