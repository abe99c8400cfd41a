"""Shared by tests/test_kitti_eval.py and tests/test_kitti_eval_gpu.py: the fixture tests/golden/kitti_eval.npz
(generator: tests/golden/make_golden_kitti_eval.py) turned back into the annotation lists ``kitti_eval`` takes."""
import os

import numpy as np

from tests import util

PATH = os.path.join(util.GOLDEN, 'kitti_eval.npz')
CLASSES = ['Car', 'Pedestrian', 'Cyclist']
# (scene, variant) -> (current_classes, eval_types, alpha override)
VARIANTS = {('val24', 'all'): (CLASSES, ['bbox', 'bev', '3d', 'aos'], None),
            ('val24', 'car'): (['Car'], ['bbox', 'bev', '3d', 'aos'], None),
            ('val24', 'noaos'): (CLASSES, ['bbox', 'bev', '3d'], -10.0),
            ('edge', 'all'): (CLASSES, ['bbox', 'bev', '3d', 'aos'], None),
            ('single', 'all'): (CLASSES, ['bbox', 'bev', '3d', 'aos'], None)}
SCENES = ('val24', 'edge', 'single')
MIN_OVERLAPS = {0: (0.7, 0.5), 1: (0.7, 0.5, 0.25), 2: (0.7, 0.5, 0.25)}
GT_KEYS = ('name', 'bbox', 'location', 'dimensions', 'rotation_y', 'alpha', 'occluded', 'truncated')
DT_KEYS = GT_KEYS + ('score',)

_Z = None


def fixture():
    global _Z
    if _Z is None:
        with np.load(PATH) as z:
            _Z = {k: z[k] for k in z.files}
    return _Z


def annos(scene, alpha=None, frames=None):
    """(gt_annos, dt_annos) of a scene: lists of per-frame dicts of arrays"""
    z = fixture()
    out = []
    for side, keys in (('gt', GT_KEYS), ('dt', DT_KEYS)):
        off = np.concatenate([[0], np.cumsum(z[f'{scene}/{side}_num'])])
        lst = []
        for f in range(len(off) - 1):
            a = {k: z[f'{scene}/{side}_{k}'][off[f]:off[f + 1]].copy() for k in keys}
            if alpha is not None:
                a['alpha'] = np.full_like(a['alpha'], alpha)
            lst.append(a)
        out.append(lst[:frames] if frames else lst)
    return out[0], out[1]


def kitti_min_overlaps(num_classes=3):
    """the [2, 3, class] array kitti_eval builds for Car, Pedestrian, Cyclist"""
    strict = np.array([[0.7, 0.5, 0.5]] * 3)
    loose = np.array([[0.7, 0.5, 0.5], [0.5, 0.25, 0.25], [0.5, 0.25, 0.25]])
    return np.stack([strict, loose], 0)[:, :, :num_classes]
