"""CPU: BEV NMS / rotated IoU above the kernels -- the C ABI's symbols, argument checks, workspace formula and
cap; the refusal of CPU tensors; patch_reference's rebinding; and the fp64 numpy stand-in of the fixture
generator (tests/golden/make_golden_box_nms.py) against overlaps computed by hand.

Fixture numbers (tests/golden/box_nms.npz): over every pair of every scene the numpy float32 run of the IoU
algorithm differs from the fp64 run by at most ``fp32_iou_error`` = 7.2e-7; no pair's fp64 IoU lies within
``guard_band`` = 1e-4 of the NMS threshold (>= 4 x the error: 1e-4 is 139 x)."""
import ctypes
import importlib
import importlib.util
import math
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('dfm_box_nms_workspace_bytes', 'dfm_box_nms_rotated', 'dfm_box_nms_aligned', 'dfm_box_iou_rotated')


@pytest.fixture(scope='module')
def pkg():
    importlib.import_module('depth-from-motion_amd.build').build_hip()
    return importlib.import_module('depth-from-motion_amd')


@pytest.fixture(scope='module')
def gen():
    """the generator module (its numpy stand-in); nothing in it touches the reference at import"""
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    try:
        spec = importlib.util.spec_from_file_location('make_golden_box_nms',
                                                      os.path.join(util.GOLDEN, 'make_golden_box_nms.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.pop(0)
    return mod


def test_header_binding_and_library_agree_on_the_new_symbols(pkg):
    text = open(os.path.join(ROOT, 'include', 'dfm_hip.h')).read()
    declared = set(re.findall(r'DFM_API\s+[\w\s\*]+?\b(dfm_\w+)\s*\(', text))
    h = ctypes.CDLL(pkg._capi.LIB_PATH)
    for name in NEW:
        assert name in declared, f'{name} not declared in dfm_hip.h'
        assert name in pkg._capi.EXPORTS, f'{name} not in _capi.EXPORTS'
        assert hasattr(h, name), f'{name} not exported by the library'
    assert int(re.search(r'#define\s+DFM_BOX_NMS_MAX_N\s+(\d+)', text).group(1)) == pkg._capi.BOX_NMS_MAX_N
    assert pkg._capi.lib().dfm_version() == 3
    for name in ('nms_bev', 'nms_normal_bev', 'box3d_multiclass_nms', 'box_iou_rotated'):
        assert callable(getattr(pkg, name)) and name in pkg.__all__


def test_workspace_formula_and_cap(pkg):
    lib = pkg._capi.lib()
    cap = pkg._capi.BOX_NMS_MAX_N
    for n, c in ((1, 1), (64, 1), (65, 2), (4096, 3), (cap, 1), (cap, 32)):
        assert lib.dfm_box_nms_workspace_bytes(n, c) == c * n * ((n + 63) // 64) * 8
    assert cap * ((cap + 63) // 64) * 8 * 32 == 1 << 30          # the largest mask: exactly 1 GiB
    assert lib.dfm_box_nms_workspace_bytes(0, 3) == 0
    assert lib.dfm_box_nms_workspace_bytes(cap + 1, 1) == 0
    assert str(cap).encode() in lib.dfm_last_error()
    assert lib.dfm_box_nms_workspace_bytes(cap, 33) == 0         # above 1 GiB
    assert b'1 GiB' in lib.dfm_last_error()
    assert lib.dfm_box_nms_workspace_bytes(-1, 1) == 0
    assert lib.dfm_box_nms_workspace_bytes(8, 0) == 0


def test_bad_arguments_are_rejected_without_touching_the_gpu(pkg):
    lib = pkg._capi.lib()
    cap = pkg._capi.BOX_NMS_MAX_N
    null = (None,) * 2
    # (boxes, num_boxes, [xyxyr,] order, counts, n, classes, thr, keep, kept_counts, workspace, bytes, stream)
    rot = lambda nb, n, c: lib.dfm_box_nms_rotated(None, nb, 1, *null, n, c, 0.25, None, None, None, 0, None)  # noqa: E731
    ali = lambda nb, n, c: lib.dfm_box_nms_aligned(None, nb, *null, n, c, 0.25, None, None, None, 0, None)  # noqa: E731
    for fn in (rot, ali):
        assert fn(8, 8, 0) == -1                                  # no class
        assert fn(8, -1, 1) == -1
        assert fn(-1, 8, 1) == -1
        assert fn(8, 0, 1) == 0                                   # n = 0: a valid no-op, pointers not looked at
        assert fn(8, 8, 1) == -1                                  # NULL pointers
        assert b'NULL' in lib.dfm_last_error()
        assert fn(cap + 1, cap + 1, 1) == pkg._capi.DFM_ERR_UNSUPPORTED
        assert str(cap).encode() in lib.dfm_last_error()
        assert fn(cap, cap, 33) == pkg._capi.DFM_ERR_UNSUPPORTED
    # a workspace that is too small: non-NULL host addresses are never dereferenced before the size check
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.dfm_box_nms_rotated(p, 8, 1, p, p, 8, 1, 0.25, p, p, p, 63, None) == -3
    assert b'64' in lib.dfm_last_error()
    iou = lib.dfm_box_iou_rotated
    assert iou(None, -1, None, 2, 0, None, None) == -1
    assert iou(None, 2, None, 3, 1, None, None) == -1            # aligned with different counts
    assert iou(None, 0, None, 3, 0, None, None) == 0             # empty: a valid no-op
    assert iou(None, 2, None, 2, 0, None, None) == -1
    assert b'NULL' in lib.dfm_last_error()


def test_cpu_tensors_are_refused(pkg):
    b, s = torch.zeros(4, 5), torch.zeros(4)
    for call in (lambda: pkg.nms_bev(b, s, 0.25), lambda: pkg.nms_normal_bev(b, s, 0.25),
                 lambda: pkg.box_iou_rotated(b, b),
                 lambda: pkg.box3d_multiclass_nms(b, b, torch.zeros(4, 4), 0.1, 10,
                                                  dict(use_rotate_nms=True, nms_thr=0.25))):
        with pytest.raises(RuntimeError, match='no CPU path'):
            call()


def test_patch_reference_rebinds_only_loaded_modules(pkg):
    """modules that hold the three functions are rebound where already imported, and never imported for it
    (box3d_nms.py needs numba and mmcv.ops)"""
    names = ('mmdet3d', 'mmdet3d.core', 'mmdet3d.core.post_processing', 'mmdet3d.core.post_processing.box3d_nms',
             'mmdet3d.models', 'mmdet3d.models.dense_heads', 'mmdet3d.models.dense_heads.anchor3d_head')
    before = {k: sys.modules.get(k) for k in names}
    old = lambda *a, **k: None  # noqa: E731
    try:
        for k in names:
            m = types.ModuleType(k)
            m.__path__ = []
            sys.modules[k] = m
        del sys.modules['mmdet3d.core']                           # one holder that is NOT loaded
        for k in ('mmdet3d.core.post_processing.box3d_nms', 'mmdet3d.core.post_processing'):
            for f in ('box3d_multiclass_nms', 'nms_bev', 'nms_normal_bev'):
                setattr(sys.modules[k], f, old)
        sys.modules['mmdet3d.models.dense_heads.anchor3d_head'].box3d_multiclass_nms = old
        integ = importlib.import_module('depth-from-motion_amd.integration')
        done = integ.apply_patches('nms')                         # what patch_reference adds to its report
        assert done['modules'] == [] and done['methods'] == []
        done = done['functions']
        assert sys.modules['mmdet3d.core.post_processing.box3d_nms'].nms_bev is pkg.nms_bev
        assert sys.modules['mmdet3d.core.post_processing'].nms_normal_bev is pkg.nms_normal_bev
        head = sys.modules['mmdet3d.models.dense_heads.anchor3d_head']
        assert head.box3d_multiclass_nms is pkg.box3d_multiclass_nms and not hasattr(head, 'nms_bev')
        assert 'mmdet3d.core' not in sys.modules
        assert len(done) == 7 and 'mmdet3d.core.post_processing.box3d_nms.nms_bev' in done
    finally:
        for k, v in before.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_stand_in_reproduces_hand_computed_overlaps(gen):
    iou = lambda a, b, dt=np.float64: float(gen.rbox_iou(np.array([a]), np.array([b]), dt)[0])  # noqa: E731
    # unit squares offset by half a side: intersection 1/2, union 3/2
    assert abs(iou([0, 0, 1, 1, 0], [0.5, 0, 1, 1, 0]) - 1 / 3) < 1e-15
    assert abs(iou([70, -30, 1, 1, 0.0], [70, -29.5, 1, 1, math.pi / 2]) - 1 / 3) < 1e-13
    # a square of side 4 over the same square turned by 45 degrees: a regular octagon of inradius 2,
    # area 8 r^2 tan(pi/8) = 32 (sqrt 2 - 1); IoU = A / (32 - A)
    A = 32 * (math.sqrt(2) - 1)
    assert abs(iou([0, 0, 4, 4, 0], [0, 0, 4, 4, math.pi / 4]) - A / (32 - A)) < 1e-14
    assert abs(iou([0, 0, 4, 4, math.pi / 4], [0, 0, 4, 4, 0]) - A / (32 - A)) < 1e-14
    # identical, contained, edge-touching, disjoint, zero-area
    assert iou([3, 4, 2, 1, 0.7], [3, 4, 2, 1, 0.7]) == pytest.approx(1.0, abs=1e-14)
    assert abs(iou([0, 0, 4, 4, 0.3], [0, 0, 2, 2, 0.3]) - 0.25) < 1e-14
    assert iou([0, 0, 2, 2, 0], [2, 0, 2, 2, 0]) == 0.0
    assert iou([0, 0, 2, 2, 0], [9, 0, 2, 2, 1.0]) == 0.0
    assert iou([0, 0, 0, 2, 0], [0, 0, 2, 2, 0]) == 0.0
    # mirroring both boxes (the other sense of rotation) changes nothing
    a, b = [1.0, 2.0, 3.9, 1.6, 0.4], [1.8, 2.5, 3.0, 1.2, -1.1]
    am, bm = [1.0, -2.0, 3.9, 1.6, -0.4], [1.8, -2.5, 3.0, 1.2, 1.1]
    assert abs(iou(a, b) - iou(am, bm)) < 1e-14 and 0.1 < iou(a, b) < 0.9
    # the float32 run of the same code is close
    assert abs(iou(a, b, np.float32) - iou(a, b)) < 1e-6
    # axis-aligned
    ab = lambda p, q: float(gen.abox_iou(np.array([p]), np.array([q]))[0])  # noqa: E731
    assert abs(ab([0, 0, 1, 1], [0.5, 0, 1.5, 1]) - 1 / 3) < 1e-15
    assert ab([0, 0, 1, 1], [1, 0, 2, 1]) == 0.0 and ab([0, 0, 0, 1], [0, 0, 1, 1]) == 0.0


def test_stand_in_greedy_suppression(gen):
    """strictly greater; visited in descending score order; kept in that order"""
    boxes = torch.tensor([[0, 0, 4, 4, 0], [0, 0, 2, 2, 0], [10, 0, 2, 2, 0], [0.1, 0, 4, 4, 0]], dtype=torch.float32)
    scores = torch.tensor([0.5, 0.9, 0.7, 0.6])
    # IoU(0, 1) = 0.25 exactly: not suppressed at 0.25, suppressed just below
    assert gen.nms_rotated(boxes, scores, 0.25)[1].tolist() == [1, 2, 3]
    assert gen.nms_rotated(boxes, scores, 0.2499)[1].tolist() == [1, 2]


def test_fixture_is_decidable_in_fp32():
    z = np.load(os.path.join(util.GOLDEN, 'box_nms.npz'))
    err, band = float(z['fp32_iou_error']), float(z['guard_band'])
    assert 0 < err and band >= 4 * err
    assert err <= 7.2e-7 and band == 1e-4                          # the numbers the docstrings quote
