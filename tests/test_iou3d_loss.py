"""CPU: the differentiable rotated IoU / IOU3DLoss above the kernels -- the fixture's fp64 values against overlaps
computed by hand, properties of its stored gradients, the exported names, the registry entry, the C ABI's symbols
and argument checks, the refusal of CPU tensors and patch_reference's rebinding.

Fixture numbers (tests/golden/iou3d.npz, generator tests/golden/make_golden_iou3d.py): over every pair of every
scene the fp32 CPU run of the stand-in differs from its fp64 run by at most ``fp32_iou_error`` = 2.8e-7 in the
IoU and ``fp32_grad_error`` = 6.3e-6 in a gradient component; decode + loss from fp32 deltas by
``fp32_head_loss_error`` = 7.0e-6 and ``fp32_head_grad_error`` = 1.24e-4.  The GPU tests read these four."""
import ctypes
import importlib
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
NEW = ('dfm_diff_iou_rotated', 'dfm_iou3d_loss_from_deltas')
NAMES = ('diff_iou_rotated_3d', 'diff_iou_rotated_2d', 'iou3d_loss', 'IOU3DLoss', 'iou3d_loss_from_deltas')


@pytest.fixture(scope='module')
def pkg():
    importlib.import_module('depth-from-motion_amd.build').build_hip()
    return importlib.import_module('depth-from-motion_amd')


@pytest.fixture(scope='module')
def z():
    return np.load(os.path.join(util.GOLDEN, 'iou3d.npz'))


def special(z, box1, box2):
    """the stored fp64 IoU of the special pair with these boxes"""
    b1, b2 = z['special/boxes1'], z['special/boxes2']
    hit = np.all(b1 == np.asarray(box1, np.float32), 1) & np.all(b2 == np.asarray(box2, np.float32), 1)
    assert hit.sum() == 1, (box1, box2)
    return float(z['special/iou'][hit][0])


def test_stored_values_match_hand_computed_overlaps(z):
    # unit cubes offset by half a side: intersection 1/2, union 3/2
    assert abs(special(z, [0, 0, 0, 1, 1, 1, 0], [0.5, 0, 0, 1, 1, 1, 0]) - 1 / 3) < 1e-15
    # a unit square over itself turned by 45 degrees: a regular octagon of inradius 1/2, area 2 (sqrt 2 - 1)
    # (pi / 4 is stored in fp32: the angle is off by 2.2e-8, the area by less than that)
    A = 2 * (math.sqrt(2) - 1)
    assert abs(special(z, [0, 0, 0, 1, 1, 1, 0], [0, 0, 0, 1, 1, 1, math.pi / 4]) - A / (2 - A)) < 1e-7
    # half z overlap of equal boxes: W = V / 2, IoU = (V / 2) / (3 V / 2)
    assert abs(special(z, [0, 0, 0, 2, 2, 2, 0.3], [0, 0, 1, 2, 2, 2, 0.3]) - 1 / 3) < 1e-15
    # containment: a cube of side 2 inside one of side 4
    assert abs(special(z, [0, 0, 0, 4, 4, 4, 0.3], [0, 0, 0, 2, 2, 2, 0.3]) - 1 / 8) < 1e-15
    # a diamond inscribed in a square covers half of it (sqrt 2 and pi / 4 in fp32)
    s2 = math.sqrt(2)
    assert abs(special(z, [0, 0, 0, s2, s2, 1, math.pi / 4], [0, 0, 0, 2, 2, 1, 0]) - 0.5) < 1e-6
    # identical boxes; touching, disjoint and empty boxes are exactly 0
    assert abs(special(z, [10, 5, -1, 3.9, 1.6, 1.56, 0.3], [10, 5, -1, 3.9, 1.6, 1.56, 0.3]) - 1) < 1e-14
    assert special(z, [40, 10, 0, 2, 2, 2, 0], [42, 10, 0, 2, 2, 2, 0]) == 0.0
    assert special(z, [5, 5, 0, 3.9, 1.6, 1.5, 0.2], [5.3, 5.1, 1.5, 3.9, 1.6, 1.5, 0.4]) == 0.0
    assert special(z, [5, 5, 0, 3.9, 1.6, 1.5, 0.2], [15, 5, 0, 3.9, 1.6, 1.5, 0.4]) == 0.0
    assert special(z, [5, 5, 0, 0, 1.6, 1.5, 0.2], [5, 5, 0, 3.9, 1.6, 1.5, 0.2]) == 0.0
    assert int((z['special/iou'] == 0).sum()) >= 8


@pytest.mark.parametrize('scene', ['general', 'aligned'])
def test_stored_gradients_are_translation_invariant(z, scene):
    g1, g2, iou = z[f'{scene}/grad1'], z[f'{scene}/grad2'], z[f'{scene}/iou']
    assert g1.shape == g2.shape == (len(iou), 7) and g1.dtype == np.float64
    assert np.abs(g1[:, :3] + g2[:, :3]).max() < 1e-12          # moving both boxes together changes nothing
    assert np.abs(g1).max() > 1.0 and (iou > 0).mean() > 0.75
    assert np.all(g1[iou == 0] == 0) and np.all(g2[iou == 0] == 0)
    if scene == 'general':
        # rotating both boxes about any point changes nothing either: about the origin,
        # sum over the two boxes of (x g_y - y g_x + g_yaw) = 0
        b1, b2 = z['general/boxes1'].astype(np.float64), z['general/boxes2'].astype(np.float64)
        rot = sum(b[:, 0] * g[:, 1] - b[:, 1] * g[:, 0] + g[:, 6] for b, g in ((b1, g1), (b2, g2)))
        assert np.abs(rot).max() < 1e-10
        assert len(iou) == 1024 and np.abs(b1[:, :2]).max() > 70
        # every yaw quadrant
        assert set(np.floor(b1[:, 6] / (np.pi / 2)).astype(int)) == {-2, -1, 0, 1}
    else:
        assert np.array_equal(z['aligned/boxes1'][:, 6], z['aligned/boxes2'][:, 6]) and len(iou) == 64


def test_stored_error_figures(z):
    for key in ('fp32_iou_error', 'fp32_grad_error', 'fp32_head_loss_error', 'fp32_head_grad_error'):
        v = float(z[key])
        assert 0 < v < 1e-3 and math.isfinite(v), key
    assert float(z['fp32_iou_error']) <= 2.9e-7 and float(z['fp32_grad_error']) <= 6.4e-6   # the docstrings' numbers
    assert float(z['guard']) == 1e-3
    assert os.path.getsize(os.path.join(util.GOLDEN, 'iou3d.npz')) < 512 * 1024


def test_head_cases_are_stored_whole(z):
    R = z['head/anchors'].shape[0]
    assert R == 600 and z['head/bbox_pred'].shape == (R, 7)
    for case, P in (('p257', 257), ('p1', 1), ('p0', 0), ('nan', 257)):
        pos = z[f'head/{case}/pos_inds']
        assert pos.shape == (P,) and pos.dtype == np.int64 and len(np.unique(pos)) == P
        assert z[f'head/{case}/loss_rows'].shape == (P,) and z[f'head/{case}/grad_rows'].shape == (R, 7)
        rest = np.setdiff1d(np.arange(R), pos)
        assert np.all(z[f'head/{case}/grad_rows'][rest] == 0) and np.all(z[f'head/{case}/grad_reduced'][rest] == 0)
        # the reduced loss is the per-row sum over the tensor avg_factor
        assert abs(z[f'head/{case}/loss_rows'].sum() / z[f'head/{case}/avg_factor'] - z[f'head/{case}/loss_reduced']) < 1e-12
    assert float(z['head/p0/loss_reduced']) == 0.0
    nan = np.isnan(z['head/nan/bbox_targets'])
    assert nan.sum() > 150 and not np.isnan(z['head/p257/bbox_targets']).any()
    assert np.isfinite(z['head/nan/loss_rows']).all() and np.isfinite(z['head/nan/grad_rows']).all()


def test_names_are_exported(pkg):
    for name in NAMES:
        assert callable(getattr(pkg, name)) and name in pkg.__all__, name
    mod = importlib.import_module('depth-from-motion_amd.iou3d_loss')
    assert set(NAMES) == set(mod.__all__)


def test_registry_builds_the_configs_loss(pkg):
    reg = importlib.import_module('depth-from-motion_amd.registry')
    loss = reg.build(dict(type='IOU3DLoss', loss_weight=1.0))     # the KITTI configs' loss_iou
    assert isinstance(loss, pkg.IOU3DLoss) and loss.reduction == 'mean' and loss.loss_weight == 1.0
    assert reg.build(dict(type='IOU3DLoss', reduction='sum', loss_weight=0.5)).reduction == 'sum'
    with pytest.raises(AssertionError):
        reg.build(dict(type='IOU3DLoss', reduction='median'))
    # a loss is no stage of the feature path: enable_fast_path does not convert around it
    assert pkg.IOU3DLoss not in reg.path_classes() and reg.registered()['DfMBackbone'] in reg.path_classes()


def test_header_binding_and_library_agree_on_the_new_symbols(pkg):
    text = open(os.path.join(ROOT, 'include', 'dfm_hip.h')).read()
    declared = set(re.findall(r'DFM_API\s+[\w\s\*]+?\b(dfm_\w+)\s*\(', text))
    h = ctypes.CDLL(pkg._capi.LIB_PATH)
    for name in NEW:
        assert name in declared, f'{name} not declared in dfm_hip.h'
        assert name in pkg._capi.EXPORTS, f'{name} not in _capi.EXPORTS'
        assert hasattr(h, name), f'{name} not exported by the library'
    assert pkg._capi.lib().dfm_version() == 3
    for phrase in ('z - dz / 2', 'I Z / (V1 + V2 - I Z)', 'counter-clockwise', '1e-14'):
        assert phrase in text, phrase                             # the semantics are stated in the header


def test_bad_arguments_are_rejected_without_touching_the_gpu(pkg):
    lib = pkg._capi.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    # (boxes1, boxes2, n, width, iou, grad1, grad2, stream)
    iou = lib.dfm_diff_iou_rotated
    assert iou(None, None, -1, 7, None, None, None, None) == -1
    assert iou(None, None, 4, 6, None, None, None, None) == -1       # width 7 or 5
    assert b'width' in lib.dfm_last_error()
    for width in (5, 7):
        assert iou(None, None, 0, width, None, None, None, None) == 0    # n = 0: a valid no-op, pointers not looked at
        assert iou(None, None, 4, width, None, None, None, None) == -1
        assert b'NULL' in lib.dfm_last_error()
        assert iou(p, None, 4, width, p, None, None, None) == -1
    assert iou(p, p, 4, 7, p, p, None, None) == -1                   # one gradient pointer without the other
    assert b'together' in lib.dfm_last_error()
    # (anchors, bbox_pred, bbox_targets, pos_inds, num_rows, code_size, num_pos, loss, jac, stream)
    fused = lib.dfm_iou3d_loss_from_deltas
    assert fused(None, None, None, None, -1, 7, 4, None, None, None) == -1
    assert fused(None, None, None, None, 8, 7, -1, None, None, None) == -1
    assert fused(None, None, None, None, 8, 6, 4, None, None, None) == -1
    assert b'code_size' in lib.dfm_last_error()
    assert fused(None, None, None, None, 8, 7, 0, None, None, None) == 0     # no positives: a valid no-op
    assert fused(None, None, None, None, 8, 9, 4, None, None, None) == -1
    assert b'NULL' in lib.dfm_last_error()
    assert fused(p, p, p, None, 8, 7, 4, p, None, None) == -1


def test_cpu_tensors_are_refused(pkg):
    b = torch.zeros(1, 4, 7)
    rows, pos = torch.zeros(4, 7), torch.zeros(2, dtype=torch.int64)
    for call in (lambda: pkg.diff_iou_rotated_3d(b, b), lambda: pkg.diff_iou_rotated_2d(b[..., :5], b[..., :5]),
                 lambda: pkg.iou3d_loss(rows, rows), lambda: pkg.IOU3DLoss()(rows, rows),
                 lambda: pkg.iou3d_loss_from_deltas(rows, rows, rows, pos)):
        with pytest.raises(RuntimeError, match='no CPU path'):
            call()


def test_patch_reference_rebinds_the_loaded_loss_module(pkg):
    """the reference's iou3d_loss.py holds mmcv's op by name; it is rebound where the module is already
    imported, and never imported for it"""
    name = 'mmdet3d.models.losses.iou3d_loss'
    chain = ('mmdet3d', 'mmdet3d.models', 'mmdet3d.models.losses', name)
    before = {k: sys.modules.get(k) for k in chain}
    old = lambda *a, **k: None  # noqa: E731
    integ = importlib.import_module('depth-from-motion_amd.integration')
    try:
        for k in chain:
            sys.modules.pop(k, None)
        nothing = {'modules': [], 'functions': [], 'methods': []}
        assert integ.apply_patches('iou') == nothing and name not in sys.modules
        for k in chain:
            m = types.ModuleType(k)
            m.__path__ = []
            sys.modules[k] = m
        sys.modules[name].diff_iou_rotated_3d = old
        done = integ.apply_patches('iou')                         # what patch_reference adds to its report
        assert done == dict(nothing, functions=[name + '.diff_iou_rotated_3d'])
        assert sys.modules[name].diff_iou_rotated_3d is pkg.diff_iou_rotated_3d
        assert not hasattr(sys.modules['mmdet3d.models.losses'], 'diff_iou_rotated_3d')
    finally:
        for k, v in before.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
