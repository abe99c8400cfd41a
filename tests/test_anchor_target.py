"""CPU: the anchor-target feature above the kernels -- the fixture's stored overlaps against box pairs computed by
hand, the fixture's cases, guards and error figures, the exported names, the registry entry, the C ABI's symbols and
argument checks, the refusal of CPU tensors and patch_reference's rebinding.

Fixture numbers (tests/golden/anchor_target.npz, generator tests/golden/make_golden_anchor_target.py): over every
overlap of every case the fp32 CPU run of the reference differs from its fp64 run by at most ``fp32_overlap_error``
= 2.2e-6 (pedestrian-sized boxes 20 m out: a coordinate's rounding, 1.9e-6 m, against a 0.6 m side) and in an
encoded target by ``fp32_target_error`` = 1.2e-7.  The GPU tests read these two."""
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
NEW = ('dfm_nearest_bev_overlaps', 'dfm_anchor_target_3d')
NAMES = ('bbox_overlaps_nearest_3d', 'BboxOverlapsNearest3D', 'anchor_target_3d', 'HipAnchorTrainMixin')
CASES = {'small': (180, [7]), 'posw': (180, [7]), 'odd': (378, [7]), 'batch': (8640, [9, 5]),
         'empty': (8640, [6, 0]), 'g70': (8640, [70]), 'shared': (8640, [7]), 'rules_all': (8640, [11]),
         'rules_first': (8640, [11])}


@pytest.fixture(scope='module')
def pkg():
    importlib.import_module('depth-from-motion_amd.build').build_hip()
    return importlib.import_module('depth-from-motion_amd')


@pytest.fixture(scope='module')
def z():
    return np.load(os.path.join(util.GOLDEN, 'anchor_target.npz'))


def test_stored_overlaps_match_hand_computed_pairs(z):
    b1, b2 = z['hand/boxes1'], z['hand/boxes2']
    iou, iof = z['hand/aligned_iou'], z['hand/aligned_iof']
    assert b1.shape == b2.shape == (8, 7) and iou.dtype == np.float64
    # 2 x 2 squares one metre apart: overlap 2, union 6; over the first box 2 / 4
    assert abs(iou[0] - 1 / 3) < 1e-15 and iof[0] == 0.5
    # yaw pi / 2: the 4 x 2 box becomes 2 x 4; against the same box unturned the overlap is 2 x 2 of 8 + 8 - 4
    assert abs(iou[1] - 1 / 3) < 1e-15 and iof[1] == 0.5
    # yaw 0.7 is below pi / 4 = 0.785: no swap, the boxes coincide; yaw 0.8 is above: the swap of pair 1
    assert iou[2] == 1.0 and abs(iou[3] - 1 / 3) < 1e-15
    # yaw pi + 0.1 is 0.1 after the period is taken off; -pi / 2 + 0.1 is 1.47: swapped, equal to the 2 x 4 box
    assert iou[4] == 1.0 and iou[7] == 1.0 and iof[7] == 1.0
    # disjoint boxes, and two empty boxes (0 / max(0, 1e-6))
    assert iou[5] == 0.0 and iou[6] == 0.0 and iof[6] == 0.0
    # the matrix holds the aligned values on its diagonal
    assert np.array_equal(np.diag(z['hand/iou']), iou) and np.array_equal(np.diag(z['hand/iof']), iof)
    assert z['overlaps/iou'].shape == (130, 37) and z['overlaps/aligned_iof'].shape == (37,)
    assert np.array_equal(np.diag(z['overlaps/iou'][:37]), z['overlaps/aligned_iou'])
    assert (z['overlaps/iou'] > 0).sum() > 37 and z['overlaps/iou'].max() <= 1.0


def test_stored_error_figures_and_guards(z):
    for key in ('fp32_overlap_error', 'fp32_target_error'):
        v = float(z[key])
        assert 0 < v < 1e-5 and math.isfinite(v), key
    assert float(z['fp32_overlap_error']) <= 2.3e-6 and float(z['fp32_target_error']) <= 1.2e-7   # the docstring's
    assert float(z['guard']) == 1e-5 and float(z['dir_guard']) == 1e-4
    assert z['thresholds'].tolist() == [[0.6, 0.45, 0.45], [0.5, 0.35, 0.35], [0.5, 0.35, 0.35]]
    assert os.path.getsize(os.path.join(util.GOLDEN, 'anchor_target.npz')) < 512 * 1024


@pytest.mark.parametrize('case', sorted(CASES))
def test_cases_are_stored_whole(z, case):
    A, G = CASES[case]
    B = len(G)
    assert np.diff(z[f'{case}/gt_offsets']).tolist() == G
    assert z[f'{case}/anchors'].shape[3:] == (3, 2, 7) and z[f'{case}/anchors'][0].size == A * 7
    assert z[f'{case}/gt_boxes'].shape == (sum(G), 7) and z[f'{case}/gt_labels'].dtype == np.int64
    labels, lw, bw, dw = (z[f'{case}/{k}'] for k in ('labels', 'label_weights', 'bbox_weights', 'dir_weights'))
    assert labels.shape == (B, A) and labels.dtype == np.int64 and z[f'{case}/dir_targets'].dtype == np.int64
    assert z[f'{case}/bbox_targets'].shape == (B, A, 7) and bw.shape == (B, A, 7)
    pos = bw[:, :, 0] > 0
    counts = z[f'{case}/counts']
    assert np.array_equal(counts[:, 0], pos.sum(1)) and np.array_equal(counts[:, 1], ((lw > 0) & ~pos).sum(1))
    assert int(z[f'{case}/num_total_pos']) == np.maximum(counts[:, 0], 1).sum()
    assert int(z[f'{case}/num_total_neg']) == np.maximum(counts[:, 1], 1).sum()
    # positives carry a class label and unit box / direction weights; everything else the background label
    assert np.all(labels[pos] < 3) and np.all(labels[~pos] == 3) and np.all(dw[pos] == 1) and np.all(dw[~pos] == 0)
    assert np.all(z[f'{case}/bbox_targets'][~pos] == 0) and set(np.unique(z[f'{case}/dir_targets'])) <= {0, 1}
    want = 2.0 if case == 'posw' else 1.0
    assert np.all(lw[pos] == want)


def test_cases_reach_every_branch(z):
    # an image without GT: everything negative; a class without GT in image 1 of 'batch'
    assert z['empty/counts'][1].tolist() == [0, 8640] and int(z['empty/num_total_pos']) == z['empty/counts'][0, 0] + 1
    second = z['batch/gt_labels'][z['batch/gt_offsets'][1]:]
    assert 2 not in second.tolist() and {0, 1} <= set(second.tolist())
    assert set(z['g70/gt_labels'].tolist()) == {0} and len(z['g70/gt_labels']) > 64   # more than one GT_CHUNK
    assert int(z['shared/assign_per_class']) == 0 and int(z['small/assign_per_class']) == 1
    # the tie: gt_max_assign_all assigns both anchors, without it only the first (two positives fewer / more)
    assert int(z['rules_all/gt_max_assign_all']) == 1 and int(z['rules_first/gt_max_assign_all']) == 0
    assert np.array_equal(z['rules_all/gt_boxes'], z['rules_first/gt_boxes'])
    all_pos, first_pos = z['rules_all/bbox_weights'][0, :, 0] > 0, z['rules_first/bbox_weights'][0, :, 0] > 0
    assert np.all(all_pos[first_pos]) and all_pos.sum() > first_pos.sum()
    # the ignore band is populated everywhere GT boxes are
    for case in CASES:
        assert (z[f'{case}/label_weights'][0] == 0).sum() > 0, case
    # yaws either side of pi / 4
    r = np.abs(z['rules_all/gt_boxes'][:, 6].astype(np.float64))
    assert np.any(np.abs(r - (np.pi / 4 - 0.02)) < 1e-6) and np.any(np.abs(r - (np.pi / 4 + 0.02)) < 1e-6)


def test_names_are_exported(pkg):
    for name in NAMES:
        assert callable(getattr(pkg, name)) and name in pkg.__all__, name
    mod = importlib.import_module('depth-from-motion_amd.anchor_target')
    assert set(NAMES) == set(mod.__all__)


def test_registry_builds_the_iou_calculator(pkg):
    reg = importlib.import_module('depth-from-motion_amd.registry')
    calc = reg.build(dict(type='BboxOverlapsNearest3D'))          # the KITTI configs' iou_calculator
    assert isinstance(calc, pkg.BboxOverlapsNearest3D) and calc.coordinate == 'lidar'
    with pytest.raises(AssertionError):
        reg.build(dict(type='BboxOverlapsNearest3D', coordinate='polar'))
    assert pkg.BboxOverlapsNearest3D not in reg.path_classes()


def test_header_binding_and_library_agree_on_the_new_symbols(pkg):
    text = open(os.path.join(ROOT, 'include', 'dfm_hip.h')).read()
    declared = set(re.findall(r'DFM_API\s+[\w\s\*]+?\b(dfm_\w+)\s*\(', text))
    h = ctypes.CDLL(pkg._capi.LIB_PATH)
    for name in NEW + ('dfm_anchor_target_workspace_bytes',):
        assert name in declared, f'{name} not declared in dfm_hip.h'
        assert name in pkg._capi.EXPORTS, f'{name} not in _capi.EXPORTS'
        assert hasattr(h, name), f'{name} not exported by the library'
    for phrase in ('floor(yaw / pi + 0.5) * pi', 'r > pi / 4', 'max(a1 + a2 - overlap, 1e-6)', 'max(a1, 1e-6)',
                   'LOWEST index', 'A later GT overrides'):
        assert phrase in text, phrase                             # the semantics are stated in the header
    # the descriptor's size follows the header: 13 ints, 1 float, 3 x 8 floats, 3 floats
    assert ctypes.sizeof(pkg._capi.AnchorTargetDesc) == 4 * (13 + 1 + 24 + 3)
    assert int(re.search(r'#define DFM_ANCHOR_TARGET_MAX_SLOTS (\d+)', text).group(1)) == pkg._capi.ANCHOR_TARGET_MAX_SLOTS
    assert int(re.search(r'#define DFM_ANCHOR_TARGET_MAX_BATCH (\d+)', text).group(1)) == pkg._capi.ANCHOR_TARGET_MAX_BATCH


def desc(pkg, **kw):
    d = pkg._capi.AnchorTargetDesc(num_locations=4, num_slots=3, num_rotations=2, box_width=7, batch=1,
                                   num_classes=3, has_labels=1, assign_per_class=1, match_low_quality=1,
                                   gt_max_assign_all=1, ignore_iof_thr=-1.0, pos_weight=-1.0)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_bad_arguments_are_rejected_without_touching_the_gpu(pkg):
    lib = pkg._capi.lib()
    buf = ctypes.create_string_buffer(256 + 16)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)      # 16-byte aligned host memory, never dereferenced
    # (boxes1, n, boxes2, m, width, mode, aligned, out, stream)
    ov = lib.dfm_nearest_bev_overlaps
    assert ov(None, -1, None, 4, 7, 0, 0, None, None) == -1
    assert ov(None, 4, None, 4, 6, 0, 0, None, None) == -1 and b'width' in lib.dfm_last_error()
    assert ov(None, 4, None, 4, 7, 2, 0, None, None) == -1 and b'mode' in lib.dfm_last_error()
    assert ov(None, 4, None, 5, 7, 0, 1, None, None) == -1 and b'aligned' in lib.dfm_last_error()
    assert ov(None, 0, None, 5, 9, 1, 0, None, None) == 0          # an empty set: a valid no-op
    assert ov(None, 4, None, 4, 7, 0, 0, None, None) == -1 and b'NULL' in lib.dfm_last_error()
    assert ov(p, 4, p, 4, 7, 0, 0, None, None) == -1
    # (desc, anchors, gt_boxes, gt_labels, gt_offsets, 6 outputs, counts, workspace, workspace_bytes, stream)
    at = lib.dfm_anchor_target_3d
    off = (ctypes.c_int32 * 2)(0, 2)
    outs = (p,) * 7

    def call(d, anchors=p, gt=p, labels=p, offsets=off, outputs=outs, ws=p, ws_bytes=256):
        return at(ctypes.byref(d) if d is not None else None, anchors, gt, labels, offsets, *outputs, ws, ws_bytes, None)
    unsupported = pkg._capi.DFM_ERR_UNSUPPORTED
    assert call(None) == -1
    assert call(desc(pkg, box_width=9)) == unsupported and b'width' in lib.dfm_last_error()
    assert call(desc(pkg, sampler=1)) == unsupported and b'sampler' in lib.dfm_last_error()
    assert call(desc(pkg, neg_iou_thr_is_range=1)) == unsupported and b'neg_iou_thr' in lib.dfm_last_error()
    assert call(desc(pkg, ignore_iof_thr=0.5, num_ignore_boxes=2)) == unsupported and b'ignore' in lib.dfm_last_error()
    assert call(desc(pkg, num_slots=9)) == unsupported and call(desc(pkg, batch=65)) == unsupported
    assert call(desc(pkg, num_slots=0)) == -1 and call(desc(pkg, num_locations=-1)) == -1
    assert call(desc(pkg, batch=0)) == 0 and call(desc(pkg, num_locations=0)) == 0      # nothing to do: no-ops
    assert call(desc(pkg), offsets=None) == -1
    assert call(desc(pkg), offsets=(ctypes.c_int32 * 2)(1, 2)) == -1
    assert call(desc(pkg), offsets=(ctypes.c_int32 * 2)(0, -1)) == -1
    assert call(desc(pkg), anchors=None) == -1 and b'NULL' in lib.dfm_last_error()
    assert call(desc(pkg), gt=None) == -1 and call(desc(pkg), labels=None) == -1
    assert call(desc(pkg), outputs=(p,) * 6 + (None,)) == -1
    assert call(desc(pkg, has_labels=0)) == -1 and b'assign_per_class' in lib.dfm_last_error()
    assert call(desc(pkg), ws=None) == -3 and call(desc(pkg), ws_bytes=8) == -3        # 3 slots x 2 GT x 8 bytes
    assert b'workspace' in lib.dfm_last_error()
    assert call(desc(pkg), ws=ctypes.c_void_p(p.value + 8)) == -1 and b'aligned' in lib.dfm_last_error()
    assert lib.dfm_anchor_target_workspace_bytes(3, 70) == 3 * 70 * 8
    assert lib.dfm_anchor_target_workspace_bytes(3, 0) == 0


def test_cpu_tensors_are_refused(pkg):
    boxes = torch.zeros(4, 7)
    anchors = torch.zeros(1, 2, 2, 3, 2, 7)
    cfg = dict(num_classes=3, assign_per_class=True, dir_offset=0.7854, dir_limit_offset=0, pos_weight=-1)
    assigners = [dict(pos_iou_thr=0.6, neg_iou_thr=0.45, min_pos_iou=0.45)] * 3
    for call in (lambda: pkg.bbox_overlaps_nearest_3d(boxes, boxes),
                 lambda: pkg.BboxOverlapsNearest3D()(boxes, boxes, 'iof', True),
                 lambda: pkg.anchor_target_3d(anchors, [boxes], [torch.zeros(4, dtype=torch.int64)], assigners, **cfg)):
        with pytest.raises(RuntimeError, match='no CPU path'):
            call()


def test_patch_reference_rebinds_a_stub_train_mixins_module(pkg):
    """AnchorTrainMixin.anchor_target_3d and bbox_overlaps_nearest_3d are rebound where their modules are already
    imported, and never imported for it; the replaced method is kept for the fallback policy"""
    mixins, calc = 'mmdet3d.models.dense_heads.train_mixins', 'mmdet3d.core.bbox.iou_calculators.iou3d_calculator'
    chain = ('mmdet3d', 'mmdet3d.models', 'mmdet3d.models.dense_heads', mixins, 'mmdet3d.core', 'mmdet3d.core.bbox',
             'mmdet3d.core.bbox.iou_calculators', calc)
    before = {k: sys.modules.get(k) for k in chain}
    integ = importlib.import_module('depth-from-motion_amd.integration')
    fb = importlib.import_module('depth-from-motion_amd.fallback')
    nothing = {'modules': [], 'functions': [], 'methods': []}
    kept = dict(fb.REPLACED)
    try:
        for k in chain:
            sys.modules.pop(k, None)
        assert integ.apply_patches('anchor_target') == nothing and mixins not in sys.modules
        for k in chain:
            m = types.ModuleType(k)
            m.__path__ = []
            sys.modules[k] = m

        class AnchorTrainMixin(object):
            def anchor_target_3d(self, *args):
                return 'reference', args
        original = AnchorTrainMixin.__dict__['anchor_target_3d']
        sys.modules[mixins].AnchorTrainMixin = AnchorTrainMixin
        sys.modules[calc].bbox_overlaps_nearest_3d = lambda *a, **k: None
        done = integ.apply_patches('anchor_target')               # what patch_reference adds to its report
        assert done == dict(nothing, functions=[calc + '.bbox_overlaps_nearest_3d'],
                            methods=['AnchorTrainMixin.anchor_target_3d'])
        assert sys.modules[calc].bbox_overlaps_nearest_3d is pkg.bbox_overlaps_nearest_3d
        assert not hasattr(sys.modules['mmdet3d.core.bbox'], 'bbox_overlaps_nearest_3d')
        assert AnchorTrainMixin.__dict__['anchor_target_3d'] is pkg.HipAnchorTrainMixin.__dict__['anchor_target_3d']
        key = 'AnchorTrainMixin.anchor_target_3d'
        assert fb.REPLACED[key] is original
        assert integ.apply_patches('anchor_target') == done and fb.REPLACED[key] is original      # twice
        # a configuration the kernels do not cover goes to the kept method under 'warn' and is an error under 'raise'
        head = AnchorTrainMixin()
        head.bbox_assigner, head.bbox_sampler = [dict(type='MaxIoUAssigner')], object()
        args = ([[torch.zeros(1, 1, 1, 1, 2, 7)]], [torch.zeros(0, 7)], [dict()], None, None, 1, 3, True)
        with pytest.warns(RuntimeWarning, match='sampler'):
            assert head.anchor_target_3d(*args) == ('reference', args)
        head.fallback_policy = 'raise'
        with pytest.raises(pkg.MfmaPathError, match='sampler'):
            head.anchor_target_3d(*args)
    finally:
        fb.REPLACED.clear()
        fb.REPLACED.update(kept)
        fb.WARNED.clear()
        for k, v in before.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
