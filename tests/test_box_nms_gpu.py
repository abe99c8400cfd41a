"""GPU: BEV NMS and rotated IoU (csrc/box_nms.hip behind depth-from-motion_amd/box_nms.py) against
tests/golden/box_nms.npz -- the reference's own box3d_multiclass_nms / nms_bev / nms_normal_bev over an fp64
numpy stand-in for mmcv's two CUDA ops (tests/golden/make_golden_box_nms.py).

Bars.  Keep indices: exact, in every scene.  That is decidable because the generator accepts a scene only when
no pair's fp64 IoU lies within ``guard_band`` = 1e-4 of the threshold, and 1e-4 is 139 x the largest difference
between the fp64 IoU and the same algorithm in numpy float32 over every pair of the fixture
(``fp32_iou_error`` = 7.2e-7; both numbers are stored in the npz and checked in tests/test_box_nms.py).
IoU matrix: within 2 x fp32_iou_error = 1.43e-6 of the fp64 values, read from the fixture where it is used.

Inputs the functions convert rather than refuse: boxes of any floating dtype / stride become contiguous fp32;
scores are only sorted and gathered, so bf16 scores are taken as they are
(test_non_contiguous_and_bf16_inputs_are_converted)."""
import importlib
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu
SCENES = ('dense', 'sparse', 'n65', 'n1', 'n0', 'special')
MAX_NUMS = {'dense': (500, 50), 'sparse': (500, 20), 'n65': (500,), 'n1': (500,), 'n0': (500,), 'special': (500,)}


@pytest.fixture(scope='module')
def pkg():
    importlib.import_module('depth-from-motion_amd.build').build_hip()
    return importlib.import_module('depth-from-motion_amd')


@pytest.fixture(scope='module')
def z():
    return np.load(os.path.join(util.GOLDEN, 'box_nms.npz'))


def scene(z, name):
    return (torch.from_numpy(z[f'{name}/boxes']).cuda(), torch.from_numpy(z[f'{name}/scores']).cuda(),
            float(z[f'{name}/score_thr']), float(z['nms_thr']))


def test_box_iou_rotated_matches_the_fp64_matrix(pkg, z):
    bound = 2 * float(z['fp32_iou_error'])                      # 2 x 7.15e-7 = 1.43e-6
    b1, b2 = torch.from_numpy(z['iou_boxes1']).cuda(), torch.from_numpy(z['iou_boxes2']).cuda()
    got = pkg.box_iou_rotated(b1, b2)
    assert got.shape == (b1.shape[0], b2.shape[0]) and got.dtype == torch.float32
    err = float((got.double().cpu() - torch.from_numpy(z['iou'])).abs().max())
    print('box_iou_rotated: max |gpu - fp64| =', err, 'bound', bound)
    assert err <= bound
    assert int((got > 0).sum()) > 1000                          # the matrix is not trivially zero
    # aligned: the diagonal of the square part
    n = min(b1.shape[0], b2.shape[0])
    diag = pkg.box_iou_rotated(b1[:n], b2[:n], aligned=True)
    assert diag.shape == (n,)
    assert torch.equal(diag, got[:n, :n].diagonal())
    # both argument orders agree within the bound; empty inputs give empty outputs
    assert float((pkg.box_iou_rotated(b2, b1).t() - got).abs().max()) <= bound
    assert pkg.box_iou_rotated(b1[:0], b2).shape == (0, b2.shape[0])
    assert pkg.box_iou_rotated(b1[:0], b2[:0], aligned=True).shape == (0,)
    with pytest.raises(ValueError):
        pkg.box_iou_rotated(b1[:3], b2[:4], aligned=True)


@pytest.mark.parametrize('name', SCENES)
def test_single_class_nms_matches_the_fixture(pkg, z, name):
    boxes, scores, _, thr = scene(z, name)
    if boxes.shape[0] == 0:
        for fn in (pkg.nms_bev, pkg.nms_normal_bev):
            keep = fn(boxes, scores[:, 0], thr)
            assert keep.shape == (0,) and keep.dtype == torch.int64 and keep.is_cuda
        return
    keep = pkg.nms_bev(boxes, scores[:, 0], thr)
    assert keep.dtype == torch.int64
    assert keep.cpu().tolist() == z[f'{name}/keep_rot'].tolist()
    keep_a = pkg.nms_normal_bev(boxes, scores[:, 0], thr)
    assert keep_a.cpu().tolist() == z[f'{name}/keep_aligned'].tolist()
    # keep indexes the caller's arrays: the kept scores descend
    s = scores[keep, 0]
    assert bool((s[1:] < s[:-1]).all())


def test_pre_and_post_max_size_cuts(pkg, z):
    boxes, scores, _, thr = scene(z, 'sparse')
    for key, (pre, post) in (('keep_rot_pre100_post10', (100, 10)), ('keep_rot_pre100', (100, None)),
                             ('keep_rot_post5', (None, 5))):
        keep = pkg.nms_bev(boxes, scores[:, 0], thr, pre_max_size=pre, post_max_size=post)
        assert keep.cpu().tolist() == z[f'sparse/{key}'].tolist(), key
    assert len(z['sparse/keep_rot_pre100_post10']) == 10 and len(z['sparse/keep_rot_post5']) == 5


def run_multiclass(pkg, boxes, scores, score_thr, thr, max_num, rot, extras=False):
    n = boxes.shape[0]
    index = torch.arange(n, dtype=torch.float32, device='cuda')[:, None]
    cfg = SimpleNamespace(use_rotate_nms=rot, nms_thr=thr)
    kw = {}
    if extras:
        kw = dict(mlvl_dir_scores=torch.arange(n, device='cuda') % 2,
                  mlvl_attr_scores=torch.arange(n, device='cuda', dtype=torch.float32) * 3,
                  mlvl_bboxes2d=torch.arange(n, device='cuda', dtype=torch.float32)[:, None].repeat(1, 4))
    return pkg.box3d_multiclass_nms(index, boxes, scores, score_thr, max_num, cfg, **kw), kw


@pytest.mark.parametrize('rot', [True, False], ids=['rotated', 'aligned'])
@pytest.mark.parametrize('name', SCENES)
def test_multiclass_nms_matches_the_fixture(pkg, z, name, rot):
    boxes, scores, score_thr, thr = scene(z, name)
    tag = 'rot' if rot else 'aligned'
    for max_num in MAX_NUMS[name]:
        (b, s, lab, d, a, b2d), kw = run_multiclass(pkg, boxes, scores, score_thr, thr, max_num, rot, extras=True)
        want_idx = torch.from_numpy(z[f'{name}/mc_{tag}_{max_num}_idx']).cuda()
        want_lab = torch.from_numpy(z[f'{name}/mc_{tag}_{max_num}_labels']).cuda()
        assert b.shape == (len(want_idx), 1) and lab.dtype == torch.long
        idx = b[:, 0].long()
        assert torch.equal(idx, want_idx), (name, tag, max_num)
        assert torch.equal(lab, want_lab)
        assert torch.equal(s, scores[idx, lab])
        if len(idx):
            assert torch.equal(d, kw['mlvl_dir_scores'][idx]) and torch.equal(a, kw['mlvl_attr_scores'][idx])
            assert torch.equal(b2d, kw['mlvl_bboxes2d'][idx])
        else:   # the reference's empty-result tensors
            assert s.shape == (0,) and d.shape == (0,) and a.shape == (0,) and b2d.shape == (0, 4)
            assert s.dtype == scores.dtype
    if name == 'dense':
        assert len(z['dense/mc_rot_50_idx']) == 50 < len(z['dense/mc_rot_500_idx'])   # the max_num cut was taken
    if name == 'sparse':
        assert 1 not in z['sparse/mc_rot_500_labels']                                  # the class without candidates


@pytest.mark.parametrize('rot', [True, False], ids=['rotated', 'aligned'])
@pytest.mark.parametrize('name', ['dense', 'sparse', 'special'])
def test_one_launch_equals_the_per_class_loop(pkg, z, name, rot):
    """box3d_multiclass_nms == this module's own nms_bev / nms_normal_bev once per class, as the reference
    loops (boolean index per class, box3d_nms.py:53-84)"""
    boxes, scores, score_thr, thr = scene(z, name)
    (b, s, lab), _ = run_multiclass(pkg, boxes, scores, score_thr, thr, 10 ** 6, rot)
    fn = pkg.nms_bev if rot else pkg.nms_normal_bev
    idx, labels = [], []
    everything = torch.arange(boxes.shape[0], device='cuda')
    for c in range(scores.shape[1] - 1):
        sel = scores[:, c] > score_thr
        if not sel.any():
            continue
        keep = fn(boxes[sel], scores[sel, c], thr)
        idx.append(everything[sel][keep])
        labels.append(torch.full((len(keep),), c, device='cuda'))
    assert torch.equal(b[:, 0].long(), torch.cat(idx)) and torch.equal(lab, torch.cat(labels))


def test_result_is_the_same_on_a_side_stream(pkg, z):
    boxes, scores, score_thr, thr = scene(z, 'dense')
    (b0, s0, l0), _ = run_multiclass(pkg, boxes, scores, score_thr, thr, 500, True)
    k0 = pkg.nms_bev(boxes, scores[:, 0], thr)
    i0 = pkg.box_iou_rotated(torch.from_numpy(z['iou_boxes1']).cuda(), torch.from_numpy(z['iou_boxes2']).cuda())
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        (b1, s1, l1), _ = run_multiclass(pkg, boxes, scores, score_thr, thr, 500, True)
        k1 = pkg.nms_bev(boxes, scores[:, 0], thr)
        i1 = pkg.box_iou_rotated(torch.from_numpy(z['iou_boxes1']).cuda(), torch.from_numpy(z['iou_boxes2']).cuda())
    side.synchronize()
    assert torch.equal(b0, b1) and torch.equal(s0, s1) and torch.equal(l0, l1)
    assert torch.equal(k0, k1) and torch.equal(i0, i1)


def test_non_contiguous_and_bf16_inputs_are_converted(pkg, z):
    """boxes: any stride / floating dtype -> contiguous fp32 inside; scores: sorted in their own dtype.  n65's
    scores are k / 128, exact and distinct in bf16."""
    boxes, scores, score_thr, thr = scene(z, 'n65')
    want = z['n65/keep_rot'].tolist()
    wide = torch.zeros(65, 10, device='cuda')
    wide[:, ::2] = boxes
    assert not wide[:, ::2].is_contiguous()
    assert pkg.nms_bev(wide[:, ::2], scores[:, 0], thr).cpu().tolist() == want
    assert pkg.nms_bev(boxes.double(), scores[:, 0], thr).cpu().tolist() == want
    sb = scores.to(torch.bfloat16)
    assert torch.equal(sb.float(), scores)
    assert pkg.nms_bev(boxes, sb[:, 0], thr).cpu().tolist() == want
    assert pkg.nms_normal_bev(wide[:, ::2], sb[:, 0], thr).cpu().tolist() == z['n65/keep_aligned'].tolist()
    (b, s, lab), _ = run_multiclass(pkg, wide[:, ::2], sb, score_thr, thr, 500, True)
    assert b[:, 0].long().cpu().tolist() == z['n65/mc_rot_500_idx'].tolist() and s.dtype == torch.bfloat16
    i1 = torch.from_numpy(z['iou_boxes1']).cuda()
    assert torch.equal(pkg.box_iou_rotated(i1.double()[:, None, :].expand(-1, 2, -1)[:, 1], i1[:8]),
                       pkg.box_iou_rotated(i1, i1[:8]))


def test_more_candidates_than_the_cap_is_a_clear_error(pkg):
    n = pkg._capi.BOX_NMS_MAX_N + 1
    boxes = torch.zeros(n, 5, device='cuda')
    scores = torch.rand(n, device='cuda')
    with pytest.raises(ValueError, match=str(pkg._capi.BOX_NMS_MAX_N)):
        pkg.nms_bev(boxes, scores, 0.25)
    # cut below the cap it runs (zero-area boxes: everything is kept)
    keep = pkg.nms_bev(boxes, scores, 0.25, pre_max_size=1000)
    assert keep.shape == (1000,)
