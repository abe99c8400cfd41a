"""GPU: nearest-BEV overlaps and the anchor head's training targets (csrc/anchor_target.hip behind
depth-from-motion_amd/anchor_target.py) against tests/golden/anchor_target.npz -- the reference's own
AnchorTrainMixin.anchor_target_3d, encode, get_direction_target and bbox_overlaps_nearest_3d over stand-ins for
mmdet's assigner and sampler (tests/golden/make_golden_anchor_target.py), run in fp64.

Discrete outputs -- labels, the three weight tensors, direction bins, counts -- are compared EXACTLY: the generator
keeps every maximum 1e-5 from every threshold, near-ties 1e-5 apart and offset_rot / pi 1e-4 from an integer, far
more than fp32 moves them.  Bars of the continuous outputs, read from the fixture where they are used (the
generator stores the largest |fp64 - fp32 CPU| difference it saw):
  bbox_targets          within 4 x fp32_target_error  (1.2e-7 -> 4.8e-7)
  standalone overlaps   within 4 x fp32_overlap_error (2.2e-6 -> 8.8e-6)
The factor 4 has the meaning it has in test_iou3d_loss_gpu.py: an operation order and a device logf that differ
from the CPU run.

The g70 case has 70 GT boxes of one class: more than GT_CHUNK = 64 (csrc/anchor_target.hip), so its GT boxes pass
through LDS in two rounds."""
import importlib
import os
import types

import numpy as np
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu
CASES = ('small', 'posw', 'odd', 'batch', 'empty', 'g70', 'shared', 'rules_all', 'rules_first')
DENSE = ('labels', 'label_weights', 'bbox_targets', 'bbox_weights', 'dir_targets', 'dir_weights')


@pytest.fixture(scope='module')
def pkg():
    importlib.import_module('depth-from-motion_amd.build').build_hip()
    return importlib.import_module('depth-from-motion_amd')


@pytest.fixture(scope='module')
def z():
    return np.load(os.path.join(util.GOLDEN, 'anchor_target.npz'))


def dev(x):
    return torch.from_numpy(np.asarray(x)).cuda()


def assigners(z, case):
    return [dict(type='MaxIoUAssigner', iou_calculator=dict(type='BboxOverlapsNearest3D'), pos_iou_thr=float(p),
                 neg_iou_thr=float(n), min_pos_iou=float(m), ignore_iof_thr=-1,
                 gt_max_assign_all=bool(z[f'{case}/gt_max_assign_all'])) for p, n, m in z['thresholds']]


def inputs(z, case):
    off = z[f'{case}/gt_offsets']
    gts = [dev(z[f'{case}/gt_boxes'][a:b]) for a, b in zip(off[:-1], off[1:])]
    labels = [dev(z[f'{case}/gt_labels'][a:b]) for a, b in zip(off[:-1], off[1:])]
    return dev(z[f'{case}/anchors']), gts, labels


def config(z, case):
    return dict(num_classes=int(z['num_classes']), assign_per_class=bool(z[f'{case}/assign_per_class']),
                dir_offset=float(z['dir_offset']), dir_limit_offset=float(z['dir_limit_offset']),
                pos_weight=float(z[f'{case}/pos_weight']))


def run(pkg, z, case):
    anchors, gts, labels = inputs(z, case)
    return pkg.anchor_target_3d(anchors, gts, labels, assigners(z, case), **config(z, case))


@pytest.fixture(scope='module')
def results(pkg, z):
    """every case once, shared by the tests below and left unchanged"""
    return {case: run(pkg, z, case) for case in CASES}


@pytest.mark.parametrize('case', CASES)
def test_targets_match_the_reference(z, results, case):
    out = dict(zip(DENSE + ('counts',), results[case]))
    assert out['labels'].dtype == torch.int64 and out['dir_targets'].dtype == torch.int64
    assert out['counts'].dtype == torch.int32 and out['counts'].is_cuda
    for k in ('label_weights', 'bbox_targets', 'bbox_weights', 'dir_weights'):
        assert out[k].dtype == torch.float32
    for k in ('labels', 'label_weights', 'bbox_weights', 'dir_targets', 'dir_weights', 'counts'):
        want = z[f'{case}/{k}']
        got = out[k].cpu().numpy()
        assert got.shape == want.shape, k
        assert np.array_equal(got, want), (k, int((got != want).sum()), np.argwhere(got != want)[:5].tolist())
    bar = 4 * float(z['fp32_target_error'])
    e = float(np.abs(out['bbox_targets'].double().cpu().numpy() - z[f'{case}/bbox_targets']).max())
    print(f'{case}: counts {out["counts"].tolist()}, max |gpu - fp64| bbox_targets {e:.3g} (bar {bar:.3g})')
    assert e <= bar


def test_standalone_overlaps(pkg, z):
    bar = 4 * float(z['fp32_overlap_error'])
    calc = importlib.import_module('depth-from-motion_amd.registry').build(dict(type='BboxOverlapsNearest3D'))
    for tag in ('overlaps', 'hand'):
        b1, b2 = dev(z[f'{tag}/boxes1']), dev(z[f'{tag}/boxes2'])
        n = b2.shape[0]
        got = {'iou': pkg.bbox_overlaps_nearest_3d(b1, b2), 'iof': calc(b1, b2, 'iof'),
               'aligned_iou': pkg.bbox_overlaps_nearest_3d(b1[:n], b2, is_aligned=True),
               'aligned_iof': calc(b1[:n], b2, mode='iof', is_aligned=True)}
        for k, v in got.items():
            want = z[f'{tag}/{k}']
            assert v.dtype == torch.float32 and v.shape == want.shape, (tag, k)
            e = float(np.abs(v.double().cpu().numpy() - want).max())
            print(f'{tag}/{k}: max |gpu - fp64| {e:.3g} (bar {bar:.3g})')
            assert e <= bar
        # the matrix and the aligned call run the same function: the same bits
        assert torch.equal(torch.diagonal(got['iou'][:n]), got['aligned_iou'])
    b1, b2 = dev(z['overlaps/boxes1']), dev(z['overlaps/boxes2'])
    base = pkg.bbox_overlaps_nearest_3d(b1, b2)
    # S = 9: the columns beyond 7 are ignored; fp64 and non-contiguous inputs are converted
    wide1 = torch.cat([b1, torch.full((b1.shape[0], 2), 3.0, device='cuda')], 1)
    wide2 = torch.cat([b2, torch.full((b2.shape[0], 2), -1.0, device='cuda')], 1)
    assert torch.equal(pkg.bbox_overlaps_nearest_3d(wide1, wide2), base)
    assert torch.equal(pkg.bbox_overlaps_nearest_3d(b1.double(), b2.double()), base)
    assert torch.equal(pkg.bbox_overlaps_nearest_3d(wide1.t().contiguous().t(), wide2), base)
    assert pkg.bbox_overlaps_nearest_3d(b1[:0], b2).shape == (0, 37)
    assert pkg.bbox_overlaps_nearest_3d(b1[:0], b2[:0], is_aligned=True).shape == (0,)
    with pytest.raises(ValueError):
        pkg.bbox_overlaps_nearest_3d(b1, b2, mode='giou')
    with pytest.raises(ValueError):
        pkg.bbox_overlaps_nearest_3d(b1, b2, is_aligned=True)
    with pytest.raises(ValueError):
        pkg.bbox_overlaps_nearest_3d(b1[:, :6], b2[:, :6])


def test_every_output_element_is_written_and_runs_repeat(pkg, z, results, monkeypatch):
    """outputs allocated with ``empty`` come back fully overwritten -- shown by pre-filling them with NaN / a
    sentinel -- and a second call on the same stream gives the same bits: the scratch is zeroed again"""
    real_empty = torch.empty

    def poisoned(*args, **kwargs):
        t = real_empty(*args, **kwargs)
        if t.is_cuda and t.numel():
            t.fill_(float('nan') if t.is_floating_point() else -77)
        return t

    class Torch:                                                 # torch as that module sees it, ``empty`` poisoned
        empty = staticmethod(poisoned)

        def __getattr__(self, name):
            return getattr(torch, name)
    mod = importlib.import_module('depth-from-motion_amd.anchor_target')
    monkeypatch.setattr(mod, 'torch', Torch())
    for case in ('odd', 'batch', 'g70', 'rules_first'):
        again = run(pkg, z, case)
        for name, a, b in zip(DENSE + ('counts',), again, results[case]):
            assert not bool(torch.isnan(a).any()) if a.is_floating_point() else bool((a != -77).all()), (case, name)
            assert torch.equal(a, b), (case, name)


def test_unsupported_settings_raise(pkg, z):
    anchors, gts, labels = inputs(z, 'small')
    cfg = config(z, 'small')
    a = assigners(z, 'small')
    err = pkg._capi.DfmHipError
    with pytest.raises(err, match='sampler'):
        pkg.anchor_target_3d(anchors, gts, labels, a, sampler='RandomSampler', **cfg)
    with pytest.raises(err, match='neg_iou_thr'):
        pkg.anchor_target_3d(anchors, gts, labels, [dict(x, neg_iou_thr=(0.1, 0.4)) for x in a], **cfg)
    with pytest.raises(err, match='ignore'):
        pkg.anchor_target_3d(anchors, gts, labels, [dict(x, ignore_iof_thr=0.5) for x in a], num_ignore_boxes=3, **cfg)
    wide = torch.cat([anchors, torch.zeros_like(anchors[..., :2])], -1)
    with pytest.raises(err, match='width'):
        pkg.anchor_target_3d(wide, [torch.cat([g, g[:, :2]], 1) for g in gts], labels, a, **cfg)
    with pytest.raises(ValueError):
        pkg.anchor_target_3d(anchors, gts, labels, a[:2], **cfg)


class Boxes:
    """what the mixin is handed for GT boxes: an object with ``.tensor``"""

    def __init__(self, tensor):
        self.tensor = tensor

    def __len__(self):
        return self.tensor.shape[0]


def make_head(pkg, z, case):
    class Head(pkg.HipAnchorTrainMixin):
        pass
    head = Head()
    class MaxIoUAssigner:
        def __init__(self, type, **fields):
            self.__dict__.update(fields)
    head.bbox_assigner = [MaxIoUAssigner(**a) for a in assigners(z, case)]
    head.bbox_sampler = type('PseudoSampler', (), {})()
    head.bbox_coder = type('DeltaXYZWLHRBBoxCoder', (), {})()
    head.train_cfg = types.SimpleNamespace(pos_weight=float(z[f'{case}/pos_weight']))
    head.dir_offset, head.dir_limit_offset = float(z['dir_offset']), float(z['dir_limit_offset'])
    head.assign_per_class, head.box_code_size = bool(z[f'{case}/assign_per_class']), 7
    return head


@pytest.mark.parametrize('case', ['batch', 'empty'])
def test_mixin_returns_the_reference_tuple(pkg, z, results, case):
    anchors, gts, labels = inputs(z, case)
    head = make_head(pkg, z, case)
    B = len(gts)
    levels = [anchors]                                           # get_anchors: the same list for every image
    res = head.anchor_target_3d([levels for _ in range(B)], [Boxes(g) for g in gts], [dict() for _ in range(B)],
                                gt_labels_list=labels, num_classes=3, sampling=False)
    assert isinstance(res, tuple) and len(res) == 8
    for per_level, want in zip(res[:6], results[case]):
        assert isinstance(per_level, list) and len(per_level) == 1
        assert torch.equal(per_level[0], want)                   # (B, anchors of the level, ...)
    assert type(res[6]) is int and type(res[7]) is int
    assert res[6] == int(z[f'{case}/num_total_pos']) and res[7] == int(z[f'{case}/num_total_neg'])
    # a head the kernels do not cover and no reference method behind the mixin: an error, not a quiet fallback
    head.bbox_sampler = object()
    with pytest.raises(pkg.MfmaPathError, match='sampler'):
        head.anchor_target_3d([levels for _ in range(B)], gts, [dict() for _ in range(B)], gt_labels_list=labels,
                              num_classes=3, sampling=False)


def test_single_assigner_sees_every_anchor_as_one_slot(pkg, z):
    """one assigner (not a list): train_mixins.py:231-236, all anchors against all GT boxes with its thresholds"""
    anchors, gts, labels = inputs(z, 'shared')
    one = assigners(z, 'shared')[1]
    labels_out, label_weights, _, bbox_weights, _, _, counts = pkg.anchor_target_3d(
        anchors, gts, labels, one, **config(z, 'shared'))
    A = anchors[..., 0].numel()
    pos = bbox_weights[0, :, 0] > 0
    ignored = label_weights[0] == 0
    assert int(counts[0, 0]) == int(pos.sum()) and int(counts.sum()) + int(ignored.sum()) == A
    # every GT box reaches min_pos_iou on some anchor of its own class here: each has a positive with its label
    assert set(labels_out[0][pos].tolist()) == set(z['shared/gt_labels'].tolist()) and int(pos.sum()) >= 7


def test_output_feeds_the_iou_loss(pkg, z, results):
    anchors, _, _ = inputs(z, 'batch')
    flat = anchors.view(-1, 7)
    _, _, bbox_targets, bbox_weights, _, _, counts = results['batch']
    for b in range(2):
        pos = torch.nonzero(bbox_weights[b, :, 0] > 0).view(-1)
        assert pos.numel() == int(counts[b, 0])
        pred = (bbox_targets[b] + 0.02).requires_grad_(True)
        loss = pkg.iou3d_loss_from_deltas(flat, pred, bbox_targets[b], pos)
        assert loss.shape == (pos.numel(),) and bool(torch.isfinite(loss).all())
        assert 0 < float(loss.detach().mean()) < 0.5                      # deltas 0.02 off their targets: high IoU
        loss.sum().backward()
        assert bool(torch.isfinite(pred.grad).all())
