"""GPU: 2-D box overlaps and the 2-D ATSS head's training targets (csrc/atss_target.hip behind
depth-from-motion_amd/atss_target.py) against tests/golden/atss_target.npz -- the reference's own
ATSS3DCenterAssigner.assign and LIGAATSSHead._get_target_single over stand-ins for mmdet's helpers
(tests/golden/make_golden_atss_target.py), run in fp64.

Discrete outputs -- labels, label and box weights, assigned GT indices, counts -- are compared EXACTLY: the generator
keeps the distance cut of every (GT, level) 1e-3 px wide, every candidate's overlap 1e-5 from its threshold, every
centre-in-box margin 1e-3 from 0.01 and competing claims 1e-5 apart, far more than fp32 moves them.  Bars of the
continuous outputs, read from the fixture where they are used (the generator stores the largest |fp64 - fp32 CPU|
difference it saw):
  bbox_targets          within 4 x fp32_target_error  (1.2e-6 -> 4.8e-6; the targets are deltas / 0.1 and / 0.2)
  standalone overlaps   within 4 x fp32_overlap_error (1.5e-7 -> 5.8e-7)
The factor 4 has the meaning it has in test_anchor_target_gpu.py: an operation order and a device logf that differ
from the CPU run.

Ties are built here, not stored: a GT point midway between anchor centres of tiny's first level makes four, then
eight anchors share a distance, and a GT box that every anchor contains makes their overlaps the same bits, so the
threshold mean + std equals that overlap exactly and the positives ARE the chosen candidates."""
import importlib
import os
import types

import numpy as np
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu
CASES = ('tiny', 'odd', 'five', 'posw', 'empty', 'g70', 'border', 'valid', 'centre4', 'rules')
NAMES = ('labels', 'label_weights', 'bbox_targets', 'bbox_weights', 'assigned_gt_inds', 'counts')


@pytest.fixture(scope='module')
def pkg():
    importlib.import_module('depth-from-motion_amd.build').build_hip()
    return importlib.import_module('depth-from-motion_amd')


@pytest.fixture(scope='module')
def z():
    return np.load(os.path.join(util.GOLDEN, 'atss_target.npz'))


def dev(x):
    return torch.from_numpy(np.asarray(x)).cuda()


def inputs(z, case):
    off = z[f'{case}/gt_offsets']
    gts = [dev(z[f'{case}/gt_boxes'][a:b]) for a, b in zip(off[:-1], off[1:])]
    labels = [dev(z[f'{case}/gt_labels'][a:b]) for a, b in zip(off[:-1], off[1:])]
    inside = z[f'{case}/inside']
    return dev(z[f'{case}/anchors']), z[f'{case}/level_sizes'].tolist(), gts, labels, \
        (None if inside.all() else dev(inside))


def config(z, case):
    return dict(topk=int(z['topk']), num_classes=int(z['num_classes']), pos_weight=float(z[f'{case}/pos_weight']),
                target_means=z['target_means'].tolist(), target_stds=z['target_stds'].tolist())


def run(pkg, z, case):
    anchors, sizes, gts, labels, inside = inputs(z, case)
    return pkg.atss_target_2d(anchors, sizes, gts, labels, inside_flags=inside, **config(z, case))


@pytest.fixture(scope='module')
def results(pkg, z):
    """every case once, shared by the tests below and left unchanged"""
    return {case: run(pkg, z, case) for case in CASES}


@pytest.mark.parametrize('case', CASES)
def test_targets_match_the_reference(z, results, case):
    out = dict(zip(NAMES, results[case]))
    assert out['labels'].dtype == torch.int64 and out['assigned_gt_inds'].dtype == torch.int64
    assert out['counts'].dtype == torch.int32 and out['counts'].is_cuda
    for k in ('label_weights', 'bbox_targets', 'bbox_weights'):
        assert out[k].dtype == torch.float32
    for k in ('labels', 'label_weights', 'bbox_weights', 'assigned_gt_inds', 'counts'):
        want = z[f'{case}/{k}']
        got = out[k].cpu().numpy()
        assert got.shape == want.shape, k
        assert np.array_equal(got, want), (k, int((got != want).sum()), np.argwhere(got != want)[:5].tolist())
    want = z[f'{case}/bbox_targets']
    assert tuple(out['bbox_targets'].shape) == want.shape
    bar = 4 * float(z['fp32_target_error'])
    e = float(np.abs(out['bbox_targets'].double().cpu().numpy() - want).max())
    print(f'{case}: counts {out["counts"].tolist()}, max |gpu - fp64| bbox_targets {e:.3g} (bar {bar:.3g})')
    assert e <= bar


def test_standalone_overlaps(pkg, z):
    bar = 4 * float(z['fp32_overlap_error'])
    calc = importlib.import_module('depth-from-motion_amd.registry').build(dict(type='BboxOverlaps2D'))
    for tag in ('overlaps', 'hand'):
        b1, b2 = dev(z[f'{tag}/boxes1']), dev(z[f'{tag}/boxes2'])
        n = b2.shape[0]
        got = {'iou': pkg.bbox_overlaps(b1, b2), 'iof': calc(b1, b2, 'iof'),
               'aligned_iou': pkg.bbox_overlaps(b1[:n], b2, is_aligned=True),
               'aligned_iof': calc(b1[:n], b2, mode='iof', is_aligned=True)}
        for k, v in got.items():
            want = z[f'{tag}/{k}']
            assert v.dtype == torch.float32 and v.shape == want.shape, (tag, k)
            e = float(np.abs(v.double().cpu().numpy() - want).max())
            print(f'{tag}/{k}: max |gpu - fp64| {e:.3g} (bar {bar:.3g})')
            assert e <= bar
        # the matrix and the aligned call run the same function: the same bits
        assert torch.equal(torch.diagonal(got['iou'][:n]), got['aligned_iou'])
        assert torch.equal(torch.diagonal(got['iof'][:n]), got['aligned_iof'])
    b1, b2 = dev(z['overlaps/boxes1']), dev(z['overlaps/boxes2'])
    base = pkg.bbox_overlaps(b1, b2)
    # fp64 and non-contiguous inputs are converted
    wide1 = torch.cat([b1, torch.full((b1.shape[0], 2), 3.0, device='cuda')], 1)
    assert torch.equal(pkg.bbox_overlaps(wide1[:, :4], b2), base)
    assert torch.equal(pkg.bbox_overlaps(b1.t().contiguous().t(), b2.double()), base)
    assert torch.equal(calc(torch.cat([b1, b1[:, :1]], 1), b2), base)          # a score column is cut
    assert pkg.bbox_overlaps(b1[:0], b2).shape == (0, 37)
    assert pkg.bbox_overlaps(b1[:0], b2[:0], is_aligned=True).shape == (0,)
    with pytest.raises(ValueError):
        pkg.bbox_overlaps(b1, b2, mode='giou')
    with pytest.raises(ValueError):
        pkg.bbox_overlaps(b1, b2, is_aligned=True)
    with pytest.raises(ValueError):
        pkg.bbox_overlaps(b1, b2, eps=1e-7)
    with pytest.raises(ValueError):
        pkg.bbox_overlaps(wide1, b2)


def test_equal_distances_go_in_ascending_anchor_index(pkg, z):
    """tiny's first level: 4 x 6 centres on (8 x, 8 y).  A GT point at (12, 12) has four anchors at the same distance
    (indices 7, 8, 13, 14) and eight at the next (1, 2, 6, 9, 12, 15, 19, 20).  Every 128 px anchor contains the GT
    box, so all overlaps are the same bits, the threshold equals them and every candidate whose centre lies in the
    box is positive: the positives are the ascending-index prefix of the tied group."""
    n = int(z['tiny/level_sizes'][0])
    anchors = dev(z['tiny/anchors'][:n])
    assert n == 24 and anchors[7].tolist() == [8 - 64, 8 - 64, 8 + 64, 8 + 64]
    gt = [torch.tensor([[-4.0, -4.0, 28.0, 28.0, 12.0, 12.0]], device='cuda')]
    lab = [torch.tensor([1], device='cuda')]
    for topk, want in ((2, [7, 8]), (3, [7, 8, 13]), (4, [7, 8, 13, 14]), (6, [1, 2, 7, 8, 13, 14]),
                       (9, [1, 2, 6, 7, 8, 9, 12, 13, 14])):
        out = pkg.atss_target_2d(anchors, [n], gt, lab, topk=topk, num_classes=3)
        chosen = torch.nonzero(out[4][0] > 0).view(-1).tolist()
        assert chosen == want, (topk, chosen)
        assert out[5].tolist() == [[topk, n - topk]] and out[0][0][chosen].tolist() == [1] * topk
    # a single candidate has no threshold (the reference's NaN compares false): no positive
    out = pkg.atss_target_2d(anchors, [n], gt, lab, topk=1, num_classes=3)
    assert out[5].tolist() == [[0, n]]


def test_identical_gts_resolve_to_the_lower_index(pkg, z):
    anchors, sizes, gts, labels, _ = inputs(z, 'five')
    won = z['five/assigned_gt_inds'][0]
    g = int(np.bincount(won[won > 0]).argmax()) - 1               # the GT of image 0 with the most positives
    box = gts[0][g:g + 1]
    out = pkg.atss_target_2d(anchors, sizes, [torch.cat([box, box, box])], [torch.tensor([2, 0, 1], device='cuda')],
                             **config(z, 'five'))
    assigned = out[4][0]
    assert int((assigned == 1).sum()) > 0 and int((assigned > 1).sum()) == 0
    assert set(out[0][0][assigned == 1].tolist()) == {2}


def test_batch_independence_and_inside_none(pkg, z, results):
    anchors, sizes, gts, labels, _ = inputs(z, 'five')
    alone = pkg.atss_target_2d(anchors, sizes, gts[1:], labels[1:], **config(z, 'five'))
    for name, a, b in zip(NAMES, alone, results['five']):
        assert torch.equal(a[0], b[1]), name                      # image 1 alone: the same bits as in the batch
    ones = torch.ones((2, anchors.shape[0]), dtype=torch.bool, device='cuda')
    full = pkg.atss_target_2d(anchors, sizes, gts, labels, inside_flags=ones, **config(z, 'five'))
    for name, a, b in zip(NAMES, full, results['five']):
        assert torch.equal(a, b), name                            # inside=None is an all-ones inside
    # without labels every positive is class 0
    bare = pkg.atss_target_2d(anchors, sizes, gts, None, **config(z, 'five'))
    assert torch.equal(bare[4], results['five'][4])
    assert set(bare[0][bare[4] > 0].tolist()) == {0} and set(bare[0][bare[4] <= 0].tolist()) == {3}


def test_every_output_element_is_written_and_runs_repeat(pkg, z, results, monkeypatch):
    """outputs allocated with ``empty`` come back fully overwritten -- shown by pre-filling them with NaN / a
    sentinel -- and a second call on the same stream gives the same bits: the keys are zeroed again"""
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
    mod = importlib.import_module('depth-from-motion_amd.atss_target')
    monkeypatch.setattr(mod, 'torch', Torch())
    for case in ('odd', 'empty', 'border', 'g70'):
        again = run(pkg, z, case)
        for name, a, b in zip(NAMES, again, results[case]):
            assert not bool(torch.isnan(a).any()) if a.is_floating_point() else bool((a != -77).all()), (case, name)
            assert torch.equal(a, b), (case, name)


def test_the_plain_function_does_not_wait_for_the_device(pkg, z, results):
    """no device-to-host copy and no synchronisation inside atss_target_2d: with a long kernel pending on the stream
    the call returns while that kernel is still running"""
    if not hasattr(torch.cuda, '_sleep'):
        pytest.skip('torch.cuda._sleep is unavailable: nothing to hold the stream with')
    anchors, sizes, gts, labels, inside = inputs(z, 'border')
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        pkg.atss_target_2d(anchors, sizes, gts, labels, inside_flags=inside, **config(z, 'border'))   # warm: scratch
        s.synchronize()
        torch.cuda._sleep(20_000_000)
        out = pkg.atss_target_2d(anchors, sizes, gts, labels, inside_flags=inside, **config(z, 'border'))
        pending = not s.query()
    s.synchronize()
    assert pending, 'atss_target_2d returned only after the stream had drained: it waits for the device'
    for name, a, b in zip(NAMES, out, results['border']):
        assert torch.equal(a, b), name


def test_unsupported_settings_raise(pkg, z):
    anchors, sizes, gts, labels, _ = inputs(z, 'tiny')
    cfg = config(z, 'tiny')
    err = pkg._capi.DfmHipError
    with pytest.raises(err, match='thresh_mode'):
        pkg.atss_target_2d(anchors, sizes, gts, labels, thresh_mode='ratio', **cfg)
    with pytest.raises(err, match='sampler'):
        pkg.atss_target_2d(anchors, sizes, gts, labels, sampler='RandomSampler', **cfg)
    with pytest.raises(err, match='coder'):
        pkg.atss_target_2d(anchors, sizes, gts, labels, coder='TBLRBBoxCoder', **cfg)
    with pytest.raises(err, match='reg_width'):
        pkg.atss_target_2d(anchors, sizes, gts, labels, reg_width=6, **cfg)
    with pytest.raises(err, match='ignore'):
        pkg.atss_target_2d(anchors, sizes, gts, labels, ignore_iof_thr=0.5, num_ignore_boxes=2, **cfg)
    with pytest.raises(err, match='topk'):
        pkg.atss_target_2d(anchors, sizes, gts, labels, **dict(cfg, topk=17))
    with pytest.raises(ValueError):
        pkg.atss_target_2d(anchors, sizes[:1], gts, labels, **cfg)
    with pytest.raises(ValueError):
        pkg.atss_target_2d(anchors, sizes, gts, labels, inside_flags=torch.ones(2, 5, device='cuda'), **cfg)


def make_head(pkg, z, case):
    class Head(pkg.HipATSSTargetMixin):
        pass
    head = Head()
    head.assigner = type('ATSS3DCenterAssigner', (), {})()
    head.assigner.topk, head.assigner.thresh_mode, head.assigner.ignore_iof_thr = int(z['topk']), 'meanstd', -1
    head.assigner.append_3d_centers = z[f'{case}/gt_boxes'].shape[1] == 6
    head.assigner.iou_calculator = pkg.BboxOverlaps2D()
    head.sampler = type('PseudoSampler', (), {})()
    head.bbox_coder = type('DeltaXYWHBBoxCoder', (), dict(means=tuple(z['target_means']), stds=tuple(z['target_stds'])))()
    head.train_cfg = types.SimpleNamespace(allowed_border=int(z[f'{case}/allowed_border']),
                                           pos_weight=float(z[f'{case}/pos_weight']))
    head.num_classes, head.num_reg_channel, head.num_anchors = int(z['num_classes']), 4, 1
    return head


@pytest.mark.parametrize('case', ['five', 'empty', 'border'])
def test_mixin_returns_the_reference_tuple(pkg, z, results, case):
    anchors, sizes, gts, labels, _ = inputs(z, case)
    head = make_head(pkg, z, case)
    B = len(gts)
    levels = list(torch.split(anchors, sizes))                   # get_anchors: the same list for every image
    valid = [list(torch.split(dev(z[f'{case}/valid_flags'][b]).bool(), sizes)) for b in range(B)]
    metas = [dict(img_shape=(int(h), int(w), 3)) for h, w in z[f'{case}/img_shapes']]
    res = head.get_targets([levels for _ in range(B)], valid, gts, metas, gt_labels_list=labels)
    assert isinstance(res, tuple) and len(res) == 7
    inside = dev(z[f'{case}/inside']).bool()
    dense = (anchors[None] * inside[..., None], *results[case][:4])
    for per_level, want in zip(res[:5], dense):
        assert isinstance(per_level, list) and [t.shape[1] for t in per_level] == sizes
        assert torch.equal(torch.cat(per_level, 1), want)         # (B, anchors of the level, ...) in level order
    assert np.array_equal(torch.cat(res[0], 1).cpu().numpy(), z[f'{case}/anchors_out'].astype(np.float32))
    assert type(res[5]) is int and type(res[6]) is int
    assert res[5] == int(z[f'{case}/num_total_pos']) and res[6] == int(z[f'{case}/num_total_neg'])
    # a head the kernels do not cover and no reference method behind the mixin: an error, not a quiet fallback
    head.assigner.thresh_mode = 'ratio'
    with pytest.raises(pkg.MfmaPathError, match='ratio'):
        head.get_targets([levels for _ in range(B)], valid, gts, metas, gt_labels_list=labels)
