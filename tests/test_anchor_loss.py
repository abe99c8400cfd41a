"""CPU: the host side of the 3-D anchor head's loss (depth-from-motion_amd/anchor_loss.py, csrc/anchor_loss.hip): what
the C ABI refuses before any HIP call, the refusal of CPU tensors, the mixin's average factors for both head classes
against tests/golden/anchor_loss.npz (the reference's own loss_single bodies in fp64, tests/golden/
make_golden_anchor_loss.py), its fallback rule, and patch_reference's rebinding of both classes."""
import ctypes
import importlib
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests import anchor_loss_ref as ref
from tests import util

CASES = ('plain', 'plain_cw', 'plain_nodir', 'liga', 'liga_reduce', 'liga_iou', 'liga_reduce_iou', 'nopos')


@pytest.fixture(scope='module')
def pkg():
    importlib.import_module('depth-from-motion_amd.build').build_hip()
    return importlib.import_module('depth-from-motion_amd')


@pytest.fixture(scope='module')
def al():
    return importlib.import_module('depth-from-motion_amd.anchor_loss')


@pytest.fixture(scope='module')
def z():
    return np.load(os.path.join(util.GOLDEN, 'anchor_loss.npz'))


def desc(pkg, **over):
    d = pkg._capi.AnchorLossDesc(batch=2, h=5, w=6, anchors_per_location=6, num_classes=3, box_code_size=7,
                                 dtype=pkg._capi.DFM_F32, has_dir=1, with_iou=0, diff_rad_by_sin=1, gamma=2.0,
                                 alpha=0.25, beta=1.0 / 9.0)
    d.code_weight[:] = [1.0] * 16
    for k, v in over.items():
        setattr(d, k, v)
    return d


def test_unsupported_descriptors_are_refused_before_any_hip_call(pkg):
    """no GPU here: a HIP call would fail with DFM_ERR_HIP (-4), so -2 shows the refusal came first"""
    lib = pkg._capi.lib()
    unsupported = pkg._capi.DFM_ERR_UNSUPPORTED
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    fwd = lambda d: lib.dfm_anchor3d_loss_fwd(ctypes.byref(d), *[p] * 12, p, 1 << 20, None)  # noqa: E731
    bwd = lambda d: lib.dfm_anchor3d_loss_bwd(ctypes.byref(d), *[p] * 15, None)  # noqa: E731
    size = lambda d: lib.dfm_anchor3d_loss_workspace_bytes(ctypes.byref(d))  # noqa: E731
    rules = [(dict(box_code_size=6), b'box_code_size'), (dict(box_code_size=17), b'box_code_size'),
             (dict(box_code_size=9, with_iou=1), b'IoU'), (dict(num_classes=0), b'num_classes'),
             (dict(dtype=2), b'dtype'), (dict(batch=1 << 20, h=64, w=64), b'2^31'),
             (dict(batch=1, h=1 << 16, w=1 << 15, anchors_per_location=1), b'2^31')]
    for over, word in rules:
        for call in (fwd, bwd):
            assert call(desc(pkg, **over)) == unsupported, over
            assert word in lib.dfm_last_error(), (over, lib.dfm_last_error())
        assert size(desc(pkg, **over)) == 0
    assert size(desc(pkg, box_code_size=16)) == size(desc(pkg, box_code_size=7, with_iou=1)) == 16 * 2    # both taken
    # (2^31 - 1 rows exactly are taken)
    assert size(desc(pkg, batch=1, h=1, w=(1 << 31) - 1, anchors_per_location=1)) == 16 * (1 << 23)
    assert size(desc(pkg)) == 16 * 2                                   # 360 rows: two workgroups of 256
    # empty input: the backward launches nothing and says OK; nothing is read, NULL included
    for over in (dict(batch=0), dict(h=0), dict(w=0)):
        assert lib.dfm_anchor3d_loss_bwd(ctypes.byref(desc(pkg, **over)), *[None] * 15, None) == 0
        assert size(desc(pkg, **over)) == 0
    assert bwd(desc(pkg, batch=-1)) == -1 and bwd(desc(pkg, anchors_per_location=0)) == -1
    assert bwd(desc(pkg, beta=0.0)) == -1 and b'beta' in lib.dfm_last_error()
    assert lib.dfm_anchor3d_loss_bwd(ctypes.byref(desc(pkg)), None, *[p] * 14, None) == -1
    assert b'NULL' in lib.dfm_last_error()
    assert lib.dfm_anchor3d_loss_bwd(ctypes.byref(desc(pkg, with_iou=1)), *[p] * 9, None, *[p] * 5, None) == -1
    assert b'anchors' in lib.dfm_last_error()


def inputs(z, labels=None):
    t = lambda k: torch.from_numpy(z[k])  # noqa: E731
    return [t('cls'), t('reg'), t('dir'), t('labels') if labels is None else torch.from_numpy(labels),
            t('label_weights'), t('bbox_targets'), t('bbox_weights'), t('dir_targets'), t('dir_weights'), t('anchors')]


def test_cpu_tensors_are_refused(pkg, z):
    args = inputs(z)
    with pytest.raises(RuntimeError, match='no CPU path'):
        pkg.anchor3d_loss(*args, num_classes=3, scale=torch.ones(4), with_iou=True)
    with pytest.raises(RuntimeError, match='no CPU path'):
        pkg.anchor3d_loss(*args[:2], None, *args[3:9], num_classes=3, scale=torch.ones(4))
    assert set(importlib.import_module('depth-from-motion_amd.anchor_loss').counters()) == {
        'kernel_launches', 'memsets', 'host_waits'}


class FocalLoss(object):
    def __init__(self, **kw):
        self.use_sigmoid, self.gamma, self.alpha, self.reduction, self.loss_weight = True, 2.0, 0.25, 'mean', 1.0
        vars(self).update(kw)


class SmoothL1Loss(object):
    def __init__(self, **kw):
        self.beta, self.reduction, self.loss_weight = 1.0 / 9.0, 'mean', 2.0
        vars(self).update(kw)


class CrossEntropyLoss(object):
    def __init__(self, **kw):
        self.use_sigmoid, self.use_mask, self.class_weight, self.reduction, self.loss_weight = False, False, None, 'mean', 0.2
        vars(self).update(kw)


class IOU3DLoss(object):
    def __init__(self, **kw):
        self.reduction, self.loss_weight = 'mean', 1.0
        vars(self).update(kw)


def stub_head(pkg, z, case, base=object):
    """a head with the attributes loss_single reads, set as make_golden_anchor_loss.py sets them for ``case``"""
    name = 'LIGAAnchor3DHead' if case.startswith('liga') or case == 'nopos' else 'Anchor3DHead'
    head = type(name, (pkg.HipAnchor3DLossMixin, base), {})()
    head.num_classes, head.box_code_size, head.use_sigmoid_cls = 3, 7, True
    head.use_direction_classifier = case != 'plain_nodir'
    head.diff_rad_by_sin = case != 'plain_cw'
    head.train_cfg = dict(code_weight=z['code_weight'].tolist() if case == 'plain_cw' else None)
    w = {k: float(z[f'weight/{k}']) for k in ('loss_cls', 'loss_bbox', 'loss_dir', 'loss_iou')}
    head.loss_cls, head.loss_bbox = FocalLoss(loss_weight=w['loss_cls']), SmoothL1Loss(loss_weight=w['loss_bbox'])
    head.loss_dir = CrossEntropyLoss(loss_weight=w['loss_dir'])
    head.loss_iou = IOU3DLoss(loss_weight=w['loss_iou']) if case.endswith('iou') else None
    if name == 'LIGAAnchor3DHead':
        head.normalizer_clamp_value, head.reduce_avg_factor = 10, 'reduce' in case
    nts = float(z[f'{case}/num_total_samples'])
    return head, (None if nts < 0 else int(nts))


@pytest.mark.parametrize('case', CASES)
def test_mixin_average_factors_match_the_reference_heads(pkg, z, case):
    """scale (the mixin's, on the host) times the fp64 term sums = what the reference's loss_single returned"""
    head, nts = stub_head(pkg, z, case)
    assert head._loss_single_unsupported() is None
    scale = head._loss_single_scale(nts, 2, torch.device('cpu'))
    assert scale.dtype == torch.float32 and scale.shape == (4,)
    args = inputs(z, z['nopos/labels'] if case == 'nopos' else None)
    if not head.use_direction_classifier:
        args[2] = None
    sums = ref.loss_terms(*args, num_classes=3, code_weight=head.train_cfg['code_weight'],
                          diff_rad_by_sin=head.diff_rad_by_sin, with_iou=head.loss_iou is not None)
    want = z[f'{case}/out']
    for i, s in enumerate(sums):
        if np.isnan(want[i]):
            assert float(scale[i]) == 0.0                      # a term the head does not have
            continue
        got = float(scale[i].double() * s)
        assert abs(got - want[i]) <= 2e-7 * abs(want[i]), (case, i, got, want[i])      # scale is one fp32 rounding


def test_mixin_falls_back_or_raises_for_what_the_kernels_do_not_do(pkg, al, z):
    class Reference(object):
        def loss_single(self, *args):
            return 'reference', args
    args = tuple(inputs(z)) + (41,)
    reasons = [
        (lambda h: setattr(h, 'use_sigmoid_cls', False), 'softmax classification'),
        (lambda h: setattr(h, 'loss_cls', CrossEntropyLoss()), 'loss_cls = CrossEntropyLoss'),
        (lambda h: setattr(h, 'loss_cls', FocalLoss(use_sigmoid=False)), 'without use_sigmoid'),
        (lambda h: setattr(h, 'loss_bbox', type('L1Loss', (), dict(reduction='mean'))()), 'loss_bbox = L1Loss'),
        (lambda h: setattr(h, 'loss_dir', CrossEntropyLoss(use_sigmoid=True)), 'not the softmax one'),
        (lambda h: setattr(h, 'loss_dir', CrossEntropyLoss(class_weight=[1.0, 2.0])), 'class_weight'),
        (lambda h: setattr(h, 'loss_dir', FocalLoss()), 'loss_dir = FocalLoss'),
        (lambda h: setattr(h, 'loss_iou', SmoothL1Loss()), 'loss_iou = SmoothL1Loss'),
        (lambda h: setattr(h, 'loss_bbox', SmoothL1Loss(reduction='sum')), "reduction='sum'"),
        (lambda h: setattr(h, 'loss_cls', FocalLoss(reduction='none')), "reduction='none'"),
        (lambda h: setattr(h, 'box_code_size', 17), '17 columns'),
        (lambda h: (setattr(h, 'box_code_size', 9), setattr(h, 'loss_iou', IOU3DLoss())), 'loss_iou on a box code of 9'),
    ]
    try:
        for change, word in reasons:
            head, _ = stub_head(pkg, z, 'liga', Reference)
            change(head)
            assert word in head._loss_single_unsupported()
            with pytest.warns(RuntimeWarning, match='not covered by the anchor-loss kernels'):
                assert head.loss_single(*args) == ('reference', args)
            head.fallback_policy = 'raise'
            with pytest.raises(pkg.MfmaPathError) as e:
                head.loss_single(*args)
            assert word in str(e.value)
            alone, _ = stub_head(pkg, z, 'plain')                 # no reference method: an error under 'warn' too
            change(alone)
            with pytest.raises(pkg.MfmaPathError, match='no reference method'):
                alone.loss_single(*args)
        # what the kernels do reaches them: CPU maps are refused there, not sent to the reference
        head, nts = stub_head(pkg, z, 'liga_iou', Reference)
        with pytest.raises(RuntimeError, match='no CPU path'):
            head.loss_single(*args)
    finally:
        importlib.import_module('depth-from-motion_amd.fallback').WARNED.clear()


def test_patch_reference_rebinds_both_head_classes(pkg, al, z):
    """loss_single of Anchor3DHead and of LIGAAnchor3DHead (which overrides it) are rebound where their modules are
    already imported, never imported for it; the replaced methods are kept per class; a second call changes nothing"""
    names = ('mmdet3d.models.dense_heads.anchor3d_head', 'mmdet3d.models.dense_heads.liga_anchor3d_head')
    chain = ('mmdet3d', 'mmdet3d.models', 'mmdet3d.models.dense_heads') + names
    before = {k: sys.modules.get(k) for k in chain}
    integ = importlib.import_module('depth-from-motion_amd.integration')
    fb = importlib.import_module('depth-from-motion_amd.fallback')
    nothing = {'modules': [], 'functions': [], 'methods': []}
    kept = dict(fb.REPLACED)
    try:
        for k in chain:
            sys.modules.pop(k, None)
        assert integ.apply_patches('anchor_loss') == nothing and not any(n in sys.modules for n in names)
        for k in chain:
            m = types.ModuleType(k)
            m.__path__ = []
            sys.modules[k] = m

        class Anchor3DHead(object):
            def loss_single(self, *args):
                return 'plain', args

        class LIGAAnchor3DHead(Anchor3DHead):
            def loss_single(self, *args):
                return 'liga', args
        originals = (Anchor3DHead.__dict__['loss_single'], LIGAAnchor3DHead.__dict__['loss_single'])
        both = ['Anchor3DHead.loss_single', 'LIGAAnchor3DHead.loss_single']
        sys.modules[names[0]].Anchor3DHead = Anchor3DHead
        assert integ.apply_patches('anchor_loss') == dict(nothing, methods=both[:1])   # the other file is not imported
        sys.modules[names[1]].LIGAAnchor3DHead = LIGAAnchor3DHead
        for _ in range(2):
            assert integ.apply_patches('anchor_loss') == dict(nothing, methods=both)
            for klass, original in zip((Anchor3DHead, LIGAAnchor3DHead), originals):
                assert klass.__dict__['loss_single'] is pkg.HipAnchor3DLossMixin.__dict__['loss_single']
                assert fb.REPLACED[f'{klass.__name__}.loss_single'] is original
        assert 'anchor_loss' in integ.PATCHES and 'anchor_head' in integ.PATCHES     # what patch_reference() iterates
        # each class falls back to its own replaced method
        args = tuple(inputs(z)) + (41,)
        for klass, tag in ((Anchor3DHead, 'plain'), (LIGAAnchor3DHead, 'liga')):
            head = klass()
            head.use_sigmoid_cls = False
            with pytest.warns(RuntimeWarning, match='softmax'):
                assert head.loss_single(*args) == (tag, args)
            fb.WARNED.clear()
    finally:
        fb.REPLACED.clear()
        fb.REPLACED.update(kept)
        fb.WARNED.clear()
        for k, v in before.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
