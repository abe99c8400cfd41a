"""CPU: the host side of the 2-D ATSS head's loss (depth-from-motion_amd/atss_loss.py, csrc/atss_loss.hip): the torch
restatement of the header's formulas (tests/atss_loss_ref.py) against tests/golden/atss_loss.npz (the reference's own
loss_single and centerness_target in fp64, tests/golden/make_golden_atss_loss.py), what the C ABI refuses before any
HIP call, the refusal of CPU tensors, the mixin's fallback rule and patch_reference's rebinding of LIGAATSSHead.loss."""
import ctypes
import importlib
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests import atss_loss_ref as ref
from tests import util

CASES = ('tiny', 'tiny_agn', 'kinks', 'five', 'empty', 'rules')
FIXTURE = os.path.join(util.GOLDEN, 'atss_loss.npz')


@pytest.fixture(scope='module')
def pkg():
    importlib.import_module('depth-from-motion_amd.build').build_hip()
    return importlib.import_module('depth-from-motion_amd')


@pytest.fixture(scope='module')
def z():
    return np.load(FIXTURE)


@pytest.fixture(scope='module')
def zt():
    return np.load(os.path.join(util.GOLDEN, 'atss_target.npz'))


def inputs(z, zt, case):
    """the stored inputs of a case as torch tensors on the host: three per-level map lists (fp32, NCHW), anchors
    (A, 4), labels (B, A), label_weights (B, A) and bbox_targets (B, A, 4) as the fp32 values the kernels read, and the
    keywords of the loss"""
    src = str(z[f'{case}/maps_of']) if f'{case}/maps_of' in z.files else case
    levels = len(z[f'{case}/level_hw'])
    maps = [[torch.from_numpy(z[f'{src}/{key}{l}']) for l in range(levels)] for key in ('cls', 'reg', 'ctr')]
    t = str(z[f'{case}/targets'])
    dense = (torch.from_numpy(zt[f'{t}/anchors']), torch.from_numpy(zt[f'{t}/labels']),
             torch.from_numpy(zt[f'{t}/label_weights'].astype(np.float32)),
             torch.from_numpy(zt[f'{t}/bbox_targets'].astype(np.float32)))
    kw = dict(num_classes=int(z['num_classes']), reg_class_agnostic=bool(z[f'{case}/reg_class_agnostic']),
              target_means=zt['target_means'].tolist(), target_stds=zt['target_stds'].tolist())
    return maps, dense, kw


def weights(z):
    return tuple(float(z[f'weight/{k}']) for k in ('loss_cls', 'loss_bbox', 'loss_centerness'))


@pytest.mark.parametrize('case', CASES)
def test_restatement_reproduces_the_reference_in_fp64(z, zt, case):
    """tests/atss_loss_ref.py, written from the header, run in fp64 on the stored inputs: the loss dict and the
    gradient of sum grad_out * loss with respect to every map, to 1e-12 relative (element by element; an element the
    reference has exactly 0 is exactly 0)"""
    maps, dense, kw = inputs(z, zt, case)
    leaves = [[m.double().requires_grad_(True) for m in kind] for kind in maps]
    t = str(z[f'{case}/targets'])
    terms = ref.loss_terms(*leaves, *dense, **kw)
    losses = ref.loss_dict(terms, int(zt[f'{t}/num_total_pos']), weights(z))
    out = torch.stack([torch.stack(losses[k]) for k in ('loss_cls', 'loss_bbox', 'loss_centerness')], 1)
    want = torch.from_numpy(z[f'{case}/loss'])
    assert out.shape == want.shape
    worst = float(((out.detach() - want).abs() / want.abs().clamp(min=1e-300)).max())
    assert bool(((want == 0) == (out.detach() == 0)).all())
    assert float(terms[3].clamp(min=1)) == pytest.approx(float(z[f'{case}/bbox_avg_factor']), rel=1e-13)
    total = (out * torch.from_numpy(z[f'{case}/grad_out'])).sum()
    flat = [m for kind in leaves for m in kind]
    grads = torch.autograd.grad(total, flat, allow_unused=True)
    L = len(maps[0])
    for i, (m, g) in enumerate(zip(flat, grads)):
        g = torch.zeros_like(m) if g is None else g
        w = torch.from_numpy(z[f"{case}/{('grad_cls', 'grad_reg', 'grad_ctr')[i // L]}{i % L}"])
        assert bool(((w == 0) == (g == 0)).all()), (case, i)
        worst = max(worst, float(((g - w).abs() / w.abs().clamp(min=1e-300)).max()))
    print(f'{case}: worst relative difference {worst:.3g}')
    assert worst <= 1e-12


def test_fixture_is_small_and_holds_its_figures(z):
    assert os.path.getsize(FIXTURE) < 512 * 1024
    for k in ('fp32_loss_error', 'fp32_grad_cls_error', 'fp32_grad_reg_error', 'fp32_grad_ctr_error'):
        assert 0 < float(z[k]) < 1e-5, k
    # a level without a positive: loss_bbox and loss_centerness exactly 0, and so are their gradients
    loss = z['empty/loss']
    assert not loss[1:, 1:].any() and loss[0].all() and loss[:, 0].all()
    assert all(not z[f'empty/{k}{l}'].any() for k in ('grad_reg', 'grad_ctr') for l in range(1, 5))


def desc(pkg, **over):
    d = pkg._capi.AtssLossDesc(batch=2, num_levels=2, num_anchors=30, num_classes=3, reg_class_agnostic=0,
                               dtype=pkg._capi.DFM_F32, reg_dtype=pkg._capi.DFM_F32, gamma=2.0, alpha=0.25)
    d.target_stds[:] = [0.1, 0.1, 0.2, 0.2]
    d.h[:2], d.w[:2], d.row_offset[:2] = [4, 2], [6, 3], [0, 24]
    for k, v in over.items():
        if isinstance(v, (list, tuple)):
            getattr(d, k)[:len(v)] = v
        else:
            setattr(d, k, v)
    return d


def test_unsupported_descriptors_are_refused_before_any_hip_call(pkg):
    """no GPU here: a HIP call would fail with DFM_ERR_HIP (-4), so -2 shows the refusal came first"""
    lib = pkg._capi.lib()
    unsupported = pkg._capi.DFM_ERR_UNSUPPORTED
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    table = (ctypes.c_void_p * 24)(*[p.value] * 24)
    fwd = lambda d: lib.dfm_atss_loss_fwd(ctypes.byref(d), table, p, p, p, p, p, p, 1 << 20, None)  # noqa: E731
    bwd = lambda d: lib.dfm_atss_loss_bwd(ctypes.byref(d), table, p, p, p, p, p, table, None)  # noqa: E731
    size = lambda d: lib.dfm_atss_loss_workspace_bytes(ctypes.byref(d))  # noqa: E731
    rules = [(dict(num_levels=9), b'levels'), (dict(num_classes=0), b'num_classes'), (dict(dtype=2), b'dtype'),
             (dict(reg_dtype=3), b'dtype'),
             (dict(batch=1 << 10, num_anchors=1 << 30, h=[1 << 10, 1 << 10], w=[1 << 10, 1 << 10],
                   row_offset=[0, 1 << 20]), b'2^31'),
             (dict(batch=1, num_anchors=1 << 30, h=[1 << 16, 1], w=[1 << 15, 1], row_offset=[0, 0]), b'2^31')]
    for over, word in rules:
        for call in (fwd, bwd):
            assert call(desc(pkg, **over)) == unsupported, over
            assert word in lib.dfm_last_error(), (over, lib.dfm_last_error())
        assert size(desc(pkg, **over)) == 0
    # 60 rows: one workgroup of 256, one partial row of 3 * 8 + 1 floats; 2^31 - 1 rows exactly are taken
    assert size(desc(pkg)) == 25 * 4
    assert size(desc(pkg, batch=1, num_anchors=(1 << 31) - 1, h=[1, 0], w=[(1 << 31) - 1, 0],
                     row_offset=[0, 0])) == 25 * 4 * (1 << 23)
    # empty input: the backward launches nothing and says OK; nothing is read, NULL included
    for over in (dict(batch=0), dict(h=[0, 0]), dict(w=[0, 0])):
        assert lib.dfm_atss_loss_bwd(ctypes.byref(desc(pkg, **over)), *[None] * 7, None) == 0
        assert size(desc(pkg, **over)) == 0
    assert bwd(desc(pkg, num_levels=0)) == -1 and bwd(desc(pkg, batch=-1)) == -1
    assert bwd(desc(pkg, row_offset=[0, 25])) == -1 and b'outside' in lib.dfm_last_error()
    assert lib.dfm_atss_loss_bwd(ctypes.byref(desc(pkg)), None, p, p, p, p, p, table, None) == -1
    assert b'NULL' in lib.dfm_last_error()


def test_cpu_tensors_are_refused(pkg, z, zt):
    maps, dense, kw = inputs(z, zt, 'tiny')
    with pytest.raises(RuntimeError, match='no CPU path'):
        pkg.atss_loss_2d(*maps, *dense, **kw)
    al = importlib.import_module('depth-from-motion_amd.atss_loss')
    assert set(al.counters()) == {'kernel_launches', 'memsets', 'host_waits'}
    assert 'atss_loss_2d' in pkg.__all__ and 'HipATSSLossMixin' in pkg.__all__


def test_the_three_symbols_are_in_the_library(pkg):
    fresh = ctypes.CDLL(pkg._capi.LIB_PATH)
    for name in ('dfm_atss_loss_workspace_bytes', 'dfm_atss_loss_fwd', 'dfm_atss_loss_bwd'):
        assert hasattr(fresh, name) and name in pkg._capi.SIGNATURES
    assert pkg._capi.STRUCTS['dfm_atss_loss_desc'] is pkg._capi.AtssLossDesc


class FocalLoss(object):
    def __init__(self, **kw):
        self.use_sigmoid, self.gamma, self.alpha, self.reduction, self.loss_weight = True, 2.0, 0.25, 'mean', 1.0
        vars(self).update(kw)


class GIoULoss(object):
    def __init__(self, **kw):
        self.eps, self.reduction, self.loss_weight = 1e-6, 'mean', 2.0
        vars(self).update(kw)


class CrossEntropyLoss(object):
    def __init__(self, **kw):
        self.use_sigmoid, self.use_mask, self.class_weight, self.reduction, self.loss_weight = True, False, None, 'mean', 1.0
        vars(self).update(kw)


def configure(head, z, agnostic):
    """the attributes HipATSSLossMixin.loss reads beyond those of the target mixin, set as the fixture's head"""
    w = weights(z)
    head.num_classes, head.num_reg_channel, head.num_anchors = int(z['num_classes']), 4, 1
    head.reg_class_agnostic, head.reg_avg_factor, head.seperate_extra_reg_branch = agnostic, 'default', False
    head.use_sigmoid_cls = True
    head.loss_cls, head.loss_bbox = FocalLoss(loss_weight=w[0]), GIoULoss(loss_weight=w[1])
    head.loss_centerness = CrossEntropyLoss(loss_weight=w[2])
    return head


def test_mixin_falls_back_or_raises_for_what_the_kernels_do_not_do(pkg, z, zt):
    class Reference(object):
        def loss(self, *args):
            return 'reference', args

        def loss_single(self, *args):
            return 'reference loss_single'
    maps, dense, kw = inputs(z, zt, 'tiny')
    args = (*maps, [torch.zeros(0, 6)], [torch.zeros(0, dtype=torch.int64)], [dict(img_shape=(32, 48, 3))], None)
    reasons = [
        (lambda h: setattr(h, 'reg_avg_factor', 'sum_centerness'), "reg_avg_factor='sum_centerness'"),
        (lambda h: setattr(h, 'num_reg_channel', 6), '6 regression channels'),
        (lambda h: setattr(h, 'loss_cls', CrossEntropyLoss()), 'loss_cls = CrossEntropyLoss'),
        (lambda h: setattr(h, 'loss_cls', FocalLoss(use_sigmoid=False)), 'without use_sigmoid'),
        (lambda h: setattr(h, 'loss_bbox', type('IoULoss', (), dict(reduction='mean'))()), 'loss_bbox = IoULoss'),
        (lambda h: setattr(h, 'loss_bbox', GIoULoss(reduction='sum')), "reduction='sum'"),
        (lambda h: setattr(h, 'loss_centerness', CrossEntropyLoss(use_sigmoid=False)), 'not the sigmoid one'),
        (lambda h: setattr(h, 'loss_centerness', FocalLoss()), 'loss_centerness = FocalLoss'),
        (lambda h: setattr(h, 'num_anchors', 3), '3 anchors per location'),
    ]
    fb = importlib.import_module('depth-from-motion_amd.fallback')
    try:
        for change, word in reasons:
            head = configure(type('LIGAATSSHead', (pkg.HipATSSLossMixin, Reference), {})(), z, False)
            change(head)
            assert word in head._atss_loss_unsupported(2)
            with pytest.warns(RuntimeWarning, match='not covered by the ATSS-loss kernels'):
                assert head.loss(*args) == ('reference', args)
            head.fallback_policy = 'raise'
            with pytest.raises(pkg.MfmaPathError) as e:
                head.loss(*args)
            assert word in str(e.value)
            alone = configure(type('LIGAATSSHead', (pkg.HipATSSLossMixin,), {})(), z, False)
            change(alone)                                        # no reference method: an error under 'warn' too
            with pytest.raises(pkg.MfmaPathError, match='no reference method'):
                alone.loss(*args)
        # the mixin defines no loss_single: the kept reference loss finds the reference's own
        assert 'loss_single' not in vars(pkg.HipATSSLossMixin)
        assert type('H', (pkg.HipATSSLossMixin, Reference), {})().loss_single() == 'reference loss_single'
        functions = lambda k: {n for n, f in vars(k).items() if isinstance(f, types.FunctionType)}  # noqa: E731
        assert not functions(pkg.HipATSSLossMixin) & functions(pkg.HipATSSTargetMixin)      # both land on one class
    finally:
        fb.WARNED.clear()


def test_patch_reference_rebinds_a_stub_liga_atss_head_loss(pkg, z, zt):
    """LIGAATSSHead.loss is rebound where its module is already imported, and never imported for it; the inherited
    method is kept for the fallback policy; applying twice changes nothing; the 'atss_target' group reports what it
    did before"""
    name = 'mmdet3d.models.dense_heads.liga_atss_head'
    chain = ('mmdet3d', 'mmdet3d.models', 'mmdet3d.models.dense_heads', name)
    before = {k: sys.modules.get(k) for k in chain}
    integ = importlib.import_module('depth-from-motion_amd.integration')
    fb = importlib.import_module('depth-from-motion_amd.fallback')
    nothing = {'modules': [], 'functions': [], 'methods': []}
    kept = dict(fb.REPLACED)
    try:
        for k in chain:
            sys.modules.pop(k, None)
        assert integ.apply_patches('atss_loss') == nothing and name not in sys.modules
        for k in chain:
            m = types.ModuleType(k)
            m.__path__ = []
            sys.modules[k] = m

        class ATSSHead(object):
            def loss(self, *args):
                return 'reference', args, self.loss_single()

            def get_targets(self, *args):
                return 'reference targets'

        class LIGAATSSHead(ATSSHead):
            def loss_single(self, *args):
                return 'the reference loss_single'
        original = ATSSHead.__dict__['loss']
        sys.modules[name].LIGAATSSHead = LIGAATSSHead
        done = dict(nothing, methods=['LIGAATSSHead.loss'])
        for _ in range(2):
            assert integ.apply_patches('atss_loss') == done
            assert LIGAATSSHead.__dict__['loss'] is pkg.HipATSSLossMixin.__dict__['loss']
            assert ATSSHead.__dict__['loss'] is original and fb.REPLACED['LIGAATSSHead.loss'] is original
            assert LIGAATSSHead.__dict__['_atss_loss_unsupported'] is pkg.HipATSSLossMixin.__dict__[
                '_atss_loss_unsupported']
            assert 'get_targets' not in vars(LIGAATSSHead) and 'loss_single' in vars(LIGAATSSHead)
        assert integ.apply_patches('atss_target') == dict(nothing, methods=['LIGAATSSHead.get_targets'])
        assert integ.apply_patches('atss_loss') == done and 'atss_loss' in integ.PATCHES
        # an unsupported setting goes to the kept method, which finds the reference's own loss_single
        maps, _, _ = inputs(z, zt, 'tiny')
        args = (*maps, [torch.zeros(0, 6)], [torch.zeros(0, dtype=torch.int64)], [dict()], None)
        head = configure(LIGAATSSHead(), z, False)
        head.reg_avg_factor = 'sum_centerness'
        with pytest.warns(RuntimeWarning, match='sum_centerness'):
            assert head.loss(*args) == ('reference', args, 'the reference loss_single')
        head.fallback_policy = 'raise'
        with pytest.raises(pkg.MfmaPathError, match='sum_centerness'):
            head.loss(*args)
    finally:
        fb.REPLACED.clear()
        fb.REPLACED.update(kept)
        fb.WARNED.clear()
        for k, v in before.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
