"""CPU: the box-decode feature above the kernels -- the fixture's cases, guards and error figures, the exported names,
the C ABI's symbols and argument checks, the refusal of CPU tensors, the mixin's fallback policy and
patch_reference's rebinding.

Fixture numbers (tests/golden/bbox_decode.npz, generator tests/golden/make_golden_bbox_decode.py): over every case the
fp32 CPU run of the reference differs from its fp64 run by at most ``fp32_score_error`` = 8.0e-8 in a score, by
``fp32_decode_error`` = 1.1e-6 (x, 20 m out) ... 1.2e-7 (the yaw: one addition) per box column, by ``fp32_bev_error``
<= 1.9e-6 per BEV column and by ``fp32_fixed_yaw_error`` = 3.3e-7 in the yaw after the direction fix.  The GPU tests
read these four."""
import ctypes
import importlib
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('dfm_anchor_head_candidates', 'dfm_anchor_head_candidates_workspace_bytes', 'dfm_delta_xyzwlhr_decode')
NAMES = ('delta_xyzwlhr_decode', 'anchor_head_candidates', 'anchor3d_get_bboxes', 'HipAnchor3DHeadMixin')
# case: (map sizes per level, B, C, S, nms_pre, compared in order, has the NMS results)
CASES = {'small': ([(5, 6)], 1, 3, 7, 64, 1, True), 'odd': ([(7, 9)], 1, 3, 7, 100, 1, True),
         'nocut': ([(5, 6)], 1, 3, 7, 4096, 1, True), 'nocut_neg': ([(5, 6)], 1, 3, 7, -1, 1, True),
         'batch': ([(20, 18)], 2, 3, 7, 512, 0, True), 'wide': ([(40, 36)], 1, 3, 7, 4096, 0, True),
         's9': ([(5, 6)], 1, 1, 9, 64, 1, True), 'levels': ([(5, 6), (3, 4)], 1, 3, 7, 32, 1, True),
         'ties': ([(7, 9)], 1, 3, 7, 100, 1, False), 'special': ([(7, 9)], 1, 3, 7, 100, 1, False)}


@pytest.fixture(scope='module')
def pkg():
    importlib.import_module('depth-from-motion_amd.build').build_hip()
    return importlib.import_module('depth-from-motion_amd')


@pytest.fixture(scope='module')
def z():
    return np.load(os.path.join(util.GOLDEN, 'bbox_decode.npz'))


def f32(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def keys64(z, case, level, b):
    C = int(z[f'{case}/num_classes'])
    logits = torch.from_numpy(z[f'{case}/cls{level}'])[b].double().permute(1, 2, 0).reshape(-1, C)
    return logits.sigmoid().max(1)[0].numpy()


def test_stored_error_figures_and_settings(z):
    assert 0 < float(z['fp32_score_error']) <= 8.0e-8                                        # the docstring's
    dec, bev = z['fp32_decode_error'], z['fp32_bev_error']
    assert dec.shape == (9,) and bev.shape == (5,) and np.all(np.isfinite(dec)) and np.all(np.isfinite(bev))
    assert np.all(dec[:7] > 0) and dec.max() <= 1.1e-6 and dec[6] <= 1.2e-7 < float(z['fp32_fixed_yaw_error']) <= 3.3e-7 and np.all(bev > 0) and bev.max() <= 2e-6
    assert np.all(dec[7:] == 0)              # bf16-exact deltas on zero anchor columns: t + 0 is exact
    assert float(z['guard']) == 1e-5 and float(z['dir_guard']) == 1e-4 and float(z['dir_logit_guard']) == 1e-3
    assert float(z['nms_guard_band']) == float(np.load(os.path.join(util.GOLDEN, 'box_nms.npz'))['guard_band'])
    assert float(z['dir_offset']) == 0.7854 and float(z['score_thr']) == 0.1 and float(z['nms_thr']) == 0.25
    assert os.path.getsize(os.path.join(util.GOLDEN, 'bbox_decode.npz')) < 1000 * 1000


@pytest.mark.parametrize('case', sorted(CASES))
def test_cases_are_stored_whole(z, case):
    shapes, B, C, S, nms_pre, ordered, with_nms = CASES[case]
    assert int(z[f'{case}/num_levels']) == len(shapes) and int(z[f'{case}/nms_pre']) == nms_pre
    assert (int(z[f'{case}/num_classes']), int(z[f'{case}/box_code_size']), int(z[f'{case}/ordered'])) == (C, S, ordered)
    K = 0
    for l, (H, W) in enumerate(shapes):
        N = H * W * 6
        assert z[f'{case}/cls{l}'].shape == (B, 6 * C, H, W) and z[f'{case}/cls{l}'].dtype == np.float32
        assert z[f'{case}/reg{l}_bf16'].shape == (B, 6 * S, H, W) and z[f'{case}/reg{l}_bf16'].dtype == np.uint16
        assert z[f'{case}/dir{l}_bf16'].shape == (B, 12, H, W) and z[f'{case}/anchors{l}'].shape == (N, S)
        K += nms_pre if 0 < nms_pre < N else N
    assert z[f'{case}/bboxes'].shape == (B, K, S) and z[f'{case}/bboxes'].dtype == np.float64
    assert z[f'{case}/bboxes_for_nms'].shape == (B, K, 5) and z[f'{case}/scores'].shape == (B, K, C)
    assert z[f'{case}/topk_inds'].shape == (B, K) and z[f'{case}/topk_inds'].dtype == np.int64
    assert z[f'{case}/dir_scores'].dtype == np.int64 and set(np.unique(z[f'{case}/dir_scores'])) <= {0, 1}
    for b in range(B):
        assert (f'{case}/out{b}_labels' in z.files) == with_nms
        if with_nms:
            n = len(z[f'{case}/out{b}_labels'])
            assert 0 < n <= int(z['max_num']) and z[f'{case}/out{b}_boxes'].shape == (n, S)
            assert np.all(z[f'{case}/out{b}_scores'] > float(z['score_thr']))
    # the stored rows are the decode of the stored inputs: the yaw column is delta + anchor, exactly in fp64
    if len(shapes) == 1:
        H, W = shapes[0]
        reg = f32(z[f'{case}/reg0_bf16']).astype(np.float64)
        for b in range(B):
            n = z[f'{case}/topk_inds'][b]
            a, pos = n % 6, n // 6
            yaw = reg[b, a * S + 6, pos // W, pos % W] + z[f'{case}/anchors0'][n, 6].astype(np.float64)
            assert np.allclose(z[f'{case}/bboxes'][b, :, 6], yaw, rtol=1e-9, atol=0)
            assert np.array_equal(z[f'{case}/bboxes_for_nms'][b, :, 4], z[f'{case}/bboxes'][b, :, 6])


@pytest.mark.parametrize('case', ('small', 'odd', 'batch', 'wide', 's9', 'levels'))
def test_key_guards_hold(z, case):
    shapes, B, C, S, nms_pre, ordered, _ = CASES[case]
    guard, at = float(z['guard']), 0
    for l, (H, W) in enumerate(shapes):
        for b in range(B):
            k = keys64(z, case, l, b)
            order = np.argsort(-k, kind='stable')
            assert k[order[nms_pre - 1]] - k[order[nms_pre]] >= guard
            got = z[f'{case}/topk_inds'][b, at:at + nms_pre]
            if ordered:
                assert np.all(-np.diff(k[order[:nms_pre]]) >= guard) and np.array_equal(got, order[:nms_pre])
            else:
                assert np.array_equal(np.sort(got), np.sort(order[:nms_pre]))
        at += nms_pre


def test_direction_guards_hold(z):
    for case, (shapes, B, C, S, _, _, with_nms) in CASES.items():
        for l in range(len(shapes)):
            pair = f32(z[f'{case}/dir{l}_bf16']).astype(np.float64).reshape(B, 6, 2, *shapes[l])
            gap = np.abs(pair[:, :, 0] - pair[:, :, 1])
            if case == 'special':
                assert (gap == 0).sum() == 1 and np.sort(gap.ravel())[1] >= float(z['dir_logit_guard'])
            else:
                assert gap.min() >= float(z['dir_logit_guard'])
        for b in range(B if with_nms else 0):
            q = (z[f'{case}/out{b}_boxes'][:, 6] - float(z['dir_offset'])) / np.pi + float(z['dir_limit_offset'])
            assert np.abs(q - np.round(q)).min() >= float(z['dir_guard']) * 0.999      # (the fixed yaw, a period off)


@pytest.mark.parametrize('case', [c for c, v in CASES.items() if v[6]])
def test_scores_the_nms_can_order_are_distinct(z, case):
    """box3d_multiclass_nms leaves the order of equal scores undefined (per class, and across the classes at its
    max_num cut): every score of an image above score_thr is score_gap from the next"""
    shapes, B = CASES[case][0], CASES[case][1]
    assert float(z['score_gap']) == 1e-6 > 12 * float(z['fp32_score_error'])
    for b in range(B):
        v = np.concatenate([torch.from_numpy(z[f'{case}/cls{l}'][b]).double().sigmoid().numpy().ravel()
                            for l in range(len(shapes))]) if len(shapes) == 1 else None
        if v is None:                       # several levels meet in one NMS call: the kept candidates' scores
            v = z[f'{case}/scores'][b].ravel()
        v = np.sort(v[v > float(z['score_thr'])])
        assert len(v) > 10 and np.diff(v).min() >= float(z['score_gap'])


def test_ties_and_special_cases_are_what_they_claim(z):
    k = keys64(z, 'ties', 0, 0)
    values, counts = np.unique(k, return_counts=True)
    assert len(values) == 4 and counts.max() >= 100
    order = np.argsort(-k, kind='stable')[:100]
    assert np.array_equal(z['ties/topk_inds'][0], order)                 # the rule: a stable descending argsort
    cut = k[order[-1]]
    assert (k == cut).sum() > (k[order] == cut).sum() > 1 and cut < k.max()          # the cut falls inside a tie
    cls = z['special/cls0']
    assert np.isposinf(cls).sum() == 1 and np.isneginf(cls).sum() == 1 and np.isnan(cls).sum() == 1
    assert (f32(z['special/reg0_bf16']) == 100).sum() == 1
    inds, scores, boxes = z['special/topk_inds'][0], z['special/scores'][0], z['special/bboxes'][0]
    assert np.isnan(scores[0]).sum() == 1 and scores[1].max() == 1.0      # NaN first, then the +inf logit's 1.0
    assert np.isinf(boxes).sum() == 1 and np.isinf(z['special/bboxes_for_nms'][0]).sum() == 2
    row = int(np.nonzero(np.isinf(boxes).any(1))[0][0])
    assert z['special/dir_scores'][0, row] == 0                           # the equal direction pair: index 0
    assert len(set(inds.tolist())) == 100
    low = np.nonzero(inds == (5 * 9 + 1) * 6 + 3)[0]                      # the -inf logit's anchor: where it is kept,
    assert np.all(scores[low, 0] == 0)                                    # its score is exactly 0


def test_names_are_exported(pkg):
    for name in NAMES:
        assert callable(getattr(pkg, name)) and name in pkg.__all__, name
    mod = importlib.import_module('depth-from-motion_amd.bbox_decode')
    assert set(NAMES) == set(mod.__all__)


def test_header_binding_and_library_agree_on_the_new_symbols(pkg):
    """that header, table and library agree is tests/test_capi_binding.py; here: what this header says of its own"""
    text = open(os.path.join(ROOT, 'include', 'dfm_hip_bbox_decode.h')).read()
    capi, lib = pkg._capi, pkg._capi.lib()
    assert all(n in capi.SIGNATURES and n in capi._BINDING['dfm_hip_bbox_decode.h'] for n in NEW)
    for phrase in ('cls[b][a * C + c][y][x]', 'reg[b][a * S + s][y][x]', 'dir[b][a * 2 + j][y][x]',
                   'n = (y * w + x) * A + a', 'ASCENDING anchor index', 'those with the lowest indices stay',
                   'A NaN key ranks above every number', 'K > DFM_BOX_NMS_MAX_N', 'S outside 7 .. 16'):
        assert phrase in text, phrase                                 # the semantics are stated in the header
    assert ctypes.sizeof(capi.AnchorHeadDesc) == 8 * 4 + 3 * 4 * 8
    assert int(re.search(r'#define DFM_ANCHOR_HEAD_MAX_BATCH (\d+)', text).group(1)) == capi.ANCHOR_HEAD_MAX_BATCH
    assert lib.dfm_version() == 3


def desc(pkg, **kw):
    d = pkg._capi.AnchorHeadDesc(batch=1, h=5, w=6, anchors_per_location=6, num_classes=3, box_code_size=7, nms_pre=64,
                                 dtype=0)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_bad_arguments_are_rejected_without_touching_the_gpu(pkg):
    lib = pkg._capi.lib()
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)      # 16-byte aligned host memory, never dereferenced
    unsupported = pkg._capi.DFM_ERR_UNSUPPORTED
    size = lib.dfm_anchor_head_candidates_workspace_bytes

    def call(d, ptrs=(p,) * 9, ws=p, ws_bytes=1 << 15):
        return lib.dfm_anchor_head_candidates(ctypes.byref(d) if d is not None else None, *ptrs, ws, ws_bytes, None)
    assert call(None) == -1
    for width in (6, 17):
        assert call(desc(pkg, box_code_size=width)) == unsupported and b'box_code_size' in lib.dfm_last_error()
    assert call(desc(pkg, batch=65)) == unsupported and b'DFM_ANCHOR_HEAD_MAX_BATCH' in lib.dfm_last_error()
    assert call(desc(pkg, h=60, w=60, nms_pre=-1)) == unsupported and b'DFM_BOX_NMS_MAX_N' in lib.dfm_last_error()
    assert call(desc(pkg, h=60, w=60, nms_pre=16385)) == unsupported
    assert call(desc(pkg, dtype=2)) == unsupported and b'dtype' in lib.dfm_last_error()
    assert call(desc(pkg, h=-1)) == -1 and call(desc(pkg, num_classes=0)) == -1
    assert call(desc(pkg, anchors_per_location=0)) == -1
    assert call(desc(pkg, batch=0)) == 0 and call(desc(pkg, h=0)) == 0                   # nothing to do: no-ops
    assert call(desc(pkg), ptrs=(p,) * 8 + (None,)) == -1 and b'NULL' in lib.dfm_last_error()
    assert call(desc(pkg), ptrs=(None,) + (p,) * 8) == -1
    # 180 anchors cut to 64: three histograms of 2048 bins, a counter, four words of selection state, one tie count,
    # 180 keys (to a 16-byte boundary), 64 candidates of 8 bytes
    need = 4 * (3 * 2048 + 1 + 4 + 1 + 180 + 2) + 64 * 8
    assert size(ctypes.byref(desc(pkg))) == need
    assert size(ctypes.byref(desc(pkg, nms_pre=4096))) == 0 and size(ctypes.byref(desc(pkg, nms_pre=-1))) == 0
    assert size(ctypes.byref(desc(pkg, box_code_size=5))) == 0 and size(None) == 0
    assert call(desc(pkg), ws=None) == -3 and call(desc(pkg), ws_bytes=need - 1) == -3
    assert b'workspace' in lib.dfm_last_error()
    assert call(desc(pkg), ws=ctypes.c_void_p(p.value + 8)) == -1 and b'aligned' in lib.dfm_last_error()
    dec = lib.dfm_delta_xyzwlhr_decode
    assert dec(p, p, -1, 7, p, None) == -1
    assert dec(p, p, 4, 6, p, None) == unsupported and dec(p, p, 4, 17, p, None) == unsupported
    assert dec(None, None, 0, 9, None, None) == 0
    assert dec(None, p, 4, 7, p, None) == -1 and b'NULL' in lib.dfm_last_error()


def test_cpu_tensors_are_refused(pkg):
    cls, reg, dirs, anchors = torch.zeros(1, 18, 5, 6), torch.zeros(1, 42, 5, 6), torch.zeros(1, 12, 5, 6), \
        torch.zeros(180, 7)
    cfg = dict(nms_pre=64, score_thr=0.1, max_num=500, use_rotate_nms=True, nms_thr=0.25)
    for call in (lambda: pkg.delta_xyzwlhr_decode(anchors, anchors),
                 lambda: pkg.anchor_head_candidates([cls], [reg], [dirs], [anchors], num_classes=3, nms_pre=64),
                 lambda: pkg.anchor3d_get_bboxes([cls], [reg], [dirs], [anchors], cfg, num_classes=3,
                                                 dir_offset=0.7854, dir_limit_offset=0)):
        with pytest.raises(RuntimeError, match='no CPU path'):
            call()


class LidarBoxes(object):
    def __init__(self, tensor, box_dim=7):
        self.tensor, self.box_dim = tensor, box_dim

    @property
    def bev(self):
        return self.tensor[:, [0, 1, 3, 4, 6]]


class CameraBoxes(LidarBoxes):
    @property
    def bev(self):                                        # the camera boxes' columns and reversed yaw
        bev = self.tensor[:, [0, 2, 3, 5, 6]].clone()
        bev[:, -1] = -bev[:, -1]
        return bev


def stand_in_head(pkg, base=object):
    class Head(pkg.HipAnchor3DHeadMixin, base):
        pass
    head = Head()
    head.num_classes, head.box_code_size, head.use_sigmoid_cls = 3, 7, True
    head.dir_offset, head.dir_limit_offset, head.test_cfg = 0.7854, 0, dict(nms_pre=64)
    return head


def test_mixin_falls_back_or_raises_for_what_the_kernel_does_not_do(pkg):
    class Reference(object):
        def get_bboxes(self, *args):
            return 'reference', args
    maps = ([torch.zeros(1, 18, 5, 6)], [torch.zeros(1, 42, 5, 6)], [torch.zeros(1, 12, 5, 6)])
    lidar, camera = [dict(box_type_3d=LidarBoxes)], [dict(box_type_3d=CameraBoxes)]
    try:
        head = stand_in_head(pkg, Reference)
        assert head._get_bboxes_unsupported(lidar) is None
        with pytest.warns(RuntimeWarning, match='bev'):
            assert head.get_bboxes(*maps, camera) == ('reference', (*maps, camera, None, False))
        head.use_sigmoid_cls = False
        with pytest.warns(RuntimeWarning, match='softmax'):
            assert head.get_bboxes(*maps, lidar, None, True) == ('reference', (*maps, lidar, None, True))
        head.fallback_policy = 'raise'
        with pytest.raises(pkg.MfmaPathError, match='softmax'):
            head.get_bboxes(*maps, lidar)
        head.use_sigmoid_cls = True
        with pytest.raises(pkg.MfmaPathError, match='CameraBoxes'):
            head.get_bboxes(*maps, camera)
        head.bbox_coder = type('CenterPointBBoxCoder', (), {})()
        with pytest.raises(pkg.MfmaPathError, match='box coder'):
            head.get_bboxes(*maps, lidar)
        # without a reference method to run it is an error under 'warn' as well
        alone = stand_in_head(pkg)
        with pytest.raises(pkg.MfmaPathError, match='no reference method'):
            alone.get_bboxes(*maps, camera)
        # what the kernel does do reaches it: CPU maps are refused there, not sent to the reference
        head = stand_in_head(pkg, Reference)
        head.anchor_generator = types.SimpleNamespace(grid_anchors=lambda sizes, device: [torch.zeros(180, 7)])
        with pytest.raises(RuntimeError, match='no CPU path'):
            head.get_bboxes(*maps, lidar)
    finally:
        importlib.import_module('depth-from-motion_amd.fallback').WARNED.clear()


def test_patch_reference_rebinds_a_stub_anchor3d_head_module(pkg):
    """Anchor3DHead.get_bboxes is rebound where its module is already imported, never imported for it, and reported
    under 'methods'; the replaced method is kept for the fallback policy"""
    name = 'mmdet3d.models.dense_heads.anchor3d_head'
    chain = ('mmdet3d', 'mmdet3d.models', 'mmdet3d.models.dense_heads', name)
    before = {k: sys.modules.get(k) for k in chain}
    integ = importlib.import_module('depth-from-motion_amd.integration')
    fb = importlib.import_module('depth-from-motion_amd.fallback')
    nothing = {'modules': [], 'functions': [], 'methods': []}
    kept = dict(fb.REPLACED)
    try:
        for k in chain:
            sys.modules.pop(k, None)
        assert integ.apply_patches('anchor_head') == nothing and name not in sys.modules
        for k in chain:
            m = types.ModuleType(k)
            m.__path__ = []
            sys.modules[k] = m

        class Anchor3DHead(object):
            def get_bboxes(self, *args):
                return 'reference', args
        original = Anchor3DHead.__dict__['get_bboxes']
        sys.modules[name].Anchor3DHead = Anchor3DHead
        done = dict(nothing, methods=['Anchor3DHead.get_bboxes'])
        assert integ.apply_patches('anchor_head') == done                      # what patch_reference reports
        assert Anchor3DHead.__dict__['get_bboxes'] is pkg.HipAnchor3DHeadMixin.__dict__['get_bboxes']
        assert fb.REPLACED['Anchor3DHead.get_bboxes'] is original
        assert integ.apply_patches('anchor_head') == done and fb.REPLACED['Anchor3DHead.get_bboxes'] is original
        assert 'anchor_head' in integ.PATCHES                                   # what patch_reference() iterates
        # a subclass (LIGAAnchor3DHead) inherits the rebound method; softmax heads go to the kept one
        head = type('LIGAAnchor3DHead', (Anchor3DHead,), {})()
        head.use_sigmoid_cls, head.box_code_size = False, 7
        args = ([torch.zeros(1, 18, 5, 6)], [torch.zeros(1, 42, 5, 6)], [torch.zeros(1, 12, 5, 6)],
                [dict(box_type_3d=LidarBoxes)], None, False)
        with pytest.warns(RuntimeWarning, match='softmax'):
            assert head.get_bboxes(*args) == ('reference', args)
    finally:
        fb.REPLACED.clear()
        fb.REPLACED.update(kept)
        fb.WARNED.clear()
        for k, v in before.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_two_patched_classes_fall_back_each_to_its_own_get_bboxes(pkg, monkeypatch):
    """a subclass that overrides get_bboxes and is patched too keeps its own original: the store is keyed
    'Class.method', not by the bare method name"""
    integ = importlib.import_module('depth-from-motion_amd.integration')
    fb = importlib.import_module('depth-from-motion_amd.fallback')
    name = 'mmdet3d.models.dense_heads.anchor3d_head'
    kept = dict(fb.REPLACED)
    try:
        fb.REPLACED.clear()

        class Anchor3DHead(object):
            def get_bboxes(self, *args):
                return 'plain', args

        class OtherHead(Anchor3DHead):
            def get_bboxes(self, *args):
                return 'other', args
        originals = {'Anchor3DHead.get_bboxes': Anchor3DHead.__dict__['get_bboxes'],
                     'OtherHead.get_bboxes': OtherHead.__dict__['get_bboxes']}
        monkeypatch.setitem(sys.modules, name, types.SimpleNamespace(Anchor3DHead=Anchor3DHead, OtherHead=OtherHead))
        assert integ.apply_patches('anchor_head')['methods'] == ['Anchor3DHead.get_bboxes']
        assert integ._apply_method(integ.Method(name, 'OtherHead', 'get_bboxes', pkg.HipAnchor3DHeadMixin)) == \
            ('methods', 'OtherHead.get_bboxes')
        assert fb.REPLACED == originals
        args = ([torch.zeros(1, 18, 5, 6)], [torch.zeros(1, 42, 5, 6)], [torch.zeros(1, 12, 5, 6)],
                [dict(box_type_3d=LidarBoxes)], None, False)
        for klass, tag in ((Anchor3DHead, 'plain'), (OtherHead, 'other'), (type('Sub', (OtherHead,), {}), 'other')):
            assert klass.get_bboxes is pkg.HipAnchor3DHeadMixin.__dict__['get_bboxes']
            head = klass()
            head.use_sigmoid_cls, head.box_code_size = False, 7
            with pytest.warns(RuntimeWarning, match='softmax'):
                assert head.get_bboxes(*args) == (tag, args)
            fb.WARNED.clear()
    finally:
        fb.REPLACED.clear()
        fb.REPLACED.update(kept)
        fb.WARNED.clear()
