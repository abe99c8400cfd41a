"""The 3-D anchor head's maps to boxes on the HIP path.

Mirror of ``Anchor3DHead.get_bboxes`` / ``get_bboxes_single`` (mmdet3d/models/dense_heads/anchor3d_head.py:407-547)
and of ``DeltaXYZWLHRBBoxCoder.decode`` (mmdet3d/core/bbox/coders/delta_xyzwhlr_bbox_coder.py:58-91).  mmdet is not a
dependency: the semantics are those stated in include/dfm_hip_bbox_decode.h (a part of include/dfm_hip.h).

Per image the reference regenerates every anchor, permutes and copies the three maps, runs a sigmoid over every class
logit, a row maximum, ``torch.topk`` over all anchors, four gathers, the 15-operation decode, ``xywhr2xyxyr`` and a
padding concatenation to keep ``nms_pre`` rows.  ``anchor_head_candidates`` is one call of
``dfm_anchor_head_candidates`` per level for the whole batch: a radix select over 32-bit keys on the device, then a
gather and decode of the kept rows only; the maps are read in place (NCHW, channels-last, any strides; fp32 or bf16),
nothing is copied to the host.  ``anchor3d_get_bboxes`` feeds the candidates to ``box3d_multiclass_nms`` (one count
copy per image, as that function documents) and makes the direction fix; ``HipAnchor3DHeadMixin.get_bboxes`` has the
reference method's signature.

Equal keys: ``torch.topk`` leaves their order undefined; here equal keys go in ascending anchor index, at the cut as
well.  CPU tensors are refused: there is no CPU path.
"""

import numpy as np
import torch

from . import _capi
from .box_nms import box3d_multiclass_nms
from .fallback import run_reference
from .derived import derived
from ._launch import DTYPES, STREAM, WS, launch, require_gpu

__all__ = ['delta_xyzwlhr_decode', 'anchor_head_candidates', 'anchor3d_get_bboxes', 'HipAnchor3DHeadMixin']

BEV_COLUMNS = (0, 1, 3, 4, 6)     # BaseInstance3DBoxes.bev (base_box3d.py:138-141): what the kernel builds


def delta_xyzwlhr_decode(anchors, deltas):
    """``DeltaXYZWLHRBBoxCoder.decode(anchors, deltas)``: ``(..., S)`` anchors and deltas, ``7 <= S <= 16`` ->
    ``(..., S)`` fp32 boxes, the columns beyond 7 as ``t + a``.  Inputs of any floating dtype or stride are
    converted to contiguous fp32."""
    require_gpu(anchors, 'anchors')
    require_gpu(deltas, 'deltas')
    if anchors.shape != deltas.shape or anchors.dim() < 1:
        raise ValueError(f'anchors and deltas have one shape (..., S), got {tuple(anchors.shape)} and '
                         f'{tuple(deltas.shape)}')
    width = anchors.shape[-1]
    a = anchors.detach().to(torch.float32).contiguous()
    t = deltas.detach().to(torch.float32).contiguous()
    out = torch.empty_like(a)
    launch('dfm_delta_xyzwlhr_decode', a, t, a.numel() // width if width else 0, width, out, STREAM)
    return out


def _level(cls, reg, dirs, anchors, num_classes, nms_pre, code):
    for name, t in (('cls_scores', cls), ('bbox_preds', reg), ('dir_cls_preds', dirs), ('anchors', anchors)):
        require_gpu(t, name)
    if cls.dim() != 4 or reg.dim() != 4 or dirs.dim() != 4:
        raise ValueError('the head\'s maps are (B, channels, H, W)')
    if not (cls.shape[0] == reg.shape[0] == dirs.shape[0] and cls.shape[2:] == reg.shape[2:] == dirs.shape[2:]):
        raise ValueError(f'the three maps of a level differ in batch or map size: {tuple(cls.shape)}, '
                         f'{tuple(reg.shape)}, {tuple(dirs.shape)}')
    if not cls.dtype == reg.dtype == dirs.dtype or cls.dtype not in DTYPES:
        raise TypeError(f'the three maps share one dtype, fp32 or bf16; got {cls.dtype}, {reg.dtype}, {dirs.dtype}')
    batch, _, h, w = cls.shape
    if num_classes <= 0 or cls.shape[1] % num_classes:
        raise ValueError(f'{cls.shape[1]} class channels are no multiple of num_classes = {num_classes}')
    per_loc = cls.shape[1] // num_classes
    if reg.shape[1] != per_loc * code or dirs.shape[1] != per_loc * 2:
        raise ValueError(f'{per_loc} anchors per location: bbox_preds need {per_loc * code} channels and dir_cls_preds '
                         f'{per_loc * 2}, got {reg.shape[1]} and {dirs.shape[1]}')
    n = h * w * per_loc
    if anchors.dim() != 2 or tuple(anchors.shape) != (n, code):
        raise ValueError(f'the anchors of a {h} x {w} map with {per_loc} per location are ({n}, {code}), got '
                         f'{tuple(anchors.shape)}')
    a = anchors.detach().to(torch.float32).contiguous()
    d = _capi.AnchorHeadDesc(batch=batch, h=h, w=w, anchors_per_location=per_loc, num_classes=num_classes,
                             box_code_size=code, nms_pre=int(nms_pre), dtype=DTYPES[cls.dtype])
    for field, t in ((d.cls_stride, cls), (d.reg_stride, reg), (d.dir_stride, dirs)):
        field[:] = t.stride()
    k = nms_pre if 0 < nms_pre < n else n
    device = cls.device
    bboxes = torch.empty((batch, k, code), dtype=torch.float32, device=device)
    for_nms = torch.empty((batch, k, 5), dtype=torch.float32, device=device)
    scores = torch.empty((batch, k, num_classes + 1), dtype=torch.float32, device=device)
    dir_scores = torch.empty((batch, k), dtype=torch.int64, device=device)
    inds = torch.empty((batch, k), dtype=torch.int64, device=device)
    launch('dfm_anchor_head_candidates', d, cls.detach(), reg.detach(), dirs.detach(), a, bboxes, for_nms, scores,
           dir_scores, inds, WS, STREAM, ws_bytes=_capi.lib().dfm_anchor_head_candidates_workspace_bytes(d))
    return bboxes, for_nms, scores, dir_scores, inds


def anchor_head_candidates(cls_scores, bbox_preds, dir_cls_preds, anchors, *, num_classes, nms_pre, box_code_size=7):
    """``get_bboxes_single`` up to its NMS call (anchor3d_head.py:487-533), for the whole batch.

    ``cls_scores`` / ``bbox_preds`` / ``dir_cls_preds``: per-level lists of ``(B, A*C, H, W)`` / ``(B, A*S, H, W)`` /
    ``(B, A*2, H, W)`` maps as the head returns them, fp32 or bf16, read in place whatever their strides;
    ``anchors``: per level ``(H*W*A, S)``.  Per level the ``nms_pre`` anchors with the greatest
    ``max_c sigmoid(logit)`` are kept per image in descending order (equal keys in ascending anchor index; all
    anchors in anchor order when ``nms_pre <= 0`` or there are no more than ``nms_pre``).

    Returns ``(bboxes (B, K, S), bboxes_for_nms (B, K, 5), scores (B, K, C + 1), dir_scores (B, K) int64,
    topk_inds (B, K) int64)``, the levels concatenated along ``K``; ``topk_inds`` index each level's own anchors.
    The outputs are fp32 whatever the maps' dtype: a bf16 map gives exactly what its ``.float()`` gives, all
    arithmetic being fp32, whereas the reference run on bf16 maps would round every intermediate to bf16.  Nothing
    is copied to the host."""
    if not (len(cls_scores) == len(bbox_preds) == len(dir_cls_preds) == len(anchors)) or not len(cls_scores):
        raise ValueError('cls_scores, bbox_preds, dir_cls_preds and anchors are per-level lists of one length')
    parts = [_level(c, r, d, a, int(num_classes), int(nms_pre), int(box_code_size))
             for c, r, d, a in zip(cls_scores, bbox_preds, dir_cls_preds, anchors)]
    if len(parts) == 1:
        return parts[0]
    return tuple(torch.cat([p[i] for p in parts], dim=1) for i in range(5))


def _cfg(cfg, name, *default):
    if isinstance(cfg, dict):
        return cfg.get(name, *default) if default else cfg[name]
    return getattr(cfg, name, *default)


def anchor3d_get_bboxes(cls_scores, bbox_preds, dir_cls_preds, anchors, cfg, *, num_classes, dir_offset,
                        dir_limit_offset, box_code_size=7):
    """``get_bboxes`` without the box class (anchor3d_head.py:407-545): the candidates, per image
    ``box3d_multiclass_nms`` (its one count copy to the host per image), then the direction fix
    ``yaw = limit_period(yaw - dir_offset, dir_limit_offset, pi) + dir_offset + pi * dir_score``.

    ``cfg`` supplies ``nms_pre`` (default -1), ``score_thr`` (default 0), ``max_num``, ``use_rotate_nms`` and
    ``nms_thr`` (attributes or keys, the head's ``test_cfg``).  Returns per image ``(bboxes (n, S), scores (n,),
    labels (n,))``."""
    bboxes, for_nms, scores, dir_scores, _ = anchor_head_candidates(
        cls_scores, bbox_preds, dir_cls_preds, anchors, num_classes=num_classes, nms_pre=_cfg(cfg, 'nms_pre', -1),
        box_code_size=box_code_size)
    score_thr, max_num = _cfg(cfg, 'score_thr', 0), _cfg(cfg, 'max_num')
    out = []
    for b in range(bboxes.shape[0]):
        boxes, kept_scores, labels, dirs = box3d_multiclass_nms(bboxes[b], for_nms[b], scores[b], score_thr, max_num,
                                                                cfg, dir_scores[b])
        if boxes.shape[0] > 0:
            val = boxes[..., 6] - dir_offset                                       # limit_period (utils.py:24)
            dir_rot = val - torch.floor(val / np.pi + dir_limit_offset) * np.pi
            boxes[..., 6] = dir_rot + dir_offset + np.pi * dirs.to(boxes.dtype)
        out.append((boxes, kept_scores, labels))
    return out


_STANDARD_BEV = {}


def _standard_bev(box_type, code):
    """whether ``box_type(tensor, box_dim=code).bev`` is the columns ``BEV_COLUMNS`` (the LiDAR and depth boxes; the
    camera boxes take other columns and turn the yaw): asked of the class once, on a one-row CPU probe"""
    key = (box_type, code)
    if key not in _STANDARD_BEV:
        probe = torch.arange(1, code + 1, dtype=torch.float32)[None]
        try:
            bev = box_type(probe.clone(), box_dim=code).bev
            ok = tuple(bev.shape) == (1, 5) and bool(torch.equal(bev, probe[:, list(BEV_COLUMNS)]))
        except Exception:  # noqa: BLE001  (a box class the probe cannot build is not one the kernel mirrors)
            ok = False
        _STANDARD_BEV[key] = ok
    return _STANDARD_BEV[key]


class HipAnchor3DHeadMixin(object):
    """``Anchor3DHead.get_bboxes`` (anchor3d_head.py:407-456) on the HIP path, for a head class
    ``class FastHead(HipAnchor3DHeadMixin, LIGAAnchor3DHead)`` (``patch_reference()`` rebinds the reference head's
    method to this one).  It reads ``self.anchor_generator``, ``self.num_classes``, ``self.box_code_size``,
    ``self.use_sigmoid_cls``, ``self.dir_offset``, ``self.dir_limit_offset`` and ``self.test_cfg`` as the reference
    does and returns its list: per image ``(input_meta['box_type_3d'](bboxes, box_dim=S), scores, labels)``.  The
    anchors are generated once per (feature map sizes, device) and kept in the head's ``derived.Derived`` cache.

    What the kernel does not do -- softmax classification (``use_sigmoid_cls=False``), a box class whose ``bev`` is
    not the columns (0, 1, 3, 4, 6) (camera boxes), a box coder other than ``DeltaXYZWLHRBBoxCoder`` -- follows
    the package's fallback policy: 'warn' says so once and calls the reference method, 'raise' makes it an
    ``MfmaPathError``; without a reference method to call it is an error either way."""

    def _get_bboxes_unsupported(self, input_metas):
        if not getattr(self, 'use_sigmoid_cls', True):
            return 'softmax classification (use_sigmoid_cls=False)'
        coder = type(getattr(self, 'bbox_coder', None)).__name__
        if coder not in ('DeltaXYZWLHRBBoxCoder', 'NoneType'):
            return f'the box coder {coder}'
        for meta in input_metas:
            if not _standard_bev(meta['box_type_3d'], self.box_code_size):
                return (f'the box class {getattr(meta["box_type_3d"], "__name__", meta["box_type_3d"])}, whose bev is '
                        f'not the columns {BEV_COLUMNS}')
        return None

    def _mlvl_anchors(self, featmap_sizes, device):
        def make():
            return [a.reshape(-1, self.box_code_size).to(torch.float32).contiguous()
                    for a in self.anchor_generator.grid_anchors(featmap_sizes, device=device)]
        return derived(self).get('get_bboxes_anchors', (), make, extra=(tuple(featmap_sizes), str(device)))

    def get_bboxes(self, cls_scores, bbox_preds, dir_cls_preds, input_metas, cfg=None, rescale=False):
        assert len(cls_scores) == len(bbox_preds)
        assert len(cls_scores) == len(dir_cls_preds)
        why = self._get_bboxes_unsupported(input_metas)
        if why is not None:
            return run_reference(self, 'get_bboxes', why, 'box-decode',
                                 (cls_scores, bbox_preds, dir_cls_preds, input_metas, cfg, rescale),
                                 mixin=HipAnchor3DHeadMixin)
        featmap_sizes = [tuple(int(v) for v in c.shape[-2:]) for c in cls_scores]
        anchors = self._mlvl_anchors(featmap_sizes, cls_scores[0].device)
        cfg = self.test_cfg if cfg is None else cfg
        results = anchor3d_get_bboxes(cls_scores, bbox_preds, dir_cls_preds, anchors, cfg,
                                      num_classes=self.num_classes, dir_offset=self.dir_offset,
                                      dir_limit_offset=self.dir_limit_offset, box_code_size=self.box_code_size)
        assert len(results) == len(input_metas)
        return [(meta['box_type_3d'](boxes, box_dim=self.box_code_size), scores, labels)
                for meta, (boxes, scores, labels) in zip(input_metas, results)]
