"""Generate tests/golden/bbox_decode.npz: the 3-D anchor head's maps to NMS candidates and to boxes.

Run in the build container only (needs the reference checkout):   python tests/golden/make_golden_bbox_decode.py

Executed unmodified, lifted by AST as make_golden_anchor_target.py does (the files cannot be imported: they need
mmcv / mmdet):
  * ``Anchor3DHead.get_bboxes`` and ``get_bboxes_single`` (models/dense_heads/anchor3d_head.py:407-547);
  * ``DeltaXYZWLHRBBoxCoder.decode`` (core/bbox/coders/delta_xyzwhlr_bbox_coder.py:58-91);
  * ``xywhr2xyxyr`` and ``limit_period`` (core/bbox/structures/utils.py, their array-converter decorators taken
    off: tensors only here) and ``BaseInstance3DBoxes.bev`` (core/bbox/structures/base_box3d.py:138-141);
  * ``Anchor3DRangeGenerator`` (core/anchor/anchor_3d_generator.py, its registry decorator taken off);
  * ``box3d_multiclass_nms`` / ``nms_bev`` (core/post_processing/box3d_nms.py) over the fp64 stand-ins for mmcv's
    ``nms_rotated`` / ``nms`` that make_golden_box_nms.py restates.
Nothing of the reference is stored, only inputs and the outputs it produced.

The call of ``box3d_multiclass_nms`` inside ``get_bboxes_single`` is wrapped to record its arguments: they are the
candidates (``bboxes``, ``bboxes_for_nms``, ``scores``, ``dir_scores``).  ``topk_inds`` is ``max_scores.topk(nms_pre)``
repeated outside with the reference's own expressions and checked against the recorded rows.

Inputs.  Class logits are fp32.  Box deltas and direction logits are bf16-exact and stored as their 16 upper bits
(``*_bf16`` arrays, uint16; value = bits << 16 as fp32), which is what keeps the file under 1 MB.  Expected values
are fp64, rounded to 32 significant bits (relative 2.3e-10: under 1 % of the smallest bound a test derives from the
fp32 error figures) so that the zlib container can drop the low bytes of each: without it the file does not fit.
For the same reason the class logits are drawn on a 2^-12 grid (exact in fp32).

Every case runs twice, in fp64 (the stored fp32 inputs cast up; the expected outputs) and in fp32 on the CPU.
Stored error figures, read by the GPU tests (nothing is written into a test), each the largest |fp64 - fp32| over
the finite values of all cases:
  fp32_score_error        of any sigmoid score
  fp32_decode_error       per column of the candidates' ``bboxes`` (9 columns: 7 and 8 from the S = 9 case)
  fp32_bev_error          per column of ``bboxes_for_nms`` (a half-size subtracted from or added to a centre: one
                          more rounding at the centre's magnitude than the ``bboxes`` columns it is made of, so
                          it has a figure of its own)
  fp32_fixed_yaw_error    of the yaw column of the boxes ``get_bboxes`` returns, which has been through the
                          direction fix (seven more fp32 operations at magnitude pi); the other columns of those
                          boxes are candidates' values and are held to fp32_decode_error

Discrete results must not hang on rounding.  Asserted for every case; a draw that violates one is redrawn (the
next seed), no case is dropped:
  * the K-th and (K+1)-th greatest keys differ by at least GUARD = 1e-5 in fp64 (every case with a cut);
  * in the cases compared in order, all kept keys are pairwise at least GUARD apart;
  * every box kept by the NMS has (r - dir_offset) / pi + dir_limit_offset at least DIR_GUARD = 1e-4 from an
    integer;
  * the two direction logits of every anchor differ by at least 1e-3 (by construction), except the one equal
    pair of ``special``;
  * no two candidates that the NMS can compare (both above score_thr in a common class) have a rotated IoU
    within make_golden_box_nms.GUARD_BAND of nms_thr (the xy deltas of an offending box are redrawn);
  * all scores of an image that the NMS can see (above score_thr, whatever the class: the max_num cut orders the
    classes together) are pairwise at least SCORE_GAP = 1e-6 apart (by construction: live logits sit on distinct
    points of the 2^-12 grid), a dozen times the fp32 score error: box3d_multiclass_nms leaves the order of equal
    scores undefined;
  * the fp32 and fp64 runs agree on every index, direction bin and label.

Cases: config K's sizes, rotations, dir_offset 0.7854, score_thr 0.1, nms_thr 0.25, rotated NMS, max_num 500.
  small    5 x 6   (180 anchors: under one block)     B = 1  nms_pre 64    compared in order
  odd      7 x 9   (378: no multiple of 64)           B = 1  nms_pre 100   compared in order
  nocut    small's maps, nms_pre 4096 >= N; nocut_neg: nms_pre -1: all anchors in anchor order
  batch    20 x 18 (2160: several workgroups)         B = 2  nms_pre 512   compared as a set: 512 kept keys between
           0.1 and 1 that are pairwise 1e-5 apart do not come out of a random draw (about nine pairs closer than
           that are expected per image), and keys placed by hand would no longer be a detector's; the test checks
           the set, then the order on the call's own keys
  wide     40 x 36 (8640)                             B = 1  nms_pre 4096  the shipped K; compared as a set
  s9       5 x 6, S = 9 (two velocity columns), C = 1        nms_pre 64    compared in order
  levels   two levels, 5 x 6 and 3 x 4                B = 1  nms_pre 32    compared in order
  ties     7 x 9, class logits drawn from four values: hundreds of equal keys, the cut inside a tie.  Expected:
           the library's rule (a stable descending argsort of the keys in numpy) applied to the rows the
           reference computes without a cut -- not torch.topk, whose order among equal keys is undefined
  special  odd's shape with a +inf logit, a -inf logit, a NaN logit, a size delta of 100 (exp overflows in fp32,
           not in fp64: where the fp32 run is not finite its value is the expected one) and an equal direction
           pair; up to the NMS call only, compared with NaN equal to NaN
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402
import make_golden_anchor_target as at  # noqa: E402
import make_golden_box_nms as nb  # noqa: E402

GUARD = 1e-5
DIR_GUARD = 1e-4
DIR_LOGIT_GUARD = 1e-3
DIR_OFFSET, DIR_LIMIT_OFFSET = 0.7854, 0
SCORE_THR, NMS_THR, MAX_NUM = 0.1, 0.25, 500
KEEP_BITS = 32
SCORE_GAP = 1e-6
LIVE_LOGIT = -2.3                # sigmoid(-2.3) = 0.091, below score_thr


class Cfg(dict):
    """the head's test_cfg: keys readable as attributes, as mmcv's ConfigDict"""
    __getattr__ = dict.__getitem__


def bf16_exact(x):
    """fp32 values rounded to the nearest bf16 (ties to even)"""
    return torch.from_numpy(np.asarray(x, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def bf16_bits(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    assert np.all(u & 0xffff == 0), 'not bf16-exact'
    return (u >> 16).astype(np.uint16)


def keep_bits(x):
    """fp64 rounded to KEEP_BITS significant bits; non-finite values untouched"""
    x = np.asarray(x, np.float64).copy()
    fin = np.isfinite(x)
    m, e = np.frexp(x[fin])
    x[fin] = np.ldexp(np.round(m * 2.0 ** KEEP_BITS) / 2.0 ** KEEP_BITS, e)
    return x


def load_reference():
    mmcv = types.SimpleNamespace(is_list_of=lambda seq, kind: isinstance(seq, list) and
                                 all(isinstance(x, kind) for x in seq))              # (the stand-in of
    g = {'torch': torch, 'np': np, 'mmcv': mmcv}                                     # make_golden_anchor_target.py)
    at.lift(mg.REF + 'core/bbox/structures/utils.py', ['limit_period', 'xywhr2xyxyr'], g)
    mg.extract_method(mg.REF + 'core/bbox/structures/base_box3d.py', 'BaseInstance3DBoxes', 'bev', g)
    bev = property(g.pop('bev'))

    def init(self, tensor, box_dim=7):
        self.tensor, self.box_dim = tensor, box_dim
    g['Boxes'] = type('Boxes', (), dict(__init__=init, bev=bev))
    mg.extract_method(mg.REF + 'core/bbox/coders/delta_xyzwhlr_bbox_coder.py', 'DeltaXYZWLHRBBoxCoder', 'decode', g)
    at.lift(mg.REF + 'core/anchor/anchor_3d_generator.py', ['Anchor3DRangeGenerator'], g)
    nms = {'torch': torch, 'nms_rotated': nb.nms_rotated, 'nms': nb.nms}
    mg.extract(mg.REF + 'core/post_processing/box3d_nms.py', ['box3d_multiclass_nms', 'nms_bev', 'nms_normal_bev'], nms)
    g['_nms'] = nms['box3d_multiclass_nms']
    g['_seen'] = []
    g['_skip_nms'] = False

    def recording_nms(mlvl_bboxes, mlvl_bboxes_for_nms, mlvl_scores, score_thr, max_num, cfg, mlvl_dir_scores=None):
        g['_seen'].append((mlvl_bboxes.clone(), mlvl_bboxes_for_nms.clone(), mlvl_scores.clone(),
                           mlvl_dir_scores.clone()))
        if g['_skip_nms']:
            return (mlvl_bboxes[:0], mlvl_scores[:0, 0], mlvl_dir_scores[:0], mlvl_dir_scores[:0])
        return g['_nms'](mlvl_bboxes, mlvl_bboxes_for_nms, mlvl_scores, score_thr, max_num, cfg, mlvl_dir_scores)
    g['box3d_multiclass_nms'] = recording_nms
    for name in ('get_bboxes', 'get_bboxes_single'):
        mg.extract_method(mg.REF + 'models/dense_heads/anchor3d_head.py', 'Anchor3DHead', name, g)
    g['Head'] = type('Head', (), dict(get_bboxes=g['get_bboxes'], get_bboxes_single=g['get_bboxes_single']))
    return g


def make_anchors(g, H, W, S):
    """(H * W * 6, S) fp32: config K's three sizes x two rotations on a 0.5 m grid"""
    if S == 7:
        return at.make_anchors(g, H, W).reshape(-1, 7)
    x0, y0 = 2.0, -H / 4
    ranges = [[x0, y0, z, x0 + at.STRIDE * (W - 1), y0 + at.STRIDE * (H - 1), z] for z in at.Z]
    gen = g['Anchor3DRangeGenerator'](ranges=ranges, sizes=at.SIZES, rotations=at.ROTATIONS,
                                      custom_values=[0.0] * (S - 7))
    anchors = gen.grid_anchors([(H, W)], device='cpu')[0]
    assert anchors.shape == (H * W * 6, S) and anchors.dtype == torch.float32
    return anchors


def run(g, levels, dtype, C, S, nms_pre, skip_nms=False):
    """the reference's get_bboxes in ``dtype`` over ``levels`` = [(cls, reg, dir, anchors)], fp32 arrays ->
    (per image candidates dict, per image results dict)"""
    head = g['Head']()
    head.num_classes, head.box_code_size, head.use_sigmoid_cls = C, S, True
    head.bbox_coder = types.SimpleNamespace(decode=g['decode'])
    head.dir_offset, head.dir_limit_offset = DIR_OFFSET, DIR_LIMIT_OFFSET
    head.test_cfg = Cfg(use_rotate_nms=True, nms_across_levels=False, nms_pre=nms_pre, nms_thr=NMS_THR,
                        score_thr=SCORE_THR, min_bbox_size=0, max_num=MAX_NUM)
    anchors = [torch.from_numpy(a).to(dtype) for _, _, _, a in levels]
    head.anchor_generator = types.SimpleNamespace(grid_anchors=lambda sizes, device: anchors)
    maps = [[torch.from_numpy(l[i]).to(dtype) for l in levels] for i in range(3)]
    B = maps[0][0].shape[0]
    g['_seen'].clear()
    g['_skip_nms'] = skip_nms
    with np.errstate(all='ignore'):
        results = head.get_bboxes(maps[0], maps[1], maps[2], [dict(box_type_3d=g['Boxes'])] * B)
    assert len(g['_seen']) == B
    cands, outs = [], []
    for b in range(B):
        bboxes, for_nms, scores, dirs = g['_seen'][b]
        assert scores.shape[1] == C + 1 and torch.all(scores[:, C] == 0) and dirs.dtype == torch.int64
        inds = []
        for cls, _, _, _ in zip(*maps, anchors):                      # anchor3d_head.py:498-513, repeated
            s = cls[b].permute(1, 2, 0).reshape(-1, C).sigmoid()
            if nms_pre > 0 and s.shape[0] > nms_pre:
                inds.append(s.max(dim=1)[0].topk(nms_pre)[1])
            else:
                inds.append(torch.arange(s.shape[0]))
        rows = torch.cat([cls[b].permute(1, 2, 0).reshape(-1, C).sigmoid()[i] for cls, i in zip(maps[0], inds)])
        assert torch.equal(torch.nan_to_num(rows, nan=-7.0), torch.nan_to_num(scores[:, :C], nan=-7.0))
        cands.append(dict(bboxes=bboxes.double().numpy(), bboxes_for_nms=for_nms.double().numpy(),
                          scores=scores[:, :C].double().numpy(), dir_scores=dirs.numpy(),
                          topk_inds=torch.cat(inds).numpy()))
        boxes, kept_scores, labels = results[b]
        outs.append(dict(boxes=boxes.tensor.double().numpy(), scores=kept_scores.double().numpy(),
                         labels=labels.numpy()))
    return cands, outs


def keys64(cls, b, C):
    """fp64 keys of image b of one level: max over the classes of the sigmoid"""
    s = torch.from_numpy(cls[b]).double().permute(1, 2, 0).reshape(-1, C).sigmoid()
    return s.max(dim=1)[0].numpy()


def draw_level(rng, B, H, W, C, S, mean):
    A = 6
    cls = (np.round(rng.normal(mean, 1.5, (B, A * C, H, W)) * 4096) / 4096).astype(np.float32)
    for b in range(B):          # distinct scores wherever the NMS can see them: the live logits of an image (score
        flat = cls[b].reshape(-1)                        # above 0.091) each get a grid point of their own
        live = np.nonzero(flat > LIVE_LOGIT)[0]
        used = set()
        for i in live:
            q = int(round(float(flat[i]) * 4096))
            while q in used:
                q += 1
            used.add(q)
            flat[i] = q / 4096
    reg = rng.normal(0, 0.25, (B, A * S, H, W))
    reg.reshape(B, A, S, H, W)[:, :, 6] = rng.uniform(-1.5, 1.5, (B, A, H, W))
    reg = bf16_exact(reg)
    dirs = bf16_exact(rng.normal(0, 1, (B, A * 2, H, W)))
    pair = dirs.reshape(B, A, 2, H, W)
    close = np.abs(pair[:, :, 0] - pair[:, :, 1]) < 0.02           # well clear of 1e-3 after the bf16 rounding
    pair[:, :, 1][close] = bf16_exact(pair[:, :, 0][close] + 0.5)
    assert np.abs(pair[:, :, 0] - pair[:, :, 1]).min() >= DIR_LOGIT_GUARD
    return cls, reg, dirs


def band_offenders(cand):
    """candidates (rows) that take part in a pair the NMS can compare whose fp64 IoU is within the guard band"""
    live = np.nonzero((cand['scores'] > SCORE_THR).any(1))[0]
    if len(live) < 2:
        return []
    xywhr = nb.to_xywhr(cand['bboxes_for_nms'][live])
    i, j = nb.near_pairs(xywhr, xywhr, True, True)
    common = ((cand['scores'][live][i] > SCORE_THR) & (cand['scores'][live][j] > SCORE_THR)).any(1)
    i, j = i[common], j[common]
    v = nb.rbox_iou(xywhr[i], xywhr[j])
    return sorted(set(live[j[np.abs(v - NMS_THR) <= nb.GUARD_BAND]].tolist()))


def dir_offenders(out):
    v = (out['boxes'][:, 6] - DIR_OFFSET)                               # the yaw before the fix, up to a period
    q = v / np.pi + DIR_LIMIT_OFFSET
    return int((np.abs(q - np.round(q)) < DIR_GUARD).sum())


def main():
    g = load_reference()
    out = {}
    err = dict(score=0.0, decode=np.zeros(9), bev=np.zeros(5), fixed_yaw=0.0)

    def measure(c64, c32):
        for a, b in zip(c64, c32):
            for k in ('topk_inds', 'dir_scores'):
                assert np.array_equal(a[k], b[k]), k
            for k, tgt in (('scores', 'score'), ('bboxes', 'decode'), ('bboxes_for_nms', 'bev')):
                with np.errstate(invalid='ignore'):
                    d = np.abs(a[k] - b[k])
                same = (a[k] == b[k]) | (np.isnan(a[k]) & np.isnan(b[k]))
                assert np.all(np.isfinite(a[k]) | same), k                 # non-finite fp64 values: the same in fp32
                d = np.where(np.isfinite(b[k]), d, 0.0)                    # (an fp32 overflow is no rounding error)
                if tgt == 'score':
                    err['score'] = max(err['score'], float(d.max()))
                else:
                    col = d.max(0)
                    err[tgt][:len(col)] = np.maximum(err[tgt][:len(col)], col)

    def store(name, levels, C, S, nms_pre, ordered, c64, o64):
        out[f'{name}/num_levels'] = np.int32(len(levels))
        out[f'{name}/nms_pre'], out[f'{name}/num_classes'] = np.int32(nms_pre), np.int32(C)
        out[f'{name}/box_code_size'], out[f'{name}/ordered'] = np.int32(S), np.int32(ordered)
        for l, (cls, reg, dirs, anchors) in enumerate(levels):
            out[f'{name}/cls{l}'] = cls
            out[f'{name}/reg{l}_bf16'], out[f'{name}/dir{l}_bf16'] = bf16_bits(reg), bf16_bits(dirs)
            out[f'{name}/anchors{l}'] = anchors
        for k in ('bboxes', 'bboxes_for_nms', 'scores'):
            out[f'{name}/{k}'] = keep_bits(np.stack([c[k] for c in c64]))
        for k in ('dir_scores', 'topk_inds'):
            out[f'{name}/{k}'] = np.stack([c[k] for c in c64]).astype(np.int64)
        if o64 is not None:
            for b, o in enumerate(o64):
                out[f'{name}/out{b}_boxes'], out[f'{name}/out{b}_scores'] = keep_bits(o['boxes']), keep_bits(o['scores'])
                out[f'{name}/out{b}_labels'] = o['labels'].astype(np.int64)

    def case(name, shapes, B, C, S, nms_pre, ordered, seed, mean=-1.0, reuse=None, guard_pre=None):
        """draw (or reuse) the maps, run both precisions, check the guards; a violated guard -> the next seed"""
        for attempt in range(400):
            rng = np.random.RandomState(seed + 1000 * attempt)
            levels = reuse or [(*draw_level(rng, B, H, W, C, S, mean), make_anchors(g, H, W, S).numpy())
                               for H, W in shapes]
            ok = True
            for cls, _, _, _ in levels:
                for b in range(B):
                    k = np.sort(keys64(cls, b, C))[::-1]
                    for pre in guard_pre or [nms_pre]:
                        if 0 < pre < len(k):
                            ok &= k[pre - 1] - k[pre] >= GUARD
                            if ordered:
                                ok &= np.all(-np.diff(k[:pre]) >= GUARD)
            for cls, _, _, _ in levels:                                      # scores the NMS can order: SCORE_GAP apart
                for b in range(B):
                    v = torch.from_numpy(cls[b]).double().sigmoid().numpy().ravel()
                    v = np.sort(v[v > SCORE_THR - 1e-3])
                    ok &= len(v) < 2 or np.diff(v).min() >= SCORE_GAP
            if not ok:
                assert reuse is None, 'reused maps violate a key or score guard'
                continue
            for _ in range(20):                                            # move boxes out of the NMS guard band
                c64, o64 = run(g, levels, torch.float64, C, S, nms_pre)
                bad = [(b, band_offenders(c)) for b, c in enumerate(c64)]
                if not any(rows for _, rows in bad):
                    break
                assert reuse is None, 'reused maps violate the NMS guard band'
                kept = [n_l if not 0 < nms_pre < n_l else nms_pre for n_l in (l[3].shape[0] for l in levels)]
                for b, rows in bad:
                    for r in rows:
                        lvl, at_ = 0, int(r)
                        while at_ >= kept[lvl]:
                            at_ -= kept[lvl]
                            lvl += 1
                        n = int(c64[b]['topk_inds'][r])
                        reg = levels[lvl][1]
                        H, W = reg.shape[2:]
                        a, pos = n % 6, n // 6
                        reg[b, a * S:a * S + 2, pos // W, pos % W] = bf16_exact(rng.normal(0, 0.25, 2))
            else:
                continue
            if any(dir_offenders(o) for o in o64):
                assert reuse is None, 'reused maps violate the direction guard'
                continue
            c32, o32 = run(g, levels, torch.float32, C, S, nms_pre)
            measure(c64, c32)
            for a, b in zip(o64, o32):
                assert np.array_equal(a['labels'], b['labels']) and a['boxes'].shape == b['boxes'].shape
                assert np.abs(a['boxes'] - b['boxes']).max(initial=0) < 1e-4       # the same boxes, in the same order
                if len(a['boxes']):              # the returned boxes are candidates' rows but for the yaw, which has
                    err['fixed_yaw'] = max(err['fixed_yaw'],            # been through the direction fix: its own figure
                                           float(np.abs(a['boxes'][:, 6] - b['boxes'][:, 6]).max()))
                    err['score'] = max(err['score'], float(np.abs(a['scores'] - b['scores']).max()))
            store(name, levels, C, S, nms_pre, ordered, c64, o64)
            print(f'  {name}: seed {seed + 1000 * attempt}, rows {c64[0]["topk_inds"].shape[0]}, kept by the NMS '
                  f'{[len(o["labels"]) for o in o64]}')
            return levels
        raise RuntimeError(f'{name}: no draw satisfies the guards')

    # nocut first: its candidates are all 180 anchors, so the guards that hold for it hold for small's subset
    small = case('nocut', [(5, 6)], 1, 3, 7, 4096, True, 11, guard_pre=[64])
    case('nocut_neg', None, 1, 3, 7, -1, True, 0, reuse=small)
    case('small', None, 1, 3, 7, 64, True, 0, reuse=small)
    case('odd', [(7, 9)], 1, 3, 7, 100, True, 12)
    case('batch', [(20, 18)], 2, 3, 7, 512, False, 13, mean=-3.0)
    case('wide', [(40, 36)], 1, 3, 7, 4096, False, 14, mean=-3.5)
    case('s9', [(5, 6)], 1, 1, 9, 64, True, 15)
    case('levels', [(5, 6), (3, 4)], 1, 3, 7, 32, True, 16)

    # ties: the library's rule over the reference's uncut rows
    rng = np.random.RandomState(17)
    H, W, C, S, nms_pre = 7, 9, 3, 7, 100
    cls, reg, dirs = draw_level(rng, 1, H, W, C, S, -1.0)
    cls = rng.choice(np.asarray([-2.0, -0.5, 0.25, 1.5], np.float32), cls.shape, p=[0.55, 0.3, 0.1, 0.05])
    levels = [(cls, reg, dirs, make_anchors(g, H, W, S).numpy())]
    k = keys64(cls, 0, C)
    order = np.argsort(-k, kind='stable')[:nms_pre]                        # descending keys, equal keys by index
    srt = np.sort(k)[::-1]
    assert srt[nms_pre - 1] == srt[nms_pre] < srt[0], 'the cut does not fall inside a tie below the top key'
    assert len(np.unique(k)) <= 4 and np.max(np.bincount(np.unique(k, return_inverse=True)[1])) >= 100
    full64, _ = run(g, levels, torch.float64, C, S, -1)
    full32, _ = run(g, levels, torch.float32, C, S, -1)
    pick = lambda c: [{key: v[order] for key, v in c[0].items()}]  # noqa: E731
    c64, c32 = pick(full64), pick(full32)
    assert np.array_equal(c64[0]['topk_inds'], order)
    measure(c64, c32)
    store('ties', levels, C, S, nms_pre, True, c64, None)
    print('  ties: keys', np.unique(k).tolist(), 'cut key', srt[nms_pre], 'count', int((k == srt[nms_pre]).sum()))

    # special: non-finite logits, an overflowing size delta, an equal direction pair; up to the NMS call
    for attempt in range(400):
        rng = np.random.RandomState(18 + 1000 * attempt)
        H, W, C, S, nms_pre = 7, 9, 3, 7, 100
        cls, reg, dirs = draw_level(rng, 1, H, W, C, S, -1.0)
        cls[0, 4, 2, 3] = np.inf            # anchor (2 * 9 + 3) * 6 + 1, class 1
        cls[0, 9, 5, 1] = -np.inf           # anchor (5 * 9 + 1) * 6 + 3, class 0
        cls[0, 17, 6, 8] = np.nan           # anchor (6 * 9 + 8) * 6 + 5, class 2
        k = keys64(cls, 0, C)
        k[[(6 * 9 + 8) * 6 + 5, (2 * 9 + 3) * 6 + 1]] = -1
        top = int(np.argmax(k))                                          # the best ordinary row: surely kept
        a, pos = top % 6, top // 6
        reg[0, a * S + 4, pos // W, pos % W] = 100.0
        dirs[0, a * 2 + 1, pos // W, pos % W] = dirs[0, a * 2, pos // W, pos % W]
        k = keys64(cls, 0, C)
        fin = np.sort(k[np.isfinite(k)])[::-1]
        if np.all(-np.diff(fin[:nms_pre]) >= GUARD):
            break
    levels = [(cls, reg, dirs, make_anchors(g, H, W, S).numpy())]
    c64, _ = run(g, levels, torch.float64, C, S, nms_pre, skip_nms=True)
    c32, _ = run(g, levels, torch.float32, C, S, nms_pre, skip_nms=True)
    measure(c64, c32)
    for key in ('bboxes', 'bboxes_for_nms', 'scores'):                     # exp(100) overflows in fp32 only: the
        over = ~np.isfinite(c32[0][key])                                   # expected value there is the fp32 run's
        c64[0][key][over] = c32[0][key][over]
    inds = c64[0]['topk_inds']
    assert inds[0] == (6 * 9 + 8) * 6 + 5 and inds[1] == (2 * 9 + 3) * 6 + 1 and inds[2] == top       # NaN, 1.0, ...
    assert np.isnan(c64[0]['scores'][0, 2]) and c64[0]['scores'][1, 1] == 1.0
    assert np.isinf(c64[0]['bboxes'][2, 4]) and c64[0]['dir_scores'][2] == 0
    store('special', levels, C, S, nms_pre, True, c64, None)
    print('  special: first rows', inds[:4].tolist())

    print('fp32_score_error', err['score'], '\nfp32_decode_error', err['decode'], '\nfp32_bev_error', err['bev'],
          '\nfp32_fixed_yaw_error', err['fixed_yaw'])
    out.update(fp32_score_error=np.float64(err['score']), fp32_decode_error=err['decode'], fp32_bev_error=err['bev'],
               fp32_fixed_yaw_error=np.float64(err['fixed_yaw']),
               guard=np.float64(GUARD), dir_guard=np.float64(DIR_GUARD), dir_logit_guard=np.float64(DIR_LOGIT_GUARD),
               nms_guard_band=np.float64(nb.GUARD_BAND), score_gap=np.float64(SCORE_GAP), dir_offset=np.float64(DIR_OFFSET),
               dir_limit_offset=np.float64(DIR_LIMIT_OFFSET), score_thr=np.float64(SCORE_THR),
               nms_thr=np.float64(NMS_THR), max_num=np.int32(MAX_NUM))
    path = os.path.join(HERE, 'bbox_decode.npz')
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1000 * 1000


if __name__ == '__main__':
    if not os.path.isdir(mg.REF):
        sys.exit('reference not mounted; the fixture is committed, nothing to do')
    torch.set_num_threads(1)
    main()
