"""Generate tests/golden/kitti_eval.npz: the KITTI evaluation (overlaps, clean_data flags, thresholds, tp / fp / fn /
similarity, the AP curves, mAP arrays, ret_dict and the result text).

Run in the build container only (needs the reference checkout):   python tests/golden/make_golden_kitti_eval.py

The reference's ``core/evaluation/kitti_utils/eval.py`` and ``rotate_iou.py`` run UNMODIFIED under stand-in ``numba``
/ ``numba.cuda`` modules, loaded as a throw-away package so that ``from .rotate_iou import ...`` resolves:
``jit`` / ``njit`` are identity decorators, ``prange = range``, ``cuda.local.array = np.zeros``; ``numba.float32`` is
np.float64 for the expected values and np.float32 to measure what fp32 costs.  ``rotate_iou_gpu_eval`` (the launch of
the device kernel) is replaced by a loop that calls the file's own ``devRotateIoUEval(qbox, box, criterion)`` per
pair, in the kernel's argument order, on inputs rounded to fp32 as the reference rounds them.  Nothing of the reference
is stored, only inputs and the results it produced.

``fp32_iou_error`` = the largest |fp64 - fp32| of the reference's own algorithm over every stored pair, bev and 3d;
``GUARD_BAND`` = 4 x that.  Conditions asserted here (boxes are moved and everything re-checked until they hold, no
comparison is dropped): no stored overlap, DontCare overlap included, within GUARD_BAND of a min-overlap of its
metric (0.7 / 0.5 for bbox, 0.7 / 0.5 / 0.25 for bev and 3d); scores distinct within a frame; for one ground truth, no
two detections above the smallest min-overlap with overlaps closer than GUARD_BAND; in ``val24`` every class has a
true positive, a false positive and a false negative at the strict overlap in every metric; no printed value within
1e-6 of a rounding boundary of its print format; no pair of coincident boxes.

Scenes: ``val24`` (24 frames, 2-9 ground truths of Car / Pedestrian / Cyclist / Van / Person_sitting / DontCare with
mixed occlusion and truncation, 2-D heights on both sides of 25 and 40 px; detections = jittered ground truths plus
false positives, some inside DontCare boxes), evaluated as ``all`` (bbox, bev, 3d, aos; three classes), ``car``
(current_classes=['Car']: no Overall keys) and ``noaos`` (all alphas -10);  ``edge`` (a non-empty frame, an empty
frame, ground truth only, detections only, 1 ground truth with 70 jittered detections, 9 ground truths with 130
detections);  ``single`` (one frame, one ground truth, one detection);  ``crit`` (40 x 30 rotated boxes through
rotate_iou_gpu_eval with criterion -1, 0, 1, 2).
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = '/root/reference/mmdet3d/core/evaluation/kitti_utils'
OUT = os.path.join(HERE, 'kitti_eval.npz')
CLASSES = ['Car', 'Pedestrian', 'Cyclist']
MIN_OVERLAPS = {0: (0.7, 0.5), 1: (0.7, 0.5, 0.25), 2: (0.7, 0.5, 0.25)}

_PAIR_CACHE = {}


def _identity_jit(*args, **kwargs):
    if len(args) == 1 and callable(args[0]) and not kwargs:
        return args[0]
    return lambda f: f


def load_reference(float_dtype, tag):
    """the two reference files as the package ``_ref_kitti_<tag>``, with numba.float32 = float_dtype"""
    numba = types.ModuleType('numba')
    numba.jit = numba.njit = _identity_jit
    numba.prange = range
    numba.float32 = float_dtype
    cuda = types.ModuleType('numba.cuda')
    cuda.jit = _identity_jit
    cuda.local = types.SimpleNamespace(array=lambda shape, dtype: np.zeros(shape, dtype=dtype))
    cuda.shared = types.SimpleNamespace(array=lambda shape, dtype: np.zeros(shape, dtype=dtype))
    numba.cuda = cuda
    sys.modules['numba'], sys.modules['numba.cuda'] = numba, cuda
    pkg_name = f'_ref_kitti_{tag}'
    pkg = types.ModuleType(pkg_name)
    pkg.__path__ = [REF_DIR]
    sys.modules[pkg_name] = pkg
    mods = {}
    for name in ('rotate_iou', 'eval'):
        spec = importlib.util.spec_from_file_location(f'{pkg_name}.{name}', os.path.join(REF_DIR, name + '.py'))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
        setattr(pkg, name, mod)
        mods[name] = mod
    rot = mods['rotate_iou']
    dev = rot.devRotateIoUEval

    def rotate_iou_gpu_eval(boxes, query_boxes, criterion=-1, device_id=0):
        boxes = boxes.astype(np.float32)
        query_boxes = query_boxes.astype(np.float32)
        n, k = boxes.shape[0], query_boxes.shape[0]
        iou = np.zeros((n, k), dtype=float_dtype)
        b, q = boxes.astype(float_dtype), query_boxes.astype(float_dtype)
        for i in range(n):
            for j in range(k):
                key = (tag, criterion, boxes[i].tobytes(), query_boxes[j].tobytes())
                if key not in _PAIR_CACHE:
                    with np.errstate(all='ignore'):
                        _PAIR_CACHE[key] = dev(q[j], b[i], criterion)
                iou[i, j] = _PAIR_CACHE[key]
        return iou
    rot.rotate_iou_gpu_eval = rotate_iou_gpu_eval
    return mods['eval'], rot


# ---------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------
SIZES = {'Car': (3.9, 1.5, 1.6), 'Van': (5.0, 2.2, 1.9), 'Pedestrian': (0.8, 1.75, 0.6),
         'Person_sitting': (0.8, 1.3, 0.6), 'Cyclist': (1.8, 1.7, 0.6)}
HEIGHTS = np.array([18, 22, 24, 26, 28, 33, 38, 39, 41, 43, 55, 80, 120], dtype=np.float64)


def empty_anno(with_score):
    a = dict(name=np.zeros(0, dtype='<U16'), bbox=np.zeros((0, 4)), location=np.zeros((0, 3)),
             dimensions=np.zeros((0, 3)), rotation_y=np.zeros(0), alpha=np.zeros(0), occluded=np.zeros(0),
             truncated=np.zeros(0))
    if with_score:
        a['score'] = np.zeros(0)
    return a


def stack_anno(rows, with_score):
    if not rows:
        return empty_anno(with_score)
    a = dict(name=np.array([r['name'] for r in rows]), bbox=np.array([r['bbox'] for r in rows], dtype=np.float64),
             location=np.array([r['location'] for r in rows], dtype=np.float64),
             dimensions=np.array([r['dimensions'] for r in rows], dtype=np.float64),
             rotation_y=np.array([r['rotation_y'] for r in rows], dtype=np.float64),
             alpha=np.array([r['alpha'] for r in rows], dtype=np.float64),
             occluded=np.array([r.get('occluded', 0) for r in rows], dtype=np.float64),
             truncated=np.array([r.get('truncated', 0) for r in rows], dtype=np.float64))
    if with_score:
        a['score'] = np.array([r['score'] for r in rows], dtype=np.float64)
    return a


def random_gt(rng, name):
    h2d = float(rng.choice(HEIGHTS)) + float(rng.uniform(0.1, 0.9))
    x1, y1 = float(rng.uniform(0, 1000)), float(rng.uniform(100, 250))
    w2d = h2d * float(rng.uniform(0.6, 2.2))
    row = dict(name=name, bbox=[x1, y1, x1 + w2d, y1 + h2d], occluded=int(rng.choice([0, 0, 0, 1, 1, 2, 3])),
               truncated=float(rng.choice([0.0, 0.0, 0.05, 0.2, 0.4, 0.6])), alpha=float(rng.uniform(-3.1, 3.1)))
    if name == 'DontCare':
        row['bbox'] = [x1, y1, x1 + float(rng.uniform(60, 200)), y1 + float(rng.uniform(30, 90))]
        row.update(location=[-1000.0, -1000.0, -1000.0], dimensions=[-1.0, -1.0, -1.0], rotation_y=-10.0,
                   alpha=-10.0, occluded=-1, truncated=-1.0)
        return row
    size = np.array(SIZES[name]) * rng.uniform(0.9, 1.1, 3)
    row.update(location=[float(rng.uniform(-20, 20)), float(rng.uniform(1.2, 2.0)), float(rng.uniform(5, 40))],
               dimensions=size.tolist(), rotation_y=float(rng.uniform(-3.1, 3.1)))
    return row


def jitter(rng, gt, scale):
    """a detection near ``gt``: ``scale`` 1 is a tight match, 3 a loose one"""
    row = dict(name=gt['name'] if gt['name'] in CLASSES else {'Van': 'Car', 'Person_sitting': 'Pedestrian'}[gt['name']])
    row['bbox'] = (np.array(gt['bbox']) + rng.normal(0, 1.2 * scale, 4)).tolist()
    row['location'] = (np.array(gt['location']) + rng.normal(0, 0.05 * scale, 3)).tolist()
    row['dimensions'] = (np.array(gt['dimensions']) * (1 + rng.normal(0, 0.02 * scale, 3))).tolist()
    row['rotation_y'] = gt['rotation_y'] + float(rng.normal(0, 0.03 * scale))
    row['alpha'] = gt['alpha'] + float(rng.normal(0, 0.15 * scale))
    row['score'] = float(rng.uniform(0.05, 1.0))
    return row


def false_positive(rng, inside=None):
    name = str(rng.choice(CLASSES))
    row = random_gt(rng, name)
    if inside is not None:                      # a 2-D box inside a DontCare box
        x1, y1, x2, y2 = inside
        w, h = (x2 - x1), (y2 - y1)
        row['bbox'] = [x1 + 0.1 * w, y1 + 0.05 * h, x2 - 0.1 * w, y2 - 0.05 * h]
    row['score'] = float(rng.uniform(0.05, 1.0))
    for k in ('occluded', 'truncated'):
        row.pop(k)
    return row


def val_frame(rng):
    n = int(rng.integers(2, 10))
    names = rng.choice(['Car', 'Pedestrian', 'Cyclist', 'Van', 'Person_sitting', 'DontCare'], n,
                       p=[0.32, 0.2, 0.2, 0.08, 0.08, 0.12])
    gts = [random_gt(rng, str(nm)) for nm in names]
    dts = []
    for g in gts:
        if g['name'] == 'DontCare':
            if rng.random() < 0.7:
                dts.append(false_positive(rng, inside=g['bbox']))
            continue
        if rng.random() < 0.8:
            dts.append(jitter(rng, g, float(rng.choice([0.5, 1.0, 2.0, 4.0]))))
    for _ in range(int(rng.integers(1, 4))):
        dts.append(false_positive(rng))
    order = rng.permutation(len(dts))
    return gts, [dts[i] for i in order]


def build_scenes(rng):
    scenes = {'val24': [val_frame(rng) for _ in range(24)]}
    first = val_frame(rng)
    while first[0][0]['name'] == 'DontCare':
        first = val_frame(rng)
    gt_only, dt_only = val_frame(rng), val_frame(rng)
    one = random_gt(rng, 'Car')
    one.update(occluded=0, truncated=0.0)
    one['bbox'][3] = one['bbox'][1] + 60.0
    crowd = [jitter(rng, one, float(rng.uniform(0.3, 5.0))) for _ in range(70)]
    nine = [random_gt(rng, str(nm)) for nm in ['Car', 'Car', 'Pedestrian', 'Cyclist', 'Van', 'Car', 'Pedestrian',
                                               'Cyclist', 'DontCare']]
    many = []
    for i in range(130):
        g = nine[i % 9]
        many.append(false_positive(rng, inside=g['bbox']) if g['name'] == 'DontCare'
                    else jitter(rng, g, float(rng.uniform(0.3, 6.0))))
    scenes['edge'] = [first, ([], []), (gt_only[0], []), ([], dt_only[1]), ([one], crowd), (nine, many)]
    g = random_gt(rng, 'Car')
    g.update(occluded=0, truncated=0.0)
    g['bbox'][3] = g['bbox'][1] + 60.0
    d = jitter(rng, g, 0.5)
    scenes['single'] = [([g], [d])]
    return scenes


def annos_of(frames, alpha=None):
    gt = [stack_anno(g, False) for g, _ in frames]
    dt = [stack_anno(d, True) for _, d in frames]
    if alpha is not None:
        for a in gt + dt:
            a['alpha'] = np.full_like(a['alpha'], alpha)
    return gt, dt


# ---------------------------------------------------------------------------------------------------------
# overlaps and guards
# ---------------------------------------------------------------------------------------------------------
def overlaps_of(ev, gt, dt):
    """[metric][frame] -> (n_dt, n_gt) blocks, as eval_class asks for them"""
    out = []
    for metric in range(3):
        blocks, _, _, _ = ev.calculate_iou_partly(dt, gt, metric, max(len(gt), 1))
        out.append([np.asarray(b, dtype=np.float64) for b in blocks])
    return out


def dontcare_overlaps(ev, gt, dt):
    out = []
    for g, d in zip(gt, dt):
        dc = g['bbox'][g['name'] == 'DontCare'].reshape(-1, 4)
        out.append(ev.image_box_overlap(d['bbox'].reshape(-1, 4), dc, 0))
    return out


def offenders(ov64, dc, dt, guard):
    """{(frame, detection)} that break a per-frame condition"""
    bad = set()
    for metric in range(3):
        for f, block in enumerate(ov64[metric]):
            for t in MIN_OVERLAPS[metric]:
                for j, _ in zip(*np.nonzero(np.abs(block - t) <= guard)):
                    bad.add((f, int(j)))
            low = min(MIN_OVERLAPS[metric])
            for i in range(block.shape[1]):
                col = block[:, i]
                idx = np.nonzero(col > low - guard)[0]
                srt = idx[np.argsort(col[idx])]
                for a, b in zip(srt[:-1], srt[1:]):
                    if col[b] - col[a] <= guard:
                        bad.add((f, int(b)))
            if metric and np.any(block >= 1 - 1e-9):
                for j, _ in zip(*np.nonzero(block >= 1 - 1e-9)):
                    bad.add((f, int(j)))                       # coincident boxes
    for f, block in enumerate(dc):
        for t in MIN_OVERLAPS[0]:
            for j, _ in zip(*np.nonzero(np.abs(block - t) <= guard)):
                bad.add((f, int(j)))
    for f, d in enumerate(dt):
        s = d['score']
        for j in range(len(s)):
            if np.sum(s == s[j]) > 1:
                bad.add((f, j))
    return bad


def max_error(ov64, ov32):
    err = 0.0
    for metric in (1, 2):
        for a, b in zip(ov64[metric], ov32[metric]):
            if a.size:
                err = max(err, float(np.max(np.abs(a - b))))
    return err


# ---------------------------------------------------------------------------------------------------------
# the recorded evaluation
# ---------------------------------------------------------------------------------------------------------
def record_eval(ev, gt, dt, classes, eval_types, store, prefix):
    calls = []
    inner = ev.fused_compute_statistics

    def spy(overlaps, pr, *args, **kwargs):
        if not calls or calls[-1][0] is not pr:
            calls.append((pr, np.array(kwargs['thresholds'], dtype=np.float64)))
        return inner(overlaps, pr, *args, **kwargs)
    curves = []
    inner_class = ev.eval_class

    def spy_class(*args, **kwargs):
        ret = inner_class(*args, **kwargs)
        curves.append((args[4], {k: v.copy() for k, v in ret.items()}))
        return ret
    firsts = []
    inner_thr = ev.get_thresholds

    def spy_thr(scores, num_gt, *args, **kwargs):
        firsts.append((np.array(scores, dtype=np.float64), int(num_gt)))
        return inner_thr(scores, num_gt, *args, **kwargs)
    maps = []
    inner_do = ev.do_eval

    def spy_do(*args, **kwargs):
        out = inner_do(*args, **kwargs)
        maps.append([None if a is None else np.array(a, dtype=np.float64) for a in out])
        return out
    ev.fused_compute_statistics, ev.eval_class, ev.get_thresholds, ev.do_eval = spy, spy_class, spy_thr, spy_do
    try:
        types_in = list(eval_types)
        with np.errstate(all='ignore'):
            text, ret = ev.kitti_eval(gt, dt, list(classes), types_in)
    finally:
        ev.fused_compute_statistics, ev.eval_class, ev.get_thresholds = inner, inner_class, inner_thr
        ev.do_eval = inner_do
    assert len(maps) == 1
    for label, a in zip(('mAP11_bbox', 'mAP11_bev', 'mAP11_3d', 'mAP11_aos', 'mAP40_bbox', 'mAP40_bev', 'mAP40_3d',
                         'mAP40_aos'), maps[0]):
        if a is not None:
            store[f'{prefix}/{label}'] = a                     # [class, difficulty, min_overlap], before the means
    C, L, K = len(classes), 3, 2
    assert len(calls) == len(firsts) == len(curves) * C * L * K
    for n, (metric, ret_curves) in enumerate(curves):
        thr = np.zeros((C, L, K, 41))
        nthr = np.zeros((C, L, K), dtype=np.int32)
        pr = np.zeros((C, L, K, 41, 4))
        for c in range(C * L * K):
            arr, t = calls[n * C * L * K + c]
            m, l, k = c // (L * K), (c // K) % L, c % K
            nthr[m, l, k] = len(t)
            thr[m, l, k, :len(t)] = t
            pr[m, l, k, :len(t)] = arr
        store[f'{prefix}/m{metric}/thresholds'], store[f'{prefix}/m{metric}/num_thresholds'] = thr, nthr
        store[f'{prefix}/m{metric}/pr'] = pr
        mine = firsts[n * C * L * K:(n + 1) * C * L * K]         # the first pass: what get_thresholds was given
        store[f'{prefix}/m{metric}/first_scores'] = np.concatenate([f[0] for f in mine])
        store[f'{prefix}/m{metric}/first_counts'] = np.array([len(f[0]) for f in mine], dtype=np.int64)
        store[f'{prefix}/m{metric}/first_num_gt'] = np.array([f[1] for f in mine], dtype=np.int64)
        for key, v in ret_curves.items():
            store[f'{prefix}/m{metric}/{key}'] = v
    store[f'{prefix}/eval_types_after'] = np.array(types_in)
    store[f'{prefix}/ret_keys'] = np.array(list(ret.keys()))
    store[f'{prefix}/ret_values'] = np.array([float(v) for v in ret.values()], dtype=np.float64)
    store[f'{prefix}/result'] = np.array(text)
    store[f'{prefix}/classes'] = np.array(list(classes))
    store[f'{prefix}/eval_types'] = np.array(list(eval_types))
    return text, ret, curves


def check_printed(ret, curves, ev):
    """no printed value within 1e-6 of a rounding boundary: .4f for the APs, .2f for the AOS"""
    for v in ret.values():
        frac = (float(v) * 1e4) % 1.0
        assert abs(frac - 0.5) * 1e-4 > 1e-6, v
    for metric, c in curves:
        if metric == 0:
            for fn in (ev.get_mAP11, ev.get_mAP40):
                a = fn(c['orientation'])
                for v in list(a.ravel()) + list(a.mean(axis=0).ravel()):
                    frac = (float(v) * 1e2) % 1.0
                    assert abs(frac - 0.5) * 1e-2 > 1e-6, v


def main():
    ev64, rot64 = load_reference(np.float64, 'f64')
    ev32, _ = load_reference(np.float32, 'f32')
    rng = np.random.default_rng(20261019)
    scenes = build_scenes(rng)
    guard = 0.0
    for attempt in range(200):
        err, bad_total = 0.0, 0
        computed = {}
        for name, frames in scenes.items():
            gt, dt = annos_of(frames)
            ov64, ov32 = overlaps_of(ev64, gt, dt), overlaps_of(ev32, gt, dt)
            computed[name] = (gt, dt, ov64, dontcare_overlaps(ev64, gt, dt))
            err = max(err, max_error(ov64, ov32))
        guard = 4 * err
        for name, frames in scenes.items():
            gt, dt, ov64, dc = computed[name]
            for f, j in sorted(offenders(ov64, dc, dt, guard)):
                bad_total += 1
                old = frames[f][1][j]
                new = dict(old)
                new['bbox'] = (np.array(old['bbox']) + rng.normal(0, 0.7, 4)).tolist()
                new['location'] = (np.array(old['location']) + rng.normal(0, 0.03, 3)).tolist()
                new['score'] = float(rng.uniform(0.05, 1.0))
                frames[f][1][j] = new
        print(f'attempt {attempt}: fp32_iou_error {err:.3e}, moved {bad_total}')
        if bad_total == 0:
            break
    else:
        raise AssertionError('the guards did not settle')

    store = {'fp32_iou_error': np.float64(err), 'GUARD_BAND': np.float64(guard)}
    assert 0 < err < 1e-3
    for name, frames in scenes.items():
        gt, dt, ov64, dc = computed[name]
        for side, annos in (('gt', gt), ('dt', dt)):
            store[f'{name}/{side}_num'] = np.array([len(a['name']) for a in annos], dtype=np.int64)
            for key in annos[0]:
                store[f'{name}/{side}_{key}'] = np.concatenate([a[key] for a in annos], 0)
        for metric in range(3):
            store[f'{name}/overlaps{metric}'] = np.concatenate([b.reshape(-1) for b in ov64[metric]] or [np.zeros(0)])
        store[f'{name}/dc_overlaps'] = np.concatenate([b.reshape(-1) for b in dc])
        ig = np.zeros((3, 3, int(store[f'{name}/gt_num'].sum())), dtype=np.int8)
        idt = np.zeros((3, 3, int(store[f'{name}/dt_num'].sum())), dtype=np.int8)
        valid = np.zeros((3, 3), dtype=np.int64)
        for m in range(3):
            for l in range(3):
                rets = [ev64.clean_data(g, d, m, l) for g, d in zip(gt, dt)]
                ig[m, l] = np.concatenate([np.array(r[1], dtype=np.int8) for r in rets])
                idt[m, l] = np.concatenate([np.array(r[2], dtype=np.int8) for r in rets])
                valid[m, l] = sum(r[0] for r in rets)
        store[f'{name}/ignored_gt'], store[f'{name}/ignored_dt'], store[f'{name}/num_valid_gt'] = ig, idt, valid
        variants = [('all', CLASSES, ['bbox', 'bev', '3d', 'aos'], None)]
        if name == 'val24':
            variants += [('car', ['Car'], ['bbox', 'bev', '3d', 'aos'], None),
                         ('noaos', CLASSES, ['bbox', 'bev', '3d'], -10.0)]
        for tag, classes, types_, alpha in variants:
            g2, d2 = annos_of(frames, alpha)
            text, ret, curves = record_eval(ev64, g2, d2, classes, types_, store, f'{name}/{tag}')
            check_printed(ret, curves, ev64)
            if name == 'val24' and tag == 'all':
                print(text)
                for metric, _ in curves:
                    pr = store[f'{name}/{tag}/m{metric}/pr']
                    nthr = store[f'{name}/{tag}/m{metric}/num_thresholds']
                    for m in range(3):
                        last = pr[m, 2, 0, nthr[m, 2, 0] - 1]
                        assert nthr[m, 2, 0] > 0 and last[0] >= 1 and last[1] >= 1 and last[2] >= 1, (metric, m, last)
    # crit: one 40 x 30 box set through rotate_iou_gpu_eval, every criterion
    boxes = np.stack([rng.uniform(-10, 10, 40), rng.uniform(5, 30, 40), rng.uniform(1, 5, 40), rng.uniform(1, 3, 40),
                      rng.uniform(-3.1, 3.1, 40)], 1)
    query = np.stack([rng.uniform(-10, 10, 30), rng.uniform(5, 30, 30), rng.uniform(1, 5, 30), rng.uniform(1, 3, 30),
                      rng.uniform(-3.1, 3.1, 30)], 1)
    query[:10] = boxes[:10] + rng.normal(0, 0.1, (10, 5))
    store['crit/boxes'], store['crit/query_boxes'] = boxes, query
    crit_err = 0.0
    for crit in (-1, 0, 1, 2):
        with np.errstate(all='ignore'):
            a = rot64.rotate_iou_gpu_eval(boxes, query, crit)
            b = sys.modules['_ref_kitti_f32.rotate_iou'].rotate_iou_gpu_eval(boxes, query, crit)
        store[f'crit/iou_{crit}'] = a
        crit_err = max(crit_err, float(np.max(np.abs(a - b))))
        assert (a > 0).sum() >= 10
    store['crit/fp32_error'] = np.float64(crit_err)
    np.savez_compressed(OUT, **store)
    size = os.path.getsize(OUT)
    print(f'{OUT}: {size} bytes, fp32_iou_error {err:.3e}, GUARD_BAND {guard:.3e}, crit fp32 error {crit_err:.3e}')
    assert size < 1024 * 1024


if __name__ == '__main__':
    main()
