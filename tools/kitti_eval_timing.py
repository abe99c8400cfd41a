"""Time the KITTI evaluation on a seeded synthetic set of val-split size.

    python tools/kitti_eval_timing.py [--frames 3769] [--out profiles/r15_kitti_eval_timing.json]

3769 frames, about 6 ground truths and 10 detections per frame, KITTI-like boxes (detections = jittered ground truths
plus false positives).  Reports, in ms (median of --repeats runs after one warm-up, host clock around a device
synchronisation): the host concatenation of the annotations, the overlaps of all three metrics (uploads and one
launch), the matching of the three metrics (clean_data flags, first pass, host thresholds, second pass), the whole
``kitti_eval`` with 3 classes and 4 eval types; and the kernel launches, memsets and host waits of that whole
evaluation, for the full set and for a tenth of it (they must be equal).  There is no reference figure: the
reference's kernel cannot run on this hardware.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLASSES = ['Car', 'Pedestrian', 'Cyclist']
SIZES = {'Car': (3.9, 1.5, 1.6), 'Pedestrian': (0.8, 1.75, 0.6), 'Cyclist': (1.8, 1.7, 0.6), 'Van': (5.0, 2.2, 1.9)}


def synthetic_set(frames, seed=0):
    rng = np.random.default_rng(seed)
    names = np.array(['Car', 'Pedestrian', 'Cyclist', 'Van', 'DontCare'])
    gt_annos, dt_annos = [], []
    for _ in range(frames):
        n = int(rng.integers(2, 11))
        nm = rng.choice(names, n, p=[0.5, 0.2, 0.1, 0.1, 0.1])
        h = rng.uniform(15, 150, n)
        x1, y1 = rng.uniform(0, 1000, n), rng.uniform(100, 250, n)
        bbox = np.stack([x1, y1, x1 + h * rng.uniform(0.6, 2.2, n), y1 + h], 1)
        dims = np.array([SIZES.get(k, (1.0, 1.0, 1.0)) for k in nm]) * rng.uniform(0.9, 1.1, (n, 3))
        loc = np.stack([rng.uniform(-20, 20, n), rng.uniform(1.2, 2.0, n), rng.uniform(5, 60, n)], 1)
        gt = dict(name=nm, bbox=bbox, location=loc, dimensions=dims, rotation_y=rng.uniform(-3.1, 3.1, n),
                  alpha=rng.uniform(-3.1, 3.1, n), occluded=rng.integers(0, 4, n).astype(np.float64),
                  truncated=rng.choice([0.0, 0.1, 0.2, 0.4, 0.6], n))
        keep = np.nonzero((nm != 'DontCare') & (rng.random(n) < 0.85))[0]
        k, extra = len(keep), int(rng.integers(2, 8))
        d_name = np.concatenate([np.where(nm[keep] == 'Van', 'Car', nm[keep]), rng.choice(CLASSES, extra)])
        d_bbox = np.concatenate([bbox[keep] + rng.normal(0, 2.0, (k, 4)), bbox[rng.integers(0, n, extra)] +
                                 rng.normal(0, 40.0, (extra, 4))])
        d_loc = np.concatenate([loc[keep] + rng.normal(0, 0.15, (k, 3)),
                                np.stack([rng.uniform(-20, 20, extra), rng.uniform(1.2, 2.0, extra),
                                          rng.uniform(5, 60, extra)], 1)])
        d_dims = np.concatenate([dims[keep] * (1 + rng.normal(0, 0.04, (k, 3))),
                                 np.array([SIZES[c] for c in d_name[k:]]).reshape(extra, 3)])
        dt = dict(name=d_name, bbox=d_bbox, location=d_loc, dimensions=d_dims,
                  rotation_y=np.concatenate([gt['rotation_y'][keep] + rng.normal(0, 0.1, k),
                                             rng.uniform(-3.1, 3.1, extra)]),
                  alpha=np.concatenate([gt['alpha'][keep] + rng.normal(0, 0.3, k), rng.uniform(-3.1, 3.1, extra)]),
                  score=rng.uniform(0.05, 1.0, k + extra))
        gt_annos.append(gt)
        dt_annos.append(dt)
    return gt_annos, dt_annos


def timed(fn, repeats):
    fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=3769)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    importlib.import_module('depth-from-motion_amd.build').build_hip()
    ke = importlib.import_module('depth-from-motion_amd.kitti_eval')
    gt, dt = synthetic_set(args.frames)
    types_ = ['bbox', 'bev', '3d', 'aos']
    strict = np.array([[0.7, 0.5, 0.5]] * 3)
    loose = np.array([[0.7, 0.5, 0.5], [0.5, 0.25, 0.25], [0.5, 0.25, 0.25]])
    min_overlaps = np.stack([strict, loose], 0)

    base = ke._Set(gt, dt)
    concat_ms = timed(lambda: ke._Set(gt, dt), args.repeats)

    def overlaps():                                   # uploads of the boxes and tables, one launch
        base.overlaps.clear()
        base.compute_overlaps([0, 1, 2])
    overlaps()

    def matching():                                   # flags, first pass, thresholds, second pass, per metric
        base._flags.clear()
        for m in range(3):
            ke._eval_metric(base, [0, 1, 2], [0, 1, 2], m, min_overlaps, m == 0)
    result = {'frames': args.frames, 'ground_truths': base.total_gt, 'detections': base.total_dt,
              'same_frame_pairs': int(base.pair_off[-1]), 'device': torch.cuda.get_device_name(0),
              'host_concatenate_ms': round(concat_ms, 3),
              'overlaps_3_metrics_ms': round(timed(overlaps, args.repeats), 3),
              'matching_3_metrics_ms': round(timed(matching, args.repeats), 3),
              'kitti_eval_3_classes_4_types_ms': round(timed(lambda: ke.kitti_eval(gt, dt, CLASSES, types_),
                                                             args.repeats), 3)}
    for label, n in (('full', args.frames), ('tenth', max(args.frames // 10, 1))):
        ke.counters(reset=True)
        ke.kitti_eval(gt[:n], dt[:n], CLASSES, types_)
        result[f'counters_{label}'] = ke.counters()
    assert result['counters_full'] == result['counters_tenth'], 'launches or host waits grew with the frames'
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
