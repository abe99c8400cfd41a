"""Time the depth loss's targets (depth map + box-id mask) at the KITTI config's size.

    python tools/depth_targets_timing.py [--out profiles/depth_targets_timing.json]

The ``config`` case of tests/golden/depth_targets.npz (pad 320 x 1280, 20 000 points, 12 boxes) at B = 1 and B = 8 (the
sample repeated).  Two clocks around ``generate_depth_targets``, each the median of --repeats runs after --warmup:
``event_ms`` between two events recorded on the current stream before and after the call (the device side: the table
upload, the concatenation at B = 8, the memset and the two kernels; how much of the host's work before the first launch
falls inside depends on when the runtime stamps an event recorded on an idle stream, so it is NOT a host figure), and
``host_sync_ms``, the host clock from before the call to after a device synchronisation (everything: argument checks,
the FP64 inverse, the descriptor, the pinned upload, the allocations of the two maps, the launches and their
execution).  And the module's launch counters for each batch size, which count this package's own kernels and memsets,
not torch's copies.  Beside it, on the same box, the CPU computation of the same maps for ONE sample: the
reference's own ``GenerateDepthMap`` (the functions tests/golden/make_golden_depth_targets.py lifts from the reference
checkout) when that checkout is there, otherwise this package's numpy path -- the result says which.
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
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))


def device_ms(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        out.append(start.elapsed_time(stop))
    return statistics.median(out)


def host_sync_ms(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def host_ms(fn, repeats):
    fn()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def cpu_baseline(c, dt):
    """(label, callable) of the CPU computation of one sample's two maps"""
    try:
        gen = importlib.import_module('make_golden_depth_targets')
        g = gen.load_reference()
        sample = (c['points'], c['boxes'], c['P'], c['cam2img'], c['img_shape'], c['pad_shape'])
        return "the reference's GenerateDepthMap (numpy stand-in for mmcv's points_in_boxes_cpu)", \
            lambda: gen.reference_maps(g, *sample)
    except (OSError, ImportError):
        return "this package's numpy path (no reference checkout on this box)", \
            lambda: dt.generate_depth_targets([c['points']], [c['boxes']], [c['P']], [c['cam2img']], [c['img_shape']],
                                              c['pad_shape'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--cpu-repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    importlib.import_module('depth-from-motion_amd.build').build_hip()
    dt = importlib.import_module('depth-from-motion_amd.depth_targets')
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'depth_targets.npz'))
    c = {k: z[f'config/{k}'] for k in ('points', 'boxes', 'P', 'cam2img')}
    c['img_shape'], c['pad_shape'] = tuple(z['config/img_shape']), tuple(z['config/pad_shape'])
    result = {'device': torch.cuda.get_device_name(0), 'pad_shape': [int(v) for v in c['pad_shape'][:2]],
              'points_per_sample': int(c['points'].shape[0]), 'boxes_per_sample': int(c['boxes'].shape[0]),
              'repeats': args.repeats, 'warmup': args.warmup}
    points, boxes = torch.from_numpy(c['points']).cuda(), torch.from_numpy(c['boxes']).cuda()
    for B in (1, 8):
        def run(B=B):
            return dt.generate_depth_targets([points] * B, [boxes] * B, [c['P']] * B, [c['cam2img']] * B,
                                             [c['img_shape']] * B, c['pad_shape'])
        result[f'event_ms_B{B}'] = round(device_ms(run, args.warmup, args.repeats), 4)
        result[f'host_sync_ms_B{B}'] = round(host_sync_ms(run, args.warmup, args.repeats), 4)
        torch.cuda.synchronize()
        dt.counters(reset=True)
        run()
        result[f'counters_B{B}'] = dt.counters(reset=True)
    assert result['counters_B1'] == result['counters_B8'], 'launches grew with the batch'
    label, fn = cpu_baseline(c, dt)
    result['cpu_baseline'] = label
    result['cpu_ms_one_sample'] = round(host_ms(fn, args.cpu_repeats), 3)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
