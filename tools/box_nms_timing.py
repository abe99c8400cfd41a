"""Device time of the BEV NMS on the dense scene of tests/golden/box_nms.npz: N = 4096 boxes in KITTI-like
clusters, 3 classes, config K's test_cfg (use_rotate_nms, nms_thr 0.25, score_thr 0.1, max_num 500).

    python tools/box_nms_timing.py [--iters 100] [--warmup 20] [--out FILE]

Rows, each the median with p10 / p90 over ``iters`` iterations between two events on the stream:
  kernels      the mask launch + the reduce launch for all classes (``box_nms._launch``), nothing else; no host
               synchronisation inside the loop
  multiclass   ``box3d_multiclass_nms`` whole: the torch filter / argsort before, the two launches, the kept-count
               copy to the host (the call's one synchronisation) and the gathers after
  per class    the reference's shape: a Python loop of boolean index + ``nms_bev`` per class (this module's own)
  aligned      ``kernels`` with the axis-aligned IoU
and the fraction of the (row, column > row) pairs of each class that pass the centre-distance test and reach
the polygon clip, recomputed here with torch in fp32 as the kernel evaluates it."""
import argparse
import importlib
import os
import statistics
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return statistics.median(t), t[int(0.1 * (iters - 1))], t[int(0.9 * (iters - 1))]


def clip_fraction(bev, order, counts):
    """pairs (i, j > i) of each class's candidates whose circumscribed circles meet / all such pairs"""
    x, y = (bev[:, 0] + bev[:, 2]) / 2, (bev[:, 1] + bev[:, 3]) / 2
    w, h = bev[:, 2] - bev[:, 0], bev[:, 3] - bev[:, 1]
    r = 0.5 * torch.sqrt(w * w + h * h)
    reach = pairs = 0
    for c, n in enumerate(counts.tolist()):
        o = order[c, :n]
        dx, dy = x[o][:, None] - x[o][None, :], y[o][:, None] - y[o][None, :]
        rr = r[o][:, None] + r[o][None, :]
        near = torch.triu(~(dx * dx + dy * dy > rr * rr), 1)
        reach += int(near.sum())
        pairs += n * (n - 1) // 2
    return reach, pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert args.iters >= 50
    pkg = importlib.import_module('depth-from-motion_amd')
    bn = importlib.import_module('depth-from-motion_amd.box_nms')
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'box_nms.npz'))
    bev = torch.from_numpy(z['dense/boxes']).cuda()
    scores = torch.from_numpy(z['dense/scores']).cuda()
    thr, score_thr = float(z['nms_thr']), float(z['dense/score_thr'])
    cfg = SimpleNamespace(use_rotate_nms=True, nms_thr=thr)
    boxes7 = torch.zeros(bev.shape[0], 7, device='cuda')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    C = scores.shape[1] - 1
    cls_scores = scores[:, :C].t()
    valid = cls_scores > score_thr
    counts = valid.sum(dim=1, dtype=torch.int32)
    order = torch.sort(cls_scores.masked_fill(~valid, float('-inf')), dim=1, descending=True, stable=True)[1].contiguous()
    say(f'{torch.cuda.get_device_name(0)}; dense scene: N = {bev.shape[0]}, {C} classes, candidates per class '
        f'{counts.tolist()}, nms_thr {thr}, score_thr {score_thr}')
    keep, kept = bn._launch(bev, order, counts, thr, True, True)
    say(f'kept per class before the max_num cut: {kept.tolist()}')
    reach, pairs = clip_fraction(bev, order, counts)
    say(f'pairs that reach the clip: {reach} of {pairs} = {100.0 * reach / pairs:.2f} %')

    def per_class():
        for c in range(C):
            sel = scores[:, c] > score_thr
            if not sel.any():
                continue
            pkg.nms_bev(bev[sel], scores[sel, c], thr)

    rows = (('kernels (mask + reduce, 3 classes)', lambda: bn._launch(bev, order, counts, thr, True, True)),
            ('box3d_multiclass_nms, whole call', lambda: pkg.box3d_multiclass_nms(boxes7, bev, scores, score_thr, 500, cfg)),
            ('per-class loop of nms_bev', per_class),
            ('kernels, axis-aligned IoU', lambda: bn._launch(bev, order, counts, thr, False, True)))
    say(f'{"":40s} {"median":>9s} {"p10":>9s} {"p90":>9s}   (us, {args.iters} iterations after {args.warmup})')
    for name, fn in rows:
        med, lo, hi = timed(fn, args.iters, args.warmup)
        say(f'{name:40s} {med:9.1f} {lo:9.1f} {hi:9.1f}')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
