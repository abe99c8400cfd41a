"""Device time of the differentiable IoU loss at P = 512 and P = 16384 positives, forward and forward + backward.

    python tools/iou3d_loss_timing.py [--iters 100] [--warmup 20] [--out FILE]

Rows, each the median with p10 / p90 over ``iters`` iterations between two events on the stream:
  fused     ``iou3d_loss_from_deltas`` (gather, decode, NaN rule, IoU, Jacobian: one launch) and the reduction
            ``sum() / avg_factor`` with a device-tensor avg_factor, as ``loss_single`` forms the term
  unfused   this package's ``IOU3DLoss`` on boxes decoded with torch ops (the reference's call sequence)
  torch     the fixture generator's torch restatement of the IoU (tests/golden/make_golden_iou3d.py, fp32, on the
            GPU) under the same decode and reduction: the only composition baseline there is -- mmcv is not
            installed
The scene: R = 4 P anchors of config K's three classes, targets near the anchors, predictions = targets + noise."""
import argparse
import importlib
import importlib.util
import os
import statistics
import sys

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


def decode(anchors, deltas):
    """DeltaXYZWLHRBBoxCoder.decode's arithmetic (delta_xyzwhlr_bbox_coder.py:58-91) with torch ops"""
    xa, ya, za, wa, la, ha, ra = torch.split(anchors, 1, dim=-1)
    xt, yt, zt, wt, lt, ht, rt = torch.split(deltas, 1, dim=-1)
    za = za + ha / 2
    diagonal = torch.sqrt(la ** 2 + wa ** 2)
    hg = torch.exp(ht) * ha
    return torch.cat([xt * diagonal + xa, yt * diagonal + ya, zt * ha + za - hg / 2, torch.exp(wt) * wa,
                      torch.exp(lt) * la, hg, rt + ra], dim=-1)


def scene(P, seed):
    rng = np.random.RandomState(seed)
    R = 4 * P
    sizes = np.array([[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]])
    kind = rng.randint(0, 3, R)
    anchors = np.concatenate([rng.uniform(2, 59.6, (R, 1)), rng.uniform(-30.4, 30.4, (R, 1)),
                              np.where(kind == 0, -1.78, -0.6)[:, None], sizes[kind],
                              rng.choice([0.0, 1.57], R)[:, None]], 1)
    scale = np.array([0.1, 0.1, 0.1, 0.08, 0.08, 0.08, 0.2])
    targets = rng.normal(0, 1, (R, 7)) * scale
    pred = targets + rng.normal(0, 1, (R, 7)) * scale
    pos = np.sort(rng.permutation(R)[:P])
    f = lambda x: torch.from_numpy(x.astype(np.float32)).cuda()  # noqa: E731
    return f(anchors), f(pred), f(targets), torch.from_numpy(pos).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert args.iters >= 50
    pkg = importlib.import_module('depth-from-motion_amd')
    spec = importlib.util.spec_from_file_location('make_golden_iou3d',
                                                  os.path.join(ROOT, 'tests', 'golden', 'make_golden_iou3d.py'))
    gen = importlib.util.module_from_spec(spec)
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    spec.loader.exec_module(gen)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f'{torch.cuda.get_device_name(0)}; us, median / p10 / p90 of {args.iters} iterations after {args.warmup}')
    loss_mod = pkg.IOU3DLoss()
    for P in (512, 16384):
        anchors, pred, targets, pos = scene(P, P)
        avg = torch.tensor(float(P), device='cuda')
        leaf = pred.clone().requires_grad_(True)

        def fused(p):
            return pkg.iou3d_loss_from_deltas(anchors, p, targets, pos).sum() / avg

        def unfused(p):
            return loss_mod(decode(anchors[pos], p[pos]), decode(anchors[pos], targets[pos]), avg_factor=avg)

        def composed(p):
            a, b = decode(anchors[pos], p[pos]), decode(anchors[pos], targets[pos])
            b = torch.where(torch.isnan(b), a, b)
            return (1 - gen.iou3d_pairs(a, b)).sum() / avg

        with torch.no_grad():
            want = composed(pred)
            say(f'P = {P}: loss fused {float(fused(pred)):.6f}, unfused {float(unfused(pred)):.6f}, '
                f'torch restatement {float(want):.6f}')
        for name, fn in (('fused (iou3d_loss_from_deltas)', fused), ('unfused (decode + IOU3DLoss)', unfused),
                         ('torch restatement of the IoU', composed)):
            def fwd():
                with torch.no_grad():
                    fn(pred)

            def both():
                leaf.grad = None
                fn(leaf).backward()
            f_med, f_lo, f_hi = timed(fwd, args.iters, args.warmup)
            b_med, b_lo, b_hi = timed(both, args.iters, args.warmup)
            say(f'P = {P:6d} {name:34s} forward {f_med:9.1f} {f_lo:9.1f} {f_hi:9.1f}   forward + backward '
                f'{b_med:9.1f} {b_lo:9.1f} {b_hi:9.1f}')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
