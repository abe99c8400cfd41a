"""Time of the 3-D anchor head's loss_single, forward + backward, at config K's head: a 304 x 288 BEV map, three
classes x two rotations = 525 312 anchors, B = 1, C = 3, 15 GT boxes through ``anchor_target_3d``, bf16 channels-last
maps.

    python tools/anchor_loss_timing.py [--iters 200] [--warmup 30] [--out profiles/anchor_loss_timing.json]

Two paths over the same inputs, timed in alternating blocks of iterations between two events on the stream (the
interval holds the host's issue time as well as the device's work: whichever is longer), median with p10 / p90:
  hip     ``anchor3d_loss``: two launches forward, one backward, no wait for the host
  torch   tests/anchor_loss_ref.py's ``loss_terms`` in fp32 on the same device -- permuted copies of the maps, the
          element-wise focal loss, ``nonzero``, indexed gathers, three reductions, autograd -- with the package's
          ``iou3d_loss_from_deltas`` as its IoU term: what a user of the package has without the fused kernels.
Per path also: the device kernels + memsets + copies of one forward + backward and the time inside them
(torch.profiler; null where it is not available), and the host waits of one forward + backward
(``torch.cuda.set_sync_debug_mode('warn')``, counted).  The two are compared first.  One JSON object goes to ``--out``
and, as one line, to stdout."""
import argparse
import importlib
import json
import os
import statistics
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from anchor_target_timing import DIR_OFFSET, H, THRESHOLDS, W, anchors_k, device_ops, ground_truth  # noqa: E402
from tests import anchor_loss_ref as ref  # noqa: E402

A, C, S = 6, 3, 7
LOSS_WEIGHTS = (1.0, 2.0, 0.2, 1.0)           # config K: loss_cls, loss_bbox, loss_dir, loss_iou
GRAD_OUT = (1.0, 1.0, 1.0, 1.0)


def alternating(fns, iters, warmup, block=10):
    """{name: sorted times in us}: blocks of ``block`` iterations of each path in turn"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    times = {k: [] for k in fns}
    for _ in range(iters // block):
        for name, fn in fns.items():
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(block)]
            for a, b in ev:
                a.record()
                fn()
                b.record()
            torch.cuda.synchronize()
            times[name] += [a.elapsed_time(b) * 1e3 for a, b in ev]
    return {k: sorted(v) for k, v in times.items()}


def host_waits(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('warn')
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter('always')
            fn()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    return sum('synchroniz' in str(w.message).lower() for w in seen)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert args.iters >= 50
    pkg = importlib.import_module('depth-from-motion_amd')
    al = importlib.import_module('depth-from-motion_amd.anchor_loss')
    anchors = anchors_k()
    gt, gt_labels = ground_truth(anchors)
    assigners = [dict(pos_iou_thr=p, neg_iou_thr=n, min_pos_iou=m) for p, n, m in THRESHOLDS]
    *dense, counts = pkg.anchor_target_3d(anchors, [gt], [gt_labels], assigners, num_classes=C, assign_per_class=True,
                                          dir_offset=DIR_OFFSET, dir_limit_offset=0, pos_weight=-1)
    labels, label_weights, bbox_targets, bbox_weights, dir_targets, dir_weights = dense
    num_pos = int(((labels >= 0) & (labels < C)).sum())
    flat = anchors.reshape(-1, S)
    g = torch.Generator(device='cuda').manual_seed(0)
    N = H * W * A

    def as_map(rows):                                          # (N, width) -> bf16 channels-last (1, A * width, H, W)
        m = rows.reshape(1, H, W, -1).permute(0, 3, 1, 2).to(torch.bfloat16)
        return m.contiguous(memory_format=torch.channels_last).requires_grad_(True)
    cls = as_map(torch.randn(N, C, generator=g, device='cuda') * 1.5 - 4.0)
    reg = as_map(bbox_targets.reshape(N, S) + 0.1 * torch.randn(N, S, generator=g, device='cuda'))
    dirs = as_map(torch.randn(N, 2, generator=g, device='cuda'))
    avg = float(max(num_pos, 1))
    scale = torch.tensor([w / avg for w in LOSS_WEIGHTS], dtype=torch.float32, device='cuda')
    go = [torch.tensor(v, device='cuda') for v in GRAD_OUT]
    maps = (cls, reg, dirs)

    def hip():
        out = pkg.anchor3d_loss(cls, reg, dirs, labels, label_weights, bbox_targets, bbox_weights, dir_targets,
                                dir_weights, flat, num_classes=C, scale=scale, with_iou=True)
        return out, torch.autograd.grad(out, maps, go)

    def iou_term(a, p, t):
        rows = torch.arange(a.shape[0], device=a.device)
        return pkg.iou3d_loss_from_deltas(a, p, t, rows)

    def torch_path():
        sums = ref.loss_terms(cls, reg, dirs, labels, label_weights, bbox_targets, bbox_weights, dir_targets,
                              dir_weights, flat, num_classes=C, with_iou=True, iou=iou_term, dtype=torch.float32)
        out = [s * c for s, c in zip(sums, scale.unbind(0))]
        return out, torch.autograd.grad(out, maps, go)

    (o1, g1), (o2, g2) = hip(), torch_path()
    agree = dict(out_relative=[abs(float(a) - float(b)) / max(abs(float(b)), 1e-30) for a, b in zip(o1, o2)],
                 grad_max_abs=[float((a.float() - b.float()).abs().max()) for a, b in zip(g1, g2)])
    al.counters(reset=True)
    hip()
    counted = al.counters(reset=True)
    times = alternating(dict(hip=hip, torch=torch_path), args.iters, args.warmup)
    result = dict(device=torch.cuda.get_device_name(0), anchors=N, positives=num_pos, batch=1, classes=C,
                  maps='bf16 channels-last', what='forward + backward, us between two stream events',
                  iters=len(times['hip']), warmup=args.warmup, agreement=agree)
    for name, fn in (('hip', hip), ('torch', torch_path)):
        t = times[name]
        ops = device_ops(fn)
        result[name] = dict(median_us=statistics.median(t), p10_us=t[int(0.1 * (len(t) - 1))],
                            p90_us=t[int(0.9 * (len(t) - 1))], device_ops=ops[0] if ops else None,
                            device_ops_us=ops[1] if ops else None, host_waits=host_waits(fn))
    result['hip'].update(counters=counted)
    result['speedup_median'] = result['torch']['median_us'] / result['hip']['median_us']
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(json.dumps(result, indent=1) + '\n')


if __name__ == '__main__':
    main()
