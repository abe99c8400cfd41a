"""Time of the 2-D ATSS head's loss, forward + backward, at config K's head: a 320 x 1280 crop, five levels at strides
4 .. 64 = 25 600 + 6 400 + 1 600 + 400 + 100 = 34 100 anchors, B = 1, C = 3, class-specific regression (12 box
channels), 12 GT boxes through ``atss_target_2d``, fp32 NCHW maps (the head sits outside the bf16 path).

    python tools/atss_loss_timing.py [--iters 200] [--warmup 30] [--out profiles/atss_loss_timing.json]

Two paths over the same inputs, from the dense targets to the loss dict and back to the 15 map gradients, timed in
alternating blocks of iterations between two events on the stream (the interval holds the host's issue time as well as
the device's work: whichever is longer), median with p10 / p90:
  hip     ``atss_loss_2d`` and the average factors formed on the device: two launches forward, one backward, no wait
          for the host
  torch   tests/atss_loss_ref.py's ``loss_terms`` and ``loss_dict`` in fp32 on the same device -- per level the
          permuted copies of the maps, the ``cat`` + ``gather``, the element-wise focal loss, ``nonzero``, indexed
          gathers, three decodes, GIoULoss's ``torch.any``, and both average factors through ``.item()`` -- with
          autograd: what a user of the package has without the fused kernels.
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

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from anchor_loss_timing import alternating, host_waits  # noqa: E402
from anchor_target_timing import device_ops  # noqa: E402
from atss_target_timing import H, MEANS, NUM_CLASSES, STDS, STRIDES, TOPK, W, anchors_k, ground_truth  # noqa: E402
from tests import atss_loss_ref as ref  # noqa: E402

C = NUM_CLASSES
LOSS_WEIGHTS = (1.0, 2.0, 1.0)                # config K: loss_cls, loss_bbox, loss_centerness


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert args.iters >= 50
    pkg = importlib.import_module('depth-from-motion_amd')
    al = importlib.import_module('depth-from-motion_amd.atss_loss')
    levels = anchors_k()
    sizes = [l.size(0) for l in levels]
    shapes = [(-(-H // s), -(-W // s)) for s in STRIDES]
    anchors = torch.cat(levels)
    gts, gt_labels = ground_truth((12,))
    labels, label_weights, bbox_targets, _, _, counts = pkg.atss_target_2d(
        anchors, sizes, gts, gt_labels, topk=TOPK, num_classes=C, target_means=MEANS, target_stds=STDS)
    positive = (labels >= 0) & (labels < C)
    num_pos = int(positive.sum())
    g = torch.Generator(device='cuda').manual_seed(0)
    A = anchors.shape[0]
    cls_rows = torch.randn(1, A, C, generator=g, device='cuda') * 1.5 - 4.0
    ctr_rows = torch.randn(1, A, 1, generator=g, device='cuda')
    reg_rows = torch.randn(1, A, 4 * C, generator=g, device='cuda')
    own = bbox_targets + torch.randn(1, A, 4, generator=g, device='cuda') * torch.tensor([0.5, 0.5, 0.8, 0.8], device='cuda')
    cols = torch.arange(4, device='cuda')[None, None] * C + labels.clamp(0, C - 1)[..., None]
    reg_rows = torch.where(positive[..., None].expand_as(reg_rows), reg_rows.scatter(2, cols, own), reg_rows)
    maps, start = ([], [], []), 0
    for (h, w), n in zip(shapes, sizes):
        for dst, rows in zip(maps, (cls_rows, reg_rows, ctr_rows)):
            dst.append(rows[:, start:start + n].reshape(1, h, w, -1).permute(0, 3, 1, 2).contiguous().requires_grad_(True))
        start += n
    flat = [m for kind in maps for m in kind]
    kw = dict(num_classes=C, reg_class_agnostic=False, target_means=MEANS, target_stds=STDS)
    weights = torch.tensor(LOSS_WEIGHTS, device='cuda')

    def total_of(losses):
        return sum(torch.stack(losses[k]).sum() for k in ('loss_cls', 'loss_bbox', 'loss_centerness'))

    def hip():
        s_cls, s_box, s_ctr, total = pkg.atss_loss_2d(*maps, anchors, labels, label_weights, bbox_targets, **kw)
        samples = counts[:, 0].clamp(min=1).sum().float().clamp(min=1.0)
        factor = total.clamp(min=1.0)
        losses = dict(loss_cls=list((s_cls * (weights[0] / samples)).unbind(0)),
                      loss_bbox=list((s_box * (weights[1] / factor)).unbind(0)),
                      loss_centerness=list((s_ctr * (weights[2] / samples)).unbind(0)))
        return losses, torch.autograd.grad(total_of(losses), flat)

    def torch_path():
        terms = ref.loss_terms(*maps, anchors, labels, label_weights, bbox_targets, dtype=torch.float32, **kw)
        losses = ref.loss_dict(terms, counts[:, 0].clamp(min=1).sum(), LOSS_WEIGHTS, host_factors=True)
        return losses, torch.autograd.grad(total_of(losses), flat, allow_unused=True)

    (o1, g1), (o2, g2) = hip(), torch_path()
    agree = dict(
        loss_relative=max(abs(float(a.detach()) - float(b.detach())) / max(abs(float(b.detach())), 1e-30)
                          for k in o1 for a, b in zip(o1[k], o2[k]) if float(b.detach()) != 0),
        grad_max_abs=max(float((a - (torch.zeros_like(a) if b is None else b)).abs().max()) for a, b in zip(g1, g2)))
    al.counters(reset=True)
    hip()
    counted = al.counters(reset=True)
    times = alternating(dict(hip=hip, torch=torch_path), args.iters, args.warmup)
    result = dict(device=torch.cuda.get_device_name(0), anchors=A, levels=sizes, positives=num_pos, batch=1, classes=C,
                  maps='fp32 NCHW, class-specific regression',
                  what='forward + backward, us between two stream events', iters=len(times['hip']),
                  warmup=args.warmup, agreement=agree)
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
