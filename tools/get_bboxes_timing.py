"""Time of the anchor head's maps -> NMS candidates step at config K's real size: a 304 x 288 BEV map, three sizes x
two rotations = 525 312 anchors, C = 3, B = 1, nms_pre 4096.

    python tools/get_bboxes_timing.py [--iters 100] [--warmup 20] [--out FILE]

Rows, each the median with p10 / p90 over ``iters`` iterations between two events on the stream (the interval holds
the host's issue time as well as the device's work: whichever is longer), then the number of device kernels, memsets
and copies one call issues and the sum of their durations (torch.profiler; 'n/a' where it is not available):
  fused                  ``anchor_head_candidates``: a memset and six launches
  torch                  the same step written with torch ops on the same GPU, for one image (what
                         anchor3d_head.py:491-533 computes: rows from the maps, sigmoid, best class, topk, four
                         gathers, the box decode, the BEV corners, a zero background column), with the anchors
                         rebuilt on the device in every call, as get_bboxes regenerates them.  It is this tool's own
                         composition -- vectorised column operations, anchors by broadcasting -- not the reference's
                         program: mmdet is not installed, and the reference's generator also reads its linspace
                         bounds back from the device, which this one does not, so the row flatters the baseline
  torch, cached anchors  the same chain with the anchors generated once
The two paths are compared first: the number of indices and direction bins that differ and the largest score and box
differences are printed (the composition rounds in another order -- hypot, 0.5 * x -- so small differences are
expected in the boxes).  The per-kernel times of the fused call are listed last (which launch dominates)."""
import argparse
import importlib
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]]
X_RANGE, Y_RANGE, Z = (2.0, 59.6), (-30.4, 30.4), [-1.78, -0.6, -0.6]
ROTATIONS = [0, 1.57]
H, W, C, S, NMS_PRE = 304, 288, 3, 7, 4096


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


def device_ops(fn):
    """[(name, duration in us)] of the device kernels, memsets and copies of one call, or None"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        ops = [e for e in prof.events() if getattr(e, 'device_type', None) is not None and
               'cuda' in str(e.device_type).lower()]
        return [(e.name, e.device_time_total if hasattr(e, 'device_time_total') else e.cuda_time_total)
                for e in ops] or None
    except Exception as exc:  # noqa: BLE001  (a profiler that is not there only costs the two columns)
        print(f'(torch.profiler unavailable: {type(exc).__name__}: {exc})')
        return None


def grid_anchors(device):
    """config K's anchors for one level, (H * W * 6, 7) in the order (row, column, size, rotation): centres on the
    generator's linspace grids, filled by broadcasting.  Built on the device from host constants, every call"""
    out = torch.empty(H, W, len(SIZES), len(ROTATIONS), S, device=device)
    out[..., 0] = torch.linspace(X_RANGE[0], X_RANGE[1], W, device=device).view(1, W, 1, 1)
    out[..., 1] = torch.linspace(Y_RANGE[0], Y_RANGE[1], H, device=device).view(H, 1, 1, 1)
    out[..., 2] = torch.tensor(Z, device=device).view(1, 1, -1, 1)
    out[..., 3:6] = torch.tensor(SIZES, device=device).view(1, 1, -1, 1, 3)
    out[..., 6] = torch.tensor(ROTATIONS, device=device).view(1, 1, 1, -1)
    return out.view(-1, S)


def torch_chain(cls_map, reg_map, dir_map, anchors):
    """what the head does between its maps and the NMS for one image and one level, as plain torch: maps to
    (anchor, channel) rows, sigmoid, best class, topk, gathers, box decode, BEV corners, a zero background column"""
    n = anchors.shape[0]
    logits = cls_map.permute(1, 2, 0).reshape(n, C)
    deltas = reg_map.permute(1, 2, 0).reshape(n, S)
    direction = dir_map.permute(1, 2, 0).reshape(n, 2).argmax(dim=1)
    prob = torch.sigmoid(logits)
    keep = torch.topk(prob.amax(dim=1), NMS_PRE).indices
    a, t, prob, direction = anchors[keep], deltas[keep], prob[keep], direction[keep]
    boxes = torch.empty_like(a)
    diag = torch.hypot(a[:, 3], a[:, 4])
    boxes[:, 0:2] = t[:, 0:2] * diag[:, None] + a[:, 0:2]
    boxes[:, 3:6] = torch.exp(t[:, 3:6]) * a[:, 3:6]
    boxes[:, 2] = t[:, 2] * a[:, 5] + (a[:, 2] + 0.5 * a[:, 5]) - 0.5 * boxes[:, 5]
    boxes[:, 6] = t[:, 6] + a[:, 6]
    half = 0.5 * boxes[:, 3:5]
    bev = torch.cat([boxes[:, 0:2] - half, boxes[:, 0:2] + half, boxes[:, 6:7]], dim=1)
    scores = torch.nn.functional.pad(prob, (0, 1))
    return boxes, bev, scores, direction, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert args.iters >= 50
    pkg = importlib.import_module('depth-from-motion_amd')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    device = torch.device('cuda', 0)
    gen = torch.Generator(device='cpu').manual_seed(304288)
    # a detector's maps: mostly background (logits around -4), a fp32 head
    cls = (torch.randn(1, 6 * C, H, W, generator=gen) * 1.5 - 4.0).to(device)
    reg = (torch.randn(1, 6 * S, H, W, generator=gen) * 0.25).to(device)
    dirs = torch.randn(1, 12, H, W, generator=gen).to(device)
    anchors = grid_anchors(device)

    def fused():
        return pkg.anchor_head_candidates([cls], [reg], [dirs], [anchors], num_classes=C, nms_pre=NMS_PRE)

    def chain():
        return torch_chain(cls[0], reg[0], dirs[0], grid_anchors(device))

    def chain_cached():
        return torch_chain(cls[0], reg[0], dirs[0], anchors)

    say(f'{torch.cuda.get_device_name(0)}; us, median / p10 / p90 of {args.iters} iterations after {args.warmup}')
    got, want = fused(), chain()
    same_set = int(len(set(got[4][0].tolist()) ^ set(want[4].tolist())))
    pos = torch.empty(anchors.shape[0], dtype=torch.int64, device=device)
    pos[want[4]] = torch.arange(NMS_PRE, device=device)
    rows = pos[got[4][0]] if same_set == 0 else torch.arange(NMS_PRE, device=device)
    say(f'{anchors.shape[0]} anchors -> {NMS_PRE} rows; fused against torch: {same_set} indices in one set only, '
        f'{int((got[4][0] != want[4]).sum())} rows in another order (equal or near-equal keys), '
        f'{int((got[3][0] != want[3][rows]).sum())} direction bins differ, scores within '
        f'{float((got[2][0] - want[2][rows]).abs().max()):.3g}, boxes within '
        f'{float((got[0][0] - want[0][rows]).abs().max()):.3g}, BEV boxes within '
        f'{float((got[1][0] - want[1][rows]).abs().max()):.3g}')
    fused_ops = None
    for name, fn in (('fused (anchor_head_candidates)', fused), ('torch, anchors rebuilt per call', chain),
                     ('torch, cached anchors', chain_cached)):
        med, lo, hi = timed(fn, args.iters, args.warmup)
        ops = device_ops(fn)
        tail = (f'{len(ops):5d} device operations, {sum(t for _, t in ops):9.1f} us in them' if ops
                else 'device operations n/a')
        say(f'{name:32s} {med:9.1f} {lo:9.1f} {hi:9.1f}   {tail}')
        if fn is fused:
            fused_ops = ops
    for name, t in fused_ops or ():
        say(f'    fused: {t:8.1f} us  {name[:100]}')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
