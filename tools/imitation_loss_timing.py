"""Device time of the feature-imitation loss at config K's two pairs -- volume_features (1, 32, 5, 304, 288) and
spatial_features_2d (1, 64, 304, 288), about 40 boxes, a sparse teacher target -- for the fused path
(``imitation_reg_layer_loss``: one launch forward, one backward) and for the torch composition of the
reference's ops (dfm.py:468-540: permute, any(!= 0), three boolean-mask gathers, normalise, isnan / where,
square, weight, two means) on the same GPU in the same process.  The composition is the only baseline there
is: nothing else in this repository computes the loss.  Its in-box mask is computed once outside the timed
region (the reference gets it from an mmcv op that is not available here), so the baseline is timed WITHOUT
the box test and the fused path with it.

    python tools/imitation_loss_timing.py [--iters 100] [--warmup 20] [--out FILE]

Per variant: forward and forward + backward, the median with p10 / p90 over ``iters`` iterations, each between
two events on the stream, no host synchronisation inside the loop; the in-box fraction of the scene; the
part's store rate (``dfm_store_probe`` and a linear fill), which bounds the backward's dense gradient write."""
import argparse
import ctypes
import importlib
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import imitation_util as iu  # noqa: E402

PAIRS = (('volume_features bf16 NDHWC student, fp32 planar teacher', (1, 32, 5, 304, 288), torch.bfloat16),
         ('volume_features fp32 NDHWC student, fp32 planar teacher', (1, 32, 5, 304, 288), torch.float32),
         ('spatial_features_2d fp32 NHWC student, fp32 planar teacher', (1, 64, 304, 288), torch.float32))


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

    points, boxes = iu.seeded_scene(31, 1, 304, 288, 0.2, 40, x0=2.0)
    cells = iu.inbox_cells(points, boxes).cuda()
    points, boxes = points.cuda(), boxes.cuda()
    say(f'device {torch.cuda.get_device_name(0)}; scene 304 x 288 cells, 40 boxes, in-box fraction '
        f'{float(cells.float().mean()):.4f}; {args.iters} iterations after {args.warmup} warm-up, microseconds')
    cfg = dict(mode='inbox', loss_weight=1.0)
    for name, shape, dtype in PAIRS:
        gen = torch.Generator().manual_seed(32)
        fmt = torch.channels_last_3d if len(shape) == 5 else torch.channels_last
        pred = torch.randn(shape, generator=gen).cuda().to(dtype).contiguous(memory_format=fmt).requires_grad_(True)
        t = torch.randn(shape, generator=gen)
        target = (t * (torch.rand((1, 1) + shape[2:], generator=gen) < 0.3)).cuda()
        layers = [pkg.NormalizeLayer('cw_scale', shape[1]).cuda().train() for _ in range(2)]

        def fused(backward):
            loss, _ = pkg.imitation_reg_layer_loss(pred, target, cfg, boxes, points, norm_layer=layers[0])
            if backward:
                pred.grad = None
                loss.backward()

        def composed(backward):
            loss, _ = iu.restate(pred, target, cells, layers[1], 1.0)
            if backward:
                pred.grad = None
                loss.backward()

        say(f'{name} {shape}')
        res = {}
        for key, fn in (('fused', fused), ('torch composition', composed)):
            for bw in (False, True):
                res[key, bw] = timed(lambda: fn(bw), args.iters, args.warmup)
                m, lo, hi = res[key, bw]
                say(f'  {key:18s} {"fwd+bwd" if bw else "fwd    "}  median {m:9.1f}  p10 {lo:9.1f}  p90 {hi:9.1f}')
        for bw in (False, True):
            say(f'  {"fwd+bwd" if bw else "fwd"}: fused median / composition p10 = '
                f'{res["fused", bw][0] / res["torch composition", bw][1]:.3f}')
    # the part: what a dense write of the volume pair's gradient can reach
    out = torch.empty((1, 32, 5 * 304 * 288), dtype=torch.float32, device='cuda')
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib = pkg._capi.lib()

    def probe(fn):
        m, _, _ = timed(fn, 50, 5)
        return out.numel() * out.element_size() / (m * 1e-6) / 1e9
    tile = probe(lambda: pkg._capi.check(lib.dfm_store_probe(ctypes.c_void_p(out.data_ptr()), 1, 32,
                                                             5 * 304 * 288 * 4, 0, 0, st)))
    say(f'store probe: {tile:.0f} GB/s (dfm_store_probe, 4 KiB runs), linear fill {probe(out.zero_):.0f} GB/s '
        f'over {out.numel() * 4 / 1e6:.1f} MB')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
