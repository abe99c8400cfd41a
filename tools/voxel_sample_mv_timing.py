"""Wall time of the depth-supervision sampling of the multi-view detector (multiview_dfm.py:220-256) at the W
shape of SURVEY.md 8d: the loop of B x Nv ``voxel_sample`` calls + ``torch.cat`` against one ``voxel_sample_mv``
call, alternating in one process, for a bf16 channels-last and an fp32 contiguous volume.

    python tools/voxel_sample_mv_timing.py [--iters 10] [--rounds 5]

Prints per variant the median and the min..max over the rounds (each round: ``iters`` calls between two device
synchronisations, host work included -- the inversions, uploads and launches are part of what is compared), and
the achieved share of 8 TB/s from the algorithmic bytes (result written once + the volume read once per view)."""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

B, NV, C = 2, 5, 64
N_VOXELS = (220, 300, 12)
VOXEL_RANGE = [-35.0, -75.0, -2.0, 75.0, 75.0, 4.0]
VOXEL_SIZE = [0.5, 0.5, 0.5]
INPUT_SHAPE, DS, NUM_BINS = (832, 1248), 4, 48


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    pkg = importlib.import_module('depth-from-motion_amd')
    import make_golden as g1
    cams = g1.waymo_like_cameras(NV, B, 9).reshape(B, NV, 4, 4)
    s = np.diag([8.0, 8.0, 1.0, 1.0]).astype(np.float32)      # 104 x 156 intrinsics -> 832 x 1248
    cams = np.stack([[s @ m for m in cams[b]] for b in range(B)]).astype(np.float32)
    depths = torch.tensor([(i + 0.5) * (59.6 - 2) / NUM_BINS + 2 for i in range(NUM_BINS)])
    shapes = [[INPUT_SHAPE] * NV] * B
    gen = torch.Generator().manual_seed(1)
    base = torch.randn((B, C) + N_VOXELS, generator=gen).cuda()

    def batched(vol):
        return pkg.voxel_sample_mv(vol, VOXEL_RANGE, VOXEL_SIZE, depths, cams, DS, [1.0] * B, [0] * B, [False] * B,
                                   INPUT_SHAPE, shapes, NV)

    def looped(vol):
        return torch.cat([pkg.voxel_sample(vol[b][None], VOXEL_RANGE, VOXEL_SIZE, depths,
                                           torch.from_numpy(cams[b][v]), DS, 1.0, 0, False, INPUT_SHAPE,
                                           INPUT_SHAPE, aligned=True) for b in range(B) for v in range(NV)])

    for name, vol in (('bf16 channels_last_3d', base.bfloat16().contiguous(memory_format=torch.channels_last_3d)),
                      ('fp32 contiguous', base)):
        a, b = batched(vol), looped(vol)
        assert torch.equal(a, b)
        nbytes = a.numel() * a.element_size() + NV * vol.numel() * vol.element_size()
        print(f'{name}: result {tuple(a.shape)}, nonzero {float((a != 0).float().mean()):.3f}, '
              f'algorithmic bytes {nbytes / 1e6:.1f} MB')
        del a, b
        times = {'loop': [], 'batched': []}
        for _ in range(args.rounds):               # alternating: loop, batched, loop, batched ...
            for key, fn in (('loop', looped), ('batched', batched)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.iters):
                    fn(vol)
                torch.cuda.synchronize()
                times[key].append((time.perf_counter() - t0) / args.iters * 1e3)
        for key, t in times.items():
            med = statistics.median(t)
            print(f'  {key:8s} median {med:8.3f} ms  (min {min(t):.3f}, max {max(t):.3f} over {args.rounds} rounds of '
                  f'{args.iters})  {nbytes / med / 1e9 / 8.0 * 100:5.1f} % of 8 TB/s')
        print(f'  batched / loop = {statistics.median(times["batched"]) / statistics.median(times["loop"]):.3f}')


if __name__ == '__main__':
    main()
