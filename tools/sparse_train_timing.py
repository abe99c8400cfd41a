#!/usr/bin/env python
"""Time one training step (forward + backward) of the LiDAR teacher's sparse encoder at its real size on one GPU.

    python tools/sparse_train_timing.py [--points 120000] [--iters 10] [--warmup 3]

The encoder is that of configs/dfm/second_teacher.py (``sparse_shape=[41, 1600, 1408]``, SyncBN eps 1e-3 momentum
0.01); the input is the seeded synthetic 120 000-point frame of tools/lidar_teacher_timing.py, voxelized over the
config's range (at most 40 000 voxels).  The tool prints, as medians over --iters runs timed with device events: the
eval forward (unmarked encoder, ``torch.no_grad()``: the number the training step is compared with), the training
forward, the backward and the whole step of the encoder marked by ``enable_sparse_training``; then per layer the time
of its convolution, BatchNorm forward (statistics + apply + running statistics), BatchNorm backward (reduce + apply),
input-gradient and weight-gradient launches, and the number of C-ABI launches of one step.  One JSON line at the end
repeats the figures.
"""
import argparse
import importlib
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POINT_CLOUD_RANGE = [0, -40, -3, 70.4, 40, 1]
ENCODER = dict(in_channels=3, output_channels=32, encoder_strides=((1, ), (2, 1, 1), (2, 1, 1), ((2, 1, 1), 1, 1)),
               sparse_shape=[41, 1600, 1408], order=('conv', 'norm', 'act'),
               norm_cfg=dict(type='SyncBN', eps=1e-3, momentum=0.01), with_final_bnrelu=False, output_volume_feat=True)
GROUPS = {'dfm_sparse_bn_stats': 'bn fwd', 'dfm_sparse_bn_apply': 'bn fwd', 'dfm_sparse_bn_running': 'bn fwd',
          'dfm_sparse_bn_bwd_reduce': 'bn bwd', 'dfm_sparse_bn_bwd_apply': 'bn bwd',
          'dfm_sparse_conv_wgrad': 'weight grad', 'dfm_sparse_inverse_table': 'inverse table'}


def synthetic_cloud(points, seed):
    spec = importlib.util.spec_from_file_location('lidar_teacher_timing',
                                                  os.path.join(ROOT, 'tools', 'lidar_teacher_timing.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.synthetic_cloud(points, seed)


def median_ms(pairs, skip):
    return float(np.median([a.elapsed_time(b) for a, b in pairs[skip:]]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=120000)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    pkg = importlib.import_module('depth-from-motion_amd')
    st = importlib.import_module('depth-from-motion_amd.sparse_train')
    sc = importlib.import_module('depth-from-motion_amd.sparse_conv')
    torch.manual_seed(0)
    cloud = torch.from_numpy(synthetic_cloud(args.points, 7)).cuda()
    voxel_layer = pkg.Voxelization([0.05, 0.05, 0.1], POINT_CLOUD_RANGE, 5, (40000, 40000)).cuda()
    voxels, coors, num, count = voxel_layer.forward_batch([cloud])
    feats = pkg.HardSimpleVFE(num_features=3)(voxels, num, coors).contiguous()
    enc = pkg.CustomSparseEncoder(**ENCODER).cuda()
    runs = args.warmup + args.iters

    def event():
        return torch.cuda.Event(enable_timing=True)

    # the eval forward of the unmarked encoder
    enc.eval()
    eval_pairs = []
    with torch.no_grad():
        for _ in range(runs):
            a, b = event(), event()
            a.record()
            enc(feats, coors, 1)
            b.record()
            eval_pairs.append((a, b))
    enc.check_status()

    pkg.enable_sparse_training(enc)
    enc.train()
    weights = None

    def step(marks=None):
        nonlocal weights
        for p in enc.parameters():
            p.grad = None
        e = [event() for _ in range(3)]
        e[0].record()
        _, volume = enc(feats, coors, 1)
        if weights is None:
            weights = torch.rand_like(volume)
        e[1].record()
        if marks is not None:
            marks.append('backward')
        (volume * weights).sum().backward()
        e[2].record()
        return e

    whole = [step() for _ in range(runs)]
    enc.check_status()
    torch.cuda.synchronize()
    rows = [int((t.indices[:, 0] >= 0).sum()) for t in enc.forward_stages(feats, coors, 1)]

    # per launch: every C-ABI launch of the step between two events, keyed by its place in the step
    real = st.launch
    samples, order, phase = {}, [], []

    def timed(name, *a, **k):
        a0, b0 = event(), event()
        a0.record()
        out = real(name, *a, **k)
        b0.record()
        index = len(order)
        kind = GROUPS.get(name) or (('input grad' if phase else 'conv fwd') if name == 'dfm_sparse_conv_fwd' else name)
        order.append((kind, name))
        samples.setdefault(index, []).append((a0, b0))
        return out

    st.launch = sc.launch = timed
    try:
        for _ in range(runs):
            order.clear()
            phase.clear()
            step(phase)
    finally:
        st.launch = sc.launch = real
    torch.cuda.synchronize()

    layers = ['conv_input'] + [f'{n}.{i}' for n, s in enc.encoder_layers.named_children() for i in range(len(s))] + \
        ['conv_out']
    convs = [m for m in enc.modules() if isinstance(m, (pkg.SubMConv3d, pkg.SparseConv3d))]
    label = {n: f'{n} {type(c).__name__} {c.in_channels}->{c.out_channels}' for n, c in zip(layers, convs)}
    per_layer = {n: {} for n in layers}
    seen = {}
    backward_kinds = ('bn bwd', 'input grad', 'weight grad')
    bn_layers = [n for n, c in zip(layers, convs) if n != 'conv_out']
    grad_in_layers = [n for n, c in zip(layers, convs) if c.in_channels in (16, 32, 64)]
    for index, (kind, name) in enumerate(order):
        ms = median_ms(samples[index], args.warmup)
        if kind in ('conv fwd', 'weight grad'):
            names = layers
        elif kind in ('bn fwd', 'bn bwd'):
            names = bn_layers
        elif kind == 'input grad':
            names = grad_in_layers
        else:
            per_layer.setdefault('index and tables', {})
            per_layer['index and tables'][kind] = per_layer['index and tables'].get(kind, 0.0) + ms
            continue
        per_kernel = {'bn fwd': 3, 'bn bwd': 2}.get(kind, 1)
        i = seen.get(kind, 0)
        seen[kind] = i + 1
        layer = names[len(names) - 1 - i // per_kernel] if kind in backward_kinds else names[i // per_kernel]
        per_layer[layer][kind] = per_layer[layer].get(kind, 0.0) + ms

    eval_ms = median_ms(eval_pairs, args.warmup)
    fwd_ms = median_ms([(e[0], e[1]) for e in whole], args.warmup)
    bwd_ms = median_ms([(e[1], e[2]) for e in whole], args.warmup)
    step_ms = median_ms([(e[0], e[2]) for e in whole], args.warmup)
    print(f'cloud: {args.points} points -> {int(count)} voxels (max_voxels 40000); live rows after conv_input, the '
          f'four stages and conv_out: {rows}')
    print(f'eval forward (unmarked, no_grad) {eval_ms:8.3f} ms')
    print(f'training forward                 {fwd_ms:8.3f} ms')
    print(f'training backward                {bwd_ms:8.3f} ms')
    print(f'training step                    {step_ms:8.3f} ms = {step_ms / eval_ms:.2f} x the eval forward')
    kinds = ('conv fwd', 'bn fwd', 'bn bwd', 'input grad', 'weight grad')
    print(f'{"layer (us)":48s}' + ''.join(f'{k:>13s}' for k in kinds))
    for n in layers:
        print(f'{label[n]:48s}' + ''.join(f'{per_layer[n].get(k, 0.0) * 1000:13.1f}' for k in kinds))
    for k, v in per_layer.get('index and tables', {}).items():
        print(f'{k:48s}{v * 1000:13.1f}')
    totals = {k: sum(per_layer[n].get(k, 0.0) for n in layers) for k in kinds}
    print(f'{"sum":48s}' + ''.join(f'{totals[k] * 1000:13.1f}' for k in kinds))
    print(f'C-ABI launches of one step: {len(order)}')
    print(json.dumps(dict(points=args.points, voxels=int(count), live_rows=rows, eval_forward_ms=round(eval_ms, 3),
                          train_forward_ms=round(fwd_ms, 3), train_backward_ms=round(bwd_ms, 3),
                          train_step_ms=round(step_ms, 3), ratio=round(step_ms / eval_ms, 2),
                          per_layer_us={label[n]: {k: round(v * 1000, 1) for k, v in per_layer[n].items()}
                                        for n in layers},
                          kind_us={k: round(v * 1000, 1) for k, v in totals.items()}, launches=len(order))))


if __name__ == '__main__':
    main()
