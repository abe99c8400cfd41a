#!/usr/bin/env python
"""Time the optimizer step -- global-norm clip + AdamW -- on the parameter set of DfMStereoPath at config K after
enable_fast_path(bf16), with seeded gradients.

    python tools/optimizer_step_timing.py [--out profiles/optimizer_step_timing.json]

Three versions of the same step, ALTERNATED in one process (window after window, so clock and temperature drift hit all
alike); a window is at least --window seconds of back-to-back steps between two device synchronisations, timed on the
host clock (the step is launches and little else: what matters is how long the loop takes), and the figure of a
version is the median of its windows' time per step:

  hip          : FusedAdamW(grad_clip=dict(max_norm=35, norm_type=2)).step() -- one table copy, two launches.
  torch_master : torch's equivalent of the SAME semantics: fp32 master copies of the bf16 parameters stepped by
                 torch.optim.AdamW(fused=True), the bf16 gradients cast to fp32 (torch._foreach_copy_ into preallocated
                 buffers), torch.nn.utils.clip_grad_norm_(foreach=True), the masters copied back to the bf16 parameters
                 (torch._foreach_copy_).  fp32 parameters are stepped in place.  This is the baseline.
  torch_plain  : for information only: clip_grad_norm_(foreach=True) and AdamW(fused=True) on the bf16 parameters
                 themselves.  It moves fewer bytes and does not train: bf16 updates round away (tests/test_optim.py).

There is no figure of the parent commit: it has no optimizer.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MAX_NORM, LR, WD = 35.0, 1e-3, 1e-4


def clones(params, grads):
    out = [torch.nn.Parameter(p.detach().clone(memory_format=torch.preserve_format)) for p in params]
    for p, g in zip(out, grads):
        p.grad = g.clone(memory_format=torch.preserve_format)
    return out


def hip_version(pkg, params):
    opt = pkg.FusedAdamW(params, lr=LR, weight_decay=WD, grad_clip=dict(max_norm=MAX_NORM, norm_type=2))
    return opt.step


def torch_master_version(params):
    narrow = [p for p in params if p.dtype != torch.float32]
    masters = [torch.nn.Parameter(p.detach().float()) for p in narrow]
    for m in masters:
        m.grad = torch.zeros_like(m)
    stepped = [p for p in params if p.dtype == torch.float32] + masters
    opt = torch.optim.AdamW(stepped, lr=LR, weight_decay=WD, fused=True)
    narrow_grads, master_grads = [p.grad for p in narrow], [m.grad for m in masters]
    narrow_data, master_data = [p.detach() for p in narrow], [m.detach() for m in masters]

    def step():
        torch._foreach_copy_(master_grads, narrow_grads)
        torch.nn.utils.clip_grad_norm_(stepped, MAX_NORM, norm_type=2.0, foreach=True)
        opt.step()
        torch._foreach_copy_(narrow_data, master_data)
    return step


def torch_plain_version(params):
    opt = torch.optim.AdamW(params, lr=LR, weight_decay=WD, fused=True)

    def step():
        torch.nn.utils.clip_grad_norm_(params, MAX_NORM, norm_type=2.0, foreach=True)
        opt.step()
    return step


def window(step, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--window', type=float, default=0.5, help='seconds of back-to-back steps per window, at least')
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    importlib.import_module('depth-from-motion_amd.build').build_hip()
    pkg = importlib.import_module('depth-from-motion_amd')
    optim = importlib.import_module('depth-from-motion_amd.optim')
    dev = torch.device('cuda:0')
    with open(os.path.join(ROOT, 'tests', 'golden', 'configs_dfm.json')) as f:
        model = dict(json.load(f)['dfm_r34_1x8_kitti-3d-3class.py']['model'])
    torch.manual_seed(0)
    path = pkg.DfMStereoPath(model).to(dev).train()
    pkg.enable_fast_path(path)
    params = [p for p in path.parameters() if p.requires_grad]
    gen = torch.Generator(device=dev).manual_seed(1)
    grads = [torch.empty_like(p).copy_(1e-2 * torch.randn(p.shape, generator=gen, device=dev))  # the parameter's layout
             for p in params]
    n32 = sum(p.numel() for p in params if p.dtype == torch.float32)
    n16 = sum(p.numel() for p in params if p.dtype == torch.bfloat16)
    chunks = len(optim.chunk_table([p.numel() for p in params]))
    versions = {'hip': hip_version(pkg, clones(params, grads)),
                'torch_master': torch_master_version(clones(params, grads)),
                'torch_plain': torch_plain_version(clones(params, grads))}
    steps = {}
    for name, step in versions.items():
        for _ in range(args.warmup):
            step()
        per_step = window(step, 20)
        steps[name] = max(20, int(args.window / (per_step * 1e-3)) + 1)
    optim.counters(reset=True)
    versions['hip']()
    counters = optim.counters(reset=True)
    times = {name: [] for name in versions}
    for _ in range(args.windows):
        for name, step in versions.items():
            times[name].append(window(step, steps[name]))
    result = {
        'device': torch.cuda.get_device_name(0),
        'parameters': {'tensors': len(params), 'fp32_tensors': sum(p.dtype == torch.float32 for p in params),
                       'bf16_tensors': sum(p.dtype == torch.bfloat16 for p in params), 'fp32_elements': n32,
                       'bf16_elements': n16, 'chunks': chunks},
        'max_norm': MAX_NORM, 'window_s': args.window, 'windows': args.windows, 'warmup_steps': args.warmup,
        'steps_per_window': steps,
        'ms_per_step_median': {name: round(statistics.median(t), 4) for name, t in times.items()},
        'ms_per_step_min_max': {name: [round(min(t), 4), round(max(t), 4)] for name, t in times.items()},
        'hip_counters_per_step': counters,
        # fp32: 4 B (norm pass) + 28 B (g, p, m, v read; p, m, v written); bf16 with master: 2 B + 30 B
        'hip_bytes_per_step': {'norm_pass': 4 * n32 + 2 * n16, 'step_pass': 28 * n32 + 30 * n16},
    }
    med = result['ms_per_step_median']
    result['hip_over_torch_master'] = round(med['hip'] / med['torch_master'], 3)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
