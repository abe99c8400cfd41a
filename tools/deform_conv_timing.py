"""Time of the modulated deformable convolution (DCNv2) at the four layer shapes of the Waymo configs' ResNet-101 on
736 x 1088 padded views, N = 10 views (2 samples x 5 views of one frame):
  stage 3           256 -> 256   46 x 68              stride 1   (22 of the 23 stage-3 bottlenecks)
  stage 3, first    256 -> 256   92 x 136 -> 46 x 68  stride 2
  stage 4           512 -> 512   23 x 34              stride 1
  stage 4, first    512 -> 512   46 x 68 -> 23 x 34   stride 2

    python tools/deform_conv_timing.py [--iters 20] [--warmup 3] [--out FILE]

Per shape, in bf16 and fp32, forward (under no_grad) and forward + backward (gradients of x, the raw offset / mask map
and the weight), each the median with p10 / p90 of ``iters`` stream-event intervals; the variants of one row are run
in alternation, round after round, every shape warmed up first:
  dcn      ``modulated_deform_conv2d_raw``: the columns kernel, the matrix product with the (Cout, 9 Cin) weight, and
           in backward the columns again, two products and one ``dfm_deform_conv_bwd_cols`` launch
  torch    the stand-in of tests/golden/make_golden_deform_conv.py on the same GPU in the same dtype: the layer
           composed of torch operations (floor, where, four gathers, the blend, a matrix product; autograd for the
           backward) -- the only other way to run the layer without mmcv.  The bf16 ``dcn`` forward must be faster.
  plain    the same layer as a plain 3x3 convolution through ``MfmaConv2d`` (bf16: the MFMA kernels; fp32: split
           precision): the price of deformability, no bar.
Then, per shape and dtype, the backward kernel alone (C ABI, stream events): all three gradients, grad_offset and
grad_mask only, grad_x only -- the share of the kernel, and of the whole backward, that the grad_x scatter takes.  Its
atomic rate is the unmeasured assumption of the design."""
import argparse
import ctypes
import importlib
import importlib.util
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 10
SHAPES = (('stage 3', 256, 46, 68, 1), ('stage 3, first', 256, 92, 136, 2), ('stage 4', 512, 23, 34, 1),
          ('stage 4, first', 512, 46, 68, 2))


def interleaved(fns, iters, warmup):
    """{name: (median, p10, p90)} in us; the variants alternate within every round"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            times[k].append((a, b))
    torch.cuda.synchronize()
    out = {}
    for k, ev in times.items():
        t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
        out[k] = (statistics.median(t), t[int(0.1 * (len(t) - 1))], t[int(0.9 * (len(t) - 1))])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    dc = importlib.import_module('depth-from-motion_amd.deform_conv')
    conv3d = importlib.import_module('depth-from-motion_amd.conv3d')
    launch_mod = importlib.import_module('depth-from-motion_amd._launch')
    spec = importlib.util.spec_from_file_location(
        'make_golden_deform_conv', os.path.join(ROOT, 'tests', 'golden', 'make_golden_deform_conv.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f'{torch.cuda.get_device_name(0)}; us, median / p10 / p90 of {args.iters} alternating iterations after '
        f'{args.warmup}; N = {N}')
    faster = []
    for name, c, h, w, stride in SHAPES:
        ho, wo = dc.deform_conv_out_size((h, w), stride, 1, 1)
        flop = 2.0 * N * ho * wo * 9 * c * c
        say(f'{name}: {c} -> {c}, {h} x {w} -> {ho} x {wo}, stride {stride}; {flop / 1e9:.1f} GFLOP in the product')
        g = torch.Generator(device='cuda').manual_seed(5)
        for dtype in (torch.bfloat16, torch.float32):
            tag = 'bf16' if dtype == torch.bfloat16 else 'fp32'
            x = torch.randn(N, c, h, w, device='cuda', generator=g).to(dtype).contiguous(
                memory_format=torch.channels_last)
            weight = (torch.randn(c, c, 3, 3, device='cuda', generator=g) * (2.0 / (9 * c)) ** 0.5).to(dtype)
            raw = torch.randn(N, 27, ho, wo, device='cuda', generator=g).to(dtype)
            go = torch.randn(N, c, ho, wo, device='cuda', generator=g).to(dtype).contiguous(
                memory_format=torch.channels_last)
            plain = conv3d.MfmaConv2d(c, c, 3, stride=stride, padding=1, bias=False).cuda().to(dtype)
            with torch.no_grad():
                plain.weight.copy_(weight)
            leaves = [t.clone().requires_grad_(True) for t in (x, raw, weight)]
            px = x.clone().requires_grad_(True)

            def dcn_fwd():
                with torch.no_grad():
                    return dc.modulated_deform_conv2d_raw(x, raw, weight, None, stride, 1, 1, 1)

            def torch_fwd():
                with torch.no_grad():
                    return gen.dcn_forward(x, *gen.split_raw(raw, 1), weight, None, stride, 1, 1, 1)

            def plain_fwd():
                with torch.no_grad():
                    return plain(x)

            def dcn_train():
                for t in leaves:
                    t.grad = None
                dc.modulated_deform_conv2d_raw(leaves[0], leaves[1], leaves[2], None, stride, 1, 1, 1).backward(go)

            def torch_train():
                for t in leaves:
                    t.grad = None
                gen.dcn_forward(leaves[0], *gen.split_raw(leaves[1], 1), leaves[2], None, stride, 1, 1, 1).backward(go)

            def plain_train():
                px.grad = plain.weight.grad = None
                plain(px).backward(go)

            if dtype == torch.float32:   # (in bf16 the composition forms its coordinates in bf16: another function)
                a, b = dcn_fwd(), torch_fwd()
                say(f'  fp32: dcn against torch, forward: max |d| = {float((a - b).abs().max()):.3g} of '
                    f'{float(b.abs().max()):.3g}')
            fwd = interleaved(dict(dcn=dcn_fwd, torch=torch_fwd, plain=plain_fwd), args.iters, args.warmup)
            train = interleaved(dict(dcn=dcn_train, torch=torch_train, plain=plain_train), args.iters, args.warmup)
            for what, rows in (('forward', fwd), ('forward + backward', train)):
                for k in ('dcn', 'torch', 'plain'):
                    med, lo, hi = rows[k]
                    say(f'    {tag} {what:18s} {k:6s} {med:10.1f} {lo:10.1f} {hi:10.1f}'
                        + (f'   {flop / med / 1e6:7.1f} TFLOP/s of the product' if k == 'dcn' and what == 'forward'
                           else ''))
            if dtype == torch.bfloat16:
                faster.append((name, fwd['dcn'][0], fwd['torch'][0]))
            # the backward kernel alone
            geom = dc._check_geometry(tuple(x.shape), stride, 1, 1, 1)
            off, msk = dc._maps(raw, None, 1)
            gcol = torch.randn(N, ho, wo, 9, c, device='cuda', generator=g).to(dtype)
            gx = torch.zeros(N, h, w, c, device='cuda')
            gm = torch.empty(N, 27, ho, wo, device='cuda')
            so = (ctypes.c_int64 * 4)(*gm[:, :18].stride())
            sm = (ctypes.c_int64 * 4)(*gm[:, 18:].stride())
            desc = dc._desc(x, off, msk, geom, 1, True)

            def kernel(maps, data):
                def fn():
                    launch_mod.launch('dfm_deform_conv_bwd_cols', desc, x, off, msk, gcol,
                                      gm[:, :18] if maps else None, so if maps else None,
                                      gm[:, 18:] if maps else None, sm if maps else None, gx if data else None,
                                      launch_mod.STREAM)
                return fn

            k = interleaved(dict(all=kernel(True, True), maps=kernel(True, False), grad_x=kernel(False, True)),
                            max(args.iters, 20), args.warmup)
            atomic_mb = 36.0 * c * N * ho * wo * 4 / 1e6
            say(f'    {tag} dfm_deform_conv_bwd_cols alone: all {k["all"][0]:.1f}, grad_offset + grad_mask only '
                f'{k["maps"][0]:.1f}, grad_x only {k["grad_x"][0]:.1f} us; the scatter adds '
                f'{k["all"][0] - k["maps"][0]:.1f} us = {100 * (k["all"][0] - k["maps"][0]) / k["all"][0]:.0f} % of '
                f'the kernel, {100 * (k["all"][0] - k["maps"][0]) / (train["dcn"][0] - fwd["dcn"][0]):.0f} % of the '
                f'backward (forward + backward minus forward); {atomic_mb:.0f} MB of float adds if none were merged')
            del leaves, px, plain, gcol, gx, gm
            torch.cuda.empty_cache()
    say('bf16 forward, dcn against the torch composition: ' + '; '.join(
        f'{n}: {a:.0f} vs {b:.0f} us ({b / a:.1f}x)' for n, a, b in faster))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    assert all(a < b for _, a, b in faster), 'the bf16 forward is not faster than the torch composition'


if __name__ == '__main__':
    main()
