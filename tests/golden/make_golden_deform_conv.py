"""Generate tests/golden/deform_conv.npz: the modulated deformable convolution (DCNv2).

Run anywhere torch runs (it needs nothing of the reference checkout):   python tests/golden/make_golden_deform_conv.py

STAND-IN.  The reference runs these layers through ``mmcv.ops.modulated_deform_conv2d`` (mmcv/ops/
modulated_deform_conv.py over modulated_deform_conv_cuda_kernel.cuh); mmcv is not installed and is not part of the
reference tree.  ``dcn_columns`` / ``dcn_forward`` below are a torch restatement of the semantics that
include/dfm_hip_deform_conv.h states: tap k = 3 i + j, offset channel g * 18 + 2 k the row and + 1 the column
displacement, the sample 0 unless ``h > -1 && w > -1 && h < H && w < W``, ``h0 = floor(h)``, ``lh = h - h0``,
``hh = 1 - lh``, a corner outside the map 0, ``val = (((hh hw) v00 + (hh lw) v01) + (lh hw) v10) + (lh lw) v11``,
``col = val * mask``, ``out = bias + sum W col``; ``ModulatedDeformConv2dPack``'s raw 27 G-channel map is
``offset = cat(o1, o2)``, ``mask = sigmoid(o3)`` of its three chunks.  It is written once for any dtype with explicit
floor, index and ``where`` arithmetic -- no ``grid_sample`` -- one torch operation per operation of the header, and
differentiated by autograd: the derivative with respect to a coordinate is that of the floor formula, the right-hand
difference at an integer, as mmcv's dmcn_get_coordinate_weight gives it.
  * run in fp64 it gives the expected values and gradients; the fp64 gradient is checked here against central
    differences (step 1e-6, agreement asserted at 1e-6 of the gradient's largest component) on the general-position
    cases;
  * run in fp32 on the CPU (eager torch: one IEEE rounding per operation, no contraction) it gives the columns the
    kernels must reproduce bit for bit, and measures what fp32 arithmetic costs.

WHAT IS STORED.  The case table's expected values do not fit the size limit of a committed file (the columns of
``chunks`` alone are 539 KB, its fp64 weight gradient 442 KB), so the fixture holds what cannot be recomputed and pins
the rest: per case the INPUTS (x, weight and grad_out as bfloat16 bit patterns -- every value is exactly representable,
so one set of fp32 columns serves the fp32 and the bf16 kernels --, offsets / masks / the raw map and the bias in
fp32), the SHA-256 of the stand-in's fp32 columns, and the fp32-vs-fp64 ERROR FIGURES.  tests/deform_conv_ref.py
imports this file, runs the stand-in once per session on the stored inputs, and the CPU test asserts that the columns
it computed hash to the stored value: what the GPU is compared with is what this generator produced.  The small
expected outputs the CPU self-checks need (``zero_offset``, ``special``) are stored in full.

Error figures ``err_<case>`` = (forward, grad_x, grad_weight, grad_offset, grad_mask): the largest |fp32 - fp64| of
the stand-in over the quantity divided by the largest |fp64| of the quantity, and never below one fp32 ulp, 2^-23:
whatever the order of its sums, an fp32 result carries the half-ulp rounding of each product and of the result itself,
so a figure below that is the luck of one summation order on one small sample, not what fp32 arithmetic costs.  The
GPU tests read them from here; no tolerance of that kind is written into a test.  ``grad_mask`` is the gradient of
the logit in the raw cases.

General position.  In the cases whose gradients are compared, every sampling coordinate is at least GUARD = 1e-3
away from an integer (the cuts -1, H, W are integers): an offending offset is moved by 4 GUARD, none is dropped.  The
dedicated cases sit exactly on those points on purpose: ``zero_offset`` (every coordinate an integer), ``far`` (some
exactly -1, H, W; integer offsets are exact in fp32 and fp64 alike, so both precisions take the same branch).

Cases (N, Cin -> Cout, H x W, stride, padding, dilation):
  one_chunk    1  32 -> 32   5 x 7   s1        one 64-channel chunk, 35 pixels: less than one tile
  chunks       2  64 -> 96   9 x 13  s1        several chunks, pixel count no tile multiple, a tile across the images
  stride2      2  64 -> 64   9 x 13  s2        odd extents under stride 2
  dil2         1  32 -> 32   9 x 9   s1 d2 p2  dilation
  zero_offset  1  32 -> 64   6 x 6   s1, s2    raw map all zero (offsets 0, logits 0): half a plain convolution, and the
                                               right-hand derivative
  far          1  32 -> 32   6 x 8   s1        offsets to +-(H + 3): many samples outside, some in the (-1, 0) and
                                               (H - 1, H) bands, some exactly -1, H, W
  special      1  32 -> 32   5 x 5   s1        NaN, +-inf, +-1e30 offsets at a few pixels: value 0, gradients 0
  bias_raw     1  32 -> 32   5 x 7   s1        bias, and the raw 27-channel map with logits
  g2           1  64 -> 32   5 x 7   s1        deform_groups = 2
"""
import hashlib
import os

import numpy as np
import torch

GUARD = 1e-3
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'deform_conv.npz')

# name: (N, Cin, Cout, H, W, stride, padding, dilation, G, raw, bias)
CASES = {
    'one_chunk': (1, 32, 32, 5, 7, 1, 1, 1, 1, False, False),
    'chunks': (2, 64, 96, 9, 13, 1, 1, 1, 1, False, False),
    'stride2': (2, 64, 64, 9, 13, 2, 1, 1, 1, False, False),
    'dil2': (1, 32, 32, 9, 9, 1, 2, 2, 1, False, False),
    'zero_offset': (1, 32, 64, 6, 6, 1, 1, 1, 1, True, False),
    'zero_offset_s2': (1, 32, 64, 6, 6, 2, 1, 1, 1, True, False),
    'far': (1, 32, 32, 6, 8, 1, 1, 1, 1, False, False),
    'special': (1, 32, 32, 5, 5, 1, 1, 1, 1, False, False),
    'bias_raw': (1, 32, 32, 5, 7, 1, 1, 1, 1, True, True),
    'g2': (1, 64, 32, 5, 7, 1, 1, 1, 2, False, False),
}
GENERAL = ('one_chunk', 'chunks', 'stride2', 'dil2', 'bias_raw', 'g2')   # gradients in general position
QUANTITIES = ('out', 'grad_x', 'grad_weight', 'grad_offset', 'grad_mask')


def out_size(h, w, stride, padding, dilation):
    return (h + 2 * padding - (2 * dilation + 1)) // stride + 1, (w + 2 * padding - (2 * dilation + 1)) // stride + 1


def split_raw(raw, groups):
    """ModulatedDeformConv2dPack: the raw conv_offset map -> (offset, mask)"""
    o1, o2, o3 = torch.chunk(raw, 3, dim=1)
    return torch.cat((o1, o2), dim=1), torch.sigmoid(o3)


def base_coordinates(extent, stride, padding, dilation, dtype, device=None):
    """(3, extent): tap i of output index o sits at o * stride - padding + i * dilation (integers, exact)"""
    o = torch.arange(extent, dtype=torch.int64, device=device)
    i = torch.arange(3, dtype=torch.int64, device=device)
    return (o[None] * stride - padding + i[:, None] * dilation).to(dtype)


def dcn_columns(x, offset, mask, stride=1, padding=0, dilation=1, groups=1):
    """the columns (N, Ho, Wo, 9, Cin) in x's dtype, one torch operation per operation of the header"""
    n, c, h, w = x.shape
    ho, wo = out_size(h, w, stride, padding, dilation)
    cg = c // groups
    off = offset.reshape(n, groups, 9, 2, ho, wo)
    dy, dx = off[:, :, :, 0], off[:, :, :, 1]                                   # (N, G, 9, Ho, Wo)
    bh = base_coordinates(ho, stride, padding, dilation, x.dtype, x.device)     # (3, Ho)
    bw = base_coordinates(wo, stride, padding, dilation, x.dtype, x.device)     # (3, Wo)
    bh = bh[:, None, :, None].expand(3, 3, ho, wo).reshape(9, ho, wo)           # tap k = 3 i + j: row of i
    bw = bw[None, :, None, :].expand(3, 3, ho, wo).reshape(9, ho, wo)           # column of j
    hc, wc = bh + dy, bw + dx
    inside = (hc > -1) & (wc > -1) & (hc < h) & (wc < w)                         # false for NaN
    zero = torch.zeros((), dtype=x.dtype, device=x.device)
    hs, ws = torch.where(inside, hc, zero), torch.where(inside, wc, zero)
    h0, w0 = torch.floor(hs), torch.floor(ws)
    lh, lw = hs - h0, ws - w0
    hh, hw = 1 - lh, 1 - lw
    h0i, w0i = h0.detach().long(), w0.detach().long()
    flat = x.reshape(n, groups, cg, h * w)

    def corner(hi, wi):
        ok = inside & (hi >= 0) & (hi <= h - 1) & (wi >= 0) & (wi <= w - 1)
        idx = (hi.clamp(0, h - 1) * w + wi.clamp(0, w - 1)).reshape(n, groups, 1, -1).expand(n, groups, cg, -1)
        v = torch.gather(flat, 3, idx).reshape(n, groups, cg, 9, ho, wo)
        return torch.where(ok[:, :, None], v, zero)

    v00, v01, v10, v11 = corner(h0i, w0i), corner(h0i, w0i + 1), corner(h0i + 1, w0i), corner(h0i + 1, w0i + 1)
    e = lambda t: t[:, :, None]  # noqa: E731  (N, G, 1, 9, Ho, Wo)
    val = (((e(hh * hw) * v00 + e(hh * lw) * v01) + e(lh * hw) * v10) + e(lh * lw) * v11)
    col = torch.where(e(inside), val * e(mask.reshape(n, groups, 9, ho, wo)), zero)
    return col.permute(0, 4, 5, 3, 1, 2).reshape(n, ho, wo, 9, c)


def dcn_forward(x, offset, mask, weight, bias=None, stride=1, padding=0, dilation=1, groups=1):
    col = dcn_columns(x, offset, mask, stride, padding, dilation, groups)
    n, ho, wo = col.shape[:3]
    w2 = weight.permute(0, 2, 3, 1).reshape(weight.shape[0], -1)                # (Cout, 9 Cin), tap-major
    out = col.reshape(n * ho * wo, -1) @ w2.t()
    if bias is not None:
        out = out + bias
    return out.reshape(n, ho, wo, -1).permute(0, 3, 1, 2)


def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float32)


def bf16_bits(t):
    return t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def from_bf16_bits(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).view(torch.bfloat16).to(torch.float32)


def coordinates(case, offset):
    """(hc, wc) of every (n, g, k, ho, wo) in fp32, as the kernels form them"""
    n, cin, cout, h, w, stride, padding, dilation, groups, raw, _ = CASES[case]
    ho, wo = out_size(h, w, stride, padding, dilation)
    off = offset.reshape(n, groups, 9, 2, ho, wo)
    bh = base_coordinates(ho, stride, padding, dilation, torch.float32)[:, None, :, None].expand(3, 3, ho, wo)
    bw = base_coordinates(wo, stride, padding, dilation, torch.float32)[None, :, None, :].expand(3, 3, ho, wo)
    return bh.reshape(9, ho, wo) + off[:, :, :, 0], bw.reshape(9, ho, wo) + off[:, :, :, 1]


def keep_off_integers(case, offset):
    """move every offset whose coordinate lies within GUARD of an integer; none dropped"""
    offset = offset.clone()
    n, cin, cout, h, w, stride, padding, dilation, groups, raw, _ = CASES[case]
    ho, wo = out_size(h, w, stride, padding, dilation)
    for _ in range(8):
        hc, wc = coordinates(case, offset)
        bad = torch.stack((((hc.double() - hc.double().round()).abs() < GUARD),
                           ((wc.double() - wc.double().round()).abs() < GUARD)), dim=3)     # (N, G, 9, 2, Ho, Wo)
        if not bad.any():
            return offset
        offset = offset + 4 * GUARD * bad.reshape(offset.shape).float()
    raise AssertionError('could not move the offsets into general position')


def make_inputs(case, gen):
    n, cin, cout, h, w, stride, padding, dilation, groups, raw, has_bias = CASES[case]
    ho, wo = out_size(h, w, stride, padding, dilation)
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    d = dict(x=bf16_round(r(n, cin, h, w)), weight=bf16_round(r(cout, cin, 3, 3) * (2.0 / (9 * cin)) ** 0.5),
             grad_out=bf16_round(r(n, cout, ho, wo)))
    if has_bias:
        d['bias'] = r(cout)
    offset = r(n, 18 * groups, ho, wo) * 1.5
    mask = torch.rand(n, 9 * groups, ho, wo, generator=gen)
    if case.startswith('zero_offset'):
        d['raw'] = torch.zeros(n, 27 * groups, ho, wo)
        return d
    if case == 'far':
        offset = (torch.rand(n, 18, ho, wo, generator=gen) * 2 - 1) * (h + 3)
        offset = keep_off_integers(case, offset)
        o = offset.reshape(n, 9, 2, ho, wo)
        # exactly on the cuts: tap k of pixel (ho, wo) sits at row ho - 1 + k // 3, column wo - 1 + k % 3
        for k, (py, px, ty, tx) in enumerate([(0, 0, -1.0, 2.0), (1, 2, float(h), 3.0), (2, 3, 2.0, float(w)),
                                              (3, 1, -1.0, -1.0), (4, 4, float(h - 1), float(w - 1)),
                                              (5, 5, 0.0, 0.0), (1, 6, -0.5, 2.5), (2, 7, h - 0.5, w - 0.5),
                                              (0, 3, -0.25, -0.75)]):
            o[0, k, 0, py, px] = ty - (py - 1 + k // 3)
            o[0, k, 1, py, px] = tx - (px - 1 + k % 3)
        d.update(offset=offset, mask=mask)
        return d
    offset = keep_off_integers(case, offset)
    if case == 'special':
        o = offset.reshape(n, 9, 2, ho, wo)
        for k, (py, px, vy, vx) in enumerate([(0, 0, float('nan'), 0.3), (1, 1, 0.3, float('nan')),
                                              (2, 2, float('inf'), 0.2), (3, 3, 0.2, float('-inf')),
                                              (4, 4, 1e30, 0.1), (0, 4, 0.1, -1e30), (4, 0, float('nan'), float('inf')),
                                              (2, 0, -1e30, 1e30), (1, 3, float('-inf'), float('nan'))]):
            o[0, k, 0, py, px], o[0, k, 1, py, px] = vy, vx
    if raw:
        logits = r(n, 9 * groups, ho, wo) * 1.5
        d['raw'] = torch.cat((offset, logits), dim=1)
    else:
        d.update(offset=offset, mask=mask)
    return d


def run(case, inputs, dtype):
    """the stand-in in ``dtype`` on the stored inputs -> dict(col, out, grad_x, grad_weight, grad_offset, grad_mask
    [, grad_bias]); in the raw cases grad_offset / grad_mask are the two parts of the raw map's gradient (grad_mask
    that of the logits)"""
    n, cin, cout, h, w, stride, padding, dilation, groups, raw, has_bias = CASES[case]
    leaf = lambda t: t.to(dtype).clone().requires_grad_(True)  # noqa: E731
    x, weight = leaf(inputs['x']), leaf(inputs['weight'])
    bias = leaf(inputs['bias']) if has_bias else None
    if raw:
        maps = (leaf(inputs['raw']),)
        offset, mask = split_raw(maps[0], groups)
    else:
        maps = (leaf(inputs['offset']), leaf(inputs['mask']))
        offset, mask = maps
    with torch.no_grad():
        col = dcn_columns(x, offset, mask, stride, padding, dilation, groups)
    out = dcn_forward(x, offset, mask, weight, bias, stride, padding, dilation, groups)
    leaves = (x, weight, *maps) + ((bias,) if has_bias else ())
    grads = torch.autograd.grad((out * inputs['grad_out'].to(dtype)).sum(), leaves)
    res = dict(col=col.detach(), out=out.detach(), grad_x=grads[0], grad_weight=grads[1])
    if raw:
        res['grad_offset'], res['grad_mask'] = grads[2][:, :18 * groups], grads[2][:, 18 * groups:]
    else:
        res['grad_offset'], res['grad_mask'] = grads[2], grads[3]
    if has_bias:
        res['grad_bias'] = grads[-1]
    return res


def error_figures(r32, r64):
    figs = []
    for q in QUANTITIES:
        scale = r64[q].abs().max().item()
        figs.append(max((r32[q].double() - r64[q]).abs().max().item() / scale, 2.0 ** -23) if scale > 0 else 0.0)
    return np.asarray(figs, dtype=np.float64)


def columns_digest(col32):
    return hashlib.sha256(np.ascontiguousarray(col32.numpy().astype('<f4')).tobytes()).hexdigest()


def load_inputs(z, case):
    d = {k: from_bf16_bits(z[f'{case}.{k}']) for k in ('x', 'weight', 'grad_out')}
    for k in ('offset', 'mask', 'raw', 'bias'):
        if f'{case}.{k}' in z:
            d[k] = torch.from_numpy(z[f'{case}.{k}'])
    return d


def check_central_differences(case, inputs, r64, gen, count=12, step=1e-6):
    """the fp64 gradients of sum(out * grad_out) against central differences at ``count`` random components each"""
    n, cin, cout, h, w, stride, padding, dilation, groups, raw, has_bias = CASES[case]
    names = [('x', 'grad_x'), ('weight', 'grad_weight')] + \
        ([('raw', None)] if raw else [('offset', 'grad_offset'), ('mask', 'grad_mask')])

    def loss(inp):
        t = {k: v.double() for k, v in inp.items()}
        offset, mask = split_raw(t['raw'], groups) if raw else (t['offset'], t['mask'])
        out = dcn_forward(t['x'], offset, mask, t['weight'], t.get('bias'), stride, padding, dilation, groups)
        return (out * t['grad_out']).sum().item()

    for key, gname in names:
        g = torch.cat((r64['grad_offset'], r64['grad_mask']), dim=1) if gname is None else r64[gname]
        scale = g.abs().max().item()
        for _ in range(count):
            i = int(torch.randint(g.numel(), (1,), generator=gen))
            plus = {k: v.double().clone() for k, v in inputs.items()}
            minus = {k: v.double().clone() for k, v in inputs.items()}
            plus[key].view(-1)[i] += step
            minus[key].view(-1)[i] -= step
            fd = (loss(plus) - loss(minus)) / (2 * step)
            assert abs(fd - g.reshape(-1)[i].item()) <= 1e-6 * scale, (case, key, i, fd, g.reshape(-1)[i].item())


def main():
    gen = torch.Generator().manual_seed(20240607)
    store = {}
    for case in CASES:
        inputs = make_inputs(case, gen)
        for k in ('x', 'weight', 'grad_out'):
            store[f'{case}.{k}'] = bf16_bits(inputs[k])
        for k in ('offset', 'mask', 'raw', 'bias'):
            if k in inputs:
                store[f'{case}.{k}'] = inputs[k].numpy()
        r32, r64 = run(case, inputs, torch.float32), run(case, inputs, torch.float64)
        if case in GENERAL:
            check_central_differences(case, inputs, r64, gen)
        store[f'{case}.err'] = error_figures(r32, r64)
        store[f'{case}.col_sha256'] = np.asarray(columns_digest(r32['col']))
        if case.startswith('zero_offset') or case == 'special':
            store[f'{case}.out'] = r64['out'].numpy()
            store[f'{case}.grad_offset'] = r64['grad_offset'].numpy()
        print(f'{case:15s} err {store[f"{case}.err"]}')
    np.savez_compressed(OUT, **store)
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
