"""Every MFMA convolution body, exactly, at every voxel (csrc/conv3d_g.hip, conv3d_wgrad.hip, conv3d.hip,
conv3d_to1*.hip).

Operands are integers in [-4, 4]: exact in bf16, and every sum of products stays far below 2^24, so the kernels'
fp32 accumulation is exact whatever its order.  The fp32 results must then EQUAL the float64 reference, and the
bf16 results must equal it after one round-to-nearest-even.  Epilogue operands keep that: power-of-two scales,
shifts in quarters, integer residuals.  Output buffers sit inside sentinel-filled allocations whose bytes outside
the output must come back unchanged; inputs sit inside allocations filled with large values that a halo read
missing the zero page would pick up.  Each case first asserts that it still plans to the body
tests/conv_variants.py names for it.  One random-valued fp32 run per case checks the rounding against a bound
derived from the arithmetic: |got - ref| <= 27 C_in 2^-24 conv(|x|, |w|)."""
import ctypes
import importlib

import pytest
import torch
import torch.nn.functional as F

from tests import conv_variants as V

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
PRE, POST = 4096, 4096           # guard elements either side of a buffer (multiples of 8: 16-byte aligned)
SENTINEL16 = 0x5A5B               # bit pattern of the bf16 output guard
SENTINEL32 = 0x5A5B5C5D
BIG = 1024.0                      # what an input's surroundings hold


@pytest.fixture(scope='module')
def cv():
    assert torch.cuda.is_available()
    m = importlib.import_module('depth-from-motion_amd.conv3d')
    prev = m.set_fallback_policy('raise')
    yield m
    m.set_fallback_policy(prev)


def _ints(shape, seed, lo=-4, hi=4, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).to(dtype)


def _vp(addr):
    return ctypes.c_void_p(addr)


def _ptr(t):
    return _vp(t.data_ptr())


def _stream_ptr(device):
    return importlib.import_module('depth-from-motion_amd._launch').stream_ptr(device)


def _guarded_input(x_ndhwc, cstride):
    """x (N, D, H, W, C) bf16 -> (buffer, address of x's first element): x's pixels cstride elements apart, the
    other channels of each pixel and PRE / POST elements either side filled with BIG"""
    N, D, H, W, C = x_ndhwc.shape
    cs = cstride or C
    buf = torch.full((PRE + N * D * H * W * cs + POST,), BIG, dtype=torch.bfloat16, device=DEV)
    buf[PRE:PRE + N * D * H * W * cs].view(N, D, H, W, cs)[..., :C] = x_ndhwc.to(DEV)
    return buf, buf.data_ptr() + PRE * 2


def _guarded_output(numel, dtype):
    if dtype == torch.bfloat16:
        raw = torch.full((PRE + numel + POST,), SENTINEL16, dtype=torch.int16, device=DEV)
    else:
        raw = torch.full((PRE + numel + POST,), SENTINEL32, dtype=torch.int32, device=DEV)
    return raw, raw.view(dtype)[PRE:PRE + numel], raw.data_ptr() + PRE * raw.element_size()


def _guards_intact(raw, numel):
    s = SENTINEL16 if raw.dtype == torch.int16 else SENTINEL32
    return bool((raw[:PRE] == s).all()) and bool((raw[PRE + numel:] == s).all())


def _case_operands(c, seed):
    swap = any(c.transposed)
    x = _ints((c.n, c.cin, *c.size), seed)
    w = _ints((c.cin, c.cout, 3, 3, 3) if swap else (c.cout, c.cin, 3, 3, 3), seed + 1)
    return x, w, swap


def _ref64(c, x, w, swap):
    wr = w.transpose(0, 1) if swap else w
    return V.ref_conv(x.to(DEV, torch.float64), wr.to(DEV, torch.float64), c.stride, c.padding, c.transposed,
                      c.kernel1)


def _desc(cv, c, relu=False):
    out = V.g_case_out_size(c)
    return cv._conv_desc(c.n, c.cin, c.cout, c.size, out, V._triple(c.stride), V._triple(c.padding),
                         V._triple(c.transposed), relu, c.cstride, V._triple(c.kernel1))


@pytest.mark.parametrize('c', V.G_CASES, ids=[c.name for c in V.G_CASES])
def test_conv3d_g_every_body_exact_with_guards(cv, c):
    run = V.g_case_run(c)
    assert run == c.run, f'{c.name}: the planner now picks {run}, the table says {c.run}'
    lib = cv._capi.lib()
    x, w, swap = _case_operands(c, seed=c.cin + c.cout + sum(c.size))
    ref = _ref64(c, x, w, swap).permute(0, 2, 3, 4, 1).contiguous()          # (N, D', H', W', cout) float64
    xbuf, xaddr = _guarded_input(x.bfloat16().permute(0, 2, 3, 4, 1), c.cstride)
    pk = cv.pack_conv3d_g_weights(w.to(DEV), c.cin, c.cout, swap=swap)
    st = _stream_ptr(DEV)
    numel = ref.numel()
    oshape = ref.shape

    # epilogues: plain, scale / shift, residual, both + ReLU, ReLU alone
    g = torch.Generator().manual_seed(7)
    scale = (2.0 ** torch.randint(-2, 2, (c.cout,), generator=g)).float().to(DEV)
    shift = (torch.randint(-32, 33, (c.cout,), generator=g) / 4.0).float().to(DEV)
    res = _ints(tuple(oshape), seed=11, lo=-64, hi=64).bfloat16().to(DEV)
    for use_ss, use_res, relu in ((False, False, False), (True, False, False), (False, True, False),
                                  (True, True, True), (False, False, True)):
        raw, out, oaddr = _guarded_output(numel, torch.bfloat16)
        d = _desc(cv, c, relu)
        rc = lib.dfm_conv3d_g_fwd(ctypes.byref(d), _vp(xaddr), _ptr(pk),
                                  _ptr(scale) if use_ss else None, _ptr(shift) if use_ss else None,
                                  _ptr(res) if use_res else None, _vp(oaddr), st)
        assert rc == 0, lib.dfm_last_error()
        torch.cuda.synchronize()
        e = ref
        if use_ss:
            e = e * scale.double() + shift.double()
        if use_res:
            e = e + res.double()
        if relu:
            e = e.clamp_min(0)
        want = e.float().bfloat16()
        got = out.view(oshape)
        bad = (got.view(torch.int16) != want.view(torch.int16))
        assert not bad.any(), (f'{c.name} bf16 ss={use_ss} res={use_res} relu={relu}: {int(bad.sum())} voxels differ, '
                               f'first at {bad.nonzero()[0].tolist()}')
        assert _guards_intact(raw, numel), f'{c.name}: a store outside the output'

    # fp32 form: into a guarded buffer, then accumulating in place (acc_in == out)
    raw, out, oaddr = _guarded_output(numel, torch.float32)
    d = _desc(cv, c)
    assert lib.dfm_conv3d_g_fwd_f32(ctypes.byref(d), _vp(xaddr), _ptr(pk), None, _vp(oaddr), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(out.view(oshape), ref.float()), f'{c.name} fp32: max |diff| ' \
        f'{(out.view(oshape).double() - ref).abs().max().item()}'
    assert _guards_intact(raw, numel)
    acc = _ints(tuple(oshape), seed=12, lo=-1000, hi=1000)
    out.copy_(acc.view(-1))
    assert lib.dfm_conv3d_g_fwd_f32(ctypes.byref(d), _vp(xaddr), _ptr(pk), _vp(oaddr), _vp(oaddr), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(out.view(oshape), (ref + acc.to(DEV, torch.float64)).float()), f'{c.name} fp32 acc_in == out'
    assert _guards_intact(raw, numel)
    del xbuf


@pytest.mark.parametrize('c', V.G_CASES, ids=[c.name for c in V.G_CASES])
def test_conv3d_g_fp32_rounding_within_the_arithmetic_bound(cv, c):
    """random (non-integer) bf16 operands: fp32 accumulation of at most 27 C_in exact products,
    |got - ref| <= 27 C_in 2^-24 conv(|x|, |w|)"""
    assert V.g_case_run(c) == c.run
    g = torch.Generator().manual_seed(c.cin * 7 + c.cout)
    swap = any(c.transposed)
    x = torch.randn(c.n, c.cin, *c.size, generator=g).bfloat16().float()
    w = torch.randn(*((c.cin, c.cout) if swap else (c.cout, c.cin)), 3, 3, 3, generator=g).bfloat16().float()
    xs = x.bfloat16().to(DEV).contiguous(memory_format=torch.channels_last_3d)
    if c.cstride:
        wide = torch.full((c.n, c.cstride, *c.size), BIG, dtype=torch.bfloat16, device=DEV)
        wide = wide.contiguous(memory_format=torch.channels_last_3d)
        wide[:, :c.cin] = xs
        xs = wide[:, :c.cin]
    pk = cv.pack_conv3d_g_weights(w.to(DEV), c.cin, c.cout, swap=swap)
    got = cv.conv3d_g_f32(xs, pk, c.cout, c.stride, c.padding, c.transposed, c.kernel1).double()
    ref = _ref64(c, x, w, swap).permute(0, 2, 3, 4, 1)
    mag = _ref64(c, x.abs(), w.abs(), swap).permute(0, 2, 3, 4, 1)
    bound = 27 * c.cin * 2.0 ** -24 * mag
    err = (got - ref).abs()
    assert bool((err <= bound).all()), f'{c.name}: worst err / bound {(err / bound.clamp_min(1e-30)).max().item()}'


@pytest.mark.parametrize('c', V.W_CASES, ids=[c.name for c in V.W_CASES])
def test_conv3d_wgrad_every_kernel_exact(cv, c):
    run = V.w_case_run(c)
    assert tuple(run[:5]) == c.kind, f'{c.name}: wgrad_plan now gives {run}'
    g_size = V.w_case_g_size(c)
    x = _ints((c.n, c.b, *c.x_size), seed=c.b + sum(c.x_size))
    g = _ints((c.n, c.a, *g_size), seed=c.a + sum(g_size) + 1)
    ref = V.ref_wgrad(x.to(DEV, torch.float64), g.to(DEV, torch.float64), c.stride, c.padding)
    cl = torch.channels_last_3d
    xd = x.bfloat16().to(DEV).contiguous(memory_format=cl)
    gd = g.bfloat16().to(DEV).contiguous(memory_format=cl)
    w32 = cv.conv3d_weight_grad(xd, gd, c.stride, c.padding)
    w16 = cv.conv3d_weight_grad(xd, gd, c.stride, c.padding, out_dtype=torch.bfloat16)
    assert torch.equal(w32, ref.float()), f'{c.name}: max |diff| {(w32.double() - ref).abs().max().item()}'
    assert w16.dtype == torch.bfloat16 and torch.equal(w16, ref.float().bfloat16())


def _c32_io(n, d, h, w, seed, cin=32):
    x = _ints((n, cin, d, h, w), seed)
    wt = _ints((32, cin, 3, 3, 3), seed + 1)
    ref = V.ref_conv(x.to(DEV, torch.float64), wt.to(DEV, torch.float64)).permute(0, 2, 3, 4, 1).contiguous()
    return x, wt, ref


@pytest.mark.parametrize('depth_chunk', [0, 1, 3])
def test_conv3d_k3_c32_forward_forms_exact(cv, depth_chunk):
    """every <OUT_F32, ACC_IN, STATS> form conv_c32_impl launches, ragged H / W, depth chunks 0, 1 and 3 (7 planes:
    a partial last chunk)"""
    lib = cv._capi.lib()
    n, d, h, w = 2, 7, 19, 37
    x, wt, ref = _c32_io(n, d, h, w, seed=depth_chunk + 3)
    xbuf, xaddr = _guarded_input(x.bfloat16().permute(0, 2, 3, 4, 1), 0)
    pk = cv.pack_conv3d_weights(wt.to(DEV), 0)
    acc = _ints(tuple(ref.shape), seed=5, lo=-500, hi=500).to(DEV)
    numel = ref.numel()
    st = _stream_ptr(DEV)
    splits = lib.dfm_conv3d_k3_c32_stats_splits(n, d, h, w, depth_chunk)
    for out_f32, use_acc, stats, relu in ((1, True, False, 0), (1, False, False, 0), (0, True, True, 0),
                                          (0, False, True, 0), (0, True, False, 1), (0, False, False, 0)):
        raw, out, oaddr = _guarded_output(numel, torch.float32 if out_f32 else torch.bfloat16)
        part = torch.empty((n, 32, splits, 3), dtype=torch.float32, device=DEV) if stats else None
        rc = lib.dfm_conv3d_k3_c32_fwd_strided(n, d, h, w, _vp(xaddr), 32, _ptr(pk),
                                               _ptr(acc) if use_acc else None, _vp(oaddr), out_f32, relu,
                                               depth_chunk, _ptr(part) if stats else None, st)
        assert rc == 0, lib.dfm_last_error()
        torch.cuda.synchronize()
        e = ref + acc.double() if use_acc else ref
        if relu:
            e = e.clamp_min(0)
        want = e.float() if out_f32 else e.float().bfloat16()
        assert torch.equal(out.view(ref.shape), want), (out_f32, use_acc, stats, relu)
        assert _guards_intact(raw, numel), (out_f32, use_acc, stats, relu)
    del xbuf


def test_conv3d_k3_c32_to1_and_slices_exact(cv):
    lib = cv._capi.lib()
    n, d, h, w = 1, 5, 17, 33
    x, wt, ref = _c32_io(n, d, h, w, seed=21)
    xd = x.bfloat16().to(DEV).contiguous(memory_format=torch.channels_last_3d)
    st = _stream_ptr(DEV)
    # 32 -> 1: the weight in row 0 of a zero-padded (32, 32) pack, channel 0 stored
    w1 = torch.zeros_like(wt)
    w1[0] = wt[0]
    pk1 = cv.pack_conv3d_weights(w1.to(DEV), 0)
    raw, out, oaddr = _guarded_output(n * d * h * w, torch.bfloat16)
    assert lib.dfm_conv3d_k3_c32_to1_fwd(n, d, h, w, _ptr(xd), _ptr(pk1), _vp(oaddr), 0, 0, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(out.view(n, d, h, w), ref[..., 0].float().bfloat16()) and _guards_intact(raw, n * d * h * w)
    # _fwd_slices: 32 channels written into a 64- and a 96-channel tensor, the others untouched
    pk = cv.pack_conv3d_weights(wt.to(DEV), 0)
    for C, lo in ((64, 32), (96, 32), (96, 64)):
        raw, out, base = _guarded_output(n * d * h * w * C, torch.bfloat16)
        assert lib.dfm_conv3d_k3_c32_fwd_slices(n, d, h, w, _ptr(xd), 32, _ptr(pk), _vp(base + 2 * lo), C, 0,
                                                0, st) == 0
        torch.cuda.synchronize()
        o = out.view(n, d, h, w, C)
        assert torch.equal(o[..., lo:lo + 32], ref.float().bfloat16()), (C, lo)
        others = torch.cat([o[..., :lo], o[..., lo + 32:]], -1).view(torch.int16)
        assert bool((others == SENTINEL16).all()) and _guards_intact(raw, n * d * h * w * C), (C, lo)


def _autograd_ref(fn, x, w, gy):
    x64 = x.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    y = fn(x64, w64)
    y.backward(gy.double())
    return y.detach(), x64.grad, w64.grad


def _bf16_param(module, w):
    module.weight.data = w.to(DEV, torch.bfloat16)
    return module


@pytest.mark.parametrize('cin', [32, 64])
def test_mfma_conv_32_backward_exact(cv, cin):
    """_MfmaConvFn (the 32-output kernel): forward, backward-data (a 64-channel gradient through _fwd_slices) and
    the weight gradient, ragged shape"""
    n, d, h, w = 2, 5, 18, 35
    x, wt = _ints((n, cin, d, h, w), 31 + cin), _ints((32, cin, 3, 3, 3), 32 + cin)
    gy = _ints((n, 32, d, h, w), 33 + cin)
    y64, gx64, gw64 = _autograd_ref(lambda a, b: F.conv3d(a, b, padding=1), x, wt, gy)
    m = _bf16_param(cv.MfmaConv3d(cin, 32, 3, padding=1, bias=False).to(DEV), wt)
    xd = x.bfloat16().to(DEV).contiguous(memory_format=torch.channels_last_3d).requires_grad_(True)
    assert m.eligible(xd)
    y = m(xd)
    y.backward(gy.bfloat16().to(DEV).contiguous(memory_format=torch.channels_last_3d))
    assert torch.equal(y.cpu(), y64.float().bfloat16())
    assert torch.equal(xd.grad.cpu(), gx64.float().bfloat16())
    assert torch.equal(m.weight.grad.cpu(), gw64.float().bfloat16())


def test_conv3d_to1_backward_exact(cv):
    n, d, h, w = 2, 5, 17, 35
    x, wt, gy = _ints((n, 32, d, h, w), 41), _ints((1, 32, 3, 3, 3), 42), _ints((n, 1, d, h, w), 43)
    y64, gx64, gw64 = _autograd_ref(lambda a, b: F.conv3d(a, b, padding=1), x, wt, gy)
    wd = wt.to(DEV, torch.bfloat16).requires_grad_(True)
    xd = x.bfloat16().to(DEV).contiguous(memory_format=torch.channels_last_3d).requires_grad_(True)
    y = cv._MfmaConvTo1Fn.apply(xd, wd, None)
    y.backward(gy.bfloat16().to(DEV))
    assert torch.equal(y.cpu(), y64.float().bfloat16())
    assert torch.equal(xd.grad.cpu(), gx64.float().bfloat16())
    assert torch.equal(wd.grad.cpu(), gw64.float().bfloat16())


@pytest.mark.parametrize('kind,cin,cout,size,stride,padding', [
    ('conv', 32, 64, (6, 8, 10), 1, 1),
    ('conv', 64, 32, (6, 8, 12), 2, 1),           # backward-data: transposed axes
    ('conv', 64, 64, (5, 7, 9), 2, 1),            # odd extents: the aten backward-data fallback
    ('conv', 64, 128, (4, 6, 8), (1, 1, 2), 1),
    ('conv', 32, 32, (3, 5, 4), 1, (1, 1, 0)),
    ('convT', 64, 32, (3, 4, 5), 2, 1),
])
@pytest.mark.parametrize('precision', ['bf16', 'fp32'])
def test_module_gradients_exact(cv, kind, cin, cout, size, stride, padding, precision):
    """MfmaConv3dG / MfmaConvTranspose3d: _ConvGFn in bf16 and in split precision (fp32); integer
    operands, so both are exact against float64 autograd"""
    n = 2
    x = _ints((n, cin, *size), 51 + cin)
    if kind == 'conv':
        wt = _ints((cout, cin, 3, 3, 3), 52)
        fn = lambda a, b: F.conv3d(a, b, stride=stride, padding=padding)  # noqa: E731
        m = cv.MfmaConv3dG(cin, cout, 3, stride=stride, padding=padding, bias=False)
    else:
        wt = _ints((cin, cout, 3, 3, 3), 52)
        fn = lambda a, b: F.conv_transpose3d(a, b, stride=2, padding=1, output_padding=1)  # noqa: E731
        m = cv.MfmaConvTranspose3d(cin, cout, 3, stride=2, padding=1, output_padding=1, bias=False)
    y64 = fn(x.double(), wt.double())
    gy = _ints(tuple(y64.shape), 53)
    y64, gx64, gw64 = _autograd_ref(fn, x, wt, gy)
    dt = torch.bfloat16 if precision == 'bf16' else torch.float32
    m = m.to(DEV)
    m.weight.data = wt.to(DEV, dt)
    xd = x.to(DEV, dt).contiguous(memory_format=torch.channels_last_3d).requires_grad_(True)
    if precision == 'bf16':
        assert m.eligible(xd)
    y = m(xd)
    y.backward(gy.to(DEV, dt).contiguous(memory_format=torch.channels_last_3d))
    rnd = (lambda t: t.float().bfloat16()) if precision == 'bf16' else (lambda t: t.float())  # noqa: E731
    assert torch.equal(y.cpu(), rnd(y64))
    assert torch.equal(xd.grad.cpu(), rnd(gx64))
    assert torch.equal(m.weight.grad.cpu(), rnd(gw64))


@pytest.mark.parametrize('kind,stride,size', [('conv', 1, (9, 21)), ('conv', 2, (10, 22)), ('convT', 2, (5, 11))])
@pytest.mark.parametrize('precision', ['bf16', 'fp32'])
def test_2d_module_gradients_exact(cv, kind, stride, size, precision):
    """MfmaConv2d / MfmaConvTranspose2d under autograd: _ConvGFn on depth-1 views, in bf16 and in split precision (fp32)"""
    n, cin, cout = 2, 64, 32
    x = _ints((n, cin, *size), 61)
    if kind == 'conv':
        wt = _ints((cout, cin, 3, 3), 62)
        fn = lambda a, b: F.conv2d(a, b, stride=stride, padding=1)  # noqa: E731
        m = cv.MfmaConv2d(cin, cout, 3, stride=stride, padding=1, bias=False)
    else:
        wt = _ints((cin, cout, 3, 3), 62)
        fn = lambda a, b: F.conv_transpose2d(a, b, stride=2, padding=1, output_padding=1)  # noqa: E731
        m = cv.MfmaConvTranspose2d(cin, cout, 3, stride=2, padding=1, output_padding=1, bias=False)
    gy = _ints(tuple(fn(x.double(), wt.double()).shape), 63)
    y64, gx64, gw64 = _autograd_ref(fn, x, wt, gy)
    dt = torch.bfloat16 if precision == 'bf16' else torch.float32
    m = m.to(DEV)
    m.weight.data = wt.to(DEV, dt)
    xd = x.to(DEV, dt).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    if precision == 'bf16':
        assert m.train_why_not(xd) is None
    y = m(xd)
    y.backward(gy.to(DEV, dt).contiguous(memory_format=torch.channels_last))
    rnd = (lambda t: t.float().bfloat16()) if precision == 'bf16' else (lambda t: t.float())  # noqa: E731
    assert torch.equal(y.cpu(), rnd(y64))
    assert torch.equal(xd.grad.cpu(), rnd(gx64))
    assert torch.equal(m.weight.grad.cpu(), rnd(gw64))


def test_channel_split_with_a_pass_through_consumer(cv):
    """the whole tensor's gradient handed on unchanged ((a_all + z): the same tensor is z's gradient too) must not
    be modified by the slice's gradient: x's and z's gradients equal plain autograd's, bit for bit"""
    gen = torch.Generator().manual_seed(9)
    cl = torch.channels_last_3d
    mk = lambda c: torch.randn(1, c, 4, 6, 8, generator=gen).bfloat16().to(DEV).contiguous(memory_format=cl)  # noqa: E731
    x, z0, w, v = mk(64), mk(64), mk(64), mk(32)
    grads = []
    for split in (cv.channel_split, lambda t, lo, hi: (t, t[:, lo:hi])):
        xa, z = x.clone().requires_grad_(True), z0.clone().requires_grad_(True)
        a_all, a_cur = split(xa, 0, 32)
        (((a_all + z) * w).sum() + (a_cur * v).sum()).backward()
        grads.append((xa.grad, z.grad))
    (gx, gz), (rx, rz) = grads
    assert torch.equal(gz, rz) and torch.equal(gz, w), 'z: its gradient is w, whatever the slice adds into x'
    assert torch.equal(gx, rx)
