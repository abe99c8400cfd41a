"""Every plane-sweep BACKWARD kernel but the matrix-product one (tests/test_sweep_bwd_mfma_gpu.py has that) against the
fp64 reference of tests/sweep_bwd_ref.py -- autograd of the two F.grid_sample calls of build_dfm_cost, reference
dfm_backbone.py:296-311 -- element by element, on the kernels' fp32 results (``plane_sweep_backward`` or the raw C
ABI: before autograd's cast to the maps' dtype), with the kernel that ran asserted in every test.

    scatter  sweep_bwd_kernel (csrc/plane_sweep.hip), id 1            forced, and reached by h_in < 4 / rows too wide
    tile     sweep_bwd_tile_kernel (csrc/plane_sweep_bwd.hip), id 5    dense and strided lattices, kernel 8 = prev only
    window   sweep_bwdc_kernel (csrc/plane_sweep_cl.hip)               dfm_plane_sweep_bwd_cur_nhwc; stores no id
    gather   sweep_bwd_gather_kernel (+ fit, footprint table and scatter-planes kernels,
             csrc/plane_sweep_bwd_gather.hip), id 9                    all 16 instantiations, with / without the table

The bound.  Per element |got - ref| <= (n + K) u A + abs, with u = 2^-24, A = sum_k w_k |g_k| and n the number of
taps that land on the element (both from the reference), K from the kernel's arithmetic.  The library is compiled
with -ffp-contract=off: a product and a sum are two roundings unless the source says fma.  Common to all four
kernels: the sample position is the reference's fp32 position bit for bit; the fractions fx = x - floor(x) are exact
for x >= 0 and rounded once for x in [-1, 0), where the only tap inside the map has weight fx itself; a
complement 1 - f is one rounding; a weight (row factor) * (column factor) one more: at most 3 roundings per weight.
bf16 gradient volumes are widened exactly, so bf16 cases use the same bound on the fp32 results.  Each K below is the
first-order count plus one unit for the second-order terms ((1 + u)^(n + K) - 1 <= (n + K) u (1 + 2^-13) for the
n <= 2^10 of these problems, and w_k itself is off by 3 u where A uses the exact weight).

  scatter, K = 4: weight 3, ``g * w`` 1, then n global float atomics on a zero-filled map -- the first exact, every later
      one a rounding relative to a partial sum of magnitude <= A: (n - 1) + 4 = n + 3.
  window, K = 4: weight 3, ``g * w`` 1, then a lane adds its planes' products in registers and flushes each window cell
      with one atomic: n_l - 1 roundings in the lane, m - 1 among the m flushed values, n_l + m <= n + 1: <= n + 3.
      Footprints that leave the window go to memory one atomic each: the scatter's count.
  gather, K = 4: weight 3, ``v * wgt`` 1, ``acc +=`` n_g - 1 for the n_g gathered terms of the pixel's lane; the planes the
      fit does not vouch for are added afterwards by atomics (product 1, add 1 each): n roundings of sums at most: n + 3.
  tile, K = 5 and abs = (n + 2) 2^-42 M: prev map: weight 3, ``g * (w * 2^sh)`` 1 (the scale is a power of two), then the
      value is cut to a 64-bit integer -- exact sums in LDS -- and a window's sum goes back to fp32 with one rounding
      (the fma of the two words) and to the map with one float atomic per window: 5 + (m - 1), m <= n windows: n + 4.
      cur map: the lane's planes are summed by fma first (n_l roundings, none for the product), then the same
      integer path: 3 + n_l + 1 + (m - 1) <= n + 4.  The integer path's absolute error: the scale puts the local maximum
      (of the pass's gradient values, or of the register sums: both <= M = max(max |grad volume|, max A)) in
      [2^49, 2^50), so one integer unit is <= 2^-49 M.  bwd_to_fixed truncates (< 1 unit), except that for
      -2^32 < x < 0 its low word 2^32 - |x| is rounded to fp32 first, where the spacing is 2^8: <= 2^7 units per add;
      the way back rounds the low word the same way, <= 2^7 units, and the fma's rounding is the relative one counted
      above: (n + 2) 2^7 units <= (n + 2) 2^-42 M.

Exact zeros: where no tap lands (n == 0) the result must be exactly zero -- the gather and window kernels store into /
add onto maps the caller does not clear for them; the gather's outputs are pre-filled with NaN here.

Every test prints its largest err / (u A) -- for the tile kernel (err - abs) / (u A): it cuts a product below one
integer unit to zero, so an element that receives nothing else is off by all of its A, inside ``abs`` -- and the
largest per kernel so far in the session.
"""
import ctypes
import importlib
import os
import types

import numpy as np
import pytest
import torch

from tests import sweep_bwd_ref as sr
from tests import util

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
K_SCATTER, K_WINDOW, K_GATHER, K_TILE = 4, 4, 4, 5
RATIOS = {}   # kernel label -> largest err / (u A) seen in this session


@pytest.fixture(scope='module')
def pkg():
    assert torch.cuda.is_available(), 'GPU tests need a GPU (no fallback path exists)'
    p = importlib.import_module('depth-from-motion_amd')
    assert os.path.exists(p._capi.LIB_PATH)
    return p


def _launch_mod():
    return importlib.import_module('depth-from-motion_amd._launch')


def _rc(pkg, name, *args):
    """status of a raw C-ABI call (tensors -> addresses, STREAM -> the current stream)"""
    L = _launch_mod()
    return L.call(getattr(pkg._capi.lib(), name), args)


def _last(pkg):
    return pkg._capi.lib().dfm_plane_sweep_bwd_last_kernel()


def _device_geometry(pkg, k, dtype):
    ps = pkg.plane_sweep
    dev = torch.device('cuda:0')
    maps = torch.empty(k['B'], k['C'], k['H'], k['W'], dtype=dtype, device=dev)   # (shape and dtype only)
    desc = ps._make_desc(maps, k['D'], k['fsf'], k['csf'], k['img_shape'], k['flip'], k['crop'], k['scale'])
    assert (desc.h_out, desc.w_out) == (k['h_out'], k['w_out'])
    P, Pinv, T = ps.camera_matrices(torch.from_numpy(k['P'].copy()), torch.from_numpy(k['T'].copy()), k['B'], dev,
                                    cam2img_inv=torch.from_numpy(k['Pinv'].copy()))
    depths = torch.from_numpy(k['depths'].copy()).to(dev)
    return desc, depths, P, Pinv, T


def _inputs(pkg, name, dtype):
    """one problem of tests/sweep_bwd_ref.py on the device: descriptor, camera matrices, the gradient volume in the
    reference layout (``g``) and channels-last (``g_cl``: (B, D, h, w, 2C) in memory)"""
    k = sr.problem(name)
    bf16 = dtype == BF16
    desc, depths, P, Pinv, T = _device_geometry(pkg, k, dtype)
    g = torch.from_numpy((k['gout16'] if bf16 else k['gout']).copy()).to('cuda:0').to(dtype)
    if bf16:
        assert np.array_equal(g.float().cpu().numpy(), k['gout16'])   # exact in bf16
    g_cl = g.contiguous(memory_format=torch.channels_last_3d)
    assert g.is_contiguous() and not g_cl.is_contiguous()
    return types.SimpleNamespace(k=k, name=name, bf16=bf16, desc=desc, depths=depths, P=P, Pinv=Pinv, T=T, g=g,
                                 g_cl=g_cl, geo=(depths, P, Pinv, T))


def _check(got, inp, half, K, label, tile_abs=False):
    """got (B, C, H, W) fp32 on the device (any strides) against the fp64 reference of map ``half``"""
    k, ref = inp.k, sr.reference(inp.name, inp.bf16)
    assert got.dtype == F32 and tuple(got.shape) == (k['B'], k['C'], k['H'], k['W'])
    got = got.detach().cpu().numpy().astype(np.float64)
    want, A = ref['grad'][half], ref['A'][half]
    n = ref['n'][half][:, None]                                  # (B, 1, H, W)
    assert np.isfinite(got).all(), f'{label} {inp.name}: non-finite values'
    empty = np.broadcast_to(n == 0, got.shape)
    assert not got[empty].any(), f'{label} {inp.name}: {int((got[empty] != 0).sum())} values where no tap lands'
    err = np.abs(got - want)
    absolute = np.zeros_like(A)
    if tile_abs:
        g_abs = np.abs(k['gout16'] if inp.bf16 else k['gout']).max()
        absolute = (n + 2) * 2.0 ** -42 * max(float(g_abs), float(A.max())) * np.ones_like(A)
    bound = (n + K) * sr.U * A + absolute
    m = A > 0
    # (the tile kernel cuts products below one integer unit to zero: its ratio is that of the error beyond ``abs``)
    ratio = float((np.maximum(err[m] - absolute[m], 0.0) / (sr.U * A[m])).max()) if m.any() else 0.0
    RATIOS[label] = max(RATIOS.get(label, 0.0), ratio)
    which = 'prev' if half else 'cur'
    print(f'\n{label} {inp.name} {"bf16" if inp.bf16 else "fp32"} {which}: largest err / (u A) = {ratio:.2f} '
          f'(max n {int(n.max())}, K {K}); session: ' + ', '.join(f'{a} {b:.2f}' for a, b in sorted(RATIOS.items())))
    bad = err > bound
    assert not bad.any(), (f'{label} {inp.name} {which}: {int(bad.sum())} of {bad.size} beyond (n + {K}) u A, worst '
                           f'err {float(err[bad].max()):.4g}, err / bound {float((err[bad] / bound[bad]).max()):.3g} '
                           f'at {np.unravel_index(int(np.argmax(np.where(bad, err, 0))), err.shape)}')


def _forget_kernel_id(pkg, expected):
    """the library remembers the LAST backward kernel: make sure a stale ``expected`` cannot satisfy the next assertion"""
    if _last(pkg) != expected:
        return
    other = 1 if expected != 1 else 5
    inp = _inputs(pkg, 'tiny_dense-plain', F32)
    with pkg.plane_sweep.backward_kernel(other):
        pkg.plane_sweep.plane_sweep_backward(inp.desc, inp.g, *inp.geo)
    assert _last(pkg) == other


def _backward(pkg, inp, expected, kernel=None, grad=None):
    """plane_sweep_backward, the id the library reports asserted"""
    ps = pkg.plane_sweep
    _forget_kernel_id(pkg, expected)
    with ps.backward_kernel(kernel):
        gc, gp = ps.plane_sweep_backward(inp.desc, inp.g if grad is None else grad, *inp.geo)
    torch.cuda.synchronize()
    assert _last(pkg) == expected, f'kernel {_last(pkg)} took {inp.name}, not {expected}'
    return gc, gp


def _tile_plan(W, D):
    """(channels per pass, slab rows) of sweep_bwd_impl (csrc/plane_sweep_bwd.hip) for maps W wide, D planes"""
    planes = max(1, min(32, (D + 3) // 4))
    budget = 160 * 1024 - 1024 - planes * 256 * 12
    cw = 4
    while cw > 2 and budget // (cw * W * 8) < 4:
        cw >>= 1
    return cw, budget // (cw * W * 8)


# ---- scatter kernel, id 1 --------------------------------------------------------------------------------
_TINY = [f'tiny_dense-{g}' for g in ('plain', 'aug', 'batch2', 'forward', 'zplane', 'outside')] + \
        [f'tiny_strided-{g}' for g in ('plain', 'aug', 'batch2', 'forward', 'zplane', 'outside')] + ['tiny_csf8-scale103']


@pytest.mark.parametrize('name,dtype', [(n, F32) for n in _TINY] +
                         [(n, BF16) for n in ('tiny_dense-aug', 'tiny_strided-plain', 'tiny_csf8-scale103')],
                         ids=lambda v: v if isinstance(v, str) else str(v).split('.')[-1])
def test_scatter_kernel_forced(pkg, name, dtype):
    inp = _inputs(pkg, name, dtype)
    gc, gp = _backward(pkg, inp, 1, kernel=1)
    _check(gc, inp, 0, K_SCATTER, 'scatter')
    _check(gp, inp, 1, K_SCATTER, 'scatter')


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('name', ['rows3-lateral', 'wide2560-lateral'])
def test_scatter_kernel_reached_without_an_override(pkg, name, dtype):
    """h_in = 3 (no slab of four rows) and four rows of 2560 pixels (beyond the LDS budget at two channels per
    pass): the default dispatch falls back to the scatter kernel"""
    inp = _inputs(pkg, name, dtype)
    assert inp.k['H'] < 4 or _tile_plan(inp.k['W'], inp.k['D'])[1] < 4
    gc, gp = _backward(pkg, inp, 1)
    _check(gc, inp, 0, K_SCATTER, 'scatter')
    _check(gp, inp, 1, K_SCATTER, 'scatter')


# ---- tile kernel, id 5 ------------------------------------------------------------------------------------
_DENSE = [f'dense-{g}' for g in ('plain', 'aug', 'batch2', 'forward', 'zplane', 'outside')] + \
         ['deep33-plain', 'deep33-aug', 'wide1280-lateral', 'wide1280-aug']


@pytest.mark.parametrize('name,dtype', [(n, F32) for n in _DENSE] +
                         [(n, BF16) for n in ('dense-aug', 'deep33-aug', 'wide1280-aug')],
                         ids=lambda v: v if isinstance(v, str) else str(v).split('.')[-1])
def test_tile_kernel_dense_lattice(pkg, name, dtype):
    """row_tiles = 0: bands are runs of 256 points of the flat lattice (1403 points: a partial last band), 33
    planes in chunks of 9 with a partial last one, four channels per pass and two (1280-wide rows).  fp32 takes the
    tile kernel by default; bf16 would take the matrix-product kernel, so it is pinned"""
    inp = _inputs(pkg, name, dtype)
    cw, rows = _tile_plan(inp.k['W'], inp.k['D'])
    assert rows >= 4 and cw == (2 if inp.k['W'] == 1280 else 4)
    gc, gp = _backward(pkg, inp, 5, kernel=5 if dtype == BF16 else None)
    assert gc.is_contiguous() and gp.is_contiguous()
    _check(gc, inp, 0, K_TILE, 'tile', tile_abs=True)
    _check(gp, inp, 1, K_TILE, 'tile', tile_abs=True)


_STRIDED = [f'strided8-{g}' for g in ('plain', 'aug', 'batch2', 'forward', 'zplane', 'outside')] + \
           ['strided8_csf8-scale103', 'wide1280_csf4-aug']


@pytest.mark.parametrize('name,dtype', [(n, F32) for n in _STRIDED] +
                         [(n, BF16) for n in ('strided8-aug', 'strided8_csf8-scale103')],
                         ids=lambda v: v if isinstance(v, str) else str(v).split('.')[-1])
def test_tile_kernel_strided_lattice(pkg, name, dtype):
    """row_tiles > 0: no band crosses a lattice row (two bands per row at w_out = 320, there with two channels per pass)"""
    inp = _inputs(pkg, name, dtype)
    assert inp.k['csf'] >= 2
    gc, gp = _backward(pkg, inp, 5, kernel=5)
    _check(gc, inp, 0, K_TILE, 'tile', tile_abs=True)
    _check(gp, inp, 1, K_TILE, 'tile', tile_abs=True)


@pytest.mark.parametrize('name,dtype', [('strided8-aug', F32), ('strided8-aug', BF16), ('dense-batch2', F32)],
                         ids=lambda v: v if isinstance(v, str) else str(v).split('.')[-1])
def test_tile_kernel_prev_map_only(pkg, name, dtype):
    """``kernel = 8``: the prev map alone, the cur map's buffer untouched"""
    ps, L = pkg.plane_sweep, _launch_mod()
    inp = _inputs(pkg, name, dtype)
    k = inp.k
    g_cur = torch.full((k['B'], k['C'], k['H'], k['W']), 7.0, device='cuda:0')
    g_prev = torch.zeros_like(g_cur)
    _forget_kernel_id(pkg, 5)
    assert _rc(pkg, 'dfm_plane_sweep_bwd_opts', inp.desc, inp.g, *inp.geo, g_cur, g_prev, L.STREAM,
               ps.make_opts(kernel=8)) == 0
    torch.cuda.synchronize()
    assert _last(pkg) == 5
    assert bool((g_cur == 7.0).all())
    _check(g_prev, inp, 1, K_TILE, 'tile', tile_abs=True)


@pytest.mark.parametrize('name,dtype,in_place', [('strided8-aug', F32, False), ('strided8-aug', F32, True),
                                                 ('strided8-aug', BF16, False), ('strided8-aug', BF16, True),
                                                 ('dense8-aug', F32, False), ('dense8-aug', F32, True),
                                                 ('dense8-aug', BF16, True)],
                         ids=lambda v: v if isinstance(v, str) else ('in_place' if v is True else 'workspace' if v is False
                                                                     else str(v).split('.')[-1]))
def test_tile_kernel_channels_last_gradient(pkg, name, dtype, in_place):
    """dfm_plane_sweep_bwd_channels_last: the (B, D, h, w, 2C) volume re-laid into a workspace by the library's
    transpose, or read where it lies (no workspace).  (A dense bf16 volume WITH a workspace goes to the matrix-product
    kernel: not this file's.)"""
    L = _launch_mod()
    inp = _inputs(pkg, name, dtype)
    k = inp.k
    nbytes = inp.g_cl.numel() * inp.g_cl.element_size()
    vec = 16 // inp.g_cl.element_size()
    assert (2 * k['C']) % vec == 0 and (k['D'] * k['h_out'] * k['w_out']) % vec == 0   # else the workspace is ignored
    ws = None if in_place else torch.empty(nbytes, dtype=torch.uint8, device='cuda:0')
    g_cur = torch.zeros((k['B'], k['C'], k['H'], k['W']), device='cuda:0')
    g_prev = torch.zeros_like(g_cur)
    _forget_kernel_id(pkg, 5)
    assert _rc(pkg, 'dfm_plane_sweep_bwd_channels_last', inp.desc, inp.g_cl, *inp.geo, g_cur, g_prev, ws,
               0 if in_place else nbytes, L.STREAM) == 0
    torch.cuda.synchronize()
    assert _last(pkg) == 5
    _check(g_cur, inp, 0, K_TILE, 'tile', tile_abs=True)
    _check(g_prev, inp, 1, K_TILE, 'tile', tile_abs=True)


# ---- cur window kernel (dfm_plane_sweep_bwd_cur_nhwc; stores no id: the raw call is the proof) ---------------
_WINDOW = [f'k32-{g}' for g in ('plain', 'aug', 'batch2', 'forward', 'zplane', 'outside')] + \
          ['k32_csf8-scale103', 'k32_csf2-plain', 'k32_csf2-aug', 'k64_csf2-aug', 'k32_partial-plain', 'k64_csf8-scale103',
           'k64_partial_csf2-aug']


@pytest.mark.parametrize('name', _WINDOW)
def test_window_kernel_raw_call(pkg, name):
    L = _launch_mod()
    inp = _inputs(pkg, name, F32)
    k = inp.k
    if 'partial' in name or name == 'k64_csf8-scale103':
        assert (k['h_out'], k['w_out']) == (5, 16) and (k['h_out'] * k['w_out'] // 16) % 4 == 1   # a partial workgroup
    g_cur = torch.zeros((k['B'], k['H'], k['W'], k['C']), device='cuda:0')     # pixel-major
    assert _rc(pkg, 'dfm_plane_sweep_bwd_cur_nhwc', inp.desc, inp.g, *inp.geo, g_cur, L.STREAM) == 0
    torch.cuda.synchronize()
    _check(g_cur.permute(0, 3, 1, 2), inp, 0, K_WINDOW, 'window')


@pytest.mark.parametrize('name', ['k32-plain', 'k32-aug', 'k32_csf2-aug', 'k64_csf8-scale103'])
def test_default_dispatch_of_a_strided_fp32_sweep(pkg, name):
    """plane_sweep_backward on a reference-layout fp32 volume: the cur map from the window kernel (returned
    channels-last: only that kernel writes a pixel-major map here), the prev map from the gather kernel (id 9)"""
    inp = _inputs(pkg, name, F32)
    gc, gp = _backward(pkg, inp, 9)
    assert gc.is_contiguous(memory_format=torch.channels_last) and not gc.is_contiguous() and gp.is_contiguous()
    _check(gc, inp, 0, K_WINDOW, 'window')
    _check(gp, inp, 1, K_GATHER, 'gather')


def test_default_dispatch_without_the_gather_kernel(pkg):
    """``prev_gather(False)``: the window kernel for the cur map, the tile kernel (kernel 8) for the prev map"""
    inp = _inputs(pkg, 'k32-aug', F32)
    with pkg.plane_sweep.prev_gather(False):
        gc, gp = _backward(pkg, inp, 5)
    assert gc.is_contiguous(memory_format=torch.channels_last) and not gc.is_contiguous() and gp.is_contiguous()
    _check(gc, inp, 0, K_WINDOW, 'window')
    _check(gp, inp, 1, K_TILE, 'tile', tile_abs=True)


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['fp32', 'bf16'])
def test_default_dispatch_of_a_channels_last_gradient(pkg, dtype):
    """the NDHWC stack's gradient: both maps by the gather kernel, read where the volume lies, written pixel-major"""
    inp = _inputs(pkg, 'k32-batch2', dtype)
    gc, gp = _backward(pkg, inp, 9, grad=inp.g_cl)
    for t in (gc, gp):
        assert t.is_contiguous(memory_format=torch.channels_last) and not t.is_contiguous()
    _check(gc, inp, 0, K_GATHER, 'gather')
    _check(gp, inp, 1, K_GATHER, 'gather')


# ---- gather kernel, id 9 ------------------------------------------------------------------------------------
def _gather(pkg, inp, half, cl_in, cl_out, table):
    """raw dfm_plane_sweep_bwd_gather into a NaN-filled map -> ((B, C, H, W) view of the map, the planes' ``ok`` flags)"""
    L = _launch_mod()
    k = inp.k
    lib = pkg._capi.lib()
    full = int(lib.dfm_plane_sweep_bwd_prev_gather_workspace_bytes(ctypes.byref(inp.desc)))
    records = (k['B'] * k['D'] * 12 * 4 + 255) & ~255      # the plane records alone: no footprint table
    assert full >= records + k['B'] * k['D'] * k['h_out'] * k['w_out'] * 12
    nbytes = full if table else records
    ws = torch.zeros(nbytes, dtype=torch.uint8, device='cuda:0')
    shape = (k['B'], k['H'], k['W'], k['C']) if cl_out else (k['B'], k['C'], k['H'], k['W'])
    out = torch.full(shape, float('nan'), device='cuda:0')
    _forget_kernel_id(pkg, 9)
    rc = _rc(pkg, 'dfm_plane_sweep_bwd_gather', inp.desc, half, inp.g_cl if cl_in else inp.g, int(cl_in), *inp.geo, out,
             int(cl_out), ws, nbytes, L.STREAM)
    assert rc == 0
    torch.cuda.synchronize()
    assert _last(pkg) == 9
    ok = ws[:k['B'] * k['D'] * 48].view(torch.float32).view(-1, 12)[:, 9].cpu().numpy()
    return (out.permute(0, 3, 1, 2) if cl_out else out), ok


@pytest.mark.parametrize('table', [True, False], ids=['table', 'records_only'])
@pytest.mark.parametrize('cl_out', [False, True], ids=['map_planar', 'map_pixel_major'])
@pytest.mark.parametrize('cl_in', [False, True], ids=['grad_planar', 'grad_channels_last'])
@pytest.mark.parametrize('dtype', [F32, BF16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('half', [0, 1], ids=['cur', 'prev'])
def test_gather_kernel_every_instantiation(pkg, half, dtype, cl_in, cl_out, table):
    """half x dtype x gradient layout x map layout, each with the footprint table and with a workspace of the
    plane records alone (the kernel then projects every candidate itself); flip + crop + scale"""
    inp = _inputs(pkg, 'k32-aug', dtype)
    got, ok = _gather(pkg, inp, half, cl_in, cl_out, table)
    _check(got, inp, half, K_GATHER, 'gather')


_GATHER = ['k32-plain', 'k32-batch2', 'k32-forward', 'k32-zplane', 'k32-outside', 'k32_csf8-scale103', 'k32_csf2-plain',
           'k32_csf2-aug', 'k64_csf2-aug', 'k64_csf8-scale103', 'k32_partial-plain', 'k64_partial_csf2-aug']


@pytest.mark.parametrize('table', [True, False], ids=['table', 'records_only'])
@pytest.mark.parametrize('name', _GATHER)
def test_gather_kernel_geometries(pkg, name, table):
    inp = _inputs(pkg, name, F32)
    for half in (0, 1):
        got, ok = _gather(pkg, inp, half, False, False, table)
        if half == 1 and inp.k['geom'] == 'zplane':
            # the plane at z = 0 (non-finite positions) is not vouched for: the scatter-planes kernel has it, and
            # whatever else the fit declines (the mirrored plane behind the camera, if it does)
            assert (ok.reshape(inp.k['B'], -1)[:, 1] == 0).all()
        if inp.k['geom'] == 'plain' and inp.k['csf'] == 4:
            assert (ok == 1).all()
        _check(got, inp, half, K_GATHER, 'gather')


def test_gather_kernel_is_deterministic(pkg):
    """every plane gathered: a lane owns a pixel and adds plane by plane -- two runs give the same bits"""
    inp = _inputs(pkg, 'k32-plain', F32)
    for half in (0, 1):
        a, ok = _gather(pkg, inp, half, False, False, True)
        b, _ = _gather(pkg, inp, half, False, False, True)
        assert (ok == 1).all()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- shapes the entry points decline: DFM_ERR_UNSUPPORTED, the output untouched --------------------------------
def _plain(pkg, B, C, H, W, D, csf, dtype):
    k = dict(B=B, C=C, H=H, W=W, D=D, fsf=1, csf=csf, img_shape=sr.IMG_SHAPE, flip=False, crop=(0, 0), scale=1.0,
             h_out=round(H / csf), w_out=round(W / csf), P=util.KITTI_P2[None].repeat(B, 0), T=util.random_poses(B),
             depths=util.depth_planes(D))
    k['Pinv'] = util.host_inverse(k['P'])
    desc, depths, P, Pinv, T = _device_geometry(pkg, k, dtype)
    g = torch.ones((B, 2 * C, D, k['h_out'], k['w_out']), dtype=dtype, device='cuda:0')
    return types.SimpleNamespace(k=k, desc=desc, g=g, geo=(depths, P, Pinv, T))


@pytest.mark.parametrize('what,C,H,W,csf', [('c24', 24, 16, 64, 4), ('dense', 32, 8, 32, 1), ('lattice_1x1', 32, 4, 4, 4)])
def test_gather_kernel_declines(pkg, what, C, H, W, csf):
    L = _launch_mod()
    inp = _plain(pkg, 1, C, H, W, 3, csf, F32)
    if what == 'lattice_1x1':
        assert (inp.k['h_out'], inp.k['w_out']) == (1, 1)
    out = torch.full((1, C, H, W), 7.0, device='cuda:0')
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device='cuda:0')
    for half in (0, 1):
        rc = _rc(pkg, 'dfm_plane_sweep_bwd_gather', inp.desc, half, inp.g, 0, *inp.geo, out, 0, ws, ws.numel(), L.STREAM)
        assert rc == pkg._capi.DFM_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def test_window_kernel_declines_bf16(pkg):
    L = _launch_mod()
    inp = _plain(pkg, 1, 32, 16, 64, 3, 4, BF16)
    out = torch.full((1, 16, 64, 32), 7.0, device='cuda:0')
    rc = _rc(pkg, 'dfm_plane_sweep_bwd_cur_nhwc', inp.desc, inp.g, *inp.geo, out, L.STREAM)
    assert rc == pkg._capi.DFM_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
