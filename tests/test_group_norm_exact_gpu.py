"""The GroupNorm kernels (csrc/group_norm.hip) against the fp64 reference of tests/gn_ref.py at the shapes where their
code takes another path: the channels-last lane maps at their ends (one 16-byte vector block, 64 of them, group borders
inside a lane's vector, one group of 256 channels), slices at their ends (shorter than one step, the unroll boundaries,
an empty last slice, more than 256 partials, the 2048 cap, a backward whose two passes cut the tensor differently), a
large common offset and an outlier at the head of a slice in the shifted sums, the planar kernels off their vector
alignment, and the host dispatch of group_norm() for residuals the kernels do not fuse.

The kernel-level tests call the C ABI with their OWN workspace (filled with NaN first), so they can read the statistics
partials, and check the passes apart: mean / rstd against fp64 moments of the exact inputs, y elementwise against the
fp64 value built from the kernel's own mean / rstd, the backward against the fp64 formula with the kernel's own mean /
rstd and the mask of the kernel's own y.  Every bound is tests/gn_ref.py's: number formats, the fp64 reference and
operation counts read from the kernel source; tests/test_gn_ref.py shows on the CPU that torch's fp32 GroupNorm meets
them and that three one-slice / one-vector mutations do not.

Largest error / bound per checker, measured on an MI355X over every case of this file (1.0 is the bar):

    checker                          channels-last       planar              through group_norm()
                                     fp32      bf16      fp32      bf16      (fp32 / bf16, or the larger)
    mean, rstd (the larger)          0.337     0.304     0.014     0.013     0.014
    y                                0.873     1.000     0.551     1.000     0.431 / 1.000
    y behind torch's own + residual    --        --        --        --      0.920 / 1.000
    dbeta ('grid' inputs: exact)     0.127     0.005     0.070     0.000     0.148
    dgamma                           0.143     0.143     0.058     0.057     0.154
    dx                               0.349     1.000     0.176     0.999     0.207 / 1.000
    dres of a broadcast residual       --        --        --        --      0.998

The bf16 figures of y, dx and the broadcast dres sit at 1.000 by construction: half a bf16 ulp is the largest term of
their bound, and round-to-nearest moves some element of a million by just that.  What the arithmetic adds shows in the
fp32 columns.  Every partial count, every 'grid' dbeta and every residual gradient of the residual's own shape was
exact.

One figure was above 1 when first measured and is a finding, not a corrected count: y of the planar fp32 kernel, 3.9
(12.3 through group_norm() at C = 24).  gn_apply_kernel formed b = beta - mean * a with the product rounded on its
own and y = x * a + b likewise: four roundings, one of them 2^-24 |mean a|, a magnitude the bound 3 * 2^-24 (|x a| +
|b| + |res|) does not list; where beta and mean * a cancel it is more than |x a| + |b| is worth.  The kernel now uses
the channels-last kernel's two fused operations (b = fma(-mean, a, beta), y = fma(x, a, b)): 0.551.

No chain count had to be corrected after a measurement.  Two were wrong before one: the variance bound first left out
what the partial means' own rounding errors (n_abs roundings of a number as large as the data) carry into the second
moment through the merges -- 16 Dm E + 8 E^2 in gn_ref.stats_bounds, derived there; torch's fp32 CPU GroupNorm showed
it on the CPU at offset 1000 (its rstd is off by 5e-4 there, thousands of ulp; its mean stays within 2 ulp).  And
ATen's CPU backward forms dgamma from raw sums, rstd (sum g x - mean sum g): it is held to its own magnitudes
(raw_sums), the HIP kernels to sum |g xhat| as stated.
"""
import importlib

import pytest
import torch
import torch.nn.functional as F

from tests import gn_ref as G

gpu = pytest.mark.gpu
F64 = torch.float64
TDT = {'fp32': torch.float32, 'bf16': torch.bfloat16}


@pytest.fixture(scope='module')
def gn():
    return importlib.import_module('depth-from-motion_amd.group_norm')


@pytest.fixture(scope='module')
def rt():
    """(launch module, library)"""
    L = importlib.import_module('depth-from-motion_amd._launch')
    return L, importlib.import_module('depth-from-motion_amd._capi').lib()


def _workspace(lib, N, C, S, groups):
    nbytes = lib.dfm_group_norm_workspace_bytes(N, C, S, groups)
    assert nbytes > 0 and nbytes % 4 == 0
    return torch.full((nbytes // 4,), float('nan'), dtype=torch.float32, device='cuda'), nbytes


def _dev(inp):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in inp.items()}


# --------------------------------------------------------------------------------------------------------------------
# channels-last kernels through the C ABI
# --------------------------------------------------------------------------------------------------------------------
_CL = G.cl_params()


@gpu
@pytest.mark.parametrize('name,dt,mode,kind', _CL, ids=['-'.join(p) for p in _CL])
def test_channels_last_kernels(rt, name, dt, mode, kind):
    L, lib = rt
    N, C, groups, S, vec, inp = G.cl_case(name, dt, kind)
    relu, with_res = G.MODES[mode]
    bf16, cpg = dt == 'bf16', C // groups
    inp = _dev(inp)
    nsc = lambda t: t.reshape(N, C, S).permute(0, 2, 1).contiguous().to(TDT[dt])      # noqa: E731  (N, S, C) memory
    logical = lambda t: t.permute(0, 2, 1)                                             # noqa: E731  (N, C, S) view
    x, dy, res = nsc(inp['x']), nsc(inp['dy']), (nsc(inp['res']) if with_res else None)
    gamma, beta = inp['gamma'], inp['beta']
    ws, nbytes = _workspace(lib, N, C, S, groups)
    y = torch.full_like(x, float('nan'))
    mean = torch.full((N, groups), float('nan'), device='cuda')
    rstd = torch.full_like(mean, float('nan'))
    L.launch('dfm_group_norm_fwd_channels_last_res', N, C, S, groups, inp['eps'], L.DTYPES[TDT[dt]], int(relu), x,
             gamma, beta, res, y, mean, rstd, ws, nbytes, L.STREAM)
    splits = G.cl_splits(S, C)
    slices = G.cl_slices(S, splits)
    partials = ws[:N * groups * splits * 3].view(N, groups, splits, 3).clone()
    empty = G.check_partial_counts(partials, slices, cpg)
    assert empty == sum(lo == hi for lo, hi in slices) and (empty == 1 or not name.endswith('S4481'))
    x64 = G.ncs(inp['x'])
    got = dict(y=logical(y), mean=mean, rstd=rstd)
    kw = dict(dev='cuda', Dm=G.partial_mean_dev_cl(x64, groups, slices))
    chain = G.chain_cl(S, C, groups, vec)
    ratios = G.check_all(inp, groups, relu, with_res, bf16, got, chain, None, backward_too=False, **kw)
    if CL_BACKWARD[name]:
        mask = (logical(y).reshape(N, C, S) > 0).to(F64) if relu else torch.ones(N, C, S, dtype=F64, device='cuda')
        cb = G.chain_bwd_cl(S, C, vec, N)
        variants = ('y', 'x') if (relu and not with_res) else ('y',)
        outs = {}
        for v in variants:
            ws.fill_(float('nan'))
            gx = torch.full_like(x, float('nan'))
            gres = torch.full_like(x, float('nan')) if (relu and with_res) else None
            gw, gb = (torch.full((C,), float('nan'), device='cuda') for _ in range(2))
            if v == 'x':   # the mask recomputed from x (what group_norm() takes with _XMASK)
                L.launch('dfm_group_norm_bwd_channels_last_xmask', N, C, S, groups, L.DTYPES[TDT[dt]], dy, x, mean,
                         rstd, gamma, beta, gx, gw, gb, ws, nbytes, L.STREAM)
            else:
                L.launch('dfm_group_norm_bwd_channels_last', N, C, S, groups, L.DTYPES[TDT[dt]], int(relu), dy, x,
                         y if relu else None, mean, rstd, gamma, gx, gres, gw, gb, ws, nbytes, L.STREAM)
            outs[v] = dict(dx=logical(gx), dgamma=gw, dbeta=gb, dres=None if gres is None else logical(gres))
            ratios.update(G.check_backward(x64, G.ncs(inp['dy']), mask, gamma, groups, mean, rstd, outs[v], cb, bf16,
                                           exact_dbeta=kind == 'grid'))
        if len(outs) == 2:   # the same sums in the same order: bit-identical
            for k in ('dx', 'dgamma', 'dbeta'):
                assert torch.equal(outs['y'][k], outs['x'][k]), k
    print('ratios', name, dt, mode, kind, {k: round(v, 4) for k, v in ratios.items()})


CL_BACKWARD = {name: c['backward'] for name, c in G.CL_CASES.items()}


# --------------------------------------------------------------------------------------------------------------------
# planar kernels through the C ABI
# --------------------------------------------------------------------------------------------------------------------
_PL = G.planar_params()


@gpu
@pytest.mark.parametrize('name,dt,mode,kind', _PL, ids=['-'.join(p) for p in _PL])
def test_planar_kernels(rt, name, dt, mode, kind):
    L, lib = rt
    N, C, groups, S, vec, inp = G.planar_case(name, dt, kind)
    relu, _ = G.MODES[mode]
    bf16, cpg = dt == 'bf16', C // groups
    inp = _dev(inp)
    x, dy = inp['x'].to(TDT[dt]), inp['dy'].to(TDT[dt])
    gamma, beta = inp['gamma'], inp['beta']
    ws, nbytes = _workspace(lib, N, C, S, groups)
    y = torch.full_like(x, float('nan'))
    mean = torch.full((N, groups), float('nan'), device='cuda')
    rstd = torch.full_like(mean, float('nan'))
    L.launch('dfm_group_norm_fwd', N, C, S, groups, inp['eps'], L.DTYPES[TDT[dt]], int(relu), x, gamma, beta, y, mean,
             rstd, ws, nbytes, L.STREAM)
    Lg = cpg * S
    splits = G.planar_splits(Lg)
    partials = ws[:N * groups * splits * 3].view(N, groups, splits, 3).clone()
    G.check_partial_counts(partials, G.planar_slices(Lg, splits, vec), 1)
    got = dict(y=y, mean=mean, rstd=rstd)
    ratios = G.check_all(inp, groups, relu, False, bf16, got, G.chain_planar(Lg, vec), None, backward_too=False,
                         dev='cuda')
    ws.fill_(float('nan'))
    gx = torch.full_like(x, float('nan'))
    gw, gb = torch.zeros(C, device='cuda'), torch.zeros(C, device='cuda')     # (added to atomically)
    L.launch('dfm_group_norm_bwd', N, C, S, groups, L.DTYPES[TDT[dt]], int(relu), dy, x, y if relu else None, mean,
             rstd, gamma, gx, gw, gb, ws, nbytes, L.STREAM)
    mask = (y > 0).to(F64) if relu else torch.ones(N, C, S, dtype=F64, device='cuda')
    ratios.update(G.check_backward(G.ncs(inp['x']), G.ncs(inp['dy']), mask, gamma, groups, mean, rstd,
                                   dict(dx=gx, dgamma=gw, dbeta=gb), G.chain_bwd_planar(S, N), bf16,
                                   exact_dbeta=kind == 'grid', tag='-planar'))
    print('ratios', name, dt, mode, kind, {k: round(v, 4) for k, v in ratios.items()})


# --------------------------------------------------------------------------------------------------------------------
# host dispatch: group_norm() / HipGroupNorm
# --------------------------------------------------------------------------------------------------------------------
def _fmt(sp):
    return torch.channels_last_3d if len(sp) == 3 else torch.channels_last


def _saved_stats(out, N, groups):
    """(mean, rstd) (N, G) fp32 the autograd node keeps"""
    mean, rstd = out.grad_fn.saved_tensors[2:4]      # (x, y or x, mean, rstd, gamma, beta)
    assert mean.dtype == rstd.dtype == torch.float32 and mean.numel() == rstd.numel() == N * groups
    return mean.view(N, groups), rstd.view(N, groups)


@gpu
@pytest.mark.parametrize('mode,xmask', [('plain', True), ('relu', True), ('relu', False), ('relures', True)],
                         ids=['plain', 'relu-xmask', 'relu-ymask', 'relu-fused-residual'])
@pytest.mark.parametrize('dt', ['fp32', 'bf16'])
@pytest.mark.parametrize('N,C,sp,groups', [(2, 32, (9, 7, 13), 32), (3, 16, (6, 10), 4), (1, 64, (5, 9, 16), 32),
                                           (2, 8, (3, 1, 5), 1)])
def test_group_norm_through_the_module_switch(gn, monkeypatch, N, C, sp, groups, dt, mode, xmask):
    """4-D and 5-D channels-last tensors through group_norm(): no ReLU, the ReLU mask recomputed from x (_XMASK) or
    read from the kept output, a fused residual -- every checker on every path, and the output stays channels-last"""
    monkeypatch.setattr(gn, '_XMASK', xmask)
    relu, with_res = G.MODES[mode]
    S, vec, bf16 = int(torch.tensor(sp).prod()), 4 if dt == 'fp32' else 8, dt == 'bf16'
    inp = _dev(G.make_inputs(N, C, sp, 'random', 40 + N + C, bf16))
    x = inp['x'].to(TDT[dt]).contiguous(memory_format=_fmt(sp)).requires_grad_(True)
    r = inp['res'].to(TDT[dt]).contiguous(memory_format=_fmt(sp)).requires_grad_(True) if with_res else None
    w, b = inp['gamma'].clone().requires_grad_(True), inp['beta'].clone().requires_grad_(True)
    out = gn.group_norm(x, groups, w, b, inp['eps'], relu, residual=r)
    assert out.dtype == x.dtype and out.is_contiguous(memory_format=_fmt(sp))
    kept = any(t.data_ptr() == out.data_ptr() for t in out.grad_fn.saved_tensors)
    assert kept == (relu and not (xmask and not with_res)), 'the recomputing backward keeps no output tensor'
    mean, rstd = _saved_stats(out, N, groups)
    out.backward(inp['dy'].to(TDT[dt]).contiguous(memory_format=_fmt(sp)))
    got = dict(y=out.detach(), mean=mean, rstd=rstd, dx=x.grad, dgamma=w.grad, dbeta=b.grad,
               dres=r.grad if with_res else None)
    slices = G.cl_slices(S, G.cl_splits(S, C))
    G.check_all(inp, groups, relu, with_res, bf16, got, G.chain_cl(S, C, groups, vec), G.chain_bwd_cl(S, C, vec, N),
                dev='cuda', Dm=G.partial_mean_dev_cl(G.ncs(inp['x']), groups, slices))


def _unfused_case(gn, N, C, sp, groups, dt, x_layout, r_kind, relu):
    """relu?(gn(x) + r) through group_norm() with a residual the kernels do not fuse, against the fp64 formulas with the
    kernel's own statistics.  Returns nothing; asserts."""
    xdt, bf16 = TDT[dt], dt == 'bf16'
    S, vec = int(torch.tensor(sp).prod()), 4 if dt == 'fp32' else 8
    inp = _dev(G.make_inputs(N, C, sp, 'random', 90 + N + C + len(r_kind), bf16))
    fmt = _fmt(sp) if x_layout == 'cl' else torch.contiguous_format
    x = inp['x'].to(xdt).contiguous(memory_format=fmt).requires_grad_(True)
    if r_kind == 'contiguous':      # x's dtype, NC(D)HW memory
        r = inp['res'].to(xdt).contiguous()
    elif r_kind == 'fp32':          # full fp32 significands: y = y_gn + r promotes a bf16 y_gn
        r = torch.randn(inp['res'].shape, generator=torch.Generator().manual_seed(5)).cuda().contiguous(memory_format=fmt)
    else:                           # broadcast over the spatial extent
        r = inp['res'].reshape(N, C, -1)[:, :, :1].reshape((N, C) + (1,) * len(sp)).to(xdt).contiguous()
    r = r.requires_grad_(True)
    w, b = inp['gamma'].clone().requires_grad_(True), inp['beta'].clone().requires_grad_(True)
    out = gn.group_norm(x, groups, w, b, inp['eps'], relu, residual=r)
    # dtype and layout: what torch's unfused ops give for a GroupNorm output of x's dtype and layout
    with torch.no_grad():
        probe = torch.empty_like(x) + r
    assert out.dtype == probe.dtype and out.shape == probe.shape and out.stride() == probe.stride()
    assert out.dtype == torch.promote_types(xdt, r.dtype)
    mean, rstd = _saved_stats(out, N, groups)
    x64, r64, gamma, beta = G.ncs(inp['x']), G.ncs(r.detach().expand(x.shape)), inp['gamma'], inp['beta']
    eligible = x_layout == 'cl'
    if eligible:
        chain, cb = G.chain_cl(S, C, groups, vec), G.chain_bwd_cl(S, C, vec, N)
        Dm = G.partial_mean_dev_cl(x64, groups, G.cl_slices(S, G.cl_splits(S, C)))
    else:
        chain, cb, Dm = G.chain_planar(C // groups * S, vec), G.chain_bwd_planar(S, N), None
    G.check_stats(x64, groups, inp['eps'], mean, rstd, chain, Dm, tag='-dispatch')
    # y: the kernel's GroupNorm in x's dtype (3 U of its magnitudes, half a bf16 ulp in bf16), then torch's addition in
    # the promoted dtype (one more rounding of the sum)
    pre, mag = G.apply(x64, mean, rstd, gamma, beta)
    bound = 3 * G.U * mag + (0.5 * G.ulp_bf16(pre.abs() + 3 * G.U * mag) if bf16 else 0.0)
    total = pre + r64
    bound = bound + (0.5 * G.ulp_bf16(total.abs() + bound) if out.dtype == torch.bfloat16 else G.U * (total.abs() + bound))
    want = total.clamp_min(0) if relu else total
    y64 = G.ncs(out)
    G._ratio('y-unfused-' + dt, (y64 - want).abs(), bound)
    if relu:
        assert bool(((y64 > 0) == (total > 0))[total.abs() > bound].all())
    # gradients.  Where y was promoted (bf16 x, fp32 residual) dy has full fp32 significands: the residual's gradient
    # is dy behind the mask as it came in, the GroupNorm's sees it rounded to x's dtype (as behind torch's own cast)
    dy = inp['dy'] if out.dtype == xdt else torch.randn(x.shape, generator=torch.Generator().manual_seed(6)).cuda()
    dy = dy.to(out.dtype).contiguous(memory_format=fmt)
    out.backward(dy)
    mask = (y64 > 0).to(F64) if relu else torch.ones_like(y64)
    g64 = G.ncs(dy) * mask
    assert r.grad.dtype == r.dtype and r.grad.shape == r.shape
    if r_kind == 'broadcast':       # torch's sum over the extent, then one rounding to the residual's dtype
        sums, mags = g64.sum(2), g64.abs().sum(2)
        b_r = S * G.U * mags
        b_r = b_r + (0.5 * G.ulp_bf16(sums.abs() + b_r) if bf16 else 0.0)
        G._ratio('dres-dispatch', (r.grad.to(F64).reshape(N, C) - sums).abs(), b_r)
    else:                           # the masked gradient itself, exactly
        assert torch.equal(G.ncs(r.grad), g64)
    got = dict(dx=x.grad, dgamma=w.grad, dbeta=b.grad)
    assert x.grad.dtype == xdt and x.grad.shape == x.shape
    G.check_backward(x64, G.ncs(dy.to(xdt)), mask, gamma, groups, mean, rstd, got, cb, bf16, tag='-dispatch')


@gpu
@pytest.mark.parametrize('relu', [False, True], ids=['norelu', 'relu'])
@pytest.mark.parametrize('dt,r_kind', [('fp32', 'contiguous'), ('bf16', 'contiguous'), ('bf16', 'fp32'),
                                       ('fp32', 'broadcast'), ('bf16', 'broadcast')])
@pytest.mark.parametrize('N,C,sp,groups', [(2, 32, (6, 5, 12), 32), (3, 16, (7, 5), 4)])
def test_channels_last_x_with_a_residual_the_kernel_does_not_fuse(gn, N, C, sp, groups, dt, r_kind, relu):
    """a plain-contiguous residual, an fp32 one (bf16 x: y is promoted to fp32; it used to reach the backward kernel as
    a bf16 ReLU mask) and a broadcast (N, C, 1, ...) one"""
    _unfused_case(gn, N, C, sp, groups, dt, 'cl', r_kind, relu)


@gpu
@pytest.mark.parametrize('relu', [False, True], ids=['norelu', 'relu'])
@pytest.mark.parametrize('N,C,sp,groups', [(2, 32, (6, 5, 12), 32), (3, 6, (7, 5), 2)])
def test_planar_bf16_x_with_an_fp32_residual(gn, N, C, sp, groups, relu):
    _unfused_case(gn, N, C, sp, groups, 'bf16', 'planar', 'fp32', relu)


@gpu
@pytest.mark.parametrize('with_res', [False, True], ids=['nores', 'res'])
@pytest.mark.parametrize('dt', ['fp32', 'bf16'])
@pytest.mark.parametrize('N,C,sp,groups', [(2, 24, (5, 3, 7), 3), (1, 512, (3, 5), 32), (2, 24, (5, 9), 24)])
def test_channels_last_x_of_an_ineligible_width_takes_the_planar_kernels(gn, N, C, sp, groups, dt, with_res):
    """C = 24 (three or six vector blocks: no power of two) and C = 512 (> 256) in channels-last memory: the planar
    kernels on a contiguous copy -- right values, x's dtype, NC(D)HW memory like torch's own GPU GroupNorm"""
    xdt, bf16 = TDT[dt], dt == 'bf16'
    S, vec = int(torch.tensor(sp).prod()), 4 if dt == 'fp32' else 8
    inp = _dev(G.make_inputs(N, C, sp, 'random', 300 + C + N, bf16))
    x = inp['x'].to(xdt).contiguous(memory_format=_fmt(sp)).requires_grad_(True)
    r = inp['res'].to(xdt).contiguous(memory_format=_fmt(sp)).requires_grad_(True) if with_res else None
    w, b = inp['gamma'].clone().requires_grad_(True), inp['beta'].clone().requires_grad_(True)
    out = gn.group_norm(x, groups, w, b, inp['eps'], True, residual=r)
    with torch.no_grad():
        ty = F.group_norm(x.detach(), groups, inp['gamma'].to(xdt), inp['beta'].to(xdt), inp['eps'])
        ty = torch.relu(ty + r if with_res else ty)
    assert out.dtype == ty.dtype == xdt and out.shape == ty.shape
    assert out.stride() == ty.stride(), 'layout of torch\'s unfused ops'
    mean, rstd = _saved_stats(out, N, groups)
    out.backward(inp['dy'].to(xdt).contiguous(memory_format=_fmt(sp)))
    x64, gamma, beta = G.ncs(inp['x']), inp['gamma'], inp['beta']
    chain, cb = G.chain_planar(C // groups * S, vec), G.chain_bwd_planar(S, N)
    G.check_stats(x64, groups, inp['eps'], mean, rstd, chain, tag='-dispatch')
    y64 = G.ncs(out)
    mask = (y64 > 0).to(F64)
    if with_res:      # the kernel's GroupNorm, then torch's addition and ReLU in x's dtype
        pre, mag = G.apply(x64, mean, rstd, gamma, beta)
        bound = 3 * G.U * mag + (0.5 * G.ulp_bf16(pre.abs() + 3 * G.U * mag) if bf16 else 0.0)
        total = pre + G.ncs(r)
        bound = bound + (0.5 * G.ulp_bf16(total.abs() + bound) if bf16 else G.U * (total.abs() + bound))
        G._ratio('y-unfused-' + dt, (y64 - total.clamp_min(0)).abs(), bound)
        assert torch.equal(G.ncs(r.grad), G.ncs(inp['dy']) * mask)
    else:
        G.check_apply(x64, gamma, beta, None, True, out, mean, rstd, bf16, tag='-dispatch')
    G.check_backward(x64, G.ncs(inp['dy']), mask, gamma, groups, mean, rstd,
                     dict(dx=x.grad, dgamma=w.grad, dbeta=b.grad), cb, bf16, tag='-dispatch')


@gpu
def test_hip_group_norm_module_passes_relu_and_residual_through(gn):
    """HipGroupNorm.forward(x, relu, residual) is group_norm() on the module's parameters (bf16 ones included): the
    same bits, an fp32 residual promoting the output"""
    N, C, sp, groups = 2, 32, (4, 5, 6), 32
    cl = torch.channels_last_3d
    m = gn.HipGroupNorm(groups, C).cuda().to(torch.bfloat16)
    inp = _dev(G.make_inputs(N, C, sp, 'random', 17, True))
    with torch.no_grad():
        m.weight.copy_(inp['gamma'])
        m.bias.copy_(inp['beta'])
    res = []
    for call in (lambda x, r: m(x, relu=True, residual=r),
                 lambda x, r: gn.group_norm(x, groups, m.weight, m.bias, m.eps, True, residual=r)):
        x = inp['x'].bfloat16().contiguous(memory_format=cl).requires_grad_(True)
        r = (inp['res'] + 2.0 ** -12).contiguous(memory_format=cl).requires_grad_(True)      # fp32, not bf16 values
        m.zero_grad()
        out = call(x, r)
        out.backward(inp['dy'].contiguous(memory_format=cl))
        res.append((out.detach(), x.grad, r.grad, m.weight.grad.clone(), m.bias.grad.clone()))
    assert res[0][0].dtype == torch.float32 and res[0][0].is_contiguous(memory_format=cl)
    assert res[0][1].dtype == torch.bfloat16 and res[0][2].dtype == torch.float32 and res[0][3].dtype == torch.bfloat16
    for a, b in zip(*res):
        assert torch.equal(a, b)
