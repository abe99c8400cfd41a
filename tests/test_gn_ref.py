"""tests/gn_ref.py on the CPU, before a kernel is held against it: the fp64 reference pinned to torch's own fp64
GroupNorm + autograd, the launch geometry the partial-count checks rely on, and the proof that the checkers can be met
and bite -- torch's fp32 CPU GroupNorm passes every checker on every case of tests/test_group_norm_exact_gpu.py, three
small mutations of that same result fail."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import gn_ref as G
from tests import spp_ref as R

F64 = torch.float64


def test_ulp_bf16_is_spp_refs():
    g = torch.Generator().manual_seed(3)
    a = torch.cat([torch.randn(4096, generator=g, dtype=F64) * 10.0 ** torch.randint(-6, 6, (4096,), generator=g),
                   torch.tensor([0.0, 1.0, -1.5, 0.75, 2.0 ** -20, 255.5], dtype=F64)])
    assert np.array_equal(G.ulp_bf16(a).numpy(), R.ulp_bf16(a.numpy()))
    # half an ulp is what torch's own rounding to bf16 moves a value by, at most
    assert bool(((a - a.bfloat16().double()).abs() <= 0.5 * G.ulp_bf16(a)).all())


@pytest.mark.parametrize('relu,with_res', [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize('N,C,sp,groups', [(2, 6, (5, 7), 3), (1, 8, (3, 2, 5), 1), (3, 4, (9,), 4)])
def test_reference_is_torchs_fp64_group_norm_and_autograd(N, C, sp, groups, relu, with_res):
    g = torch.Generator().manual_seed(N * 10 + C)
    x, dy, res = (torch.randn(N, C, *sp, generator=g, dtype=F64) for _ in range(3))
    x = x * 2 + 0.7
    gamma, beta = torch.randn(C, generator=g, dtype=F64), torch.randn(C, generator=g, dtype=F64)
    xr, rr, wr, br = (t.clone().requires_grad_(True) for t in (x, res, gamma, beta))
    y = F.group_norm(xr, groups, wr, br, 1e-5)
    y = y + rr if with_res else y
    y = F.relu(y) if relu else y
    y.backward(dy)
    mean, var = G.moments(G.ncs(x), groups)
    tm, tv = x.reshape(N, groups, -1).mean(2), x.reshape(N, groups, -1).var(2, unbiased=False)
    assert torch.allclose(mean, tm, rtol=0, atol=1e-12) and torch.allclose(var, tv, rtol=0, atol=1e-12)
    rstd = 1 / torch.sqrt(var + 1e-5)
    pre, mag = G.apply(G.ncs(x), mean, rstd, gamma, beta, G.ncs(res) if with_res else None)
    want = pre.clamp_min(0) if relu else pre
    assert torch.allclose(want, G.ncs(y), rtol=0, atol=1e-12)
    assert bool((mag >= pre.abs() - 1e-12).all())
    mask = (G.ncs(y) > 0).to(F64) if relu else torch.ones_like(pre)
    ref = G.backward(G.ncs(x), G.ncs(dy) * mask, mean, rstd, gamma, groups)
    assert torch.allclose(ref['dbeta'], br.grad, rtol=0, atol=1e-12)
    assert torch.allclose(ref['dgamma'], wr.grad, rtol=0, atol=1e-12)
    assert torch.allclose(ref['dx'], G.ncs(xr.grad), rtol=0, atol=1e-12)
    if with_res:
        assert torch.allclose(G.ncs(dy) * mask, G.ncs(rr.grad), rtol=0, atol=1e-12)


def test_launch_geometry():
    """the slices restate the host code: they tile [0, S) in order, and the shapes the GPU cases are named after are
    what they claim"""
    for S, C in ((4481, 256), (129, 256), (1025, 4), (131584, 32), (524803, 32), (1048583, 32), (1049095, 32), (3, 256)):
        sl = G.cl_slices(S, G.cl_splits(S, C))
        assert sl[0][0] == 0 and all(a[1] == b[0] for a, b in zip(sl, sl[1:])) and sl[-1][1] == S
    sl = G.cl_slices(4481, G.cl_splits(4481, 256))
    assert len(sl) == 70 and sl[0] == (0, 65) and sl[68] == (4420, 4481) and sl[69] == (4481, 4481)   # an empty slice
    assert G.cl_slices(129, G.cl_splits(129, 256)) == [(0, 65), (65, 129)]
    assert G.cl_splits(131584, 32) == 257 and G.cl_splits(131583, 32) == 256
    assert G.cl_splits(524803, 32) == 1025 and G.cl_bwd_splits(524803, 32) == 1024
    assert G.cl_splits(1048583, 32) == 2048 and 1048583 * 32 // 16384 == 2048     # the cap reached, nothing clamped
    assert G.cl_splits(1049095, 32) == 2048 and 1049095 * 32 // 16384 == 2049     # ... and clamped
    assert G.planar_slices(65542, G.planar_splits(65542), 4) == [(0, 32772), (32772, 65542)]
    assert G.planar_slices(65542, 2, 8) == [(0, 32776), (32776, 65542)]
    assert G.planar_slices(3, 1, 8) == [(0, 3)]
    # 'grid' inputs keep every sum of dbeta an integer below 2^24
    for name, c in G.CL_CASES.items():
        assert 3 * c['N'] * c['S'] < 2 ** 24, name


def _proof(N, C, groups, S, inp, mode, bf16, exact, backward_too=True):
    relu, with_res = G.MODES[mode]
    got = G.torch_fp32(inp, groups, relu, with_res, bf16)
    chain, cb = G.chain_torch_cpu(S, C // groups, N)
    return got, G.check_all(inp, groups, relu, with_res, bf16, got, chain, cb, exact_dbeta=exact, raw_sums=True,
                            backward_too=backward_too)


_CL = G.cl_params()
_PL = G.planar_params()


@pytest.mark.parametrize('name,dt,mode,kind', _CL, ids=['-'.join(p) for p in _CL])
def test_torch_fp32_meets_every_bound_channels_last_cases(name, dt, mode, kind):
    N, C, groups, S, vec, inp = G.cl_case(name, dt, kind)
    _proof(N, C, groups, S, inp, mode, dt == 'bf16', kind == 'grid', G.CL_CASES[name]['backward'])


@pytest.mark.parametrize('name,dt,mode,kind', _PL, ids=['-'.join(p) for p in _PL])
def test_torch_fp32_meets_every_bound_planar_cases(name, dt, mode, kind):
    N, C, groups, S, vec, inp = G.planar_case(name, dt, kind)
    _proof(N, C, groups, S, inp, mode, dt == 'bf16', kind == 'grid')


# --------------------------------------------------------------------------------------------------------------------
# the checkers bite: three mutations of torch's fp32 result, each the size of one slice's edge or one vector
# --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def passing():
    """widest-g32-S129 (two slices, 65 + 64 voxels, eight channels a group), fp32, relu + residual: inputs, torch's
    fp32 result, and the arguments under which it passes"""
    N, C, groups, S, vec, inp = G.cl_case('widest-g32-S129', 'fp32', 'random')
    got, ratios = _proof(N, C, groups, S, inp, 'relures', False, False)
    assert max(ratios.values()) <= 1.0
    chain, cb = G.chain_torch_cpu(S, C // groups, N)
    return dict(N=N, C=C, groups=groups, S=S, inp=inp, got=got, chain=chain, cb=cb)


def _recheck(p, got, **kw):
    return G.check_all(p['inp'], p['groups'], True, True, False, got, p['chain'], p['cb'], raw_sums=True, **kw)


def test_mutation_a_slice_that_loses_its_last_voxel_fails_the_statistics(passing):
    p = passing
    lo, hi = G.cl_slices(p['S'], G.cl_splits(p['S'], p['C']))[0]
    keep = [v for v in range(p['S']) if v != hi - 1]
    x = p['inp']['x'][:, :, keep].contiguous()
    _, mean, rstd = torch.native_group_norm(x, None, None, p['N'], p['C'], p['S'] - 1, p['groups'], p['inp']['eps'])
    with pytest.raises(AssertionError, match='mean|rstd'):
        _recheck(p, dict(p['got'], mean=mean, rstd=rstd))
    # ... and the statistics alone, for the kernels' own chain lengths as well
    xs = G.ncs(p['inp']['x'])
    for chain in (p['chain'], G.chain_cl(p['S'], p['C'], p['groups'], 4)):
        G.check_stats(xs, p['groups'], p['inp']['eps'], p['got']['mean'], p['got']['rstd'], p['chain'])
        with pytest.raises(AssertionError):
            G.check_stats(xs, p['groups'], p['inp']['eps'], mean, rstd, chain)


def test_mutation_a_vector_normalised_with_the_next_vectors_affine_fails_the_apply(passing):
    p = passing
    inp, got = p['inp'], p['got']
    n, v, c0 = 1, 70, 8                      # one 16-byte vector: four fp32 channels of one voxel
    C = p['C']
    mean = got['mean'].repeat_interleave(C // p['groups'], 1)[n, c0:c0 + 4]    # (the group stays the same: cpg = 8)
    rstd = got['rstd'].repeat_interleave(C // p['groups'], 1)[n, c0:c0 + 4]
    wrong = (inp['x'][n, c0:c0 + 4, v] - mean) * rstd * inp['gamma'][c0 + 4:c0 + 8] + inp['beta'][c0 + 4:c0 + 8]
    y = got['y'].clone()
    y[n, c0:c0 + 4, v] = torch.relu(wrong + inp['res'][n, c0:c0 + 4, v])
    assert 1 <= int((y != got['y']).sum()) <= 4      # (the ReLU zeroes some of the four either way)
    with pytest.raises(AssertionError, match='y-fp32: error'):
        _recheck(p, dict(got, y=y), backward_too=False)


@pytest.mark.parametrize('kind', ['random', 'grid'])
def test_mutation_a_slice_left_out_of_the_parameter_gradients_fails_the_backward(passing, kind):
    p = passing
    N, C, groups, S, vec, inp = G.cl_case('widest-g32-S129', 'fp32', kind)
    got = G.torch_fp32(inp, groups, True, True, False)
    args = (inp, groups, True, True, False)
    kw = dict(exact_dbeta=kind == 'grid', raw_sums=True)
    G.check_all(*args, got, p['chain'], p['cb'], **kw)
    lo, hi = G.cl_slices(S, G.cl_splits(S, C))[1]
    g = inp['dy'] * (got['y'] > 0)
    xh = (inp['x'] - got['mean'].repeat_interleave(C // groups, 1)[:, :, None]) * \
        got['rstd'].repeat_interleave(C // groups, 1)[:, :, None]
    sl = slice(lo, hi)
    short = dict(got, dbeta=got['dbeta'] - g[:, :, sl].sum((0, 2)), dgamma=got['dgamma'] - (g * xh)[:, :, sl].sum((0, 2)))
    with pytest.raises(AssertionError, match='dbeta'):
        G.check_all(*args, short, p['chain'], p['cb'], **kw)
    with pytest.raises(AssertionError, match='dgamma'):
        G.check_all(*args, dict(short, dbeta=got['dbeta']), p['chain'], p['cb'], **kw)
    # one voxel of one channel is enough on the exact grid
    if kind == 'grid':
        one = got['dbeta'].clone()
        one[5] -= g[0, 5, S - 1] if float(g[0, 5, S - 1]) != 0 else 1.0
        with pytest.raises(AssertionError, match='dbeta'):
            G.check_all(*args, dict(got, dbeta=one), p['chain'], p['cb'], **kw)
