"""The fused tail of SPPUNetNeck's pyramid-pooling branches (csrc/spp_tail.hip: dfm_spp_tail_fwd, two kernels) against
plain fp64 references (tests/spp_ref.py) at the shapes where its code takes another path: the scalar and the MFMA
convolution for every thread map (spp_channels 8 / 16 / 32 / 64), partial pixel tiles, one-pixel branches, branches of
unequal size (the ``pmax`` stride of the workspace), batches, channel rows wider than one pass of a wave, zero to four
sources, one-row and one-column maps, and the largest shape the entry point accepts.

The references are pinned to torch's own fp64 ops on the CPU first (unmarked tests): a wrong reference cannot agree
with a wrong kernel.  The kernel-level tests call the C ABI with their own workspace so they can read the intermediate
branch maps ``small[b][branch][p][c]`` (fp32, ``pmax`` pixels reserved per branch) and check the two kernels apart:
the branch maps against the reference, the interpolation against the kernel's OWN branch maps.  Every tolerance
follows from the number formats and the reference (see the checks), none from what the kernels return."""
import ctypes
import functools
import importlib
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import spp_ref as R
from tests import util

gpu = pytest.mark.gpu
EPS = 1e-5
BF16 = torch.bfloat16

# (B, in_channels K, spp_channels C, pooled (h, w) per branch, source channels, H, W)
CASES = {
    # dynamic LDS exactly 62 KiB; four 32-pixel tiles per wave, the last one of 15 pixels; a 1 x 1 branch; a pooled
    # map larger than the output
    'mfma-limit': (1, 128, 32, ((1, 1), (1, 2), (3, 5), (12, 40)), (128, 128, 128), 9, 13),
    # lanes with cn >= C idle; B = 2; unequal pixel counts: pmax stride != P
    'mfma-c8': (2, 32, 8, ((2, 3), (1, 1)), (8,), 4, 6),
    # nks = 3; H W = 35: a last workgroup with one idle wave
    'mfma-c16': (2, 48, 16, ((5, 7), (2, 2), (1, 4)), (16, 8), 7, 5),
    # second n0 pass; 66 pixels; no sources
    'mfma-c64': (1, 64, 64, ((6, 11), (3, 5), (1, 2), (1, 1)), (), 6, 10),
    # scalar convolution (K % 16 != 0), npg = 8; two tiles, the second one short
    'scalar-c32': (2, 24, 32, ((3, 4), (7, 9)), (24,), 5, 7),
    # npg = 32; 153 pixels; four sources
    'scalar-c8': (1, 8, 8, ((9, 17),), (8, 8, 8, 8), 3, 3),
    # npg = 4; H = 1: the row scale of the interpolation is 0
    'scalar-c64': (1, 40, 64, ((2, 2), (4, 9)), (40,), 1, 9),
    # npg = 16; B = 3; W = 1
    'scalar-c16': (3, 72, 16, ((1, 1), (5, 5)), (64,), 8, 1),
    # 552 channels = 69 16-byte blocks: spp_concat_kernel's lanes take a second block each
    'wide-row': (1, 16, 16, ((2, 2), (3, 3)), (256, 256, 8), 3, 5),
    # gamma in [-1.5, -0.5]
    'neg-gamma': (2, 16, 16, ((2, 5), (3, 3)), (16,), 4, 5),
}
NAMES = tuple(CASES)
# one seed per (kind, case).  The exact-grid seeds are held to the 0.2 % cap of check (c) by
# test_fp32_emulation_of_the_kernel_stays_inside_the_cap, on the CPU, before a kernel sees them.
SEEDS = {kind: {n: 1000 * (k + 1) + i for i, n in enumerate(NAMES)} for k, kind in enumerate(('grid', 'random'))}


def make_inputs(case, seed, kind, gamma_sign=1.0):
    """CPU tensors of one call: pooled maps (B, h, w, K) bf16, weights (C, K) fp32, gamma / beta (C) fp32 per branch,
    sources (B, H, W, c) bf16.  kind 'grid': x integers in [-3, 3], weights k / 8 with integer k in [-8, 8] (exact in
    bf16: the lo half of the weight split is 0) -- every partial sum of the convolution is exact in fp32.  kind
    'random': randn x, randn / sqrt(K) weights with full fp32 significands."""
    B, K, C, pooled_hw, csrc, H, W = case
    g = torch.Generator().manual_seed(seed)
    pooled, weights, gammas, betas = [], [], [], []
    for h, w in pooled_hw:
        if kind == 'grid':
            pooled.append(torch.randint(-3, 4, (B, h, w, K), generator=g).to(BF16))
            weights.append(torch.randint(-8, 9, (C, K), generator=g).float() / 8)
        else:
            pooled.append(torch.randn(B, h, w, K, generator=g).to(BF16))
            weights.append(torch.randn(C, K, generator=g) / math.sqrt(K))
        gammas.append((0.5 + torch.rand(C, generator=g)) * gamma_sign)
        betas.append(torch.rand(C, generator=g) - 0.5)
    sources = [torch.randn(B, H, W, c, generator=g).to(BF16) for c in csrc]
    return dict(pooled=pooled, weights=weights, gammas=gammas, betas=betas, sources=sources)


@functools.lru_cache(maxsize=None)
def inputs(name, kind):
    return make_inputs(CASES[name], SEEDS[kind][name], kind, -1.0 if name == 'neg-gamma' else 1.0)


def lo_inputs(K):
    """check (e): C = 8, one branch of 2 x 2 pixels; pixel p has x[p, 0] = 2^p, x[p, 1] = -2^p; every channel's weights
    are w[0] = 1 + 2^-12, w[1] = 1.  The convolution is 2^(p - 12) through the lo half of the weight (bf16(w[0]) = 1)
    and 0 without it."""
    case = (1, K, 8, ((2, 2),), (8,), 2, 3)
    inp = make_inputs(case, 77, 'grid')
    x = torch.zeros(1, 4, K)
    x[0, :, 0] = 2.0 ** torch.arange(4)
    x[0, :, 1] = -2.0 ** torch.arange(4)
    w = torch.zeros(8, K)
    w[:, 0], w[:, 1] = 1 + 2.0 ** -12, 1.0
    inp['pooled'], inp['weights'] = [x.view(1, 2, 2, K).to(BF16)], [w]
    return case, inp


# --------------------------------------------------------------------------------------------------------------------
# 1. the references against torch's fp64 ops (CPU)
# --------------------------------------------------------------------------------------------------------------------
def test_round_bf16_is_torchs_rounding():
    g = torch.Generator().manual_seed(1)
    x = torch.cat([torch.randn(4096, generator=g) * 10.0 ** torch.randint(-6, 6, (4096,), generator=g),
                   torch.tensor([0.0, 1.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -1 - 2.0 ** -8, 255.5, 2.0 ** -20])])
    assert np.array_equal(R.round_bf16(R.f64(x)), R.f64(x.to(BF16)))           # ties to even included
    # straight from fp64: a value that fp32 would first round ONTO a bf16 tie stays on its own side of it
    assert R.round_bf16(1 + 2.0 ** -8 + 2.0 ** -40) == 1 + 2.0 ** -7
    assert np.array_equal(R.ulp_bf16(np.array([0.0, 1.0, -1.5, 0.75])), [0.0, 2.0 ** -7, 2.0 ** -7, 2.0 ** -8])


@pytest.mark.parametrize('B,h,w,K,C', [(2, 3, 5, 7, 5), (1, 1, 9, 13, 3)])
def test_branch_ref_is_conv_group_norm_relu(B, h, w, K, C):
    g = torch.Generator().manual_seed(h * w)
    x = torch.randn(B, h, w, K, generator=g, dtype=torch.float64)
    wt = torch.randn(C, K, generator=g, dtype=torch.float64)
    ga, be = torch.randn(C, generator=g, dtype=torch.float64), torch.randn(C, generator=g, dtype=torch.float64)
    ref = F.relu(F.group_norm(F.conv2d(x.permute(0, 3, 1, 2), wt.view(C, K, 1, 1)), C, ga, be, EPS))
    got = R.branch_ref(x, wt, ga, be, EPS, staged=False)
    assert got.shape == (B, h, w, C) and float(ref.max()) > 0.5
    np.testing.assert_allclose(got, ref.permute(0, 2, 3, 1).numpy(), rtol=0, atol=1e-12)
    # staged: the same two ops with torch's own bf16 casts in between (inputs whose convolution is exact in fp32,
    # so the casts see the same numbers)
    xi = torch.randint(-3, 4, (B, h, w, K), generator=g).double()
    wi = torch.randint(-8, 9, (C, K), generator=g).double() / 8
    conv = F.conv2d(xi.permute(0, 3, 1, 2), wi.view(C, K, 1, 1)).to(BF16).double()
    gn = F.group_norm(conv, C, ga, be, EPS)
    staged = R.branch_ref(xi, wi, ga, be, EPS, staged=True)
    assert np.array_equal(staged, R.round_bf16(F.relu(gn).permute(0, 2, 3, 1).numpy()))


@pytest.mark.parametrize('h,w,H,W', [(3, 5, 7, 11), (12, 7, 5, 1), (1, 4, 1, 9)])
def test_resize_ref_is_interpolate(h, w, H, W):
    x = torch.randn(2, 3, h, w, generator=torch.Generator().manual_seed(h + w), dtype=torch.float64)
    ref = F.interpolate(x, (H, W), mode='bilinear', align_corners=True)
    got = R.resize_ref(x.permute(0, 2, 3, 1), H, W)
    assert got.shape == (2, H, W, 3)
    np.testing.assert_allclose(got, ref.permute(0, 2, 3, 1).numpy(), rtol=0, atol=1e-13)


@pytest.mark.parametrize('H,W,k', [(75, 141, 8), (37, 19, (4, 3))])
def test_pool_ref_is_avg_pool(H, W, k):
    x = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(H), dtype=torch.float64)
    ref = F.avg_pool2d(x, k, stride=k)
    assert ref.shape[2] * (k if isinstance(k, int) else k[0]) < H      # the floor mode drops rows
    np.testing.assert_allclose(R.pool_ref(x, k), ref.numpy(), rtol=0, atol=1e-14)


# --------------------------------------------------------------------------------------------------------------------
# 2. the kernels through the C ABI
# --------------------------------------------------------------------------------------------------------------------
CAP = 0.002     # check (c): share of elements that may miss the staged reference, each by one bf16 ulp at most


def staged_refs(inp):
    return [R.branch_ref(x, w, ga, be, EPS, staged=True)
            for x, w, ga, be in zip(inp['pooled'], inp['weights'], inp['gammas'], inp['betas'])]


def assert_staged_match(small, refs, betas):
    """check (c).  ``small``: per branch (B, h, w, C) float32.  The fp32 statistics of the kernel differ from the
    fp64 ones by ~2^-23 relative, which moves a GroupNorm output across a bf16 rounding boundary about once in 2^14
    elements: at least 99.8 % of a case's elements are the reference's bits, the rest its neighbours; a one-pixel
    branch is exactly relu(bf16(beta)) (its convolution minus its mean is 0 in any precision)."""
    total = missed = 0
    for s, ref, be in zip(small, refs, betas):
        assert s.dtype == np.float32 and s.shape == ref.shape and np.isfinite(s).all()
        ref32 = ref.astype(np.float32)
        assert np.array_equal(ref32.astype(np.float64), ref)
        off = s != ref32
        assert (np.abs(s.astype(np.float64) - ref)[off] <= R.ulp_bf16(ref)[off]).all(), 'more than one bf16 ulp off'
        if ref.shape[1] * ref.shape[2] == 1:
            flat = np.maximum(R.round_bf16(R.f64(be)), 0).astype(np.float32)
            assert np.array_equal(s, np.broadcast_to(flat, s.shape))
        total, missed = total + off.size, missed + int(off.sum())
    assert missed <= CAP * total, f'{missed} of {total} elements are not the staged reference'
    return missed, total


def emulated(inp):
    return [np.stack([R.emulate_branch_f32(xb.reshape(-1, xb.shape[-1]), w, ga, be, EPS).reshape(*xb.shape[:2], -1)
                      for xb in x])
            for x, w, ga, be in zip(inp['pooled'], inp['weights'], inp['gammas'], inp['betas'])]


@pytest.mark.parametrize('name', NAMES + ('lo-mfma', 'lo-scalar'))
def test_fp32_emulation_of_the_kernel_stays_inside_the_cap(name):
    """The cap of check (c) is a condition on the seeds, shown here without a GPU: the branch kernel's arithmetic
    in numpy float32 (two-pass statistics with the kernel's thread map) on the same exact-grid inputs meets the
    criterion the kernel is held to."""
    if name.startswith('lo-'):
        case, inp = lo_inputs(16 if name == 'lo-mfma' else 8)
    else:
        case, inp = CASES[name], inputs(name, 'grid')
    missed, total = assert_staged_match(emulated(inp), staged_refs(inp), inp['betas'])
    print(f'[emulation] {name}: {missed} of {total} elements one bf16 ulp off the staged reference')


@pytest.fixture(scope='module')
def hip():
    import types
    names = ('_capi', '_launch', 'modules')
    return types.SimpleNamespace(**{n: importlib.import_module('depth-from-motion_amd.' + n) for n in names})


def call_tail(hip, case, inp, tweak=None, ws_delta=0):
    """dfm_spp_tail_fwd on the GPU with the test's own workspace.  Returns (out (B, H, W, ctot) bf16 on the CPU, small:
    per branch (B, h, w, C) float32).  ``out`` and the workspace start as NaN: what a kernel does not write shows.
    ``tweak(desc, args)`` edits the descriptor / the tensor lists of a refused call; a ``DfmHipError`` leaves with
    the output as the call left it in its ``out`` attribute."""
    B, K, C, pooled_hw, csrc, H, W = case
    dev = torch.device('cuda:0')
    a = {k: [t.to(dev) for t in v] for k, v in inp.items()}
    d = hip._capi.SppDesc()
    d.batch, d.h, d.w = B, H, W
    d.num_sources, d.num_branches, d.in_channels, d.spp_channels, d.eps = len(csrc), len(pooled_hw), K, C, EPS
    for i, c in enumerate(csrc):
        d.source_channels[i] = c
    for i, (h, w) in enumerate(pooled_hw):
        d.pooled_h[i], d.pooled_w[i] = h, w
    if tweak is not None:
        tweak(d, a)
    ctot = sum(csrc) + len(pooled_hw) * C
    out = torch.full((B, H, W, ctot), float('nan'), dtype=BF16, device=dev)
    need = hip._capi.lib().dfm_spp_tail_workspace_bytes(ctypes.byref(d))
    pmax = max(h * w for h, w in pooled_hw)
    ws = torch.full((max(need, B * len(pooled_hw) * pmax * C * 4, 256) // 4,), float('nan'), device=dev)
    P = hip._launch.pointers
    try:
        hip._launch.launch('dfm_spp_tail_fwd', d, P(a['pooled'], 4), P(a['weights'], 4), P(a['gammas'], 4),
                           P(a['betas'], 4), P(a['sources'], 4), out, ws, (need or ws.numel() * 4) + ws_delta,
                           hip._launch.STREAM)
    except hip._capi.DfmHipError as e:
        torch.cuda.synchronize()
        e.out = out.cpu()
        raise
    torch.cuda.synchronize()
    assert need == (B * len(pooled_hw) * pmax * C * 4 + 255) // 256 * 256
    small = ws[:B * len(pooled_hw) * pmax * C].view(B, len(pooled_hw), pmax, C).cpu().numpy()
    return out.cpu(), [small[:, i, :h * w].reshape(B, h, w, C) for i, (h, w) in enumerate(pooled_hw)]


_RAN = {}


def _ran(hip, name, kind):
    """one launch per (case, kind), shared by the checks"""
    if (name, kind) not in _RAN:
        _RAN[name, kind] = call_tail(hip, CASES[name], inputs(name, kind))
    return _RAN[name, kind]


@gpu
@pytest.mark.parametrize('kind', ('grid', 'random'))
@pytest.mark.parametrize('name', NAMES)
def test_copied_channels_are_the_sources_bits(hip, name, kind):
    """(a) out[..., :sum(csrc)] is torch.cat(sources, -1), bit for bit"""
    out, _ = _ran(hip, name, kind)
    src = inputs(name, kind)['sources']
    nsrc = sum(CASES[name][4])
    assert out.shape[-1] == nsrc + len(CASES[name][3]) * CASES[name][2]
    if src:
        assert torch.equal(out[..., :nsrc], torch.cat(src, -1))
    assert not torch.isnan(out).any(), 'a channel block was never written'


def assert_interpolated(out, small, case):
    """(b) the interpolation alone: the branch channels of ``out`` against resize_ref of the kernel's OWN branch maps,
    |out - v| <= 2^-8 |v| + 2^-16 max|small|.  First term: one bf16 round-to-nearest (8 significand bits: unit
    roundoff 2^-8) of a non-negative convex combination.  Second: the fp32 interpolation weight -- real = scale *
    dst carries at most in * 2^-23 of absolute error (in <= 40 here: < 2^-17 per axis), and it multiplies a
    difference of two values of the map, at most max|small| as the map is non-negative."""
    B, K, C, pooled_hw, csrc, H, W = case
    o = R.f64(out)
    for i, s in enumerate(small):
        v = R.resize_ref(s, H, W)
        got = o[..., sum(csrc) + i * C:sum(csrc) + (i + 1) * C]
        tol = 2.0 ** -8 * np.abs(v) + 2.0 ** -16 * np.abs(s).max(axis=(1, 2, 3), keepdims=True)
        err = np.abs(got - v)
        worst = float(np.nanmax(err / np.maximum(tol, 1e-300))) if np.isfinite(err).any() else float('nan')
        print(f'[interp] branch {i} {s.shape[1:3]} -> {(H, W)}: max err / tol = {worst:.3f}')
        assert (err <= tol).all(), f'branch {i}: {int((~(err <= tol)).sum())} elements outside the bound'
        assert float(v.max()) > 0.1, 'the branch map is (nearly) all zero: the case checks nothing'


@gpu
@pytest.mark.parametrize('kind', ('grid', 'random'))
@pytest.mark.parametrize('name', NAMES)
def test_interpolation_of_the_kernels_own_branch_maps(hip, name, kind):
    out, small = _ran(hip, name, kind)
    assert_interpolated(out, small, CASES[name])


@gpu
@pytest.mark.parametrize('name', NAMES)
def test_branch_maps_on_exact_grid_inputs_are_the_staged_reference(hip, name):
    """(c) inputs on a grid where every partial sum of the convolution is exact in fp32 and the weights are exact in
    bf16: the kernel's bf16 convolution output has the staged reference's bits in any summation order, and what is
    left is the fp32 GroupNorm (assert_staged_match)."""
    _, small = _ran(hip, name, 'grid')
    inp = inputs(name, 'grid')
    missed, total = assert_staged_match(small, staged_refs(inp), inp['betas'])
    print(f'[exact grid] {name}: {missed} of {total} elements one bf16 ulp off the staged reference')


@gpu
@pytest.mark.parametrize('name', NAMES)
def test_branch_maps_on_random_inputs_within_the_bf16_bound(hip, name):
    """(d) full-significand weights, every branch of at least 2 pixels against the UNSTAGED fp64 reference within
    spp_ref.branch_tol (derived there; computed from the reference alone)"""
    _, small = _ran(hip, name, 'random')
    inp = inputs(name, 'random')
    checked = 0
    for i, (s, x, w, ga, be) in enumerate(zip(small, inp['pooled'], inp['weights'], inp['gammas'], inp['betas'])):
        if x.shape[1] * x.shape[2] < 2:
            continue
        ref, tol = R.branch_ref(x, w, ga, be, EPS, staged=False), R.branch_tol(x, w, ga, be, EPS)
        err = np.abs(s.astype(np.float64) - ref)
        print(f'[random] {name} branch {i}: max err / tol = {float(np.nanmax(err / tol)):.3f}')
        assert (err <= tol).all(), f'branch {i}: {int((~(err <= tol)).sum())} of {err.size} elements outside the bound'
        assert float(ref.max()) > 0.5
        checked += 1
    assert checked


@gpu
@pytest.mark.parametrize('K', (16, 8), ids=('mfma', 'scalar'))
def test_the_lo_half_of_the_weights_is_used(hip, K):
    """(e) a convolution that is 2^(p - 12) with the lo product of the hi + lo weight split and 0 without it (the
    scalar path multiplies the fp32 weight itself).  The reference varies over the pixels; a kernel without the lo
    term returns relu(bf16(beta)) at every pixel."""
    case, inp = lo_inputs(K)
    conv = R.f64(inp['pooled'][0]) @ R.f64(inp['weights'][0]).T
    assert np.array_equal(conv[0].reshape(4, 8), np.repeat(2.0 ** (np.arange(4.0) - 12), 8).reshape(4, 8))
    refs = staged_refs(inp)
    flat = np.maximum(R.round_bf16(R.f64(inp['betas'][0])), 0)
    assert (np.abs(refs[0] - flat) > R.ulp_bf16(refs[0])).sum() >= refs[0].size // 4, 'the reference does not tell'
    out, small = call_tail(hip, case, inp)
    assert_staged_match(small, refs, inp['betas'])
    assert torch.equal(out[..., :8], inp['sources'][0])
    assert_interpolated(out, small, case)


# --------------------------------------------------------------------------------------------------------------------
# 3. refusals: host validation, before any launch
# --------------------------------------------------------------------------------------------------------------------
SMALL = (1, 16, 8, ((2, 2),), (8,), 2, 2)


def _five_branches(d, a):
    d.num_branches = 5


def _odd_source(d, a):
    d.source_channels[0] = 12


def _misaligned_source(d, a):
    flat = torch.zeros(a['sources'][0].numel() + 8, dtype=BF16, device=a['sources'][0].device)
    a['sources'][0] = flat[1:1 + a['sources'][0].numel()].view(a['sources'][0].shape)
    assert a['sources'][0].data_ptr() % 16 == 2


def _zero_height(d, a):
    d.pooled_h[0] = 0


REFUSALS = {
    'spp_channels-24': ((1, 16, 24, ((2, 2),), (8,), 2, 2), None, 0),
    'spp_channels-72': ((1, 16, 72, ((2, 2),), (8,), 2, 2), None, 0),
    'five-branches': (SMALL, _five_branches, 0),
    'source-of-12-channels': (SMALL, _odd_source, 0),
    'source-2-bytes-off': (SMALL, _misaligned_source, 0),
    'workspace-1-byte-short': (SMALL, None, -1),
    'zero-height-pooled-map': (SMALL, _zero_height, 0),
    # 481 pixels: one past the largest finest branch of in_channels 128, spp_channels 32 (mfma-limit runs 480)
    '481-pixels': ((1, 128, 32, ((13, 37),), (8,), 2, 2), None, 0),
}


@gpu
@pytest.mark.parametrize('name', tuple(REFUSALS))
def test_refusals_come_from_host_validation(hip, name):
    case, tweak, ws_delta = REFUSALS[name]
    with pytest.raises(hip._capi.DfmHipError, match=r'error -[123]:') as refused:      # never DFM_ERR_HIP (-4)
        call_tail(hip, case, make_inputs(case, 5, 'random'), tweak, ws_delta)
    assert torch.isnan(refused.value.out).all(), 'a refused call wrote to its output'


@gpu
def test_the_accepted_call_next_to_the_refusals_runs(hip):
    """the refusals above differ from this call in the one thing they name"""
    out, _ = call_tail(hip, SMALL, make_inputs(SMALL, 5, 'random'))
    assert not torch.isnan(out).any()


# --------------------------------------------------------------------------------------------------------------------
# 4. SPPUNetNeck: the host-side pooling, the fused tail inside the module, and its gate
# --------------------------------------------------------------------------------------------------------------------
GN16 = dict(type='GN', num_groups=16, requires_grad=True)
CL = torch.channels_last


def _neck(hip, seed=31, dtype=BF16, **kw):
    kw = dict(dict(in_channels=[3, 16, 24, 24, 24], start_level=2, spp_channel=16, norm_cfg=GN16), **kw)
    neck = hip.modules.SPPUNetNeck(**kw)
    neck.load_state_dict(util.synthetic_state_dict(neck, seed), strict=True)
    return neck.eval().cuda().to(dtype)


def _feats(channels=(3, 16, 24, 24, 24), B=2, hw=(75, 141), dtype=BF16, seed=9, fmt=CL):
    """the five level maps on the GPU; levels 2-4 are ``hw``, levels 0 / 1 (read by the up-convolutions only) tiny"""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, c, *(hw if i >= 2 else (4, 4)), generator=g).cuda().to(dtype).contiguous(memory_format=fmt)
            for i, c in enumerate(channels)]


@gpu
@pytest.mark.parametrize('shape,sizes', [((2, 16, 75, 141), ((1, 2), (2, 4), (4, 8), (9, 17))),
                                         ((1, 24, 64, 64), ((1, 1), (2, 2), (4, 4), (8, 8)))])
def test_spp_pool_is_floor_mode_window_means(hip, shape, sizes, monkeypatch):
    """one fp32 pass of 8 x 8 means, the coarser windows as means of those, on maps whose sides are NOT whole
    windows: each output within one bf16 rounding (unit roundoff 2^-8) of the fp64 window mean; 2^-20 covers the
    fp32 means of ~N(0, 1) values.  The per-branch fallback ``[p(x) for p in pools]`` meets the same bound, so the
    test also holds that no branch's own pooling module ran: the values are the one-pass path's."""
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(3)).to(BF16).cuda().contiguous(memory_format=CL)
    neck, own = _neck(hip), []
    assert all(type(b[0]) is hip.modules._WindowMean2d for b in neck.spp_branches)
    monkeypatch.setattr(hip.modules._WindowMean2d, 'forward', lambda self, t: own.append(self.kernel_size))
    with torch.no_grad():
        got = neck._spp_pool(x)
    assert not own, f'_spp_pool fell back to the per-branch pooling modules {own}'
    assert [tuple(p.shape[2:]) for p in got] == list(sizes)
    for p, k in zip(got, (64, 32, 16, 8)):
        ref = R.pool_ref(x, k)
        assert p.dtype == BF16 and p.shape[:2] == shape[:2]
        assert (np.abs(R.f64(p) - ref) <= 2.0 ** -8 * np.abs(ref) + 2.0 ** -20).all(), k


def _assert_concat(hip, neck, feats, concat):
    """a concatenated feature of ``neck`` on ``feats`` against the fp64 references end to end: sources bit for bit,
    branch i within  resize_ref(2 * branch_tol): twice check (d)'s bound, carried through the up-sampling.  The
    pooled map the kernel reads is the fp64 window mean rounded to bf16: one more relative 2^-8 on each of the
    convolution's INPUTS, independent over the K terms of a sum, which reaches the convolution output with the
    spread of the output's own rounding -- so twice (d)'s bound on the branch map.  The up-sampling is a convex
    combination, which carries a bound on the map to the same combination of it, and the bf16 rounding of its
    result is at most 2^-8 |v|: the second 2^-8 |y| that the doubling holds (the first is the GroupNorm output's
    rounding), |v| being the same combination of the |y|."""
    assert concat.is_contiguous(memory_format=CL) and not concat.is_contiguous()
    nsrc = sum(f.shape[1] for f in feats[2:])
    assert concat.shape == (feats[2].shape[0], nsrc + 4 * neck.spp_channel, *feats[2].shape[2:])
    assert torch.equal(concat[:, :nsrc], torch.cat(feats[2:], 1))
    H, W = feats[2].shape[2:]
    o = R.f64(concat.permute(0, 2, 3, 1))
    for i, (branch, k) in enumerate(zip(neck.spp_branches, (64, 32, 16, 8))):
        pooled = R.pool_ref(feats[-1], k).transpose(0, 2, 3, 1)
        w = branch[1].conv.weight.reshape(neck.spp_channel, -1)
        ga, be, eps = branch[1].gn.weight, branch[1].gn.bias, branch[1].gn.eps
        small = R.branch_ref(pooled, w, ga, be, eps, staged=False)
        v = R.resize_ref(small, H, W)
        tol = R.resize_ref(2 * R.branch_tol(pooled, w, ga, be, eps), H, W)
        err = np.abs(o[..., nsrc + i * neck.spp_channel:nsrc + (i + 1) * neck.spp_channel] - v)
        print(f'[neck] branch {i}: max err / tol = {float(np.nanmax(err / tol)):.3f}')
        assert (err <= tol).all(), f'branch {i}: {int((~(err <= tol)).sum())} of {err.size} elements outside the bound'
        assert float(v.max()) > 0.1


@gpu
def test_neck_fused_tail_against_the_references(hip):
    """in_channels 24: the scalar convolution, pooled maps 1 x 2 .. 9 x 17 cropped from 75 x 141, B = 2"""
    neck, feats = _neck(hip), _feats()
    with torch.no_grad():
        fused = neck._spp_tail_fused([None, None] + feats[2:])
    assert fused is not None
    _assert_concat(hip, neck, feats, fused)


def _concat_of_forward(neck, feats):
    """what ``forward`` hands on as the concatenated feature: with the convolutions behind it taken out, forward
    returns it as both of its outputs"""
    neck.with_upconv = False
    neck.lastconv = neck.rpnconv = torch.nn.Identity()
    stereo, sem = neck(feats)
    assert stereo is sem
    return sem


def _unfused(hip, neck, feats):
    spp = [hip.modules.bilinear_resize(b[1](p), size=tuple(feats[2].shape[2:]), align_corners=True)
           for b, p in zip(neck.spp_branches, neck._spp_pool(feats[-1]))]
    return torch.cat((*feats[2:], *spp), 1)


@gpu
@pytest.mark.parametrize('why', ('autograd', 'fp32', 'over-the-lds-gate'))
def test_gate_declines_and_forward_takes_the_unfused_ops(hip, why):
    grad = why == 'autograd'
    if why == 'over-the-lds-gate':
        # 104 x 304 with 128 channels: a finest branch of 13 x 38 = 494 pixels, (128 * 32 + 32 * 128) * 4 + 494 * 64 B
        # of LDS > 62 KiB
        ch = (3, 16, 128, 128, 128)
        neck = _neck(hip, in_channels=list(ch), spp_channel=32, norm_cfg=dict(type='GN', num_groups=32))
        feats = _feats(ch, B=1, hw=(104, 304))
    else:
        neck = _neck(hip, dtype=torch.float32 if why == 'fp32' else BF16)
        feats = _feats(dtype=torch.float32 if why == 'fp32' else BF16)
    if grad:
        feats[-1].requires_grad_(True)
    with torch.set_grad_enabled(grad):
        assert neck._spp_tail_fused(feats) is None
        got = _concat_of_forward(neck, feats)
        ref = _unfused(hip, neck, feats)
    assert got.requires_grad == grad
    assert got.shape == ref.shape and torch.equal(got.detach(), ref.detach())
    if why == 'over-the-lds-gate':
        with torch.no_grad():
            assert tuple(neck._spp_pool(feats[-1])[-1].shape[2:]) == (13, 38)
            x = feats[-1][:, :, :, :296].contiguous(memory_format=CL)          # 13 x 37 = 481 pixels: still over
            assert neck._spp_tail_fused([None, None, x, x, x]) is None
            x = x[:, :, :96].contiguous(memory_format=CL)                      # 12 x 37: the gate opens
            assert neck._spp_tail_fused([None, None, x, x, x]) is not None


@gpu
def test_gate_declines_nchw_sources_and_forward_relays_them(hip):
    """NCHW-contiguous sources: the tail itself declines; forward lays its inputs out channels-last first, so its
    concatenated feature meets the same references as the fused tail's"""
    neck, feats = _neck(hip), _feats(fmt=torch.contiguous_format)
    assert feats[2].is_contiguous()
    with torch.no_grad():
        assert neck._spp_tail_fused(feats) is None
        got = _concat_of_forward(neck, feats)
    _assert_concat(hip, neck, feats, got)
