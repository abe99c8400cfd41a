"""tests/depth_ref.py on the CPU, before a kernel is held against it: the fp64 references pinned to torch's own fp64 ops
and to the fixtures the REFERENCE class produced (tests/golden/depth_loss.npz), up_index's float32 restatement and the
host's dispatch rule, the proof that the checkers can be met and bite -- torch's fp32 CPU ops pass every checker on
every case of tests/test_depth_exact_gpu.py, five small mutations of that same result fail -- and the geometry of the
tiled backward's LDS window over every size it can meet."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import depth_ref as R
from tests import gn_ref as G
from tests import util

F64 = torch.float64


def test_ulp_bf16_is_gn_refs():
    a = torch.randn(4096, dtype=F64, generator=torch.Generator().manual_seed(1)) * 100
    assert torch.equal(R.ulp_bf16(a), G.ulp_bf16(a))


# --------------------------------------------------------------------------------------------------------------------
# references pinned
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,scale', [((2, 1, 3, 4, 5), 4), ((1, 1, 1, 1, 1), 2), ((1, 1, 5, 3, 7), 3),
                                         ((2, 1, 4, 1, 6), 1), ((1, 1, 3, 5, 1), 4)])
def test_head_reference_is_torchs_fp64_interpolate_softmax_and_autograd(shape, scale):
    g = torch.Generator().manual_seed(sum(shape) + scale)
    B, _, D, H, W = shape
    x = torch.randn(shape, generator=g, dtype=F64) * 3
    ds = R.depth_samples(D * scale)
    full = (B, 1, D * scale, H * scale, W * scale)
    gv, gs = torch.randn(full, generator=g, dtype=F64), torch.randn(full, generator=g, dtype=F64)
    gp = torch.randn((B, 1, H * scale, W * scale), generator=g, dtype=F64)
    xr = x.clone().requires_grad_(True)
    vol = F.interpolate(xr, scale_factor=scale, mode='trilinear', align_corners=True)
    soft = F.softmax(vol, dim=2)
    pred = torch.sum(soft * ds.double()[None, None, :, None, None], 2)
    rv, _, rs, rp = R.head_ref(x, ds, scale)
    for a, b in ((rv, vol), (rs, soft), (rp, pred)):
        assert torch.allclose(a, b.detach(), rtol=0, atol=1e-12)
    # the dense matrices the bounds are built from are the same map, forwards and transposed
    m = R.Mats(D, H, W, scale)
    assert torch.allclose(R.up3(x[:, 0], *m.m64), vol.detach()[:, 0], rtol=0, atol=1e-12)
    assert float(max(d.max() for d in m.dm)) <= 4 * max(D, H, W) * scale * R.U     # float32 weights: a few ulp of i
    torch.autograd.backward([vol, soft, pred], [gv, gs, gp])
    for sub in R.SUBSETS:
        grads = [t if k in sub else None for k, t in zip('vsp', (gv, gs, gp))]
        got, _ = R.head_grad(x, ds, scale, grads)
        x2 = x.clone().requires_grad_(True)
        v2 = F.interpolate(x2, scale_factor=scale, mode='trilinear', align_corners=True)
        s2 = F.softmax(v2, dim=2)
        p2 = torch.sum(s2 * ds.double()[None, None, :, None, None], 2)
        pairs = [(o, t) for o, t in zip((v2, s2, p2), grads) if t is not None]
        torch.autograd.backward([o for o, _ in pairs], [t for _, t in pairs])
        assert torch.allclose(got, x2.grad, rtol=0, atol=1e-12), sub
        # with the logits given as a leaf (bf16) it is the transposed upsample of d L / d logit: the same number
        # when the leaf holds the upsample itself
        got_leaf, gl = R.head_grad(x, ds, scale, grads, logits=v2.detach())
        assert torch.allclose(got_leaf, x2.grad, rtol=0, atol=1e-12), sub
        assert torch.allclose(R.up3_t(gl[:, 0], *m.m64), x2.grad[:, 0], rtol=0, atol=1e-12)


def test_up_index_float32_restatement():
    """against the exact index arithmetic: same cells except where the float32 product lands an ulp below an integer
    (then the weight is within that ulp of 1 and the two agree as maps), weights within a few ulp of the index"""
    for n_in, s in ((1, 2), (7, 4), (33, 2), (70, 1), (304, 4), (23, 3), (699, 8)):
        n_out = n_in * s
        i0, i1, w0, w1 = R.up_index(np.arange(n_out), n_in, n_out)
        assert w0.dtype == np.float32 and w1.dtype == np.float32
        assert i0.min() >= 0 and i1.max() <= n_in - 1 and np.all((i1 == i0 + 1) | (i1 == n_in - 1))
        assert np.all((w1 >= 0) & (w1 <= 1)) and np.all(w0 == np.float32(1) - w1)
        M32, M64 = R.up_matrix(n_in, n_out, False), R.up_matrix(n_in, n_out, True)
        assert float((M32 - M64).abs().max()) <= 4 * n_out * R.U
        assert torch.allclose(M64.sum(1), torch.ones(n_out, dtype=F64), rtol=0, atol=1e-15)
    i0, i1, w0, w1 = R.up_index(np.arange(2), 1, 2)
    assert list(i0) == [0, 0] and list(i1) == [0, 0] and list(w0) == [1, 1]


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(util.GOLDEN, 'depth_loss.npz'))


@pytest.mark.parametrize('loss_type', ['ce', 'balanced_ce', 'focal', 'balanced_focal', 'hard_ce', 'gaussian_1.5',
                                       'laplacian_2.0', 'focal_g3'])
def test_loss_reference_reproduces_the_reference_class_fixtures(gold, loss_type):
    """loss and d loss / d volumes of the REFERENCE class, to the fixtures' own fp32 noise"""
    key = loss_type.replace('.', 'p')
    lt, lw, alpha, gamma = loss_type, 0.7, 0.75, 2.0
    if loss_type == 'focal_g3':
        lt, lw, alpha, gamma = 'focal', 1.0, 1.0, 3.0
    ds, img = torch.from_numpy(gold['depth_samples']), torch.from_numpy(gold['depth_img'])
    vol = torch.from_numpy(gold['volumes']).double().requires_grad_(True)
    pix, mask = R.loss_ref(vol, img, ds, lt, 2, 59.6, alpha, gamma)
    total = R.total_ref(pix, mask, lt, lw, torch.from_numpy(gold['fgmask']), 5, 1)
    total.backward()
    np.testing.assert_allclose(float(total), float(gold[f'{key}_loss']), rtol=1e-5)
    g = gold[f'{key}_gvol']
    # (an element is a difference softmax_k A - p_k f'_k formed in fp32: where the two cancel, the fixture's noise is
    # an ulp or two of the terms, not of the element -- 1e-7 of the largest gradient)
    np.testing.assert_allclose(vol.grad.numpy(), g, rtol=1e-5, atol=1e-7 * float(np.abs(g).max()))


def test_dispatch_rule_puts_cases_on_both_kernels():
    tiles = {n: R.uses_tile_kernel(sh[2], sh[3], sh[4], s, sh[0]) for n, (sh, s, _) in R.BWD_SHAPES.items()}
    for n, (sh, s, tile) in R.BWD_SHAPES.items():
        assert tiles[n][0] == tile, n
    assert sum(t[0] for t in tiles.values()) >= 1 and sum(not t[0] for t in tiles.values()) >= 1
    assert tiles['scatter-scale1'][3] == 66528 and tiles['scatter-deep'][3] == 65664
    assert tiles['tile-scale1'][1:3] == (6, 66)
    assert all(sub in R.SUBSETS for sub in ('v', 's', 'p')) and len(R.SUBSETS) == 7
    # the existing backward fixtures all take the tile kernel (what this file's cases add to)
    for (d, h, w), s in (((6, 5, 9), 4), ((7, 9, 70), 4), ((5, 6, 40), 2)):
        assert R.uses_tile_kernel(d, h, w, s)[0]
    assert not R.uses_tile_kernel(42, 6, 66, 1)[0] and R.uses_tile_kernel(41, 6, 66, 1)[0]
    assert not R.uses_tile_kernel(304, 3, 18, 4)[0] and R.uses_tile_kernel(303, 3, 18, 4)[0]


@pytest.mark.parametrize('scale', [1, 2, 3, 4, 5, 8])
def test_tile_window_holds_every_tap(scale):
    """every h, w in 1..699: the four (h, w) taps of every output pixel of every 4 x 64 tile lie inside [0, nr) x
    [0, ncol) of the tile's window, relative to ih_lo / iw_lo -- per axis (the window is a product), with the float32
    up_index and the host's double nr / ncol"""
    for n in range(1, 700):
        _, nr, ncol, _ = R.uses_tile_kernel(1, n, n, scale)
        for tile, size in ((4, nr), (64, ncol)):
            o = np.arange(n * scale)
            i0, i1, _, _ = R.up_index(o, n, n * scale)
            lo = i0[(o // tile) * tile]                  # up_index(h0 / w0).i0 of the pixel's tile
            assert np.all(i0 >= lo) and np.all(i1 - lo < size), (n, scale, tile)
            # and what the write-back skips (ih >= H, iw >= W) holds no tap
            assert np.all(i1 < n)


# --------------------------------------------------------------------------------------------------------------------
# the bounds can be met: torch's fp32 CPU ops on every case of the GPU file
# --------------------------------------------------------------------------------------------------------------------
_FWD, _BWD, _LOSS, _FUSED, _TOT = R.fwd_params(), R.bwd_params(), R.loss_params(), R.fused_params(), R.total_params()
_ids = lambda ps: ['-'.join(str(v) for v in p) for p in ps]    # noqa: E731


@pytest.mark.parametrize('shape,content,dt', _FWD, ids=_ids(_FWD))
def test_torch_fp32_meets_every_bound_head_forward(shape, content, dt):
    sh, s = R.FWD_SHAPES[shape]
    bf16 = dt == 'bf16'
    cost = R.make_cost(sh, content, 40 + sorted(R.FWD_SHAPES).index(shape) * 8 + R.CONTENTS.index(content), bf16)
    ds = R.depth_samples(sh[2] * s)
    got = R.head_fp32(cost, ds, s, bf16)
    out = R.check_head(got, cost, ds, s, bf16, R.Mats(sh[2], sh[3], sh[4], s))
    assert set(out) >= {'soft', 'pred', 'col_max', 'col_sum'}
    v = got['vol'].double()[:, 0]
    t = v - v.amax(1, keepdim=True)
    if content == 'random30' and sh[2] > 1:   # the case is what it claims: entries below exp_nonpos's clamp, underflow
        assert float(t.min()) < -128.0 and bool(((t < -88.0) & (t > -128.0)).any())
    if content in ('rising', 'falling') and sh[2] > 1:
        d = v[:, 1:] - v[:, :-1]
        assert bool((d > 0).all()) if content == 'rising' else bool((d < 0).all())


@pytest.mark.parametrize('name,sub,dt', _BWD, ids=_ids(_BWD))
def test_torch_fp32_meets_every_bound_head_backward(name, sub, dt):
    bf16 = dt == 'bf16'
    cost, ds, s, grads = R.make_bwd(name, sub, bf16)
    got = R.head_fp32(cost, ds, s, bf16, grads)
    sh = cost.shape
    R.check_head_bwd(got['grad_cost'], cost, ds, s, grads, bf16, R.Mats(sh[2], sh[3], sh[4], s), got['vol'])


def _sigma_sides(cfg, img, ds, lt):
    if cfg.endswith('small'):
        assert R.sigma_side(img, ds, lt)[1] < 1.0
    if cfg.endswith('large'):
        assert R.sigma_side(img, ds, lt)[0] > 1.0


@pytest.mark.parametrize('shape,cfg,k,dt', _LOSS, ids=_ids(_LOSS))
def test_torch_fp32_meets_every_bound_loss(shape, cfg, k, dt):
    logits, img, ds, g_loss, lt, alpha, gamma = R.loss_case(shape, cfg, k, dt)
    _sigma_sides(cfg, img, ds, lt)
    got = R.loss_fp32(logits, img, ds, lt, alpha, gamma, g_loss, dt == 'bf16')
    R.check_loss(got, logits, img, ds, lt, alpha, gamma, g_loss, dt == 'bf16')


def test_loss_cases_hold_what_they_claim():
    logits, img, ds, g_loss, *_ = R.loss_case('wg-exact', 'ce', 2, 'fp32')
    mask = R.valid_mask(img)
    assert int(mask[1].sum()) == 0 and int(mask[0].sum()) > 0 and int(mask[2].sum()) > 0
    bv = R.border_values(ds)
    flat = img.reshape(-1)
    for v in bv:       # every border value is in the map; min / max depth themselves, 0, < 0, NaN, inf are invalid
        assert bool(((flat == v) | (torch.isnan(flat) & torch.isnan(v))).any())
    assert not bool(R.valid_mask(bv[[0, 1, 4, 5, 6, 7]]).any()) and bool(R.valid_mask(bv[[2, 3, 8, 9]]).all())
    zero = (g_loss == 0) & mask
    assert 0.2 <= float(zero.sum()) / float(mask.sum()) <= 0.3
    # the two half-way values sit exactly on hard_ce's threshold in fp32: p = 0.5 there, on either side of it nearby
    p32 = 1 - ((ds[None] - bv[8:, None]).abs() / (ds[1] - ds[0])).clamp(max=1.0)
    assert bool(((p32 - 0.5).abs() < 1e-5).any(1).all())
    x30 = R.loss_case('configK', 'ce', 30, 'fp32')[0]
    assert float(x30.max() - x30.min()) > 150        # saturated columns: a range of about +-90


@pytest.mark.parametrize('shape,cfg,k,dt', _FUSED, ids=_ids(_FUSED))
def test_torch_fp32_meets_every_bound_fused_loss(shape, cfg, k, dt):
    cost, img, ds, g_loss, s, lt, alpha, gamma = R.fused_case(shape, cfg, k, dt)
    bf16 = dt == 'bf16'
    _sigma_sides(cfg, img, ds, lt)
    sh = cost.shape
    vol = R.head_fp32(cost, ds, s, bf16)['vol'][:, 0]
    got = R.loss_fp32(vol, img, ds, lt, alpha, gamma, g_loss, False)
    R.check_loss(dict(loss=got['loss'], valid=got['valid']), vol, img, ds, lt, alpha, gamma, None, False)
    m32 = [R.up_matrix(n, n * s, False).float() for n in sh[2:]]
    gc = R.up3_t(got['grad'], *m32)[:, None]
    R.check_fused_grad(R._rnd(gc, bf16), cost, vol, img, ds, s, lt, alpha, gamma, g_loss, bf16,
                       R.Mats(sh[2], sh[3], sh[4], s))


@pytest.mark.parametrize('kind,lt,dt', _TOT, ids=_ids(_TOT))
def test_torch_fp32_meets_every_bound_total(kind, lt, dt):
    logits, img, ds, fg, cfg = R.total_case(kind, lt, dt)
    alpha, gamma = cfg.get('alpha', 1.0), cfg.get('gamma', 2.0)
    got = R.loss_fp32(logits, img, ds, lt, alpha, gamma, None, dt == 'bf16')
    pix, mask = got['loss'], got['valid']
    f, b = fg.bool() & mask, mask & ~fg.bool()
    total = cfg['loss_weight'] * cfg['loss_weight'] * (
        (cfg['fg_weight'] * (pix * f).sum() + cfg['bg_weight'] * (pix * b).sum()) / mask.sum())
    rpix, rmask = R.loss_ref(logits, img, ds, lt, alpha=alpha, gamma=gamma)
    want = R.total_ref(rpix, rmask, lt, cfg['loss_weight'], fg, cfg['fg_weight'], cfg['bg_weight'])
    bnd = R.loss_bounds(logits, img, ds, lt, alpha, gamma)
    R._ratio('total-' + dt, (total.double() - want).abs().reshape(1),
             R.total_bound(bnd['loss'], rpix, rmask, lt, cfg['loss_weight'], fg, cfg['fg_weight'],
                           cfg['bg_weight']).reshape(1))
    if kind == 'no-fg':
        assert not bool((fg.bool() & mask).any()) and bool(fg.bool().any())
    if kind == 'no-bg':
        assert not bool((mask & ~fg.bool()).any())
    if kind == 'box-ids':
        assert float(fg.max()) > 1
    if kind == 'empty-sample':
        assert int(mask[1].sum()) == 0


# --------------------------------------------------------------------------------------------------------------------
# the bounds bite: five small mutations of torch's fp32 result
# --------------------------------------------------------------------------------------------------------------------
def _loss_mut(shape, cfg, mutate, match, k=2):
    logits, img, ds, g_loss, lt, alpha, gamma = R.loss_case(shape, cfg, k, 'fp32')
    R.check_loss(R.loss_fp32(logits, img, ds, lt, alpha, gamma, g_loss, False), logits, img, ds, lt, alpha, gamma,
                 g_loss, False)
    with pytest.raises(AssertionError, match=match):
        R.check_loss(R.loss_fp32(logits, img, ds, lt, alpha, gamma, g_loss, False, mutate=mutate), logits, img, ds, lt,
                     alpha, gamma, g_loss, False)


def test_mutation_last_depth_bin_left_out_of_the_log_sum_exp():
    _loss_mut('configK', 'ce', 'lse_last_bin', 'loss-fp32')        # one of 288 bins


def test_mutation_pixel_at_max_depth_counted_valid():
    _loss_mut('wg2', 'ce', 'max_depth_valid', 'validity mask')


def test_mutation_second_term_of_the_focal_derivative_dropped():
    logits, img, ds, g_loss, lt, alpha, gamma = R.loss_case('wg-exact', 'focal-g2', 2, 'fp32')
    bad = R.loss_fp32(logits, img, ds, lt, alpha, gamma, g_loss, False, mutate='focal_second_term')
    R.check_loss(dict(bad, grad=None), logits, img, ds, lt, alpha, gamma, g_loss, False)   # the loss itself is right
    with pytest.raises(AssertionError, match='grad_vol-fp32'):
        R.check_loss(bad, logits, img, ds, lt, alpha, gamma, g_loss, False)


def test_mutation_gaussian_normaliser_without_its_clamp():
    _loss_mut('wg2', 'gaussian-small', 'no_clamp', 'loss-fp32')


@pytest.mark.parametrize('name', ['tile-last2', 'tile-scale3'])
def test_mutation_one_tap_dropped_for_the_last_tile_column(name):
    """the (i1, i1, i1) tap of the transposed upsample left out for the output pixels of the last column tile"""
    cost, ds, s, grads = R.make_bwd(name, 'vsp', False)
    sh = cost.shape
    Wo = sh[4] * s
    cols = torch.arange((Wo - 1) // 64 * 64, Wo)
    m = R.Mats(sh[2], sh[3], sh[4], s)
    good = R.head_fp32(cost, ds, s, False, grads)
    R.check_head_bwd(good['grad_cost'], cost, ds, s, grads, False, m, good['vol'])
    bad = R.head_fp32(cost, ds, s, False, grads, taps=(cols, (1,)))
    assert 0 < int((bad['grad_cost'] != good['grad_cost']).sum())
    with pytest.raises(AssertionError, match='grad_cost-fp32'):
        R.check_head_bwd(bad['grad_cost'], cost, ds, s, grads, False, m, bad['vol'])
