"""Helpers of the exact GroupNorm tests (csrc/group_norm.hip): plain fp64 restatements of what the kernels compute
-- moments per (sample, group), y = relu?(x a + b + residual), the backward (d beta, d gamma, dx, d residual) -- the
slice geometry of the launches (which voxels a workgroup owns, to read the statistics partials), and checkers whose
bounds follow from the number formats, the fp64 reference and the LENGTH OF THE CHAIN of fp32 operations a value passes
through, counted from the kernel source (the ``chain_*`` functions, one comment per number).  Never from what a kernel
returned.

Everything is torch fp64 on the device of its arguments (the CPU tests pin it to torch's own fp64 GroupNorm + autograd;
the GPU tests run the same code on the device, which keeps the 33 M element cases quick).  Tensors are taken in their
logical (N, C, *spatial) shape whatever their memory layout: ``ncs`` flattens them to (N, C, S) fp64, so one reference
serves the planar and the channels-last kernels; the layouts differ in the slice geometry and the chain lengths only.

A checker returns max(error / bound) and asserts it is <= 1; ``WORST`` keeps the largest ratio seen per checker."""
import math

import torch

U = 2.0 ** -24          # unit roundoff of fp32: one rounded operation is off by at most U * |result|
F64 = torch.float64
WORST = {}


def ncs(t):
    """(N, C, *spatial) tensor of any dtype / layout -> (N, C, S) fp64, logical order"""
    return t.detach().to(F64).reshape(t.shape[0], t.shape[1], -1)


def per_channel(stat, C):
    """(N, G) -> (N, C, 1): the statistic of the group each channel is in"""
    return stat.to(F64).repeat_interleave(C // stat.shape[1], dim=1)[:, :, None]


def ulp_bf16(a):
    """spp_ref.ulp_bf16 for a torch fp64 tensor on any device (pinned to it in tests/test_gn_ref.py)"""
    _, e = torch.frexp(a)
    return torch.where(a == 0, torch.zeros_like(a), torch.ldexp(torch.ones_like(a), e - 8))


def moments(x, groups):
    """biased (mean, var) per (sample, group) of x (N, C, S) fp64 -> two (N, G)"""
    xg = x.reshape(x.shape[0], groups, -1)
    mean = xg.mean(2)
    return mean, ((xg - mean[:, :, None]) ** 2).mean(2)


def affine(mean, rstd, gamma, beta):
    """(a, b) (N, C, 1) fp64 of y = x a + b: a = rstd gamma, b = beta - mean a.  With fp32 statistics (a kernel's) the
    product rstd * gamma is rounded to fp32 first -- ONE correctly rounded IEEE operation that every kernel performs as
    written (the library is built with -ffp-contract=off), so it is the same number everywhere; left in fp64, its
    rounding error times the group mean would enter b, a magnitude the apply bound does not list.  fp64 statistics
    (the reference's own): all fp64."""
    C = gamma.numel()
    if rstd.dtype == torch.float32:
        a = (rstd.repeat_interleave(C // rstd.shape[1], dim=1) * gamma.to(torch.float32)[None]).to(F64)[:, :, None]
    else:
        a = per_channel(rstd, C) * gamma.to(F64)[None, :, None]
    return a, beta.to(F64)[None, :, None] - per_channel(mean, C) * a


def apply(x, mean, rstd, gamma, beta, res=None):
    """(pre, mag): pre = x a + b + res before the ReLU, mag = |x a| + |b| + |res| the magnitudes that enter it"""
    a, b = affine(mean, rstd, gamma, beta)
    xa = x * a
    pre, mag = xa + b, xa.abs() + b.abs()
    if res is not None:
        pre, mag = pre + res, mag + res.abs()
    return pre, mag


def backward(x, g, mean, rstd, gamma, groups):
    """the GroupNorm backward for g = dy behind the ReLU mask, (N, C, S) fp64, with the given statistics:
    dbeta[c] = sum g, dgamma[c] = sum g xhat, dx = rstd (gamma g - (A + xhat B) / L), A = sum_group gamma g,
    B = sum_group gamma g xhat, L = cpg S; d residual is g itself.  Also the sums of magnitudes the bounds use."""
    N, C, S = x.shape
    cpg = C // groups
    mu, rs = per_channel(mean, C), per_channel(rstd, C)
    xh = (x - mu) * rs
    gam = gamma.to(F64)[None, :]
    s1, s2 = g.sum(2), (g * xh).sum(2)                       # (N, C)
    m1, m2 = g.abs().sum(2), (g * xh).abs().sum(2)
    grp = lambda t: t.reshape(N, groups, cpg).sum(2)         # noqa: E731
    A, B = grp(s1 * gam), grp(s2 * gam)
    MA, MB = grp(m1 * gam.abs()), grp(m2 * gam.abs())
    raw = ((g * x).abs() + (mu * g).abs()).sum(2) * rs[:, :, 0]     # the terms of rstd (sum g x - mean sum g)
    L = float(cpg * S)
    Am, Bm = per_channel(A, C) / L, per_channel(B, C) / L
    dx = rs * (gam[:, :, None] * g - Am - xh * Bm)
    return dict(dbeta=s1.sum(0), dgamma=s2.sum(0), dx=dx, xh=xh, rs=rs, mu=mu, Am=Am, Bm=Bm,
                abs_dbeta=m1.sum(0), abs_dgamma=m2.sum(0), MA=per_channel(MA, C) / L, MB=per_channel(MB, C) / L,
                raw_dgamma=raw.sum(0), MBraw=per_channel(grp(raw * gam.abs()), C) / L)


# --------------------------------------------------------------------------------------------------------------------
# launch geometry (restated from the host code of csrc/group_norm.hip; the partial counts check it against the kernels)
# --------------------------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def cl_splits(S, C):
    """pick_splits_cl: workgroups per sample of the channels-last statistics and apply passes"""
    return min(max(S * C // 16384, 1), 2048)


def cl_bwd_splits(S, C):
    """min(GN_BW_SPLITS, pick_splits_cl): workgroups per sample of the channels-last backward's statistics pass"""
    return min(cl_splits(S, C), 1024)


def cl_slices(S, splits):
    """[lo, hi) voxels of every workgroup: per = ceil(S / splits), clamped to S (the last ones may be empty)"""
    per = cdiv(S, splits)
    return [(min(s * per, S), min(min(s * per, S) + per, S)) for s in range(splits)]


def planar_splits(L):
    """pick_splits: workgroups per group (forward, L = cpg S) or per channel (backward, L = S) of the planar kernels"""
    return min(max(L // 32768, 1), 256)


def planar_slices(L, splits, vec):
    """slice_of: [lo, hi) elements of the group's L, in whole 16-byte vectors"""
    per = cdiv(cdiv(L, vec), splits) * vec
    return [(min(s * per, L), min(min(s * per, L) + per, L)) for s in range(splits)]


# --------------------------------------------------------------------------------------------------------------------
# chain lengths.  A sum whose terms pass through at most d additions is off by at most d U sum|terms|; a product or a
# quotient adds one U of its own magnitude.  n_abs counts roundings of numbers as large as the data (|mean| + D, D the
# group's largest deviation from its mean), n_dev roundings of differences of two data values (at most 2 D), n_var
# roundings on the way to the second moment, whose terms are (v - K)^2 with K any value of the group (the shift of the
# channels-last sums, the reference mean of the merge): (v - K)^2 <= 2 (v - mean)^2 + 2 (K - mean)^2, at most
# var + 4 D^2 per element on average (var <= D^2).
# --------------------------------------------------------------------------------------------------------------------
def chain_cl(S, C, groups, vec):
    """gn_stats_cl_kernel + gn_merge_partials_kernel -> dict(n_abs, n_dev, n_var)"""
    nvb, cpg, splits = C // vec, C // groups, cl_splits(S, C)
    vpi = 256 // nvb
    steps = cdiv(cdiv(S, splits), vpi)                 # additions into a lane's s1 / s2: its voxels of the slice
    shfl = max(int(math.log2(64 // nvb)), 0)           # __shfl_xor steps o = 32 .. nvb
    n_sum = steps + shfl + 4                           # + the four waves through LDS
    mp = cdiv(splits, 256) + 6 + 4                     # merge_partials_256: strided loop, wave shuffle, four waves
    n_abs = (1                                         # shK[c] + a
             + (cpg - 1)                               # merge() of the group's channels: a.mean + delta f, in sequence
             + 1)                                      # ref + a
    n_dev = (1 + n_sum + 1                             # d = v - K; the sum; a = a1 / cnt
             + 3 * (cpg - 1)                           # merge(): delta, f = b.n / r.n, delta f
             + 2 + mp + 1)                             # d = mean_i - ref, n d; S1; a = S1 / N
    n_var = ((2 + n_sum)                               # d's rounding enters d d twice; fma sum
             + (1 + n_sum + 1 + 1) + 1                 # a1, a = a1 / cnt, a1 a; a2 - a1 a
             + 7 * (cpg - 1)                           # merge(): delta (twice), delta^2, a.n, f, two additions
             + (2 + 1 + 1 + 2 * cdiv(splits, 256) + 10)   # d (twice), n d, (n d) d; S2 += M2_i + ..: two additions a step
             + (2 + mp + 1 + 1) + 1)                   # S1, a = S1 / N, S1 a; S2 - S1 a
    return dict(n_abs=n_abs, n_dev=n_dev, n_var=n_var)


def chain_planar(L, vec):
    """gn_stats_kernel + the merge at the head of gn_apply_kernel -> dict(n_abs, n_dev, n_var)"""
    splits = planar_splits(L)
    steps = cdiv(cdiv(cdiv(L, vec), splits), 256)      # vectors a thread merges into its running moments
    merges = steps + 6 + 3 + splits                    # thread, wave_merge, block_merge, the partials in sequence
    n_abs = (vec                                       # sm = sum of the vector's raw values (vec - 1), sm / n
             + merges)                                 # merge(): a.mean + delta f
    n_dev = 3 * merges                                 # merge(): delta, f, delta f
    n_var = (2 + vec                                   # f - mean_v (twice), the vector's sum of squares
             + 7 * merges)                             # merge(): as in chain_cl
    return dict(n_abs=n_abs, n_dev=n_dev, n_var=n_var)


def chain_bwd_cl(S, C, vec, N):
    """gn_bwd_stats_cl_kernel + gn_bwd_coef_kernel: additions a term of sum g / sum g xhat passes through, per
    (sample, channel) and in all (the parameter gradients add the samples in sequence)"""
    nvb, splits = C // vec, cl_bwd_splits(S, C)
    nc = (cdiv(cdiv(S, splits), 256 // nvb)            # a lane's voxels of the slice
          + 256 // nvb                                 # the lanes of a channel vector, in sequence through LDS
          + cdiv(splits, 64) + 6)                      # gn_bwd_coef_kernel: strided loop, wave shuffle
    return dict(nc=nc, total=nc + N)


def chain_bwd_planar(S, N):
    """gn_bwd_stats_kernel + the head of gn_bwd_apply_kernel (atomicAdd over the samples)"""
    splits = planar_splits(S)
    nc = cdiv(cdiv(S, splits), 256) + 6 + 4 + splits   # a thread's elements, wave shuffle, four waves, the partials
    return dict(nc=nc, total=nc + N)


def chain_torch_cpu(S, cpg, N):
    """ATen's CPU GroupNorm in fp32 (the proof that the bounds can be met): RowwiseMoments is a Welford update per SIMD
    lane, mean += (x - mean) / k, in chunks of 16 vectors merged pairwise (a binary cascade, then the lanes): a value
    passes through at most 16 updates of its chunk, log2 of the number of chunks and log2 of the lane count merges --
    each one rounding at the level of the data and three at the level of a deviation, seven on the way to M2; the
    backward's sums run per channel over S in SIMD lanes, at most S additions deep.  The counts are taken with room:
    this is the yardstick's own arithmetic, not the code under test."""
    depth = 16 + max(int(math.ceil(math.log2(max(cpg * S, 2)))), 1) + 4
    return (dict(n_abs=depth, n_dev=3 * depth, n_var=7 * depth + 4), dict(nc=S + cpg, total=S + cpg + N))


# --------------------------------------------------------------------------------------------------------------------
# checkers
# --------------------------------------------------------------------------------------------------------------------
def _ratio(name, err, bound):
    """max(err / bound) with 0 / 0 = 0 and x / 0 = inf; recorded, asserted <= 1"""
    err, bound = err.to(F64), bound.to(F64)
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    worst = float(r.max()) if r.numel() else 0.0
    worst = worst if worst == worst else float('inf')   # (a NaN anywhere is a failure)
    WORST[name] = max(WORST.get(name, 0.0), worst)
    assert worst <= 1.0, f'{name}: error / bound = {worst:.4g} (max error {float(err.max()):.4g}, ' \
                         f'{int((err > bound).sum())} of {err.numel()} over their bound)'
    return worst


def partial_mean_dev_cl(x, groups, slices):
    """(N, G): the largest distance of a (channel, slice) mean from its group's mean -- the partial means that the
    channels-last statistics merge (gn_stats_cl_kernel's channels, gn_merge_partials_kernel's slices)"""
    N, C, S = x.shape
    per = slices[0][1] - slices[0][0]
    pad = torch.full((N, C, per * len(slices) - S), float('nan'), dtype=F64, device=x.device)
    pm = torch.cat([x, pad], 2).reshape(N, C, len(slices), per).nanmean(3)        # an empty slice: NaN
    mean = x.reshape(N, groups, -1).mean(2)
    dev = (pm - per_channel(mean, C)).abs().nan_to_num(0.0)
    return dev.reshape(N, groups, -1).amax(2)


def stats_bounds(x, groups, eps, chain, Dm=None):
    """(mean, var, mean bound, relative rstd bound) (N, G) fp64 from the exact input values.  Dm (N, G): the largest
    distance of a partial mean from the group's mean, where the partition is known (default D: any partial mean)."""
    mean, var = moments(x, groups)
    D = (x.reshape(x.shape[0], groups, -1) - mean[:, :, None]).abs().amax(2)
    Dm = D if Dm is None else Dm
    E = U * chain['n_abs'] * (mean.abs() + D)           # what the roundings at the level of the data leave in a mean
    b_mean = E + U * chain['n_dev'] * 2 * D
    # the second moment: its own chain on terms of at most var + 4 D^2 per element, and the partial means' errors e_i,
    # |e_i| <= E, carried into it by the merges: a term n_i (m_i - ref)^2 with |m_i - ref| <= 2 Dm moves by at most
    # n_i (2 (2 Dm) (2 E) + (2 E)^2), and S1^2 / N <= sum n_i (m_i - ref)^2 by as much again
    b_var = U * chain['n_var'] * (var + 4 * D * D) + 16 * Dm * E + 8 * E * E
    # rstd = 1 / sqrt(m2 / n + eps): the quotient and the sum under the root count half, the root and the reciprocal
    # whole: 3 U on top of half the relative error of var + eps
    return mean, var, b_mean, 0.5 * b_var / (var + eps) + 3 * U


def check_stats(x, groups, eps, got_mean, got_rstd, chain, Dm=None, tag=''):
    """a kernel's fp32 mean / rstd (N, G) against the fp64 moments of x (N, C, S)"""
    mean, var, b_mean, b_rstd = stats_bounds(x, groups, eps, chain, Dm)
    rstd = 1.0 / torch.sqrt(var + eps)
    n, g = mean.shape
    r1 = _ratio('mean' + tag, (got_mean.to(F64).reshape(n, g) - mean).abs(), b_mean)
    r2 = _ratio('rstd' + tag, (got_rstd.to(F64).reshape(n, g) - rstd).abs() / rstd, b_rstd)
    return max(r1, r2)


def check_partial_counts(partials, slices, per_voxel):
    """forward partials (N, G, splits, 3) of a statistics pass: every count is per_voxel * (slice length) exactly,
    the counts add up to the group, empty slices are (0, 0, 0)"""
    p = partials.detach().cpu().to(F64)
    want = torch.tensor([per_voxel * (hi - lo) for lo, hi in slices], dtype=F64)
    assert p.shape[2] == len(slices)
    assert torch.equal(p[..., 0], want.expand_as(p[..., 0])), 'a partial count is not its slice'
    assert bool((p[..., 0].sum(2) == per_voxel * slices[-1][1]).all()) and slices[-1][1] == max(h for _, h in slices)
    empty = want == 0
    assert bool((p[:, :, empty] == 0).all()), 'an empty slice must be (0, 0, 0)'
    assert bool(torch.isfinite(p).all())
    return int(empty.sum())


def check_apply(x, gamma, beta, res, relu, got_y, got_mean, got_rstd, bf16, tag=''):
    """y against the fp64 value of relu?(x a + b + res) built from the kernel's OWN mean / rstd (N, G) fp32: elementwise,
    bound 3 U (|x a| + |b| + |res|) -- the roundings of b, of x a + b and of the residual's addition, each at most U of
    a partial result that the three magnitudes bound -- plus half a bf16 ulp where y is stored in bf16.  Where |pre|
    exceeds its bound the kernel's y > 0 must agree with pre > 0 (the mask of the backward)."""
    pre, mag = apply(x, got_mean, got_rstd, gamma, beta, res)
    bound = 3 * U * mag
    want = pre.clamp_min(0) if relu else pre
    y = ncs(got_y)
    full = bound + (0.5 * ulp_bf16(want.abs() + bound) if bf16 else 0.0)
    r = _ratio('y' + ('-bf16' if bf16 else '-fp32') + tag, (y - want).abs(), full)
    if relu:
        sure = pre.abs() > bound
        assert bool(((y > 0) == (pre > 0))[sure].all()), 'sign of y against the fp64 value outside its bound'
    return r


def check_backward(x, dy, mask, gamma, groups, got_mean, got_rstd, got, cb, bf16, exact_dbeta=False, tag='',
                   raw_sums=False):
    """dbeta, dgamma (fp32 (C)), dx and optionally dres (storage dtype) in ``got`` against the fp64 backward with the
    kernel's own mean / rstd and the mask of the kernel's own forward output.  cb: chain_bwd_*.  raw_sums: the
    implementation forms dgamma as rstd (sum g x - mean sum g), as ATen's CPU kernel does, not as sum g xhat: terms as
    large as the data enter it (and B, through it dx), and its bounds carry them (the HIP kernels' do not)."""
    N, C, S = x.shape
    cpg = C // groups
    g = dy * mask
    ref = backward(x, g, got_mean, got_rstd, gamma, groups)
    out = {}
    if exact_dbeta:   # 'grid' inputs: every partial sum is an integer below 2^24, exact in fp32 in any order
        assert float(ref['abs_dbeta'].max()) < 2.0 ** 24
        assert torch.equal(got['dbeta'].to(F64), ref['dbeta']), 'dbeta of exact-grid inputs must be exact'
        out['dbeta'] = 0.0
    else:
        out['dbeta'] = _ratio('dbeta' + tag, (got['dbeta'].to(F64) - ref['dbeta']).abs(),
                              cb['total'] * U * ref['abs_dbeta'])
    # + 3: x - mu, * rs, g * xhat
    b_dgamma = (cb['total'] + 3) * U * ref['abs_dgamma']
    if raw_sums:
        b_dgamma = b_dgamma + (cb['total'] + 3) * U * ref['raw_dgamma']
    out['dgamma'] = _ratio('dgamma' + tag, (got['dgamma'].to(F64) - ref['dgamma']).abs(), b_dgamma)
    # dx = k1 g + k2 x + k3, k1 = rs gamma, k2 = -rs rs Bm, k3 = rs (rs mu Bm - Am) (gn_bwd_coef_kernel; the planar
    # kernel's rs (gamma g - Am - xhat Bm) has the same terms without the two that carry mu).  Longest chain, through
    # Bm = B invL: invL = 1 / (cpg S) 2, the product 1; k2: rs rs, * Bm 2; k2 x 1; the two additions 2 = 8; k3 has
    # 3 + 4 and the last addition.  Magnitudes entering: |k1 g|, |k2 x|, rs rs |mu Bm|, rs |Am|.
    rs, mu, gam = ref['rs'], ref['mu'], gamma.to(F64)[None, :, None]
    elem = 8 * U * ((rs * gam * g).abs() + (rs * rs * ref['Bm'] * x).abs() + (rs * rs * mu * ref['Bm']).abs()
                    + (rs * ref['Am']).abs())
    # the two group sums as the kernel has them: per (sample, channel) chain, * gamma 1, the group's channels cpg;
    # B's terms carry xhat's three roundings
    MB = ref['MB'] + ref['MBraw'] if raw_sums else ref['MB']
    prop = rs * U * ((cb['nc'] + 1 + cpg) * ref['MA'] + (cb['nc'] + 4 + cpg) * MB * ref['xh'].abs())
    bound = elem + prop
    if bf16:
        bound = bound + 0.5 * ulp_bf16(ref['dx'].abs() + bound)
    out['dx'] = _ratio('dx' + ('-bf16' if bf16 else '-fp32') + tag, (ncs(got['dx']) - ref['dx']).abs(), bound)
    if got.get('dres') is not None:   # the masked gradient itself: no arithmetic
        assert torch.equal(ncs(got['dres']), g), 'dres is dy behind the mask, exactly'
    return out


# --------------------------------------------------------------------------------------------------------------------
# inputs
# --------------------------------------------------------------------------------------------------------------------
KINDS = ('random', 'grid', 'off100', 'off1000', 'outlier', 'neggamma', 'zerochan', 'eps3')


def make_inputs(N, C, sp, kind, seed, bf16, outlier_at=0):
    """CPU tensors of one case, planar: x, dy, res (N, C, *sp) fp32 holding values of the storage type, gamma, beta (C)
    fp32, eps.  'random': x = 2 randn + 0.7.  'grid': x, dy, res integers in [-3, 3], gamma powers of two, beta
    quarters -- every partial sum of dbeta is an integer.  'off100' / 'off1000': x = offset + 0.01 randn (fp32).
    'outlier': the voxel ``outlier_at`` (the first of a middle slice) of every channel at mean + 50 sigma.
    'neggamma': gamma < 0.  'zerochan': two channels with gamma = beta = 0.  'eps3': eps = 1e-3."""
    assert kind in KINDS
    g = torch.Generator().manual_seed(seed)
    shape = (N, C) + tuple(sp)
    if kind == 'grid':
        x, dy, res = (torch.randint(-3, 4, shape, generator=g).float() for _ in range(3))
        gamma = 2.0 ** torch.randint(-1, 2, (C,), generator=g).float()
        beta = torch.randint(-4, 5, (C,), generator=g).float() / 4
    else:
        x = torch.randn(shape, generator=g) * 2 + 0.7
        if kind in ('off100', 'off1000'):
            assert not bf16
            x = torch.randn(shape, generator=g) * 0.01 + (100.0 if kind == 'off100' else 1000.0)
        dy, res = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
        gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
        if kind == 'outlier':
            x.reshape(N, C, -1)[:, :, outlier_at] = 0.7 + 50 * 2.0
        if kind == 'neggamma':
            gamma = -gamma.abs()
        if kind == 'zerochan':
            gamma[[C // 2, C - 1]] = 0.0
            beta[[C // 2, C - 1]] = 0.0
    if bf16:
        x, dy, res = (t.bfloat16().float() for t in (x, dy, res))
    return dict(x=x, dy=dy, res=res, gamma=gamma, beta=beta, eps=1e-3 if kind == 'eps3' else 1e-5)


def torch_fp32(inp, groups, relu, with_res, bf16):
    """torch's fp32 CPU GroupNorm forward / backward on a case's values: what a correct fp32 implementation returns
    (y, dx, dres rounded to bf16 where the kernels store bf16)"""
    x = inp['x'].clone().requires_grad_(True)
    w, b = inp['gamma'].clone().requires_grad_(True), inp['beta'].clone().requires_grad_(True)
    r = inp['res'].clone().requires_grad_(True) if with_res else None
    N, C = x.shape[:2]
    S = x.numel() // (N * C)
    y, mean, rstd = torch.native_group_norm(x, w, b, N, C, S, groups, inp['eps'])
    y = y if r is None else y + r
    y = torch.relu(y) if relu else y
    y.backward(inp['dy'])
    rnd = (lambda t: t.bfloat16().float()) if bf16 else (lambda t: t)
    return dict(y=rnd(y.detach()), mean=mean.detach(), rstd=rstd.detach(), dx=rnd(x.grad), dgamma=w.grad,
                dbeta=b.grad, dres=None if r is None else rnd(r.grad))


def check_all(inp, groups, relu, with_res, bf16, got, chain, cb, exact_dbeta=False, backward_too=True, dev=None,
              Dm=None, raw_sums=False):
    """every checker on one implementation's results ``got`` (y, mean, rstd, dx, dgamma, dbeta, dres)"""
    to = (lambda t: t.to(dev)) if dev is not None else (lambda t: t)
    x, dy = ncs(to(inp['x'])), ncs(to(inp['dy']))
    res = ncs(to(inp['res'])) if with_res else None
    gamma, beta = to(inp['gamma']), to(inp['beta'])
    out = dict(stats=check_stats(x, groups, inp['eps'], got['mean'], got['rstd'], chain, Dm),
               y=check_apply(x, gamma, beta, res, relu, got['y'], got['mean'].reshape(x.shape[0], groups),
                             got['rstd'].reshape(x.shape[0], groups), bf16))
    if backward_too:
        yk = ncs(got['y'])
        mask = (yk > 0).to(F64) if relu else torch.ones_like(yk)
        out.update(check_backward(x, dy, mask, gamma, groups, got['mean'].reshape(x.shape[0], groups),
                                  got['rstd'].reshape(x.shape[0], groups), got, cb, bf16, exact_dbeta,
                                  raw_sums=raw_sums))
    return out


# --------------------------------------------------------------------------------------------------------------------
# the cases (shared by the CPU proof in tests/test_gn_ref.py and the GPU tests)
# --------------------------------------------------------------------------------------------------------------------
SPECIAL = ('off100', 'off1000', 'outlier', 'neggamma', 'zerochan', 'eps3')
MODES = {'plain': (False, False), 'res': (False, True), 'relu': (True, False), 'relures': (True, True)}  # relu, residual


def _cl_cases():
    """channels-last cases by name: N, C per dtype, groups, S, kinds beyond ('random', 'grid'), dtypes, modes, whether
    the backward runs"""
    out, k = {}, 0

    def add(name, C, groups, S, special=False, dtypes=('fp32', 'bf16'), modes=tuple(MODES), backward=True, N=None):
        nonlocal k
        out[name] = dict(N=N or 1 + k % 3, C=C, groups=groups, S=S, special=special, dtypes=dtypes, modes=modes,
                         backward=backward)
        k += 1
    # one vector block: nvb = 1, vpi = 256, the wave shuffle down to 1; slices shorter than one vpi step; the U = 4 /
    # U = 2 unroll boundary (a lane's 4th / 2nd vector is voxel 768 / 256 + its own) and one either side
    for gsel in ('1', 'C'):
        for S in (1, 3, 255, 256, 257, 1023, 1024, 1025):
            add(f'block-g{gsel}-S{S}', {'fp32': 4, 'bf16': 8}, gsel, S, special=(gsel == '1' and S == 1025))
    # widest: nvb = 64 (fp32: vpi = 4, no shuffle), group borders inside a lane's vector (cpg = 1), one group of 256
    # channels (gn_bwd_coef_kernel's cc += 64 loop); 129 voxels = slices of 65 + 64; 4481: 70 slices, the last one empty
    for groups in (1, 32, 256):
        for S in (3, 129, 4481):
            add(f'widest-g{groups}-S{S}', 256, groups, S, special=(groups == 32 and S == 4481))
    for C in (32, 64, 128):
        for S in (2 * 3 * 5, 9 * 7 * 13, 18 * 20 * 41):
            add(f'shipped-C{C}-S{S}', C, 32, S, special=(C, S) in ((32, 819), (64, 14760)))
    # 257 partials per group: merge_partials_256's strided loop takes a second step in thread 0
    add('partials257', 32, 32, 257 * 16384 // 32, special=True, N=1)
    # 1025 apply slices against 1024 statistics slices in the backward: the two passes cut the tensor differently
    add('bwd1025', 32, 32, 524803, dtypes=('bf16',), modes=('plain', 'relu', 'relures'), N=1)
    # the 2048-split cap of the forward: S C / 16384 = 2048.01 reaches it, 2049.0 is clamped by it
    add('cap2048', 32, 32, 1048583, dtypes=('bf16',), modes=('plain', 'relures'), backward=False, N=1)
    add('cap2048-over', 32, 32, 1049095, dtypes=('bf16',), modes=('relures',), backward=False, N=1)
    return out


CL_CASES = _cl_cases()


def cl_params():
    """(case, dtype, mode, kind) of every channels-last test"""
    out = []
    for name, c in CL_CASES.items():
        for dt in c['dtypes']:
            for kind in ('random', 'grid'):
                out += [(name, dt, m, kind) for m in c['modes']]
            if c['special']:
                for kind in SPECIAL:
                    if not (dt == 'bf16' and kind.startswith('off')):
                        out += [(name, dt, m, kind) for m in ('plain', 'relu')]
    return out


def cl_case(name, dt, kind):
    """(N, C, groups, S, vec, inputs) of a channels-last case"""
    c = CL_CASES[name]
    C = c['C'][dt] if isinstance(c['C'], dict) else c['C']
    groups = {'1': 1, 'C': C}.get(c['groups'], c['groups'])
    S, vec = c['S'], 4 if dt == 'fp32' else 8
    splits = cl_splits(S, C)
    seed = 1 + sorted(CL_CASES).index(name) * 16 + KINDS.index(kind) * 2 + (dt == 'bf16')
    inp = make_inputs(c['N'], C, (S,), kind, seed, dt == 'bf16', outlier_at=cl_slices(S, splits)[splits // 2][0])
    return c['N'], C, groups, S, vec, inp


# planar (NC(D)HW) cases: N, C, groups, S -- spatial % VEC != 0 (misaligned group starts, the scalar path), L < VEC,
# a group of two slices (L = 65542: 32772 + 32770 elements in fp32, 32776 + 32766 in bf16, the last vector partial),
# groups 1 and C
PLANAR_CASES = {'odd-g1': (2, 6, 1, 35), 'odd-gC': (2, 6, 6, 35), 'odd-g2': (3, 6, 2, 63), 'tiny-gC': (2, 3, 3, 3),
                'tiny-g1': (1, 2, 1, 3), 'aligned': (2, 8, 2, 64), 'twoslices': (2, 4, 2, 32771),
                'twoslices-gC': (1, 2, 2, 65539)}


def planar_params():
    return [(name, dt, m, kind) for name in PLANAR_CASES for dt in ('fp32', 'bf16') for kind in ('random', 'grid')
            for m in ('plain', 'relu')]


def planar_case(name, dt, kind):
    N, C, groups, S = PLANAR_CASES[name]
    seed = 7000 + sorted(PLANAR_CASES).index(name) * 8 + KINDS.index(kind) * 2 + (dt == 'bf16')
    return N, C, groups, S, 4 if dt == 'fp32' else 8, make_inputs(N, C, (S,), kind, seed, dt == 'bf16')
