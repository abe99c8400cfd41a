"""Helpers of the exact depth-head / depth-loss tests (csrc/depth_head.hip, csrc/depth_loss.hip): plain fp64
restatements of what the kernels compute -- the trilinear upsample with align_corners=True, the softmax over depth and its
expectation (``head_ref``), the per-pixel depth-distribution losses of DepthHead.loss (``loss_ref``) and its reductions
(``total_ref``) --, per-element error bounds, torch fp32 restatements of the same operations (the proof that the bounds
can be met) and the case tables shared by tests/test_depth_ref.py (CPU) and tests/test_depth_exact_gpu.py.

Everything is torch fp64 on the device of its arguments.  A checker returns max(error / bound) and asserts it is <= 1;
``WORST`` keeps the largest ratio seen per checker.

How a bound is made.  U = 2^-24 is the unit roundoff of fp32: one rounded operation is off by at most U |result|.  A sum
of n terms, in any order (the atomics have none), is off by at most n U sum|terms|.  Every count below is read from the
kernel source and has a comment; every magnitude is a sum of absolute values of the fp64 terms (sum_d p_d |f(lp_d)| for
a loss, sum |w gl| for a scattered gradient).  A value stored in bf16 adds half a bf16 ulp.  Never from what a kernel
returned.

The elementary functions have no count to read: each gets an allowance in ulp (ULP = 2^-23 relative: an ulp of a value
is between 2^-24 and 2^-23 of it), named below.  They were not fixed in advance: they are the smallest integers for
which torch's fp32 CPU restatement of the same operation (``head_fp32``, ``loss_fp32``) passes every checker on every
case of the GPU file -- tests/test_depth_ref.py runs that.  The search starts at 1, because no allowance can be 0: the
correctly rounded result is already half an ulp off.  All five passed at 1, so none had to be raised.  (Set to 0 one at
a time, expf fails -- hard_ce at logits x30 --, so its 1 is needed; the other four still pass at 0, on the slack of the
counted roundings around them, which says nothing about the functions.)

The floor of a saturated entry.  exp_nonpos clamps its argument at -128 and returns 0 below it (2^-185 is out of range),
where the exact value is at most e^-128 = 2.6e-56; between e^-87.3 (FLT_MIN = 2^-126) and there the result is a
denormal, which the hardware may round to a multiple of 2^-149 or flush to 0.  Either way the ABSOLUTE error of an
exponential is at most FLOOR = 2^-126 whatever its relative bound says; a column sum is >= 1 (its maximum contributes
exp(0) = 1 exactly), so 1 / sum <= 1 and a probability inherits the floor, once more for its own product: 2 FLOOR.  The
loss kernel's expf has the same range; its floors are carried the same way.  The same holds for any fp32 product that
lands below 2^-126 (a gradient of a saturated column does): the gradients carry one FLOOR per product on their way."""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24            # unit roundoff of fp32
ULP = 2.0 ** -23          # the largest relative size of one fp32 ulp
FLOOR = 2.0 ** -126       # FLT_MIN: the absolute error of an exponential in or below the denormal range
F64 = torch.float64
F32 = torch.float32
WORST = {}

# ulp allowances of the elementary functions (see above: the smallest integers >= 1 that torch's fp32 CPU ops need)
EXPNP_ULP = 1             # exp_nonpos (dfm_common.h), the depth head's softmax
EXPF_ULP = 1              # expf, the loss kernel
LOGF_ULP = 1              # logf, the loss kernel's log-sum-exp
POWF_ULP = 1              # powf, the generic focal branch (gamma not in {0, 1, 2})
RCP_ULP = 1               # the 1 / sum reciprocal (depth head: one division per column; loss: 1 / max(psum, 1))

MIN_DEPTH, MAX_DEPTH = 2.0, 59.6


def ulp_bf16(a):
    """gn_ref.ulp_bf16: spacing of the bf16 values in the binade of a (0 for 0)"""
    _, e = torch.frexp(a)
    return torch.where(a == 0, torch.zeros_like(a), torch.ldexp(torch.ones_like(a), e - 8))


def _ratio(name, err, bound):
    """gn_ref._ratio: max(err / bound) with 0 / 0 = 0 and x / 0 = inf; recorded, asserted <= 1"""
    err, bound = err.to(F64), bound.to(F64).expand_as(err)
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    worst = float(r.max()) if r.numel() else 0.0
    worst = worst if worst == worst else float('inf')   # (a NaN anywhere is a failure)
    WORST[name] = max(WORST.get(name, 0.0), worst)
    assert worst <= 1.0, f'{name}: error / bound = {worst:.4g} (max error {float(err.max()):.4g}, ' \
                         f'{int((err > bound).sum())} of {err.numel()} over their bound)'
    return worst


def _stored(bound, want, bf16):
    """+ half a bf16 ulp where the result is stored in bf16 (below 2^-126 a bf16 value is a multiple of 2^-133, or
    flushed: FLOOR covers both)"""
    return bound + 0.5 * ulp_bf16(want.abs() + bound) + FLOOR if bf16 else bound


def depth_samples(D):
    """bin centres of [MIN_DEPTH, MAX_DEPTH] (mode 'UD'), fp32"""
    interval = (MAX_DEPTH - MIN_DEPTH) / D
    return torch.tensor([(k + 0.5) * interval + MIN_DEPTH for k in range(D)], dtype=F32)


# --------------------------------------------------------------------------------------------------------------------
# the upsample: up_index in float32 (a faithful copy of dfm_common.h:178-192), its exact counterpart, dense 1-D matrices
# --------------------------------------------------------------------------------------------------------------------
def up_index(i, n_in, n_out):
    """(i0, i1, w0, w1) of output indices ``i`` (array), every operation in numpy.float32 as the device code has it"""
    f = np.float32
    i = np.asarray(i, np.int64)
    scale = f(n_in - 1) / f(n_out - 1) if n_out > 1 else f(0.0)
    real = (scale * i.astype(f)).astype(f)
    a = np.minimum(np.floor(real).astype(np.int64), n_in - 1)
    lam = np.minimum(np.maximum((real - a.astype(f)).astype(f), f(0.0)), f(1.0))
    return a, np.minimum(a + 1, n_in - 1), (f(1.0) - lam).astype(f), lam


def up_index_exact(i, n_in, n_out):
    """the same in exact arithmetic: quotient and remainder in integers, the weights in fp64"""
    i = np.asarray(i, np.int64)
    if n_out == 1:
        a, lam = np.zeros_like(i), np.zeros(i.shape, np.float64)
    else:
        num = i * (n_in - 1)
        a, lam = num // (n_out - 1), (num % (n_out - 1)).astype(np.float64) / (n_out - 1)
    a = np.minimum(a, n_in - 1)
    return a, np.minimum(a + 1, n_in - 1), 1.0 - lam, lam


def up_matrix(n_in, n_out, exact, taps=(0, 1)):
    """(n_out, n_in) fp64: row o holds the weights of output o (both on one cell where i1 == i0).  ``taps``: which of
    the two taps to keep (a mutation of tests/test_depth_ref.py drops one)"""
    i0, i1, w0, w1 = (up_index_exact if exact else up_index)(np.arange(n_out), n_in, n_out)
    M = np.zeros((n_out, n_in), np.float64)
    if 0 in taps:
        np.add.at(M, (np.arange(n_out), i0), w0.astype(np.float64))
    if 1 in taps:
        np.add.at(M, (np.arange(n_out), i1), w1.astype(np.float64))
    return torch.from_numpy(M)


class Mats:
    """the three axes' matrices of one (D, H, W, scale): exact (m64), the kernel's float32 weights (m32), their
    distance (dm) and, per input cell, how many outputs reach it (cnt)"""

    def __init__(self, D, H, W, s, dev='cpu'):
        self.m64 = [up_matrix(n, n * s, True).to(dev) for n in (D, H, W)]
        self.m32 = [up_matrix(n, n * s, False).to(dev) for n in (D, H, W)]
        self.dm = [(a - b).abs() for a, b in zip(self.m32, self.m64)]
        c = [(m != 0).to(F64).sum(0) for m in self.m32]
        self.cnt = c[0][:, None, None] * c[1][None, :, None] * c[2][None, None, :]     # (D, H, W)


def up3(x, A, B, C):
    """(B, D, H, W) -> (B, Do, Ho, Wo) through three 1-D matrices"""
    return torch.einsum('bdhw,Dd,Hh,Ww->bDHW', x, A, B, C)


def up3_t(g, A, B, C):
    """the transposed map, (B, Do, Ho, Wo) -> (B, D, H, W)"""
    return torch.einsum('bDHW,Dd,Hh,Ww->bdhw', g, A, B, C)


def _weight_err(fn, t, m):
    """|fn(t, m32...) - fn(t, m64...)| bounded term by term: m32 x m32 x m32 - m64 x m64 x m64 telescopes into
    dm x m32 x m32 + m64 x dm x m32 + m64 x m64 x dm, exactly"""
    a = t.abs()
    return (fn(a, m.dm[0], m.m32[1], m.m32[2]) + fn(a, m.m64[0], m.dm[1], m.m32[2])
            + fn(a, m.m64[0], m.m64[1], m.dm[2]))


def logit_err(x, m):
    """(B, Do, Ho, Wo): how far an fp32 logit of the kernels is from the fp64 upsample of x (B, D, H, W).  Three nested
    lerp_fma(w0, a, w1, b) = fma(w0, a, w1 * b): two roundings each, U (|w0 a| + |w1 b|) apiece -> 6 U of the upsampled
    |x|; plus the distance of the float32 weights from the exact ones."""
    return 6 * U * up3(x.abs(), *m.m32) + _weight_err(up3, x, m)


# --------------------------------------------------------------------------------------------------------------------
# depth head: reference and bounds
# --------------------------------------------------------------------------------------------------------------------
def head_ref(cost, ds, scale, logits=None):
    """cost (B, 1, D, H, W), ds (Do) -> (vol, logit, soft, pred) in fp64 with torch's own ops: vol = trilinear
    upsample with align_corners=True of cost (it carries the graph back to ``cost``), soft = softmax over depth of
    ``logit``, pred = sum soft ds.  logit is vol itself, or -- bf16 -- a LEAF holding the volume the kernel stored
    (``logits``): backward through soft / pred then leaves d L / d logit in logit.grad, and vol.backward of it is the
    fp64 transposed upsample (``head_grad`` does both)."""
    B, _, D, H, W = cost.shape
    vol = F.interpolate(cost.to(F64), size=(D * scale, H * scale, W * scale), mode='trilinear', align_corners=True)
    logit = vol if logits is None else logits.detach().to(F64).clone().requires_grad_(True)
    soft = F.softmax(logit, dim=2)
    pred = (soft * ds.to(F64)[None, None, :, None, None]).sum(2)
    return vol, logit, soft, pred


def head_grad(cost, ds, scale, grads, logits=None):
    """d / d cost (fp64) and d / d logit for the incoming gradients ``grads`` = (g_vol, g_soft, g_pred), any of them
    None, by autograd"""
    x = cost.detach().to(F64).clone().requires_grad_(True)
    vol, logit, soft, pred = head_ref(x, ds, scale, logits)
    gv, gs, gp = (None if g is None else g.detach().to(F64) for g in grads)
    outs = [(o, g) for o, g in ((soft, gs), (pred, gp)) if g is not None]
    if logits is None:
        outs += [(vol, gv)] if gv is not None else []
        torch.autograd.backward([o for o, _ in outs], [g for _, g in outs], inputs=[x])
        return x.grad, None
    gl = torch.zeros_like(logit)
    if outs:
        torch.autograd.backward([o for o, _ in outs], [g for _, g in outs], inputs=[logit])
        gl = logit.grad
    gl = gl if gv is None else gl + gv
    vol.backward(gl, inputs=[x])
    return x.grad, gl


def _softmax_terms(v, E, online):
    """p, and the relative bounds of one exponential's share and of the column sum, for logits v (B, Do, Ho, Wo) fp64
    known to E (tensor or 0.0).  online: the forward's sum (chunks of 8, rescaled when the maximum moved), else the
    backward's plain one."""
    Do = v.shape[1]
    t = v - v.amax(1, keepdim=True)
    p = F.softmax(v, dim=1)
    Emax = E.amax(1, keepdim=True) if torch.is_tensor(E) else 0.0
    # one exponential: the rounded difference logit - max moves the argument by U |t| (the maximum itself may be
    # another logit within E: 2 Emax more of |t|), exp_nonpos its allowance
    one = U * (t.abs() + 2 * Emax) + EXPNP_ULP * ULP
    nch = -(-Do // 8)
    if online:
        # a term is rescaled by exp_nonpos(mx - mnew) once per later chunk at most: the arguments of these add up to
        # at most |t| again (2 U |t| in all), nch more allowances, nch products; then Do additions
        ssum = (p * (2 * U * t.abs())).sum(1, keepdim=True) + (nch + 1) * EXPNP_ULP * ULP + (nch + Do) * U
    else:
        ssum = (p * one).sum(1, keepdim=True) + Do * U
    # logits known to E only: p' / p = e^(d_k) / sum_j p_j e^(d_j) lies within e^(+-(E_k + Emax))
    known = torch.expm1(E + Emax) if torch.is_tensor(E) else 0.0
    return p, t, one, ssum, known, Emax


def head_bounds(v, E, ds, bf16):
    """bounds of soft (B, Do, Ho, Wo), pred (B, Ho, Wo), col_max, col_sum of dfm_depth_head_fwd / _stats_fwd against
    the softmax of the fp64 logits v"""
    p, t, one, ssum, known, Emax = _softmax_terms(v, E, True)
    Do = v.shape[1]
    # p = exp_nonpos(v - mx) * (1 / sum): the exponential, the sum, the reciprocal, the product
    b_soft = p * (one + ssum + RCP_ULP * ULP + U + known) + 2 * FLOOR
    dsa = ds.to(F64).abs()[None, :, None, None]
    # acc += soft * ds: a product and Do additions on terms |p ds|, and what the (stored) probabilities are off by
    b_pred = (_stored(b_soft, p, bf16) * dsa).sum(1) + (Do + 1) * U * (p * dsa).sum(1)
    S = torch.exp(t).sum(1)
    two = torch.expm1(2 * Emax[:, 0]) if torch.is_tensor(E) else 0.0
    b_sum = S * (ssum[:, 0] + two) + Do * FLOOR
    return dict(soft=_stored(b_soft, p, bf16), pred=_stored(b_pred, (p * dsa).sum(1), bf16), col_sum=b_sum,
                col_max=Emax[:, 0] if torch.is_tensor(E) else torch.zeros_like(S), S=S, p=p)


def check_head(got, cost, ds, scale, bf16, m, tag=''):
    """``got``: vol, soft, pred (any may be missing), col_max, col_sum of the kernels.  fp32: against the fp64 upsample
    of cost, the logits known to logit_err; bf16: against the softmax of the stored volume got['vol'] exactly."""
    dev = cost.device
    x = cost.detach().to(F64)
    dt = '-bf16' if bf16 else '-fp32'
    vol, logit, soft, pred = head_ref(x, ds.to(dev), scale, got['vol'] if bf16 else None)
    v = logit.detach()[:, 0]
    E = 0.0 if bf16 else logit_err(x[:, 0], m)
    b = head_bounds(v, E, ds.to(dev), bf16)
    out = {}
    if not bf16 and got.get('vol') is not None:
        out['vol'] = _ratio('vol' + dt + tag, (got['vol'].to(F64)[:, 0] - v).abs(), E)
    if got.get('soft') is not None:
        out['soft'] = _ratio('soft' + dt + tag, (got['soft'].to(F64)[:, 0] - soft.detach()[:, 0]).abs(), b['soft'])
    if got.get('pred') is not None:
        out['pred'] = _ratio('pred' + dt + tag, (got['pred'].to(F64)[:, 0] - pred.detach()[:, 0]).abs(), b['pred'])
    if got.get('col_max') is not None:
        out['col_max'] = _ratio('col_max' + dt + tag, (got['col_max'].to(F64) - v.amax(1)).abs(), b['col_max'])
        out['col_sum'] = _ratio('col_sum' + dt + tag, (got['col_sum'].to(F64) - b['S']).abs(), b['col_sum'])
    return out


def scatter_bound(gl, dgl, m):
    """bound of sum_o w(o, c) gl_o per input cell c (B, D, H, W), gl known to dgl: what the terms are off by, the sum
    of n = cnt(c) terms in no fixed order (atomics) -- + 8 for the roundings on a term's way (gl * w_d, the (h, w)
    weight product, its product with the depth-reduced sum, and up to four tiles' partial sums meeting in memory; the
    scatter kernel has three products and nothing else) --, and the float32 weights' distance from the exact ones"""
    return (up3_t(dgl, *m.m32) + (m.cnt[None] + 8) * (U * up3_t(gl.abs(), *m.m32) + FLOOR)
            + _weight_err(up3_t, gl, m))


def head_bwd_bound(v, E, ds, grads, m, bf16, ref):
    """bound of dfm_depth_head_bwd's grad_cost (B, D, H, W) against ``ref`` (fp64), both kernels.
    gl_d = g_vol_d + p_d (s_d - dot), s_d = g_soft_d + g_pred ds_d, dot = sum_k p_k s_k"""
    gv, gs, gp = (None if g is None else g.detach().to(F64) for g in grads)
    zero = torch.zeros_like(v)
    gl, dgl = (zero if gv is None else gv[:, 0]), zero
    if gs is not None or gp is not None:
        p, t, one, ssum, known, _ = _softmax_terms(v, E, False)
        Do = v.shape[1]
        rp = one + ssum + U + known                       # p = exp_nonpos(.) / sum: + the division
        dsd = ds.to(F64)[None, :, None, None]
        a_soft = zero if gs is None else gs[:, 0]
        a_pred = zero if gp is None else gp[:, 0][:, None] * dsd
        s, smag = a_soft + a_pred, a_soft.abs() + a_pred.abs()
        d_s = U * (a_soft.abs() + 2 * a_pred.abs())       # the product g_pred ds, the addition
        dot, dotmag = (p * s).sum(1, keepdim=True), (p * smag).sum(1, keepdim=True)
        # dot += p * sd: the product and Do additions, p's own error, s's
        d_dot = (p * ((rp + (Do + 1) * U) * smag + d_s)).sum(1, keepdim=True) + 2 * FLOOR * smag.sum(1, keepdim=True)
        # p * (sd - dot): the difference is absolute in |s| + |dot|; the product; then + g_vol
        soft_gl = p * (s - dot)
        dgl = (p * ((rp + 2 * U) * (s - dot).abs() + d_s + d_dot + U * (smag + dotmag))
               + 2 * FLOOR * (smag + dotmag))
        gl = gl + soft_gl
        dgl = dgl + U * gl.abs()
    return _stored(scatter_bound(gl, dgl, m), ref, bf16)


def check_head_bwd(got, cost, ds, scale, grads, bf16, m, vol=None, tag='', out_bf16=None):
    """grad_cost of the kernels against fp64 autograd; bf16: at the stored logits ``vol``.  out_bf16: whether ``got``
    was rounded to bf16 (default: as the inputs; the C entry point itself returns fp32)"""
    out_bf16 = bf16 if out_bf16 is None else out_bf16
    dev = cost.device
    ref, _ = head_grad(cost, ds.to(dev), scale, grads, vol if bf16 else None)
    x = cost.detach().to(F64)
    v = vol.detach().to(F64)[:, 0] if bf16 else up3(x[:, 0], *m.m64)
    E = 0.0 if bf16 else logit_err(x[:, 0], m)
    bound = head_bwd_bound(v, E, ds.to(dev), grads, m, out_bf16, ref[:, 0])
    return _ratio('grad_cost' + ('-bf16' if bf16 else '-fp32') + tag, (got.to(F64)[:, 0] - ref[:, 0]).abs(), bound)


def uses_tile_kernel(d, h, w, scale, batch=1):
    """the host rule of dfm_depth_head_bwd: the tiled kernel when the input window of a 4 x 64 output tile fits 64 KiB
    of LDS.  Returns (tile?, nr, ncol, bytes)"""
    Ho, Wo = h * scale, w * scale
    sh = (h - 1) / (Ho - 1) if Ho > 1 else 0.0          # C doubles
    sw = (w - 1) / (Wo - 1) if Wo > 1 else 0.0
    nr, ncol = min(h, int(3 * sh) + 3), min(w, int(63 * sw) + 3)
    lds = d * nr * ncol * 4
    return lds <= 64 * 1024 and batch <= 65535 and (Ho + 3) // 4 <= 65535, nr, ncol, lds


# --------------------------------------------------------------------------------------------------------------------
# depth loss: reference and bounds
# --------------------------------------------------------------------------------------------------------------------
def parse_loss(loss_type):
    """-> (target kind, sigma as the kernel holds it (fp32), focal?)"""
    if loss_type in ('ce', 'balanced_ce', 'focal', 'balanced_focal'):
        return 'linear', 0.0, 'focal' in loss_type
    if loss_type == 'hard_ce':
        return 'hard', 0.0, False
    kind, sigma = loss_type.split('_')
    assert kind in ('gaussian', 'laplacian')
    return kind, float(np.float32(float(sigma))), False


def valid_mask(depth_img, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH):
    """depth_head.py:89 in fp32, as the reference evaluates it"""
    img = depth_img.to(F32)
    return (img > min_depth) & (img < max_depth)


def _target(gt, ds, kind, sigma):
    """the soft target over the bins for gt (n) fp32, ds (D) fp32 -> dict(p (n, D) fp64, raw, psum, dist, r).  fp64 on
    the fp32 inputs; the steps in fp32 as the reference has them: interval = ds[1] - ds[0], and hard_ce's threshold."""
    interval = (ds[1] - ds[0]).to(F64)                                   # an fp32 difference, then exact
    dist = (ds.to(F64)[None] - gt.to(F64)[:, None]).abs()
    out = dict(dist=dist, interval=interval)
    if kind in ('linear', 'hard'):
        r = dist / interval
        p = 1 - r.clamp(max=1.0)
        if kind == 'hard':
            p32 = 1 - ((ds[None] - gt[:, None]).abs() / (ds[1] - ds[0])).clamp(max=1.0)      # fp32 throughout
            p = (p32 >= 0.5).to(F64)
        out.update(p=p, r=r)
    else:
        arg = -0.5 * dist ** 2 / sigma ** 2 if kind == 'gaussian' else -dist / sigma
        raw = torch.exp(arg)
        psum = raw.sum(1, keepdim=True)
        out.update(p=raw / psum.clamp(min=1.0), raw=raw, psum=psum, arg=arg)
    return out


def _focal(lp, alpha, gamma):
    return alpha * (1 - lp.exp()) ** gamma * lp


def loss_ref(logits, depth_img, ds, loss_type, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, alpha=1.0, gamma=2.0):
    """(per-pixel loss (B, H, W) fp64, 0 at invalid pixels; mask (B, H, W) bool): depth_head.py:89-182 before the
    reductions, for logits (B, D, H, W).  The log-softmax and everything after it in fp64 (differentiable w.r.t.
    logits, if they require it)."""
    kind, sigma, focal = parse_loss(loss_type)
    mask = valid_mask(depth_img, min_depth, max_depth)
    x = logits.to(F64).permute(0, 2, 3, 1)[mask]                         # (n, D)
    tg = _target(depth_img.to(F32)[mask], ds.to(F32), kind, sigma)
    lp = F.log_softmax(x, dim=1)
    f = _focal(lp, alpha, gamma) if focal else lp
    out = torch.zeros(mask.shape, dtype=F64, device=x.device)
    return out.masked_scatter(mask, -(tg['p'] * f).sum(1)) if x.requires_grad else \
        out.masked_scatter_(mask, -(tg['p'] * f).sum(1)), mask


def total_ref(pix, mask, loss_type, loss_weight, fgmask=None, fg_weight=1.0, bg_weight=1.0):
    """the reductions of DepthHead.loss (depth_head.py:118-186): the mean over the valid pixels, or the fg / bg
    weighted sum over n; loss_weight applied twice (:186).  None where no pixel is valid."""
    n = int(mask.sum())
    if n == 0:
        return None
    if 'balanced' in loss_type:
        fg = fgmask.bool() & mask
        loss = (fg_weight * pix[fg].sum() + bg_weight * pix[mask & ~fg].sum()) / n
    else:
        loss = pix[mask].sum() / n
    return loss_weight * loss_weight * loss


def loss_bounds(logits, depth_img, ds, loss_type, alpha=1.0, gamma=2.0, g_loss=None, bf16=False, g_rel=0.0):
    """per-element bounds of depth_loss_kernel: 'loss' (B, H, W) and, with g_loss (B, H, W), 'grad' (B, D, H, W) (the
    materialised kernel's gradient volume, stored in the logits' type) and 'gl' / 'dgl' (the fused kernel's fp32 logit
    gradient and its bound, before the transposed upsample).  The logits are exact inputs (stored values)."""
    kind, sigma, focal = parse_loss(loss_type)
    mask = valid_mask(depth_img)
    dev = logits.device
    x = logits.detach().to(F64).permute(0, 2, 3, 1)[mask]
    n, D = x.shape
    tg = _target(depth_img.to(F32)[mask], ds.to(F32), kind, sigma)
    p = tg['p']
    # ---- log-sum-exp, online: se = se * expf(mx - x) + 1 when the maximum moves, else se += expf(x - mx)
    mx = x.amax(1, keepdim=True)
    t = x - mx
    sm = F.softmax(x, dim=1)
    run = torch.cummax(x, 1).values
    n_up = (run[:, 1:] > run[:, :-1]).sum(1, keepdim=True).to(F64)       # rescales of the running sum
    # a term: its own expf and one per later rescale, the arguments' roundings add up to 2 U |t|; a product and an
    # addition per rescale, D additions
    rel_se = (n_up + 1) * (EXPF_ULP * ULP + 2 * U) + D * U + (sm * 2 * U * t.abs()).sum(1, keepdim=True) + D * FLOOR
    lse = mx + torch.log(torch.exp(t).sum(1, keepdim=True))
    d_lse = rel_se + LOGF_ULP * ULP * (lse - mx).abs() + U * lse.abs()    # logf, mx + logf
    lp = F.log_softmax(x, dim=1)        # (not x - lse: in a saturated column that rounds to 0 even in fp64)
    d_lp = d_lse + U * lp.abs()
    # ---- target
    if kind == 'linear':     # |ds - gt|, / interval, 1 - .: absolute 3 U around the bins it reaches
        rel_p, abs_p = torch.zeros_like(p), 3 * U * (tg['r'] < 1 + 1e-6).to(F64)
    elif kind == 'hard':     # the fp32 expressions themselves: 0 or 1
        rel_p, abs_p = torch.zeros_like(p), torch.zeros_like(p)
    else:
        # the argument: gaussian (d, d d, -0.5 d d, s s, /) 6 U, laplacian (d, /) 2 U of |arg|; expf; the sum of D
        # terms; max(., 1) is 1-Lipschitz; the reciprocal; the product
        rel_t = (6 if kind == 'gaussian' else 2) * U * tg['arg'].abs() + EXPF_ULP * ULP
        den = tg['psum'].clamp(min=1.0)
        rel_p = rel_t + ((tg['raw'] * rel_t).sum(1, keepdim=True) + D * U * tg['psum'] + D * FLOOR) / den \
            + RCP_ULP * ULP + U
        abs_p = torch.full_like(p, 2 * FLOOR)
    # ---- f(lp), f'(lp)
    one = torch.ones_like(lp)
    if not focal:
        f, df, d_f, d_df = lp, one, d_lp, torch.zeros_like(lp)
    else:
        pr = lp.exp()
        om = 1 - pr
        d_pr = pr * (d_lp + EXPF_ULP * ULP) + FLOOR
        d_om = d_pr + U * om
        hi = om + d_om

        def power(g):        # (om^g, its absolute bound): dl_pow's shortcuts, else powf
            if g == 0:
                return one, torch.zeros_like(om)
            if g == 1:
                return om, d_om
            rel = U if g == 2 else POWF_ULP * ULP
            return om ** g, g * hi ** (g - 1) * d_om + rel * om ** g
        w_, d_w_ = power(gamma)
        W, d_W = alpha * w_, alpha * (d_w_ + U * w_)
        f = W * lp
        d_f = d_W * lp.abs() + W * d_lp + U * f.abs()
        if gamma == 0:
            dw, d_dw = torch.zeros_like(om), torch.zeros_like(om)
        else:
            q, d_q = power(gamma - 1)
            dw = alpha * gamma * q * pr                                   # alpha * gamma * pow * pr: three products
            d_dw = alpha * gamma * (d_q * pr + q * d_pr) + 3 * U * dw
        df = W - dw * lp
        d_df = d_W + d_dw * lp.abs() + dw * d_lp + 2 * U * (W.abs() + (dw * lp).abs())
    # ---- loss -= p * f over the bins with p != 0
    nz = (p != 0).sum(1, keepdim=True).to(F64)
    b_loss = (((rel_p + (nz + 1) * U) * p + abs_p) * f.abs() + p * d_f + FLOOR).sum(1)
    out = dict(loss=torch.zeros(mask.shape, dtype=F64, device=dev).masked_scatter_(mask, b_loss), mask=mask)
    if g_loss is None:
        return out
    gp = g_loss.detach().to(F64)[mask][:, None]
    A, Amag = (p * df).sum(1, keepdim=True), (p * df.abs()).sum(1, keepdim=True)
    d_A = (((rel_p + (nz + 1) * U) * p + abs_p) * df.abs() + p * d_df).sum(1, keepdim=True)
    # grad = gp * (expf(lp) * A - p * df)
    d_sm = sm * (d_lp + EXPF_ULP * ULP) + FLOOR
    t1, t2 = sm * A, p * df
    d_t1 = d_sm * Amag + sm * d_A + U * (sm * Amag)
    d_t2 = ((rel_p + U) * p + abs_p) * df.abs() + p * d_df
    gl = gp * (t1 - t2)
    # (four products that may underflow: expf(lp) * A, p * df, their difference times gp, and p = target * pnorm)
    dgl = gp.abs() * (d_t1 + d_t2 + 2 * U * (t1.abs() + t2.abs())) + g_rel * gl.abs() + 4 * FLOOR
    B, H, W_ = mask.shape

    def vol(cols):
        full = torch.zeros(B, H, W_, D, dtype=F64, device=dev)
        full[mask] = cols
        return full.permute(0, 3, 1, 2)
    out.update(gl=vol(gl), dgl=vol(dgl))
    out['grad'] = _stored(out['dgl'], out['gl'], bf16)
    return out


def loss_grad_ref(logits, depth_img, ds, loss_type, alpha, gamma, g_loss):
    """d (sum g_loss * pixel loss) / d logits by fp64 autograd"""
    x = logits.detach().to(F64).clone().requires_grad_(True)
    pix, _ = loss_ref(x, depth_img, ds, loss_type, alpha=alpha, gamma=gamma)
    pix.backward(g_loss.detach().to(F64))
    return x.grad


def check_loss(got, logits, depth_img, ds, loss_type, alpha, gamma, g_loss, bf16, tag='', g_rel=0.0):
    """``got``: loss (B, H, W), valid (B, H, W) and optionally grad (B, D, H, W) of the materialised kernels"""
    dt = '-bf16' if bf16 else '-fp32'
    pix, mask = loss_ref(logits.detach(), depth_img, ds, loss_type, alpha=alpha, gamma=gamma)
    assert torch.equal(got['valid'].bool(), mask), 'the validity mask is the fp32 expression, exactly'
    b = loss_bounds(logits, depth_img, ds, loss_type, alpha, gamma, g_loss, bf16, g_rel)
    out = dict(loss=_ratio('loss' + dt + tag, (got['loss'].to(F64) - pix).abs(), b['loss']))
    if got.get('grad') is not None:
        ref = loss_grad_ref(logits, depth_img, ds, loss_type, alpha, gamma, g_loss)
        out['grad'] = _ratio('grad_vol' + dt + tag, (got['grad'].to(F64) - ref).abs(), b['grad'])
    return out


def check_fused_grad(got, cost, vol, depth_img, ds, scale, loss_type, alpha, gamma, g_loss, bf16, m, tag=''):
    """grad_cost (B, 1, cd, ch, cw) of dfm_depth_loss_fused_bwd: the fp64 transposed upsample of the fp64
    d loss / d logit at the kernel's stored logits ``vol`` (B, D, H, W)"""
    b = loss_bounds(vol, depth_img, ds, loss_type, alpha, gamma, g_loss, False)
    gl = loss_grad_ref(vol, depth_img, ds, loss_type, alpha, gamma, g_loss)
    ref = up3_t(gl, *m.m64)
    bound = _stored(scatter_bound(gl, b['dgl'], m), ref, bf16)
    return _ratio('grad_cost_fused' + ('-bf16' if bf16 else '-fp32') + tag, (got.to(F64)[:, 0] - ref).abs(), bound)


def total_bound(b_pix, pix, mask, loss_type, loss_weight, fgmask=None, fg_weight=1.0, bg_weight=1.0):
    """bound of DepthHead.loss's scalar: the pixels' bounds through the same weights, and torch's fp32 reductions over
    the (B, H, W) map -- N pixels deep at most, with room: that is the yardstick's arithmetic, not a kernel's"""
    n = int(mask.sum())
    w = torch.ones_like(pix)
    if 'balanced' in loss_type:
        fg = fgmask.bool() & mask
        w = torch.where(fg, fg_weight * w, bg_weight * w)
    w = w * mask
    return loss_weight ** 2 * ((w * b_pix).sum() + (pix.numel() + 8) * U * (w * pix.abs()).sum()) / n


# --------------------------------------------------------------------------------------------------------------------
# torch's fp32 CPU ops on the same values: what a correct fp32 implementation returns
# --------------------------------------------------------------------------------------------------------------------
def _rnd(t, bf16):
    return t.bfloat16().float() if bf16 else t


def head_fp32(cost, ds, scale, bf16, grads=None, taps=None):
    """cost (B, 1, D, H, W) fp32 (bf16 values where bf16) -> vol, soft, pred, col_max, col_sum and, with grads,
    grad_cost: the upsample through the float32 weights of up_index (einsum in fp32), torch's fp32 softmax, sum and
    autograd; results rounded to bf16 where the kernels store bf16.  taps (per axis): a mutation."""
    B, _, D, H, W = cost.shape
    m32 = [up_matrix(n, n * scale, False).float() for n in (D, H, W)]
    x = cost.float().clone().requires_grad_(True)
    vol = up3(x[:, 0], *m32)[:, None]
    if bf16:   # the softmax reads the stored volume
        vol = vol + (vol.detach().bfloat16().float() - vol.detach())
    mx = vol.detach().amax(2)
    soft = F.softmax(vol, dim=2)
    soft_st = soft + (_rnd(soft.detach(), bf16) - soft.detach())
    pred = (soft_st * ds.float()[None, None, :, None, None]).sum(2)
    out = dict(vol=vol.detach(), soft=soft_st.detach(), pred=_rnd(pred.detach(), bf16), col_max=mx[:, 0],
               col_sum=torch.exp(vol.detach() - mx[:, None]).sum(2)[:, 0])
    if grads is not None:
        pairs = [(o, g.float()) for o, g in zip((vol, soft, pred), grads) if g is not None]
        torch.autograd.backward([o for o, _ in pairs], [g for _, g in pairs])
        gx = x.grad
        if taps is not None:   # the same gradient with some taps' contributions left out for some output columns
            cols, drop = taps
            gx = gx - _dropped(out, cost, ds, scale, grads, cols, drop)
        out['grad_cost'] = _rnd(gx, bf16)
    return out


def _dropped(out, cost, ds, scale, grads, cols, drop):
    """what the (i1, i1, i1) tap (``drop``) of the output columns ``cols`` adds to grad_cost, in fp32"""
    B, _, D, H, W = cost.shape
    _, gl = head_grad(cost, ds, scale, grads, out['vol'])
    sel = torch.zeros(W * scale, dtype=F64)
    sel[cols] = 1.0
    mats = [up_matrix(n, n * scale, False, taps=drop) for n in (D, H, W)]
    mats[2] = mats[2] * sel[:, None]
    return up3_t(gl[:, 0], *mats)[:, None].float()


def loss_fp32(logits, depth_img, ds, loss_type, alpha, gamma, g_loss, bf16, mutate=None):
    """the reference's own lines (depth_head.py:89-182) in torch fp32 on the CPU, per pixel, and autograd for
    g_loss: loss, valid, grad (rounded to bf16 where the kernels store bf16).  ``mutate``: one of the small errors of
    tests/test_depth_ref.py ('lse_last_bin', 'max_depth_valid', 'focal_second_term', 'no_clamp')."""
    kind, sigma, focal = parse_loss(loss_type)
    img, ds = depth_img.to(F32), ds.to(F32)
    mask = (img > MIN_DEPTH) & (img < MAX_DEPTH)
    if mutate == 'max_depth_valid':
        mask = (img > MIN_DEPTH) & (img <= MAX_DEPTH)
    x = logits.float().clone().requires_grad_(True)
    cost = x.permute(0, 2, 3, 1)[mask]
    gt = img[mask]
    if mutate == 'lse_last_bin':
        lp = cost - torch.logsumexp(cost[:, :-1], 1, keepdim=True)
    else:
        lp = F.log_softmax(cost, dim=1)
    interval = ds[1] - ds[0]
    dist = torch.abs(ds - gt.unsqueeze(-1))
    if kind in ('linear', 'hard'):
        prob = 1 - (dist / interval).clamp(max=1.0)
        if kind == 'hard':
            prob = (prob >= 0.5).float()
    else:
        prob = torch.exp(-0.5 * dist ** 2 / sigma ** 2) if kind == 'gaussian' else torch.exp(-dist / sigma)
        prob = prob / (prob.sum(1, keepdim=True) if mutate == 'no_clamp' else
                       torch.clamp(prob.sum(1, keepdim=True), min=1.0))
    if focal and mutate == 'focal_second_term':
        f = (alpha * (1 - lp.exp()).pow(gamma)).detach() * lp      # the weight's own derivative is lost
    elif focal:
        f = alpha * (1 - lp.exp()).pow(gamma) * lp
    else:
        f = lp
    pix = torch.zeros(mask.shape).masked_scatter(mask, -(prob * f).sum(-1))
    out = dict(loss=pix.detach(), valid=mask)
    if g_loss is not None:
        pix.backward(g_loss.float())
        out['grad'] = _rnd(x.grad, bf16)
    return out


# --------------------------------------------------------------------------------------------------------------------
# the cases (shared by the CPU proof in tests/test_depth_ref.py and the GPU tests)
# --------------------------------------------------------------------------------------------------------------------
DTYPES = ('fp32', 'bf16')

# depth head forward and statistics: cost shape (B, 1, D, H, W), scale
FWD_SHAPES = {'one': ((2, 1, 1, 1, 1), 2),            # Do = 2: below one chunk of 8; up_index at in = 1
              'row': ((1, 1, 3, 1, 5), 4), 'column': ((1, 1, 3, 5, 1), 4),
              'lane4': ((1, 1, 5, 3, 7), 4),          # Wo = 28: the 4-pixel lane
              'lane1': ((1, 1, 5, 3, 7), 3)}          # Wo = 21: the 1-pixel lane; Do = 15, not a multiple of 8
CONTENTS = ('random3', 'rising', 'falling', 'random30')


def fwd_params():
    return [(s, c, dt) for s in FWD_SHAPES for c in CONTENTS for dt in DTYPES]


def make_cost(shape, content, seed, bf16):
    """random x3; strictly increasing / decreasing along depth (the running maximum moves in every chunk / never);
    random x30: a range near +-90, entries below the -128 clamp (the corner column spans 200), underflow"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    if content in ('rising', 'falling'):
        D = shape[2]
        ramp = torch.arange(D, dtype=F32)[None, None, :, None, None] * 4.0
        x = (ramp if content == 'rising' else -ramp) + x          # steps of 4 +- randn: monotone for |randn| < 2
        x = torch.sort(x, dim=2, descending=content == 'falling').values
    else:
        x = x * (30.0 if content == 'random30' else 3.0)
        if content == 'random30' and shape[2] > 1:    # and one column from -100 to 100 for certain
            x[:, :, 0, 0, 0], x[:, :, -1, 0, 0] = -100.0, 100.0
    return x.bfloat16().float() if bf16 else x


# depth head backward: name -> (cost shape, scale, tile kernel?)
BWD_SHAPES = {'tile-one': ((1, 1, 1, 1, 1), 2, True), 'tile-row': ((1, 1, 3, 1, 5), 4, True),
              'tile-column': ((1, 1, 3, 5, 1), 4, True),
              'tile-scale1': ((2, 1, 4, 6, 70), 1, True),      # window 6 x 66, two column tiles
              'tile-last2': ((1, 1, 5, 7, 33), 2, True),       # Wo = 66, Ho = 14: last tiles of 2 columns / 2 rows
              'tile-scale3': ((1, 1, 4, 5, 23), 3, True),
              'scatter-scale1': ((1, 1, 42, 6, 66), 1, False),  # 66528 bytes > 64 KiB
              'scatter-deep': ((1, 1, 304, 3, 18), 4, False)}   # 65664 bytes
SUBSETS = ('v', 's', 'p', 'vs', 'vp', 'sp', 'vsp')              # of (g_vol, g_soft, g_pred)
ALL_SUBSETS_ON = ('tile-last2', 'scatter-scale1')


def bwd_params():
    return [(n, sub, dt) for n in BWD_SHAPES for sub in (SUBSETS if n in ALL_SUBSETS_ON else ('vsp',))
            for dt in DTYPES]


def make_bwd(name, subset, bf16):
    """(cost, ds, scale, grads): cost random x3, the incoming gradients random (bf16 values where bf16)"""
    shape, s, _ = BWD_SHAPES[name]
    B, _, D, H, W = shape
    seed = 100 + sorted(BWD_SHAPES).index(name) * 2 + bf16
    cost = make_cost(shape, 'random3', seed, bf16)
    g = torch.Generator().manual_seed(seed + 5000)
    full = (B, 1, D * s, H * s, W * s)
    gv, gs = torch.randn(full, generator=g), torch.randn(full, generator=g) * 4
    gp = torch.randn((B, 1, H * s, W * s), generator=g)
    grads = [_rnd(t, bf16) if k in subset else None for k, t in zip('vsp', (gv, gs, gp))]
    return cost, depth_samples(D * s), s, grads


# depth loss: volume shapes (B, D, H, W); loss configurations name -> (loss_type or sigma rule, alpha, gamma)
LOSS_SHAPES = {'pixel': (1, 2, 1, 1), 'wg2': (2, 5, 1, 257),     # a second workgroup that holds one pixel
               'wg-exact': (3, 7, 16, 16),                       # HW = 256; sample 1 has no valid pixel
               'configK': (1, 288, 2, 3)}
LOSS_CFGS = {'ce': ('ce', 1.0, 2.0), 'balanced_ce': ('balanced_ce', 1.0, 2.0), 'hard_ce': ('hard_ce', 1.0, 2.0),
             'focal-g0': ('focal', 0.75, 0.0), 'focal-g1': ('focal', 0.75, 1.0), 'focal-g2': ('focal', 0.75, 2.0),
             'focal-g3': ('focal', 0.75, 3.0), 'balanced_focal': ('balanced_focal', 0.75, 2.0),
             'gaussian-small': ('gaussian', 0.1), 'gaussian-large': ('gaussian', 3.0),
             'laplacian-small': ('laplacian', 0.1), 'laplacian-large': ('laplacian', 3.0)}
LOGIT_SCALES = (2.0, 30.0)
# fused: cost (B, 1, cd, ch, cw), scale
FUSED_SHAPES = {'one': ((1, 1, 1, 1, 1), 2), 'row': ((2, 1, 3, 1, 4), 4), 'scale1': ((1, 1, 6, 5, 9), 1),
                'scale3': ((1, 1, 4, 3, 5), 3), 'scale4': ((2, 1, 6, 9, 13), 4)}


def loss_params():
    return [(s, c, int(k), dt) for s in LOSS_SHAPES for c in LOSS_CFGS for k in LOGIT_SCALES for dt in DTYPES]


def fused_params():
    return [(s, c, int(k), dt) for s in FUSED_SHAPES for c in LOSS_CFGS for k in LOGIT_SCALES for dt in DTYPES]


def loss_cfg(cfg, D):
    """(loss_type, alpha, gamma) of a configuration at D bins: the sigmas are 0.1 and 3 bin widths (the small one
    keeps the target sum below 1, the large one above; the tests assert both from the reference)"""
    c = LOSS_CFGS[cfg]
    if len(c) == 3:
        return c
    sigma = float(np.float32(c[1] * (MAX_DEPTH - MIN_DEPTH) / D))
    return f'{c[0]}_{sigma!r}', 1.0, 2.0


def border_values(ds):
    """the hand-placed depth_img values: exactly min / max depth (invalid), their neighbours towards the inside
    (valid), 0, a negative value, NaN, +inf, and two values exactly half-way between two bins (hard_ce's 0.5
    threshold), representable in fp32"""
    lo, hi = np.float32(MIN_DEPTH), np.float32(MAX_DEPTH)
    half = (ds[1] - ds[0]) / 2
    return torch.tensor([lo, hi, np.nextafter(lo, hi), np.nextafter(hi, lo), 0.0, -3.5, float('nan'), float('inf'),
                         float(ds[0] + half), float(ds[-1] - half)], dtype=F32)


def make_depth_img(B, H, W, ds, seed, empty_sample=None):
    """depth_img (B, H, W) fp32: about half the pixels valid at random depths, none within 1e-3 interval of a bin's
    half-way point, the others 0 / beyond max_depth / negative; then the border values by hand, every 3rd pixel from
    the first, as many as fit in half the map (rotated by the seed so that the small maps see all of them over the
    cases); ``empty_sample`` has no valid pixel at all"""
    g = torch.Generator().manual_seed(seed)
    n = B * H * W
    interval = float(ds[1] - ds[0])
    gt = torch.rand(n, generator=g) * (MAX_DEPTH - MIN_DEPTH - 0.2) + MIN_DEPTH + 0.1
    r = ((gt - ds[0]) / interval) % 1.0                 # the half-way points are at r = 0.5
    gt = torch.where((r - 0.5).abs() < 2e-3, gt + 4e-3 * interval, gt).to(F32)
    r = ((gt.double() - float(ds[0])) / interval) % 1.0
    assert bool(((r - 0.5).abs() > 1e-3).all())
    invalid = torch.tensor([0.0, 70.0, -1.0])[torch.randint(0, 3, (n,), generator=g)]
    coin = torch.rand(n, generator=g) < 0.5
    if n < 8:
        coin = torch.arange(n) % 2 == 0                 # (a handful of pixels: alternate)
    img = torch.where(coin, gt, invalid)
    if n >= 64:
        assert 0.2 <= float(coin.float().mean()) <= 0.8
    bv = border_values(ds)
    k = min(len(bv), n // 2)
    for j in range(k):
        img[3 * j if 3 * k <= n else j] = bv[(j + seed) % len(bv)]
    img = img.reshape(B, H, W)
    if empty_sample is not None:
        img[empty_sample] = torch.where(valid_mask(img[empty_sample]), torch.zeros(()), img[empty_sample])
    return img


def make_loss_case(shape, scale_k, seed, bf16, empty_sample=None):
    """(logits (B, D, H, W), depth_img, ds, g_loss): logits random x scale_k; g_loss random with exact zeros at a
    quarter of the valid pixels (the zero-column branch of the backward)"""
    B, D, H, W = shape
    ds = depth_samples(D)
    g = torch.Generator().manual_seed(seed)
    logits = _rnd(torch.randn(shape, generator=g) * scale_k, bf16)
    img = make_depth_img(B, H, W, ds, seed, empty_sample)
    g_loss = torch.randn(B, H, W, generator=g)
    mask = valid_mask(img)
    idx = mask.reshape(-1).nonzero()[:, 0]
    g_loss.reshape(-1)[idx[::4]] = 0.0
    return logits, img, ds, g_loss


def loss_case(shape_name, cfg, scale_k, dt):
    shape = LOSS_SHAPES[shape_name]
    seed = 300 + sorted(LOSS_SHAPES).index(shape_name) * 64 + sorted(LOSS_CFGS).index(cfg) * 4 + (scale_k > 2) * 2 \
        + (dt == 'bf16')
    return make_loss_case(shape, float(scale_k), seed, dt == 'bf16', 1 if shape_name == 'wg-exact' else None) + \
        loss_cfg(cfg, shape[1])


def fused_case(shape_name, cfg, scale_k, dt):
    """(cost, depth_img, ds, g_loss, scale, loss_type, alpha, gamma)"""
    shape, s = FUSED_SHAPES[shape_name]
    B, _, cd, ch, cw = shape
    seed = 900 + sorted(FUSED_SHAPES).index(shape_name) * 64 + sorted(LOSS_CFGS).index(cfg) * 4 + (scale_k > 2) * 2 \
        + (dt == 'bf16')
    _, img, ds, g_loss = make_loss_case((B, cd * s, ch * s, cw * s), 1.0, seed, False)
    cost = make_cost(shape, 'random30' if scale_k > 2 else 'random3', seed, dt == 'bf16')
    return (cost, img, ds, g_loss, s) + loss_cfg(cfg, cd * s)


def sigma_side(img, ds, loss_type):
    """(min, max) over the valid pixels of the gaussian / laplacian target sum, from the reference"""
    kind, sigma, _ = parse_loss(loss_type)
    tg = _target(img[valid_mask(img)], ds, kind, sigma)
    return float(tg['psum'].min()), float(tg['psum'].max())


# DepthHead.loss against total_ref: balanced losses on (3, 7, 16, 16) with fg_weight 5, loss_weight 0.7
TOTAL_KINDS = ('no-fg', 'no-bg', 'box-ids', 'bg-weight-0', 'empty-sample')
TOTAL_CFG = {'balanced_ce': dict(type='balanced_ce', loss_weight=0.7, fg_weight=5, bg_weight=1),
             'balanced_focal': dict(type='balanced_focal', loss_weight=0.7, fg_weight=5, bg_weight=1, alpha=0.75,
                                    gamma=2)}


def total_params():
    return [(k, t, dt) for k in TOTAL_KINDS for t in TOTAL_CFG for dt in DTYPES]


def total_case(kind, loss_type, dt):
    """(logits, depth_img, ds, fgmask, cfg): no fg pixel among the valid ones (the invalid ones are all fg); no bg
    pixel; box ids above 1; bg_weight = 0; one all-invalid sample in the batch of three"""
    seed = 1700 + TOTAL_KINDS.index(kind) * 4 + sorted(TOTAL_CFG).index(loss_type) * 2 + (dt == 'bf16')
    logits, img, ds, _ = make_loss_case((3, 7, 16, 16), 3.0, seed, dt == 'bf16', 1 if kind == 'empty-sample' else None)
    g = torch.Generator().manual_seed(seed)
    mask = valid_mask(img)
    fg = (torch.rand(img.shape, generator=g) < 0.3).float()
    if kind == 'no-fg':
        fg = (~mask).float()
    elif kind == 'no-bg':
        fg = mask.float()
    elif kind == 'box-ids':
        fg = torch.tensor([0.0, 1.0, 2.0, 5.0])[torch.randint(0, 4, img.shape, generator=g)]
    cfg = dict(TOTAL_CFG[loss_type])
    if kind == 'bg-weight-0':
        cfg['bg_weight'] = 0
    return logits, img, ds, fg, cfg


def total_g_loss(mask, fgmask, cfg):
    """d total / d pixel loss (fp64): loss_weight^2 w_i / n"""
    fg = fgmask.bool() & mask
    w = torch.where(fg, float(cfg['fg_weight']), float(cfg['bg_weight'])).to(F64) * mask
    return cfg['loss_weight'] ** 2 * w / int(mask.sum())
