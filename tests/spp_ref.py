"""Helpers of the fused-SPP-tail tests (csrc/spp_tail.hip): plain fp64 restatements of what the tail computes
(1x1 convolution + GroupNorm with one channel per group + ReLU, bilinear up-sampling with align_corners=True,
floor-mode window means), the error bound of a branch map that follows from those alone, and an fp32 emulation
of the branch kernel's arithmetic.  Everything here runs on the CPU; tests/test_spp_tail_gpu.py pins the three
references to torch's own fp64 ops before it holds a kernel against them."""
import numpy as np
import torch


def f64(t):
    """tensor (any dtype, any device) or array -> fp64 ndarray"""
    if torch.is_tensor(t):
        return t.detach().cpu().to(torch.float64).numpy()
    return np.asarray(t, np.float64)


def round_bf16(a):
    """fp64 -> the nearest bf16 value (8 significand bits, ties to even), kept in fp64; straight from fp64, no
    second rounding through fp32.  (bf16's exponent range is fp32's: no test value comes near its ends.)"""
    m, e = np.frexp(np.asarray(a, np.float64))          # a = m 2^e, 0.5 <= |m| < 1
    return np.ldexp(np.rint(m * 256.0), e - 8)


def ulp_bf16(a):
    """spacing of the bf16 values in the binade of ``a`` (0 for 0)"""
    a = np.asarray(a, np.float64)
    _, e = np.frexp(a)
    return np.where(a == 0, 0.0, np.ldexp(1.0, e - 8))


def _stats(conv):
    axes = tuple(range(1, conv.ndim - 1))
    mu = conv.mean(axes, keepdims=True)
    var = ((conv - mu) ** 2).mean(axes, keepdims=True)   # biased
    return mu, var


def branch_ref(x, w, gamma, beta, eps, staged):
    """one SPP branch on its pooled map ``x`` (B, ..pixels.., K), weights ``w`` (C, K): 1x1 convolution, GroupNorm
    with one channel per group (biased variance over the sample's pixels), affine, ReLU -- all fp64.  ``staged``
    rounds the convolution and the GroupNorm output to bf16 where the unfused modules store a bf16 tensor (and the
    kernel rounds).  Returns (B, ..pixels.., C) fp64."""
    conv = f64(x) @ f64(w).T
    if staged:
        conv = round_bf16(conv)
    mu, var = _stats(conv)
    y = (conv - mu) / np.sqrt(var + eps) * f64(gamma) + f64(beta)
    if staged:
        y = round_bf16(y)
    return np.maximum(y, 0.0)


def branch_tol(x, w, gamma, beta, eps):
    """per-element bound on |kernel branch map - branch_ref(staged=False)|, from the reference alone:

        tol = 2^-8 * ( |gamma_c| * (M_c / s_c) * (2 + |z|) + |y| )

    with conv the fp64 convolution, M_c = max_p |conv|, s_c = sqrt(var_c + eps), z = (conv - mu_c) / s_c and
    y = gamma_c z + beta_c.  Derivation, with u = 2^-8 the unit roundoff of bf16 (8 significand bits, round to
    nearest): the kernel's one deliberate loss before the statistics is the bf16 rounding of the convolution
    output, conv'_p = conv_p + d_p with |d_p| <= u |conv_p| <= u M_c.  To first order
    dz_p = (d_p - dmu) / s - z_p ds / s,  where |dmu| = |mean d| <= u M_c and ds = mean((conv - mu) d) / s, so
    |ds| <= sqrt(mean (conv - mu)^2) sqrt(mean d^2) / s <= u M_c (Cauchy-Schwarz, sqrt(var) <= s).  Hence
    |dz_p| <= u (M_c / s_c) (2 + |z_p|), times |gamma_c| through the affine map; the bf16 rounding of the GroupNorm
    output adds u |y|; ReLU is 1-Lipschitz.  That is the worst case of every rounding at once: each d_p at its
    full u M_c (a rounding error is u / 2 of its value on average, and most |conv_p| are well below M_c) and all of
    them aligned in dmu and ds (they are independent: mean d shrinks like 1 / sqrt(P)).  Counting a rounding at
    its mean 2^-9 the bound is twice the first-order estimate; either way the 2^-17 of the hi + lo weight split and
    the fp32 accumulation and statistics (2^-24 each) are far below it."""
    conv = f64(x) @ f64(w).T
    mu, var = _stats(conv)
    s = np.sqrt(var + eps)
    z = (conv - mu) / s
    y = z * f64(gamma) + f64(beta)
    big = np.abs(conv).max(tuple(range(1, conv.ndim - 1)), keepdims=True)
    return 2.0 ** -8 * (np.abs(f64(gamma)) * (big / s) * (2.0 + np.abs(z)) + np.abs(y))


def _taps(n_in, n_out):
    """align_corners=True: src = dst (in - 1) / (out - 1) with the quotient and the remainder taken in integers
    (0 for a one-pixel output, as ATen)"""
    dst = np.arange(n_out, dtype=np.int64)
    if n_out == 1:
        i0, frac = np.zeros(1, np.int64), np.zeros(1, np.float64)
    else:
        num = dst * (n_in - 1)
        i0 = num // (n_out - 1)
        frac = (num % (n_out - 1)).astype(np.float64) / (n_out - 1)
    return i0, np.minimum(i0 + 1, n_in - 1), frac


def resize_ref(small, H, W):
    """bilinear resize of a channels-last map (B, h, w, C) to (B, H, W, C), align_corners=True, fp64"""
    small = f64(small)
    y0, y1, fy = _taps(small.shape[1], H)
    x0, x1, fx = _taps(small.shape[2], W)
    fy, fx = fy[None, :, None, None], fx[None, None, :, None]
    rows = small[:, y0] * (1.0 - fy) + small[:, y1] * fy
    return rows[:, :, x0] * (1.0 - fx) + rows[:, :, x1] * fx


def pool_ref(x, k):
    """means over the non-overlapping k x k windows of (B, C, H, W), floor mode (trailing rows / columns that do
    not fill a window are dropped), fp64"""
    x = f64(x)
    kh, kw = (k, k) if isinstance(k, int) else k
    B, C, H, W = x.shape
    ho, wo = H // kh, W // kw
    return x[:, :, :ho * kh, :wo * kw].reshape(B, C, ho, kh, wo, kw).mean(axis=(3, 5))


def emulate_branch_f32(x, w, gamma, beta, eps):
    """the arithmetic of spp_branch_kernel in numpy float32, for one sample's pooled pixels ``x`` (P, K) on
    EXACT-GRID inputs (small integers times weights k / 8: every partial sum of the convolution is exact in fp32,
    so its accumulation order does not matter and fp64 gives the same bits).  What is emulated is everything after
    the convolution: its bf16 rounding, the two-pass statistics with the kernel's thread map (256 / C partial sums
    per channel over pixels pg, pg + npg, ..., combined in order; the second pass accumulates with a fused
    multiply-add), 1 / sqrt(var + eps), the unfused affine expression (the library is built with
    -ffp-contract=off), the bf16 rounding of the GroupNorm output, ReLU.  Returns (P, C) float32.
    Not bit-faithful in one place: fmaf(d, d, v) is taken as the fp64 sum d * d + v rounded to fp32, two roundings
    where the instruction has one; they can differ in the last bit of a variance partial sum (a relative 2^-24 of
    the variance), far too little to move the share of elements the cap is about."""
    f32 = np.float32
    ys = round_bf16(f64(x) @ f64(w).T).astype(f32)
    P, C = ys.shape
    npg = 256 // C
    part = np.zeros((npg, C), f32)
    for p in range(P):
        part[p % npg] += ys[p]
    t = np.zeros(C, f32)
    for g in range(npg):
        t = t + part[g]
    m = t / f32(P)
    part = np.zeros((npg, C), f32)
    for p in range(P):
        d = ys[p] - m
        # fmaf(d, d, v): d * d is exact in fp64; the sum is rounded to fp64 and then to fp32
        part[p % npg] = (d.astype(np.float64) ** 2 + part[p % npg].astype(np.float64)).astype(f32)
    t = np.zeros(C, f32)
    for g in range(npg):
        t = t + part[g]
    rs = f32(1.0) / np.sqrt(t / f32(P) + f32(eps))
    ga, be = np.asarray(f64(gamma), f32), np.asarray(f64(beta), f32)
    y = (ys - m) * rs * ga + be
    assert y.dtype == f32
    return np.maximum(round_bf16(y.astype(np.float64)), 0.0).astype(f32)
