"""Which kernel body each MFMA convolution problem runs, and one table of problems that reaches every body.

The bodies are chosen by shape inside the library, not by the caller, so a test of "the convolution" only tests
the bodies its shapes happen to reach.  The helpers here mirror the host code that chooses (no GPU needed); the
tables are what tests/test_conv_variant_coverage.py checks for completeness on the CPU and what
tests/test_conv_variants_exact_gpu.py runs at every voxel on the GPU.
"""
import ctypes
import importlib
import itertools
from collections import namedtuple

import torch

# (CW, PFW, F32, FAST): one conv3d_g_kernel<CW, PFW, F32, FAST> instantiation
GBody = namedtuple('GBody', 'cw pfw f32 fast')
# what a problem runs: the instantiation plus what g_plan decides at run time inside it
GRun = namedtuple('GRun', 'cw pfw fast resident classes k1d')

# conv3d_g_launch (csrc/conv3d_g.hip, G_LAUNCH): CW in {1, 2} x PFW in {1..4} x {bf16, fp32} x {FAST, generic};
# the fp32 FAST form exists for CW * PFW < 8 only (the 128-accumulator form spills): 31 bodies
ALL_G_BODIES = frozenset(GBody(cw, pfw, f32, fast) for cw, pfw, f32, fast in
                         itertools.product((1, 2), (1, 2, 3, 4), (False, True), (False, True))
                         if not (f32 and fast and cw * pfw >= 8))

LDS_BUDGET = 160 * 1024


def _cv():
    return importlib.import_module('depth-from-motion_amd.conv3d')


def _triple(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v, v)


def g_run(n, cin, cout, size, stride=1, padding=1, transposed=False, kernel1=False, cstride=0):
    """GRun of a dfm_conv3d_g_fwd / _fwd_f32 problem, from dfm_conv3d_g_plan's plan8 and the descriptor:
      * cw, pfw: plan8[1], plan8[0];
      * classes: 2 ** (transposed axes) (g_plan: classes *= 2 per up axis);
      * resident: classes > 1 and ceil(block_px * 4 / 256) * 4096 * (cin / 32) <= 160 KiB (g_plan: `resident`);
      * fast: not resident, no transposed axis, kernel extent 3 along w and along d or h (conv3d_g_launch: `fast`);
      * k1d: kernel extent 1 along depth (the 2-D form)."""
    cv = _cv()
    stride, padding, transposed, kernel1 = _triple(stride), _triple(padding), _triple(transposed), _triple(kernel1)
    out = cv.conv3d_g_out_size(size, stride, padding, transposed, kernel1)
    d = cv._conv_desc(n, cin, cout, size, out, stride, padding, transposed, False, cstride, kernel1)
    plan = (ctypes.c_int64 * 8)()
    rc = cv._capi.lib().dfm_conv3d_g_plan(ctypes.byref(d), plan)
    if rc != 0:
        raise ValueError(f'dfm_conv3d_g_plan: {rc} {cv._capi.lib().dfm_last_error()}')
    pfw, cw, block_px, lds = plan[0], plan[1], plan[5], plan[6]
    classes = 2 ** sum(1 for t in transposed if t)
    rounds = -(-block_px * 4 // 256)
    resident = classes > 1 and rounds * 4096 * (cin // 32) <= LDS_BUDGET
    # (the plan's LDS bytes hold every chunk exactly when the block is resident)
    assert lds == rounds * 4096 * ((cin // 32) if resident else 1), (plan[:], resident)
    fast = (not resident and not any(transposed) and not kernel1[2] and not (kernel1[0] and kernel1[1]))
    return GRun(cw, pfw, fast, resident, classes, bool(kernel1[0]))


def g_body(run, f32):
    """the conv3d_g_kernel instantiation a GRun launches in bf16 (dfm_conv3d_g_fwd) or fp32 (_fwd_f32) form"""
    return GBody(run.cw, run.pfw, bool(f32), bool(run.fast and (not f32 or run.cw * run.pfw < 8)))


# ---- conv3d_g cases -------------------------------------------------------------------------------------------
# name, N, cin, cout, input (d, h, w), stride, padding, transposed axes, kernel-extent-1 axes, input pixel stride
# (0: dense; > cin: the input is the first cin channels of a wider tensor), and the GRun the planner must choose.
GCase = namedtuple('GCase', 'name n cin cout size stride padding transposed kernel1 cstride run')
_F, _T = (False,) * 3, (True,) * 3
_UPHW, _UPW, _UPD = (False, True, True), (False, False, True), (True, False, False)
_K1D = (True, False, False)

G_CASES = [
    # FAST: every (CW, PFW), plain correlations
    GCase('fast_1x1_ragged', 1, 32, 32, (5, 7, 9), 1, 1, _F, _F, 0, GRun(1, 1, True, False, 1, False)),
    GCase('fast_2x1_n2', 2, 64, 64, (6, 10, 12), 1, 1, _F, _F, 0, GRun(2, 1, True, False, 1, False)),
    GCase('fast_2x1_stride2_odd', 1, 64, 64, (7, 9, 11), 2, 1, _F, _F, 0, GRun(2, 1, True, False, 1, False)),
    GCase('fast_2x1_pad_110', 1, 256, 256, (3, 5, 3), 1, (1, 1, 0), _F, _F, 0, GRun(2, 1, True, False, 1, False)),
    GCase('fast_1x1_pad2', 1, 32, 32, (3, 4, 5), 1, 2, _F, _F, 0, GRun(1, 1, True, False, 1, False)),
    GCase('fast_1x2_cout96', 1, 32, 96, (7, 33, 33), 1, 1, _F, _F, 0, GRun(1, 2, True, False, 1, False)),
    GCase('fast_1x2', 1, 32, 32, (12, 40, 80), 1, 1, _F, _F, 0, GRun(1, 2, True, False, 1, False)),
    GCase('fast_2x2', 1, 32, 64, (12, 40, 80), 1, 1, _F, _F, 0, GRun(2, 2, True, False, 1, False)),
    GCase('fast_1x3', 1, 32, 32, (24, 40, 80), 1, 1, _F, _F, 0, GRun(1, 3, True, False, 1, False)),
    GCase('fast_2x3', 1, 32, 64, (24, 40, 80), 1, 1, _F, _F, 0, GRun(2, 3, True, False, 1, False)),
    GCase('fast_1x4', 1, 32, 32, (31, 40, 80), 1, 1, _F, _F, 0, GRun(1, 4, True, False, 1, False)),
    GCase('fast_2x4', 1, 32, 64, (31, 40, 80), 1, 1, _F, _F, 0, GRun(2, 4, True, False, 1, False)),
    GCase('fast_2x1_slice', 1, 64, 64, (5, 6, 9), (1, 1, 2), 1, _F, _F, 128, GRun(2, 1, True, False, 1, False)),
    # the 2-D form (a depth-1 volume, kernel (1, 3, 3)): FAST, and transposed on (h, w)
    GCase('fast2d_2x1_stride2', 2, 32, 64, (1, 13, 18), (1, 2, 2), (0, 1, 1), _F, _K1D, 0, GRun(2, 1, True, False, 1, True)),
    GCase('gen2d_1x1_up', 1, 64, 32, (1, 7, 10), 1, (0, 1, 1), _UPHW, _K1D, 0, GRun(1, 1, False, True, 4, True)),
    # generic, resident: 2 / 4 / 8 parity classes
    GCase('gen_1x1_8cls_res', 2, 32, 32, (3, 4, 5), 1, 1, _T, _F, 0, GRun(1, 1, False, True, 8, False)),
    GCase('gen_1x1_4cls_res_cout96', 1, 32, 96, (3, 5, 4), 1, 1, _UPHW, _F, 0, GRun(1, 1, False, True, 4, False)),
    GCase('gen_2x1_2cls_res_slice', 1, 32, 64, (3, 5, 7), 1, 1, _UPW, _F, 64, GRun(2, 1, False, True, 2, False)),
    GCase('gen_1x2_8cls_res', 1, 32, 32, (12, 40, 80), 1, 1, _T, _F, 0, GRun(1, 2, False, True, 8, False)),
    # generic, streamed (the block of every chunk does not fit the LDS): 2 / 4 / 8 parity classes
    GCase('gen_1x1_8cls_str', 1, 224, 32, (1, 3, 3), 1, 1, _T, _F, 0, GRun(1, 1, False, False, 8, False)),
    GCase('gen_2x1_4cls_str_n2', 2, 160, 64, (1, 3, 3), 1, 1, _UPHW, _F, 0, GRun(2, 1, False, False, 4, False)),
    GCase('gen_1x2_2cls_str', 1, 128, 32, (1, 3, 3), 1, 1, _UPW, _F, 0, GRun(1, 2, False, False, 2, False)),
    GCase('gen_2x3_2cls_str', 1, 128, 64, (2, 3, 16), 1, 1, _UPD, _F, 0, GRun(2, 3, False, False, 2, False)),
    GCase('gen_2x2_8cls_str', 1, 128, 64, (1, 3, 3), 1, 1, _T, _F, 0, GRun(2, 2, False, False, 8, False)),
    GCase('gen_1x3_4cls_str', 1, 128, 32, (1, 3, 3), 1, 1, _UPHW, _F, 0, GRun(1, 3, False, False, 4, False)),
    GCase('gen_2x3_4cls_str', 1, 64, 64, (3, 3, 3), 1, 1, _UPHW, _F, 0, GRun(2, 3, False, False, 4, False)),
    GCase('gen_1x4_4cls_str', 1, 128, 32, (8, 40, 80), 1, 1, _UPHW, _F, 0, GRun(1, 4, False, False, 4, False)),
    GCase('gen_2x4_4cls_str', 1, 64, 64, (12, 20, 80), 1, 1, _UPHW, _F, 0, GRun(2, 4, False, False, 4, False)),
]


def g_case_run(c):
    return g_run(c.n, c.cin, c.cout, c.size, c.stride, c.padding, c.transposed, c.kernel1, c.cstride)


def g_case_out_size(c):
    return _cv().conv3d_g_out_size(c.size, _triple(c.stride), _triple(c.padding), _triple(c.transposed),
                                   _triple(c.kernel1))


# what the table must reach besides the 31 bodies: (classes, resident) of the generic body wherever the planner can
# produce them, the 2-D form in both precisions, N = 2, a channel-slice input and cout = 96 (CW = 1, 3 channel tiles)
REQUIRED_GENERIC_CLASSES = frozenset(itertools.product((2, 4, 8), (True, False)))


def g_table_gaps(cases):
    """names of whatever the cases miss (empty: the table reaches everything)"""
    runs = [(c, g_run(c.n, c.cin, c.cout, c.size, c.stride, c.padding, c.transposed, c.kernel1, c.cstride))
            for c in cases]
    gaps = []
    bodies = {g_body(r, f32) for _, r in runs for f32 in (False, True)}
    for b in sorted(ALL_G_BODIES - bodies):
        gaps.append(f'conv3d_g_kernel<CW={b.cw}, PFW={b.pfw}, F32={b.f32}, FAST={b.fast}>')
    gen = {(r.classes, r.resident) for _, r in runs if not r.fast and r.classes > 1}
    for cl, res in sorted(REQUIRED_GENERIC_CLASSES - gen):
        gaps.append(f'generic body, {cl} parity classes, {"resident" if res else "streamed"}')
    if not any(r.k1d and r.fast for _, r in runs):
        gaps.append('the 2-D form (kernel1 depth) in the FAST body, bf16 and fp32')
    if not any(c.n == 2 for c, _ in runs):
        gaps.append('N = 2')
    if not any(c.cstride > c.cin for c, _ in runs):
        gaps.append('an input that is a channel slice (in_channel_stride > cin)')
    if not any(c.cout == 96 and r.cw == 1 for c, r in runs):
        gaps.append('cout = 96 (CW = 1, three channel tiles)')
    return gaps


# ---- conv3d_wgrad ---------------------------------------------------------------------------------------------
# WRun: col (column mode), sw (row stride of the contracted axis), flat, swap (contract along H), dchunk, scratch bytes
WRun = namedtuple('WRun', 'col sw flat swap dchunk scratch')
WG_TH, WG_THREADS, WG_BATCH = 2, 192, 3


def w_kernel(run):
    """the conv3d_wgrad_kernel<SW, FLAT, COL> instantiation a WRun launches (wgrad_impl)"""
    return (1, False, True) if run.col else (run.sw, bool(run.flat), False)


ALL_W_KERNELS = frozenset({(1, False, True), (1, False, False), (1, True, False), (2, False, False), (2, True, False)})


def w_run(n, a, b, g_size, x_size, stride, padding):
    """mirror of wgrad_plan (csrc/conv3d_wgrad.hip) for g (n, g_size, a), x (n, x_size, b)"""
    stride, padding = _triple(stride), _triple(padding)
    swap = g_size[1] > g_size[2]                                  # contract along the longer in-plane axis
    hi, wi = (2, 1) if swap else (1, 2)
    Do, Ho, Wo, Di = g_size[0], g_size[hi], g_size[wi], x_size[0]
    sd, sh, sw, pd = stride[0], stride[hi], stride[wi], padding[0]
    TW = 64 if sw == 1 else 32
    tiles_w, tiles_h = -(-Wo // TW), -(-Ho // WG_TH)
    nt = n * Do * tiles_h * tiles_w
    pairs = (a // 32) * (b // 32)
    wpp = max(1, min((512 + pairs - 1) // pairs, (nt + 7) // 8))
    RH = (WG_TH - 1) * sh + 3
    flat = Di == 1 and Do == 1 and pd == 1 and sd == 1
    col, dchunk = False, 1
    order_ok = 3 * RH * 4 * ((TW + 16) // 4) == 5 * WG_THREADS and WG_BATCH == 3
    if order_ok and sw == 1 and sd == 1 and sh == 1 and not flat and Do > 1:
        cols = n * tiles_h * tiles_w
        wgs = max(1, 512 // pairs)
        dc, best = Do, 1e30
        for c in range(min(Do, 3), Do + 1):
            items = cols * -(-Do // c)
            cost = -(-items // wgs) * (c + 0.7)
            if cost < best - 1e-9:
                best, dc = cost, c
        dchunk = dc
        items = cols * -(-Do // dc)
        if items < 2 ** 31:
            wpp = max(1, min(wgs, items))
            col = True
    return WRun(col, sw, flat, swap, dchunk, pairs * wpp * 27 * 1024 * 4)


# name, N, B (x channels), A (g channels), x (d, h, w), stride, padding, and the WRun's (col, sw, flat, swap, dchunk)
WCase = namedtuple('WCase', 'name n b a x_size stride padding kind')
W_CASES = [
    WCase('col_swap0_ragged_chunk', 1, 32, 32, (7, 6, 20), 1, 1, (True, 1, False, False, 3)),
    WCase('col_swap1_n2', 2, 64, 32, (5, 20, 6), 1, 1, (True, 1, False, True, 3)),
    WCase('col_pad_110', 1, 64, 64, (3, 5, 9), 1, (1, 1, 0), (True, 1, False, False, 3)),
    WCase('tile_sw1_depth_stride2', 1, 32, 64, (6, 8, 20), (2, 1, 1), 1, (False, 1, False, False, 1)),
    WCase('tile_sw2_swap0', 1, 32, 64, (8, 12, 16), 2, 1, (False, 2, False, False, 1)),
    WCase('tile_sw2_swap1_odd', 2, 64, 32, (7, 17, 9), 2, 1, (False, 2, False, True, 1)),
    WCase('flat_sw1', 1, 64, 32, (1, 12, 40), 1, 1, (False, 1, True, False, 1)),
    WCase('flat_sw2_swap1', 2, 32, 64, (1, 24, 16), (1, 2, 2), 1, (False, 2, True, True, 1)),
]


def w_case_g_size(c):
    st, pd = _triple(c.stride), _triple(c.padding)
    return tuple((s + 2 * p - 3) // t + 1 for s, t, p in zip(c.x_size, st, pd))


def w_case_run(c):
    return w_run(c.n, c.a, c.b, w_case_g_size(c), c.x_size, c.stride, c.padding)


def w_table_gaps(cases):
    runs = [w_case_run(c) for c in cases]
    gaps = [f'conv3d_wgrad_kernel<SW={k[0]}, FLAT={k[1]}, COL={k[2]}>'
            for k in sorted(ALL_W_KERNELS - {w_kernel(r) for r in runs})]
    for s in (False, True):
        if not any(r.swap == s for r in runs):
            gaps.append(f'swap = {int(s)}')
    if not any(r.col and w_case_g_size(c)[0] % r.dchunk for c, r in zip(cases, runs)):
        gaps.append('column mode with Do not a multiple of dchunk')
    return gaps


# ---- float64 references (any device: the GPU tests run them on the GPU, the CPU tier checks them against torch) --
def _axis_forms(x, stride, padding, transposed, kernel1):
    """x (N, C, D, H, W) -> (the input padded / zero-inserted so that output o of axis a reads element
    step[a] * o + j, per axis: step, [(j, kernel index)], output extent)"""
    forms = []
    for a in range(3):
        dim, n = 2 + a, x.shape[2 + a]
        if transposed[a]:
            # x2 transposed (k 3, s 2, p 1, op 1): out[o] = sum_k x[i] w[k] over 2 i - 1 + k = o
            #   = a correlation with the mirrored kernel over the zero-inserted input, one zero in front
            shape = list(x.shape)
            shape[dim] = 2 * n + 2
            u = x.new_zeros(shape)
            u.narrow(dim, 1, 2 * n).unfold(dim, 1, 2).copy_(x.unsqueeze(-1))
            x = u
            forms.append((1, [(j, 2 - j) for j in range(3)], 2 * n))
        elif kernel1[a]:
            forms.append((stride[a], [(0, 1)], (n - 1) // stride[a] + 1))
        else:
            o = (n + 2 * padding[a] - 3) // stride[a] + 1
            need = stride[a] * (o - 1) + 3
            shape = list(x.shape)
            shape[dim] = max(need, n + padding[a])
            u = x.new_zeros(shape)
            u.narrow(dim, padding[a], min(n, shape[dim] - padding[a])).copy_(x.narrow(dim, 0, min(n, shape[dim] - padding[a])))
            x = u
            forms.append((stride[a], [(j, j) for j in range(3)], o))
    return x, forms


def _tap_view(xp, forms, jd, jh, jw):
    (sd, _, od), (sh, _, oh), (sw, _, ow) = forms
    return xp[:, :, jd:jd + sd * (od - 1) + 1:sd, jh:jh + sh * (oh - 1) + 1:sh, jw:jw + sw * (ow - 1) + 1:sw]


def ref_conv(x, w, stride=1, padding=1, transposed=False, kernel1=False):
    """conv3d_g's operation in x's dtype: x (N, cin, D, H, W), w (cout, cin, 3, 3, 3) indexed as the kernel reads
    it (a transposed axis: ConvTranspose3d's own weight index), per-axis correlation / x2 transposed / extent 1"""
    stride, padding, transposed, kernel1 = _triple(stride), _triple(padding), _triple(transposed), _triple(kernel1)
    xp, forms = _axis_forms(x, stride, padding, transposed, kernel1)
    out = x.new_zeros((x.shape[0], w.shape[0], forms[0][2], forms[1][2], forms[2][2]))
    for jd, kd in forms[0][1]:
        for jh, kh in forms[1][1]:
            for jw, kw in forms[2][1]:
                out += torch.einsum('ncdhw,oc->nodhw', _tap_view(xp, forms, jd, jh, jw), w[:, :, kd, kh, kw])
    return out


def ref_wgrad(x, g, stride, padding):
    """out[a][b][k] = sum_o g[:, a, o] x[:, b, o * stride - padding + k] in x's dtype (the conv3d_wgrad operation)"""
    stride, padding = _triple(stride), _triple(padding)
    xp, forms = _axis_forms(x, stride, padding, (False,) * 3, (False,) * 3)
    assert tuple(f[2] for f in forms) == tuple(g.shape[2:])
    out = x.new_zeros((g.shape[1], x.shape[1], 3, 3, 3))
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                out[:, :, kd, kh, kw] = torch.einsum('nadhw,nbdhw->ab', g, _tap_view(xp, forms, kd, kh, kw))
    return out
