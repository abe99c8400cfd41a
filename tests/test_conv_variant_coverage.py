"""The case table of tests/conv_variants.py against the planners (host code, no GPU): it reaches every
conv3d_g_kernel and conv3d_wgrad_kernel body, each case still plans to the body the table names, and the float64
references the exact GPU tests compare with are torch's convolutions.  Also: the 16-byte alignment checks of the
bf16 convolution entry points, which must refuse a bad pointer before any HIP call."""
import ctypes
import importlib

import pytest
import torch
import torch.nn.functional as F

from tests import conv_variants as V


@pytest.fixture(scope='module')
def cv():
    importlib.import_module('depth-from-motion_amd.build').build_hip()
    return importlib.import_module('depth-from-motion_amd.conv3d')


def test_there_are_31_conv3d_g_bodies():
    assert len(V.ALL_G_BODIES) == 31
    assert V.GBody(2, 4, True, True) not in V.ALL_G_BODIES and V.GBody(1, 4, True, True) in V.ALL_G_BODIES


def test_every_case_plans_to_the_body_the_table_names(cv):
    moved = [(c.name, c.run, V.g_case_run(c)) for c in V.G_CASES if V.g_case_run(c) != c.run]
    assert not moved, f'the planner moved these cases (name, table, now): {moved}'
    assert len({c.name for c in V.G_CASES}) == len(V.G_CASES)


def test_the_table_reaches_every_conv3d_g_body(cv):
    gaps = V.g_table_gaps(V.G_CASES)
    assert not gaps, 'the conv3d_g case table misses: ' + '; '.join(gaps)


def test_a_table_without_a_body_names_it(cv):
    """the gap report is what fails the test above when a case is dropped or moves"""
    cases = [c for c in V.G_CASES if c.name != 'fast_2x4']
    assert V.g_table_gaps(cases) == ['conv3d_g_kernel<CW=2, PFW=4, F32=False, FAST=True>']
    cases = [c for c in V.G_CASES if not (c.run.classes == 8 and not c.run.resident)]
    assert 'generic body, 8 parity classes, streamed' in V.g_table_gaps(cases)
    cases = [c for c in V.G_CASES if c.name != 'fast2d_2x1_stride2']
    assert V.g_table_gaps(cases) == ['the 2-D form (kernel1 depth) in the FAST body, bf16 and fp32']


def test_body_of_the_fp32_form(cv):
    """conv3d_g_launch: the fp32 form of a FAST problem runs the generic body when CW * PFW >= 8"""
    assert V.g_body(V.GRun(2, 4, True, False, 1, False), True) == V.GBody(2, 4, True, False)
    assert V.g_body(V.GRun(2, 4, True, False, 1, False), False) == V.GBody(2, 4, False, True)
    assert V.g_body(V.GRun(1, 4, True, False, 1, False), True) == V.GBody(1, 4, True, True)
    assert V.g_body(V.GRun(1, 2, False, True, 8, False), True) == V.GBody(1, 2, True, False)


def test_wgrad_mirror_agrees_with_the_library(cv):
    """wgrad_plan's choices are not exported; its scratch size is, and depends on column mode (work items) and
    on the tiling: the mirror's must equal dfm_conv3d_wgrad_workspace_bytes for every case"""
    capi = cv._capi
    lib = capi.lib()
    for c in V.W_CASES:
        run = V.w_case_run(c)
        assert tuple(run[:5]) == c.kind, (c.name, run)
        g_size = V.w_case_g_size(c)
        d = capi.Conv3dWgradDesc()
        d.n, d.a, d.b = c.n, c.a, c.b
        for i in range(3):
            d.g_size[i], d.x_size[i] = g_size[i], c.x_size[i]
            d.stride[i], d.padding[i] = V._triple(c.stride)[i], V._triple(c.padding)[i]
        gs = (g_size[0] * g_size[1] * g_size[2] * c.a, g_size[1] * g_size[2] * c.a, g_size[2] * c.a, c.a)
        xs = (c.x_size[0] * c.x_size[1] * c.x_size[2] * c.b, c.x_size[1] * c.x_size[2] * c.b, c.x_size[2] * c.b, c.b)
        for i in range(4):
            d.g_stride[i], d.x_stride[i] = gs[i], xs[i]
        assert lib.dfm_conv3d_wgrad_workspace_bytes(ctypes.byref(d)) == run.scratch, c.name


def test_the_table_reaches_every_wgrad_kernel():
    gaps = V.w_table_gaps(V.W_CASES)
    assert not gaps, 'the conv3d_wgrad case table misses: ' + '; '.join(gaps)
    cases = [c for c in V.W_CASES if not V.w_case_run(c).flat or V.w_case_run(c).sw != 2]
    assert V.w_table_gaps(cases) == ['conv3d_wgrad_kernel<SW=2, FLAT=True, COL=False>']


def _naive_conv(x, w, stride, padding, transposed, kernel1):
    """the per-axis definition, one output voxel and tap at a time: correlation i = o s - p + k; kernel extent 1:
    k = 1 only, i = o s; x2 transposed (k 3, s 2, p 1, op 1): 2 i - 1 + k = o"""
    def taps(a, o):
        n = x.shape[2 + a]
        if transposed[a]:
            return [(k, (o + 1 - k) // 2) for k in range(3) if (o + 1 - k) % 2 == 0 and 0 <= (o + 1 - k) // 2 < n]
        if kernel1[a]:
            return [(1, o * stride[a])]
        return [(k, o * stride[a] - padding[a] + k) for k in range(3) if 0 <= o * stride[a] - padding[a] + k < n]
    out_size = [2 * x.shape[2 + a] if transposed[a] else
                (x.shape[2 + a] - 1) // stride[a] + 1 if kernel1[a] else
                (x.shape[2 + a] + 2 * padding[a] - 3) // stride[a] + 1 for a in range(3)]
    out = x.new_zeros((x.shape[0], w.shape[0], *out_size))
    for od in range(out_size[0]):
        for oh in range(out_size[1]):
            for ow in range(out_size[2]):
                for kd, i in taps(0, od):
                    for kh, j in taps(1, oh):
                        for kw, m in taps(2, ow):
                            out[:, :, od, oh, ow] += x[:, :, i, j, m] @ w[:, :, kd, kh, kw].t()
    return out


@pytest.mark.parametrize('stride,padding,transposed,kernel1', [
    (1, 1, False, False), (2, 1, False, False), ((1, 1, 2), (1, 1, 0), False, False), (1, 2, False, False),
    (1, 1, True, False), (1, 1, (False, True, True), False), (1, 1, (True, False, False), False),
    ((1, 2, 2), (0, 1, 1), False, (True, False, False)), (1, (0, 1, 1), (False, True, True), (True, False, False))])
def test_float64_reference_is_torchs_convolution(stride, padding, transposed, kernel1):
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(2, 5, 4, 6, 7, generator=gen, dtype=torch.float64)
    tr, k1 = V._triple(transposed), V._triple(kernel1)
    if k1[0]:
        x = x[:, :, :1]
    w = torch.randn(3, 5, 3, 3, 3, generator=gen, dtype=torch.float64)
    got = V.ref_conv(x, w, stride, padding, transposed, kernel1)
    if all(tr):
        ref = F.conv_transpose3d(x, w.transpose(0, 1), stride=2, padding=1, output_padding=1)
    elif any(tr):
        ref = _naive_conv(x, w, V._triple(stride), V._triple(padding), tr, k1)
    else:
        ref = F.conv3d(x, w[:, :, 1:2] if k1[0] else w, stride=stride, padding=padding)
    assert got.shape == ref.shape
    torch.testing.assert_close(got, ref, rtol=1e-12, atol=1e-12)


def test_float64_weight_gradient_reference_is_autograds():
    gen = torch.Generator().manual_seed(4)
    for stride, padding, size in ((1, 1, (4, 5, 6)), (2, 1, (5, 6, 7)), ((1, 2, 2), (1, 1, 1), (1, 6, 8)),
                                  (1, (1, 1, 0), (3, 5, 4))):
        x = torch.randn(2, 4, *size, generator=gen, dtype=torch.float64)
        w = torch.randn(3, 4, 3, 3, 3, generator=gen, dtype=torch.float64, requires_grad=True)
        y = F.conv3d(x, w, stride=stride, padding=padding)
        g = torch.randn(y.shape, generator=gen, dtype=torch.float64)
        y.backward(g)
        torch.testing.assert_close(V.ref_wgrad(x, g, stride, padding), w.grad, rtol=1e-12, atol=1e-12)


@pytest.mark.skipif(torch.cuda.is_available(), reason='fake device pointers: only where no device is visible')
def test_bf16_convolutions_refuse_buffers_that_are_not_16_byte_aligned(cv):
    """dfm_conv3d_g_fwd (x, residual, out) and the 32-channel kernel's entries (x, acc_in, out) store and load
    16-byte vectors: an 8-byte-offset pointer is DFM_ERR_INVALID_ARG before any HIP call (fake pointers, nothing
    is launched)"""
    lib = cv._capi.lib()
    base = 1 << 32          # a fake, 16-byte-aligned device address
    d = cv._conv_desc(1, 32, 32, (4, 4, 4), (4, 4, 4), (1, 1, 1), (1, 1, 1), (False,) * 3, False)
    x, w, out, res = base, base + 4096, base + 65536, base + 131072
    for args in ((x + 8, w, None, None, None, out), (x, w, None, None, None, out + 8),
                 (x, w, None, None, res + 8, out)):
        assert lib.dfm_conv3d_g_fwd(ctypes.byref(d), *args, None) == -1
        assert b'16-byte aligned' in lib.dfm_last_error()
    assert lib.dfm_conv3d_g_fwd_f32(ctypes.byref(d), x, w, None, out + 8, None) == -1
    assert b'16-byte aligned' in lib.dfm_last_error()
    assert lib.dfm_conv3d_g_fwd_f32(ctypes.byref(d), x + 8, w, None, out, None) == -1
    assert b'16-byte aligned' in lib.dfm_last_error()
    for xp, acc, op, f32 in ((x + 8, None, out, 0), (x, None, out + 8, 0), (x, None, out + 8, 1),
                             (x, res + 8, out, 1)):
        assert lib.dfm_conv3d_k3_c32_fwd_strided(1, 4, 4, 4, xp, 32, w, acc, op, f32, 0, 0, None, None) == -1
        assert b'16-byte aligned' in lib.dfm_last_error()
        assert lib.dfm_conv3d_k3_c32_fwd(1, 4, 4, 4, xp, w, acc, op, f32, 0, 0, None, None) == -1
    assert lib.dfm_conv3d_k3_c32_fwd_slices(1, 4, 4, 4, x + 8, 32, w, out, 64, 0, 0, None) == -1
    assert b'16-byte aligned' in lib.dfm_last_error()
