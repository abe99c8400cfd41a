"""Which launches one forward + backward of each MFMA convolution module makes, in order.

tests/test_conv_variants_exact_gpu.py pins what the modules compute; this file pins HOW: the entry points, the
descriptor of every general-kernel launch, the layout (swap, flip) of every weight pack and the operand order of
every weight-gradient launch.  The expected sequences are written out below as the host code produced them before
its autograd functions were merged into one; a change of ``conv3d.py`` that is meant to keep the launches must
reproduce them.  Consecutive equal records are run-length encoded as (record, count): the six (or three) products of
a split-precision convolution differ in their operands' addresses only.
"""
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')

# kind, cin, cout, size, stride, padding: the rows of test_module_gradients_exact and test_2d_module_gradients_exact
# (tests/test_conv_variants_exact_gpu.py) plus the 3-channel image skip of SPPUNetNeck
CASES_3D = [
    ('conv', 32, 64, (6, 8, 10), 1, 1),
    ('conv', 64, 32, (6, 8, 12), 2, 1),
    ('conv', 64, 64, (5, 7, 9), 2, 1),
    ('conv', 64, 128, (4, 6, 8), (1, 1, 2), 1),
    ('conv', 32, 32, (3, 5, 4), 1, (1, 1, 0)),
    ('convT', 64, 32, (3, 4, 5), 2, 1),
]
CASES_2D = [
    ('conv', 64, 32, (9, 21), 1, 1),
    ('conv', 64, 32, (10, 22), 2, 1),
    ('convT', 64, 32, (5, 11), 2, 1),
    ('conv', 3, 32, (6, 8), 1, 1),
]
CASES = [c + (p,) for c in CASES_3D + CASES_2D for p in ('bf16', 'fp32')]


def case_id(case):
    kind, cin, cout, size, stride, padding, precision = case
    st = 'x'.join(map(str, stride)) if isinstance(stride, tuple) else str(stride)
    pd = 'x'.join(map(str, padding)) if isinstance(padding, tuple) else str(padding)
    return f'{kind}{len(size)}d-{cin}-{cout}-{"x".join(map(str, size))}-s{st}-p{pd}-{precision}'


def _record(name, args):
    if name.startswith('dfm_conv3d_g_fwd'):
        d = args[0]
        return (name, d.cin, d.cout, tuple(d.stride), tuple(d.padding), tuple(d.transposed), tuple(d.kernel1))
    if name.startswith('dfm_conv3d_g_pack_weights'):
        return (name, args[2], args[3], args[4], args[5])
    if name == 'dfm_conv3d_wgrad_to':
        d = args[0]
        return (name, d.a, d.b, tuple(d.stride), tuple(d.padding))
    return (name,)


def _run_lengths(records):
    out = []
    for r in records:
        if out and out[-1][0] == r:
            out[-1] = (r, out[-1][1] + 1)
        else:
            out.append((r, 1))
    return out


def record_case(cv, monkeypatch, case):
    """the run-length encoded launch records of one forward + backward of the case's module"""
    kind, cin, cout, size, stride, padding, precision = case
    two_d = len(size) == 2
    if kind == 'conv':
        cls = cv.MfmaConv2d if two_d else cv.MfmaConv3dG
        m = cls(cin, cout, 3, stride=stride, padding=padding, bias=False)
    else:
        cls = cv.MfmaConvTranspose2d if two_d else cv.MfmaConvTranspose3d
        m = cls(cin, cout, 3, stride=2, padding=1, output_padding=1, bias=False)
    dt = torch.bfloat16 if precision == 'bf16' else torch.float32
    cl = torch.channels_last if two_d else torch.channels_last_3d
    gen = torch.Generator().manual_seed(71)
    m = m.to(DEV, dt)
    m.weight.data = torch.randint(-4, 5, tuple(m.weight.shape), generator=gen).to(DEV, dt)
    x = torch.randint(-4, 5, (2, cin, *size), generator=gen).to(DEV, dt).contiguous(memory_format=cl)
    x.requires_grad_(True)
    records = []
    for attr in ('launch', 'try_launch'):
        def wrapped(name, *args, _inner=getattr(cv, attr), **kw):
            records.append(_record(name, args))
            return _inner(name, *args, **kw)
        monkeypatch.setattr(cv, attr, wrapped)
    y = m(x)
    gy = torch.randint(-4, 5, tuple(y.shape), generator=gen).to(DEV, dt).contiguous(memory_format=cl)
    y.backward(gy)
    torch.cuda.synchronize()
    assert x.grad is not None and x.grad.shape == x.shape and m.weight.grad.shape == m.weight.shape
    return _run_lengths(records)


@pytest.fixture(scope='module')
def cv():
    assert torch.cuda.is_available()
    m = importlib.import_module('depth-from-motion_amd.conv3d')
    prev = m.set_fallback_policy('raise')
    yield m
    m.set_fallback_policy(prev)


EXPECTED = {'conv3d-32-64-6x8x10-s1-p1-bf16': [(('dfm_conv3d_g_pack_weights', 32, 64, 0, 0), 1),
                                    (('dfm_conv3d_g_fwd', 32, 64, (1, 1, 1), (1, 1, 1), (0, 0, 0), (0, 0, 0)), 1),
                                    (('dfm_conv3d_g_pack_weights', 64, 32, 1, 7), 1),
                                    (('dfm_conv3d_g_fwd', 64, 32, (1, 1, 1), (1, 1, 1), (0, 0, 0), (0, 0, 0)), 1),
                                    (('dfm_conv3d_wgrad_to', 64, 32, (1, 1, 1), (1, 1, 1)), 1)],
 'conv3d-32-64-6x8x10-s1-p1-fp32': [(('dfm_conv3d_g_pack_weights', 32, 64, 0, 0), 3),
                                    (('dfm_conv3d_g_fwd_f32', 32, 64, (1, 1, 1), (1, 1, 1), (0, 0, 0), (0, 0, 0)), 6),
                                    (('dfm_conv3d_g_pack_weights', 64, 32, 1, 7), 3),
                                    (('dfm_conv3d_g_fwd_f32', 64, 32, (1, 1, 1), (1, 1, 1), (0, 0, 0), (0, 0, 0)), 6),
                                    (('dfm_conv3d_wgrad_to', 64, 32, (1, 1, 1), (1, 1, 1)), 6)],
 'conv3d-64-32-6x8x12-s2-p1-bf16': [(('dfm_conv3d_g_pack_weights', 64, 32, 0, 0), 1),
                                    (('dfm_conv3d_g_fwd', 64, 32, (2, 2, 2), (1, 1, 1), (0, 0, 0), (0, 0, 0)), 1),
                                    (('dfm_conv3d_g_pack_weights', 32, 64, 1, 0), 1),
                                    (('dfm_conv3d_g_fwd', 32, 64, (1, 1, 1), (1, 1, 1), (1, 1, 1), (0, 0, 0)), 1),
                                    (('dfm_conv3d_wgrad_to', 32, 64, (2, 2, 2), (1, 1, 1)), 1)],
 'conv3d-64-32-6x8x12-s2-p1-fp32': [(('dfm_conv3d_g_pack_weights', 64, 32, 0, 0), 3),
                                    (('dfm_conv3d_g_fwd_f32', 64, 32, (2, 2, 2), (1, 1, 1), (0, 0, 0), (0, 0, 0)), 6),
                                    (('dfm_conv3d_g_pack_weights', 32, 64, 1, 0), 3),
                                    (('dfm_conv3d_g_fwd_f32', 32, 64, (1, 1, 1), (1, 1, 1), (1, 1, 1), (0, 0, 0)), 6),
                                    (('dfm_conv3d_wgrad_to', 32, 64, (2, 2, 2), (1, 1, 1)), 6)],
 'conv3d-64-64-5x7x9-s2-p1-bf16': [(('dfm_conv3d_g_pack_weights', 64, 64, 0, 0), 1),
                                   (('dfm_conv3d_g_fwd', 64, 64, (2, 2, 2), (1, 1, 1), (0, 0, 0), (0, 0, 0)), 1),
                                   (('dfm_conv3d_wgrad_to', 64, 64, (2, 2, 2), (1, 1, 1)), 1)],
 'conv3d-64-64-5x7x9-s2-p1-fp32': [(('dfm_conv3d_g_pack_weights', 64, 64, 0, 0), 3),
                                   (('dfm_conv3d_g_fwd_f32', 64, 64, (2, 2, 2), (1, 1, 1), (0, 0, 0), (0, 0, 0)), 6),
                                   (('dfm_conv3d_wgrad_to', 64, 64, (2, 2, 2), (1, 1, 1)), 6)],
 'conv3d-64-128-4x6x8-s1x1x2-p1-bf16': [(('dfm_conv3d_g_pack_weights', 64, 128, 0, 0), 1),
                                        (('dfm_conv3d_g_fwd', 64, 128, (1, 1, 2), (1, 1, 1), (0, 0, 0), (0, 0, 0)),
                                         1),
                                        (('dfm_conv3d_g_pack_weights', 128, 64, 1, 6), 1),
                                        (('dfm_conv3d_g_fwd', 128, 64, (1, 1, 1), (1, 1, 1), (0, 0, 1), (0, 0, 0)),
                                         1),
                                        (('dfm_conv3d_wgrad_to', 128, 64, (1, 1, 2), (1, 1, 1)), 1)],
 'conv3d-64-128-4x6x8-s1x1x2-p1-fp32': [(('dfm_conv3d_g_pack_weights', 64, 128, 0, 0), 3),
                                        (('dfm_conv3d_g_fwd_f32',
                                          64,
                                          128,
                                          (1, 1, 2),
                                          (1, 1, 1),
                                          (0, 0, 0),
                                          (0, 0, 0)),
                                         6),
                                        (('dfm_conv3d_g_pack_weights', 128, 64, 1, 6), 3),
                                        (('dfm_conv3d_g_fwd_f32',
                                          128,
                                          64,
                                          (1, 1, 1),
                                          (1, 1, 1),
                                          (0, 0, 1),
                                          (0, 0, 0)),
                                         6),
                                        (('dfm_conv3d_wgrad_to', 128, 64, (1, 1, 2), (1, 1, 1)), 6)],
 'conv3d-32-32-3x5x4-s1-p1x1x0-bf16': [(('dfm_conv3d_g_pack_weights', 32, 32, 0, 0), 1),
                                       (('dfm_conv3d_g_fwd', 32, 32, (1, 1, 1), (1, 1, 0), (0, 0, 0), (0, 0, 0)), 1),
                                       (('dfm_conv3d_g_pack_weights', 32, 32, 1, 7), 1),
                                       (('dfm_conv3d_g_fwd', 32, 32, (1, 1, 1), (1, 1, 2), (0, 0, 0), (0, 0, 0)), 1),
                                       (('dfm_conv3d_wgrad_to', 32, 32, (1, 1, 1), (1, 1, 0)), 1)],
 'conv3d-32-32-3x5x4-s1-p1x1x0-fp32': [(('dfm_conv3d_g_pack_weights', 32, 32, 0, 0), 3),
                                       (('dfm_conv3d_g_fwd_f32', 32, 32, (1, 1, 1), (1, 1, 0), (0, 0, 0), (0, 0, 0)),
                                        6),
                                       (('dfm_conv3d_g_pack_weights', 32, 32, 1, 7), 3),
                                       (('dfm_conv3d_g_fwd_f32', 32, 32, (1, 1, 1), (1, 1, 2), (0, 0, 0), (0, 0, 0)),
                                        6),
                                       (('dfm_conv3d_wgrad_to', 32, 32, (1, 1, 1), (1, 1, 0)), 6)],
 'convT3d-64-32-3x4x5-s2-p1-bf16': [(('dfm_conv3d_g_pack_weights', 64, 32, 1, 0), 1),
                                    (('dfm_conv3d_g_fwd', 64, 32, (1, 1, 1), (1, 1, 1), (1, 1, 1), (0, 0, 0)), 1),
                                    (('dfm_conv3d_g_pack_weights', 32, 64, 0, 0), 1),
                                    (('dfm_conv3d_g_fwd', 32, 64, (2, 2, 2), (1, 1, 1), (0, 0, 0), (0, 0, 0)), 1),
                                    (('dfm_conv3d_wgrad_to', 64, 32, (2, 2, 2), (1, 1, 1)), 1)],
 'convT3d-64-32-3x4x5-s2-p1-fp32': [(('dfm_conv3d_g_pack_weights', 64, 32, 1, 0), 3),
                                    (('dfm_conv3d_g_fwd_f32', 64, 32, (1, 1, 1), (1, 1, 1), (1, 1, 1), (0, 0, 0)), 6),
                                    (('dfm_conv3d_g_pack_weights', 32, 64, 0, 0), 3),
                                    (('dfm_conv3d_g_fwd_f32', 32, 64, (2, 2, 2), (1, 1, 1), (0, 0, 0), (0, 0, 0)), 6),
                                    (('dfm_conv3d_wgrad_to', 64, 32, (2, 2, 2), (1, 1, 1)), 6)],
 'conv2d-64-32-9x21-s1-p1-bf16': [(('dfm_conv3d_g_pack_weights_2d', 64, 32, 0, 0), 1),
                                  (('dfm_conv3d_g_fwd', 64, 32, (1, 1, 1), (0, 1, 1), (0, 0, 0), (1, 0, 0)), 1),
                                  (('dfm_conv3d_g_pack_weights_2d', 32, 64, 1, 7), 1),
                                  (('dfm_conv3d_g_fwd', 32, 64, (1, 1, 1), (0, 1, 1), (0, 0, 0), (1, 0, 0)), 1),
                                  (('dfm_conv3d_wgrad_to', 32, 64, (1, 1, 1), (1, 1, 1)), 1)],
 'conv2d-64-32-9x21-s1-p1-fp32': [(('dfm_conv3d_g_pack_weights', 64, 32, 0, 0), 3),
                                  (('dfm_conv3d_g_fwd_f32', 64, 32, (1, 1, 1), (0, 1, 1), (0, 0, 0), (1, 0, 0)), 6),
                                  (('dfm_conv3d_g_pack_weights', 32, 64, 1, 7), 3),
                                  (('dfm_conv3d_g_fwd_f32', 32, 64, (1, 1, 1), (0, 1, 1), (0, 0, 0), (1, 0, 0)), 6),
                                  (('dfm_conv3d_wgrad_to', 32, 64, (1, 1, 1), (1, 1, 1)), 6)],
 'conv2d-64-32-10x22-s2-p1-bf16': [(('dfm_conv3d_g_pack_weights_2d', 64, 32, 0, 0), 1),
                                   (('dfm_conv3d_g_fwd', 64, 32, (1, 2, 2), (0, 1, 1), (0, 0, 0), (1, 0, 0)), 1),
                                   (('dfm_conv3d_g_pack_weights_2d', 32, 64, 1, 4), 1),
                                   (('dfm_conv3d_g_fwd', 32, 64, (1, 1, 1), (0, 1, 1), (0, 1, 1), (1, 0, 0)), 1),
                                   (('dfm_conv3d_wgrad_to', 32, 64, (1, 2, 2), (1, 1, 1)), 1)],
 'conv2d-64-32-10x22-s2-p1-fp32': [(('dfm_conv3d_g_pack_weights', 64, 32, 0, 0), 3),
                                   (('dfm_conv3d_g_fwd_f32', 64, 32, (1, 2, 2), (0, 1, 1), (0, 0, 0), (1, 0, 0)), 6),
                                   (('dfm_conv3d_g_pack_weights', 32, 64, 1, 4), 3),
                                   (('dfm_conv3d_g_fwd_f32', 32, 64, (1, 1, 1), (0, 1, 1), (0, 1, 1), (1, 0, 0)), 6),
                                   (('dfm_conv3d_wgrad_to', 32, 64, (1, 2, 2), (1, 1, 1)), 6)],
 'convT2d-64-32-5x11-s2-p1-bf16': [(('dfm_conv3d_g_pack_weights_2d', 64, 32, 1, 0), 1),
                                   (('dfm_conv3d_g_fwd', 64, 32, (1, 1, 1), (0, 1, 1), (0, 1, 1), (1, 0, 0)), 1),
                                   (('dfm_conv3d_g_pack_weights_2d', 32, 64, 0, 0), 1),
                                   (('dfm_conv3d_g_fwd', 32, 64, (1, 2, 2), (0, 1, 1), (0, 0, 0), (1, 0, 0)), 1),
                                   (('dfm_conv3d_wgrad_to', 64, 32, (1, 2, 2), (1, 1, 1)), 1)],
 'convT2d-64-32-5x11-s2-p1-fp32': [(('dfm_conv3d_g_pack_weights', 64, 32, 1, 0), 3),
                                   (('dfm_conv3d_g_fwd_f32', 64, 32, (1, 1, 1), (0, 1, 1), (0, 1, 1), (1, 0, 0)), 6),
                                   (('dfm_conv3d_g_pack_weights', 32, 64, 0, 0), 3),
                                   (('dfm_conv3d_g_fwd_f32', 32, 64, (1, 2, 2), (0, 1, 1), (0, 0, 0), (1, 0, 0)), 6),
                                   (('dfm_conv3d_wgrad_to', 64, 32, (1, 2, 2), (1, 1, 1)), 6)],
 'conv2d-3-32-6x8-s1-p1-bf16': [(('dfm_conv3d_g_pack_weights_2d', 32, 32, 0, 0), 1),
                                (('dfm_conv3d_g_fwd', 32, 32, (1, 1, 1), (0, 1, 1), (0, 0, 0), (1, 0, 0)), 1),
                                (('dfm_conv3d_g_pack_weights_2d', 32, 32, 1, 7), 1),
                                (('dfm_conv3d_g_fwd', 32, 32, (1, 1, 1), (0, 1, 1), (0, 0, 0), (1, 0, 0)), 1),
                                (('dfm_conv3d_wgrad_to', 32, 32, (1, 1, 1), (1, 1, 1)), 1)],
 'conv2d-3-32-6x8-s1-p1-fp32': [(('dfm_conv3d_g_pack_weights', 32, 32, 0, 0), 3),
                                (('dfm_conv3d_g_fwd_f32', 32, 32, (1, 1, 1), (0, 1, 1), (0, 0, 0), (1, 0, 0)), 6),
                                (('dfm_conv3d_g_pack_weights', 32, 32, 1, 7), 3),
                                (('dfm_conv3d_g_fwd_f32', 32, 32, (1, 1, 1), (0, 1, 1), (0, 0, 0), (1, 0, 0)), 6),
                                (('dfm_conv3d_wgrad_to', 32, 32, (1, 1, 1), (1, 1, 1)), 6)]}


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_launch_trace(cv, monkeypatch, case):
    assert record_case(cv, monkeypatch, case) == EXPECTED[case_id(case)]
