"""GPU: the 3-D anchor head's loss_single (csrc/anchor_loss.hip behind depth-from-motion_amd/anchor_loss.py) against
tests/anchor_loss_ref.py run in fp64 on the same inputs (bf16 maps upcast exactly), and against tests/golden/
anchor_loss.npz (the reference's own loss_single bodies, through the mixin on stub heads).

Bounds (none is taken from the kernels' output):
  out[i]     relative 1e-5: the terms are non-negative, a term is a dozen fp32 roundings plus exp / log1p, a tree sum
             adds 2^-24 log2 N.
  grad_cls   |err| <= 1e-5 |ref| + 1e-30 |g scale|                      (no cancellation in either branch)
  grad_dir   |err| <= 1e-5 |g scale w|
  grad_reg   |err| <= 1e-5 |g scale w| (1 + |p| + |t|) / beta           (p - t cancels: the error scales with the
             operands), plus, with the IoU term, the IoU Jacobian's bound of tests/test_iou3d_loss_gpu.py:
             2 x 4 x fp32_head_grad_error of tests/golden/iou3d.npz per unit of |g scale| (a unit-weight row).  That
             figure was measured on boxes near their anchors; the draws here (deltas ~ N(0, 1) up to 3: boxes up to
             e^3 times the anchor) carry the decode's factors further, so the bound is the larger of it and 4 x the
             error of the fp32 torch stand-in (tests/golden/make_golden_iou3d.py) against its fp64 run on the same
             rows, computed here for each case.
  bf16       the fp32 bound plus 2^-8 |ref| (one round-to-nearest-even of the fp32 result).
Each test prints its figures before it asserts."""
import importlib
import os

import numpy as np
import pytest
import torch

from tests import anchor_loss_ref as ref
from tests import util
from tests.test_anchor_loss import CASES, inputs as golden_inputs, stub_head

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 2, 1), (2, 5, 7, 6, 3), (1, 33, 65, 6, 3), (2, 48, 64, 6, 3)]       # (B, h, w, A, C)
SIZES = torch.tensor([[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]])
GRAD_OUT = (0.3, 1.7, -2.0, 0.5)
SCALE = (1.0 / 37.0, 2.0 / 41.0, 0.2 / 41.0, 1.0 / 41.0)
BETA = 1.0 / 9.0


@pytest.fixture(scope='module')
def pkg():
    importlib.import_module('depth-from-motion_amd.build').build_hip()
    return importlib.import_module('depth-from-motion_amd')


@pytest.fixture(scope='module')
def al():
    return importlib.import_module('depth-from-motion_amd.anchor_loss')


@pytest.fixture(scope='module')
def iou_bar():
    z = np.load(os.path.join(util.GOLDEN, 'iou3d.npz'))
    return 2 * 4 * float(z['fp32_head_grad_error'])


def to_map(rows, B, H, W, dtype, layout):
    """(B * N, width) fp32 rows -> the (B, A * width, H, W) map of ``dtype`` in ``layout``, a leaf that wants a gradient"""
    m = rows.reshape(B, H, W, -1).permute(0, 3, 1, 2).to(dtype)
    if layout == 'nchw':
        m = m.contiguous()
    elif layout == 'cl':
        m = m.contiguous(memory_format=torch.channels_last)
    else:                                                      # a channel and column slice of a wider NCHW tensor
        wide = torch.zeros(B, m.shape[1] + 5, H, W + 3, dtype=dtype, device=m.device)
        wide[:, 3:3 + m.shape[1], :, 1:1 + W] = m
        m = wide[:, 3:3 + m.shape[1], :, 1:1 + W]
        assert m.stride() != m.contiguous().stride()
    return m.detach().requires_grad_(True)


def draw(shape, seed, dtype=torch.float32, layout='nchw', positives='some', S=7, extremes=True):
    """the inputs of one call on the GPU: maps (leaves), dense targets, anchors"""
    B, H, W, A, C = shape
    N = H * W * A
    R = B * N
    g = torch.Generator(device='cuda').manual_seed(seed)
    rand = lambda *s: torch.rand(*s, generator=g, device='cuda')  # noqa: E731
    randn = lambda *s: torch.randn(*s, generator=g, device='cuda')  # noqa: E731
    labels = torch.full((R,), C, dtype=torch.int64, device='cuda')
    if positives == 'some':
        pos = rand(R) < max(0.02, min(1.0, 3.0 / R))
        pos[-1] = True
        odd = torch.tensor([C, -1, C + 5], device='cuda')[torch.randint(0, 3, (R,), generator=g, device='cuda')]
        labels = torch.where(rand(R) < 0.1, odd, labels)
    elif positives == 'all':
        pos = torch.ones(R, dtype=torch.bool, device='cuda')
    elif positives == 'last':
        pos = torch.zeros(R, dtype=torch.bool, device='cuda')
        pos[-1] = True
    else:
        pos = torch.zeros(R, dtype=torch.bool, device='cuda')
    labels = torch.where(pos, torch.randint(0, C, (R,), generator=g, device='cuda'), labels)
    label_weights = (rand(R) > 0.15).float()
    tgt = randn(R, S).clamp(-3, 3)
    noise = torch.where(rand(R, S) < 0.5, (rand(R, S) * 2 - 1) * BETA, randn(R, S))
    pred = torch.where(pos[:, None], tgt + noise, randn(R, S))
    bbox_targets = torch.where(pos[:, None], tgt, torch.zeros_like(tgt))
    bbox_weights = pos[:, None].float().expand(R, S).contiguous()
    dir_targets = torch.where(pos, torch.randint(0, 2, (R,), generator=g, device='cuda'), torch.zeros_like(labels))
    dir_weights = pos.float() * (0.5 + rand(R))
    cls = randn(R, C) * 1.5 - 2.0
    if extremes and R * C >= 8:
        flat = cls.view(-1)
        at = torch.randperm(R * C, generator=g, device='cuda')[:8]
        flat[at] = torch.tensor([80.0, -80.0, 1e4, -1e4, 80.0, -80.0, 1e4, -1e4], device='cuda')
        row = at[4:] // C                                      # four of them on rows that count: target class and not
        if positives in ('some', 'all'):
            labels[row[:2]] = (at[4:6] % C)
        label_weights[row] = 1.0
    dirs = randn(R, 2)
    cls_idx = torch.arange(N, device='cuda') % A % 3
    anchors = torch.cat([rand(N, 2) * 60 - torch.tensor([0.0, 30.0], device='cuda'), rand(N, 1) - 1.8,
                         SIZES.cuda()[cls_idx], (torch.arange(N, device='cuda') % 2)[:, None] * 1.57], 1)
    if S > 7:
        anchors = torch.cat([anchors, torch.zeros(N, S - 7, device='cuda')], 1)
    maps = [to_map(r, B, H, W, dtype, layout) for r in (cls, pred, dirs)]
    return dict(maps=maps, labels=labels.view(B, N), label_weights=label_weights.view(B, N),
                bbox_targets=bbox_targets.view(B, N, S), bbox_weights=bbox_weights.view(B, N, S),
                dir_targets=dir_targets.view(B, N), dir_weights=dir_weights.view(B, N), anchors=anchors, C=C, S=S, A=A)


def targets(d):
    return [d[k] for k in ('labels', 'label_weights', 'bbox_targets', 'bbox_weights', 'dir_targets', 'dir_weights')]


def run_hip(pkg, d, with_dir=True, with_iou=True, grad_out=GRAD_OUT, scale=SCALE, **kw):
    """(out (4,), [grad_cls, grad_reg, grad_dir]) of the package's function; the gradients through grad_out"""
    maps = [m.detach().requires_grad_(True) for m in d['maps']]
    sc = torch.tensor(scale, dtype=torch.float32, device='cuda')
    out = pkg.anchor3d_loss(maps[0], maps[1], maps[2] if with_dir else None, *targets(d),
                            d['anchors'] if with_iou else None, num_classes=d['C'], scale=sc, with_iou=with_iou, **kw)
    assert len(out) == 4 and all(o.dim() == 0 and o.dtype == torch.float32 for o in out)
    wanted = maps if with_dir else maps[:2]
    grads = torch.autograd.grad(out, wanted, [torch.tensor(g, device='cuda') for g in grad_out])
    return torch.stack([o.detach() for o in out]), list(grads)


def run_ref(d, with_dir=True, with_iou=True, grad_out=GRAD_OUT, scale=SCALE, **kw):
    """the same in fp64 from tests/anchor_loss_ref.py"""
    maps = [m.detach().double().requires_grad_(True) for m in d['maps']]
    sums = ref.loss_terms(maps[0], maps[1], maps[2] if with_dir else None, *targets(d),
                          d['anchors'] if with_iou else None, num_classes=d['C'], with_iou=with_iou, **kw)
    out = torch.stack([s * c for s, c in zip(sums, scale)])
    total = sum(o * g for o, g in zip(out, grad_out))
    wanted = maps if with_dir else maps[:2]
    grads = torch.autograd.grad(total, wanted, allow_unused=True)
    return out.detach(), [torch.zeros_like(m) if g is None else g for m, g in zip(wanted, grads)]


def iou_jacobian_bar(d, iou_bar):
    """per unit of |g scale|: the larger of the fixture's figure and 4 x |fp32 stand-in - fp64 stand-in| on these rows"""
    labels = d['labels'].reshape(-1)
    pos = ((labels >= 0) & (labels < d['C'])).nonzero().reshape(-1)
    if not len(pos):
        return iou_bar
    S = d['S']
    a = d['anchors'][pos % d['anchors'].shape[0]][:, :7]
    t = d['bbox_targets'].reshape(-1, S)[pos][:, :7]
    p = ref.rows_of(d['maps'][1].detach().float(), S)[pos][:, :7]
    jac = []
    for dtype in (torch.float64, torch.float32):
        q = p.to(dtype).requires_grad_(True)
        jac.append(torch.autograd.grad(ref.iou_rows(a.to(dtype), q, t.to(dtype)).sum(), q)[0].double())
    return max(iou_bar, 4 * float((jac[0] - jac[1]).abs().max()))


def compare(d, got, want, iou_bar, with_dir=True, with_iou=True, grad_out=GRAD_OUT, scale=SCALE, beta=BETA,
            code_weight=None, what=''):
    """print the figures, then hold out and the three gradients to the bounds of the module docstring"""
    (out, grads), (out64, grads64) = got, want
    bf16 = d['maps'][0].dtype == torch.bfloat16
    C, S = d['C'], d['S']
    rel = ((out.double() - out64).abs() / out64.abs().clamp(min=1e-300)).tolist()
    gs = [abs(g * s) for g, s in zip(grad_out, scale)]
    labels = d['labels'].reshape(-1)
    pos = (labels >= 0) & (labels < C)
    rows = lambda g, width: ref.rows_of(g.detach().double(), width)  # noqa: E731
    extra = lambda r: 2.0 ** -8 * r.abs() if bf16 else 0.0  # noqa: E731
    worst = {}

    def hold(name, g, g64, bound):
        err = (g - g64).abs()
        worst[name] = float((err / bound.clamp(min=1e-300)).max()) if err.numel() else 0.0
        return bool((err <= bound).all())
    g_cls, r_cls = rows(grads[0], C), rows(grads64[0], C)
    ok_cls = hold('cls', g_cls, r_cls, 1e-5 * r_cls.abs() + 1e-30 * gs[0] + extra(r_cls))
    p = rows(d['maps'][1], S)
    t = d['bbox_targets'].reshape(-1, S).double()
    w = d['bbox_weights'].reshape(-1, S).double()
    if code_weight is not None:
        w = w * w.new_tensor(list(code_weight))
    g_reg, r_reg = rows(grads[1], S), rows(grads64[1], S)
    bound = 1e-5 * gs[1] * w.abs() * (1 + p.abs() + t.abs()) / beta + extra(r_reg)
    jac_bar = 0.0
    if with_iou:
        jac_bar = iou_jacobian_bar(d, iou_bar)
        bound[:, :7] += pos[:, None].double() * jac_bar * gs[3]
    ok_reg = hold('reg', g_reg, r_reg, bound)
    ok_dir = True
    if with_dir:
        g_dir, r_dir = rows(grads[2], 2), rows(grads64[2], 2)
        ok_dir = hold('dir', g_dir, r_dir, 1e-5 * gs[2] * d['dir_weights'].reshape(-1, 1).double().abs() + extra(r_dir)
                      + torch.zeros_like(r_dir))
    print(f'{what}: positives {int(pos.sum())} of {len(labels)}, out {out.tolist()}, relative error {rel} (bar 1e-5), '
          f'worst gradient error / bound {worst}, IoU Jacobian bar {jac_bar:.3g}')
    for i in range(4):
        if out64[i] == 0:
            assert out[i] == 0, (i, out.tolist())
        else:
            assert rel[i] <= 1e-5, (i, rel)
    assert ok_cls and ok_reg and ok_dir, worst
    # exact zeros: rows that are not positive in grad_reg and grad_dir, rows without weight in grad_cls
    assert bool((g_reg[~pos] == 0).all()) and (not with_dir or bool((rows(grads[2], 2)[~pos] == 0).all()))
    assert bool((g_cls[d['label_weights'].reshape(-1) == 0] == 0).all())
    for g in grads:
        assert bool(torch.isfinite(g.float()).all())
    assert bool(torch.isfinite(out).all())


@pytest.mark.parametrize('layout', ['nchw', 'cl', 'sliced'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_all_terms_match_fp64(pkg, iou_bar, shape, dtype, layout):
    """every shape x dtype x layout with all four terms: labels of C, -1 and C + 5, zero label weights, logits of
    +-80 and +-1e4, the last row positive"""
    d = draw(shape, seed=sum(shape), dtype=dtype, layout=layout)
    compare(d, run_hip(pkg, d), run_ref(d), iou_bar, what=f'{shape} {dtype} {layout}')


VARIANTS = {
    'no_positive': dict(positives='none'),
    'all_positive': dict(positives='all'),
    'last_row_only': dict(positives='last'),
    'gamma_1.5_alpha_0.4': dict(kw=dict(gamma=1.5, alpha=0.4)),
    'code_weight': dict(kw=dict(code_weight=[1.0, 0.5, 2.0, 1.0, 1.5, 1.0, 0.2])),
    'no_sin_difference': dict(kw=dict(diff_rad_by_sin=False)),
    'no_direction_map': dict(with_dir=False),
    'no_iou': dict(with_iou=False),
    'code_9_no_iou': dict(with_iou=False, S=9, kw=dict(code_weight=[1.0] * 7 + [0.2, 0.2])),
    'code_16_no_iou_no_dir': dict(with_iou=False, with_dir=False, S=16),
}


@pytest.mark.parametrize('config', [(torch.float32, 'nchw'), (torch.bfloat16, 'cl')], ids=['fp32-nchw', 'bf16-cl'])
@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('shape', SHAPES[1:3], ids=lambda s: 'x'.join(map(str, s)))
def test_variants_match_fp64(pkg, iou_bar, shape, variant, config):
    v = VARIANTS[variant]
    with_dir, with_iou, kw = v.get('with_dir', True), v.get('with_iou', True), v.get('kw', {})
    d = draw(shape, seed=11 + len(variant), dtype=config[0], layout=config[1], positives=v.get('positives', 'some'),
             S=v.get('S', 7))
    got = run_hip(pkg, d, with_dir, with_iou, **kw)
    compare(d, got, run_ref(d, with_dir, with_iou, **kw), iou_bar, with_dir, with_iou,
            code_weight=kw.get('code_weight'), what=f'{shape} {variant} {config}')
    if v.get('positives') == 'none':
        assert bool((got[0][1:] == 0).all()) and all(not bool(g.float().abs().sum()) for g in got[1][1:])
    if not with_dir:
        assert got[0][2] == 0
    if not with_iou:
        assert got[0][3] == 0


def test_each_term_reaches_its_gradient_and_maps_may_be_skipped(pkg, iou_bar):
    """grad_out one-hot per term: the class term reaches grad_cls only, the box and IoU terms grad_reg only, the
    direction term grad_dir only; a map that wants no gradient gets none and the others are the same bits"""
    d = draw(SHAPES[1], seed=5)
    full = run_hip(pkg, d)
    for i, live in enumerate((0, 1, 2, 1)):
        one = tuple(1.0 if k == i else 0.0 for k in range(4))
        _, grads = run_hip(pkg, d, grad_out=one)
        for k, g in enumerate(grads):
            assert bool(g.abs().sum() > 0) == (k == live), (i, k)
        compare(d, run_hip(pkg, d, grad_out=one), run_ref(d, grad_out=one), iou_bar, grad_out=one, what=f'term {i}')
    sc = torch.tensor(SCALE, dtype=torch.float32, device='cuda')
    for wanted in ((0,), (1,), (2,), (0, 2)):
        maps = [m.detach().requires_grad_(k in wanted) for k, m in enumerate(d['maps'])]
        out = pkg.anchor3d_loss(*maps, *targets(d), d['anchors'], num_classes=d['C'], scale=sc, with_iou=True)
        grads = torch.autograd.grad(out, [maps[k] for k in wanted], [torch.tensor(g, device='cuda') for g in GRAD_OUT])
        for k, g in zip(wanted, grads):
            assert torch.equal(g, full[1][k])


def test_two_runs_give_the_same_bits(pkg):
    d = draw(SHAPES[3], seed=3, dtype=torch.bfloat16, layout='cl')
    a, b = run_hip(pkg, d), run_hip(pkg, d)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    d = draw(SHAPES[2], seed=4)
    a, b = run_hip(pkg, d), run_hip(pkg, d)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_every_gradient_element_is_written_once_over_nan(pkg, al, dtype):
    """the C entry on buffers filled with NaN (strides of their own: the class gradient channels-last for an NCHW
    map): no NaN comes back, and the values are those of the autograd path"""
    _launch = importlib.import_module('depth-from-motion_amd._launch')
    d = draw(SHAPES[2], seed=8, dtype=dtype)
    _, want = run_hip(pkg, d)
    cls, reg, dirs = (m.detach() for m in d['maps'])
    desc = al._desc(cls, reg, dirs, d['C'], 7, 2.0, 0.25, BETA, None, True, True)
    bufs = [torch.full_like(cls, float('nan'), memory_format=torch.channels_last), torch.full_like(reg, float('nan')),
            torch.full_like(dirs, float('nan'))]
    for field, t in zip((desc.grad_cls_stride, desc.grad_reg_stride, desc.grad_dir_stride), bufs):
        field[:] = t.stride()
    sc = torch.tensor(SCALE, dtype=torch.float32, device='cuda')
    go = torch.tensor(GRAD_OUT, dtype=torch.float32, device='cuda')
    _launch.launch('dfm_anchor3d_loss_bwd', desc, cls, reg, dirs, *targets(d), d['anchors'], sc, go, *bufs,
                   _launch.STREAM)
    for got, ref_ in zip(bufs, want):
        assert not bool(torch.isnan(got.float()).any())
        assert torch.equal(got, ref_)
    # a NULL gradient pointer skips that map: the other buffers are written, this one is left alone
    bufs[1].fill_(float('nan'))
    bufs[0].fill_(float('nan'))
    _launch.launch('dfm_anchor3d_loss_bwd', desc, cls, reg, dirs, *targets(d), d['anchors'], sc, go, bufs[0], None,
                   bufs[2], _launch.STREAM)
    assert torch.equal(bufs[0], want[0]) and bool(torch.isnan(bufs[1].float()).all())


def test_iou_term_is_the_sum_of_iou3d_loss_from_deltas(pkg):
    d = draw(SHAPES[2], seed=9)
    sc = torch.tensor([1.0, 1.0, 1.0, 1.0], device='cuda')
    with torch.no_grad():
        out = pkg.anchor3d_loss(*d['maps'], *targets(d), d['anchors'], num_classes=d['C'], scale=sc, with_iou=True)
    labels = d['labels'].reshape(-1)
    pos = ((labels >= 0) & (labels < d['C'])).nonzero().reshape(-1)
    assert len(pos) > 64
    n = d['anchors'].shape[0]
    rows = pkg.iou3d_loss_from_deltas(d['anchors'].repeat(labels.numel() // n, 1), ref.rows_of(d['maps'][1].detach(), 7),
                                      d['bbox_targets'].reshape(-1, 7), pos)
    want = float(rows.double().sum())
    print('S_iou', float(out[3]), 'sum of iou3d_loss_from_deltas in fp64', want)
    assert 0 < want < len(pos) and abs(float(out[3]) - want) <= 1e-5 * want


def test_launch_counts_do_not_depend_on_the_size_and_nothing_waits(pkg, al):
    counts = []
    for shape in (SHAPES[1], SHAPES[3]):
        d = draw(shape, seed=2, dtype=torch.bfloat16, layout='cl')
        sc = torch.tensor(SCALE, dtype=torch.float32, device='cuda')
        go = [torch.tensor(g, device='cuda') for g in GRAD_OUT]
        torch.cuda.synchronize()
        al.counters(reset=True)
        torch.cuda.set_sync_debug_mode('error')
        try:
            out = pkg.anchor3d_loss(*d['maps'], *targets(d), d['anchors'], num_classes=d['C'], scale=sc, with_iou=True)
        finally:
            torch.cuda.set_sync_debug_mode('default')
        assert al.counters() == {'kernel_launches': 2, 'memsets': 0, 'host_waits': 0}
        torch.autograd.grad(out, d['maps'], go)
        counts.append(al.counters(reset=True))
    assert counts[0] == counts[1] == {'kernel_launches': 3, 'memsets': 0, 'host_waits': 0}


def test_empty_input_gives_zeros_and_launches_nothing(pkg, al):
    sc = torch.ones(4, device='cuda')
    for B, H in ((0, 3), (2, 0)):
        maps = [torch.zeros(B, c, H, 4, device='cuda', requires_grad=True) for c in (18, 42, 12)]
        dense = [torch.zeros(B, H * 24, dtype=torch.int64, device='cuda'), torch.zeros(B, H * 24, device='cuda'),
                 torch.zeros(B, H * 24, 7, device='cuda'), torch.zeros(B, H * 24, 7, device='cuda'),
                 torch.zeros(B, H * 24, dtype=torch.int64, device='cuda'), torch.zeros(B, H * 24, device='cuda')]
        al.counters(reset=True)
        out = pkg.anchor3d_loss(*maps, *dense, torch.zeros(H * 24, 7, device='cuda'), num_classes=3, scale=sc,
                                with_iou=True)
        assert all(float(o.detach()) == 0 for o in out)
        grads = torch.autograd.grad(out, maps, [torch.ones((), device='cuda')] * 4)
        assert all(g.shape == m.shape for g, m in zip(grads, maps))
        assert al.counters() == {'kernel_launches': 0, 'memsets': 1, 'host_waits': 0}


@pytest.mark.parametrize('case', CASES)
def test_mixin_matches_the_reference_heads(pkg, iou_bar, case):
    """HipAnchor3DLossMixin.loss_single on stub heads set up as the fixture's: the reference's tuple and the gradients
    of sum_i grad_out[i] * loss_i, the fixture's anchors given per image as the head passes them"""
    z = np.load(os.path.join(util.GOLDEN, 'anchor_loss.npz'))
    head, nts = stub_head(pkg, z, case)
    args = [t.cuda() for t in golden_inputs(z, z['nopos/labels'] if case == 'nopos' else None)]
    maps = [m.requires_grad_(True) for m in args[:3]]
    with_dir, with_iou = head.use_direction_classifier, head.loss_iou is not None
    anchors = args[9][None].expand(2, -1, -1)
    losses = head.loss_single(maps[0], maps[1], maps[2] if with_dir else None, *args[3:9], anchors, nts)
    want = z[f'{case}/out']
    assert len(losses) == (4 if with_iou else 3) and (losses[2] is None) == (not with_dir)
    grad_out = z['grad_out'].tolist()
    live = [(v, g) for v, g in zip(losses, grad_out) if v is not None]
    wanted = maps if with_dir else maps[:2]
    grads = torch.autograd.grad([v for v, _ in live], wanted, [torch.tensor(g, device='cuda', dtype=torch.float32)
                                                               for _, g in live])
    out = torch.stack([torch.zeros((), device='cuda') if v is None else v.detach() for v in losses] +
                      ([] if with_iou else [torch.zeros((), device='cuda')]))
    out64 = torch.from_numpy(np.nan_to_num(want, nan=0.0)).cuda()
    grads64 = [torch.from_numpy(z[f'{case}/{k}']).cuda().double()
               for k in ('grad_cls', 'grad_reg', 'grad_dir')[:len(wanted)]]
    scale = head._loss_single_scale(nts, 2, torch.device('cpu')).tolist()
    d = dict(maps=maps, labels=args[3], label_weights=args[4], bbox_targets=args[5], bbox_weights=args[6],
             dir_targets=args[7], dir_weights=args[8], anchors=args[9], C=3, S=7, A=6)
    compare(d, (out, list(grads)), (out64, grads64), iou_bar, with_dir, with_iou, grad_out=grad_out,
            scale=scale, code_weight=head.train_cfg['code_weight'], what=case)


@pytest.mark.parametrize('case', ['plain', 'liga', 'liga_reduce_iou'])
def test_a_device_average_factor_gives_the_same_scale_without_a_wait(pkg, case):
    """num_total_samples as a device scalar (an all-reduced count): the factors are formed on the device"""
    z = np.load(os.path.join(util.GOLDEN, 'anchor_loss.npz'))
    head, nts = stub_head(pkg, z, case)
    host = head._loss_single_scale(nts, 2, torch.device('cuda'))
    count = torch.tensor(float(nts), device='cuda')
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        on_device = head._loss_single_scale(count, 2, torch.device('cuda'))
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert on_device.is_cuda and on_device.dtype == torch.float32 and on_device.shape == (4,)
    assert torch.allclose(on_device, host, rtol=3e-7, atol=0), (on_device.tolist(), host.tolist())
