"""GPU: the differentiable rotated IoU and IOU3DLoss (csrc/iou3d_loss.hip behind depth-from-motion_amd/
iou3d_loss.py) against tests/golden/iou3d.npz -- the reference's own iou3d_loss / IOU3DLoss / DeltaXYZWLHRBBoxCoder.
decode over an fp64 torch stand-in for mmcv's diff_iou_rotated_3d (tests/golden/make_golden_iou3d.py).

Bars, all read from the fixture where they are used.  The generator runs its stand-in in fp64 (the expected values)
and in fp32 on the CPU and stores the largest difference over every pair of every scene:
  IoU of pairs      within 4 x fp32_iou_error  (2.8e-7 -> 1.13e-6)
  gradient of pairs within 4 x fp32_grad_error (6.3e-6 -> 2.5e-5), absolute
  per-row loss / bbox_pred gradient from deltas within 4 x fp32_head_loss_error (7.0e-6 -> 2.8e-5) /
                    4 x fp32_head_grad_error (1.24e-4 -> 5.0e-4): there fp32 also rounds the decoded centres
                    (3.8e-6 m at 60 m) and the gradient carries the decode's factors (the anchor diagonal, 4.2 m)
The factor 4 covers an operation order and device sinf / cosf / expf that differ from the CPU run.  A reduced loss
is a mean of P such terms (or their sum for 'sum': the bar is scaled by the sum of the weights); loss_weight scales
value and bar alike."""
import importlib
import os

import numpy as np
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu
CASES = ('p257', 'p1', 'p0', 'nan')


@pytest.fixture(scope='module')
def pkg():
    importlib.import_module('depth-from-motion_amd.build').build_hip()
    return importlib.import_module('depth-from-motion_amd')


@pytest.fixture(scope='module')
def z():
    return np.load(os.path.join(util.GOLDEN, 'iou3d.npz'))


def dev(x, dtype=None):
    t = torch.from_numpy(np.asarray(x)).cuda()
    return t if dtype is None else t.to(dtype)


def err(got, want):
    want = torch.from_numpy(np.asarray(want)).reshape(got.shape)
    return float((got.detach().double().cpu() - want).abs().max()) if got.numel() else 0.0


def run_pairs(pkg, b1, b2):
    """(iou, grad1, grad2) of one (1, N, 7) call; the gradient rows through backward with unit weights"""
    p = dev(b1)[None].requires_grad_(True)
    q = dev(b2)[None].requires_grad_(True)
    iou = pkg.diff_iou_rotated_3d(p, q)
    iou.sum().backward()
    return iou[0], p.grad[0], q.grad[0]


@pytest.mark.parametrize('scene', ['general', 'aligned'])
def test_values_and_gradients_match_fp64(pkg, z, scene):
    iou, g1, g2 = run_pairs(pkg, z[f'{scene}/boxes1'], z[f'{scene}/boxes2'])
    assert iou.dtype == torch.float32 and g1.dtype == torch.float32
    e_iou, e1, e2 = err(iou, z[f'{scene}/iou']), err(g1, z[f'{scene}/grad1']), err(g2, z[f'{scene}/grad2'])
    b_iou, b_grad = 4 * float(z['fp32_iou_error']), 4 * float(z['fp32_grad_error'])
    print(f'{scene}: max |gpu - fp64| IoU {e_iou:.3g} (bar {b_iou:.3g}), grad1 {e1:.3g}, grad2 {e2:.3g} (bar {b_grad:.3g})')
    assert e_iou <= b_iou
    assert e1 <= b_grad and e2 <= b_grad
    assert float(g1.abs().max()) > 1.0                          # the gradients are not trivially small
    # translation invariance, at the bar of two components
    assert float((g1[:, :3] + g2[:, :3]).abs().max()) <= 2 * b_grad


def test_special_pairs(pkg, z):
    iou, g1, g2 = run_pairs(pkg, z['special/boxes1'], z['special/boxes2'])
    want = z['special/iou']
    e = err(iou, want)
    print('special: max |gpu - fp64| IoU', e, 'bar', 4 * float(z['fp32_iou_error']), 'values', iou.tolist())
    assert e <= 4 * float(z['fp32_iou_error'])
    for t in (iou, g1, g2):
        assert bool(torch.isfinite(t).all())
    zero = torch.from_numpy(want == 0).cuda()
    assert int(zero.sum()) >= 8
    assert bool((iou[zero] == 0).all())                         # exactly 0 ...
    assert bool((g1[zero] == 0).all()) and bool((g2[zero] == 0).all())   # ... with exactly zero gradients


@pytest.mark.parametrize('n', [1, 63, 64, 65, 257])
def test_pair_counts_cover_lane_and_block_edges(pkg, z, n):
    b1, b2 = z['general/boxes1'][5:5 + n], z['general/boxes2'][5:5 + n]
    iou, g1, g2 = run_pairs(pkg, b1, b2)
    full = run_pairs(pkg, z['general/boxes1'], z['general/boxes2'])
    assert iou.shape == (n,) and g1.shape == (n, 7)
    # a pair's result does not depend on where in the launch it sits
    assert torch.equal(iou, full[0][5:5 + n]) and torch.equal(g1, full[1][5:5 + n]) and torch.equal(g2, full[2][5:5 + n])


def test_batched_shape_and_no_grad_path(pkg, z):
    b1 = dev(z['general/boxes1'][:66]).view(2, 33, 7)
    b2 = dev(z['general/boxes2'][:66]).view(2, 33, 7)
    iou = pkg.diff_iou_rotated_3d(b1, b2)                        # nothing requires a gradient: values only
    assert iou.shape == (2, 33) and not iou.requires_grad
    flat = run_pairs(pkg, z['general/boxes1'][:66], z['general/boxes2'][:66])
    assert torch.equal(iou.view(-1), flat[0])
    # a gradient to one input only
    p = b1.clone().requires_grad_(True)
    (pkg.diff_iou_rotated_3d(p, b2) * 2).sum().backward()
    assert torch.equal(p.grad.view(-1, 7), 2 * flat[1])
    assert pkg.diff_iou_rotated_3d(b1[:, :0], b2[:, :0]).shape == (2, 0)
    with pytest.raises(ValueError):
        pkg.diff_iou_rotated_3d(b1, b2[:, :5])


def test_2d_variant_equals_3d_with_unit_height(pkg, z):
    n = 200
    b1, b2 = z['general/boxes1'][:n].copy(), z['general/boxes2'][:n].copy()
    b1[:, 2] = b2[:, 2] = 0
    b1[:, 5] = b2[:, 5] = 1
    iou3, g31, g32 = run_pairs(pkg, b1, b2)
    cols = [0, 1, 3, 4, 6]
    p = dev(b1[:, cols])[None].requires_grad_(True)
    q = dev(b2[:, cols])[None].requires_grad_(True)
    iou2 = pkg.diff_iou_rotated_2d(p, q)
    iou2.sum().backward()
    assert iou2.shape == (1, n)
    assert torch.equal(iou2[0], iou3)
    assert torch.equal(p.grad[0], g31[:, cols]) and torch.equal(q.grad[0], g32[:, cols])
    assert int((iou3 > 0).sum()) > 100


def test_bf16_and_non_contiguous_inputs_are_converted(pkg, z):
    b1, b2 = dev(z['general/boxes1'][:100]), dev(z['general/boxes2'][:100])
    # bf16 in: the kernel sees the bf16 values exactly; the gradient comes back in bf16
    h1 = b1.to(torch.bfloat16)[None].requires_grad_(True)
    h2 = b2.to(torch.bfloat16)[None]
    iou = pkg.diff_iou_rotated_3d(h1, h2)
    iou.sum().backward()
    ref = run_pairs(pkg, h1.detach()[0].float().cpu().numpy(), h2[0].float().cpu().numpy())
    assert iou.dtype == torch.float32 and h1.grad.dtype == torch.bfloat16
    assert torch.equal(iou[0], ref[0]) and torch.equal(h1.grad[0], ref[1].to(torch.bfloat16))
    # fp64 in, gradient in fp64
    d1 = b1.double()[None].requires_grad_(True)
    pkg.diff_iou_rotated_3d(d1, b2.double()[None]).sum().backward()
    assert d1.grad.dtype == torch.float64
    # non-contiguous
    wide = torch.zeros(1, 100, 14, device='cuda')
    wide[0, :, ::2] = b1
    view = wide[:, :, ::2]
    assert not view.is_contiguous()
    want = run_pairs(pkg, z['general/boxes1'][:100], z['general/boxes2'][:100])[0]
    assert torch.equal(pkg.diff_iou_rotated_3d(view, b2[None])[0], want)


def test_two_runs_are_bit_identical(pkg, z):
    a = run_pairs(pkg, z['general/boxes1'], z['general/boxes2'])
    b = run_pairs(pkg, z['general/boxes1'], z['general/boxes2'])
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    h = [head_from_deltas(pkg, z, 'nan') for _ in range(2)]
    assert torch.equal(h[0][0], h[1][0]) and torch.equal(h[0][1], h[1][1])


# ---------------------------------------------------------------------------------------------------------
# IOU3DLoss on decoded boxes
# ---------------------------------------------------------------------------------------------------------
def module_inputs(z, case):
    p = dev(z[f'head/{case}/pred_boxes']).requires_grad_(True)
    t = dev(z[f'head/{case}/target_boxes']).requires_grad_(True)
    return p, t, dev(z['head/module_weight'])


@pytest.mark.parametrize('case', ['p257', 'nan'])
def test_iou3d_loss_module_reductions(pkg, z, case):
    bar = 4 * float(z['fp32_iou_error'])
    p, t, w = module_inputs(z, case)
    P, wsum = p.shape[0], float(w.sum())
    tag = f'head/{case}/module'
    build = importlib.import_module('depth-from-motion_amd.registry').build
    for red, scale, wscale in (('none', 1.0, 1.5), ('mean', 1.0, 1.5), ('sum', P, wsum)):
        loss_fn = build(dict(type='IOU3DLoss', reduction=red))
        got, got_w = loss_fn(p, t), loss_fn(p, t, weight=w)
        assert got.shape == z[f'{tag}/{red}'].shape              # (1, P) for 'none', as the reference
        e, ew = err(got, z[f'{tag}/{red}']), err(got_w, z[f'{tag}/{red}_weight'])
        print(f'{case} {red}: |gpu - fp64| {e:.3g} (bar {bar * scale:.3g}), weighted {ew:.3g} (bar {bar * wscale:.3g})')
        assert e <= bar * scale and ew <= bar * wscale           # weights are below 1.5
    mod = pkg.IOU3DLoss()
    assert err(mod(p, t, weight=w, avg_factor=37.5), z[f'{tag}/mean_avg_float']) <= bar * wsum / 37.5
    assert err(mod(p, t, avg_factor=37.5, reduction_override='none'), z[f'{tag}/none_avg_float']) <= bar
    with pytest.raises(ValueError):
        pkg.IOU3DLoss(reduction='sum')(p, t, avg_factor=37.5)
    # loss_weight 2, weight, a device-tensor avg_factor: value and both gradients
    loss = pkg.IOU3DLoss(loss_weight=2.0)(p, t, weight=w, avg_factor=torch.tensor(37.5, device='cuda'))
    assert err(loss, z[f'{tag}/w2_mean_avg_tensor']) <= 2 * bar * wsum / 37.5
    loss.backward()
    # per row: loss_weight x weight / avg_factor; a replaced (NaN) component receives the sum of two gradient entries
    gbar = 4 * float(z['fp32_grad_error']) * 2 * 1.5 / 37.5 * (2 if case == 'nan' else 1)
    ep, et = err(p.grad, z[f'{tag}/w2_mean_avg_tensor_grad_pred']), err(t.grad, z[f'{tag}/w2_mean_avg_tensor_grad_target'])
    print(f'{case}: gradient |gpu - fp64| pred {ep:.3g}, target {et:.3g} (bar {gbar:.3g})')
    assert ep <= gbar and et <= gbar
    if case == 'nan':                                            # a replaced component: all of it goes to pred
        nan = torch.isnan(t.detach())
        assert int(nan.sum()) > 100 and bool((t.grad[nan] == 0).all())
        assert float(p.grad[nan].abs().max()) > 0


def test_iou3d_loss_without_positives(pkg):
    p = torch.zeros(0, 7, device='cuda', requires_grad=True)
    t = torch.zeros(0, 7, device='cuda')
    none = pkg.iou3d_loss(p, t, reduction='none')
    assert none.shape == (0,)
    loss = pkg.IOU3DLoss()(p, t, avg_factor=torch.tensor(10.0, device='cuda'))
    assert float(loss.detach()) == 0.0
    loss.backward()
    assert p.grad.shape == (0, 7)
    assert float(pkg.iou3d_loss(p, t, reduction='sum')) == 0.0


# ---------------------------------------------------------------------------------------------------------
# the fused head entry
# ---------------------------------------------------------------------------------------------------------
def head_from_deltas(pkg, z, case, dtype=torch.float32, pad=0):
    """(per-row loss, gradient of (row_weights . loss) with respect to bbox_pred)"""
    def widen(x):
        x = dev(x, dtype)
        return torch.cat([x, torch.full((x.shape[0], pad), 3.0, device='cuda', dtype=dtype)], 1) if pad else x
    anchors, targets = widen(z['head/anchors']), widen(z[f'head/{case}/bbox_targets'])
    pred = widen(z['head/bbox_pred']).requires_grad_(True)
    pos = dev(z[f'head/{case}/pos_inds'])
    loss = pkg.iou3d_loss_from_deltas(anchors, pred, targets, pos)
    (loss * dev(z['head/row_weights'])[:len(pos)]).sum().backward()
    return loss.detach(), pred.grad


@pytest.mark.parametrize('case', CASES)
def test_from_deltas_matches_the_reference_pipeline(pkg, z, case):
    lbar, gbar = 4 * float(z['fp32_head_loss_error']), 4 * float(z['fp32_head_grad_error'])
    rows, grad = head_from_deltas(pkg, z, case)
    pos = z[f'head/{case}/pos_inds']
    assert rows.shape == (len(pos),) and rows.dtype == torch.float32 and grad.shape == z['head/bbox_pred'].shape
    e_rows = err(rows, z[f'head/{case}/loss_rows'])
    e_grad = err(grad, z[f'head/{case}/grad_rows'])
    print(f'{case}: P = {len(pos)}, |gpu - fp64| per-row loss {e_rows:.3g} (bar {lbar:.3g}), bbox_pred gradient '
          f'{e_grad:.3g} (bar {gbar:.3g})')
    assert e_rows <= lbar
    assert e_grad <= gbar                                       # the quantity the generator measured: weights in
    # rows outside pos_inds: exactly zero
    rest = np.setdiff1d(np.arange(grad.shape[0]), pos)
    assert bool((grad[torch.from_numpy(rest).cuda()] == 0).all())
    # the reduced loss with a tensor avg_factor, as loss_single forms it, and its gradient.  fp32_head_grad_error
    # was measured with row weights of at least 0.5, so a unit-weight row is within 2 x the figure
    pred = dev(z['head/bbox_pred']).requires_grad_(True)
    per_row = pkg.iou3d_loss_from_deltas(dev(z['head/anchors']), pred, dev(z[f'head/{case}/bbox_targets']), dev(pos))
    avg = torch.tensor(float(z[f'head/{case}/avg_factor']), device='cuda')
    reduced = per_row.sum() / avg
    reduced.backward()
    assert err(reduced, z[f'head/{case}/loss_reduced']) <= lbar * max(len(pos), 1) / float(avg)
    assert err(pred.grad, z[f'head/{case}/grad_reduced']) <= 2 * gbar / float(avg)
    if len(pos):
        # the unfused composition of this package's own ops on the fixture's decoded fp32 boxes: each side is
        # within its bar of the fp64 pipeline
        p, t = dev(z[f'head/{case}/pred_boxes']), dev(z[f'head/{case}/target_boxes'])
        unfused = pkg.iou3d_loss(p, t, reduction='none').reshape(-1)
        assert float((unfused - per_row.detach()).abs().max()) <= 2 * lbar
        w = dev(z['head/row_weights'])[:len(pos)]
        weighted = pkg.iou3d_loss_from_deltas(dev(z['head/anchors']), dev(z['head/bbox_pred']),
                                              dev(z[f'head/{case}/bbox_targets']), dev(pos), bbox_weights=w)
        assert torch.equal(weighted, rows * w)


def test_from_deltas_input_forms(pkg, z):
    base = head_from_deltas(pkg, z, 'p257')
    wide = head_from_deltas(pkg, z, 'p257', pad=2)              # S = 9: the columns beyond 7 are ignored
    assert torch.equal(wide[0], base[0]) and torch.equal(wide[1][:, :7], base[1])
    assert bool((wide[1][:, 7:] == 0).all())
    d = head_from_deltas(pkg, z, 'p257', dtype=torch.float64)   # fp32-representable values: the same launch
    assert d[1].dtype == torch.float64 and torch.equal(d[0].float(), base[0]) and torch.equal(d[1].float(), base[1])
    h = head_from_deltas(pkg, z, 'p1', dtype=torch.bfloat16)
    assert h[1].dtype == torch.bfloat16 and bool(torch.isfinite(h[1].float()).all())
    # no gradient wanted: values only, the same values
    with torch.no_grad():
        rows = pkg.iou3d_loss_from_deltas(dev(z['head/anchors']), dev(z['head/bbox_pred']),
                                          dev(z['head/p257/bbox_targets']), dev(z['head/p257/pos_inds']))
    assert torch.equal(rows, base[0]) and not rows.requires_grad
